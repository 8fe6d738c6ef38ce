"""GPU parity of the tuner bank (sdrhip_tuner_bank_*): every channel of one capture as complex baseband rows, one launch of the tuner's
fused tile kernel with a channel axis.  Row j is held to the restated Pipe on the stream mixed with table j (tests/tuner_model.py) --
independent of the product -- and to the definition: a hip.Tuner of the same arguments on the same launches.  Every comparison is bit
for bit, every output buffer starts as NaN canaries, and the floats between the rows are the canaries still afterwards.  Stream,
cuts and tables are those of tests/test_gpu_tuner.py (tests/tuner_bank_cases.py): 5 blocks of 8192 u8 samples, 5105 outputs, ten tiles
of 512, the last ragged."""
import threading

import numpy as np
import pytest

import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, CUTS, K_ALL = BC.B, BC.CUTS, BC.K_ALL
launch_route = T.launch_route                  # Cross outputs in the tile kernel / tile kernel + fix-up launch


def run_bank(bank, d_in, n_out, seam, cuts, u8, stride=None, k0=0, in_base=0, stream=None):
    """Outputs [k0, k0 + n_out) of every channel as launches cut at k0 + cuts -> rows [channels, 2 n_out].  The buffer is canaries
    before the first launch; the floats of every row beyond its outputs must be canaries after the last."""
    nch = bank.channels
    stride = 2 * n_out if stride is None else stride
    out = dev_empty_f32(nch * stride)
    edges = [0] + [c for c in cuts if c < n_out] + [n_out]
    for a, b in zip(edges[:-1], edges[1:]):
        (bank.run_u8 if u8 else bank.run)(ptr(d_in), in_base, ptr(out) + 8 * a, stride, k0 + a, k0 + b, seam, stream)
    whole = to_host(out).reshape(nch, stride)                 # (checks the guard bands around the buffer)
    gaps = whole.view(np.uint32)[:, 2 * n_out:]
    assert (gaps == CANARY).all(), f"{int((gaps != CANARY).sum())} floats between the rows were written"
    return whole[:, :2 * n_out]


def inputs(oracle, u8=None):
    u8 = T.stream_u8() if u8 is None else u8
    return ((True, to_dev(u8)), (False, to_dev(oracle.convert_u8(u8))))


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
@pytest.mark.parametrize("nch", [1, 3, 32])
def test_banked_launch_against_the_model(hip, oracle, nch, seam, launch_route):
    tables = BC.bank_tables(nch)
    exp = [BC.expected(oracle, t, seam) for t in tables]
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    assert bank.channels == nch and [bank.period(j) for j in range(nch)] == [t.size // 2 for t in tables]
    assert (bank.factor, bank.num_coeffs) == (8, 128)
    bank.set_route(bank.ROUTE_BANKED)
    for is_u8, d_in in inputs(oracle):
        what = f"{nch} channels, seam {seam}, {'u8' if is_u8 else 'cfloat'}"
        for cuts, n_out, name in (([], K_ALL, "one launch"), (CUTS, K_ALL, "cut into launches"), ([], 4097, "one output into the ninth tile"),
                                  ([], 4608, "whole tiles")):
            b0, f0 = hip.tuner_bank_launches(), hip.tuner_fused_launches()
            rows = run_bank(bank, d_in, n_out, seam, cuts, is_u8)
            assert hip.tuner_bank_launches() - b0 == len(cuts) + 1, what + f", {name}: one banked launch per launch"
            assert hip.tuner_fused_launches() == f0, what + f", {name}: a banked run launched a tuner's own kernel"
            for j in range(nch):
                assert_bit_equal(rows[j], exp[j][:2 * n_out], what + f", {name}: channel {j} (period {bank.period(j)})")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
def test_against_the_definition(hip, oracle, seam, launch_route):
    """Every row equals a hip.Tuner of the same arguments on the same launches, on the banked route and channel by channel."""
    tables = BC.bank_tables(3) + [T.osc_table(5), T.osc_table(65536)]
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    for is_u8, d_in in inputs(oracle):
        ref = [T.run_ranges(hip.Tuner(8, S.taps_decim127(), t), d_in, K_ALL, seam, CUTS, is_u8) for t in tables]
        for route in (bank.ROUTE_BANKED, bank.ROUTE_CHANNELS):
            bank.set_route(route)
            b0 = hip.tuner_bank_launches()
            rows = run_bank(bank, d_in, K_ALL, seam, CUTS, is_u8)
            assert hip.tuner_bank_launches() - b0 == ((len(CUTS) + 1) if route == bank.ROUTE_BANKED else 0), f"route {route}"
            for j in range(len(tables)):
                assert_bit_equal(rows[j], ref[j], f"route {route}, seam {seam}, {'u8' if is_u8 else 'cfloat'}: channel {j} vs its tuner")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 2, 6])
def test_row_stride(hip, oracle, extra, launch_route):
    """32 rows 2 n, 2 n + 2 and 2 n + 6 floats apart, n = 5105: 2 n = 2 (mod 4), so with no gap every odd row is only 8-byte aligned and
    with the gaps every row is 16-byte aligned until a cut at an odd output (1, 1009) moves all of them."""
    tables = BC.bank_tables(32)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    stride = 2 * K_ALL + extra
    assert (stride % 4 == 2) == (extra == 0)
    for route in (bank.ROUTE_BANKED, bank.ROUTE_CHANNELS):
        bank.set_route(route)
        for is_u8, d_in in inputs(oracle):
            for cuts in ([], [1, 1009, 1024]):
                rows = run_bank(bank, d_in, K_ALL, B, cuts, is_u8, stride=stride)
                for j in range(32):
                    assert_bit_equal(rows[j], BC.expected(oracle, tables[j], B), f"route {route}, stride 2 n + {extra}, cuts {cuts}, "
                                     f"{'u8' if is_u8 else 'cfloat'}: channel {j}")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_far_stream_position(hip, oracle, launch_route):
    """k_begin = 3 * 2^30 + 5 and in_base = 8 k_begin, periods 1000 and 5 in one bank, the device buffer holds only the slice: each
    channel's launch phase is a 64-bit reduction of its own (in_base mod 1000 = 816, mod 5 = 1)."""
    k_begin, in_base = BC.FAR_K0, 8 * BC.FAR_K0
    assert in_base % B == 40 and in_base % 1000 == 816 and in_base % 5 == 1
    ns = 3 * B - 40
    u8 = T.stream_u8()[:2 * ns]
    tables = [T.osc_table(1000), T.osc_table(5)]
    exp = [TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, oracle.convert_u8(u8), t, B, in_base, block_out=1) for t in tables]
    n_out = exp[0].size // 2
    assert n_out == (ns - 128) // 8 + 1
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    for route in (bank.ROUTE_BANKED, bank.ROUTE_CHANNELS):
        bank.set_route(route)
        for is_u8, d_in in inputs(oracle, u8):
            for cuts in ([], BC.FAR_CUTS):
                b0 = hip.tuner_bank_launches()
                rows = run_bank(bank, d_in, n_out, B, cuts, is_u8, k0=k_begin, in_base=in_base)
                assert hip.tuner_bank_launches() - b0 == ((len(cuts) + 1) if route == bank.ROUTE_BANKED else 0)
                for j in range(2):
                    assert_bit_equal(rows[j], exp[j], f"route {route}, cuts {cuts}, {'u8' if is_u8 else 'cfloat'}: channel {j}")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _short_case(hip, oracle, order, factor, ntaps):
    """3 blocks of 4096 samples, two channels (periods 5 and 1000): (bank, inputs, expected rows, outputs)."""
    nb, blk = 3, 4096
    u8 = T.stream_u8()[:2 * nb * blk]
    taps = S.taps_decim127() if ntaps == 127 else S.gauss_taps(ntaps, 40 + ntaps)
    tables = [T.osc_table(5), T.osc_table(1000)]
    exp = [TM.tuner_expected(oracle, taps, order, factor, oracle.convert_u8(u8), t, blk, 0, block_out=1) for t in tables]
    return hip.TunerBank(factor, taps, tables, order), inputs(oracle, u8), exp, exp[0].size // 2


@pytest.mark.parametrize("factor,ntaps", [(4, 127), (16, 127), (8, 31), (8, 52), (8, 64), (4, 52), (16, 31)])
def test_banked_launch_other_factors_and_tap_counts(hip, oracle, factor, ntaps, launch_route):
    bank, ins, exp, n_out = _short_case(hip, oracle, PM.ORDER_AVX, factor, ntaps)
    bank.set_route(bank.ROUTE_BANKED)
    for is_u8, d_in in ins:
        for cuts in ([], [64, 500]):
            b0, f0 = hip.tuner_bank_launches(), hip.tuner_fused_launches()
            rows = run_bank(bank, d_in, n_out, 4096, cuts, is_u8)
            assert hip.tuner_bank_launches() - b0 == len(cuts) + 1 and hip.tuner_fused_launches() == f0
            for j in range(2):
                assert_bit_equal(rows[j], exp[j], f"factor {factor}, {ntaps} taps, cuts {cuts}, {'u8' if is_u8 else 'cfloat'}: channel {j}")


@pytest.mark.parametrize("order,factor", [(PM.ORDER_SSE, 8), (PM.ORDER_SCALAR, 8), (PM.ORDER_AVX, 5)])
def test_other_orders_and_factors_go_channel_by_channel(hip, oracle, order, factor):
    bank, ins, exp, n_out = _short_case(hip, oracle, order, factor, 127)
    for is_u8, d_in in ins:
        b0 = hip.tuner_bank_launches()
        rows = run_bank(bank, d_in, n_out, 4096, [64, 500], is_u8)
        assert hip.tuner_bank_launches() == b0, "auto banked a shape the banked kernel does not serve"
        for j in range(2):
            assert_bit_equal(rows[j], exp[j], f"order {order}, factor {factor}, {'u8' if is_u8 else 'cfloat'}: channel {j}")
    bank.set_route(bank.ROUTE_BANKED)                        # no kernel for this shape: an error, not another route
    out = dev_empty_f32(4 * n_out)
    with pytest.raises(hip.SdrHipError):
        bank.run(ptr(ins[1][1]), 0, ptr(out), 2 * n_out, 0, n_out, 4096)
    assert (to_host(out).view(np.uint32) == CANARY).all(), "a refused run wrote a row"


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_auto_falls_back_where_a_launch_is_not_aligned(hip, oracle):
    """Factor 4 on u8: output 1's window starts 8 bytes into the buffer, which the tile kernel's 16-byte loads cannot take -- auto
    runs [1, 2) channel by channel and the other two launches banked, same bits; forced, the banked route refuses it."""
    u8 = T.stream_u8()[:2 * 3 * 4096]
    taps = S.taps_decim127()
    tables = [T.osc_table(1000), T.osc_table(5), BC.IDENTITY]
    exp = [TM.tuner_expected(oracle, taps, PM.ORDER_AVX, 4, oracle.convert_u8(u8), t, 4096, 0, block_out=1) for t in tables]
    n_out = exp[0].size // 2
    bank = hip.TunerBank(4, taps, tables)
    d_in = to_dev(u8)
    b0, f0 = hip.tuner_bank_launches(), hip.tuner_fused_launches()
    rows = run_bank(bank, d_in, n_out, 4096, [1, 2], True)
    assert hip.tuner_bank_launches() - b0 == 2               # [0, 1) and [2, n) are aligned, [1, 2) is not
    assert hip.tuner_fused_launches() == f0                  # ... and its tuners run it on their two-pass route
    for j in range(3):
        assert_bit_equal(rows[j], exp[j], f"factor 4, cut at outputs 1 and 2: channel {j}")
    bank.set_route(bank.ROUTE_BANKED)
    out = dev_empty_f32(6)
    with pytest.raises(hip.SdrHipError):
        bank.run_u8(ptr(d_in), 0, ptr(out), 2, 1, 2, 4096)
    assert (to_host(out).view(np.uint32) == CANARY).all(), "a refused run wrote a row"


def test_the_edges_of_the_auto_rule(hip, oracle):
    """Auto banks 2 or more channels and launches of at most 2^24 input samples (the rectangle of profiles/tuner_bank_bench.txt): one
    channel goes to its tuner, and one output past 2^24 / 8 goes channel by channel -- the same bits on both sides of each edge, held
    to tuners on the device."""
    import torch
    taps = S.taps_decim127()
    one = hip.TunerBank(8, taps, BC.bank_tables(1))
    d_u8 = to_dev(T.stream_u8())
    b0, f0 = hip.tuner_bank_launches(), hip.tuner_fused_launches()
    rows = run_bank(one, d_u8, K_ALL, B, [], True)
    assert hip.tuner_bank_launches() == b0 and hip.tuner_fused_launches() == f0 + 1, "auto banked one channel"
    assert_bit_equal(rows[0], BC.expected(oracle, BC.bank_tables(1)[0], B), "one channel under auto")
    edge = (1 << 24) // 8
    tables = [T.osc_table(1000), T.osc_table(5)]
    bank = hip.TunerBank(8, taps, tables)
    big = torch.randint(0, 256, (2 * (8 * edge + 128),), dtype=torch.uint8, device="cuda")
    for n_out, banked in ((edge, 1), (edge + 1, 0)):
        out = torch.zeros(2 * 2 * n_out, dtype=torch.float32, device="cuda")
        ref = torch.zeros(2 * n_out, dtype=torch.float32, device="cuda")
        b0 = hip.tuner_bank_launches()
        bank.run_u8(ptr(big), 0, ptr(out), 2 * n_out, 0, n_out, B)
        assert hip.tuner_bank_launches() - b0 == banked, f"{n_out} outputs of 2 channels under auto"
        for j, t in enumerate(tables):
            hip.Tuner(8, taps, t).run_u8(ptr(big), 0, ptr(ref), 0, n_out, B)
            torch.cuda.synchronize()
            assert torch.equal(out[2 * n_out * j:2 * n_out * (j + 1)].view(torch.int32), ref.view(torch.int32)), f"{n_out} outputs: channel {j}"


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_run_time_refusals_write_nothing(hip, oracle):
    bank = hip.TunerBank(8, S.taps_decim127(), BC.bank_tables(3))
    d_u8 = to_dev(T.stream_u8()[:2 * B])
    d_cf = to_dev(oracle.convert_u8(T.stream_u8()[:2 * B]))
    n = 64
    b0 = hip.tuner_bank_launches()
    for route in (0, 1, 2):
        bank.set_route(route)
        for run, d_in in ((hip.lib.sdrhip_tuner_bank_run, d_cf), (hip.lib.sdrhip_tuner_bank_run_u8, d_u8)):
            out = dev_empty_f32(3 * 2 * n)

            def refused(what, *args):
                assert run(bank.h, None, *args) == -1, f"route {route}: {what}"
                assert b"sdrhip_tuner_bank_run" in hip.lib.sdrhip_last_error(), what
                assert (to_host(out).view(np.uint32) == CANARY).all(), f"route {route}: {what}: a refused run wrote a row"

            refused("a seam block shorter than the 128 prepared taps", ptr(d_in), 0, ptr(out), 2 * n, 0, n, 127)
            refused("the first window starts before d_in", ptr(d_in), 8, ptr(out), 2 * n, 0, n, 0)
            refused("null input", None, 0, ptr(out), 2 * n, 0, n, 0)
            refused("null output", ptr(d_in), 0, None, 2 * n, 0, n, 0)
            refused("rows would overlap", ptr(d_in), 0, ptr(out), 2 * n - 2, 0, n, 0)
            refused("an odd out_stride", ptr(d_in), 0, ptr(out), 2 * n + 1, 0, n, 0)
            refused("k_end < k_begin", ptr(d_in), 0, ptr(out), 2 * n, n, 0, 0)
            assert run(bank.h, None, ptr(d_in), 0, ptr(out), 2 * n, 7, 7, 0) == 0             # an empty range: nothing to do
            assert (to_host(out).view(np.uint32) == CANARY).all()
    assert hip.tuner_bank_launches() == b0
    bank.set_route(bank.ROUTE_BANKED)
    out = dev_empty_f32(3 * 2 * n)
    with pytest.raises(hip.SdrHipError):
        bank.run(ptr(d_cf), 0, ptr(out), 2 * n, 0, n, -1)    # every output Cross: not a banked launch
    assert (to_host(out).view(np.uint32) == CANARY).all()
    bank.set_route(bank.ROUTE_AUTO)                          # ... auto runs it channel by channel: the tuner's bits
    bank.run(ptr(d_cf), 0, ptr(out), 2 * n, 0, n, -1)
    for j, t in enumerate(BC.bank_tables(3)):
        ref = dev_empty_f32(2 * n)
        hip.Tuner(8, S.taps_decim127(), t).run(ptr(d_cf), 0, ptr(ref), 0, n, -1)
        assert_bit_equal(to_host(out).reshape(3, 2 * n)[j], to_host(ref), f"all-Cross launch: channel {j} vs its tuner")
    assert hip.tuner_bank_launches() == b0


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_one_bank_two_host_threads(hip, oracle):
    """One bank, two host threads, each on a stream of its own, both routes in turn: the same bits as one thread."""
    import torch
    tables = BC.bank_tables(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    d_u8 = to_dev(T.stream_u8())
    for route in (bank.ROUTE_BANKED, bank.ROUTE_CHANNELS):
        bank.set_route(route)
        outs = [dev_empty_f32(3 * 2 * K_ALL) for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        errors = []
        torch.cuda.synchronize()

        def work(i):
            try:
                for rep in range(4):
                    edges = [0] + [c + i for c in CUTS] + [K_ALL]
                    for a, b in zip(edges[:-1], edges[1:]):
                        bank.run_u8(ptr(d_u8), 0, ptr(outs[i]) + 8 * a, 2 * K_ALL, a, b, B, stream=streams[i].cuda_stream)
                streams[i].synchronize()
            except Exception as e:                           # noqa: BLE001 -- reported below, on the main thread
                errors.append(e)

        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for q in th:
            q.start()
        for q in th:
            q.join()
        assert not errors, errors
        for i in range(2):
            rows = to_host(outs[i]).reshape(3, 2 * K_ALL)
            for j in range(3):
                assert_bit_equal(rows[j], BC.expected(oracle, tables[j], B), f"route {route}, thread {i}, channel {j}")
