"""GPU parity of 16-bit signed IQ into the tuner family: sdrhip_tuner_run_i16, sdrhip_tuner_bank_run_i16 and the bank's int16 Pipe.

Expected values are the restated Pipe (tests/tuner_model.py) on the stream oracle.convert_i16 makes of the int16 stream -- c(s) =
s * 2^-11, pinned to the reference build -- and the definition: the cfloat calls on the buffer sdrhip_convert_i16_run makes of the same
int16 buffer, and for the Pipe K one-row Pipe.tuner fed the converted floats at the same boundaries.  Every comparison is bit for bit
and every output buffer starts as NaN canaries.  Geometry: tests/test_gpu_tuner.py / tests/tuner_bank_cases.py -- 5 blocks of 8192
samples, 127 taps / 8, 5105 outputs (ten tiles of 512, the last ragged); the stream is tests/tuner_i16_cases.py's."""
import ctypes as C
import os
import struct
import subprocess
import threading

import numpy as np
import pytest

import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, CUTS, K_ALL, LP, D = IC.B, IC.CUTS, IC.K_ALL, 128, 8
launch_route = T.launch_route                  # Cross outputs in the tile kernel / tile kernel + fix-up launch
_f32p, _i16p = C.POINTER(C.c_float), C.POINTER(C.c_int16)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def counters(hip):
    return np.array([hip.tuner_bank_launches(), hip.tuner_bank_cross_launches(), hip.tuner_i16_launches(), hip.tuner_fused_launches()])


def dev_convert(hip, d_i16):
    """The definition's cfloat buffer: sdrhip_convert_i16_run on the device buffer itself."""
    import torch
    out = torch.empty(d_i16.numel(), dtype=torch.float32, device="cuda")
    hip.check(hip.lib.sdrhip_convert_i16_run(None, ptr(d_i16), ptr(out), d_i16.numel()), "sdrhip_convert_i16_run")
    torch.cuda.synchronize()
    return out


def run_bank(bank, d_in, n_out, seam, cuts, i16=True, stride=None, k0=0, in_base=0, stream=None, in_ptr=None):
    """Outputs [k0, k0 + n_out) of every channel as launches cut at k0 + cuts -> rows [channels, 2 n_out]; the floats between the
    rows must be canaries afterwards."""
    nch = bank.channels
    stride = 2 * n_out if stride is None else stride
    out = dev_empty_f32(nch * stride)
    edges = [0] + [c for c in cuts if c < n_out] + [n_out]
    p = ptr(d_in) if in_ptr is None else in_ptr
    for a, b in zip(edges[:-1], edges[1:]):
        (bank.run_i16 if i16 else bank.run)(p, in_base, ptr(out) + 8 * a, stride, k0 + a, k0 + b, seam, stream)
    whole = to_host(out).reshape(nch, stride)
    gaps = whole.view(np.uint32)[:, 2 * n_out:]
    assert (gaps == CANARY).all(), f"{int((gaps != CANARY).sum())} floats between the rows were written"
    return whole[:, :2 * n_out]


def run_tuner(t, d_in, K, seam, cuts, i16=True, k0=0, in_base=0, in_ptr=None):
    out = dev_empty_f32(2 * K)
    edges = [0] + [c for c in cuts if c < K] + [K]
    p = ptr(d_in) if in_ptr is None else in_ptr
    for a, b in zip(edges[:-1], edges[1:]):
        (t.run_i16 if i16 else t.run)(p, in_base, ptr(out) + 8 * a, k0 + a, k0 + b, seam)
    return to_host(out)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
@pytest.mark.parametrize("nch", [1, 3, 32])
def test_banked_launch_against_the_model(hip, oracle, nch, seam, launch_route):
    tables = BC.bank_tables(nch)
    exp = [IC.expected(oracle, t, seam) for t in tables]
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    bank.set_route(bank.ROUTE_BANKED)
    d_in = to_dev(IC.stream_i16())
    what = f"{nch} channels, seam {seam}"
    for cuts, n_out, name in (([], K_ALL, "one launch"), (CUTS, K_ALL, "cut into launches"), ([], 4097, "one output into the ninth tile"),
                              ([], 4608, "whole tiles")):
        c0 = counters(hip)
        rows = run_bank(bank, d_in, n_out, seam, cuts)
        d = counters(hip) - c0
        assert (d[0], d[2], d[3]) == (len(cuts) + 1, len(cuts) + 1, 0), what + f", {name}: (banked, int16 tile kernel, tuners' own) launches"
        for j in range(nch):
            assert_bit_equal(rows[j], exp[j][:2 * n_out], what + f", {name}: channel {j} (period {bank.period(j)})")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
def test_against_the_definition(hip, oracle, seam, launch_route):
    """The same launches of TunerBank.run on the buffer sdrhip_convert_i16_run makes, on routes 1, 2 and 0."""
    tables = BC.bank_tables(3) + [T.osc_table(5), T.osc_table(65536)]
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    d_in = to_dev(IC.stream_i16())
    d_cf = dev_convert(hip, d_in)
    assert_bit_equal(to_host(d_cf), oracle.convert_i16(IC.stream_i16()), "sdrhip_convert_i16_run against the oracle")
    for route in (bank.ROUTE_BANKED, bank.ROUTE_CHANNELS, bank.ROUTE_AUTO):
        bank.set_route(route)
        ref = run_bank(bank, d_cf, K_ALL, seam, CUTS, i16=False)
        c0 = counters(hip)
        rows = run_bank(bank, d_in, K_ALL, seam, CUTS)
        d = counters(hip) - c0
        n = len(CUTS) + 1
        # channel by channel every launch is five one-row launches of the same int16 tile kernel, none of them a banked launch
        assert (d[0], d[2], d[3]) == ((0, 5 * n, 0) if route == bank.ROUTE_CHANNELS else (n, n, 0)), f"route {route}"
        for j in range(len(tables)):
            assert_bit_equal(rows[j], ref[j], f"route {route}, seam {seam}: channel {j} vs the cfloat bank on the converted buffer")
            assert_bit_equal(rows[j], IC.expected(oracle, tables[j], seam), f"route {route}, seam {seam}: channel {j} vs the model")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [0, 2, 6])
def test_row_stride(hip, oracle, extra, launch_route):
    tables = BC.bank_tables(32)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    bank.set_route(bank.ROUTE_BANKED)
    stride = 2 * K_ALL + extra
    assert (stride % 4 == 2) == (extra == 0)
    d_in = to_dev(IC.stream_i16())
    rows = run_bank(bank, d_in, K_ALL, B, [1, 1009, 1024], stride=stride)
    for j in range(32):
        assert_bit_equal(rows[j], IC.expected(oracle, tables[j], B), f"stride 2 n + {extra}: channel {j}")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [4097, K_ALL, 100])
def test_the_ragged_end_reads_no_sample_past_the_last_window(hip, oracle, n_out, launch_route):
    """The device buffer holds exactly the samples the call may read, followed by the stream's own continuation with the top bit of
    every value flipped: a loader that read past the last window would mix other values."""
    s = IC.stream_i16()
    need = (n_out - 1) * D + LP
    cont = np.concatenate([s, s])[2 * need:2 * need + 2 * 4096]
    guard = (cont.view(np.uint16) ^ np.uint16(0x8000)).view(np.int16)
    d_in = to_dev(np.concatenate([s[:2 * need], guard]))
    tables = BC.bank_tables(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    bank.set_route(bank.ROUTE_BANKED)
    rows = run_bank(bank, d_in, n_out, B, [])
    for j in range(3):
        assert_bit_equal(rows[j], IC.expected(oracle, tables[j], B)[:2 * n_out], f"{n_out} outputs, {need} samples: channel {j}")
    t = hip.Tuner(8, S.taps_decim127(), tables[0])
    for route in (hip.TUNER_ROUTE_FUSED, hip.TUNER_ROUTE_TWO_PASS):
        t.set_route(route)
        assert_bit_equal(run_tuner(t, d_in, n_out, B, []), IC.expected(oracle, tables[0], B)[:2 * n_out], f"one row, route {route}")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_far_stream_position(hip, oracle, launch_route):
    k_begin, in_base = BC.FAR_K0, 8 * BC.FAR_K0
    assert in_base % B == 40 and in_base % 1000 == 816 and in_base % 5 == 1
    ns = 3 * B - 40
    s = IC.stream_i16()[:2 * ns]
    tables = [T.osc_table(1000), T.osc_table(5)]
    exp = [TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, oracle.convert_i16(s), t, B, in_base, block_out=1) for t in tables]
    n_out = exp[0].size // 2
    assert n_out == (ns - 128) // 8 + 1
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    d_in = to_dev(s)
    for route in (bank.ROUTE_BANKED, bank.ROUTE_CHANNELS):
        bank.set_route(route)
        for cuts in ([], BC.FAR_CUTS):
            c0 = counters(hip)
            rows = run_bank(bank, d_in, n_out, B, cuts, k0=k_begin, in_base=in_base)
            assert (counters(hip) - c0)[0] == ((len(cuts) + 1) if route == bank.ROUTE_BANKED else 0)
            for j in range(2):
                assert_bit_equal(rows[j], exp[j], f"route {route}, cuts {cuts}: channel {j}")


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,ntaps", [(4, 127), (16, 127), (8, 64), (8, 52), (8, 128), (4, 52), (16, 31)])
def test_banked_launch_other_factors_and_tap_counts(hip, oracle, factor, ntaps, launch_route):
    """Factors 4 and 16, 64 taps, tap counts that are 4 mod 8 (52 prepared taps: the TC = 4 walk) and exactly 128 taps (the unguarded
    walk): 3 blocks of 4096 samples, two channels."""
    nb, blk = 3, 4096
    s = IC.stream_i16()[:2 * nb * blk]
    taps = S.taps_decim127() if ntaps == 127 else S.gauss_taps(ntaps, 40 + ntaps)
    tables = [T.osc_table(5), T.osc_table(1000)]
    bank = hip.TunerBank(factor, taps, tables)
    if ntaps in (52, 128):
        assert bank.num_coeffs == ntaps
    exp = [IC.expected(oracle, t, blk, factor=factor, taps=taps, i16=s) for t in tables]
    n_out = exp[0].size // 2
    bank.set_route(bank.ROUTE_BANKED)
    d_in = to_dev(s)
    for cuts in ([], [64, 500]):
        c0 = counters(hip)
        rows = run_bank(bank, d_in, n_out, blk, cuts)
        d = counters(hip) - c0
        assert (d[0], d[2], d[3]) == (len(cuts) + 1, len(cuts) + 1, 0)
        for j in range(2):
            assert_bit_equal(rows[j], exp[j], f"factor {factor}, {ntaps} taps, cuts {cuts}: channel {j}")


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_alignment(hip, oracle):
    """d_in one sample (4 bytes) past a 16-byte boundary: the banked route refuses with nothing written, auto falls back and gives the
    same bits; 2 bytes past it is no int16 IQ buffer at all and is refused on every route."""
    s = IC.stream_i16()
    tables = BC.bank_tables(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    d4 = to_dev(np.concatenate([np.full(2, 12345, np.int16), s]))
    assert ptr(d4) % 16 == 0
    n = 600
    bank.set_route(bank.ROUTE_BANKED)
    out = dev_empty_f32(3 * 2 * n)
    c0 = counters(hip)
    with pytest.raises(hip.SdrHipError):
        bank.run_i16(ptr(d4) + 4, 0, ptr(out), 2 * n, 0, n, B)
    assert (to_host(out).view(np.uint32) == CANARY).all() and (counters(hip) == c0).all(), "a refused run wrote a row or launched"
    bank.set_route(bank.ROUTE_AUTO)
    rows = run_bank(bank, d4, K_ALL, B, CUTS, in_ptr=ptr(d4) + 4)
    d = counters(hip) - c0
    assert d[0] == 0 and d[2] == 0 and d[3] == 0, "a launch that is not aligned went to a tile kernel"
    for j in range(3):
        assert_bit_equal(rows[j], IC.expected(oracle, tables[j], B), f"4 bytes off, auto: channel {j}")
    t = hip.Tuner(8, S.taps_decim127(), tables[0])
    t.set_route(hip.TUNER_ROUTE_FUSED)
    with pytest.raises(hip.SdrHipError):
        t.run_i16(ptr(d4) + 4, 0, ptr(out), 0, n, B)
    assert (to_host(out).view(np.uint32) == CANARY).all()
    d2 = to_dev(np.concatenate([np.full(1, 12345, np.int16), s]))
    for route in (0, 1, 2):
        bank.set_route(route)
        t.set_route(route)
        with pytest.raises(hip.SdrHipError):
            bank.run_i16(ptr(d2) + 2, 0, ptr(out), 2 * n, 0, n, B)
        with pytest.raises(hip.SdrHipError):
            t.run_i16(ptr(d2) + 2, 0, ptr(out), 0, n, B)
    assert (to_host(out).view(np.uint32) == CANARY).all() and (counters(hip) - c0)[2] == 0


def test_the_edges_of_the_auto_rule(hip, oracle):
    """Auto banks 2 or more channels and launches of at most 2^24 input samples (the rectangle of profiles/tuner_i16_bench.txt): one
    channel goes to its tuner -- the same kernel, counted as no banked launch -- and one output past 2^24 / 8 goes channel by channel;
    the same bits on both sides of the edge, held to one-row tuners on the device."""
    import torch
    taps = S.taps_decim127()
    one = hip.TunerBank(8, taps, BC.bank_tables(1))
    d_in = to_dev(IC.stream_i16())
    c0 = counters(hip)
    rows = run_bank(one, d_in, K_ALL, B, [])
    assert tuple(counters(hip) - c0) == (0, 0, 1, 0), "auto banked one channel"
    assert_bit_equal(rows[0], IC.expected(oracle, BC.bank_tables(1)[0], B), "one channel under auto")
    edge = (1 << 24) // 8
    tables = [T.osc_table(1000), T.osc_table(5)]
    bank = hip.TunerBank(8, taps, tables)
    big = torch.randint(-32768, 32768, (2 * (8 * edge + 128),), dtype=torch.int16, device="cuda")
    for n_out, banked in ((edge, 1), (edge + 1, 0)):
        out = torch.zeros(2 * 2 * n_out, dtype=torch.float32, device="cuda")
        ref = torch.zeros(2 * n_out, dtype=torch.float32, device="cuda")
        c0 = counters(hip)
        bank.run_i16(ptr(big), 0, ptr(out), 2 * n_out, 0, n_out, B)
        d = counters(hip) - c0
        assert (d[0], d[2]) == (banked, 1 if banked else 2), f"{n_out} outputs of 2 channels under auto"
        for j, t in enumerate(tables):
            hip.Tuner(8, taps, t).run_i16(ptr(big), 0, ptr(ref), 0, n_out, B)
            torch.cuda.synchronize()
            assert torch.equal(out[2 * n_out * j:2 * n_out * (j + 1)].view(torch.int32), ref.view(torch.int32)), f"{n_out} outputs: channel {j}"


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
def test_one_row_tuner(hip, oracle, seam, launch_route):
    d_in = to_dev(IC.stream_i16())
    for n in (1000, 5, 1):
        table = T.osc_table(n)
        exp = IC.expected(oracle, table, seam)
        t = hip.Tuner(8, S.taps_decim127(), table)
        t.set_route(hip.TUNER_ROUTE_FUSED)
        c0 = counters(hip)
        assert_bit_equal(run_tuner(t, d_in, K_ALL, seam, []), exp, f"period {n}, seam {seam}, fused: one launch")
        assert_bit_equal(run_tuner(t, d_in, K_ALL, seam, CUTS), exp, f"period {n}, seam {seam}, fused: cut into launches")
        assert tuple(counters(hip) - c0) == (0, 0, len(CUTS) + 2, 0), "(banked, cross, int16 tile kernel, cfloat / u8 tile kernel) launches"
        t.set_route(hip.TUNER_ROUTE_TWO_PASS)
        prev = hip.set_tuner_chunk(12000)               # 40960 samples: four chunks
        try:
            c0 = counters(hip)
            assert_bit_equal(run_tuner(t, d_in, K_ALL, seam, []), exp, f"period {n}, seam {seam}, two-pass in four chunks")
            assert_bit_equal(run_tuner(t, d_in, K_ALL, seam, CUTS), exp, f"period {n}, seam {seam}, two-pass, cut into launches")
            assert (counters(hip) == c0).all(), "the two-pass route launched a tile kernel of the tuner family"
        finally:
            hip.set_tuner_chunk(prev)


def test_one_row_tuner_shapes_only_the_two_pass_route_serves(hip, oracle):
    s = IC.stream_i16()
    d_in = to_dev(s)
    d_cf = dev_convert(hip, d_in)
    x = oracle.convert_i16(s)
    table = T.osc_table(1000)
    for order, factor in ((PM.ORDER_SSE, 8), (PM.ORDER_AVX, 3)):
        taps = S.taps_decim127()
        t = hip.Tuner(factor, taps, table, order)
        K = (IC.NBLK * B - t.num_coeffs) // factor + 1
        for seam in ((B, 0) if factor == 8 else (0,)):
            e = TM.tuner_expected(oracle, taps, order, factor, x, table, seam, 0, block_out=1)
            c0 = counters(hip)
            assert_bit_equal(run_tuner(t, d_in, K, seam, CUTS), e, f"order {order}, factor {factor}, seam {seam}: auto")
            assert (counters(hip) == c0).all()
        t.set_route(hip.TUNER_ROUTE_FUSED)
        out = dev_empty_f32(2 * 64)
        with pytest.raises(hip.SdrHipError):
            t.run_i16(ptr(d_in), 0, ptr(out), 0, 64, 0)
        assert (to_host(out).view(np.uint32) == CANARY).all(), "a refused run wrote"
    # seam_block = -1 (every output Cross) on route 2, against the definition
    t = hip.Tuner(8, S.taps_decim127(), table)
    t.set_route(hip.TUNER_ROUTE_TWO_PASS)
    assert_bit_equal(run_tuner(t, d_in, 700, -1, [1, 300]), run_tuner(t, d_cf, 700, -1, [1, 300], i16=False), "seam_block -1, two-pass")


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_run_time_refusals_write_nothing(hip, oracle):
    bank = hip.TunerBank(8, S.taps_decim127(), BC.bank_tables(3))
    d_in = to_dev(IC.stream_i16()[:2 * B])
    n = 64
    c0 = counters(hip)
    run = hip.lib.sdrhip_tuner_bank_run_i16
    for route in (0, 1, 2):
        bank.set_route(route)
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
        assert run(bank.h, None, ptr(d_in), 0, ptr(out), 2 * n, 7, 7, 0) == 0
        assert (to_host(out).view(np.uint32) == CANARY).all()
    bank.set_route(bank.ROUTE_BANKED)
    out = dev_empty_f32(3 * 2 * n)
    with pytest.raises(hip.SdrHipError):
        bank.run_i16(ptr(d_in), 0, ptr(out), 2 * n, 0, n, -1)     # every output Cross: not a banked launch
    assert (to_host(out).view(np.uint32) == CANARY).all()
    assert (counters(hip) == c0).all()
    bank.set_route(bank.ROUTE_AUTO)                               # ... auto runs it channel by channel: the definition's bits
    bank.run_i16(ptr(d_in), 0, ptr(out), 2 * n, 0, n, -1)
    ref = dev_empty_f32(3 * 2 * n)
    bank.run(ptr(dev_convert(hip, d_in)), 0, ptr(ref), 2 * n, 0, n, -1)
    assert_bit_equal(to_host(out), to_host(ref), "all-Cross launch against the cfloat bank on the converted buffer")


def test_one_bank_two_host_threads(hip, oracle):
    import torch
    tables = BC.bank_tables(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    d_in = to_dev(IC.stream_i16())
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
                        bank.run_i16(ptr(d_in), 0, ptr(outs[i]) + 8 * a, 2 * K_ALL, a, b, B, stream=streams[i].cuda_stream)
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
                assert_bit_equal(rows[j], IC.expected(oracle, tables[j], B), f"route {route}, thread {i}, channel {j}")


# ==== the Pipe ======================================================================================================================
PNBLK = 19                                     # 19 blocks: two submissions of 16 coalesced blocks, seven of 3
_pcache = {}


def to_f32(i16):
    return i16.astype(np.float32) * np.float32(2.0 ** -11)          # exact: c(s)


def cut(s, sizes):
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] * 2 <= s.size
    return [s[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:])]


def tables_for(nch):
    return [T.osc_table(1000), T.osc_table(5)] if nch == 2 else BC.bank_tables(nch)


def one_row_expected(hip, table, sizes, block_out, s, factor=8, taps=None, state=None):
    """The definition: Pipe.tuner over a Tuner with this table, fed the converted float blocks (once per case, shared, never written)."""
    taps = S.taps_decim127() if taps is None else taps
    key = (np.asarray(table, np.float32).tobytes(), tuple(int(v) for v in sizes), block_out, factor, taps.tobytes(), s.size, s[:64].tobytes())
    if state is None and key in _pcache:
        return _pcache[key]
    p = hip.Pipe.tuner(hip.Tuner(factor, taps, table), block_out)
    p.set_adaptive(0)
    outs = list(p.restore(state)) if state is not None else []
    for blk in cut(s, sizes):
        outs += p.push(to_f32(blk))
    outs += p.flush()
    e = np.concatenate(outs) if outs else np.empty(0, np.float32)
    e.setflags(write=False)
    if state is None:
        _pcache[key] = e
    return e


class BankPipe:
    """The bank's int16 Pipe through the raw C calls: every pop goes into canaries and the words around each row are checked."""

    def __init__(self, hip, bank, block_out):
        self.hip, self.bo = hip, block_out
        self.p = hip.Pipe.tuner_bank(bank, block_out, input_i16=True)
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []

    def _pop(self, ready):
        self.counts.append(ready)
        if ready <= 0:
            return
        n, gap = ready * 2 * self.bo, 6
        stride = n + gap
        buf = np.full(8 + self.rows * stride, CANARY, np.uint32)
        out = buf[8:].view(np.float32)
        nb = self.hip.check(self.hip.lib.sdrhip_pipe_pop_rows(self.p.h, out.ctypes.data_as(_f32p), stride, ready), "sdrhip_pipe_pop_rows")
        assert nb == ready
        r = buf[8:].reshape(self.rows, stride)
        assert (buf[:8] == CANARY).all() and (r[:, n:] == CANARY).all(), "a pop wrote outside its rows"
        for j in range(self.rows):
            self.got[j].append(r[j, :n].copy())

    def push(self, blk, via_buffer=False):
        if via_buffer:
            view = self.p.input_buffer(blk.size // 2)
            assert view.dtype == np.int16 and view.size == blk.size
            view[:] = blk
            rc = self.hip.lib.sdrhip_pipe_push_i16(self.p.h, view.ctypes.data_as(_i16p), blk.size // 2)
        else:
            b = np.ascontiguousarray(blk)
            rc = self.hip.lib.sdrhip_pipe_push_i16(self.p.h, b.ctypes.data_as(_i16p), b.size // 2)
        self._pop(self.hip.check(rc, "sdrhip_pipe_push_i16"))

    def flush(self):
        self._pop(self.hip.check(self.hip.lib.sdrhip_pipe_flush(self.p.h), "sdrhip_pipe_flush"))

    def restore(self, state):
        self._pop(self.hip.check(self.hip.lib.sdrhip_pipe_restore(self.p.h, state, C.c_size_t(len(state))), "sdrhip_pipe_restore"))

    def row(self, j):
        return np.concatenate(self.got[j]).view(np.float32) if self.got[j] else np.empty(0, np.float32)


def check_rows(hip, bp, tables, sizes, block_out, what, s, **kw):
    for j, t in enumerate(tables):
        exp = one_row_expected(hip, t, sizes, block_out, s, **kw)
        assert exp.size > 0
        assert_bit_equal(bp.row(j), exp, f"{what}: channel {j} vs its one-row Pipe.tuner on the converted floats")


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3, 16])
@pytest.mark.parametrize("nch", [1, 2, 3, 32])
def test_pipe_uniform_pushes(hip, oracle, nch, group):
    tables = tables_for(nch)
    sizes = [B] * PNBLK
    s = IC.stream_i16(PNBLK * B)
    blocks = cut(s, sizes)
    for bo in (1000, 1024):
        bank = hip.TunerBank(8, S.taps_decim127(), tables)
        if nch == 1:
            bank.set_route(bank.ROUTE_BANKED)
        bp = BankPipe(hip, bank, bo)
        assert bp.rows == nch
        bp.p.set_adaptive(0)
        if group > 1:
            bp.p.set_coalesce(group)
        c0 = counters(hip)
        for blk in blocks:
            bp.push(blk)
        bp.flush()
        what = f"{nch} channels, {group} blocks per submission, block_size_out {bo}"
        nsub = -(-PNBLK // group)
        assert tuple(counters(hip) - c0) == (nsub, 0, nsub, 0), what + ": (banked, cross, int16 tile kernel, tuners' own) launches"
        assert sum(bp.counts) == bp.row(0).size // (2 * bo) == ((PNBLK * B - LP) // D + 1) // bo, what + ": blocks per channel"
        check_rows(hip, bp, tables, sizes, bo, what, s)
        if nch == 2 and group == 3 and bo == 1000:
            x = oracle.convert_i16(s)
            for j, t in enumerate(tables):
                m = TM.mix(x, t)
                model = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=8)
                out, _ = PM.fir_decimator_pipe(model, [m[2 * B * i:2 * B * (i + 1)] for i in range(PNBLK)], bo)
                assert_bit_equal(bp.row(j), np.concatenate(out), what + f": channel {j} vs the restated Pipe")


# ---- 11 --------------------------------------------------------------------------------------------------------------------------
def ragged_sizes(lo=LP, hi=3 * B, n=20, seed=5):
    rng = np.random.default_rng(seed)
    return [B, B, B] + [int(v) for v in rng.integers(lo, hi + 1, n)]


def cross_counts(sizes, lp=LP, d=D):
    out, e = [], 0
    for n in sizes:
        m_done = (e - lp) // d + 1 if e >= lp else 0
        m_split = max(-(-e // d), m_done)
        out.append(m_split - m_done)
        e += n
    return out


@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
def test_pipe_ragged_pushes(hip, oracle, mode):
    """Per ragged submission ONE cross launch for all channels and ONE banked launch -- odd sizes included, because the copy lands
    where the banked launch's first window is 16-byte aligned.  Every third push goes through input_buffer."""
    sizes = ragged_sizes()
    big = IC.stream_i16(28 * B)
    assert sum(sizes) <= 28 * B and any(v % 2 for v in sizes[3:]) and any(v % 8 == 0 for v in sizes[3:-1])
    ragged = cross_counts(sizes)[3:]
    assert min(ragged) == 15 and max(ragged) == 16 == -(-LP // D), "the seed shows both Cross counts, the maximal one included"
    tables = tables_for(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    bp = BankPipe(hip, bank, 1000)
    if mode == "plain":
        bp.p.set_adaptive(0)
    elif mode == "coalesce 7":
        bp.p.set_coalesce(7)
    else:
        bp.p.set_adaptive(32)
    blocks = cut(big, sizes)
    for i, blk in enumerate(blocks[:3]):
        bp.push(blk, via_buffer=(i == 1))
    c0 = counters(hip)
    bp.push(blocks[3])                                  # ends the uniform run: what is still staged goes out, then the ragged block
    c1 = counters(hip)
    assert c1[1] - c0[1] == 1 and c1[3] == c0[3] and 1 <= c1[0] - c0[0] <= 2 and c1[2] - c0[2] == c1[0] - c0[0], mode
    for i, blk in enumerate(blocks[4:]):
        bp.push(blk, via_buffer=(i % 3 == 0))
        c2 = counters(hip)
        assert tuple(c2 - c1) == (1, 1, 1, 0), (f"{mode}: ragged push {i + 4} of {blk.size // 2} samples: (banked, cross, int16 tile "
                                                "kernel, tuners' own) launches")
        c1 = c2
    bp.flush()
    assert (counters(hip) == c1).all(), "flush launched although nothing was staged"
    check_rows(hip, bp, tables, sizes, 1000, f"ragged pushes, {mode}", big)
    if mode == "plain":
        x = oracle.convert_i16(big)
        edges = np.concatenate([[0], np.cumsum(sizes)])
        for j, t in enumerate(tables[:2]):
            m = TM.mix(x, t)
            model = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=8)
            out, _ = PM.fir_decimator_pipe(model, [m[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:])], 1000)
            assert_bit_equal(bp.row(j), np.concatenate(out), f"ragged pushes: channel {j} vs the restated Pipe")


# ---- 12 --------------------------------------------------------------------------------------------------------------------------
def test_pipe_pushes_without_an_output_and_short_pushes(hip):
    tables = tables_for(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    s = IC.stream_i16(PNBLK * B)
    bp = BankPipe(hip, bank, 1000)
    bp.p.set_coalesce(4)                                 # three pushes are staged: no submission, no launch
    c0 = counters(hip)
    for blk in cut(s, [B, B, B]):
        bp.push(blk)
    assert (counters(hip) == c0).all() and bp.counts == [0, 0, 0]
    bp.flush()
    assert tuple(counters(hip) - c0) == (1, 0, 1, 0)
    c1 = counters(hip)
    short = np.ascontiguousarray(s[:2 * (LP - 1)])
    rc = hip.lib.sdrhip_pipe_push_i16(bp.p.h, short.ctypes.data_as(_i16p), LP - 1)
    assert rc == -1 and b"shorter than the filter" in hip.lib.sdrhip_last_error()
    assert (counters(hip) == c1).all()
    bp.p.set_coalesce(0)
    bp.p.set_adaptive(0)
    bp.push(s[2 * 3 * B:2 * 4 * B])
    bp.flush()
    check_rows(hip, bp, tables, [B] * 4, 1000, "after a refused push", s)


def test_the_wrong_push_call_is_refused_for_each_input_type(hip):
    bank = hip.TunerBank(8, S.taps_decim127(), tables_for(2))
    s = np.ascontiguousarray(IC.stream_i16()[:2 * B])
    f = to_f32(s)
    u = (s.view(np.uint16) >> 8).astype(np.uint8)
    pi, pu, pf = hip.Pipe.tuner_bank(bank, 1000, input_i16=True), hip.Pipe.tuner_bank(bank, 1000, input_u8=True), hip.Pipe.tuner_bank(bank, 1000)
    push = {"f": lambda p: hip.lib.sdrhip_pipe_push(p.h, f.ctypes.data_as(_f32p), B),
            "u": lambda p: hip.lib.sdrhip_pipe_push_u8(p.h, u.ctypes.data_as(C.POINTER(C.c_uint8)), B),
            "i": lambda p: hip.lib.sdrhip_pipe_push_i16(p.h, s.ctypes.data_as(_i16p), B)}
    buf = {"f": hip.lib.sdrhip_pipe_input_buffer, "u": hip.lib.sdrhip_pipe_input_buffer_u8, "i": hip.lib.sdrhip_pipe_input_buffer_i16}
    names = {"f": b"float blocks (sdrhip_pipe_push)", "u": b"u8 IQ blocks (sdrhip_pipe_push_u8)", "i": b"int16 IQ blocks (sdrhip_pipe_push_i16)"}
    c0 = counters(hip)
    for own, p in (("i", pi), ("u", pu), ("f", pf)):
        for other in "fui":
            if other == own:
                continue
            assert push[other](p) == -1, f"a {own} pipe took a push of type {other}"
            assert names[own] in hip.lib.sdrhip_last_error(), hip.lib.sdrhip_last_error()
            assert not buf[other](p.h, B), f"a {own} pipe lent a buffer of type {other}"
            assert names[own].replace(b"push", b"input_buffer") in hip.lib.sdrhip_last_error(), hip.lib.sdrhip_last_error()
    for p, bad in ((pi, f), (pi, u), (pu, s), (pu, f), (pf, u)):
        with pytest.raises(hip.SdrHipError):
            p.push(bad)
    for p in (pi, pu, pf):
        assert p.flush() == []                          # nothing was staged
    assert (counters(hip) == c0).all()
    assert len(pi.push(s) + pi.flush()) == 1            # ... and the right call still works through the binding


# ---- 13 --------------------------------------------------------------------------------------------------------------------------
def test_pipe_save_and_restore(hip):
    tables = tables_for(3)
    taps = S.taps_decim127()
    bank = hip.TunerBank(8, taps, tables)
    sizes = [2048] * 40
    s = IC.stream_i16(PNBLK * B)
    blocks = cut(s, sizes)
    a = BankPipe(hip, bank, 1000)
    for blk in blocks[:5]:
        a.push(blk)
    state = a.p.save()
    version, = struct.unpack_from("<I", state, 4)
    assert version == 2
    b = BankPipe(hip, bank, 1000)

    def refused(pipe, st, what):
        assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
        assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what
        assert hip.lib.sdrhip_pipe_poll(pipe.h) == 0, what + ": the pipe changed"

    refused(b.p, state[:-1], "a truncated state")
    refused(b.p, state[:60], "a state cut inside its header")
    refused(hip.Pipe.tuner_bank(hip.TunerBank(8, taps, tables[:2]), 1000, input_i16=True), state, "another row count")
    pu, pf = hip.Pipe.tuner_bank(bank, 1000, input_u8=True), hip.Pipe.tuner_bank(bank, 1000)
    refused(pu, state, "an int16 state on a u8 pipe")
    refused(pf, state, "an int16 state on a cfloat pipe")
    for p, blk, what in ((pu, (blocks[0].view(np.uint16) >> 8).astype(np.uint8), "u8"), (pf, to_f32(blocks[0]), "cfloat")):
        q = hip.Pipe.tuner_bank(bank, 1000, input_u8=(what == "u8"))
        q.push(blk)
        st = q.save()
        refused(b.p, st, f"a {what} state on an int16 pipe")
        other = pf if what == "u8" else pu
        refused(other, st, f"a {what} state on the other float / u8 pipe")
    one16 = hip.Pipe.tuner_bank(hip.TunerBank(8, taps, tables[:1]), 1000, input_i16=True)
    refused(one16, state, "a three-row state on a one-row int16 pipe")
    refused(hip.Pipe.tuner_bank(bank, 1024, input_i16=True), state, "another block_size_out")
    refused(hip.Pipe.tuner_bank(hip.TunerBank(16, taps, tables), 1000, input_i16=True), state, "another factor")
    refused(hip.Pipe.tuner(hip.Tuner(8, taps, tables[0]), 1000), state, "a one-row tuner pipe")
    b.restore(state)                                     # ... and after all those refusals the pipe is as fresh as it was
    for blk in blocks[5:]:
        a.push(blk)
        b.push(blk)
    a.flush()
    b.flush()
    check_rows(hip, a, tables, sizes, 1000, "the saved pipe", s)
    nb_before = sum(a.counts[:5])
    for j in range(3):
        assert_bit_equal(b.row(j), a.row(j)[nb_before * 2000:], f"restored pipe: channel {j}")


def test_pipe_state_names_the_input_type_and_keeps_the_history_as_int16(hip):
    """Version 2, input type 2 behind the header, and the state is smaller than the cfloat pipe's by 4 bytes per history sample."""
    bank = hip.TunerBank(8, S.taps_decim127(), tables_for(3))
    s = IC.stream_i16(PNBLK * B)
    states = {}
    for kind in ("i16", "cf"):
        p = hip.Pipe.tuner_bank(bank, 1000, input_i16=(kind == "i16"))
        p.set_adaptive(0)
        blk = s[:2 * B]
        p.push(blk if kind == "i16" else to_f32(blk))
        p.flush()
        states[kind] = p.save()
    assert struct.unpack_from("<I", states["i16"], 4)[0] == 2
    hist_n, = struct.unpack_from("<q", states["i16"], 72)
    assert hist_n > 0 and len(states["cf"]) - len(states["i16"]) == 4 * hist_n, "the history travels as int16 pairs: 4 bytes per sample, not 8"
    # (rows, input type) directly behind the 112-byte header
    assert struct.unpack_from("<ii", states["i16"], 112) == (3, 2) and struct.unpack_from("<ii", states["cf"], 112) == (3, 0)


def moved(state, samples, factor=8):
    e_prev, m_done = struct.unpack_from("<qq", state, 48)
    assert samples % factor == 0
    return state[:48] + struct.pack("<qq", e_prev + samples, m_done + samples // factor) + state[64:]


def test_pipe_far_stream_position(hip):
    tables = [T.osc_table(1000), T.osc_table(5)]
    taps = S.taps_decim127()
    bank = hip.TunerBank(8, taps, tables)
    sizes = [B] * 6
    s = IC.stream_i16(PNBLK * B)
    blocks = cut(s, sizes)
    far = 1 << 33
    a = BankPipe(hip, bank, 1000)
    a.p.set_adaptive(0)
    a.push(blocks[0])
    a.flush()
    st = moved(a.p.save(), far)
    b = BankPipe(hip, bank, 1000)
    b.p.set_adaptive(0)
    b.restore(st)
    c0 = counters(hip)
    for blk in blocks[1:]:
        b.push(blk)
    b.flush()
    assert tuple(counters(hip) - c0) == (5, 0, 5, 0)
    for j, t in enumerate(tables):
        one = hip.Pipe.tuner(hip.Tuner(8, taps, t), 1000)
        one.set_adaptive(0)
        one.push(to_f32(blocks[0]))
        one.flush()
        exp = one_row_expected(hip, t, sizes[1:], 1000, s[2 * B:], state=moved(one.save(), far))
        assert exp.size >= 4 * 2000
        assert_bit_equal(b.row(j), exp, f"far position: channel {j}")


def test_pipe_pop_against_pop_rows(hip):
    s = IC.stream_i16(PNBLK * B)
    blocks = cut(s, [B] * 4)
    t1 = tables_for(1)
    p = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), t1), 1000, input_i16=True)
    p.set_adaptive(0)
    assert p.rows == 1
    for blk in blocks:
        hip.check(hip.lib.sdrhip_pipe_push_i16(p.h, np.ascontiguousarray(blk).ctypes.data_as(_i16p), B), "push")
    ready = hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush")
    assert ready == 4
    got = []
    for k in range(ready):
        if k % 2:
            got.append(p.pop_rows(1).reshape(-1))
        else:
            o = np.empty(2000, np.float32)
            assert hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(_f32p), 1000) == 1000
            got.append(o)
    assert_bit_equal(np.concatenate(got), one_row_expected(hip, t1[0], [B] * 4, 1000, s), "pop and pop_rows on a one-channel int16 bank")
    tables = tables_for(3)
    q = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), tables), 1000, input_i16=True)
    q.set_adaptive(0)
    for blk in blocks:
        hip.check(hip.lib.sdrhip_pipe_push_i16(q.h, np.ascontiguousarray(blk).ctypes.data_as(_i16p), B), "push")
    assert hip.check(hip.lib.sdrhip_pipe_flush(q.h), "flush") == 4
    o = np.full(3 * 8000, CANARY, np.uint32)
    assert hip.lib.sdrhip_pipe_pop(q.h, o.view(np.float32).ctypes.data_as(_f32p), 4000) == -1 and (o == CANARY).all()
    rows = q.pop_rows(4)
    assert rows.shape == (3, 4, 2000)
    for j, t in enumerate(tables):
        assert_bit_equal(rows[j].reshape(-1), one_row_expected(hip, t, [B] * 4, 1000, s), f"pop_rows: channel {j}")


# ---- 14 --------------------------------------------------------------------------------------------------------------------------
def test_channel_replay_s16(hip, tmp_path):
    exe = os.path.join(ROOT, "examples", "bin", "channel_replay")
    if not os.path.exists(exe):
        from sdr_amd import build as Bd
        Bd.build_examples()
    assert os.path.exists(exe)
    n = 6 * B + 1234                                     # six whole pushes and a ragged rest
    s = IC.stream_i16(PNBLK * B)[:2 * n]
    cap, tp = tmp_path / "capture.s16", tmp_path / "taps.f32"
    s.tofile(cap)
    S.taps_decim127().tofile(tp)
    r = subprocess.run([exe, str(cap), str(tp), str(tmp_path / "out"), "--channels", "1/4,-3/1000,0/1", "--block-out", "500", "--s16"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tables = [hip.tuner_shift_table(1, 4), hip.tuner_shift_table(-3, 1000), hip.tuner_shift_table(0, 1)]
    p = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), tables), 500, input_i16=True)
    p.set_adaptive(0)
    outs = []
    for blk in cut(s, [B] * 6 + [1234]):
        outs += p.push(blk)
    outs += p.flush()
    rows = np.concatenate(outs, axis=1)
    assert rows.shape == (3, ((n - LP) // D + 1) // 500 * 1000)
    for j in range(3):
        assert_bit_equal(np.fromfile(tmp_path / f"out.ch{j}.cf32", np.float32), rows[j], f"channel_replay --s16: channel {j}")
