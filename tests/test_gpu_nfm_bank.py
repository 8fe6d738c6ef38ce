"""GPU parity of the narrow-band FM bank (sdrhip_nfm_bank_*): fmDemod of every channel of one capture.  Rows are held to the models
(tests/nfm_bank_cases.py: the restated Pipe on the stream mixed with the channel's table, then oracle.fm_demod -- independent of the
product) and the three routes to each other.  Every comparison is bit for bit, NaN by position; every output buffer starts as NaN
canaries and every float between and around the rows is a canary still afterwards."""
import threading

import numpy as np
import pytest

import am_bank_cases as AC
import nfm_bank_cases as NC
import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, K_ALL, OUTS, ADV = NC.B, NC.K_ALL, NC.OUTS, NC.ADV
ROUTES = (1, 2, 0)


def device_inputs(oracle):
    u8 = T.stream_u8()
    return {"u8": to_dev(u8), "cf32": to_dev(oracle.convert_u8(u8)), "i16": to_dev(IC.stream_i16())}


def counters(hip):
    """[OUT_FM tile, OUT_FM cross, tuner bank, AM tile, AM fix-up, rows (fmDemod rows among them), int16]"""
    return np.array([hip.nfm_bank_launches(), hip.nfm_bank_cross_launches(), hip.tuner_bank_launches(), hip.am_bank_launches(),
                     hip.am_bank_fixup_launches(), hip.lib.sdrhip_debug_rows_launches(), hip.tuner_i16_launches()], np.int64)


def run_nfm(hip, nb, fmt, d_in, count, seam, cuts=(), k0=0, in_base=0, stride=None, base=0, state=None, stream=None, workspace=True):
    """Outputs [k0, k0 + count) of every channel as launches cut at k0 + cuts, the two state arrays swapped between the launches ->
    (rows [channels, count], final state [channels, 2]).  state None = a null d_state for the first launch.  Row j starts `base`
    floats + j * stride into a buffer of canaries; every float of it outside the rows must be a canary after the last launch."""
    import torch
    nch = nb.channels
    stride = count if stride is None else stride
    out = dev_empty_f32(base + nch * stride + 5)
    wsb = nb.workspace_bytes(count) if workspace else 0
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda") if workspace else None
    st = [to_dev(np.ascontiguousarray(np.zeros((nch, 2)) if state is None else state, np.float32).reshape(-1)), dev_empty_f32(2 * nch)]
    run = {"cf32": nb.run, "u8": nb.run_u8, "i16": nb.run_i16}[fmt]
    edges = [0] + [c for c in cuts if c < count] + [count]
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        first = None if (i == 0 and state is None) else ptr(st[i & 1])
        run(ptr(d_in), in_base, ptr(out) + 4 * (base + a), stride, k0 + a, k0 + b, seam, first, ptr(st[(i + 1) & 1]),
            ptr(ws) if workspace else None, wsb, stream)
    whole = to_host(out).view(np.uint32)                       # (checks the guard bands around the buffer)
    mask = np.zeros(whole.size, bool)
    for j in range(nch):
        mask[base + j * stride:base + j * stride + count] = True
    assert (whole[~mask] == CANARY).all(), f"{int((whole[~mask] != CANARY).sum())} floats between or around the rows were written"
    rows = np.stack([whole[base + j * stride:base + j * stride + count] for j in range(nch)]).view(np.float32)
    return rows, to_host(st[(len(edges) - 1) & 1]).reshape(nch, 2)


def tables_for(nch):
    """BC.bank_tables with the +-1 table among the channels ({1, 0} and the subnormal table are there already)."""
    ts = list(BC.bank_tables(nch))
    if nch >= 3:
        ts[0 if nch == 3 else 5] = NC.PM1
    return ts


# ---- 1: counts, channels, seams, factors, formats, routes, counters --------------------------------------------------------------
@pytest.mark.parametrize("factor", [8, 16])
@pytest.mark.parametrize("seam", [0, B, NC.LP], ids=["seam0", "seam8192", "seamLp"])
@pytest.mark.parametrize("nch", [1, 3, 32])
def test_counts_formats_and_routes_against_the_model(hip, oracle, nch, seam, factor):
    """Factor 16 with seam 8192: the tile (512 outputs x 16 samples) holds two seams.  seam = Lp: every output but one a block is Cross."""
    tables = tables_for(nch)
    nb = hip.NfmBank(hip.TunerBank(factor, S.taps_decim127(), tables))
    ins = device_inputs(oracle)
    n_all = NC.expected(oracle, tables[0], seam, "u8", factor).size
    first_cross = BC.straddlers(seam, n_all, NC.LP, factor)[0] if seam else 0
    k0 = int(first_cross)                                      # seamed runs start ON a Cross output: every count holds some
    for fmt in NC.FORMATS:
        exp = [NC.expected(oracle, t, seam, fmt, factor) for t in tables]
        st0 = [NC.state_before(oracle, t, seam, fmt, k0, factor) for t in tables]
        for count in NC.COUNTS:
            what = f"{len(tables)} channels, factor {factor}, seam {seam}, {fmt}, {count} outputs from {k0}"
            assert k0 + count <= n_all
            got = {}
            for route in ROUTES:
                nb.set_route(route)
                c0 = counters(hip)
                rows, fin = run_nfm(hip, nb, fmt, ins[fmt], count, seam, k0=k0, state=st0)
                d = counters(hip) - c0
                if route == 1:
                    assert d[0] == 1 and not d[1:6].any() and d[6] == int(fmt == "i16"), what + f": route 1 {d}"
                if route == 2:
                    assert d[0] == 0 and d[1] == 0 and d[5] >= 1 and d[3] == 0 and d[4] == 0, what + f": route 2 {d}"
                for j, t in enumerate(tables):
                    assert_bit_equal(rows[j], exp[j][k0:k0 + count], what + f", route {route}: channel {j}")
                    assert_bit_equal(fin[j], NC.state_before(oracle, t, seam, fmt, k0 + count, factor), what + f", route {route}: d_final {j}")
                got[route] = rows
            assert_bit_equal(got[1], got[2], what + ": route 1 against route 2")
            assert_bit_equal(got[0], got[2], what + ": route 0 against route 2")


# ---- 2: state and stream position -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
def test_cut_streams_equal_one_run(hip, oracle, seam):
    """The whole stream as three and as five runs cut at odd outputs, the state arrays swapped between runs, from a null state."""
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    ins = device_inputs(oracle)
    for fmt in NC.FORMATS:
        for route in (1, 2):
            nb.set_route(route)
            for cuts in ([], NC.ODD_CUTS3, NC.ODD_CUTS5):
                rows, fin = run_nfm(hip, nb, fmt, ins[fmt], K_ALL, seam, cuts)
                for j, t in enumerate(tables):
                    what = f"{fmt}, seam {seam}, route {route}, cuts {cuts}: channel {j}"
                    assert_bit_equal(rows[j], NC.expected(oracle, t, seam, fmt), what)
                    assert_bit_equal(fin[j], NC.state_before(oracle, t, seam, fmt, K_ALL), what + " d_final")


def test_a_non_zero_starting_state(hip, oracle):
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    d_in = device_inputs(oracle)["u8"]
    state = np.array([[0.25, -0.5], [-3.0, 0.0], [0.0, 7.5]], np.float32)
    for route in ROUTES:
        nb.set_route(route)
        rows, _ = run_nfm(hip, nb, "u8", d_in, OUTS + 1, B, state=state)
        for j, t in enumerate(tables):
            e = NC.demod(oracle, NC.expected_iq(oracle, t, B, "u8")[:2 * (OUTS + 1)], state[j])
            assert_bit_equal(rows[j], e, f"route {route}: channel {j} from {state[j]}")


def test_negative_zero_states_on_a_silent_start(hip, oracle):
    """States of -0 in front of the directed stream's silent start: zeros of both signs under `phase 0 = 0` (the one way a -0 reaches
    the demodulator: a FIR sum cannot yield it), and in front of the seeded stream: a non-zero output on a signed-zero predecessor."""
    tables = NC.directed_tables()
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    state = np.array([[-0.0, -0.0], [0.0, -0.0], [-0.0, 0.0]], np.float32)
    assert np.signbit(state).sum() == 4
    for name, d_in in (("directed", to_dev(NC.directed_u8())), ("seeded", device_inputs(oracle)["u8"])):
        for route in ROUTES:
            nb.set_route(route)
            rows, _ = run_nfm(hip, nb, "u8", d_in, OUTS + 1, 0, state=state)
            for j, t in enumerate(tables):
                e = NC.demod(oracle, NC.expected_iq(oracle, t, 0, "u8", stream=name)[:2 * (OUTS + 1)], state[j])
                assert_bit_equal(rows[j], e, f"{name} stream, route {route}: channel {j} from {state[j]}")


def test_far_stream_position(hip, oracle):
    """k_begin = 3 * 2^30 + 5 and in_base = 8 k_begin, periods 1000 and 5 in one bank; the device holds only the slice."""
    k_begin, in_base = BC.FAR_K0, 8 * BC.FAR_K0
    ns = 3 * B - 40
    u8 = T.stream_u8()[:2 * ns]
    tables = [T.osc_table(1000), T.osc_table(5)]
    iq = [TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, oracle.convert_u8(u8), t, B, in_base, block_out=1) for t in tables]
    state = np.array([[0.25, -0.5], [1.5, 2.0]], np.float32)
    exp = [NC.demod(oracle, q, s) for q, s in zip(iq, state)]
    n_out = exp[0].size
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    for fmt, d_in in (("u8", to_dev(u8)), ("cf32", to_dev(oracle.convert_u8(u8)))):
        for route in ROUTES:
            nb.set_route(route)
            for cuts in ([], BC.FAR_CUTS):
                rows, fin = run_nfm(hip, nb, fmt, d_in, n_out, B, cuts, k0=k_begin, in_base=in_base, state=state)
                for j in range(2):
                    assert_bit_equal(rows[j], exp[j], f"{fmt}, route {route}, cuts {cuts}: channel {j}")
                    assert_bit_equal(fin[j], iq[j][-2:], f"{fmt}, route {route}, cuts {cuts}: d_final {j}")


# ---- 3: rows and addresses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1, 2, 3])
@pytest.mark.parametrize("extra", [0, 1, 3])
def test_odd_cuts_strides_and_bases(hip, oracle, extra, base):
    """Rows count, count + 1 and count + 3 floats apart (count = 5105 is odd), bases 0 / 4 / 8 / 12 bytes past a 16-byte boundary."""
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    ins = device_inputs(oracle)
    for fmt in NC.FORMATS:
        for route in (1, 2):
            nb.set_route(route)
            for cuts in ([], NC.ODD_CUTS5):
                what = f"{fmt}, route {route}, stride n + {extra}, base {4 * base} bytes, cuts {cuts}"
                rows, _ = run_nfm(hip, nb, fmt, ins[fmt], K_ALL, B, cuts, stride=K_ALL + extra, base=base)
                for j, t in enumerate(tables):
                    assert_bit_equal(rows[j], NC.expected(oracle, t, B, fmt), what + f": channel {j}")


def test_a_neighbour_row_of_nan(hip, oracle):
    """Three rows written between two rows that hold NaN, with no gap (count = OUTS + 1 is odd)."""
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    nb.set_route(1)
    d_in = device_inputs(oracle)["u8"]
    n = OUTS + 1
    out = dev_empty_f32(5 * n)
    out[:] = float("nan")                                      # rows 0 and 4 are neighbours of NaN; rows 1 .. 3 are written
    nb.run_u8(ptr(d_in), 0, ptr(out) + 4 * n, n, 0, n, B)
    got = to_host(out).reshape(5, n)
    assert np.isnan(got[0]).all() and np.isnan(got[4]).all()
    for j, t in enumerate(tables):
        assert_bit_equal(got[1 + j], NC.expected(oracle, t, B, "u8")[:n], f"channel {j} beside NaN rows")


def test_auto_falls_back_where_a_launch_is_not_aligned(hip, oracle):
    """cfloat input 4 bytes past a 16-byte boundary: route 1 refuses and writes nothing, auto runs it composed, same bits."""
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    x = oracle.convert_u8(T.stream_u8())
    shifted = to_dev(np.concatenate([np.zeros(1, np.float32), x]))
    d_off = shifted[1:]
    assert ptr(d_off) % 16 == 4
    n = 1100
    nb.set_route(1)
    out, fin = dev_empty_f32(3 * n), dev_empty_f32(6)
    c0 = counters(hip)
    with pytest.raises(hip.SdrHipError):
        nb.run(ptr(d_off), 0, ptr(out), n, 0, n, B, None, ptr(fin))
    assert (to_host(out).view(np.uint32) == CANARY).all() and (to_host(fin).view(np.uint32) == CANARY).all(), "a refused run wrote"
    nb.set_route(0)
    rows, _ = run_nfm(hip, nb, "cf32", d_off, n, B)
    d = counters(hip) - c0
    assert d[0] == 0 and d[5] >= 1, "auto took the fused route on an input it does not fit"
    for j, t in enumerate(tables):
        assert_bit_equal(rows[j], NC.expected(oracle, t, B, "cf32")[:n], f"fallback: channel {j}")


def test_the_edges_of_the_auto_rule(hip, oracle):
    """Auto takes the fused launch exactly in the ranges read from profiles/nfm_bank_bench.txt (sdr_hip.h states them), with n =
    (count - 1) * factor + 128 input samples; the same bits on both sides of each edge."""
    import torch
    big = torch.randint(0, 256, (2 * ((1 << 20) + 16 + 128),), dtype=torch.uint8, device="cuda")
    t32 = BC.bank_tables(32)
    # (factor, channels, seam_block, n, fused)
    points = [(8, 1, 0, 8192, 1), (8, 32, 0, 1 << 20, 1), (8, 3, B, 1 << 20, 1), (8, 3, B, (1 << 20) + 8, 0), (8, 1, B, (1 << 20) + 8, 1),
              (8, 3, 4096, 8192, 0), (8, 3, 2 * B, 1 << 17, 1),
              (16, 2, 0, 1 << 20, 1), (16, 8, 0, 1 << 17, 1), (16, 8, 0, (1 << 17) + 16, 0), (16, 3, 0, (1 << 17) + 16, 0), (16, 32, 0, 8192, 1),
              (16, 32, 0, 8192 + 16, 0), (16, 9, 0, 8192 + 16, 0),
              (16, 1, B, 8192, 0), (16, 1, B, (1 << 17) - 16, 0), (16, 1, B, 1 << 17, 1), (16, 8, B, 1 << 20, 1), (16, 8, B, (1 << 20) + 16, 0),
              (16, 32, B, 1 << 17, 1), (16, 32, B, (1 << 17) + 16, 0), (16, 9, B, 1 << 20, 0),
              (4, 1, 0, 8192, 0)]
    for factor, nch, seam, n, fused in points:
        n_out = (n - 128) // factor + 1
        assert (n_out - 1) * factor + 128 == n
        nb = hip.NfmBank(hip.TunerBank(factor, S.taps_decim127(), t32[:nch]))
        ws = torch.empty(nb.workspace_bytes(n_out), dtype=torch.uint8, device="cuda")
        out, ref = (torch.zeros(nch * n_out, dtype=torch.float32, device="cuda") for _ in range(2))
        fin = [torch.zeros(2 * nch, dtype=torch.float32, device="cuda") for _ in range(2)]
        what = f"factor {factor}, {nch} channels, seam {seam}, {n} samples"
        c0 = counters(hip)
        nb.run_u8(ptr(big), 0, ptr(out), n_out, 0, n_out, seam, None, ptr(fin[0]), ptr(ws), ws.numel())
        assert (counters(hip) - c0)[0] == fused, what + ": auto took the other route"
        nb.set_route(2 if fused else 1)
        nb.run_u8(ptr(big), 0, ptr(ref), n_out, 0, n_out, seam, None, ptr(fin[1]), ptr(ws), ws.numel())
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), what + ": the two routes differ"
        assert torch.equal(fin[0].view(torch.int32), fin[1].view(torch.int32)), what + ": d_final differs"


# ---- 4: value classes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [0, B])
def test_silent_and_constant_stretches(hip, oracle, seam):
    """The directed stream: all-zero windows at the launch's start (zero state) and across a tile edge -- phase(0) with both zero
    signs -- and a constant stretch under the +-1 table across the next tile edge: exact +pi and -pi, also as a launch's first output."""
    tables = NC.directed_tables()
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    d_in = to_dev(NC.directed_u8())
    k_pi = int(NC.inside(NC.CONST)[3])                         # a launch that starts inside the constant stretch
    for route in ROUTES:
        nb.set_route(route)
        rows, _ = run_nfm(hip, nb, "u8", d_in, K_ALL, seam, [k_pi, k_pi + 1])
        for j, t in enumerate(tables):
            assert_bit_equal(rows[j], NC.expected(oracle, t, seam, "u8", stream="directed"), f"seam {seam}, route {route}: channel {j}")


def test_inf_and_nan_samples(hip, oracle):
    tables = [T.osc_table(1000), BC.IDENTITY, T.osc_table(5)]
    d_in = to_dev(AC.nonfinite_stream(oracle))
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    for route in ROUTES:
        nb.set_route(route)
        rows, _ = run_nfm(hip, nb, "cf32", d_in, K_ALL, B, [1009])
        for j, t in enumerate(tables):
            e = NC.nonfinite_expected(oracle, t, B)[1]
            nan = np.isnan(e)
            assert np.array_equal(np.isnan(rows[j]), nan), f"route {route}: channel {j}: NaN positions"
            assert_bit_equal(rows[j][~nan], e[~nan], f"route {route}: channel {j}")


# ---- 5: refusals and edges --------------------------------------------------------------------------------------------------------
def test_run_time_refusals_write_nothing(hip, oracle):
    import torch
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables_for(3)))
    d_in = device_inputs(oracle)["u8"]
    n = 64
    ws = torch.empty(nb.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = to_dev(np.full(12, 0.5, np.float32))                  # two arrays of 3 pairs back to back
    c0 = counters(hip)
    for route in ROUTES:
        nb.set_route(route)
        out = dev_empty_f32(3 * n)

        def refused(what, *args):
            assert hip.lib.sdrhip_nfm_bank_run_u8(nb.h, None, *args) == -1, f"route {route}: {what}"
            assert b"sdrhip_nfm_bank_run" in hip.lib.sdrhip_last_error(), what
            assert (to_host(out).view(np.uint32) == CANARY).all() and (to_host(st) == 0.5).all(), f"route {route}: {what}: a refused run wrote"

        ok = (ptr(ws), ws.numel())
        refused("the same state array twice", ptr(d_in), 0, ptr(out), n, 0, n, 0, ptr(st), ptr(st), *ok)
        refused("state arrays one pair apart", ptr(d_in), 0, ptr(out), n, 0, n, 0, ptr(st), ptr(st) + 8, *ok)
        refused("d_final five floats in front of d_state", ptr(d_in), 0, ptr(out), n, 0, n, 0, ptr(st) + 20, ptr(st), *ok)
        refused("rows would overlap", ptr(d_in), 0, ptr(out), n - 1, 0, n, 0, ptr(st), ptr(st) + 24, *ok)
        refused("a seam block shorter than the filter", ptr(d_in), 0, ptr(out), n, 0, n, 127, ptr(st), ptr(st) + 24, *ok)
        refused("the first window before d_in", ptr(d_in), 8, ptr(out), n, 0, n, 0, ptr(st), ptr(st) + 24, *ok)
        if route != 1:
            refused("a short workspace", ptr(d_in), 0, ptr(out), n, 0, n, 0, ptr(st), ptr(st) + 24, ptr(ws), 15)
    assert (counters(hip) == c0).all()


def test_an_empty_range_copies_the_state(hip, oracle):
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables_for(3)))
    d_in = device_inputs(oracle)["u8"]
    st = to_dev(np.arange(6, dtype=np.float32) + 0.5)
    for route in ROUTES:
        nb.set_route(route)
        c0 = counters(hip)
        out, fin = dev_empty_f32(8), dev_empty_f32(6)
        nb.run_u8(ptr(d_in), 0, ptr(out), 1, 7, 7, B, ptr(st), ptr(fin))
        assert_bit_equal(to_host(fin), to_host(st), f"route {route}: d_final of an empty range")
        nb.run_u8(ptr(d_in), 0, ptr(out), 1, 7, 7, B, None, ptr(fin))
        assert_bit_equal(to_host(fin), np.zeros(6, np.float32), f"route {route}: d_final of an empty range from a null state")
        assert (to_host(out).view(np.uint32) == CANARY).all()
        assert not (counters(hip) - c0)[:2].any()


# ---- 6: concurrency and follow-on stages ------------------------------------------------------------------------------------------
def test_one_bank_two_host_threads(hip, oracle):
    """One bank, two host threads, each with a stream, a pair of state arrays and a workspace of its own."""
    import torch
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    d_u8 = device_inputs(oracle)["u8"]
    for route in (1, 2):
        nb.set_route(route)
        outs = [dev_empty_f32(3 * K_ALL) for _ in range(2)]
        states = [[torch.zeros(6, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(2)]
        wss = [torch.empty(nb.workspace_bytes(K_ALL), dtype=torch.uint8, device="cuda") for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        errors = []
        torch.cuda.synchronize()

        def work(i):
            try:
                for rep in range(3):
                    edges = [0] + [c + i for c in NC.ODD_CUTS5] + [K_ALL]
                    for q, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                        nb.run_u8(ptr(d_u8), 0, ptr(outs[i]) + 4 * a, K_ALL, a, b, B, None if q == 0 else ptr(states[i][q & 1]),
                                  ptr(states[i][(q + 1) & 1]), ptr(wss[i]), wss[i].numel(), stream=streams[i].cuda_stream)
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
            rows = to_host(outs[i]).reshape(3, K_ALL)
            for j, t in enumerate(tables):
                assert_bit_equal(rows[j], NC.expected(oracle, t, B, "u8"), f"route {route}, thread {i}, channel {j}")
                assert_bit_equal(to_host(states[i][5 & 1]).reshape(3, 2)[j], NC.state_before(oracle, t, B, "u8", K_ALL), f"thread {i}, d_final {j}")


def test_follow_on_stages_on_one_stream(hip, oracle):
    """NfmBank.run -> Resampler.run_rows -> Filter.run_rows for three channels on one stream without synchronisation, against the same
    stages on the model's rows, row by row."""
    import torch
    tables = tables_for(3)
    nb = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), tables))
    nb.set_route(1)
    rs = hip.Resampler(3, 10, S.gauss_taps(60, 7))
    fl = hip.Filter(S.gauss_taps(32, 9))
    n = K_ALL
    n_r = ((n - rs.num_coeffs - 10) * 3) // 10
    n_f = n_r - fl.num_coeffs + 1
    d_u8 = device_inputs(oracle)["u8"]
    stream = torch.cuda.Stream()
    audio, res, fin = dev_empty_f32(3 * n), dev_empty_f32(3 * n_r), dev_empty_f32(3 * n_f)
    torch.cuda.synchronize()
    s = stream.cuda_stream
    nb.run_u8(ptr(d_u8), 0, ptr(audio), n, 0, n, B, stream=s)
    rs.run_rows(ptr(audio), ptr(res), 0, n_r, stream=s, in_stride=n, out_stride=n_r, rows=3)
    fl.run_rows(ptr(res), ptr(fin), 0, n_f, stream=s, in_stride=n_r, out_stride=n_f, rows=3)
    stream.synchronize()
    got = to_host(fin).reshape(3, n_f)
    for j, t in enumerate(tables):
        a = to_dev(NC.expected(oracle, t, B, "u8"))
        r1, f1 = dev_empty_f32(n_r), dev_empty_f32(n_f)
        rs.run(ptr(a), 0, ptr(r1), 0, n_r, 0)
        fl.run(ptr(r1), 0, ptr(f1), 0, n_f, 0)
        assert_bit_equal(got[j], to_host(f1), f"channel {j} through resampler and filter")
