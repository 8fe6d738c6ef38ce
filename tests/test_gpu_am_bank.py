"""GPU parity of the AM bank (sdrhip_am_bank_*): every channel's envelope, and its dcBlocker, from one capture.  Rows are held to the
models (tests/am_bank_cases.py: the restated Pipe on the stream mixed with the channel's table, Data.Complex.magnitude, the oracle's
dcBlocker -- independent of the product) and the three routes to each other.  Every comparison is bit for bit, NaN by position; every
output buffer starts as NaN canaries and every float between and around the rows is a canary still afterwards."""
import threading

import numpy as np
import pytest

import am_bank_cases as AC
import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, K_ALL, OUTS = AC.B, AC.K_ALL, AC.OUTS
launch_route = T.launch_route                  # Cross outputs in the tile kernel / tile kernel + fix-up launch
ROUTES = (1, 2, 0)


def device_inputs(oracle):
    u8 = T.stream_u8()
    return {"u8": to_dev(u8), "cf32": to_dev(oracle.convert_u8(u8)), "i16": to_dev(IC.stream_i16())}


def counters(hip):
    return np.array([hip.am_bank_launches(), hip.am_bank_fixup_launches(), hip.lib.sdrhip_debug_am_demod_launches(),
                     hip.tuner_bank_launches(), hip.tuner_i16_launches()], np.int64)


def run_am(hip, am, fmt, d_in, count, seam, cuts=(), k0=0, in_base=0, stride=None, base=0, state=None, stream=None, workspace=True):
    """Outputs [k0, k0 + count) of every channel as launches cut at k0 + cuts -> (rows [channels, count], final state [channels, 2]).
    Row j starts `base` floats (0 .. 3: 0 / 4 / 8 / 12 bytes past a 16-byte boundary) + j * stride into a buffer of canaries; every
    float of it outside the rows must be a canary after the last launch."""
    import torch
    nch = am.channels
    stride = count if stride is None else stride
    out = dev_empty_f32(base + nch * stride + 5)
    wsb = am.workspace_bytes(count) if workspace else 0
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda") if workspace else None
    st = to_dev(np.ascontiguousarray(state, np.float32).reshape(-1)) if am.dc_block else None
    run = {"cf32": am.run, "u8": am.run_u8, "i16": am.run_i16}[fmt]
    edges = [0] + [c for c in cuts if c < count] + [count]
    for a, b in zip(edges[:-1], edges[1:]):
        run(ptr(d_in), in_base, ptr(out) + 4 * (base + a), stride, k0 + a, k0 + b, seam, ptr(st) if am.dc_block else None,
            ptr(ws) if workspace else None, wsb, stream)
    whole = to_host(out).view(np.uint32)                       # (checks the guard bands around the buffer)
    mask = np.zeros(whole.size, bool)
    for j in range(nch):
        mask[base + j * stride:base + j * stride + count] = True
    assert (whole[~mask] == CANARY).all(), f"{int((whole[~mask] != CANARY).sum())} floats between or around the rows were written"
    rows = np.stack([whole[base + j * stride:base + j * stride + count] for j in range(nch)]).view(np.float32)
    return rows, (to_host(st).reshape(nch, 2) if am.dc_block else None)


# ---- 1: counts, channels, seams, formats, routes, counters -------------------------------------------------------------------------
@pytest.mark.parametrize("dc", [False, True], ids=["envelope", "dc_block"])
@pytest.mark.parametrize("seam", [0, B])
@pytest.mark.parametrize("nch", [1, 3, 32])
def test_counts_formats_and_routes_against_the_model(hip, oracle, nch, seam, dc, launch_route):
    tables = BC.bank_tables(nch)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=dc)
    ins = device_inputs(oracle)
    k0 = AC.K0_CROSS if seam else 0                            # seamed runs start ON a Cross output: every count holds some
    fixup = seam != 0 and launch_route.startswith("tile")
    for fmt in AC.FORMATS:
        exp = [AC.expected(oracle, t, seam, fmt, dc) for t in tables]
        st0 = [AC.state_before(oracle, t, seam, fmt, k0) for t in tables]
        for count in AC.COUNTS:
            what = f"{nch} channels, seam {seam}, {fmt}, {count} outputs from {k0}"
            got = {}
            for route in ROUTES:
                am.set_route(route)
                c0 = counters(hip)
                rows, fin = run_am(hip, am, fmt, ins[fmt], count, seam, k0=k0, state=st0)
                d = counters(hip) - c0
                if route == 1:
                    assert d[0] == 1 and d[1] == int(fixup) and d[2] == 0 and d[3] == 0 and d[4] == int(fmt == "i16"), what + f": route 1 {d}"
                if route == 2:
                    # (the tuner bank under ITS auto rule: banked from 2 channels on, one channel goes to its tuner)
                    assert d[0] == 0 and d[1] == 0 and d[2] == 1 and d[3] == int(nch >= 2), what + f": route 2 {d}"
                for j in range(nch):
                    assert_bit_equal(rows[j], exp[j][k0:k0 + count], what + f", route {route}: channel {j}")
                    if dc:
                        assert_bit_equal(fin[j], AC.state_before(oracle, tables[j], seam, fmt, k0 + count), what + f", route {route}: state {j}")
                got[route] = rows
            assert_bit_equal(got[1], got[2], what + ": route 1 against route 2")
            assert_bit_equal(got[0], got[2], what + ": route 0 against route 2")


# ---- 2: other factors and tap counts ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,ntaps", [(4, 127), (16, 127), (8, 64)])
def test_other_factors_and_the_64_tap_bank(hip, oracle, factor, ntaps, launch_route):
    """The factor-4, factor-16 and 64-tap banks of the tuner bank's tests: 3 blocks of 4096 samples, periods 5 and 1000."""
    nb, blk = 3, 4096
    u8 = T.stream_u8()[:2 * nb * blk]
    taps = S.taps_decim127() if ntaps == 127 else S.gauss_taps(ntaps, 40 + ntaps)
    tables = [T.osc_table(5), T.osc_table(1000)]
    x = oracle.convert_u8(u8)
    env = [AC.envelope(TM.tuner_expected(oracle, taps, PM.ORDER_AVX, factor, x, t, blk, 0, block_out=1)) for t in tables]
    n_out = env[0].size
    am = hip.AmBank(hip.TunerBank(factor, taps, tables), dc_block=True)
    audio = [oracle.dc_blocker(e, 0.0, 0.0) for e in env]
    for fmt, d_in in (("u8", to_dev(u8)), ("cf32", to_dev(x))):
        for route in ROUTES:
            am.set_route(route)
            # odd cuts wherever the launch they start stays 16-byte aligned: u8 at factor 4 moves 8 bytes per output
            for cuts in ([], [64, 500] if (fmt, factor) == ("u8", 4) else [63, 501]):
                c0 = counters(hip)
                rows, fin = run_am(hip, am, fmt, d_in, n_out, blk, cuts, state=np.zeros((2, 2)))
                if route == 1:
                    assert (counters(hip) - c0)[0] == len(cuts) + 1
                for j in range(2):
                    what = f"factor {factor}, {ntaps} taps, {fmt}, route {route}, cuts {cuts}: channel {j}"
                    assert_bit_equal(rows[j], audio[j][0], what)
                    assert_bit_equal(fin[j], np.array(audio[j][1:], np.float32), what + " state")


# ---- 3: cuts, strides, bases ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [0, 1, 2, 3])
@pytest.mark.parametrize("extra", [0, 1, 3])
def test_odd_cuts_strides_and_bases(hip, oracle, extra, base, launch_route):
    """Rows count, count + 1 and count + 3 floats apart (count = 5105 is odd: the last thread's pair is cut, and with no gap every odd
    row starts 4 bytes off 8-byte alignment), bases 0 / 4 / 8 / 12 bytes past a 16-byte boundary, launches cut at odd outputs.  Three
    consecutive runs on one state array are one run: the final state is the model's for every channel."""
    tables = BC.bank_tables(3)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=True)
    plain = hip.AmBank(am.tuner_bank, dc_block=False)
    ins = device_inputs(oracle)
    for fmt in AC.FORMATS:
        for route in (1, 2):
            for bank, dc in ((am, True), (plain, False)):
                bank.set_route(route)
                for cuts in ([], AC.ODD_CUTS[:2], AC.ODD_CUTS):
                    what = f"{fmt}, route {route}, dc {dc}, stride n + {extra}, base {4 * base} bytes, cuts {cuts}"
                    rows, fin = run_am(hip, bank, fmt, ins[fmt], K_ALL, B, cuts, stride=K_ALL + extra, base=base, state=np.zeros((3, 2)))
                    for j, t in enumerate(tables):
                        assert_bit_equal(rows[j], AC.expected(oracle, t, B, fmt, dc), what + f": channel {j}")
                        if dc:
                            assert_bit_equal(fin[j], AC.state_before(oracle, t, B, fmt, K_ALL), what + f": final state {j}")


def test_a_neighbour_row_of_nan(hip, oracle):
    """Three rows written between two rows that hold NaN, with no gap (count = OUTS + 1 is odd, so rows alternate between 8-byte
    aligned and 4 bytes off): the NaN rows stay NaN and the written rows are the model's."""
    tables = BC.bank_tables(3)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=False)
    am.set_route(1)
    d_in = device_inputs(oracle)["u8"]
    n = OUTS + 1
    out = dev_empty_f32(5 * n)
    out[:] = float("nan")                                      # rows 0 and 4 are neighbours of NaN; rows 1 .. 3 are written
    am.run_u8(ptr(d_in), 0, ptr(out) + 4 * n, n, 0, n, B)
    got = to_host(out).reshape(5, n)
    assert np.isnan(got[0]).all() and np.isnan(got[4]).all()
    for j, t in enumerate(tables):
        assert_bit_equal(got[1 + j], AC.expected(oracle, t, B, "u8", False)[:n], f"channel {j} beside NaN rows")


# ---- 4: far positions -------------------------------------------------------------------------------------------------------------
def test_far_stream_position(hip, oracle, launch_route):
    """k_begin = 3 * 2^30 + 5 and in_base = 8 k_begin, periods 1000 and 5 in one bank; the device holds only the slice."""
    k_begin, in_base = BC.FAR_K0, 8 * BC.FAR_K0
    ns = 3 * B - 40
    u8 = T.stream_u8()[:2 * ns]
    tables = [T.osc_table(1000), T.osc_table(5)]
    env = [AC.envelope(TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, oracle.convert_u8(u8), t, B, in_base, block_out=1))
           for t in tables]
    audio = [oracle.dc_blocker(e, 0.25, -0.5) for e in env]
    n_out = env[0].size
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=True)
    for fmt, d_in in (("u8", to_dev(u8)), ("cf32", to_dev(oracle.convert_u8(u8)))):
        for route in ROUTES:
            am.set_route(route)
            for cuts in ([], BC.FAR_CUTS):
                rows, fin = run_am(hip, am, fmt, d_in, n_out, B, cuts, k0=k_begin, in_base=in_base, state=[[0.25, -0.5]] * 2)
                for j in range(2):
                    assert_bit_equal(rows[j], audio[j][0], f"{fmt}, route {route}, cuts {cuts}: channel {j}")
                    assert_bit_equal(fin[j], np.array(audio[j][1:], np.float32), f"{fmt}, route {route}, cuts {cuts}: state {j}")


# ---- 5: value classes -------------------------------------------------------------------------------------------------------------
def test_subnormal_and_signed_zero_envelopes(hip, oracle, launch_route):
    tables = BC.bank_tables(3)
    assert tables[2] is BC.SUBNORMALS
    d_in = to_dev(AC.sparse_stream())
    exp = [AC.envelope(AC.sparse_expected_iq(oracle, t, B)) for t in tables]
    for dc in (False, True):
        am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=dc)
        for route in ROUTES:
            am.set_route(route)
            rows, _ = run_am(hip, am, "cf32", d_in, AC.SPARSE_OUT, B, [1, 700], state=np.zeros((3, 2)))
            for j in range(3):
                e = oracle.dc_blocker(exp[j], 0.0, 0.0)[0] if dc else exp[j]
                assert_bit_equal(rows[j], e, f"sparse stream, dc {dc}, route {route}: channel {j}")


def test_inf_and_nan_samples(hip, oracle, launch_route):
    tables = [T.osc_table(1000), BC.IDENTITY, T.osc_table(5)]
    d_in = to_dev(AC.nonfinite_stream(oracle))
    for dc in (False, True):
        am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=dc)
        for route in ROUTES:
            am.set_route(route)
            rows, _ = run_am(hip, am, "cf32", d_in, K_ALL, B, [1009], state=np.zeros((3, 2)))
            for j, t in enumerate(tables):
                e = AC.nonfinite_expected(oracle, t, B, dc)
                nan = np.isnan(e)
                assert np.array_equal(np.isnan(rows[j]), nan), f"dc {dc}, route {route}: channel {j}: NaN positions"
                assert_bit_equal(rows[j][~nan], e[~nan], f"dc {dc}, route {route}: channel {j}")


# ---- 6: no dcBlocker, no workspace; fallback; refusals ---------------------------------------------------------------------------
def test_route_1_without_dc_block_takes_no_state_and_no_workspace(hip, oracle):
    tables = BC.bank_tables(3)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=False)
    am.set_route(1)
    rows, _ = run_am(hip, am, "u8", device_inputs(oracle)["u8"], K_ALL, B, AC.ODD_CUTS, workspace=False)
    for j, t in enumerate(tables):
        assert_bit_equal(rows[j], AC.expected_env(oracle, t, B, "u8"), f"channel {j}")


def test_auto_falls_back_where_a_launch_is_not_aligned(hip, oracle):
    """cfloat input 4 bytes past a 16-byte boundary: route 1 refuses and writes nothing, auto runs it composed, same bits as the
    aligned copy."""
    tables = BC.bank_tables(3)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=True)
    x = oracle.convert_u8(T.stream_u8())
    shifted = to_dev(np.concatenate([np.zeros(1, np.float32), x]))
    d_off = shifted[1:]
    assert ptr(d_off) % 16 == 4
    n = 1100
    am.set_route(1)
    out = dev_empty_f32(3 * n)
    import torch
    ws = torch.empty(am.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = to_dev(np.zeros(6, np.float32))
    c0 = counters(hip)
    with pytest.raises(hip.SdrHipError):
        am.run(ptr(d_off), 0, ptr(out), n, 0, n, B, ptr(st), ptr(ws), ws.numel())
    assert (to_host(out).view(np.uint32) == CANARY).all() and (to_host(st) == 0).all(), "a refused run wrote"
    am.set_route(0)
    rows, _ = run_am(hip, am, "cf32", d_off, n, B, state=np.zeros((3, 2)))
    d = counters(hip) - c0
    assert d[0] == 0 and d[2] == 1, "auto took the fused route on an input it does not fit"
    for j, t in enumerate(tables):
        assert_bit_equal(rows[j], AC.expected_audio(oracle, t, B, "cf32")[0][:n], f"fallback: channel {j}")


def test_the_edges_of_the_auto_rule(hip, oracle):
    """Auto is fused for any channel count without dcBlocker; with it from 8 channels on, for one channel from the measured 2^20
    launch on and for two channels from the measured 2^24 launch on; always up to 2^24 input samples per launch (the points of
    profiles/am_bank_bench.txt where the fused route was ahead).  The same bits on both sides of each edge."""
    import torch
    d_u8 = device_inputs(oracle)["u8"]
    for nch, dc, fused in ((1, False, 1), (3, False, 1), (1, True, 0), (3, True, 0), (7, True, 0), (8, True, 1), (32, True, 1)):
        tables = BC.bank_tables(nch) if nch in (1, 3, 32) else BC.bank_tables(32)[:nch]
        am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=dc)
        c0 = counters(hip)
        rows, _ = run_am(hip, am, "u8", d_u8, K_ALL, B, state=np.zeros((nch, 2)))
        d = counters(hip) - c0
        assert d[0] == fused and d[2] == 1 - fused, f"{nch} channels, dc_block {dc}: auto took the other route"
        for j, t in enumerate(tables):
            assert_bit_equal(rows[j], AC.expected(oracle, t, B, "u8", dc), f"{nch} channels, dc_block {dc} under auto: channel {j}")
    edge = (1 << 24) // 8
    big = torch.randint(0, 256, (2 * (8 * edge + 128),), dtype=torch.uint8, device="cuda")
    two = [T.osc_table(1000), T.osc_table(5)]
    # (channels, dc_block, outputs, fused): 2^24 samples is the rectangle's edge; with dcBlocker one channel is fused from the measured
    # 2^20 launch (131057 outputs) on and two channels from the measured 2^24 launch (2097137 outputs) on
    for nch, dc, n_out, fused in ((2, False, edge, 1), (2, False, edge + 1, 0), (1, True, 131056, 0), (1, True, 131057, 1), (1, True, edge + 1, 0),
                                  (2, True, 2097136, 0), (2, True, 2097137, 1)):
        am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), two[:nch]), dc_block=dc)
        ws = torch.empty(am.workspace_bytes(n_out), dtype=torch.uint8, device="cuda")
        out, ref = (torch.zeros(nch * n_out, dtype=torch.float32, device="cuda") for _ in range(2))
        st = [torch.zeros(2 * nch, dtype=torch.float32, device="cuda") for _ in range(2)]
        am.set_route(0)
        c0 = counters(hip)
        am.run_u8(ptr(big), 0, ptr(out), n_out, 0, n_out, B, ptr(st[0]) if dc else None, ptr(ws), ws.numel())
        assert (counters(hip) - c0)[0] == fused, f"{n_out} outputs of {nch} channels, dc_block {dc}, under auto"
        am.set_route(2 if fused else 1)
        am.run_u8(ptr(big), 0, ptr(ref), n_out, 0, n_out, B, ptr(st[1]) if dc else None, ptr(ws), ws.numel())
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), f"{n_out} outputs x {nch}, dc_block {dc}: the two routes differ"
        assert torch.equal(st[0].view(torch.int32), st[1].view(torch.int32))


def test_run_time_refusals_write_nothing(hip, oracle):
    import torch
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), BC.bank_tables(3)), dc_block=True)
    d_in = device_inputs(oracle)["u8"]
    n = 64
    ws = torch.empty(am.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = to_dev(np.full(6, 0.5, np.float32))
    c0 = counters(hip)
    for route in ROUTES:
        am.set_route(route)
        out = dev_empty_f32(3 * n)

        def refused(what, *args):
            assert hip.lib.sdrhip_am_bank_run_u8(am.h, None, *args) == -1, f"route {route}: {what}"
            assert b"sdrhip_am_bank_run" in hip.lib.sdrhip_last_error(), what
            assert (to_host(out).view(np.uint32) == CANARY).all() and (to_host(st) == 0.5).all(), f"route {route}: {what}: a refused run wrote"

        refused("rows would overlap", ptr(d_in), 0, ptr(out), n - 1, 0, n, 0, ptr(st), ptr(ws), ws.numel())
        refused("a null state", ptr(d_in), 0, ptr(out), n, 0, n, 0, None, ptr(ws), ws.numel())
        refused("a short workspace", ptr(d_in), 0, ptr(out), n, 0, n, 0, ptr(st), ptr(ws), 15)
        refused("a seam block shorter than the filter", ptr(d_in), 0, ptr(out), n, 0, n, 127, ptr(st), ptr(ws), ws.numel())
        refused("the first window before d_in", ptr(d_in), 8, ptr(out), n, 0, n, 0, ptr(st), ptr(ws), ws.numel())
    assert (counters(hip) == c0).all()


# ---- 7: concurrency and follow-on stages ------------------------------------------------------------------------------------------
def test_one_bank_two_host_threads(hip, oracle):
    """One bank, two host threads, each with a stream, a state array and a workspace of its own."""
    import torch
    tables = BC.bank_tables(3)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=True)
    d_u8 = device_inputs(oracle)["u8"]
    for route in (1, 2):
        am.set_route(route)
        outs = [dev_empty_f32(3 * K_ALL) for _ in range(2)]
        states = [torch.zeros(6, dtype=torch.float32, device="cuda") for _ in range(2)]
        wss = [torch.empty(am.workspace_bytes(K_ALL), dtype=torch.uint8, device="cuda") for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        errors = []
        torch.cuda.synchronize()

        def work(i):
            try:
                for rep in range(3):
                    with torch.cuda.stream(streams[i]):
                        states[i].zero_()
                    edges = [0] + [c + i for c in AC.ODD_CUTS] + [K_ALL]
                    for a, b in zip(edges[:-1], edges[1:]):
                        am.run_u8(ptr(d_u8), 0, ptr(outs[i]) + 4 * a, K_ALL, a, b, B, ptr(states[i]), ptr(wss[i]), wss[i].numel(),
                                  stream=streams[i].cuda_stream)
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
                assert_bit_equal(rows[j], AC.expected_audio(oracle, t, B, "u8")[0], f"route {route}, thread {i}, channel {j}")
                assert_bit_equal(to_host(states[i]).reshape(3, 2)[j], AC.state_before(oracle, t, B, "u8", K_ALL), f"thread {i}, state {j}")


def test_follow_on_stages_on_one_stream(hip, oracle):
    """AmBank.run -> Resampler.run_rows -> Filter.run_rows for three channels on one stream without synchronisation, against the same
    stages row by row."""
    import torch
    tables = BC.bank_tables(3)
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block=True)
    am.set_route(1)
    rs = hip.Resampler(3, 10, S.gauss_taps(60, 7))
    fl = hip.Filter(S.gauss_taps(32, 9))
    n = K_ALL
    n_r = ((n - rs.num_coeffs - 10) * 3) // 10
    n_f = n_r - fl.num_coeffs + 1
    d_u8 = device_inputs(oracle)["u8"]
    stream = torch.cuda.Stream()
    audio, res, fin = dev_empty_f32(3 * n), dev_empty_f32(3 * n_r), dev_empty_f32(3 * n_f)
    ws = torch.empty(am.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    st = torch.zeros(6, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    s = stream.cuda_stream
    am.run_u8(ptr(d_u8), 0, ptr(audio), n, 0, n, B, ptr(st), ptr(ws), ws.numel(), stream=s)
    rs.run_rows(ptr(audio), ptr(res), 0, n_r, stream=s, in_stride=n, out_stride=n_r, rows=3)
    fl.run_rows(ptr(res), ptr(fin), 0, n_f, stream=s, in_stride=n_r, out_stride=n_f, rows=3)
    stream.synchronize()
    got = to_host(fin).reshape(3, n_f)
    for j, t in enumerate(tables):
        a = to_dev(AC.expected_audio(oracle, t, B, "u8")[0])
        r1, f1 = dev_empty_f32(n_r), dev_empty_f32(n_f)
        rs.run(ptr(a), 0, ptr(r1), 0, n_r, 0)
        fl.run(ptr(r1), 0, ptr(f1), 0, n_f, 0)
        assert_bit_equal(got[j], to_host(f1), f"channel {j} through resampler and filter")
