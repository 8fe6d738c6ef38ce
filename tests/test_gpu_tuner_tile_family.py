"""GPU parity of the tuner tile kernels -- k_tuner_c4 and k_tuner_bank_c4 in its three output forms -- on every (factor, prepared length)
tuner_fused_fits admits: the table of tests/tuner_tile_family_cases.py (89 shapes and twelve zero-padded tap sets, four channels, three
input formats, three seams, one run and a run cut into three launches), each row held bit for bit, NaN by position, to the models alone
(tests/tuner_model.py, am_bank_cases.envelope, nfm_bank_cases.demod).  Route 1 is forced and the launch counters show that the tile
kernel of the form ran once per launch (and the fix-up launch where the seam and threshold rule says so); every output buffer starts
as NaN canaries and every float between and around the rows is a canary still afterwards.  tests/test_tuner_tile_family_cases.py shows
on the CPU what the table reaches."""
import contextlib

import numpy as np
import pytest

import am_bank_cases as AC
import gpu_util
import narrow_bank_cases as NBC
import nfm_bank_cases as NC
import signals as S
import test_gpu_tuner as T
import tuner_model as TM
import tuner_tile_family_cases as TF
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

N = TF.N
WIDTH = {"iq": 2, "env": 1, "fm": 1, "tuner": 2}                    # floats per output
# counters: the tile launches of the three bank forms and of the one-row tuner, the int16 tile launches, the envelope fix-up launches
BANK, AM, NFM, FUSED, I16, AM_FIX = range(6)
TILE_COUNTER = {"iq": BANK, "env": AM, "fm": NFM}


def counters(hip):
    return np.array([hip.tuner_bank_launches(), hip.am_bank_launches(), hip.nfm_bank_launches(), hip.tuner_fused_launches(),
                     hip.tuner_i16_launches(), hip.am_bank_fixup_launches()], np.int64)


def device_inputs(oracle):
    u8 = TF.stream("u8")
    return {"u8": to_dev(u8), "cf32": to_dev(oracle.convert_u8(u8)), "i16": to_dev(TF.stream("i16"))}


@contextlib.contextmanager
def in_tile_cross(hip, allowed):
    """allowed: the default threshold (short seamed launches compute their Cross outputs in the tile kernel where a tile spans less
    than one buffer); not allowed: threshold 0, every seamed launch takes the fix-up launch.  test_gpu_tuner.py's launch_route."""
    prev = hip.set_small_launch_outputs(-1 if allowed else 0)
    try:
        yield
    finally:
        hip.set_small_launch_outputs(prev)


def make_op(hip, form, d, taps, tables):
    """-> (operator, [handles to close, in order])"""
    if form == "tuner":
        t = hip.Tuner(d, taps, tables[0])
        return t, [t]
    bank = hip.TunerBank(d, taps, tables)
    if form == "iq":
        return bank, [bank]
    op = hip.AmBank(bank, dc_block=False) if form == "env" else hip.NfmBank(bank)
    return op, [op, bank]


def run_case(op, form, fmt, d_in, seam, ranges, workspace):
    """The launches `ranges` (consecutive, from 0 to N) into one buffer of canaries -> (rows [channels, WIDTH N], final pairs or None).
    Rows lie WIDTH N + 2 floats apart (the one-float forms: an odd stride, so odd rows start 4 bytes off 8-byte alignment); every float
    of the buffer outside the rows must be a canary after the last launch.  fm: launch i's `final` is launch i + 1's `state`; the
    first launch takes a null state."""
    import torch
    w = WIDTH[form]
    nch = 1 if form == "tuner" else op.channels
    stride = w * N + 2
    out = dev_empty_f32(nch * stride + 3)
    name = {"cf32": "run", "u8": "run_u8", "i16": "run_i16"}[fmt]
    run = getattr(op, name)
    wsb, ws = 0, None
    if workspace and form in ("env", "fm"):
        wsb = op.workspace_bytes(N)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    st = [dev_empty_f32(2 * nch), dev_empty_f32(2 * nch)] if form == "fm" else None
    for i, (a, b) in enumerate(ranges):
        dst = ptr(out) + 4 * w * a
        if form == "tuner":
            run(ptr(d_in), 0, dst, a, b, seam)
        elif form == "iq":
            run(ptr(d_in), 0, dst, stride, a, b, seam)
        elif form == "env":
            run(ptr(d_in), 0, dst, stride, a, b, seam, None, ptr(ws) if ws is not None else None, wsb)
        else:
            run(ptr(d_in), 0, dst, stride, a, b, seam, None if i == 0 else ptr(st[i & 1]), ptr(st[(i + 1) & 1]),
                ptr(ws) if ws is not None else None, wsb)
    whole = to_host(out).view(np.uint32)
    mask = np.zeros(whole.size, bool)
    for j in range(nch):
        mask[j * stride:j * stride + w * N] = True
    assert (whole[~mask] == CANARY).all(), f"{int((whole[~mask] != CANARY).sum())} floats between or around the rows were written"
    rows = np.stack([whole[j * stride:j * stride + w * N] for j in range(nch)]).view(np.float32)
    return rows, (to_host(st[len(ranges) & 1]).reshape(nch, 2) if form == "fm" else None)


def expected_rows(oracle, form, d, p, n, seam, fmt, nch):
    f = "iq" if form == "tuner" else form
    return [TF.expected(oracle, f, d, p, n, j, seam, fmt) for j in range(nch)]


def check_case(hip, oracle, op, form, ins, d, p, n, seam, fmt, cut, route=1, in_tile=True):
    """One run or cut run of one (tap set, seam, format, form) on a route, rows [and the fm final pairs] against the models; on route 1
    the counters too."""
    f = "iq" if form == "tuner" else form
    nch = 1 if form == "tuner" else len(TF.tables())
    ranges = TF.launches(d, p, seam, fmt, f, cut)
    what = (f"factor {d}, P {p} ({n} taps), {TF.branch(d, p)}, {form}, {fmt}, seam {seam} ({TF.SEAM_NAMES[TF.seams(d, p).index(seam)]}), "
            f"launches {ranges}, route {route}" + ("" if in_tile else ", fix-up launches forced"))
    c0 = counters(hip)
    rows, fin = run_case(op, form, fmt, ins[fmt], seam, ranges, workspace=route != 1)
    dlt = counters(hip) - c0
    if route == 1:
        want = np.zeros(6, np.int64)
        want[I16] = len(ranges) if fmt == "i16" else 0
        if form == "tuner":
            want[FUSED] = 0 if fmt == "i16" else len(ranges)          # the one-row int16 tuner takes the bank's kernel with one channel
        else:
            want[TILE_COUNTER[form]] = len(ranges)
        if form == "env":
            want[AM_FIX] = TF.fixup_launches(d, p, seam, ranges, in_tile)
        assert (dlt == want).all(), what + f": launch counters {dlt} for {want} [bank, am, nfm, tuner, int16, am fix-up]"
    elif route == 2:
        assert dlt[FUSED if form == "tuner" else TILE_COUNTER[form]] == 0, what + f": route 2 launched the form's tile kernel {dlt}"
    exp = expected_rows(oracle, form, d, p, n, seam, fmt, nch)
    for j in range(nch):
        assert_bit_equal(rows[j], exp[j], what + f": channel {j}")
        if form == "fm":
            assert_bit_equal(fin[j], TF.fm_state_before(oracle, d, p, n, j, seam, fmt, N), what + f": final pair of channel {j}")


def sweep(hip, oracle, form, d):
    """Every tap set of the factor x three formats x three seams x (one run, cut run), route 1; the wide seam of the complex and
    envelope forms with the Cross outputs in the tile and by the fix-up launch; the PADDED lengths also on routes 2 and 0."""
    ins = device_inputs(oracle)
    cases = 0
    per_branch = dict.fromkeys(TF.BRANCHES, 0)
    for e, p, n in TF.TAP_SETS:
        if e != d:
            continue
        op, handles = make_op(hip, form, d, TF.taps(d, p, n), TF.tables())
        assert (op.tuner_bank if form in ("env", "fm") else op).num_coeffs == p, f"factor {d}, {n} taps prepare to {p}"
        _, _, wide = TF.seams(d, p)
        routes = (1, 2, 0) if (d, p) in TF.PADDED_SHAPES and n == p else (1,)
        for route in routes:
            op.set_route(route)                                      # 0 auto, 1 the tile kernel, 2 two-pass / channels / composed
            for seam in TF.seams(d, p):
                for fmt in TF.FORMATS:
                    for cut in (False, True):
                        for allowed in ((True, False) if seam == wide and form != "fm" and route == 1 else (True,)):
                            with in_tile_cross(hip, allowed):
                                check_case(hip, oracle, op, form, ins, d, p, n, seam, fmt, cut, route, allowed)
                            cases += 1
                            per_branch[TF.branch(d, p)] += route == 1
        for h in handles:
            h.close()
        gpu_util.check_guards()                                      # (and forget this tap set's buffers)
    print(f"    {form}, factor {d}: {cases} runs compared; route 1 by branch: { {b: c for b, c in per_branch.items() if c} }")
    return cases


@pytest.mark.parametrize("form", TF.FORMS)
@pytest.mark.parametrize("d", TF.FACTORS)
def test_the_bank_forms_on_every_length_of_a_factor(hip, oracle, d, form):
    """iq: TunerBank; env: AmBank(dc_block=False); fm: NfmBank."""
    sweep(hip, oracle, form, d)


@pytest.mark.parametrize("d", TF.FACTORS)
def test_the_one_row_tuner_on_every_length_of_a_factor(hip, oracle, d):
    """hip.Tuner has kernels of its own for cfloat and u8 and takes the bank's kernel with one channel for int16 (channel 0, period 1000)."""
    sweep(hip, oracle, "tuner", d)


# ---- the edges of the family ------------------------------------------------------------------------------------------------------------
# (factor, coefficients, prepared length): P = D twice, one tap chunk past the family, a factor outside it
EDGES = [(8, 8, 8), (16, 16, 16), (8, 129, 132), (5, 127, 128)]
EDGE_BLOCK, EDGE_SAMPLES = 4096, 5 * 4096


@pytest.mark.parametrize("form", ["env", "fm"])
@pytest.mark.parametrize("d,ntaps,p", EDGES, ids=[f"factor {d}, {n} taps" for d, n, _ in EDGES])
def test_the_edges_of_the_family_are_refused_by_route_1_and_served_by_auto(hip, oracle, d, ntaps, p, form):
    """No tile kernel serves these shapes: forced route 1 is an error that writes nothing, auto gives the model's bits without a tile
    launch.  (P = D: a buffer boundary would leave the reference's Pipe an empty remainder, which it asserts on -- one buffer only.)"""
    import torch
    assert not TF.admitted(d, p)
    taps = S.taps_decim127() if ntaps == 127 else NBC._seeded_taps(ntaps, 1000 * d + ntaps)
    tables = [T.osc_table(1000), T.osc_table(5)]
    op, handles = make_op(hip, form, d, taps, tables)
    assert op.tuner_bank.num_coeffs == p
    ins = {"u8": TF.stream("u8")[:2 * EDGE_SAMPLES], "i16": TF.stream("i16")[:2 * EDGE_SAMPLES]}
    ins["cf32"] = oracle.convert_u8(ins["u8"])
    for seam in ((0,) if p == d else (0, EDGE_BLOCK)):
        for fmt in TF.FORMATS:
            x = oracle.convert_i16(ins["i16"]) if fmt == "i16" else ins["cf32"]
            iq = [TM.tuner_expected(oracle, taps, PM.ORDER_AVX, d, x, t, seam, 0, block_out=1) for t in tables]
            n_out = iq[0].size // 2
            assert n_out > 2 * TF.OUTS
            exp = [AC.envelope(q) if form == "env" else NC.demod(oracle, q) for q in iq]
            d_in = to_dev(ins[fmt])
            run = getattr(op, {"cf32": "run", "u8": "run_u8", "i16": "run_i16"}[fmt])
            what = f"factor {d}, {ntaps} taps, {form}, {fmt}, seam {seam}"
            wsb = op.workspace_bytes(n_out)
            ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
            for route in (1, 0):
                op.set_route(route)
                out, fin = dev_empty_f32(2 * n_out + 2), dev_empty_f32(4)
                args = (ptr(d_in), 0, ptr(out), n_out + 1, 0, n_out, seam) + ((None,) if form == "env" else (None, ptr(fin))) + (ptr(ws), wsb)
                c0 = counters(hip)
                if route == 1:
                    with pytest.raises(hip.SdrHipError):
                        run(*args)
                    assert (to_host(out).view(np.uint32) == CANARY).all() and (to_host(fin).view(np.uint32) == CANARY).all(), what + ": a refused run wrote"
                    assert (counters(hip) == c0).all(), what + ": a refused run launched"
                    continue
                run(*args)
                got = to_host(out)
                dlt = counters(hip) - c0
                assert dlt[BANK] == 0 and dlt[AM] == 0 and dlt[NFM] == 0 and dlt[FUSED] == 0 and dlt[AM_FIX] == 0, what + f": auto launched a tile kernel {dlt}"
                for j in range(2):
                    assert_bit_equal(got[j * (n_out + 1):j * (n_out + 1) + n_out], exp[j], what + f", auto: channel {j}")
                    if form == "fm":
                        assert_bit_equal(to_host(fin)[2 * j:2 * j + 2], iq[j][-2:], what + f", auto: final pair of channel {j}")
                assert (got.view(np.uint32)[[n_out, 2 * n_out + 1]] == CANARY).all(), what + ": a float between the rows was written"
    for h in handles:
        h.close()
