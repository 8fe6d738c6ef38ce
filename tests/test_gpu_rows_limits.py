"""GPU: the row forms at SDRHIP_ROWS_MAX = 1024 rows and at the lane cap of the agc / dcBlocker rows plan (tests/rows_limit_cases.py;
tests/test_rows_limit_cases.py shows on the CPU what the shapes reach).

A. agc_rows / dc_blocker_rows on 1024 x 8192 (exactly 32768 lanes), 1024 x 8193 and 513 x 16385 (the chunk grown from 256 to 264
samples: the plan is no longer the one-row plan) and 1024 x 100 (the sequential walk).  Every row's output and final state against the
sequential models, every row's chunk count against the plan, the checked rows' statistics words against the scheme model under the
ROWS plan and their outputs against the one-row device call (whose plan, and so whose statistics, differ); canaries around every
row, and 0xA5 behind the reported workspace size.  Then rows further apart (another access width), then no workspace at all.
fmDemod: 1024 rows in one launch.

B. The FIR rows on the banked route with 1024 rows: blockIdx.y up to 1023 in the tile kernel, (row, seam, slot) up to row 1023 in
the fix-up kernels, against the row-by-row route on every row and the restated Pipe on five."""
import numpy as np
import pytest
import torch

import fir_rows_cases as RC
import gpu_util
import rows_limit_cases as LC
from conftest import assert_bit_equal
from test_gpu_fir_rows import desc_of, one_row_calls
from test_gpu_fir_rows import run_rows as fir_run_rows
from test_gpu_rows import Rows, _floats, _many, _same_state, one_row, run_rows

pytestmark = pytest.mark.gpu

PAD = 4096                      # bytes behind the reported workspace size that must stay 0xA5


def _call(hip, op, xs, states, in_extra, out_extra, use_ws, what):
    """test_gpu_rows.run_rows with the workspace allocated PAD bytes longer than reported and the reported size passed.
    -> (outputs, finals, statistics or None, launches)"""
    rows, width = len(xs), _floats(xs[0]).size
    n = width if op == "dc" else width // 2
    if not use_ws:
        return run_rows(hip, op, xs, states, LC.RUN_IN, LC.MU, LC.REFERENCE, in_extra, out_extra, use_ws=False, what=what)
    nbytes = (hip.lib.sdrhip_dc_blocker_rows_workspace_bytes if op == "dc" else hip.lib.sdrhip_agc_rows_workspace_bytes)(rows, n)
    whole = torch.full((nbytes + PAD,), 0xA5, dtype=torch.uint8, device="cuda")
    ws = whole[:nbytes]
    src = Rows(rows, width, in_extra, 0, host=xs)
    dst = Rows(rows, width, out_extra, 0)
    st = gpu_util.to_dev(np.asarray(states, np.float32).reshape(rows, -1))
    fin = gpu_util.dev_empty_f32(st.numel()).view(st.shape)
    l0 = hip.rows_launches()
    if op == "dc":
        hip.dc_blocker_rows(src.view, st, LC.RUN_IN, out=dst.view, final=fin, workspace=ws)
    else:
        hip.agc_rows(src.view, LC.MU, LC.REFERENCE, st.view(rows), LC.RUN_IN, out=dst.view, final=fin.view(rows), workspace=ws)
    launches = hip.rows_launches() - l0
    outs = dst.read(what)
    behind = whole[nbytes:].cpu().numpy()
    assert (behind == 0xA5).all(), f"{what}: {int((behind != 0xA5).sum())} of the {PAD} bytes behind the reported workspace size ({nbytes}) were written"
    return outs, gpu_util.to_host(fin).copy(), hip.rows_stats(ws, rows), launches


@pytest.mark.parametrize("shape", LC.IIR_SHAPES, ids=[s.name for s in LC.IIR_SHAPES])
@pytest.mark.parametrize("op", ["agc", "dc"])
def test_iir_rows_at_the_lane_cap_and_at_rows_max(hip, oracle, op, shape):
    rows, n = shape.rows, shape.n
    plan, one_plan = LC.plans(hip, op, shape)
    assert plan == shape.plan and one_plan[0] == shape.one_row[0] and (one_plan == shape.one_row or not one_plan[0]), (plan, one_plan)
    assert rows * plan[0] <= LC.LANE_CAP and shape.grown == (plan != one_plan)
    xs, states = LC.many(op, rows, n)
    for r, (x, st) in enumerate(zip(*_many(op, 8, n))):                      # the recipe of test_gpu_rows, but for the directed rows
        if not (op == "dc" and LC.fixed_row(r)):
            assert np.array_equal(_floats(x), _floats(xs[r])) and tuple(st) == tuple(states[r]), r
    t = LC.truth(op, shape, oracle)
    if op == "agc":
        assert all(np.isfinite(o).all() for o in t.outs), "the agc expected outputs are finite"
    # (gap between input rows, between output rows): tight; then 2 floats (agc) / 1 float (dcBlocker) apart on the input side, which
    # changes the access width (tight rows of an odd n are 8 / 4 bytes off already: there the gap of 2 restores float4 for agc)
    layouts = [(0, 0), (2, 0) if op == "agc" else (1, 0)]
    if op == "dc" and n % 4:
        layouts.append((4 - n % 4, 4 - n % 4))                                # dcBlocker's float4 walk on rows of an odd n
    for li, (gi, go) in enumerate(layouts):
        what = f"{op}, {shape.name}, rows +{gi} / +{go} floats apart"
        outs, fins, stats, launches = _call(hip, op, xs, states, gi, go, True, what)
        print(f"    {what}: rows plan {plan}, one-row plan {one_plan}, {launches} launches, {rows * plan[0]} lanes")
        assert launches == (5 if plan[0] else 1), what
        for r in range(rows):
            assert_bit_equal(outs[r], t.outs[r], f"{what}, row {r}")
            _same_state(fins[r], t.finals[r], f"{what}, row {r}")
            assert stats[r][3] == plan[0], (what, r, stats[r], plan)
        if not plan[0]:
            assert all(s == (0, 0, 0, 0) for s in stats), what
            continue
        for r in shape.subset:
            s = LC.row_scheme(op, shape, r, plan, oracle)
            assert not s.nan_starts
            assert stats[r] == LC.stats_of(s), (what, r, stats[r], LC.stats_of(s))
            if li == 0:
                o1, f1, st1 = one_row(hip, op, xs[r], states[r], LC.RUN_IN, LC.MU, LC.REFERENCE)
                assert_bit_equal(outs[r], o1, f"{what}, row {r} vs the one-row call")
                assert_bit_equal(fins[r], f1, f"{what}, row {r}: final state vs the one-row call")
                assert (st1[3] != stats[r][3]) == shape.grown, (what, r, st1, stats[r])     # its plan differs: nothing else of its statistics is compared
                assert shape.grown or st1 == stats[r], (what, r, st1, stats[r])
    # no workspace: every row on the sequential walk, one launch
    what = f"{op}, {shape.name}, null workspace"
    outs, fins, _, launches = _call(hip, op, xs, states, 0, 0, False, what)
    assert launches == 1, what
    for r in range(rows):
        assert_bit_equal(outs[r], t.outs[r], f"{what}, row {r}")
        _same_state(fins[r], t.finals[r], f"{what}, row {r}")


def test_fm_demod_1024_rows(hip, oracle):
    """1024 rows of 1027 samples (one workgroup a row on blockIdx.y, a tail of 3) from in_base 0, then from k_begin 3 (the
    predecessor is in the buffer; the carried array, NaN before the call, is not read): the oracle's fm_demod on every row."""
    from test_gpu_rows import _fm_rows
    rows, n = LC.FM_ROWS, LC.FM_N
    xs = _fm_rows(rows, n, seed=2000)
    lasts = np.random.default_rng(19).standard_normal((rows, 2)).astype(np.float32)
    exp = [oracle.fm_demod(_floats(x), tuple(lasts[r])) for r, x in enumerate(xs)]
    assert len({e.tobytes() for e in exp}) == rows, "no two rows expect the same"
    src = Rows(rows, 2 * n, 2, 0, host=xs)
    newest = np.stack([_floats(x)[-2:] for x in xs])
    for k_begin in (0, 3):
        what = f"fmDemod, {rows} rows of {n}, k_begin {k_begin}"
        dst = Rows(rows, n - k_begin, 1, 0)
        last = gpu_util.to_dev(lasts if k_begin == 0 else np.full((rows, 2), np.nan, np.float32))
        carry = gpu_util.dev_empty_f32(2 * rows).view(rows, 2)
        l0 = hip.rows_launches()
        hip.fm_demod_rows(src.view, last, out=dst.view, last_out=carry, in_base=0, k_begin=k_begin, k_end=n)
        assert hip.rows_launches() - l0 == 1, what
        outs = dst.read(what)
        for r in range(rows):
            assert_bit_equal(outs[r], exp[r][k_begin:], f"{what}, row {r}")
        assert_bit_equal(gpu_util.to_host(carry).ravel(), newest.ravel(), what + ": the carried samples")


# ---- B: the FIR rows, banked, 1024 rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LC.FIR_1024, ids=LC.FIR_1024)
def test_fir_rows_banked_with_1024_rows(hip, oracle, name):
    f = RC.BY_NAME[name]
    desc = desc_of(hip, f)
    for case in LC.fir_1024_cases(f):
        g = RC.resolve(hip, case, desc)
        seams = RC.seams_inside(f, g.k_begin, g.k_end, g.seam)
        assert (len(seams) >= 3) if case.seam_kind == "three" else not seams, (case.name, seams)
        xs = [LC.fir_row_stream(case, g, r) for r in range(case.rows)]
        outs = {}
        for route in (1, 2):
            what = f"{case.name}, route {route}"
            outs[route], (tiles, fixups, split) = fir_run_rows(hip, case, g, xs, route, what=what)
            print(f"    {what}: plan {g.plan}, {g.n} outputs a row, {len(seams)} seams inside, tile launches {tiles}, fix-up launches {fixups}")
            if route == 1:
                assert (tiles, fixups, split) == (1, int(bool(seams)), 0), f"{what}: {tiles} tile launches, {fixups} fix-up launches"
            else:
                assert (tiles, fixups) == (0, 0), f"{what}: the row-by-row route moved the banked counters"
        for r in range(case.rows):
            assert_bit_equal(outs[1][r], outs[2][r], f"{case.name}: banked against row by row, row {r}")
        for r in LC.FIR_PIPE_ROWS:
            assert_bit_equal(outs[1][r], RC.pipe_expected(case, g, oracle, xs[r]), f"{case.name}: banked against the restated Pipe, row {r}")
        few = [xs[r] for r in LC.FIR_PIPE_ROWS]
        one = one_row_calls(hip, case, g, few)
        for i, r in enumerate(LC.FIR_PIPE_ROWS):
            assert_bit_equal(outs[1][r], one[i], f"{case.name}: banked against the one-row call, row {r}")
