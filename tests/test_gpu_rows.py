"""GPU: the row forms of agc, dcBlocker and fmDemod (sdrhip_agc_run_rows, sdrhip_dc_blocker_run_rows, sdrhip_fm_demod_run_rows).

Every row of every launch is held, bit for bit, to the sequential truth of that row alone -- tests/agc_model.py, the oracle's
dc_blocker and fm_demod -- and to the one-row device call on that row; final states and carried samples included.  The per-row
statistics words are held to the scheme model (iir_cases.scheme) under the plan the rows hook reports.  Output buffers start as
NaN canaries, and every float outside the rows' outputs -- before, between and behind them -- is a canary afterwards.

Launch counts: sdrhip_debug_rows_launches counts the row kernels' launches (one on the sequential walk and for fmDemod, five with
chunks).  The one-row agc / dcBlocker / fmDemod kernels have no launch counter, so "none of the one-row kernels ran" is not asserted.

The row sets are those of tests/iir_rows_cases.py; tests/test_iir_rows_cases.py shows on the CPU what they reach."""
import numpy as np
import pytest
import torch

import agc_model
import gpu_util
import iir_cases as IC
import iir_rows_cases as RC
import signals as S
from conftest import assert_bit_equal
from gpu_util import CANARY

pytestmark = pytest.mark.gpu

ERR_ARG = -1
NAN_BITS = 0x7FC00BAD                                   # between the input rows: a kernel that reads past a row computes on NaN


def _floats(x):
    return np.ascontiguousarray(x).view(np.float32)


def _same_state(got, exp, what):
    got, exp = np.asarray(got, np.float32).ravel(), np.asarray(exp, np.float32).ravel()
    assert got.shape == exp.shape and IC.same(got, exp).all(), f"{what}: final state {got!r}, expected {exp!r}"


class Rows:
    """rows x width floats on the device, `extra` floats between the rows, the first row `off` floats behind a 256-byte boundary.
    As an input the gaps hold NaN, as an output (host rows None) everything holds the canary and the buffer has guard bands."""

    def __init__(self, rows, width, extra=0, off=0, host=None):
        self.rows, self.width, self.stride, self.off = rows, width, width + extra, off
        total = off + rows * self.stride + 8
        if host is None:
            self.whole = gpu_util.dev_empty_f32(total)
        else:
            w = np.full(total, NAN_BITS, np.uint32)
            for r in range(rows):
                w[off + r * self.stride: off + r * self.stride + width] = _floats(host[r]).view(np.uint32)
            self.whole = torch.from_numpy(w.view(np.float32)).cuda()
        self.view = self.whole[off:].as_strided((rows, width), (self.stride, 1))
        assert (width == 0 or self.view.data_ptr() == self.whole.data_ptr() + 4 * off) and self.whole.data_ptr() % 256 == 0

    def read(self, what=""):
        """The rows as written, after checking that every other float of the buffer (and its guard bands) is the canary still."""
        w = gpu_util.to_host(self.whole).view(np.uint32)
        mask = np.ones(w.size, bool)
        for r in range(self.rows):
            mask[self.off + r * self.stride: self.off + r * self.stride + self.width] = False
        bad = np.nonzero(mask & (w != CANARY))[0]
        assert bad.size == 0, f"{what}: {bad.size} floats outside the rows' outputs were written, first at float {bad[0]} (row stride {self.stride})"
        return [w[self.off + r * self.stride: self.off + r * self.stride + self.width].view(np.float32).copy() for r in range(self.rows)]

    def untouched(self):
        return bool((gpu_util.to_host(self.whole).view(np.uint32) == CANARY).all())


def _ws(hip, op, rows, n):
    nbytes = (hip.lib.sdrhip_dc_blocker_rows_workspace_bytes if op == "dc" else hip.lib.sdrhip_agc_rows_workspace_bytes)(rows, n)
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")        # the launch must write every word it reports


def run_rows(hip, op, xs, states, run_in, mu=0.0, ref=1.0, in_extra=0, out_extra=0, in_off=0, out_off=0, use_ws=True, what=""):
    """One rows call over the host rows xs (float32 or complex64, equal lengths) from `states` (one tuple a row).
    -> (outputs as float32 rows, final states [rows, 1 or 2], statistics per row or None, launches counted)."""
    rows, width = len(xs), _floats(xs[0]).size
    n = width if op == "dc" else width // 2
    src = Rows(rows, width, in_extra, in_off, host=xs)
    dst = Rows(rows, width, out_extra, out_off)
    st = gpu_util.to_dev(np.asarray(states, np.float32).reshape(rows, -1))
    fin = gpu_util.dev_empty_f32(st.numel()).view(st.shape)
    ws = _ws(hip, op, rows, n) if use_ws else None
    l0 = hip.rows_launches()
    if op == "dc":
        hip.dc_blocker_rows(src.view, st, run_in, out=dst.view, final=fin, workspace=ws)
    else:
        hip.agc_rows(src.view, mu, ref, st.view(rows), run_in, out=dst.view, final=fin.view(rows), workspace=ws)
    launches = hip.rows_launches() - l0
    outs = dst.read(what)
    return outs, gpu_util.to_host(fin).copy(), (hip.rows_stats(ws, rows) if use_ws else None), launches


def one_row(hip, op, x, state, run_in, mu=0.0, ref=1.0, use_ws=True):
    """The one-row device call on this row alone -> (output, final state, statistics)."""
    import test_gpu_iir as G
    case = IC.Case("one-row", op, (), x.size, run_in, "", state=tuple(state), mu=mu, reference=ref)
    return G._launch(hip, case, np.ascontiguousarray(x), tuple(float(v) for v in state), use_ws=use_ws)


# ---- 1: truth, statistics, launch counts, both routes, null workspace ------------------------------------------------------------
@pytest.mark.parametrize("rs", RC.SETS, ids=[s.name for s in RC.SETS])
def test_row_set_against_models_scheme_and_the_one_row_call(hip, oracle, rs):
    cases, plan = rs.cases(), RC.plan_of(hip, rs)
    ss = RC.schemes(hip, rs, oracle)
    xs = [IC.stream(c) for c in cases]
    states = [c.state for c in cases]
    assert plan == (hip.dc_plan(rs.n, rs.run_in) if rs.op == "dc" else hip.agc_plan(rs.n, rs.mu, rs.run_in))
    outs, fins, stats, launches = run_rows(hip, rs.op, xs, states, rs.run_in, rs.mu, rs.reference, what=rs.name)
    assert launches == (5 if plan[0] else 1), f"{rs.name}: {launches} launches of the row kernels for one call"
    for r, (c, s) in enumerate(zip(cases, ss)):
        what = f"{rs.name}, row {r} {c.stream}"
        print(f"    {what}: model {s.describe()}; device statistics {stats[r]}")
        assert_bit_equal(outs[r], _floats(s.out), what)
        _same_state(fins[r], s.final, what)
        assert not s.nan_starts
        if rs.n:                                                 # n == 0 copies the states and touches nothing else
            assert stats[r][3] == plan[0] == s.chunks, (what, stats[r], plan)
            assert stats[r][:3] == (s.left, s.rewritten, s.repaired), (what, stats[r], (s.left, s.rewritten, s.repaired))
            o1, f1, st1 = one_row(hip, rs.op, xs[r], states[r], rs.run_in, rs.mu, rs.reference)
            assert_bit_equal(outs[r], o1, what + " vs the one-row call")
            assert_bit_equal(fins[r], f1, what + ": final state vs the one-row call")
            assert stats[r] == st1, (what, stats[r], st1)
    # no workspace: every row on the sequential walk, still one launch
    outs, fins, _, launches = run_rows(hip, rs.op, xs, states, rs.run_in, rs.mu, rs.reference, use_ws=False, what=rs.name + ", null workspace")
    assert launches == 1
    for r, s in enumerate(ss):
        assert_bit_equal(outs[r], _floats(s.out), f"{rs.name}, null workspace, row {r}")
        _same_state(fins[r], s.final, f"{rs.name}, null workspace, row {r}")


# ---- 2: strides and alignment -----------------------------------------------------------------------------------------------------
# (input gap, output gap, input offset, output offset) in floats; complex rows take even gaps, real rows odd ones too
LAYOUTS_CPLX = [(2, 2, 0, 0), (6, 2, 0, 0), (2, 6, 2, 0), (0, 0, 1, 1), (0, 0, 2, 2), (6, 6, 0, 2), (0, 2, 0, 1)]
LAYOUTS_REAL = [(1, 1, 0, 0), (3, 1, 0, 0), (1, 3, 2, 0), (0, 0, 1, 1), (0, 0, 2, 2), (3, 3, 0, 2), (0, 4, 0, 0), (4, 1, 1, 0)]


@pytest.mark.parametrize("name", ["agc-branches", "dc-branches", "agc-n=129", "dc-n=129", "agc-n=127", "dc-n=7"])
def test_strides_base_offsets_and_canaries(hip, oracle, name):
    """Rows tight, +2 / +6 (complex) and +1 / +3 (real) floats apart, base pointers 4 and 8 bytes off 16-byte alignment, input and
    output laid out differently: the access width has to follow the worst of the pointers AND the strides."""
    rs = RC.BY_NAME[name]
    cases, ss = rs.cases(), RC.schemes(hip, rs, oracle)
    xs, states = [IC.stream(c) for c in cases], [c.state for c in cases]
    for use_ws in (True, False):
        for lay in (LAYOUTS_REAL if rs.op == "dc" else LAYOUTS_CPLX):
            what = f"{name}, layout {lay}, {'workspace' if use_ws else 'null workspace'}"
            outs, fins, stats, _ = run_rows(hip, rs.op, xs, states, rs.run_in, rs.mu, rs.reference, *lay, use_ws=use_ws, what=what)
            for r, s in enumerate(ss):
                assert_bit_equal(outs[r], _floats(s.out), f"{what}, row {r}")
                _same_state(fins[r], s.final, f"{what}, row {r}")
                if use_ws:
                    assert stats[r] == (s.left, s.rewritten, s.repaired, s.chunks), (what, r, stats[r])


# ---- 3: 1, 3 and 65 rows ------------------------------------------------------------------------------------------------------------
def _many(op, rows, n):
    """rows streams of n samples, each from a seed, level and state of its own (every eighth agc row silent)."""
    if op == "dc":
        xs = [np.random.default_rng(500 + r).uniform(-1, 1, n).astype(np.float32) * np.float32(1 + r % 5) for r in range(rows)]
        return xs, [(0.01 * r - 0.3, 0.5 - 0.02 * r) for r in range(rows)]
    xs = [IC._noise(n, 600 + r, (0.3, 0.05, 0.6, 0.01, 0.2, 0.1, 0.4, 0.0)[r % 8]) for r in range(rows)]
    return xs, [(1.0 + 0.03 * r,) for r in range(rows)]


@pytest.mark.parametrize("op", ["agc", "dc"])
@pytest.mark.parametrize("rows", [1, 3, 65])
def test_one_three_and_sixty_five_rows(hip, oracle, op, rows):
    """n = 601 at run_in 64 (three chunks a row: 195 lanes over four waves at 65 rows, the rows' lanes packed across them) and n = 100
    (the sequential walk, 65 workgroups)."""
    mu = 0.4
    for n, chunks in ((601, 3), (100, 0)):
        xs, states = _many(op, rows, n)
        assert (hip.dc_rows_plan(rows, n, 64) if op == "dc" else hip.agc_rows_plan(rows, n, mu, 64))[0] == chunks
        if op == "dc":
            truth = [oracle.dc_blocker(x, *st) for x, st in zip(xs, states)]
            exp, efin = [t[0] for t in truth], [np.array(t[1:], np.float32) for t in truth]
        else:
            o, f = agc_model.agc(np.stack(xs), mu, 1.0, np.array([s[0] for s in states], np.float32))
            exp, efin = [_floats(o[r]) for r in range(rows)], [f[r:r + 1] for r in range(rows)]
            assert np.isfinite(np.concatenate(exp)).all()
        for use_ws in (True, False):
            what = f"{op}, {rows} rows of {n}, {'workspace' if use_ws else 'null workspace'}"
            outs, fins, stats, launches = run_rows(hip, op, xs, states, 64, mu, 1.0, 2 if rows == 3 else 0, 0, use_ws=use_ws, what=what)
            assert launches == (5 if chunks and use_ws else 1), what
            for r in range(rows):
                assert_bit_equal(outs[r], exp[r], f"{what}, row {r}")
                _same_state(fins[r], efin[r], f"{what}, row {r}")
                if use_ws:
                    assert stats[r][3] == chunks
            if use_ws:
                for r in sorted({0, rows // 2, rows - 2 if rows > 2 else 0, rows - 1}):     # 65 rows: 0, 32, 63 and 64, either side of a wave
                    o1, f1, st1 = one_row(hip, op, xs[r], states[r], 64, mu, 1.0)
                    assert_bit_equal(outs[r], o1, f"{what}, row {r} vs the one-row call")
                    assert_bit_equal(fins[r], f1, f"{what}, row {r}: final state vs the one-row call")
                    assert stats[r] == st1, (what, r, stats[r], st1)


# ---- 4: neighbours ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["agc", "dc"])
@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_neighbour_of_nan_or_inf_changes_nothing(hip, oracle, op, poison):
    mu = 0.4
    for n in (601, 100):
        xs, states = _many(op, 3, n)
        for use_ws in (True, False):
            ref_outs, ref_fins, ref_stats, _ = run_rows(hip, op, xs, states, 64, mu, use_ws=use_ws)
            bad = [x.copy() for x in xs]
            bad[1][:] = poison
            outs, fins, stats, _ = run_rows(hip, op, bad, [states[0], (poison,) * len(states[1]), states[2]], 64, mu, use_ws=use_ws)
            for r in (0, 2):
                assert_bit_equal(outs[r], ref_outs[r], f"{op}, n = {n}: row {r} beside a row of {poison}")
                assert_bit_equal(fins[r], ref_fins[r], f"{op}, n = {n}: row {r}'s final state beside a row of {poison}")
                if use_ws:
                    assert stats[r] == ref_stats[r]
            assert not np.isfinite(outs[1]).any() or op == "dc", "the poisoned row is poisoned"


# ---- 5: a workspace one byte too small ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["agc", "dc"])
def test_short_workspace_is_refused_with_nothing_written(hip, op):
    rows, n = 3, 601
    xs, states = _many(op, rows, n)
    width = _floats(xs[0]).size
    src, dst = Rows(rows, width, host=xs), Rows(rows, width)
    st = gpu_util.to_dev(np.asarray(states, np.float32).reshape(rows, -1))
    fin = gpu_util.dev_empty_f32(st.numel())
    ws = _ws(hip, op, rows, n)
    l0 = hip.rows_launches()
    if op == "dc":
        rc = hip.lib.sdrhip_dc_blocker_run_rows(None, src.view.data_ptr(), width, dst.view.data_ptr(), width, rows, n, st.data_ptr(), fin.data_ptr(),
                                                ws.data_ptr(), ws.numel() - 1, 64)
    else:
        rc = hip.lib.sdrhip_agc_run_rows(None, src.view.data_ptr(), width, dst.view.data_ptr(), width, rows, n, 0.4, 1.0, st.data_ptr(), fin.data_ptr(),
                                         ws.data_ptr(), ws.numel() - 1, 64)
    assert rc == ERR_ARG and b"workspace" in hip.lib.sdrhip_last_error()
    torch.cuda.synchronize()
    assert hip.rows_launches() == l0 and dst.untouched()
    assert (gpu_util.to_host(fin).view(np.uint32) == CANARY).all() and (ws.cpu().numpy() == 0xA5).all()


# ---- 6: carrying state ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["agc-branches", "dc-branches"])
def test_state_carried_on_the_device_across_three_calls(hip, oracle, name):
    """The rows cut at odd sample counts into three calls, d_final == d_state, no host in between: the uncut model.  The cuts put a
    piece on either route, and their inputs are views into one buffer: rows one whole stream apart, starting at odd samples."""
    rs = RC.BY_NAME[name]
    cases, ss = rs.cases(), RC.schemes(hip, rs, oracle)
    rows, per = len(cases), 1 if rs.op == "dc" else 2
    cuts = [0, 1301, 1902, rs.n] if rs.op == "agc" else [0, 127, 1290, rs.n]
    plans = [(hip.dc_rows_plan(rows, b - a, rs.run_in) if rs.op == "dc" else hip.agc_rows_plan(rows, b - a, rs.mu, rs.run_in))[0]
             for a, b in zip(cuts[:-1], cuts[1:])]
    assert 0 in plans and max(plans) > 0, plans
    src = Rows(rows, per * rs.n, host=[IC.stream(c) for c in cases])
    dst = Rows(rows, per * rs.n, 2 * per)
    st = gpu_util.to_dev(np.asarray([c.state for c in cases], np.float32).reshape(rows, -1))
    ws = _ws(hip, rs.op, rows, rs.n)
    for a, b in zip(cuts[:-1], cuts[1:]):
        x, y = src.view[:, per * a: per * b], dst.view[:, per * a: per * b]
        if rs.op == "dc":
            hip.dc_blocker_rows(x, st, rs.run_in, out=y, final=st, workspace=ws)
        else:
            hip.agc_rows(x, rs.mu, rs.reference, st.view(rows), rs.run_in, out=y, final=st.view(rows), workspace=ws)
    outs, fins = dst.read(name), gpu_util.to_host(st)
    for r, s in enumerate(ss):
        assert_bit_equal(outs[r], _floats(s.out), f"{name} cut at {cuts[1:-1]}, row {r}")
        _same_state(fins[r], s.final, f"{name} cut at {cuts[1:-1]}, row {r}")


# ---- 7: fmDemod ----------------------------------------------------------------------------------------------------------------------
def _fm_rows(rows, n, seed=0):
    """Noise with a stretch of zeros, of samples on the axes and of repeated samples in every row: the rare branches of the phase."""
    xs = []
    for r in range(rows):
        x = IC._noise(n, 700 + seed + r, 0.5).copy()
        if n >= 64:
            x[10 + r % 7: 14 + r % 7] = 0
            x[20:24] = np.array([1, 1j, -1, -1j], np.complex64) * np.float32(0.25 + r)
            x[30:33] = x[29]
            x[40] = -x[39]
        xs.append(x)
    return xs


def _fm_one_row(hip, x, last):
    d_in = gpu_util.to_dev(_floats(x)) if x.size else torch.zeros(2, device="cuda")
    d_out = gpu_util.dev_empty_f32(x.size)
    hip.check(hip.lib.sdrhip_fm_demod_run(None, d_in.data_ptr(), 0, d_out.data_ptr(), 0, x.size, float(last[0]), float(last[1])), "sdrhip_fm_demod_run")
    return gpu_util.to_host(d_out).copy()


@pytest.mark.parametrize("rows", [1, 3, 65])
def test_fm_demod_rows(hip, oracle, rows):
    """Counts 0 .. 5 (no quad, one quad, a tail), 1027 (one workgroup, a tail of 3) and 2051 (two workgroups a row); input rows +2 / +6
    floats apart, output rows +1 / +3, bases 4 and 8 bytes off: against the oracle's fm_demod and sdrhip_fm_demod_run on each row."""
    lasts = np.random.default_rng(9).standard_normal((rows, 2)).astype(np.float32)
    for n in (0, 1, 3, 4, 5, 1027, 2051):
        xs = _fm_rows(rows, n)
        exp = [oracle.fm_demod(_floats(x), tuple(lasts[r])) for r, x in enumerate(xs)]
        exp0 = [oracle.fm_demod(_floats(x), (0.0, 0.0)) for x in xs]
        layouts = [(0, 0, 0, 0), (2, 1, 0, 0), (6, 3, 2, 1), (0, 0, 2, 2), (2, 4, 0, 0)] if n in (5, 1027, 2051) else [(0, 0, 0, 0), (2, 1, 2, 1)]
        for in_extra, out_extra, in_off, out_off in layouts:
            what = f"fmDemod, {rows} rows of {n}, layout {(in_extra, out_extra, in_off, out_off)}"
            src = Rows(rows, 2 * n, in_extra, in_off, host=xs)
            for last, want in ((gpu_util.to_dev(lasts), exp), (None, exp0)):
                dst = Rows(rows, n, out_extra, out_off)
                carry = gpu_util.dev_empty_f32(2 * rows).view(rows, 2)
                l0 = hip.rows_launches()
                hip.fm_demod_rows(src.view, last, out=dst.view, last_out=carry)
                assert hip.rows_launches() - l0 == 1, what
                outs = dst.read(what)
                for r in range(rows):
                    assert_bit_equal(outs[r], want[r], f"{what}, row {r}")
                newest = np.stack([_floats(x)[-2:] if n else (lasts[r] if last is not None else np.zeros(2, np.float32)) for r, x in enumerate(xs)])
                assert_bit_equal(gpu_util.to_host(carry).ravel(), newest.ravel(), what + ": the carried samples")
        if n in (5, 2051):
            for r in sorted({0, rows - 1}):
                assert_bit_equal(exp[r], _fm_one_row(hip, xs[r], lasts[r]), f"fmDemod, n = {n}, row {r}: the oracle vs the one-row call")
    # nothing to write: no launch
    l0 = hip.rows_launches()
    hip.fm_demod_rows(Rows(rows, 0, 2, host=_fm_rows(rows, 0)).view, None, out=Rows(rows, 0, 1).view)
    assert hip.rows_launches() == l0


def test_fm_demod_rows_neighbours_and_carried_sample(hip, oracle):
    """A row of NaN or Inf beside the others; then a stream cut into three calls with d_last_out == d_last_iq: once each call's
    buffer starts at its k_begin (the predecessor is the carried sample), once k_begin > in_base (it is in the buffer, and the
    carried array -- NaN before the call -- is not read)."""
    rows, n = 3, 1027
    xs = _fm_rows(rows, n, seed=50)
    exp = [oracle.fm_demod(_floats(x), (0.0, 0.0)) for x in xs]
    for poison in (np.nan, np.inf):
        bad = [x.copy() for x in xs]
        bad[1][:] = poison
        dst = Rows(rows, n, 1)
        hip.fm_demod_rows(Rows(rows, 2 * n, 2, host=bad).view, None, out=dst.view)
        outs = dst.read()
        for r in (0, 2):
            assert_bit_equal(outs[r], exp[r], f"fmDemod row {r} beside a row of {poison}")
    cuts = [0, 5, 514, n]
    src = Rows(rows, 2 * n, 6, host=xs)
    for from_buffer in (False, True):
        dst = Rows(rows, n, 3)
        carry = torch.zeros((rows, 2), dtype=torch.float32, device="cuda")
        for a, b in zip(cuts[:-1], cuts[1:]):
            if from_buffer:
                if a:
                    carry.fill_(float("nan"))
                hip.fm_demod_rows(src.view, carry, out=dst.view[:, a:b], last_out=carry, in_base=0, k_begin=a, k_end=b)
            else:
                hip.fm_demod_rows(src.view[:, 2 * a: 2 * b], carry, out=dst.view[:, a:b], last_out=carry, in_base=a)
            got = gpu_util.to_host(carry)
            assert_bit_equal(got.ravel(), np.stack([_floats(x)[2 * b - 2: 2 * b] for x in xs]).ravel(), f"carried sample after [{a}, {b})")
        outs = dst.read()
        for r in range(rows):
            assert_bit_equal(outs[r], exp[r], f"fmDemod cut at {cuts[1:-1]}, predecessor from the {'buffer' if from_buffer else 'carried sample'}, row {r}")


# ---- 8: 64-bit row offsets -----------------------------------------------------------------------------------------------------------
def test_row_offsets_are_64_bit(hip, oracle):
    """Two rows 2^31 + 6 floats apart on the input side with tight output rows, then the other way round, n = 129: one buffer of
    about 8.6 GB, allocated uninitialised and touched only at the rows.  A 32-bit row offset would put row 1 somewhere else."""
    stride, n, mu = 2 ** 31 + 6, 129, 0.4
    big = torch.empty(stride + 2 * n + 64, dtype=torch.float32, device="cuda")
    try:
        for op in ("agc", "dc", "fm"):
            width = n if op == "dc" else 2 * n
            if op == "dc":
                xs, states = _many("dc", 2, n)
                exp = [oracle.dc_blocker(x, *st)[0] for x, st in zip(xs, states)]
            elif op == "agc":
                xs, states = _many("agc", 2, n)
                exp = [_floats(agc_model.agc(x, mu, 1.0, st[0])[0]) for x, st in zip(xs, states)]
            else:
                xs, states = _fm_rows(2, n, seed=80), None
                exp = [oracle.fm_demod(_floats(x), (0.0, 0.0)) for x in xs]
            owidth = n if op == "fm" else width
            far = big.as_strided((2, width), (stride, 1))
            far_out = big.as_strided((2, owidth), (stride, 1))
            st = gpu_util.to_dev(np.asarray(states, np.float32).reshape(2, -1)) if states else None
            for use_ws in ((True, False) if op != "fm" else (None,)):
                def call(x, y):
                    if op == "dc":
                        hip.dc_blocker_rows(x, st, 64, out=y, workspace="auto" if use_ws else None)
                    elif op == "agc":
                        hip.agc_rows(x, mu, 1.0, st.view(2), 64, out=y, workspace="auto" if use_ws else None)
                    else:
                        hip.fm_demod_rows(x, None, out=y)
                what = f"{op}, workspace {use_ws}"
                # far input rows, tight output
                for r in range(2):
                    far[r].copy_(torch.from_numpy(_floats(xs[r]).copy()))
                dst = Rows(2, owidth)
                call(far, dst.view)
                outs = dst.read(what)
                for r in range(2):
                    assert_bit_equal(outs[r], exp[r], f"{what}: input rows 2^31 + 6 floats apart, row {r}")
                # tight input, far output rows: canaries around each row
                src = Rows(2, width, host=xs)
                big[:owidth + 32].view(torch.int32).fill_(CANARY)
                big[stride - 32: stride + owidth + 32].view(torch.int32).fill_(CANARY)
                call(src.view, far_out)
                torch.cuda.synchronize()
                for r in range(2):
                    assert_bit_equal(far_out[r].cpu().numpy(), exp[r], f"{what}: output rows 2^31 + 6 floats apart, row {r}")
                near = torch.cat([big[owidth: owidth + 32], big[stride - 32: stride], big[stride + owidth: stride + owidth + 32]])
                assert (near.view(torch.int32) == CANARY).all().item(), f"{what}: floats around the far output rows were written"
    finally:
        del big
        torch.cuda.empty_cache()


# ---- 9: behind the banks ----------------------------------------------------------------------------------------------------------------
def _tuner_bank_rows(hip, oracle):
    """TunerBank, 3 channels, 127 taps (128 padded) / 8, two blocks of 8192 samples -> (bank, device input, expected rows, outputs)."""
    import test_gpu_tuner as T
    import tuner_bank_cases as BC
    import tuner_model as TM
    from oracle import pipes_model as PM
    tables = BC.bank_tables(3)
    x = oracle.convert_u8(T.stream_u8()[:2 * 2 * BC.B])
    exp = [TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, x, t, BC.B, 0, block_out=1) for t in tables]
    n_out = (2 * BC.B - 128) // 8 + 1
    assert all(e.size == 2 * n_out for e in exp)
    return hip.TunerBank(8, S.taps_decim127(), tables), gpu_util.to_dev(x), exp, n_out, BC.B


def test_tuner_bank_rows_into_agc_rows_and_fm_demod_rows(hip, oracle):
    """One stream, no synchronisation: the bank's launch, then agc_rows and fm_demod_rows on its rows where they lie (stride 2 n + 6).
    Expected: the restated Pipe on each mixed stream (tests/tuner_model.py) through agc_model / the oracle's fm_demod."""
    bank, d_in, exp, n, B = _tuner_bank_rows(hip, oracle)
    mu, ref = 0.05, 0.5
    states = np.array([1.0, 0.5, 2.0], np.float32)
    mid = Rows(3, 2 * n, 6)
    agc_out, fm_out = Rows(3, 2 * n, 2), Rows(3, n, 1)
    st = gpu_util.to_dev(states)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())                            # the buffers were filled on the default stream
    l0 = hip.rows_launches()
    with torch.cuda.stream(stream):
        bank.run(d_in.data_ptr(), 0, mid.view.data_ptr(), mid.stride, 0, n, B, stream.cuda_stream)
        hip.agc_rows(mid.view, mu, ref, st, 64, out=agc_out.view, final=st)
        hip.fm_demod_rows(mid.view, None, out=fm_out.view)
    stream.synchronize()
    assert hip.rows_launches() - l0 == 5 + 1
    rows = mid.read("the bank's rows")
    a, f = agc_out.read("agc_rows"), fm_out.read("fm_demod_rows")
    e_agc, e_fin = agc_model.agc(np.stack([e.view(np.complex64) for e in exp]), mu, ref, states)
    assert np.isfinite(_floats(e_agc)).all()
    for j in range(3):
        assert_bit_equal(rows[j], exp[j], f"channel {j}: the bank's row")
        assert_bit_equal(a[j], _floats(e_agc[j]), f"channel {j}: agc_rows behind the bank")
        assert_bit_equal(f[j], oracle.fm_demod(exp[j], (0.0, 0.0)), f"channel {j}: fm_demod_rows behind the bank")
    assert_bit_equal(gpu_util.to_host(st), e_fin, "agc_rows behind the bank: final states")


def test_fm_bank_audio_rows_into_dc_blocker_rows(hip, oracle):
    """FmBank (3 stations, 20 source blocks) and dc_blocker_rows on its audio rows, one stream, no synchronisation.  Expected: the
    oracle's dc_blocker on each audio row (the rows themselves are held to their chains in tests/test_gpu_fm_bank.py)."""
    import test_gpu_fm_bank as FB
    import test_gpu_tuned_chain as T
    names = ["shift -3/1000", "shift 5/8313", "shift 1/4"]
    total = 20 * T.B
    d = T.stream_dev()
    bank = FB._bank(hip, names)
    q0, q1, _ = bank.plan(0, total, total)
    n = q1 - q0
    assert n == 5994
    bank.set_route(1)
    audio, out = Rows(3, n, 3), Rows(3, n, 1)
    st = torch.zeros((3, 2), dtype=torch.float32, device="cuda")                # the Pipe's start, Filter.hs:730-739
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())                            # the buffers were filled on the default stream
    b0, l0 = hip.fm_bank_launches(), hip.rows_launches()
    with torch.cuda.stream(stream):
        bank.run(d.data_ptr(), 0, total, audio.view.data_ptr(), audio.stride, q0, q1, None, 0, stream.cuda_stream)
        hip.dc_blocker_rows(audio.view, st, 512, out=out.view, final=st)
    stream.synchronize()
    assert hip.fm_bank_launches() == b0 + 1 and hip.rows_launches() - l0 == 5
    rows, got, fin = audio.read("the bank's audio"), out.read("dc_blocker_rows"), gpu_util.to_host(st)
    assert not np.array_equal(rows[0], rows[1])
    for j in range(3):
        e, fs, fo = oracle.dc_blocker(rows[j], 0.0, 0.0)
        assert_bit_equal(got[j], e, f"station {j}: dc_blocker_rows behind the bank")
        assert_bit_equal(fin[j], np.array([fs, fo], np.float32), f"station {j}: final state")
