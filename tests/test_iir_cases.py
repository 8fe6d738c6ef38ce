"""CPU: the table of tests/iir_cases.py reaches what it is there for -- shown from the sequential models (the oracle's dcBlocker,
tests/agc_model.py), the scheme model and the library's plan hooks alone: no launch, no device.

Reach conditions, not measurements: each says that a named mistake in a kernel WOULD change the expected output of the case built
for it (so the GPU comparison in tests/test_gpu_iir.py would see it), or that the scheme model finds the table to contain the
chunk patterns the statistics assertions need."""
import dataclasses
import os
from fractions import Fraction

import numpy as np
import pytest

import agc_model
import iir_cases as IC

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def lib():
    from sdr_amd import build as B
    if not os.path.exists(B.LIB):
        B.build()
    import sdr_amd.lib as L
    return L


@pytest.fixture(scope="module")
def schemes(lib, oracle):
    return {c.name: IC.scheme(c, IC.plan_of(lib, c), oracle) for c in IC.CASES}


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _differ(a, b):
    """How many elements differ, +0 and -0 counted as equal."""
    a, b = _f32(a), _f32(b)
    return int((~IC.same(a, b) & ~((a == 0) & (b == 0))).sum())


# ---- every case -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IC.CASES, ids=[c.name for c in IC.CASES])
def test_case_reaches_what_it_is_for(case, schemes):
    s = schemes[case.name]
    print(f"{case.name}: {case.reach}\n    {s.describe()}")
    out = _f32(np.ascontiguousarray(s.out).view(np.float32))
    finite = np.isfinite(out)
    assert bool(np.isnan(out).any()) == (not case.bitwise), "bitwise <=> the expected output holds no NaN"
    assert bool((~finite).any()) == case.nonfinite
    assert case.op == "dc" or finite.all(), "agc on a non-finite trajectory is out of contract"
    if case.nonfinite:
        assert finite.mean() >= 0.5, "at least half of the expected outputs are finite"
        first = int(np.nonzero(~finite)[0][0])
        assert not finite[first:].any(), "once poisoned, for good"
        edges = np.arange(1, s.chunks) * s.C
        assert s.chunks and (edges < first).any() and (edges > first).any(), "a chunk boundary in each part"
        lanes_after = edges[edges - s.W > first + 2]                      # lanes that never see the event speculate a finite state
        assert lanes_after.size >= 8 and s.wrong[lanes_after // s.C].all()
    assert IC.same(s.final[-1], IC.model(case, None).states[-1])


# ---- dcBlocker: what a restated step would change -------------------------------------------------------------------------------------
def _dc_inputs(case, oracle):
    """(d, y_prev, y) of every step of the case: the f32 difference, the state before, the state after (the oracle's)."""
    m = IC.model(case, oracle)
    x = IC.stream(case)
    xp = np.concatenate([_f32([case.state[0]]), x[:-1]])
    with np.errstate(over="ignore", invalid="ignore"):
        d = x - xp
    return x, xp, d, m.states[:-1], m.states[1:]


def _fma_step_exact(d, yp):
    """(float)fma(0.997, (double)y, (double)d): the product is not rounded.  Rationals; Fraction -> float rounds correctly."""
    c = Fraction(0.997)
    return _f32([float(Fraction(float(a)) + c * Fraction(float(b))) for a, b in zip(d, yp)])


def test_cancellation_stream_is_its_own_dc_blocker_run(oracle):
    x, y = IC.cancellation(4001, 11)
    out, _, _ = oracle.dc_blocker(x, *IC.DC_STATE)
    assert IC.same(out, y).all(), "the generator's step (Python scalars) is the oracle's"
    assert np.array_equal(x, IC.stream(IC.BY_NAME["dc/cancel-default"])[:4001])


def test_a_fused_multiply_add_shows_on_the_cancellation_stream_only(oracle):
    case = IC.BY_NAME["dc/cancel-default"]
    _, _, d, yp, y = _dc_inputs(case, oracle)
    hits = _differ(_fma_step_exact(d, yp), y)
    print(f"cancellation stream, n = {case.n}: an f64 FMA changes {hits} outputs")
    assert hits >= 64
    small = IC.BY_NAME["dc/cancel-w64"]
    _, _, d, yp, y = _dc_inputs(small, oracle)
    hits = _differ(_fma_step_exact(d, yp), y)
    print(f"cancellation stream, n = {small.n}: {hits}")
    assert hits >= 64
    uni = dataclasses.replace(IC.BY_NAME["dc/uniform-default"], name="dc/uniform, the cancellation stream's length", n=case.n)
    _, _, d, yp, y = _dc_inputs(uni, oracle)
    assert _differ(_fma_step_exact(d, yp), y) == 0, "on a uniform stream of the same length an FMA is invisible"


@pytest.mark.parametrize("name", ["dc/cancel-default", "dc/uniform-default", "dc/uniform-w64"])
def test_other_restatements_of_the_step_show_on_ordinary_signals(oracle, name):
    x, xp, d, yp, y = _dc_inputs(IC.BY_NAME[name], oracle)
    d64, y64 = d.astype(np.float64), yp.astype(np.float64)
    spec = (d64 + 0.997 * y64).astype(np.float32)
    assert IC.same(spec, y).all(), "numpy's double arithmetic restates the step"
    f32_const = (d64 + float(np.float32(0.997)) * y64).astype(np.float32)
    double_diff = ((x.astype(np.float64) - xp.astype(np.float64)) + 0.997 * y64).astype(np.float32)
    a, b = _differ(f32_const, y), _differ(double_diff, y)
    print(f"{name}: 0.997f changes {a} outputs, the difference in double {b}")
    assert a >= 64 and b >= 64


def test_value_class_streams_do_what_they_say(oracle):
    n_at = IC.POISON_AT
    for kind, first_bad, value in (("inf", n_at, np.inf), ("ninf", n_at, -np.inf), ("nan", n_at, np.nan), ("inf_inf", n_at, np.inf),
                                   ("diff_overflow", n_at + 1, -np.inf), ("cast_overflow", n_at + 1, np.inf)):
        x, xp, d, yp, y = _dc_inputs(IC.BY_NAME["dc/" + kind], oracle)
        assert np.isfinite(y[:first_bad]).all() and IC.same(y[first_bad], np.float32(value)), kind
        if kind in ("inf", "ninf", "inf_inf"):
            assert np.isnan(y[n_at + 1:]).all(), kind
        if kind == "inf_inf":
            assert np.isnan(d[n_at + 1]) and np.isinf(x[n_at]) and np.isinf(x[n_at + 1]), "Inf - Inf"
        if kind == "diff_overflow":
            assert np.isfinite(x).all() and d[first_bad] == -np.inf, "finite samples, an infinite difference"
            assert (y[first_bad:] == -np.inf).all(), "sticky, and no NaN"
        if kind == "cast_overflow":
            assert np.isfinite(d).all(), "every difference is finite"
            assert np.isfinite(float(d[first_bad]) + 0.997 * float(yp[first_bad])), "so is the f64 sum: the f32 rounding overflows"
            assert (y[first_bad:] == np.inf).all(), "sticky, and no NaN"
    x, xp, d, yp, y = _dc_inputs(IC.BY_NAME["dc/subnormal"], oracle)
    sub = (np.abs(d) < 2.0 ** -126) & (d != 0)
    assert sub.sum() >= 2000 and np.isfinite(y).all()


def test_fixed_point_sticks_in_the_subnormals(oracle):
    case = IC.BY_NAME["dc/fixed-point"]
    _, _, d, yp, y = _dc_inputs(case, oracle)
    assert (d == 0).all()
    stuck = int(np.nonzero(y.view(np.uint32) == (0x80000000 | 166))[0][0])
    print(f"fixed point: -166 subnormal units from sample {stuck} on")
    assert stuck < case.n // 2 + 16384 and (y[stuck:].view(np.uint32) == (0x80000000 | 166)).all()
    assert float(IC.dc_step(0.75, 0.75, 0.0)) == 0.0, "a lane started from 0 stays there"
    then = IC.BY_NAME["dc/fixed-then-noise"]
    _, _, _, yp, y = _dc_inputs(then, oracle)
    noise_from = then.stream[2]
    assert (yp[:noise_from + 1].view(np.uint32) == 166).all() and noise_from % 256 not in (0, 255)


# ---- agc: what a restated step would change -----------------------------------------------------------------------------------------
def _agc_steps(case):
    """Per sample: the corrected parts, the state before and after (the model's), mu and the reference as float32."""
    m = IC.model(case, None)
    x = IC.stream(case)
    s = m.states[:-1]
    with np.errstate(over="ignore", under="ignore"):
        re, im = _f32(x.real) * s, _f32(x.imag) * s
    return re, im, s, m.states[1:], np.float32(case.mu), np.float32(case.reference)


def _update(s, mu, ref, m):
    with np.errstate(over="ignore", invalid="ignore"):
        return s + mu * (ref - m)


def _variants(case):
    re, im, s, nxt, mu, ref = _agc_steps(case)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        assert IC.same(_update(s, mu, ref, agc_model.magnitude(re, im)), nxt).all(), "one vectorised step restates the model"
        naive = _update(s, mu, ref, np.sqrt(re * re + im * im))
        _, er = np.frexp(re)
        _, ei = np.frexp(im)
        k = np.maximum(er, ei)
        a, b = np.ldexp(re, -k), np.ldexp(im, -k)
        # fmaf(a, a, b * b): a * a is exact in double (48 bits); the sum with the rounded f32 square b * b is exact there too unless
        # the exponents are more than 29 apart, where double's own rounding could only matter on an exact f32 tie
        fused = (a.astype(np.float64) * a.astype(np.float64) + (b * b).astype(np.float64)).astype(np.float32)
        fma_sqrt = _update(s, mu, ref, np.ldexp(np.sqrt(fused), k))
        t = ref - agc_model.magnitude(re, im)
        fma_state = (np.float64(mu) * t.astype(np.float64) + s.astype(np.float64)).astype(np.float32)       # fmaf(mu, t, s), as above
    return {"naive sqrtf(re*re + im*im)": _differ(naive, nxt), "fmaf(a, a, b*b) under the root": _differ(fma_sqrt, nxt),
            "the state update as one fma": _differ(fma_state, nxt)}, (re, im)


def test_agc_variants_show_on_the_cases_built_for_them():
    hits, (re, im) = _variants(IC.BY_NAME["agc/range-w64"])
    print(f"agc range: {hits}")
    assert hits["naive sqrtf(re*re + im*im)"] >= case_quarter(IC.BY_NAME["agc/range-w64"]) // 2
    with np.errstate(over="ignore", under="ignore"):
        overflow = np.isinf(re * re) | np.isinf(im * im)
    sub = ((np.abs(re) < 2.0 ** -126) & (re != 0)) | ((np.abs(im) < 2.0 ** -126) & (im != 0))
    print(f"agc range: a square overflows on {overflow.mean():.3f} of the samples, a corrected part is subnormal on {int(sub.sum())}")
    assert overflow.mean() >= 0.25 and sub.sum() >= 64
    both = (np.abs(re) < 2.0 ** -126) & (np.abs(im) < 2.0 ** -126) & (re != 0) & (im != 0)
    assert both.sum() >= 16, "samples whose two corrected parts are subnormal: the larger exponent comes from a normalised subnormal"
    hits, _ = _variants(IC.BY_NAME["agc/noise-default"])
    print(f"agc noise: {hits}")
    assert hits["fmaf(a, a, b*b) under the root"] >= 64 and hits["the state update as one fma"] >= 64
    hits, (re, im) = _variants(IC.BY_NAME["agc/subnormal-parts"])
    sub = (np.abs(re) < 2.0 ** -126) & (re != 0) & (np.abs(im) < 2.0 ** -126) & (im != 0)
    print(f"agc subnormal parts: {hits}; both corrected parts subnormal on {int(sub.sum())} samples")
    assert sub.sum() >= case_quarter(IC.BY_NAME["agc/subnormal-parts"]), "most samples have both corrected parts subnormal"
    assert hits["naive sqrtf(re*re + im*im)"] >= sub.sum() // 2, "squares of subnormal parts underflow to 0, and here the state shows it"


def case_quarter(case):
    return case.n // 4


# ---- what the scheme model finds in the table ---------------------------------------------------------------------------------------------
def test_table_holds_the_chunk_patterns_the_statistics_need(schemes):
    def where(op, pred):
        return [c.name for c in IC.CASES if c.op == op and pred(c, schemes[c.name])]

    for c in IC.CASES:
        s = schemes[c.name]
        assert s.left == 0 or s.rewritten > 0
        if s.never_merging_run(IC.ROUNDS + 1):
            assert s.left > 0, f"{c.name}: more never-merging chunks in a row than rounds, yet the model spares the walk"
    either = lambda pred: where("dc", pred) + where("agc", pred)
    run1 = either(lambda c, s: s.longest_run == 1)
    run3 = either(lambda c, s: s.longest_run == 3)
    run8 = either(lambda c, s: s.never_merging_run(8))
    inside = where("dc", lambda c, s: any(end < c.n and end % s.C != 0 for _, end in s.walks))
    to_end = where("dc", lambda c, s: any(end == c.n for _, end in s.walks))
    crossing = where("agc", lambda c, s: any((end - 1) // s.C - first // s.C >= 2 for first, end in s.walks))
    clean = {op: where(op, lambda c, s: s.chunks > 0 and s.n_wrong == 0) for op in ("dc", "agc")}
    print(f"longest run exactly 1: {run1}\nexactly 3: {run3}\nat least 8, never merging: {run8}\nwalk meets the stored trajectory inside "
          f"a chunk: {inside}\nwalk runs to the last sample: {to_end}\nagc walk over two boundaries: {crossing}\nnothing starts wrong: {clean}")
    assert run1 and run3 and run8 and inside and to_end and crossing
    assert len(clean["dc"]) >= 3 and len(clean["agc"]) >= 3
    assert "dc/fixed-point" in to_end and "dc/fixed-then-noise" in inside
    assert all(schemes[name].left > 0 for name in run8)


# ---- the plan hooks -------------------------------------------------------------------------------------------------------------------------
def test_route_changes_at_two_run_ins(lib):
    for W in (4, 8, 64, 1024, 12288, 40_000):
        for plan in (lambda n: lib.dc_plan(n, W), lambda n: lib.agc_plan(n, 0.4, W))[:2 if W % 8 == 0 else 1]:
            chunks, C, used = plan(2 * W)
            assert used == W and chunks == -(-2 * W // C) and chunks >= 1
            assert plan(2 * W - 1)[0] == 0 and plan(2 * W + 1)[0] == -(-(2 * W + 1) // C)
    assert lib.dc_plan(24_575)[0] == 0 and lib.dc_plan(24_576) == (96, 256, 12288), "the default run-in"
    assert lib.dc_plan(0) == (0, 256, 12288) and lib.agc_plan(0, 0.5)[0] == 0


def test_run_in_is_rounded_up(lib):
    for run_in, used in ((1, 4), (5, 8), (61, 64), (64, 64), (65, 68)):
        assert lib.dc_plan(1 << 16, run_in)[2] == used
    for run_in, used in ((1, 8), (12, 16), (61, 64), (64, 64), (65, 72)):
        assert lib.agc_plan(1 << 16, 0.5, run_in)[2] == used
    # a block two RAW run-ins long is shorter than two rounded ones
    assert lib.dc_plan(122, 61)[0] == 0 and lib.dc_plan(128, 61)[0] == 1
    assert lib.agc_plan(122, 0.5, 61)[0] == 0 and lib.agc_plan(128, 0.5, 61)[0] == 1


@pytest.mark.parametrize("run_in", [INT_MAX, INT_MAX - 1, INT_MAX - 2, INT_MAX - 3, INT_MAX - 7])
def test_a_run_in_near_int_max_takes_the_sequential_walk(lib, run_in):
    """Rounded up it passes INT_MAX: the plan keeps it in 64 bits and decides the route first.  This is the whole regression check:
    nothing launches a kernel with such a value."""
    rounded4, rounded8 = (run_in + 3) // 4 * 4, (run_in + 7) // 8 * 8
    for n in (1, 4096, 1 << 16, 1 << 31, (1 << 32) - 17):
        chunks, _, used = lib.dc_plan(n, run_in)
        assert (chunks, used) == (0, rounded4), (n, chunks, used)
        chunks, _, used = lib.agc_plan(n, 0.5, run_in)
        assert (chunks, used) == (0, rounded8), (n, chunks, used)
    n = 1 << 33                                                # where two such run-ins do fit, the plan says so with a positive run-in
    chunks, C, used = lib.dc_plan(n, run_in)
    assert used == rounded4 > 0 and chunks == -(-n // C) > 0
