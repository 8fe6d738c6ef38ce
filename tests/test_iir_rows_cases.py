"""CPU: the row sets of tests/iir_rows_cases.py reach what they are there to reach -- shown from the sequential models, the scheme
model (iir_cases.scheme) and the library's rows plan hooks alone: no launch, no device.  tests/test_gpu_rows.py then holds every row
of a launch to these expectations: output, final state and statistics words."""
import os

import numpy as np
import pytest

import iir_cases as IC
import iir_rows_cases as RC


@pytest.fixture(scope="module")
def lib():
    from sdr_amd import build as B
    if not os.path.exists(B.LIB):
        B.build()
    import sdr_amd.lib as L
    return L


def _f32(a):
    return np.ascontiguousarray(a).view(np.float32)


def _stats(s):
    return (s.left, s.rewritten, s.repaired)


def test_agc_rows_take_all_three_branches_in_one_launch(lib, oracle):
    rs = RC.AGC_BRANCHES
    assert RC.plan_of(lib, rs) == (9, 512, 512) == lib.agc_plan(rs.n, rs.mu, rs.run_in)
    quiet, repaired, walked, silent = RC.schemes(lib, rs, oracle)
    for s in (quiet, repaired, walked, silent):
        print("    " + s.describe())
        assert not s.nan_starts and np.isfinite(_f32(s.out)).all()
    assert quiet.n_wrong == 0 and _stats(quiet) == (0, 0, 0)
    assert repaired.n_wrong == 7 and _stats(repaired) == (0, 0, 7), "seven start wrong, the rounds recompute each once, none is left"
    for s in (walked, silent):
        assert s.n_wrong == 7 and _stats(s) == (4, 1540, 18) and s.walks == [(2560, 4100)]
    assert not np.any(_f32(silent.out)), "a silent row: every output is zero whatever the state, only the state tells"
    assert len({_stats(s) for s in (quiet, repaired, walked)}) == 3, "per-row statistics that differ"
    finals = [float(s.final[0]) for s in (quiet, repaired, walked, silent)]
    assert len(set(finals)) == 4 and max(finals) > 1000 > 100 > min(finals), "final states orders of magnitude apart"


def test_dc_rows_walk_to_the_end_to_the_next_chunk_and_into_the_noise(lib, oracle):
    rs = RC.DC_BRANCHES
    assert RC.plan_of(lib, rs) == (9, 256, 64) == lib.dc_plan(rs.n, rs.run_in)
    uniform, cancel, fixed = RC.schemes(lib, rs, oracle)
    for s in (uniform, cancel, fixed):
        print("    " + s.describe())
        assert not s.nan_starts
    assert uniform.walks == [(1024, 2051)] and uniform.rewritten == 1027
    assert cancel.walks == [(1024, 1280)] and cancel.rewritten == 256, "the walk meets the stored trajectory a chunk on"
    assert fixed.walks == [(1024, 1636)] and fixed.rewritten == 612, "... and here where the noise begins"
    assert len({_stats(s) for s in (uniform, cancel, fixed)}) == 3
    assert rs.rows[2][1] != rs.rows[0][1], "the rows start from states of their own"


@pytest.mark.parametrize("rs", RC.EDGES, ids=[s.name for s in RC.EDGES])
def test_plan_edges(lib, oracle, rs):
    chunks = {127: 0, 128: 1, 129: 1, 0: 0, 1: 0, 7: 0}[rs.n]
    plan = RC.plan_of(lib, rs)
    assert plan[0] == chunks and plan[2] == 64
    assert plan == (lib.dc_plan(rs.n, 64) if rs.op == "dc" else lib.agc_plan(rs.n, rs.mu, 64))
    ss = RC.schemes(lib, rs, oracle)
    width = 1 if rs.op == "dc" else 2
    assert all(_f32(s.out).size == width * rs.n for s in ss)
    states = [c.state for c in rs.cases()]
    assert len(set(states)) == len(states), "every row starts from a state of its own"
    if rs.n == 0:
        for s, st in zip(ss, states):
            assert np.array_equal(np.asarray(s.final, np.float32).ravel(), np.asarray(st, np.float32)), "n == 0 hands the state on"
    else:
        finals = {tuple(np.asarray(s.final, np.float32).ravel().view(np.uint32)) for s in ss}
        assert len(finals) == len(ss), "a row that took its neighbour's state or stream would show in its final state"


@pytest.mark.parametrize("rs", [RC.AGC_RANGE, RC.AGC_SUBNORMAL], ids=lambda s: s.name)
def test_value_class_rows(lib, oracle, rs):
    assert RC.plan_of(lib, rs) == (9, 256, 64)
    ss = RC.schemes(lib, rs, oracle)
    cases = rs.cases()
    for c, s in zip(cases, ss):
        print(f"    {c.stream}: {s.describe()}")
        assert np.isfinite(_f32(s.out)).all() and np.isfinite(s.final).all() and not s.nan_starts
        assert s.left > 0 and s.repaired > 0, "both the rounds and the walk have work on every row"
    tiny = np.finfo(np.float32).tiny
    for c, s in zip(cases, ss):
        out = _f32(s.out).astype(np.float64)
        parts = np.abs(out)
        sub = (parts > 0) & (parts < tiny)
        with np.errstate(over="ignore"):
            naive = (out[0::2].astype(np.float32) ** 2 + out[1::2].astype(np.float32) ** 2)
        if c.stream[0] == "agc_range":
            assert np.isinf(naive).sum() >= 64, "squares overflow: only the scaled magnitude is right"
            assert sub.sum() >= 16, "and some corrected parts are subnormal"
        elif c.stream[0] == "agc_subnormal":
            assert (sub | (parts == 0)).all() and sub.mean() > 0.9, "every corrected part is subnormal"
            assert not np.any(naive), "squared where they stand, the parts underflow to zero"
        else:
            assert np.isfinite(naive).all() and not sub.any(), "the ordinary row beside them"
    assert len({_stats(s) for s in ss}) > 1 or len({float(s.final[0]) for s in ss}) == len(ss)


def test_rows_of_a_set_differ(lib, oracle):
    """A kernel that read row 0 for every row, or wrote every row to row 0, would not pass: no two rows of a set of n >= 7 expect the same."""
    for rs in RC.SETS:
        if rs.n < 7:
            continue
        outs = [_f32(s.out) for s in RC.schemes(lib, rs, oracle)]
        for a in range(len(outs)):
            for b in range(a + 1, len(outs)):
                assert (outs[a].view(np.uint32) != outs[b].view(np.uint32)).mean() > 0.9, (rs.name, a, b)
