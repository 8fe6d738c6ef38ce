"""CPU: what the tables of tests/rows_limit_cases.py reach -- shown from the library's plan hooks (host arithmetic: no launch, no
device), the sequential models, the scheme model (iir_cases) and the restated Pipes alone.  tests/test_gpu_rows_limits.py and
tests/test_gpu_fir_rows_classes.py then hold the device to these expectations."""
import os

import numpy as np
import pytest

import fir_rows_cases as RC
import rows_limit_cases as LC
import value_classes as VC


@pytest.fixture(scope="module")
def lib():
    from sdr_amd import build as B
    if not os.path.exists(B.LIB):
        B.build()
    import sdr_amd.lib as L
    return L


# ---- A ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["agc", "dc"])
def test_iir_shapes_sit_at_the_lane_cap_as_stated(lib, op):
    for sh in LC.IIR_SHAPES:
        plan, one = LC.plans(lib, op, sh)
        print(f"    {op}, {sh.name}: rows plan {plan}, one-row plan {one}, {sh.rows * plan[0]} lanes ({sh.what})")
        assert plan == sh.plan and one[0] == sh.one_row[0], (sh.name, plan, one)
        if not plan[0]:
            assert sh.n < 2 * plan[2] and one[0] == 0
            continue
        assert one == sh.one_row and plan[1] % 8 == 0 and plan[2] == LC.RUN_IN
        assert sh.rows * plan[0] <= LC.LANE_CAP < sh.rows * -(-sh.n // (plan[1] - 8)), "a chunk 8 samples shorter passes the cap"
        assert sh.grown == (sh.rows * one[0] > LC.LANE_CAP) == (plan != one)
        assert len(sh.subset) >= 8 and {0, sh.rows - 1} <= set(sh.subset) and max(sh.subset) < sh.rows
    at_cap, grown, odd, seq = LC.IIR_SHAPES
    assert at_cap.rows * at_cap.plan[0] == LC.LANE_CAP and not at_cap.grown
    assert grown.grown and grown.n - (grown.plan[0] - 1) * grown.plan[1] == 9, "the last chunk is 9 samples"
    assert odd.grown and odd.rows % 2 and odd.plan[0] % 2 and odd.rows * odd.plan[0] == 32319
    # rows either side of a wave boundary of the packed lanes are checked
    for sh in (at_cap, grown, odd):
        assert any((a * sh.plan[0]) % 64 == 0 and a - 1 in sh.subset for a in sh.subset if a), sh.name


@pytest.mark.parametrize("shape", LC.IIR_SHAPES[:3], ids=[s.name for s in LC.IIR_SHAPES[:3]])
def test_agc_checked_rows_take_all_three_branches(lib, oracle, shape):
    plan, one = LC.plans(lib, "agc", shape)
    t = LC.truth("agc", shape, oracle)
    assert all(np.isfinite(o).all() for o in t.outs) and np.isfinite(t.finals).all()
    quiet, repaired, walked, differ = [], [], [], []
    for r in shape.subset:
        s = LC.row_scheme("agc", shape, r, plan, oracle)
        s1 = LC.row_scheme("agc", shape, r, one, oracle)
        print(f"    agc, {shape.name}, row {r}: {LC.stats_of(s)}, under the one-row plan {LC.stats_of(s1)}; {s.describe()}")
        assert not s.nan_starts
        (quiet if s.n_wrong == 0 else repaired if s.left == 0 else walked).append(r)
        if LC.stats_of(s)[:3] != LC.stats_of(s1)[:3]:
            differ.append(r)
    print(f"    no chunk wrong: rows {quiet}; repaired by the rounds: {repaired}; left to the settling walk: {walked}")
    assert quiet and repaired and walked
    assert all(LC.row_scheme("agc", shape, r, plan, oracle).repaired > 0 for r in repaired + walked)
    assert bool(differ) == shape.grown, "under the grown plan the statistics words tell the two plans apart"
    assert any(r % 8 == 7 for r in walked) and not np.any(t.outs[7]), "a silent row: only the state tells"
    assert len({t.outs[r].tobytes() for r in shape.subset}) == len(shape.subset)


@pytest.mark.parametrize("shape", LC.IIR_SHAPES[:3], ids=[s.name for s in LC.IIR_SHAPES[:3]])
def test_dc_checked_rows_walk_to_the_end_and_into_the_stored_trajectory(lib, oracle, shape):
    plan, one = LC.plans(lib, "dc", shape)
    meets, runs_on, differ = [], [], []
    for r in shape.subset:
        s = LC.row_scheme("dc", shape, r, plan, oracle)
        s1 = LC.row_scheme("dc", shape, r, one, oracle)
        print(f"    dc, {shape.name}, row {r}: {LC.stats_of(s)}, under the one-row plan {LC.stats_of(s1)}; walks {s.walks}")
        assert not s.nan_starts and s.left > 0 and s.repaired > 0
        if any(b < shape.n for _, b in s.walks):
            meets.append(r)
        if any(b == shape.n for _, b in s.walks):
            runs_on.append(r)
        if LC.stats_of(s)[:3] != LC.stats_of(s1)[:3]:
            differ.append(r)
    print(f"    a walk meets the stored trajectory: rows {meets}; a walk runs to the end: rows {runs_on}")
    assert meets and all(LC.fixed_row(r) for r in meets) and len(runs_on) > len(meets)
    assert bool(differ) == shape.grown
    t = LC.truth("dc", shape, oracle)
    assert len({t.outs[r].tobytes() for r in shape.subset}) == len(shape.subset)


def test_rows_follow_the_recipe_and_differ():
    xs, states = LC.many("agc", 1024, 100)
    assert [float(np.abs(x).max() == 0) for x in xs[:16]] == [0, 0, 0, 0, 0, 0, 0, 1] * 2, "every eighth row is silent"
    assert len({s for s in states}) == 1024 and min(LC.AGC_LEVELS[:7]) == 0.01
    xs, states = LC.many("dc", 1024, 100)
    assert sum(LC.fixed_row(r) for r in range(1024)) == 16 and len(set(states)) == 1024 - 15


# ---- B ----------------------------------------------------------------------------------------------------------------------------
def test_fir_1024_cases(lib):
    kinds = set()
    for name in LC.FIR_1024:
        f = RC.BY_NAME[name]
        kinds.add((f.kind, f.complex_, f.sym))
        seamed, idle = LC.fir_1024_cases(f)
        for c in (seamed, idle):
            g = RC.resolve(lib, c)
            seams = RC.seams_inside(f, g.k_begin, g.k_end, g.seam)
            cross = RC.cross_mask(f, g.k_begin, g.k_end, g.seam, c.out_block)
            print(f"    {c.name}: plan {g.plan}, {g.n} outputs a row, seam block {g.seam}, {len(seams)} seams inside, {int(cross.sum())} Cross outputs")
            assert c.rows == 1024 == lib.ROWS_MAX and g.plan is not None
            if c is seamed:
                assert g.n == g.tile + 1 and g.plan["tiles_per_row"] == 2 and len(seams) >= 3 and cross.any()
                assert g.plan["per_lane"] == g.plan["split_per_lane"]
            else:
                assert g.n == 64 // f.M * g.plan["per_cycle"] - 1 and g.plan["tiles_per_row"] == 1 and not seams and not cross.any()
                assert g.plan["per_lane"] == 1 and g.n < 64, "one wave's worth of a 256-thread workgroup at most has work"
            a, b = LC.fir_row_stream(c, g, 0), LC.fir_row_stream(c, g, 1023)
            assert a.size == b.size and not np.array_equal(a, b)
    assert kinds == {("decimator", True, False), ("resampler", False, False), ("filter", False, True)}


# ---- C ----------------------------------------------------------------------------------------------------------------------------
def test_class_families_are_the_banked_ones_and_two_with_awkward_taps():
    assert [f.name for f in LC.CLASS_FAMILIES[:9]] == [f.name for f in RC.FAMILIES if f.banked] and len(LC.CLASS_FAMILIES) == 11
    a, b = LC.CLASS_FAMILIES[9:]
    assert not a.complex_ and b.complex_ and all(f.name not in RC.BY_NAME for f in (a, b))
    for f in (a, b):
        t, base = f.taps(), LC.BASE_FAMILY[f.name].taps()
        zeros = np.nonzero(t == 0)[0]
        assert zeros.size == 3 and np.signbit(t[zeros]).any() and not np.signbit(t[zeros]).all() and t[-1] != 0
        assert f.Lp == LC.BASE_FAMILY[f.name].Lp and np.array_equal(np.delete(t, zeros), np.delete(base, zeros))


def _small(a):
    """zero or subnormal"""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) & 0x7FFFFFFF) < 0x00800000


@pytest.mark.parametrize("f", LC.CLASS_FAMILIES, ids=[f.name for f in LC.CLASS_FAMILIES])
def test_fir_class_rows_hold_the_classes_where_the_row_kernels_meet_them(lib, oracle, f):
    w, lp = f.width, f.Lp // f.I
    cross_nan = cross_small_finite = one_nonfinite = 0
    sizes = set()
    for case, g in LC.class_cases(lib, f):
        p = g.plan
        seams = RC.seams_inside(f, g.k_begin, g.k_end, g.seam)
        sizes.add((case.size, bool(seams)))
        if case.size == "short":
            assert p["per_lane"] == 1 and p["cycles_per_tile"] < p["split_cycles_per_tile"] and p["tiles_per_row"] == 1, (case.name, p)
            longer = lib.fir_rows_plan(f.make(lib), g.k_begin, g.k_end + p["per_cycle"], LC.CLASS_ROWS, g.seam)
            assert longer["per_lane"] == 2 or longer["cycles_per_tile"] == longer["split_cycles_per_tile"], "a cycle more leaves the row-only code"
        else:
            assert p["tiles_per_row"] == 3 and (p["per_lane"], p["cycles_per_tile"]) == (p["split_per_lane"], p["split_cycles_per_tile"]), (case.name, p)
        if case.seam_kind == "none":
            assert not seams
        elif case.size == "short" and f.name in LC.TWO_SEAMS_ONLY:
            span = g.n - 1 + f.Lp
            assert len(seams) == 2 and span <= 2 * f.min_seam, f"{case.name}: {span} inputs hold at most two seams {f.min_seam} apart"
        else:
            assert len(seams) >= 3, (case.name, seams)
        xs, planted, exp = LC.class_expected(case, g, oracle)
        assert len(xs) == LC.CLASS_ROWS and all(x.size == xs[0].size for x in xs)
        assert np.isfinite(xs[0]).all() and not _small(xs[0]).any() and np.isfinite(exp[0]).all(), "row 0 is the unsalted one"
        whole = np.concatenate(exp)
        share = VC.nan_share(whole)
        have = VC.classes_present(whole)
        per_row = [VC.nan_share(e) for e in exp]
        print(f"    {case.name}: plan {p}, {g.n} outputs a row from {g.k_begin}, seam block {g.seam}, {len(seams)} seams inside; planted {planted}; "
              f"classes {have}; NaN share {share:.4f}, per row {[round(s, 3) for s in per_row]}")
        VC.assert_not_vacuous(whole, case.name)
        assert share <= 0.10, f"{case.name}: NaN share {share:.3f}"
        assert max(per_row) <= 0.5, f"{case.name}: a row with more than half of its outputs NaN: {per_row}"
        assert len({x.tobytes() for x in xs}) == LC.CLASS_ROWS
        if not seams:
            continue
        cross = RC.cross_mask(f, g.k_begin, g.k_end, g.seam, case.out_block)
        near = LC.beside_a_seam(cross)
        assert cross.any() and near.any()
        first = RC.SC.in_offset(np.arange(g.k_begin, g.k_end), f.I, f.D)
        for x, e in zip(xs[1:], exp[1:]):
            e2 = e.reshape(-1, w)
            cross_nan += int((np.isnan(e2).any(1) & cross).sum())
            one_nonfinite += int((~np.isfinite(e2).all(1) & near).sum())
            for i in np.nonzero(cross & np.isfinite(e2).all(1))[0]:
                cross_small_finite += bool(_small(x[first[i] * w:(first[i] + lp) * w]).any())
    print(f"    {f.name}: Cross outputs that are NaN {cross_nan}; finite Cross outputs whose window holds a zero or a subnormal {cross_small_finite}; "
          f"non-finite One outputs beside a seam {one_nonfinite}")
    assert sizes == {("short", True), ("short", False), ("3 tiles - 1", True), ("3 tiles - 1", False)}
    assert cross_nan > 0 and cross_small_finite > 0 and one_nonfinite > 0
