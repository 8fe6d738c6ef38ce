"""CPU: what the table of tests/fir_rows_cases.py reaches, from the seam model (tests/stream_slice_cases.py) and the plan hook
(host arithmetic of the library: no device) alone."""
import os

import numpy as np
import pytest

import fir_rows_cases as RC
import stream_slice_cases as SC


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


@pytest.fixture(scope="module")
def resolved(L):
    return [(c, RC.resolve(L, c)) for c in RC.CASES]


def test_every_dimension_occurs_in_every_banked_family(resolved):
    for f in RC.FAMILIES:
        mine = [(c, g) for c, g in resolved if c.family is f and c.first < 0]
        assert {c.rows for c, _ in mine} == set(RC.ROWS), f.name
        assert {c.size for c, _ in mine} == set(RC.SIZES), f.name
        assert {c.seam_kind for c, _ in mine} == {"none", "min", "three"}, f.name
        assert {c.pos for c, _ in mine} == {"zero", "forty", "far"}, f.name
        assert {c.layout for c, _ in mine} == {0, 1, 2}, f.name
        if f.kind == "resampler":
            assert {c.out_block for c, _ in mine} == {97, 1000}, f.name
    banked = [c for c, _ in resolved if c.family.banked and c.first < 0]
    assert {(c.rows, c.size) for c in banked} == {(r, s) for r in RC.ROWS for s in RC.SIZES}
    # chunk counts: per data type one exact count (8 or 16: where k_split has a guard-free instantiation, real data only) and one that is not
    for cplx in (False, True):
        chunks = {f.chunks for f in RC.FAMILIES if f.banked and f.complex_ == cplx}
        assert chunks & {8, 16} and chunks - {8, 16, 32}, (cplx, chunks)
    assert any(f.sym for f in RC.FAMILIES) and {f.order for f in RC.FAMILIES} == {RC.AVX, RC.SSE, RC.SCALAR}


def test_positions_and_layouts(resolved):
    for c, g in resolved:
        f = c.family
        first = int(SC.in_offset(g.k_begin, f.I, f.D))
        if c.pos == "zero":
            assert g.in_base == 0 and g.S == 0
        else:
            assert first - g.in_base == 1 and first >= 41, c.name
        if c.pos == "far":
            assert g.S > 1 << 33 and g.T * f.D == g.S * f.I and g.T % f.I == 0, c.name
            assert g.seam == 0 or (g.S % g.seam == 0), c.name
            assert c.out_block == 0 or g.T % c.out_block == 0, c.name
            assert int(SC.in_offset(g.k_begin + g.T, f.I, f.D)) == first + g.S
        gi, go, oi, oo = c.layout_floats
        if f.complex_:
            assert gi % 2 == 0 and go % 2 == 0 and oi % 2 == 0 and oo % 2 == 0
    assert {c.layout_floats[2] * 4 % 16 for c, _ in resolved if not c.family.complex_} >= {0, 4, 8}
    assert {c.layout_floats[2] * 4 % 16 for c, _ in resolved if c.family.complex_} >= {0, 8}


def test_seams_cross_outputs_and_the_resamplers_corner_cases(resolved):
    late = no_cross = seam_without_cross_output = 0
    for c, g in resolved:
        f = c.family
        edges = RC.seams_inside(f, g.k_begin, g.k_end, g.seam)
        cross = RC.cross_mask(f, g.k_begin, g.k_end, g.seam, c.out_block)
        if c.seam_kind == "none":
            assert g.seam == 0 and not edges and not cross.any()
            continue
        assert g.seam * f.I >= f.Lp and f.Lp >= f.D, c.name                      # what the one-row call asks of a seam block
        if c.seam_kind == "min":
            assert g.seam == f.min_seam
        elif c.seam_kind == "three":
            assert len(edges) >= 3, (c.name, edges)
        assert cross.any(), f"{c.name}: no Cross output in the range"
        m = np.arange(g.k_begin, g.k_end, dtype=np.int64)
        v = m * f.D
        for e in edges:
            straddle = (v < e) & (v + f.Lp > e)
            if not (straddle & cross).any():
                seam_without_cross_output += 1
                assert f.I > 1, f"{c.name}: a filter / decimator seam inside the range always has a straddler (Lp > D)"
            if not SC.seam_has_crossover(np.int64(e), f.I, f.D, f.Lp):
                no_cross += 1
                continue
            late += int((straddle & SC.late_output_is_one(m, np.int64(e), f.I, f.D, c.out_block)).sum())
    assert late > 0, "no case hits late_output_is_one"
    assert no_cross > 0, "no case has a seam without crossover"
    assert seam_without_cross_output > 0
    # the directed pair: output 1843 is One with output blocks of 97 and Cross without
    a, b = [(c, g) for c, g in resolved if c.first >= 0]
    assert a[1].k_begin <= 1843 < a[1].k_end and (a[1].k_begin, a[1].k_end, a[1].seam) == (b[1].k_begin, b[1].k_end, b[1].seam)
    assert not RC.cross_mask(a[0].family, 1843, 1844, a[1].seam, 97)[0] and RC.cross_mask(b[0].family, 1843, 1844, b[1].seam, 0)[0]


def test_plans_reach_both_tile_paths_and_both_lane_plans(resolved):
    full = partial = 0
    per_lane = set()
    for c, g in resolved:
        if not c.family.banked:
            assert g.plan is None and g.tile == 0, f"{c.name}: a fallback case inside the banked shapes"
            continue
        p = g.plan
        assert p is not None, c.name
        per_lane.add(p["per_lane"])
        tile = p["tile_outputs"]
        assert p["tiles_per_row"] == -(-(-(-g.n // p["per_cycle"])) // p["cycles_per_tile"])
        whole, rest = divmod(g.n, tile)
        full += whole > 0
        partial += rest > 0
        expect_tiles = {"one": 1, "lane group - 1": 1, "tile": 1, "tile + 1": 2, "3 tiles - 1": 3}.get(c.size)
        if expect_tiles:
            assert p["tiles_per_row"] == expect_tiles, (c.name, p)
        if c.size == "tile":
            assert g.n == tile == g.tile and rest == 0, (c.name, p)
        if c.size in ("one", "lane group - 1"):
            assert p["per_lane"] == 1 and tile < g.tile, (c.name, p)
    assert full and partial and per_lane == {1, 2}
