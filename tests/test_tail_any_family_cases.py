"""What tests/tail_any_family_cases.py reaches, shown on the CPU from the models alone (oracle/pipes_model.py and the seam rule
restated in tests/stream_slice_cases.py).  The only product code here is the predicate, asked through the binding
(AudioTail(...).general_fits(); create needs no device).

  * the restated predicate is the product's over I = 1 .. 9, D = I + 1 .. 50, group lengths 8 .. 72 and half-tap counts 8 .. 72 at
    the blocks 0, lowest - 1, lowest, 2^27 and 2^27 + 1 (nothing thinned: the sweep takes seconds);
  * the table is derived from it: 109 coprime ratios with the per-I maxima 5, 11, 17, 23, 29, 35, 41, 47, every admitted
    (I, group length) and (I, chunk count) pair, the six tap-count edges on I = 1, 3, 5, 6, 8, and the ten shapes whose window sum
    is within 7 of 5120 with their refused neighbours;
  * every seamed launch holds Cross outputs of both stages that differ IN BITS from their grouped values; a resampler of up to
    three products an output cannot (both orders sum them alike): those shapes are told apart on non-finite input, where the
    grouped walk multiplies an infinity by its padded zero taps and the sequential walk does not;
  * the seam rule marks every output the seamed Pipes compute differently; tiles hold two and more boundaries of each stage;
  * every model run the GPU test compares with is defined, finite and nonzero;
  * three planted model changes (a dropped last filter chunk, a Cross walk one term short, the windows of groups g >= 4 one input
    early) each change bits on a launch of every shape they apply to;
  * the far launches need the 64-bit remainder: their tile bases have another remainder once cut to 32 bits, in outputs and in
    upsampled units;
  * the reference's undefined zone is where tail_any_family_cases.asserts says, by search with the restated Pipes on a zero stream
    of forty blocks: inside [lowest_block, lowest_block + D), nothing above it; at most one launch a shape lies inside it."""
import collections
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

import audio_tail_any_cases as AC
import tail_any_family_cases as FC
from oracle import pipes_model as PM

SHAPES = list(FC.SHAPES.values())
ERR_ARG = -1


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differ(a, b):
    return bool((_bits(a) != _bits(b)).any())


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


# ---- the predicate --------------------------------------------------------------------------------------------------------------
def test_the_restated_predicate_is_the_products(L):
    """Where create refuses the block there is no tail to ask: the expected answer is SDRHIP_ERR_ARG from create."""
    asked = collections.Counter()
    taps, halves = {}, {}
    for I in range(1, 10):
        for D in range(I + 1, 51):
            for nloop in range(8, 73, 8):
                r = taps.setdefault(I * nloop, np.full(I * nloop, 0.01, np.float32))
                for nhalf in range(8, 73, 8):
                    a = halves.setdefault(nhalf, np.full(nhalf, 0.01, np.float32))
                    s = FC.Shape("", I, D, I * nloop, nhalf)
                    low = s.lowest_block
                    for block in (0, low - 1, low, 1 << 27, (1 << 27) + 1):
                        h = C.c_void_p()
                        rc = L.lib.sdrhip_audio_tail_create(C.byref(h), L.ORDER_AVX, I, D, L._fp(r), r.size, L._fp(a), a.size, 1.0, block)
                        if not FC.create_admits(s, block):
                            assert rc == ERR_ARG and not h.value, (I, D, nloop, nhalf, block)
                            asked["refused by create"] += 1
                            continue
                        assert rc == 0, (I, D, nloop, nhalf, block, rc)
                        got = L.lib.sdrhip_audio_tail_general_fits(h)
                        L.lib.sdrhip_audio_tail_destroy(h)
                        assert got == int(FC.general_fits(s, block)), (I, D, nloop, nhalf, block, got)
                        asked["fits" if got else "does not fit"] += 1
    print(f"    predicate sweep: {dict(asked)}")
    assert min(asked["fits"], asked["does not fit"], asked["refused by create"]) > 1000                  # every answer is a live one


@pytest.mark.parametrize("nloop", FC.NLOOPS)
def test_the_predicate_through_the_binding_on_tap_counts_inside_a_group_length(L, nloop):
    """The sweep above fills the groups; the predicate reads the tap count only through the group length: every count of a few
    ratios, through AudioTail itself, row_stride and the 64 I cap included."""
    for I, D in ((1, 5), (3, 17), (5, 29), (8, 47)):
        for n in range(max(I * (nloop - 8), 0) + 1, I * nloop + 1):
            s = FC.Shape("", I, D, n, 8)
            assert s.nloop == nloop
            t = L.AudioTail(I, D, s.resamp_taps(), s.audio_half(), block=0)
            assert t.general_fits() == FC.general_fits(s, 0), (I, D, n)


def test_the_table_is_derived_from_the_predicate(L):
    assert len(FC.RATIOS) == 109 and all(np.gcd(I, D) == 1 for I, D in FC.RATIOS)
    assert FC.MAX_D == {1: 5, 2: 11, 3: 17, 4: 23, 5: 29, 6: 35, 7: 41, 8: 47}
    # every ratio twice and more; every admitted (I, group length) and (I, chunk count) pair runs
    per_ratio = collections.Counter((s.I, s.D) for s in SHAPES if "ratio" in FC.KINDS[s.name])
    assert set(per_ratio) == set(FC.RATIOS) and min(per_ratio.values()) >= 2
    assert {(s.I, s.nloop) for s in SHAPES} == FC.ADMITTED_GROUPS == {(I, n) for I in range(1, 9) for n in FC.NLOOPS}
    assert {(s.I, s.nfc) for s in SHAPES} == FC.ADMITTED_CHUNKS == {(I, f) for I in range(1, 9) for f in range(1, 9)}
    assert {s.nhalf for s in SHAPES} == set(range(8, 65, 8))
    assert all(s.resamp_taps()[-1] != 0 and s.resamp_taps().size == s.ntaps and s.audio_half().size == s.nhalf for s in SHAPES)
    for s in SHAPES:
        assert FC.general_fits(s, 0) and FC.general_fits(s, s.lowest_block) and not FC.general_fits(s, s.lowest_block - 1), s.name
    # the tap-count edges
    for kind in FC.EDGE_KINDS:
        have = {s.I for s in SHAPES if kind in FC.KINDS[s.name]}
        assert have >= set(FC.EDGE_INTERPS) - ({1} if kind == "ntaps < I" else set()), (kind, have)
    for s in SHAPES:
        k = FC.KINDS[s.name]
        assert "ntaps == I nloop" not in k or s.ntaps == s.I * s.nloop
        assert "ntaps == I nloop - (I - 1)" not in k or s.ntaps == s.I * s.nloop - (s.I - 1)
        assert "ntaps a multiple of I, not of 8 I" not in k or (s.ntaps % s.I == 0 and s.ntaps % (8 * s.I) != 0)
        assert "ntaps == I" not in k or s.ntaps == s.I
        assert "ntaps < I" not in k or 1 < s.ntaps < s.I
        assert "ntaps == 1" not in k or s.ntaps == 1
    # the window edges, found by search
    found = [(I, D, n, lf) for I in range(1, 9) for D in range(I + 1, 64) for n in FC.NLOOPS for lf in FC.LFS
             if FC.fits(I, D, n, lf) and FC.window_sum(I, D, n, lf) >= 5120 - 7]
    assert found == FC.WINDOW_POINTS and len(found) == 10
    assert max(FC.window_sum(*p) for p in found) == 5120 and (8, 45, 32, 64) in found
    assert [(s.I, s.D, s.nloop, s.lf) for s in FC.WINDOW_EDGES] == found
    for p, refused in FC.WINDOW_NEIGHBOURS.items():
        assert refused, p
        for I, D, nloop, lf in refused:                                  # asked of the product, never launched
            assert not FC.fits(I, D, nloop, lf)
            if nloop <= 64 and lf <= 128:
                assert FC.window_sum(I, D, nloop, lf) > 5120
            s = FC.Shape("", I, D, I * nloop, lf // 2)
            assert not L.AudioTail(I, D, s.resamp_taps(), np.full(lf // 2, 0.01, np.float32), block=0).general_fits(), (I, D, nloop, lf)
    for s in FC.WINDOW_EDGES:
        assert L.AudioTail(s.I, s.D, s.resamp_taps(), s.audio_half(), block=FC.first_defined(s)).general_fits(), s.name


def test_the_launches_of_every_shape():
    held = routes = 0
    for s in SHAPES:
        mine = FC.LAUNCHES[s.name]
        assert all(FC.general_fits(s, c.block) and FC.create_admits(s, c.block) for c in mine), s.name      # no launch on a refused shape
        b1 = FC.first_defined(s)
        assert b1 >= s.lowest_block and not FC.asserts(s, b1) and all(FC.asserts(s, b) for b in range(s.lowest_block, b1))
        whole = {c.block for c in mine if (c.q0, c.q1) == (0, FC.Q_MAX) and c.seamed and not c.cuts and not c.salted}
        assert whole == {b1, FC.ODD_BLOCK} and FC.ODD_BLOCK % s.I + (s.I == 1) and FC.ODD_BLOCK % 8 and FC.ODD_BLOCK % 2
        assert any(c.block == 0 for c in mine) and {c.rows for c in mine} >= {1, 3}
        cut = [c for c in mine if c.cuts]
        assert cut and all(len(c.cuts) == 2 and all(q % 2 == 1 and (s.I == 1 or q % s.I) for q in c.cuts) for c in cut)
        if s.I >= 3:
            assert any(c.q0 % s.I and c.q1 % s.I and c.q0 % s.I != c.q1 % s.I and c.q1 - c.q0 < 100 for c in mine), s.name
        assert any(c.q1 - c.q0 == max(s.I - 1, 1) for c in mine)
        assert sum(c.route2 for c in mine) == 1
        # the cap: at most one launch inside the zone, and at least two seamed launches held to the models
        inside = [c for c in mine if c.zone]
        assert len(inside) <= 1 and all(FC.asserts(s, c.block) for c in inside) and len(inside) == bool(FC.zone(s))
        assert all(not FC.asserts(s, c.block) for c in mine if c.block and not c.zone)
        assert sum(1 for c in mine if c.seamed and not c.zone) >= 2, s.name
        held += sum(1 for c in mine if not c.zone)
        routes += len(inside)
    for I, s in FC.ONE_PER_I.items():
        mine = FC.LAUNCHES[s.name]
        assert s.D == FC.MAX_D[I] and any(c.rows == 32 for c in mine) and {c.block for c in mine if c.far} == set(FC.FAR_BLOCKS)
    for s in list(FC.ONE_PER_I.values()) + FC.WINDOW_EDGES:
        tiles = [c for c in FC.LAUNCHES[s.name] if (c.q0, c.q1) == (0, FC.TILE) and c.exact]
        assert {c.layout[2] for c in tiles} == {0, 1, 2, 3}, s.name
    for s in SHAPES:
        assert any(c.salted for c in FC.LAUNCHES[s.name]) == bool(FC.KINDS[s.name] & set(FC.SALTED_KINDS))
    assert FC.Q_MAX < 4000
    print(f"    the family: {len(FC.RATIOS)} ratios, {len(SHAPES)} shapes, {len(FC.ALL_LAUNCHES)} launches: {held} held to the models, "
          f"{routes} held route against route (at most one a shape)")
    assert routes <= len(SHAPES) and held >= 5 * len(SHAPES)


# ---- seams ----------------------------------------------------------------------------------------------------------------------
_streams = {}


def streams(oracle, shape, block):
    """Row 0: the seamed z stream, the all-One z stream, the seamed filter output of the seamed z stream and the all-One filter output
    of the same z stream."""
    key = (shape.name, block)
    if key not in _streams:
        y = AC.padded(shape, AC.y_row(shape, 0), block, FC.Q_MAX)
        z_seamed = AC.z_stream(oracle, shape, y, block)
        z_one = AC.z_stream(oracle, shape, y, 0)
        _streams[key] = (z_seamed, z_one, AC.filter_stream(oracle, shape, z_seamed, block), AC.filter_stream(oracle, shape, z_seamed, 0))
    return _streams[key]


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_seamed_launches_hold_cross_outputs_of_both_stages_that_differ_in_bits(oracle, shape):
    for case in FC.LAUNCHES[shape.name]:
        if not case.seamed or case.zone:
            continue
        z_seamed, z_one, a_seamed, a_one = streams(oracle, shape, case.block)
        za, zb = case.z_range
        rc = AC.resampler_cross(shape, case.block, za, zb)
        fc = AC.filter_cross(shape, case.block, case.q0, case.q1)
        assert rc.size and fc.size, f"{case.name}: {rc.size} resampler and {fc.size} filter Cross outputs in the range"
        r_diff = rc[_bits(z_seamed[rc]) != _bits(z_one[rc])]
        f_diff = fc[_bits(a_seamed[fc]) != _bits(a_one[fc])]
        assert f_diff.size >= 1, case.name
        if FC.few_terms(shape):
            assert r_diff.size == 0, f"{case.name}: up to three products sum alike in both orders"
        else:
            assert r_diff.size >= 1, case.name
    # the seam rule marks every output the seamed Pipes compute differently
    for block in sorted({c.block for c in FC.LAUNCHES[shape.name] if c.seamed and not c.zone}):
        z_seamed, z_one, a_seamed, a_one = streams(oracle, shape, block)
        n = min(FC.Q_MAX + shape.lf - 1, z_seamed.size, z_one.size)
        differ = np.nonzero(_bits(z_seamed[:n]) != _bits(z_one[:n]))[0]
        assert np.isin(differ, AC.resampler_cross(shape, block, 0, n)).all(), f"{shape.name}, block {block}: resampler"
        n = min(FC.Q_MAX, a_seamed.size, a_one.size)
        differ = np.nonzero(_bits(a_seamed[:n]) != _bits(a_one[:n]))[0]
        assert np.isin(differ, AC.filter_cross(shape, block, 0, n)).all(), f"{shape.name}, block {block}: filter"


def test_few_term_shapes_are_the_tap_count_edges_only():
    few = [s for s in SHAPES if FC.few_terms(s)]
    assert few and all(FC.KINDS[s.name] & {"ntaps == I", "ntaps < I", "ntaps == 1"} for s in few)
    assert all(any(c.salted for c in FC.LAUNCHES[s.name]) for s in few if "ntaps < I" in FC.KINDS[s.name])


def test_tiles_hold_two_and_more_boundaries_of_each_stage():
    for I in range(1, 9):
        many = [c for s in SHAPES if s.I == I for c in FC.LAUNCHES[s.name]
                if c.seamed and not c.zone and (c.q0, c.q1) == (0, FC.Q_MAX) and all(min(AC.boundaries_in_tile(s, c.block, t)) >= 2 for t in (0, 1))]
        assert len(many) >= 4, I
    for s in SHAPES:
        assert min(AC.boundaries_in_tile(s, FC.first_defined(s), 0)) >= 5, s.name
        assert AC.boundaries_in_tile(s, FC.ODD_BLOCK, 0)[1] >= 3, s.name


# ---- the models -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("I", range(1, 9))
def test_every_model_run_outside_the_zone_is_defined_finite_and_nonzero(oracle, I):
    runs = 0
    for s in (s for s in SHAPES if s.I == I):
        for block, rows in sorted({(c.block, c.rows) for c in FC.LAUNCHES[s.name] if not c.zone and not c.salted}):
            for r in range(rows):
                e = AC.expected(oracle, s, r, block)
                assert e.size >= FC.Q_MAX and np.isfinite(e).all() and np.count_nonzero(e) > e.size // 2, (s.name, block, r)
                runs += 1
    print(f"    I = {I}: {runs} model runs, all defined, finite and nonzero")


@contextlib.contextmanager
def planted(kind):
    """The restated Pipes with one change, for as long as the block lasts."""
    res, fil = PM.ResamplerModel, PM.FilterModel

    class Resampler(res):
        def __init__(self, oracle, interpolation, decimation, coeffs, *a, **k):
            super().__init__(oracle, interpolation, decimation, coeffs, *a, **k)
            if kind == "a Cross walk one term short":                    # the last tap of every residue class, in the sequential walk only
                c = self.coeffs.copy()
                c[-min(interpolation, c.size):] = 0
                self.coeffs = c
            if kind == "the windows of groups g >= 4 one input early":   # a contiguous stream only: one walk from group 0
                inc = self.prep["increments"].copy()
                inc[3] -= 1
                inc[interpolation - 1] += 1
                self.prep = dict(self.prep, increments=inc)

    class Filter(fil):
        def __init__(self, oracle, coeffs, *a, **k):
            c = np.array(coeffs, np.float32)
            if kind == "a dropped last filter chunk":
                c[-8:] = 0
            super().__init__(oracle, c, *a, **k)
    PM.ResamplerModel, PM.FilterModel = Resampler, Filter
    try:
        yield
    finally:
        PM.ResamplerModel, PM.FilterModel = res, fil


PLANTS = [("a dropped last filter chunk", lambda s: s.nfc >= 2, lambda s: FC.ODD_BLOCK),
          ("a Cross walk one term short", lambda s: True, FC.first_defined),
          ("the windows of groups g >= 4 one input early", lambda s: s.I >= 5 and s.ntaps >= s.I, lambda s: 0)]      # every group holds a tap


@pytest.mark.parametrize("kind,applies,block_of", PLANTS, ids=[p[0] for p in PLANTS])
def test_a_planted_model_change_shows_in_the_bits_of_every_shape_it_applies_to(oracle, kind, applies, block_of):
    """The launch it is shown on: the whole-stream launch at block 257, the one at the first defined block, the contiguous launch."""
    seen = 0
    for s in SHAPES:
        if not applies(s):
            continue
        block = block_of(s)
        case = [c for c in FC.LAUNCHES[s.name] if c.block == block and c.q1 == FC.Q_MAX and not c.cuts and not c.salted and not c.zone]
        assert case, (s.name, block)
        q0, q1 = case[0].q0, case[0].q1
        with planted(kind):
            changed = AC.expected_from(oracle, s, AC.y_row(s, 0), block, 1.0)
        assert _differ(changed[q0:q1], AC.expected(oracle, s, 0, block)[q0:q1]), f"{s.name}: {kind} changes no bit of {case[0].name}"
        seen += 1
    print(f"    {kind}: shows on {seen} shapes")
    assert seen >= 50 and PM.ResamplerModel.__name__ == "ResamplerModel"


# ---- far launches ---------------------------------------------------------------------------------------------------------------
def test_the_far_launches_need_the_64_bit_remainder():
    far = [c for c in FC.ALL_LAUNCHES if c.far]
    assert len(far) == 16 and {c.shape.I for c in far} == set(range(1, 9))
    for c in far:
        s, B = c.shape, c.block
        T, Sh = c.far_shift
        assert T > 1 << 33 and T == FC.far_shift(s, B)[0] and B % 8 and B & (B - 1)
        # the near answer is the far answer: whole blocks in outputs, in inputs and in upsampled units, whole polyphase cycles
        assert T % B == 0 and Sh % B == 0 and (T * s.D) % (B * s.I) == 0 and T * s.D == Sh * s.I and T % s.I == 0
        assert s.first_input(c.q0) + Sh == int(AC.SC.in_offset(T + c.q0, s.I, s.D))
        for qa in FC.tile_bases(s, c.q0, c.q1, T):
            assert qa % B != (qa & 0xFFFFFFFF) % B, (c.name, qa)
            assert (qa * s.D) % (B * s.I) != ((qa * s.D) & 0xFFFFFFFF) % (B * s.I), (c.name, qa)
        assert len(FC.tile_bases(s, c.q0, c.q1, T)) == 1 and FC.tile_bases(s, c.q0, c.q1) == [c.q0 // s.I * s.I]


# ---- non-finite input -----------------------------------------------------------------------------------------------------------
def test_non_finite_samples_tell_the_grouped_walk_from_the_sequential_one(oracle):
    salted = [c for c in FC.ALL_LAUNCHES if c.salted]
    assert {c.shape.I for c in salted} == set(FC.EDGE_INTERPS)
    for c in salted:
        s, B = c.shape, c.block
        y = FC.salted_row(s, B)
        assert 3 <= np.count_nonzero(~np.isfinite(y)) <= 8 and np.isnan(y).any() and np.isposinf(y).any() and np.isneginf(y).any()
        e = FC.salted_expected(oracle, s, B)
        assert e.size == FC.Q_MAX and np.isnan(e).any() and not np.isnan(e).all() and np.isfinite(e).any() and not np.isfinite(e).all(), c.name
        if s.I == 1:
            continue                                     # ntaps == nloop: no padded tap, the two walks read the same products
        yp = AC.padded(s, y, B, FC.Q_MAX)
        z_seamed, z_one = AC.z_stream(oracle, s, yp, B), AC.z_stream(oracle, s, yp, 0)
        n = min(z_seamed.size, z_one.size, FC.Q_MAX + s.lf - 1)
        rc = AC.resampler_cross(s, B, 0, n)
        only_grouped = rc[np.isnan(z_one[rc]) & ~np.isnan(z_seamed[rc])]
        both = rc[np.isnan(z_one[rc]) & np.isnan(z_seamed[rc])]
        print(f"    {c.name}: {only_grouped.size} Cross outputs are NaN in the grouped walk only (a padded zero tap times an infinity), {both.size} in both")
        assert only_grouped.size >= 1, c.name
        assert not (np.isnan(z_seamed[rc]) & ~np.isnan(z_one[rc])).any()
        # ... and the audio row has NaN behind some of those positions and not behind others
        nan_q = np.isnan(e)
        reach = np.zeros(FC.Q_MAX, bool)
        for m in only_grouped:
            reach[max(m - s.lf + 1, 0):m + 1] = True
        assert (reach & ~nan_q).any(), c.name


# ---- the reference's undefined zone ---------------------------------------------------------------------------------------------
def _search(oracle, s, blocks):
    res = PM.ResamplerModel(oracle, s.I, s.D, s.resamp_taps(), PM.ORDER_AVX)
    fil = PM.FilterModel(oracle, s.audio_half(), PM.ORDER_AVX, sym=True)
    bad = []
    for b in blocks:
        try:
            z, _ = PM.fir_resampler_pipe(res, [np.zeros(b, np.float32)] * 40, b)
            PM.fir_filter_pipe(fil, z, b)
        except PM.PipeAssert as e:
            assert str(e) == "resample 1", (s.name, b, e)
            bad.append(b)
    return bad


def test_the_references_undefined_zone_is_where_the_rule_says(oracle):
    """By search with the restated Pipes: every block of [lowest, lowest + D + 2), the table's own blocks, 601 and 1100; the rule itself (the same arithmetic, which the search confirms) on every block up to 1100."""
    zones = {}
    for s in SHAPES:
        low = s.lowest_block
        blocks = sorted(set(range(low, low + s.D + 2)) | {250, 257, 601, 1100})
        bad = _search(oracle, s, blocks)
        assert bad == [b for b in blocks if FC.asserts(s, b, 40)], s.name
        assert all(low <= b < low + s.D for b in bad), (s.name, bad)
        assert set(bad) <= set(FC.zone(s)) and FC.zone(s, 40) == bad              # a longer stream can only meet more boundaries
        assert not any(FC.asserts(s, b) for b in range(low + s.D, 1101)), s.name
        if s.rlp // s.I >= s.lf:
            assert len(FC.zone(s)) <= -(-(s.D - 1) // s.I), s.name
        zones[s.name] = bad
    widest = max(zones, key=lambda n: len(zones[n]))
    print(f"    {sum(1 for z in zones.values() if z)} of {len(zones)} shapes have blocks at which the reference asserts; the widest: {widest}: {zones[widest]}")
    # what the issue names
    for (I, D, n, nhalf), want in (((5, 29, 200, 16), list(range(40, 46))), ((3, 10, 191, 32), [64, 65, 66]), ((1, 5, 39, 8), [41, 42, 43]),
                                   ((8, 9, 511, 8), [64])):
        s = FC.Shape("", I, D, n, nhalf)
        assert _search(oracle, s, range(s.lowest_block, s.lowest_block + D + 2)) == want == FC.zone(s), (I, D, n)
    assert max(len(z) for z in zones.values()) <= 6
