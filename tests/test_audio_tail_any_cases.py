"""What tests/audio_tail_any_cases.py reaches, shown on the CPU from the models alone (oracle/pipes_model.py and the seam rule
restated in tests/stream_slice_cases.py) -- no product code runs here, so these tests hold on any build.

  * every launch marked `seamed` holds at least one resampler Cross output and at least one filter Cross output whose sequential
    value differs IN BITS from its grouped (One) value on the table's own streams: a kernel that ignored a seam cannot pass;
  * the seam rule's Cross outputs are exactly where the seamed Pipes differ from the contiguous ones;
  * tiles with two and more buffer boundaries of EACH stage exist for every shape (the one-boundary-per-tile shortcut of the FM
    kernels cannot pass), up to 54 and 35 of them at the lowest block;
  * the late first output of an output block (late_output_is_one) cannot occur with seam block = output block = B >= I: output k B
    starts B (k D mod I) into its buffer of B I upsampled units, a multiple of B, never one of the last I - 1 positions -- checked by
    search over every launch and over every block up to 1100 for every shape;
  * the blocks, ends, starts, layouts and gains the GPU test names are in the table, and the one block of this table at which the
    reference's Pipe asserts (8/9 x 511 at 64, where block * I == numCoeffsR) is the only one without expected values.  That equality
    is not the rule: the reference asserts wherever some buffer boundary k has (-k block I) mod D > block I - numCoeffsR, a zone of up
    to ceil((D - 1) / I) blocks (tests/tail_any_family_cases.py `asserts`; tests/test_tail_any_family_cases.py finds it by search)."""
import numpy as np
import pytest

import audio_tail_any_cases as AC
from oracle import pipes_model as PM

SEAMED = [c for c in AC.LAUNCHES if c.seamed]
ASSERTING = {("8/9 x 511", 64)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


_streams = {}


def streams(oracle, shape, block):
    """Row 0: the seamed z stream, the all-One z stream, the seamed filter output of the seamed z stream and the all-One filter output
    of the same z stream."""
    key = (shape.name, block)
    if key not in _streams:
        y = AC.padded(shape, AC.y_row(shape, 0), block, AC.Q_MAX)
        z_seamed = AC.z_stream(oracle, shape, y, block)
        z_one = AC.z_stream(oracle, shape, y, 0)
        _streams[key] = (z_seamed, z_one, AC.filter_stream(oracle, shape, z_seamed, block), AC.filter_stream(oracle, shape, z_seamed, 0))
    return _streams[key]


@pytest.mark.parametrize("case", SEAMED, ids=[c.name for c in SEAMED])
def test_a_seamed_launch_holds_cross_outputs_of_both_stages_that_differ_in_bits(oracle, case):
    if (case.shape.name, case.block) in ASSERTING:
        with pytest.raises(PM.PipeAssert, match="resample 1"):
            streams(oracle, case.shape, case.block)
        return
    z_seamed, z_one, a_seamed, a_one = streams(oracle, case.shape, case.block)
    za, zb = case.z_range
    edges = [case.q0] + list(case.cuts) + [case.q1]
    assert all(a < b for a, b in zip(edges[:-1], edges[1:]))
    rc = AC.resampler_cross(case.shape, case.block, za, zb)
    fc = AC.filter_cross(case.shape, case.block, case.q0, case.q1)
    assert rc.size and fc.size, f"{case.name}: {rc.size} resampler and {fc.size} filter Cross outputs in the range"
    r_diff = rc[_bits(z_seamed[rc]) != _bits(z_one[rc])]
    f_diff = fc[_bits(a_seamed[fc]) != _bits(a_one[fc])]
    print(f"    {case.name}: {rc.size} resampler Cross outputs ({r_diff.size} differ in bits), {fc.size} filter Cross ({f_diff.size} differ)")
    assert r_diff.size >= 1 and f_diff.size >= 1, case.name


def test_the_seam_rule_marks_every_output_the_seamed_pipes_compute_differently(oracle):
    for shape, block in sorted({(c.shape.name, c.block) for c in SEAMED} - ASSERTING):
        s = AC.SHAPES[shape]
        z_seamed, z_one, a_seamed, a_one = streams(oracle, s, block)
        n = min(AC.Q_MAX + s.lf - 1, z_seamed.size, z_one.size)
        differ = np.nonzero(_bits(z_seamed[:n]) != _bits(z_one[:n]))[0]
        assert np.isin(differ, AC.resampler_cross(s, block, 0, n)).all(), f"{shape}, block {block}: a resampler output outside the rule's Cross set differs"
        n = min(AC.Q_MAX, a_seamed.size, a_one.size)
        differ = np.nonzero(_bits(a_seamed[:n]) != _bits(a_one[:n]))[0]
        assert np.isin(differ, AC.filter_cross(s, block, 0, n)).all(), f"{shape}, block {block}: a filter output outside the rule's Cross set differs"


def test_tiles_hold_two_and_more_boundaries_of_each_stage():
    for s in AC.SHAPES.values():
        whole = [c for c in AC.LAUNCHES if c.shape is s and c.seamed and c.q0 == 0 and c.q1 == AC.Q_MAX]
        assert whole, s.name
        many = [c for c in whole if all(min(AC.boundaries_in_tile(s, c.block, t)) >= 2 for t in (0, 1))]
        assert many, f"{s.name}: no whole-stream launch with >= 2 boundaries of each stage in both full tiles"
        r, f = AC.boundaries_in_tile(s, s.lowest_block, 0)
        assert r >= 7 and f >= 7, (s.name, r, f)
    assert AC.boundaries_in_tile(AC.SHAPES["2/3 x 47"], 24, 0) == (54, 35)


def test_no_late_first_output_can_occur_with_one_block_for_both_sides():
    for c in AC.LAUNCHES:
        assert AC.late_first_outputs(c.shape, c.block, *c.z_range).size == 0, c.name
    for s in AC.SHAPES.values():
        for block in range(s.lowest_block, 1101):
            assert AC.late_first_outputs(s, block, 0, 40 * block).size == 0, (s.name, block)
    # the predicate itself is live: with an output block that differs from the seam block it does fire (tests/fir_rows_cases.py)
    import stream_slice_cases as SC
    assert SC.late_output_is_one(np.int64(1843), np.int64(18432), 3, 10, 97)


def test_the_table_holds_the_edges_the_gpu_test_names():
    assert set(AC.SHAPES) == {"4/5 x 63", "3/5 x 71", "2/5 x 127", "2/3 x 47", "3/4 x 95", "7/8 x 255", "8/9 x 511", "1/5 x 39", "3/10 x 191"}
    assert {s.nhalf for s in AC.SHAPES.values()} == {64, 32, 8}
    for s in AC.SHAPES.values():
        mine = [c for c in AC.LAUNCHES if c.shape is s]
        assert all(AC.general_fits(s, c.block) for c in mine), s.name
        assert {c.q1 for c in mine if c.q0 == 0} >= {1, 2, s.I, s.I + 1, AC.TILE - 1, AC.TILE, AC.TILE + 1, 2 * AC.TILE + 1, AC.Q_MAX}
        assert {c.q0 for c in mine} >= {0, 1, s.I - 1, 601, AC.TILE}
        assert {c.block for c in mine} >= {0, 200, 250, 256, 1000, s.lowest_block}
        assert {len(c.cuts) for c in mine} >= {0, 2, 4} and all(q % 2 == 1 for c in mine for q in c.cuts)
        far = [c for c in mine if c.far]
        assert {c.block for c in far} == {0, 256} and all(c.q0 == 5 for c in far)
        T, Sh = far[0].far_shift
        assert T * s.D == Sh * s.I and T % 256 == 0 and Sh % 256 == 0 and (T * s.D) % (256 * s.I) == 0
        assert any(c.exact for c in mine) and any(not c.exact for c in mine)
        assert s.end_input(AC.Q_MAX - 1) == s.n_y
        assert not AC.general_fits(s, s.lowest_block - 1) and AC.general_fits(s, s.lowest_block)
    assert AC.FM.I << 30 == 3 * 2 ** 30
    assert {c.rows for c in AC.LAUNCHES} >= {1, 3, 32}
    assert {c.layout[:2] for c in AC.LAUNCHES} >= {(0, 0), (1, 1), (5, 5), (1, 5), (5, 0)}
    assert {c.layout[2] for c in AC.LAUNCHES} >= {0, 1, 2, 3}
    assert {c.gain for c in AC.LAUNCHES} >= {1.0, -0.5, float(np.float32(1e-41))}
    assert AC.Q_MAX < 4000                               # a few thousand outputs per row


def test_expected_values_exist_everywhere_but_at_the_asserting_block(oracle):
    for shape, block in sorted({(c.shape.name, c.block) for c in AC.LAUNCHES}):
        s = AC.SHAPES[shape]
        if (shape, block) in ASSERTING:
            assert block * s.I == s.rlp
            with pytest.raises(PM.PipeAssert, match="resample 1"):
                AC.expected(oracle, s, 0, block)
        else:
            e = AC.expected(oracle, s, 0, block)
            assert e.size == AC.Q_MAX and np.isfinite(e).all() and np.abs(e).max() > 0


def test_the_composition_of_a_contiguous_stream_is_a_slice_of_any_longer_one(oracle):
    """expected() appends zeros for the Pipes' whole blocks: the outputs it keeps do not read them."""
    for s in (AC.SHAPES["4/5 x 63"], AC.SHAPES["8/9 x 511"]):
        y = AC.y_row(s, 1)
        for block in (0, 200):
            full = AC.expected_from(oracle, s, y, block, 0.5)
            short = AC.expected_from(oracle, s, y[:s.end_input(999)], block, 0.5)
            assert short.size == 1000 and (_bits(short) == _bits(full[:1000])).all(), (s.name, block)
