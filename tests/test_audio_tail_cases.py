"""What tests/audio_tail_cases.py reaches, shown on the CPU from the models alone (oracle/pipes_model.py and the seam rule restated
in tests/stream_slice_cases.py) -- no product code runs here, so these tests hold on any build.

  * every launch marked `seamed` holds at least one resampler Cross output and at least one filter Cross output whose sequential
    value differs IN BITS from its grouped (One) value on the table's own streams: a kernel that ignored a seam cannot pass;
  * the seam rule's Cross outputs are exactly where the seamed Pipes differ from the contiguous ones (up to values that happen to
    agree), so the rule the table is built on is the Pipes';
  * the late first output of an output block (late_output_is_one) does not occur with 3/10 and seam block = output block: the table
    says so, and it is checked by search over every launch and over a long stream;
  * the route-1 fit edge, the tile boundaries and the value edges the GPU test names are in the table."""
import numpy as np
import pytest

import audio_tail_cases as AC

SEAMED = [c for c in AC.LAUNCHES if c.seamed]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def streams(oracle):
    """Per block of the seamed launches, row 0: the seamed z stream, the all-One z stream, the seamed filter output of the seamed z
    stream and the all-One filter output of the same z stream."""
    out = {}
    for block in sorted({c.block for c in SEAMED}):
        y = AC.y_row(0)
        up = lambda n: -(-n // block) * block                           # noqa: E731
        pad = up(-(-(up(up(AC.Q_MAX) + AC.LF - 1) * AC.D) // AC.I) + AC.NLOOP + 1) + block
        y = np.concatenate([y, np.zeros(pad - y.size, np.float32)])
        z_seamed = AC.z_stream(oracle, y, block)
        z_one = AC.z_stream(oracle, y, 0)
        a_seamed = AC.filter_stream(oracle, z_seamed, block)
        a_one = AC.filter_stream(oracle, z_seamed, 0)
        out[block] = (z_seamed, z_one, a_seamed, a_one)
    return out


@pytest.mark.parametrize("case", SEAMED, ids=[c.name for c in SEAMED])
def test_a_seamed_launch_holds_cross_outputs_of_both_stages_that_differ_in_bits(streams, case):
    z_seamed, z_one, a_seamed, a_one = streams[case.block]
    za, zb = case.z_range
    edges = [case.q0] + list(case.cuts) + [case.q1]
    assert all(a < b for a, b in zip(edges[:-1], edges[1:]))
    rc = AC.resampler_cross(case.block, za, zb)
    fc = AC.filter_cross(case.block, case.q0, case.q1)
    assert rc.size and fc.size, f"{case.name}: {rc.size} resampler and {fc.size} filter Cross outputs in the range"
    r_diff = rc[_bits(z_seamed[rc]) != _bits(z_one[rc])]
    f_diff = fc[_bits(a_seamed[fc]) != _bits(a_one[fc])]
    print(f"    {case.name}: {rc.size} resampler Cross outputs ({r_diff.size} differ in bits), {fc.size} filter Cross ({f_diff.size} differ)")
    assert r_diff.size >= 1 and f_diff.size >= 1, case.name


def test_the_seam_rule_marks_every_output_the_seamed_pipes_compute_differently(streams):
    for block, (z_seamed, z_one, a_seamed, a_one) in streams.items():
        n = min(AC.Q_MAX + AC.LF - 1, z_seamed.size, z_one.size)
        differ = np.nonzero(_bits(z_seamed[:n]) != _bits(z_one[:n]))[0]
        assert np.isin(differ, AC.resampler_cross(block, 0, n)).all(), f"block {block}: a resampler output outside the rule's Cross set differs"
        n = min(AC.Q_MAX, a_seamed.size, a_one.size)
        differ = np.nonzero(_bits(a_seamed[:n]) != _bits(a_one[:n]))[0]
        assert np.isin(differ, AC.filter_cross(block, 0, n)).all(), f"block {block}: a filter output outside the rule's Cross set differs"


def test_no_late_first_output_exists_for_these_sizes():
    for c in AC.LAUNCHES:
        assert AC.late_first_outputs(c.block, *c.z_range).size == 0, c.name
    for block in (64, 97, 1000, 1024, AC.MIN_BLOCK, 8192):
        assert AC.late_first_outputs(block, 0, 40 * block).size == 0, block
    # the predicate itself is live: with an output block that differs from the seam block it does fire (tests/fir_rows_cases.py)
    import stream_slice_cases as SC
    m = np.int64(1843)
    assert SC.late_output_is_one(m, np.int64(18432), 3, 10, 97)


def test_the_table_holds_the_edges_the_gpu_test_names():
    assert AC.MIN_BLOCK == 7314 and AC.fused_fits(AC.MIN_BLOCK) and not AC.fused_fits(AC.MIN_BLOCK - 1) and not AC.fused_fits(1024)
    ends = {c.q1 for c in AC.LAUNCHES if c.q0 == 0}
    assert {1, 2, 3, 4, 2045, 2046, 2047, 4093, AC.Q_MAX} <= ends
    starts = {c.q0 for c in AC.LAUNCHES}
    assert {0, 1, 2, 2046} <= starts and any(q % 3 == 1 and 3 < q < AC.TILE for q in starts)
    assert any(c.far for c in AC.LAUNCHES) and AC.FAR_T % 8192 == 0 and AC.FAR_S % 8192 == 0 and AC.FAR_T * AC.D == AC.FAR_S * AC.I
    assert AC.FAR_T + 5 == 3 * 2 ** 30 + 5 and any(c.far and c.q0 == 5 for c in AC.LAUNCHES)
    assert {c.rows for c in AC.LAUNCHES} >= {1, 3, 32}
    assert {c.block for c in AC.LAUNCHES} == set(AC.BLOCKS)
    assert {len(c.cuts) for c in AC.LAUNCHES} >= {0, 2, 4}
    assert {c.layout[2] for c in AC.LAUNCHES} >= {0, 1, 2, 3}
    assert AC.end_input(AC.Q_MAX - 1) == AC.N_Y
    # a launch whose buffer holds exactly the receptive field, and one on the stream from 0
    assert any(c.exact for c in AC.LAUNCHES) and any(not c.exact for c in AC.LAUNCHES)


def test_the_composition_of_a_contiguous_stream_is_a_slice_of_any_longer_one(oracle):
    """expected() appends zeros for the Pipes' whole blocks: the outputs it keeps do not read them."""
    y = AC.y_row(1)
    for block in (0, 8192):
        full = AC.expected_from(oracle, y, block, 0.5)
        short = AC.expected_from(oracle, y[:AC.end_input(2999)], block, 0.5)
        assert short.size == 3000 and (_bits(short) == _bits(full[:3000])).all(), block
