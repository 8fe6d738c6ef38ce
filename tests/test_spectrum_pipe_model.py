"""The waterfall Pipe's bookkeeping as tests/spectrum_pipe_model.py restates it -- completed rows, tail length and skip count after
every push -- against brute force on the concatenated stream, and the int16 stream the device tests use: its forced values lie
inside rows, and the exact conversion is what oracle.convert_i16 gives.  No device, no library: the model alone."""
import numpy as np
import pytest

import spectrum_pipe_model as SP
import tuner_i16_cases as IC

GEOMETRIES = [(64, 64, 1), (64, 32, 3), (64, 101, 2), (64, 64, 33)]


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("n,hop,group", GEOMETRIES)
def test_the_model_against_brute_force(n, hop, group, seed):
    total = SP.samples_for(n, hop, 5, group) + 17
    sizes = SP.ragged_sizes(seed, total)
    assert sum(sizes) == total and 1 in sizes and any(s % 2 == 1 and s > 1 for s in sizes)
    m, pushed, rows = SP.PipeModel(n, hop, group), 0, 0
    for s in sizes:
        rows += m.push(s)
        pushed += s
        want = SP.brute_force(n, hop, group, pushed)
        assert (rows, m.tail, m.skip) == want, f"after {pushed} samples"
        assert m.rows_done == rows and m.pos == pushed
        assert m.tail <= (group - 1) * hop + n - 1, "the tail holds no whole row"
        assert m.tail == 0 or m.skip == 0
    assert rows >= 5


@pytest.mark.parametrize("n,hop,group", GEOMETRIES)
def test_one_sample_pushes_and_one_large_push(n, hop, group):
    total = SP.samples_for(n, hop, 3, group) + 5
    a, rows = SP.PipeModel(n, hop, group), 0
    for _ in range(total):
        rows += a.push(1)
    b = SP.PipeModel(n, hop, group)
    assert b.push(total) == rows == SP.brute_force(n, hop, group, total)[0]
    assert (a.tail, a.skip) == (b.tail, b.skip)


def test_a_skip_is_pending_where_hop_exceeds_n():
    m = SP.PipeModel(64, 101, 2)
    assert m.push(101 + 64) == 1 and (m.tail, m.skip) == (0, 37), "row 0 ends 37 samples before row 1's group starts"
    assert m.push(30) == 0 and (m.tail, m.skip) == (0, 7)
    assert m.push(10) == 0 and (m.tail, m.skip) == (3, 0)


@pytest.mark.parametrize("n,hop,group,rows_out", [(64, 64, 3, 43), (64, 64, 70, 2), (2048, 1024, 3, 3), (8192, 4096, 3, 1), (1000, 501, 3, 6)])
def test_forced_int16_values_occur_inside_rows(n, hop, group, rows_out):
    """The device tests take the first blocks of stream_i16, past the first block edge (the forced values sit either side of every
    edge): every forced value occurs at a position some input row covers."""
    ns = SP.samples_for(n, hop, rows_out, group)
    assert IC.B + 3 <= ns <= 3 * IC.B
    s = SP.stream("i16", 3 * IC.B)[:2 * ns]
    covered = np.zeros(ns, bool)
    for r in range(rows_out * group):
        covered[r * hop:r * hop + n] = True
    both = np.repeat(covered, 2)
    for v in IC.FORCED:
        assert np.any((s == v) & both), f"{v} does not occur inside a row"


def test_the_exact_conversion(oracle):
    s = IC.stream_i16(3 * IC.B, seed=1620)
    f = SP.i16_to_float(s)
    assert f.tobytes() == np.asarray(oracle.convert_i16(s), np.float32).tobytes()
    assert np.array_equal(f.astype(np.float64), s.astype(np.float64) * 2.0 ** -11), "exact: the double of the float is the double product"
