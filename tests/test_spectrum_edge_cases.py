"""What tests/spectrum_edge_cases.py reaches, shown without a GPU: every slicing case predicts more than one hipFFT transform or layered
launch (or, for the grid cases, more rows than the grid holds) from the host's own integer arithmetic, the boundary a case is named
for falls where the table says, the directed inputs have the closed forms the GPU tests hold the device to, the value classes land
where they are named for, and the model's check lets an expected NaN through and nothing else."""
import numpy as np
import pytest

import spectrum_edge_cases as E
import spectrum_model as M
import spectrum_reduce_model as R


# ---- A. slices, chunks and grids --------------------------------------------------------------------------------------------------------
def test_the_table_states_the_scratch_arithmetic_of_the_source():
    """The constants the table computes from are the source's: a change there shows up here before a GPU test goes stale."""
    import os
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_amd", "csrc")
    fft = open(os.path.join(csrc, "fft.cpp")).read()
    assert "SPECTRUM_SCRATCH_BYTES = (size_t)64 << 20" in fft and E.SCRATCH == 64 << 20
    kernels = open(os.path.join(csrc, "kernels_spectrum.hip")).read()
    assert kernels.count("< 4096 ? ") == 2 and E.GRID_Y_CAP == 4096                 # spectrum_prepare, spectrum_accumulate
    assert kernels.count("const int64_t resident = 2048;") == 2 and E.FUSED_GRID == 2048
    assert "SPECTRUM_REDUCE_CHUNK = 32" in open(os.path.join(csrc, "spectrum.hpp")).read().replace("  ", " ") and E.CHUNK == R.CHUNK == 32


@pytest.mark.parametrize("case", E.RUN_HIPFFT, ids=lambda c: f"{c.n}x{c.rows}")
def test_run_device_chunks(case):
    chunks = E.run_chunks(case.n, case.rows)
    assert case.batches == len(chunks) > 1 and sum(chunks) == case.rows
    assert E.samples_for(case.n, case.hop, case.rows) * 2 <= 1 << 24, "a small input"
    assert case.rows * case.n * 4 <= 52 << 20, "an output of about 50 MB at the most"
    if case.n == 16384:
        assert chunks == [256, 256, 8] and E.run_chunks(case.n, case.then_rows) == [256, 44] and case.then_batches == 2
        # three batch sizes on one object: the first plan (256) is kept, the second (8) replaced by the third (44)
        assert len({256, 8, 44}) == 3
    elif case.n == 1000:
        assert chunks == [4194, 6] and chunks[0] > E.GRID_Y_CAP, "spectrum_prepare strides over rows"
    else:
        assert chunks == [1, 1, 1] and 16 * case.n >= E.SCRATCH, "one row is the whole scratch"


@pytest.mark.parametrize("case", E.REDUCE_HIPFFT, ids=lambda c: c.edge)
def test_reduce_batches(case):
    batches = E.reduce_batches(case.n, case.rows_out, case.group)
    assert sum(nrows for _, _, nrows in batches) == case.rows_out * case.group
    assert case.rows_out * case.group * case.n * 16 <= 128 << 20, "the model's transform stays small"
    if case.edge == "grid":
        assert case.batches == 1 and case.force and case.n in E.FUSED_SIZES
        assert case.rows_out > E.GRID_Y_CAP, "spectrum_accumulate strides over output rows"
        assert case.rows_out * case.group > E.GRID_Y_CAP, "spectrum_prepare strides over input rows"
        return
    assert case.batches > 1 and case.edges
    js = [j for j, _ in case.edges]
    if case.edge == "mid-chunk":
        assert case.batches == 3 and js == [28, 56] and all(j % E.CHUNK != 0 for j in js)
    elif case.edge == "fold":
        assert case.batches == 3 and js[0] == 128 and js[0] % E.CHUNK == 0 and js[0] != 0, "a carried chunk is complete when the batch starts"
    elif case.edge == "group start":
        assert case.batches == 3 and js == [0, 0]
        # No batch of this case ends inside a group, so it never writes state: fresh scratch would hide a wrong load.  The run that
        # goes first has the same state layout (same n and rows_out) and leaves state in exactly the rows the batches here start with.
        assert E.stored_rows(case.n, case.rows_out, case.group) == []
        starts = [b0 // case.group for _, b0, _ in batches if b0]
        assert starts == [2, 4] and set(starts) <= set(E.stored_rows(case.n, case.rows_out, case.dirty_group))
        assert case.dirty_group < case.group, "the same input is long enough"
    elif case.edge == "row slices":
        assert case.batches == 3 + 1 and sorted({r0 for r0, _, _ in batches}) == [0, 128]
        assert all(j != 0 for j in js), "and the first slice's batch edges are mid-group"


def test_all_pairs_case_is_the_mid_chunk_one():
    assert E.ALL_PAIRS_CASE.edge == "mid-chunk"


@pytest.mark.parametrize("case", E.RUN_FUSED, ids=lambda c: f"{c.n}x{c.rows}")
def test_fused_grid_cases(case):
    assert case.n in E.FUSED_SIZES and case.tiles == 2050 > E.FUSED_GRID
    assert case.second_turn_row < case.rows, "a workgroup takes a second tile"
    assert case.rows * case.n * 4 <= 52 << 20
    if case.n == 64:
        assert case.rows % E.rows_per_tile(64) == 2, "a partial last tile"


def test_fused_layers_case():
    case = E.REDUCE_LAYERS
    slices = E.layer_slices(case.n, case.rows_out, case.group)
    assert case.launches == len(slices) == 4
    assert slices == [(0, 256, 0, 15), (0, 256, 15, 16), (256, 44, 0, 15), (256, 44, 15, 16)]
    assert case.model_rows == (255, 256, 299)
    # the shapes test_gpu_spectrum_reduce.py runs through layers elsewhere take one launch each: this is the only sliced one
    assert len(E.layer_slices(1024, 3, 1000)) == 1 and len(E.layer_slices(64, 2, 40000)) == 1


@pytest.mark.parametrize("n", E.FUSED_SIZES)
def test_size_cases(n):
    rows, hop = E.size_case(n)
    assert rows == E.rows_per_tile(n) + 1 and hop % 2 == 1 and 1 <= hop < n
    for fmt in (M.IQ_U8, M.IQ_CF32, E.IQ_I16):
        iq, f32 = E.format_input(fmt, n, 8)
        assert f32.dtype == np.float32 and f32.shape == iq.shape
    iq, f32 = E.format_input(E.IQ_I16, 1, 64)
    assert np.array_equal(f32.astype(np.float64), iq.astype(np.float64) / 2048.0)
    iq, f32 = E.format_input(M.IQ_U8, 1, 64)
    assert np.array_equal(f32.astype(np.float64), M.to_complex(iq, M.IQ_U8).view(np.float64))


# ---- B. directed inputs -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 1000])
def test_impulse_closed_form_is_the_model(n):
    w = M.window(M.WINDOW_HAMMING, n)
    for j in E.impulse_positions(n):
        mag, _ = M.spectrum(E.impulse(n, j), n, M.IQ_CF32, M.WINDOW_HAMMING, None, True, 0.75, n, 1)
        assert np.max(np.abs(mag - 0.75 * w[j])) <= 1e-15


@pytest.mark.parametrize("n", [64, 1000])
def test_tone_closed_form_is_the_model(n):
    for k in E.tone_bins(n):
        iq, peak = E.tone(n, k)
        assert abs(peak - n) <= 1e-7 * n, "float32 samples of a unit tone"
        for shift in (False, True):
            mag, _ = M.spectrum(iq, n, M.IQ_CF32, M.WINDOW_NONE, None, shift, 1.0, n, 1)
            at = (k + n // 2) % n if shift else k
            assert int(np.argmax(mag[0])) == at and abs(mag[0, at] - peak) <= 1e-12 * n
            assert np.max(np.delete(mag[0], at)) <= 1e-6 * n


# ---- C. value classes ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.VALUE_CLASS_SIZES)
def test_value_classes_land_where_they_are_named_for(n):
    sub, huge, over, mixed = E.value_classes(n)
    for vc in (sub, huge, over, mixed):
        iq = vc.iq()
        assert iq.dtype == np.float32 and iq.size == 2 * vc.rows * n and np.all(np.isfinite(iq))
    ref = lambda vc: E.reference(vc.iq(), n, vc.scale, n, vc.rows)
    x = sub.iq()
    assert np.all(np.abs(x) < 2.0 ** -126) and np.count_nonzero(x) > x.size // 2, "float32 subnormals in"
    r = ref(sub)
    assert 0 < r.max() < 2.0 ** -126, "float32 subnormals out"
    assert np.max(E.close_bound(r)) < 2.0 ** -148, "the bound down there is the subnormal spacing, not a fraction of the value"
    assert np.max(np.abs(huge.iq())) == E.FLT_MAX and ref(huge).max() < E.FLT_MAX and ref(huge).max() > 1e36
    r = ref(over)
    must_inf, must_close, left_out = E.overflow_split(r)
    assert left_out.sum() <= r.size // 100, "at most 1 % of the bins may be left out of the comparison"
    assert must_inf.sum() > r.size // 4 and must_close.sum() > r.size // 4, "both sides of FLT_MAX are populated"
    with np.errstate(over="ignore"):
        assert np.all(np.isinf(r[must_inf].astype(np.float32))) and np.all(np.isfinite(r[must_close].astype(np.float32)))
    x = np.abs(mixed.iq())
    assert np.any((x > 0) & (x < 2.0 ** -126)) and x.max() > 1e30


def test_close_bound_is_the_contract_at_normal_magnitudes():
    ref = np.array([[1.0, 1e-3, 2.0 ** -126, 3e38, 0.0]])
    old = 1e-11 * np.max(np.abs(ref), axis=-1, keepdims=True) + 2.0 ** -23 * np.abs(ref)
    new = E.close_bound(ref)
    assert np.array_equal(new[:, :4], old[:, :4]), "nothing loosened where float32 is normal"
    assert new[0, 4] == old[0, 4] + E.FLT_TINY


# ---- D. non-finite input ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,route", E.NONFINITE_SIZES)
@pytest.mark.parametrize("group,rows_out", E.NONFINITE_GROUPS)
def test_a_poison_lies_in_exactly_two_rows_and_two_output_rows(n, route, group, rows_out):
    hop, rows = n // 2, group * rows_out
    assert M.window(M.WINDOW_HANNING, n)[0] == 0.0
    for name, value, imaginary, at_j0 in E.POISONS:
        p, held = E.poison_place(n, group, at_j0)
        assert tuple(E.rows_holding(n, hop, rows, p)) == held
        assert sorted({r // group for r in held}) == [0, 1] and rows_out > 2, "two poisoned output rows, clean ones behind them"
        if at_j0:
            assert p - held[1] * hop == 0, "j = 0 of its second row, where the Hanning window is 0"
        iq = np.zeros(2 * E.samples_for(n, hop, rows), np.float32)
        bad = E.poisoned(iq, p, value, imaginary)
        assert np.count_nonzero(~np.isfinite(bad)) == 1 and not np.isfinite(bad[2 * p + imaginary])


def test_the_definition_propagates_a_nan():
    """The definition in numpy: [nan, inf, 0, 1] in dB gives [nan, inf, floor, 0], and a max hold keeps a NaN row."""
    v = np.array([[np.nan, np.inf, 0.0, 1.0]])
    got = R.to_db(v, R.MAX_MAGNITUDE, -120.0)
    assert np.isnan(got[0, 0]) and got[0, 1] == np.inf and got[0, 2] == -120.0 and got[0, 3] == 0.0
    mag = np.array([[1.0, 2.0], [np.nan, 1.0], [3.0, 0.5]])
    vmax, _ = R.reduce_rows(mag, 3, R.MAX_MAGNITUDE)
    assert np.isnan(vmax[0, 0]) and vmax[0, 1] == 2.0


def test_check_accepts_an_expected_nan_and_nothing_else():
    v = np.array([[np.nan, 1.0, 100.0, np.nan]])
    delta = np.where(np.isnan(v), np.nan, 0.0)
    for unit, good in ((R.LINEAR, [np.nan, 1.0, 100.0, np.nan]), (R.DB, [np.nan, 0.0, 20.0, np.nan])):
        R.check(np.array([good], np.float32), v, delta, R.MEAN_POWER, unit, -120.0)
        for k, wrong in ((0, -120.0), (0, 1.0), (1, np.nan), (2, np.inf), (3, 0.0)):
            bad = np.array([good], np.float32)
            bad[0, k] = wrong
            with pytest.raises(AssertionError):
                R.check(bad, v, delta, R.MEAN_POWER, unit, -120.0)
    with pytest.raises(AssertionError):                                     # a finite expectation still refuses a non-finite result
        R.check(np.array([[np.nan, 1.0]], np.float32), np.array([[1.0, 1.0]]), np.zeros((1, 2)), R.MEAN_POWER, R.LINEAR, -120.0)
