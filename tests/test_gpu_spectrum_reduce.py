"""The reducing form of the spectrum operator on the device (sdrhip_spectrum_reduce_*: kernels_spectrum.hip, fft.cpp): mean power, mean
magnitude or max hold over `group` consecutive rows, linear or dB, against the numpy restatement of its definition
(tests/spectrum_reduce_model.py, which also derives the tolerance from the operator's own contract).  Where the definition promises
bits (a group of one against run_device, the split modes, a row's place in the batch, the host entry point) bytes are compared.
Outputs come from gpu_util.dev_empty_f32: a row written out of place trips the NaN guard bands."""
import itertools

import numpy as np
import pytest

import gpu_util as G
import spectrum_model as M
import spectrum_reduce_model as R

pytestmark = pytest.mark.gpu

REDUCES = (R.MEAN_POWER, R.MEAN_MAGNITUDE, R.MAX_MAGNITUDE)
UNITS = (R.LINEAR, R.DB)
FLOOR = -150.0


def u8_iq(seed, n_samples):
    return np.random.default_rng(seed).integers(0, 256, 2 * n_samples, dtype=np.uint8)


def samples_for(n, hop, rows_out, group):
    return (rows_out * group - 1) * hop + n


def reduce_device(spec, iq, hop, rows_out, group, reduce, unit, floor_db=FLOOR, d_in=None):
    """iq: host array of interleaved samples -> rows_out x n float32 through reduce_device on guarded device memory."""
    d_in = G.to_dev(iq) if d_in is None else d_in
    d_out = G.dev_empty_f32(rows_out * spec.n)
    assert spec.reduce_device(G.ptr(d_in), iq.size // 2, G.ptr(d_out), group, reduce, unit, floor_db, hop=hop, rows_out=rows_out) == rows_out
    return G.to_host(d_out).reshape(rows_out, spec.n)


def against_the_model(hip, spec, iq, model_args, hop, rows_out, group, what, combos=None):
    """Every reduce x unit (or `combos`) of one input against the model; the magnitudes are computed once."""
    mag, _ = M.spectrum(iq, spec.n, *model_args, hop, rows_out * group)
    d_in = G.to_dev(iq)
    for reduce, unit in (combos or itertools.product(REDUCES, UNITS)):
        v, delta = R.reduce_rows(mag, group, reduce)
        got = reduce_device(spec, iq, hop, rows_out, group, reduce, unit, d_in=d_in)
        R.check(got, v, delta, reduce, unit, FLOOR, f"{what} reduce={reduce} unit={unit}")


# ---- 1. every reduce x unit on the sizes of the one-kernel route -------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128, 2048, 4096, 8192])
def test_every_reduce_and_unit_on_the_one_kernel_route(hip, n):
    rows_out, group, scale = 2, 3, 1.0 / n
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, scale)
    iq = u8_iq(n, samples_for(n, n, rows_out, group))
    before, before_split = hip.spectrum_fused_launches(), hip.spectrum_reduce_split_launches()
    against_the_model(hip, spec, iq, (M.IQ_U8, M.WINDOW_HANNING, None, True, scale), n, rows_out, group, f"n={n}")
    assert hip.spectrum_fused_launches() == before + 6, "the one-kernel route did not take every call"
    assert hip.spectrum_reduce_split_launches() == before_split, "a group of one chunk has nothing to split"


# ---- 2. a partial last tile, groups on both sides of the chunk length ---------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 31, 32, 33, 70])
def test_partial_last_tile_and_groups_around_the_chunk_length(hip, group):
    n, rows_out, hop = 64, 33, 48
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HAMMING, True, 1.0)
    iq = u8_iq(group, samples_for(n, hop, rows_out, group))
    before = hip.spectrum_fused_launches()
    against_the_model(hip, spec, iq, (M.IQ_U8, M.WINDOW_HAMMING, None, True, 1.0), hop, rows_out, group, f"group={group}")
    assert hip.spectrum_fused_launches() == before + 6


# ---- 3. more tiles than the launch's grid ----------------------------------------------------------------------------------------
def test_more_tiles_than_the_grid(hip):
    n, rows_out, group, hop = 2048, 2050, 2, 512
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, False, 1.0 / n)
    iq = u8_iq(3, samples_for(n, hop, rows_out, group))
    against_the_model(hip, spec, iq, (M.IQ_U8, M.WINDOW_HANNING, None, False, 1.0 / n), hop, rows_out, group, "2050 tiles",
                      combos=[(R.MEAN_POWER, R.DB), (R.MAX_MAGNITUDE, R.LINEAR)])


# ---- 4. a group of one is run_device, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 8192])
def test_group_of_one_mean_magnitude_linear_is_run_device(hip, n):
    rows, hop = 5, n - 3
    iq = u8_iq(n + 4, samples_for(n, hop, rows, 1))
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_BLACKMAN, True, 3.0)
    spec.set_route(hip.SPECTRUM_ROUTE_FUSED)
    d_in, d_rows = G.to_dev(iq), G.dev_empty_f32(rows * n)
    spec.run_device(G.ptr(d_in), iq.size // 2, G.ptr(d_rows), hop=hop, rows=rows)
    got = reduce_device(spec, iq, hop, rows, 1, R.MEAN_MAGNITUDE, R.LINEAR, d_in=d_in)
    assert got.tobytes() == G.to_host(d_rows).tobytes()


# ---- 5. split modes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows_out", [1, 3])
def test_split_modes_give_identical_bytes(hip, rows_out):
    n, group, hop = 1024, 1000, 256
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0 / n)
    iq = u8_iq(rows_out, samples_for(n, hop, rows_out, group))
    d_in = G.to_dev(iq)
    mag, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, 1.0 / n, hop, rows_out * group)
    for reduce, unit in ((R.MEAN_POWER, R.DB), (R.MEAN_MAGNITUDE, R.LINEAR), (R.MAX_MAGNITUDE, R.DB)):
        got = {}
        for mode, name in ((hip.REDUCE_SPLIT_NEVER, "never"), (hip.REDUCE_SPLIT_ALWAYS, "always"), (hip.REDUCE_SPLIT_AUTO, "auto")):
            spec.set_reduce_split(mode)
            before, before_fused = hip.spectrum_reduce_split_launches(), hip.spectrum_fused_launches()
            got[name] = reduce_device(spec, iq, hop, rows_out, group, reduce, unit, d_in=d_in)
            moved = hip.spectrum_reduce_split_launches() - before
            assert hip.spectrum_fused_launches() == before_fused + 1
            if name == "never":
                assert moved == 0, "never split, and the split counter moved"
            if name == "always":
                assert moved == 1, "always split, and the split counter did not move"
        assert got["always"].tobytes() == got["never"].tobytes(), f"reduce={reduce} unit={unit}: split and unsplit differ"
        assert got["auto"].tobytes() == got["never"].tobytes(), f"reduce={reduce} unit={unit}: auto and unsplit differ"
        v, delta = R.reduce_rows(mag, group, reduce)
        R.check(got["never"], v, delta, reduce, unit, FLOOR, f"rows_out={rows_out} reduce={reduce} unit={unit}")


def test_split_over_several_chunks_per_work_item_and_several_slices(hip):
    """Two shapes the table above does not reach: a group of so many chunks that a work item of the split takes more than one, and an
    output so large that the layers are cut into slices of output rows and of chunks (300 rows of 2048 bins, 16 chunks).  The defined
    order makes never and always agree byte for byte there too; the first shape is also held against the model."""
    n, rows_out, group, hop = 64, 2, 40000, 1
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_NONE, False, 1.0 / n)
    iq = u8_iq(8, samples_for(n, hop, rows_out, group))
    got = {}
    for mode in (hip.REDUCE_SPLIT_NEVER, hip.REDUCE_SPLIT_ALWAYS):
        spec.set_reduce_split(mode)
        got[mode] = reduce_device(spec, iq, hop, rows_out, group, R.MEAN_POWER, R.LINEAR)
    assert got[hip.REDUCE_SPLIT_NEVER].tobytes() == got[hip.REDUCE_SPLIT_ALWAYS].tobytes()
    v, delta = R.spectrum_reduce(iq, n, M.IQ_U8, M.WINDOW_NONE, None, False, 1.0 / n, hop, rows_out, group, R.MEAN_POWER)
    R.check(got[hip.REDUCE_SPLIT_NEVER], v, delta, R.MEAN_POWER, R.LINEAR, FLOOR, "1250 chunks")

    n, rows_out, group, hop = 2048, 300, 500, 16
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0 / n)
    iq = u8_iq(9, samples_for(n, hop, rows_out, group))
    d_in = G.to_dev(iq)
    got = {}
    for mode in (hip.REDUCE_SPLIT_NEVER, hip.REDUCE_SPLIT_ALWAYS):
        spec.set_reduce_split(mode)
        got[mode] = reduce_device(spec, iq, hop, rows_out, group, R.MEAN_MAGNITUDE, R.DB, d_in=d_in)
    assert got[hip.REDUCE_SPLIT_NEVER].tobytes() == got[hip.REDUCE_SPLIT_ALWAYS].tobytes()
    # the first and the last output row alone (one slice, one tile) have the batch's bits
    for row in (0, rows_out - 1):
        part = iq[2 * row * group * hop:2 * (row * group * hop + samples_for(n, hop, 1, group))].copy()
        alone = reduce_device(spec, part, hop, 1, group, R.MEAN_MAGNITUDE, R.DB)
        assert alone[0].tobytes() == got[hip.REDUCE_SPLIT_NEVER][row].tobytes(), f"row {row}"


# ---- 6. position independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 4096])
def test_an_output_row_has_the_same_bits_wherever_it_stands(hip, n):
    rows_out, group, hop = 4, 5, n // 4
    iq = u8_iq(3 * n, samples_for(n, hop, rows_out, group))
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0)
    spec.set_route(hip.SPECTRUM_ROUTE_FUSED)
    for reduce, unit in ((R.MEAN_POWER, R.DB), (R.MEAN_MAGNITUDE, R.LINEAR), (R.MAX_MAGNITUDE, R.LINEAR)):
        batch = reduce_device(spec, iq, hop, rows_out, group, reduce, unit)
        for row in range(rows_out):
            first = row * group * hop
            part = iq[2 * first:2 * (first + samples_for(n, hop, 1, group))].copy()
            alone = reduce_device(spec, part, hop, 1, group, reduce, unit)
            assert alone[0].tobytes() == batch[row].tobytes(), f"reduce={reduce} unit={unit} row {row}"


# ---- 7. the hipFFT route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [3, 40])
@pytest.mark.parametrize("n,force", [(1000, False), (16384, False), (1024, True)])
def test_hipfft_route(hip, n, force, group):
    rows_out, hop = 2, n // 2 + 1
    iq = u8_iq(n + group, samples_for(n, hop, rows_out, group))
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0 / n)
    if force:
        spec.set_route(hip.SPECTRUM_ROUTE_HIPFFT)
    before, before_split = hip.spectrum_fused_launches(), hip.spectrum_reduce_split_launches()
    against_the_model(hip, spec, iq, (M.IQ_U8, M.WINDOW_HANNING, None, True, 1.0 / n), hop, rows_out, group, f"hipFFT route n={n} group={group}")
    assert hip.spectrum_fused_launches() == before and hip.spectrum_reduce_split_launches() == before_split, "the one-kernel route ran"


# ---- 8. cf32 input -------------------------------------------------------------------------------------------------------------
def test_cf32_input(hip):
    n, rows_out, group, hop = 512, 3, 4, 512 - 5
    iq = np.random.default_rng(n).standard_normal(2 * samples_for(n, hop, rows_out, group)).astype(np.float32)
    spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_BLACKMAN, False, 0.5)
    against_the_model(hip, spec, iq, (M.IQ_CF32, M.WINDOW_BLACKMAN, None, False, 0.5), hop, rows_out, group, "cf32")


# ---- 9. dB edges ---------------------------------------------------------------------------------------------------------------
def test_db_edges(hip):
    n, group, floor_db = 256, 3, -87.3
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_NONE, False, 1.0 / n)
    silence = np.full(2 * group * n, 128, np.uint8)
    for reduce in REDUCES:
        got = reduce_device(spec, silence, n, 1, group, reduce, R.DB, floor_db)
        assert np.array_equal(got, np.full((1, n), np.float32(floor_db))), f"reduce={reduce}: v = 0 gives the floor"
        assert np.array_equal(reduce_device(spec, silence, n, 1, group, reduce, R.LINEAR, floor_db), np.zeros((1, n), np.float32))
    k0 = 37
    j = np.arange(group * n)
    t = 100.0 * np.exp(2j * np.pi * k0 * j / n)
    tone = np.empty(2 * j.size, np.uint8)
    tone[0::2], tone[1::2] = np.round(128 + t.real), np.round(128 + t.imag)
    for reduce in REDUCES:
        v, delta = R.spectrum_reduce(tone, n, M.IQ_U8, M.WINDOW_NONE, None, False, 1.0 / n, n, 1, group, reduce)
        got = reduce_device(spec, tone, n, 1, group, reduce, R.DB, floor_db)
        assert int(np.argmax(got[0])) == k0
        R.check(got, v, delta, reduce, R.DB, floor_db, f"tone reduce={reduce}")
        want = (10.0 if reduce == R.MEAN_POWER else 20.0) * np.log10(100.0 / 128.0) * (2.0 if reduce == R.MEAN_POWER else 1.0)
        assert abs(float(got[0, k0]) - want) <= 0.05, "the peak of a tone of amplitude 100 / 128, up to the rounding to bytes"
        assert np.all(got >= np.float32(floor_db))


# ---- 10. argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing_and_write_nothing(hip):
    n, rows_out, group, hop = 256, 2, 3, 128
    n_samples = samples_for(n, hop, rows_out, group)
    iq = u8_iq(9, n_samples)
    spec = hip.Spectrum(n)
    d_in, d_out = G.to_dev(iq), G.dev_empty_f32(rows_out * n)

    def run(n_samples=n_samples, group=group, reduce=hip.REDUCE_MEAN_POWER, unit=hip.UNIT_DB, floor_db=-100.0):
        return hip.lib.sdrhip_spectrum_reduce_run_device(spec.h, None, G.ptr(d_in), n_samples, hop, rows_out, group, reduce, unit, floor_db, G.ptr(d_out))

    before, before_split = hip.spectrum_fused_launches(), hip.spectrum_reduce_split_launches()
    for bad in (dict(n_samples=n_samples - 1), dict(group=0), dict(floor_db=float("inf")), dict(floor_db=float("nan")), dict(reduce=3), dict(unit=-1)):
        assert run(**bad) == -1, bad                                            # SDRHIP_ERR_ARG
    assert hip.spectrum_fused_launches() == before and hip.spectrum_reduce_split_launches() == before_split
    assert np.all(np.isnan(G.to_host(d_out))), "nothing may be written"
    assert run() == 0
    assert hip.spectrum_fused_launches() == before + 1
    assert np.all(np.isfinite(G.to_host(d_out)))


# ---- 11. the host entry point --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 1000])
def test_host_entry_point_equals_reduce_device(hip, n):
    rows_out, group, hop = 3, 34, n - 3
    iq = u8_iq(n + 1, samples_for(n, hop, rows_out, group))
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_BLACKMAN, True, 3.0)
    for reduce, unit in ((R.MEAN_POWER, R.DB), (R.MAX_MAGNITUDE, R.LINEAR)):
        host = spec.reduce(iq, group, reduce, unit, FLOOR, hop=hop)
        assert host.shape == (rows_out, n)
        assert host.tobytes() == reduce_device(spec, iq, hop, rows_out, group, reduce, unit).tobytes()
