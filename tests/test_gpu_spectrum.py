"""The spectrum operator on the device (sdr_amd/csrc/kernels_spectrum.hip, fft.cpp): raw IQ -> windowed FFT magnitude rows, against
the numpy restatement of its definition (tests/spectrum_model.py).  Every bin of every row must satisfy

    |got - ref| <= 1e-11 * max|ref| + 2^-23 * |ref|

the first term being the project's contract for the double-precision transform (tests/test_gpu_fft.py), with max|ref| taken over
the bin's own row, the second one float32 unit in the last place for the final rounding.  Outputs come from gpu_util.dev_empty_f32: a row written
out of place trips the NaN guard bands."""

import numpy as np
import pytest

import gpu_util as G
import spectrum_model as M

pytestmark = pytest.mark.gpu


def assert_close(got, ref64, what=""):
    got = np.asarray(got, dtype=np.float64).reshape(ref64.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite bins (a row not written?)"
    bound = 1e-11 * np.max(np.abs(ref64), axis=-1, keepdims=True) + 2.0 ** -23 * np.abs(ref64)
    err = np.abs(got - ref64)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: max |got - ref| = {err.max():.3e}, worst bin {worst}: err {err[worst]:.3e} vs bound {bound[worst]:.3e}")
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} bins outside the tolerance, worst {worst}: {err[worst]:.3e} > {bound[worst]:.3e}"


def run_device(hip, spec, iq, hop, rows):
    """iq: host array of interleaved samples -> rows x n float32 through run_device on guarded device memory."""
    d_in = G.to_dev(iq)
    d_out = G.dev_empty_f32(rows * spec.n)
    spec.run_device(G.ptr(d_in), iq.size // 2, G.ptr(d_out), hop=hop, rows=rows)
    return G.to_host(d_out).reshape(rows, spec.n)


def u8_iq(seed, n_samples):
    return np.random.default_rng(seed).integers(0, 256, 2 * n_samples, dtype=np.uint8)


def u8_tone(n, k, n_samples):
    j = np.arange(n_samples)
    t = 100.0 * np.exp(2j * np.pi * k * j / n)
    iq = np.empty(2 * n_samples, np.uint8)
    iq[0::2] = np.round(128 + t.real)
    iq[1::2] = np.round(128 + t.imag)
    return iq


def fused_8192_is_routed_away():
    """The header says which route 8192 takes: `(8192 included ...)` unless the one-kernel route ends at 4096."""
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdr_hip.h")).read()
    return "from 64 to 8192" not in text


# ---- 1. sizes on the one-kernel route -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 128, 256, 4096, 8192])
def test_sizes_on_the_one_kernel_route(hip, n):
    rows, scale = 3, 1.0 / n
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, scale)
    for what, iq in (("random", u8_iq(n, rows * n)), ("tone", u8_tone(n, 5, rows * n))):
        before = hip.spectrum_fused_launches()
        got = run_device(hip, spec, iq, n, rows)
        launched = hip.spectrum_fused_launches() - before
        if n == 8192 and fused_8192_is_routed_away():
            assert launched == 0
        else:
            assert launched == 1, "the one-kernel route did not run"
        ref64, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, scale, n, rows)
        assert_close(got, ref64, f"n={n} {what}")


# ---- 2. rows and hops ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rows,hop", [(256, 1, 256), (256, 6, 128), (256, 5, 256 + 37), (64, 700, 64)])
def test_rows_and_hops(hip, n, rows, hop):
    n_samples = (rows - 1) * hop + n                 # the last row ends exactly at n_samples
    iq = u8_iq(rows + hop, n_samples)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HAMMING, True, 1.0)
    before = hip.spectrum_fused_launches()
    got = run_device(hip, spec, iq, hop, rows)
    assert hip.spectrum_fused_launches() == before + 1
    ref64, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HAMMING, None, True, 1.0, hop, rows)
    assert_close(got, ref64, f"n={n} rows={rows} hop={hop}")


def test_one_sample_short_is_an_argument_error_without_a_launch(hip):
    n, rows, hop = 256, 4, 128
    n_samples = (rows - 1) * hop + n
    iq = u8_iq(9, n_samples)
    spec = hip.Spectrum(n)
    d_in, d_out = G.to_dev(iq), G.dev_empty_f32(rows * n)
    before = hip.spectrum_fused_launches()
    rc = hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d_in), n_samples - 1, hop, rows, G.ptr(d_out))
    assert rc == -1                                                             # SDRHIP_ERR_ARG
    assert hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d_in), n_samples, 0, rows, G.ptr(d_out)) == -1   # hop >= 1
    assert hip.spectrum_fused_launches() == before
    assert np.all(np.isnan(G.to_host(d_out))), "nothing may be written"
    assert hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d_in), n_samples, hop, rows, G.ptr(d_out)) == 0
    assert hip.spectrum_fused_launches() == before + 1
    assert np.all(np.isfinite(G.to_host(d_out)))


# ---- 3. each window, shift on and off ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("kind", [M.WINDOW_NONE, M.WINDOW_HANNING, M.WINDOW_HAMMING, M.WINDOW_BLACKMAN, M.WINDOW_CUSTOM])
def test_each_window(hip, kind, shift):
    n, rows = 1024, 2
    custom = np.random.default_rng(77).standard_normal(n) if kind == M.WINDOW_CUSTOM else None
    spec = hip.Spectrum(n, hip.IQ_U8, kind, shift, 2.0, custom_window=custom)
    assert np.max(np.abs(spec.window() - M.window(kind, n, custom))) <= 1e-15
    iq = u8_iq(100 + kind, rows * n)
    ref64, _ = M.spectrum(iq, n, M.IQ_U8, kind, custom, shift, 2.0, n, rows)
    assert_close(run_device(hip, spec, iq, n, rows), ref64, f"window {kind} shift {shift}")
    tone = u8_tone(n, 37, n)
    got = run_device(hip, spec, tone, n, 1)
    ref64, _ = M.spectrum(tone, n, M.IQ_U8, kind, custom, shift, 2.0, n, 1)
    assert_close(got, ref64, f"window {kind} shift {shift} tone")
    if kind != M.WINDOW_CUSTOM:                       # a random window smears the tone over every bin
        assert int(np.argmax(got[0])) == (37 + n // 2 if shift else 37)


# ---- 4. cf32 input -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 8192])
def test_cf32_input(hip, n):
    rows, hop = 3, n - 5
    iq = np.random.default_rng(n).standard_normal(2 * ((rows - 1) * hop + n)).astype(np.float32)
    spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_BLACKMAN, False, 0.5)
    ref64, _ = M.spectrum(iq, n, M.IQ_CF32, M.WINDOW_BLACKMAN, None, False, 0.5, hop, rows)
    assert_close(run_device(hip, spec, iq, hop, rows), ref64, f"cf32 n={n}")


def test_a_decimator_output_buffer_feeds_the_operator_on_device_memory(hip):
    import signals as S
    n, factor = 512, 8
    taps = S.taps_decim127()
    dec = hip.Decimator(factor, taps, hip.ORDER_AVX, complex_=True)
    count = n
    x = np.random.default_rng(5).standard_normal(2 * ((count - 1) * factor + dec.num_coeffs + 64)).astype(np.float32)
    d_x, d_y = G.to_dev(x), G.dev_empty_f32(2 * count)
    dec.run(G.ptr(d_x), 0, G.ptr(d_y), 0, count)
    spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_HANNING, True, 1.0)
    d_out = G.dev_empty_f32(n)
    before = hip.spectrum_fused_launches()
    assert spec.run_device(G.ptr(d_y), count, G.ptr(d_out)) == 1
    assert hip.spectrum_fused_launches() == before + 1
    y = G.to_host(d_y)                                 # the decimator's own output is the operator's input: the model starts there
    ref64, _ = M.spectrum(y, n, M.IQ_CF32, M.WINDOW_HANNING, None, True, 1.0, n, 1)
    assert np.max(ref64) > 0
    assert_close(G.to_host(d_out), ref64, "decimator -> spectrum")


# ---- 5. the hipFFT route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,force", [(1000, False), (16384, False), (1024, True)])
def test_hipfft_route(hip, n, force):
    rows, hop = 3, n // 2 + 1
    iq = u8_iq(n, (rows - 1) * hop + n)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0 / n)
    if force:
        spec.set_route(hip.SPECTRUM_ROUTE_HIPFFT)
    before = hip.spectrum_fused_launches()
    got = run_device(hip, spec, iq, hop, rows)
    tone = u8_tone(n, 37, n)
    got_tone = run_device(hip, spec, tone, n, 1)
    assert hip.spectrum_fused_launches() == before, "the one-kernel route ran"
    ref64, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, 1.0 / n, hop, rows)
    assert_close(got, ref64, f"hipFFT route n={n}")
    ref64, _ = M.spectrum(tone, n, M.IQ_U8, M.WINDOW_HANNING, None, True, 1.0 / n, n, 1)
    assert_close(got_tone, ref64, f"hipFFT route n={n} tone")


# ---- 6. position independence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [128, 4096])
def test_a_row_has_the_same_bits_wherever_it_stands(hip, n):
    rows, hop = 5, n // 4
    iq = u8_iq(3 * n, (rows - 1) * hop + n)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0)
    spec.set_route(hip.SPECTRUM_ROUTE_FUSED)
    batch = run_device(hip, spec, iq, hop, rows)
    for r in range(rows):
        alone = run_device(hip, spec, iq[2 * r * hop:2 * (r * hop + n)].copy(), n, 1)
        assert alone[0].tobytes() == batch[r].tobytes(), f"row {r}"


# ---- 7. the host entry point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 1000])
def test_host_entry_point_equals_run_device(hip, n):
    rows, hop = 4, n - 3
    iq = u8_iq(n + 1, (rows - 1) * hop + n)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_BLACKMAN, True, 3.0)
    host = spec.run(iq, hop=hop)
    assert host.shape == (rows, n)
    assert host.tobytes() == run_device(hip, spec, iq, hop, rows).tobytes()


# ---- 8. edge values ------------------------------------------------------------------------------------------------------------
def test_edge_values(hip):
    n, scale = 256, 0.25
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_NONE, False, scale)
    zeros = run_device(hip, spec, np.full(2 * n, 128, np.uint8), n, 1)
    assert np.array_equal(zeros, np.zeros((1, n), np.float32))
    full = np.full(2 * n, 255, np.uint8)
    got = run_device(hip, spec, full, n, 1)
    ref64, _ = M.spectrum(full, n, M.IQ_U8, M.WINDOW_NONE, None, False, scale, n, 1)
    assert ref64[0, 0] == pytest.approx(n * 127 / 128 * np.sqrt(2.0) * scale, rel=1e-14)
    assert_close(got, ref64, "all 255")
