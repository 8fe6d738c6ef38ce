"""The spectrum operator without a GPU: the numpy restatement of its definition (tests/spectrum_model.py) against a direct
O(n^2) DFT sum and the reference's window formulas (FilterDesign.hs:39-60), and the C ABI / binding surface of the operator."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import spectrum_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SPECTRUM_FUNCTIONS = ["sdrhip_spectrum_create", "sdrhip_spectrum_destroy", "sdrhip_spectrum_size", "sdrhip_spectrum_window",
                      "sdrhip_spectrum_run_device", "sdrhip_spectrum_run", "sdrhip_spectrum_set_route",
                      "sdrhip_debug_spectrum_fused_launches", "sdrhip_debug_spectrum_hipfft_batches"]


@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("shift", [False, True])
def test_model_equals_the_direct_dft_sum(n, shift):
    rng = np.random.default_rng(n)
    rows, hop, scale = 3, n // 2 + 1, 0.75
    iq = rng.integers(0, 256, 2 * ((rows - 1) * hop + n), dtype=np.uint8)
    w = M.window(M.WINDOW_HAMMING, n)
    mag, out = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HAMMING, None, shift, scale, hop, rows)
    x = (iq.astype(np.float64) - 128.0) / 128.0
    x = x[0::2] + 1j * x[1::2]
    for r in range(rows):
        xp = np.array([x[r * hop + j] * ((-1.0) ** j if shift else 1.0) * w[j] for j in range(n)])
        ref = scale * np.abs(M.direct_dft(xp))
        assert np.max(np.abs(mag[r] - ref)) <= 1e-12 * np.max(ref)
    assert out.dtype == np.float32 and np.array_equal(out, mag.astype(np.float32))


@pytest.mark.parametrize("n", [9, 64, 1024])
def test_windows_equal_the_reference_formulas(n):
    han, ham, bla = (M.window(k, n) for k in (M.WINDOW_HANNING, M.WINDOW_HAMMING, M.WINDOW_BLACKMAN))
    # the end points and, for odd n, the exact middle sample: closed forms
    for j, c1, c2 in [(0, 1.0, 1.0), (n - 1, 1.0, 1.0)] + ([((n - 1) // 2, -1.0, 1.0)] if n % 2 else []):
        assert han[j] == pytest.approx(0.5 * (1 - c1), abs=1e-15)
        assert ham[j] == pytest.approx(0.54 - 0.46 * c1, abs=1e-15)
        assert bla[j] == pytest.approx(0.42 - 0.5 * c1 + 0.08 * c2, abs=1e-15)
    # j = (n - 1) / 2 rounded down, whatever the parity of n: the formula itself, term by term
    j = (n - 1) // 2
    a = (2 * math.pi * j) / (n - 1)
    assert han[j] == pytest.approx(0.5 * (1 - math.cos(a)), abs=1e-15)
    assert ham[j] == pytest.approx(0.54 - 0.46 * math.cos(a), abs=1e-15)
    assert bla[j] == pytest.approx(0.42 - 0.5 * math.cos(a) + 0.08 * math.cos((4 * math.pi * j) / (n - 1)), abs=1e-15)
    assert np.array_equal(M.window(M.WINDOW_NONE, n), np.ones(n))


def test_header_declares_and_binding_binds_the_operator():
    """Fails on a tree without the operator: every sdrhip_spectrum_* function is declared in sdr_hip.h, exported, and bound in
    sdr_amd/lib.py with argument types."""
    text = open(os.path.join(ROOT, "include", "sdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SPECTRUM_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in sdr_hip.h"
    for macro in ("SDRHIP_IQ_U8", "SDRHIP_IQ_CF32", "SDRHIP_WINDOW_NONE", "SDRHIP_WINDOW_HANNING", "SDRHIP_WINDOW_HAMMING",
                  "SDRHIP_WINDOW_BLACKMAN", "SDRHIP_WINDOW_CUSTOM"):
        assert re.search(r"#define\s+%s\s+\d" % macro, code), macro
    import sdr_amd.lib as L
    product = C.CDLL(L.LIB_PATH)
    for name in SPECTRUM_FUNCTIONS:
        assert hasattr(product, name), f"{name} is not exported"
        assert getattr(L.lib, name).argtypes is not None, f"{name} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_spectrum_fused_launches.restype is C.c_longlong
    assert L.lib.sdrhip_debug_spectrum_hipfft_batches.restype is C.c_longlong and L.spectrum_hipfft_batches() >= 0
    assert hasattr(L, "Spectrum") and hasattr(L.Spectrum, "run") and hasattr(L.Spectrum, "run_device")
    assert (L.IQ_U8, L.IQ_CF32) == (M.IQ_U8, M.IQ_CF32)
    assert (L.WINDOW_NONE, L.WINDOW_HANNING, L.WINDOW_HAMMING, L.WINDOW_BLACKMAN, L.WINDOW_CUSTOM) == (0, 1, 2, 3, 4)


@pytest.mark.parametrize("n", [2, 64, 1000])
def test_library_windows_are_the_model_windows(n):
    """Descriptors live on the host: create and sdrhip_spectrum_window need no device."""
    import sdr_amd.lib as L
    for kind in (M.WINDOW_NONE, M.WINDOW_HANNING, M.WINDOW_HAMMING, M.WINDOW_BLACKMAN):
        s = L.Spectrum(n, L.IQ_U8, kind)
        assert np.max(np.abs(s.window() - M.window(kind, n))) <= 1e-15
        assert L.lib.sdrhip_spectrum_size(s.h) == n
    custom = np.random.default_rng(n).standard_normal(n)
    assert np.array_equal(L.Spectrum(n, L.IQ_CF32, M.WINDOW_CUSTOM, custom_window=custom).window(), custom)


def test_argument_errors_need_no_device():
    import sdr_amd.lib as L
    with pytest.raises(L.SdrHipError):
        L.Spectrum(1)                                        # the windows divide by n - 1
    with pytest.raises(L.SdrHipError):
        L.Spectrum(64, 7)
    with pytest.raises(L.SdrHipError):
        L.Spectrum(64, L.IQ_U8, M.WINDOW_CUSTOM)             # a custom window without its values
    s = L.Spectrum(1000)
    with pytest.raises(L.SdrHipError):
        s.set_route(L.SPECTRUM_ROUTE_FUSED)                  # not a power of two
    s.set_route(L.SPECTRUM_ROUTE_HIPFFT)
    iq = np.zeros(2 * 1999, np.uint8)
    before = L.spectrum_fused_launches()
    assert L.lib.sdrhip_spectrum_run(s.h, iq.ctypes.data, 1999, 1000, 2, np.empty(2000, np.float32).ctypes.data) == -1   # one sample short
    assert L.spectrum_fused_launches() == before
