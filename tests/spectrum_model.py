"""The spectrum operator's definition (include/sdr_hip.h, sdrhip_spectrum_*) restated in numpy, float64 throughout:

    x'[j]  = x[j] * (half_band_shift ? (-1)^j : 1) * w[j]
    X      = forward DFT of x', unnormalised, sign exp(-2 pi i jk/n)      (numpy.fft uses FFTW's conventions)
    out[k] = float32(scale * |X[k]|)

The windows are the reference's (FilterDesign.hs:39-60), with denominator n - 1; u8 IQ converts as (v - 128) / 128
(Util.hs:92-98)."""
import numpy as np

IQ_U8, IQ_CF32 = 0, 1
WINDOW_NONE, WINDOW_HANNING, WINDOW_HAMMING, WINDOW_BLACKMAN, WINDOW_CUSTOM = 0, 1, 2, 3, 4


def window(kind, n, custom=None):
    j = np.arange(n, dtype=np.float64)
    if kind == WINDOW_NONE:
        return np.ones(n, np.float64)
    if kind == WINDOW_HANNING:
        return 0.5 * (1 - np.cos((2 * np.pi * j) / (n - 1)))
    if kind == WINDOW_HAMMING:
        return 0.54 - 0.46 * np.cos((2 * np.pi * j) / (n - 1))
    if kind == WINDOW_BLACKMAN:
        return 0.42 - 0.5 * np.cos((2 * np.pi * j) / (n - 1)) + 0.08 * np.cos((4 * np.pi * j) / (n - 1))
    if kind == WINDOW_CUSTOM:
        w = np.asarray(custom, dtype=np.float64)
        assert w.shape == (n,)
        return w
    raise ValueError(kind)


def to_complex(iq, input_format):
    """Interleaved samples -> complex128."""
    if input_format == IQ_U8:
        v = (np.asarray(iq, dtype=np.uint8).astype(np.float64) - 128.0) / 128.0
    else:
        v = np.asarray(iq, dtype=np.float32).astype(np.float64)
    return v[0::2] + 1j * v[1::2]


def prepared_rows(iq, n, input_format, w, half_band_shift, hop, rows):
    """rows x n complex128: converted, sign-alternated, windowed."""
    x = to_complex(iq, input_format)
    assert hop >= 1 and (rows - 1) * hop + n <= x.size
    idx = np.arange(rows)[:, None] * hop + np.arange(n)[None, :]
    sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0) if half_band_shift else np.ones(n)
    return x[idx] * (sign * w)[None, :]


def spectrum(iq, n, input_format=IQ_U8, kind=WINDOW_NONE, custom=None, half_band_shift=False, scale=1.0, hop=None, rows=1):
    """-> (rows x n float64 before the final rounding, rows x n float32)."""
    hop = n if hop is None else hop
    xp = prepared_rows(iq, n, input_format, window(kind, n, custom), half_band_shift, hop, rows)
    mag = scale * np.abs(np.fft.fft(xp, axis=1))
    return mag, mag.astype(np.float32)


def direct_dft(x):
    """The O(n^2) sum the definition names."""
    n = x.shape[-1]
    k = np.arange(n)
    return x @ np.exp(-2j * np.pi * np.outer(k, k) / n)
