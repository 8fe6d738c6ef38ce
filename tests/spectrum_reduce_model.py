"""The reducing form of the spectrum operator (include/sdr_hip.h, sdrhip_spectrum_reduce_*) restated in numpy, float64 throughout.

With m_r[k] = scale * |X_r[k]| the magnitudes of input row r (spectrum_model.spectrum, before the final rounding), output row R
reduces input rows R*group .. R*group + group - 1:

    MEAN_POWER v = (sum of m^2) / group      MEAN_MAGNITUDE v = (sum of m) / group      MAX_MAGNITUDE v = max m
    LINEAR out = float32(v)                  DB out = float32(max(floor_db, c log10 v)),  c = 10 for MEAN_POWER, 20 otherwise

The sums follow the defined order: chunks of 32 consecutive rows, each summed in ascending order from 0.0, the chunk sums then added
in ascending order from 0.0.

Non-finite cf32 input: numpy's sums, np.max and np.maximum propagate a NaN, and so does the definition (include/sdr_hip.h): a NaN
magnitude makes its output bin NaN in every reduce and unit.

Tolerance: tests/test_gpu_spectrum.py allows each input row e_r = 1e-11 * max_k m_r[k] before the final rounding.  Carried through
the reductions that is, per bin, delta = mean_r e_r (MEAN_MAGNITUDE), max_r e_r (MAX_MAGNITUDE) and mean_r (2 m_r[k] e_r + e_r^2)
(MEAN_POWER)."""
import numpy as np

import spectrum_model as M

MEAN_POWER, MEAN_MAGNITUDE, MAX_MAGNITUDE = 0, 1, 2
LINEAR, DB = 0, 1
CHUNK = 32


def chunked_sum(x):
    """x: group x ... -> the sum over axis 0 in the defined order."""
    total = np.zeros(x.shape[1:], np.float64)
    for c0 in range(0, x.shape[0], CHUNK):
        acc = np.zeros(x.shape[1:], np.float64)
        for r in range(c0, min(c0 + CHUNK, x.shape[0])):
            acc = acc + x[r]
        total = total + acc
    return total


def reduce_rows(mag, group, reduce):
    """mag: (rows_out * group) x n float64 magnitudes -> (v, delta), rows_out x n each."""
    rows, n = mag.shape
    assert group >= 1 and rows % group == 0
    m = mag.reshape(rows // group, group, n)
    e = 1e-11 * np.max(m, axis=2, keepdims=True)                    # rows_out x group x 1
    if reduce == MEAN_POWER:
        v = np.stack([chunked_sum(g * g) for g in m]) / group
        delta = np.mean(2.0 * m * e + e * e, axis=1)
    elif reduce == MEAN_MAGNITUDE:
        v = np.stack([chunked_sum(g) for g in m]) / group
        delta = np.broadcast_to(np.mean(e, axis=1), v.shape).copy()
    elif reduce == MAX_MAGNITUDE:
        v = np.max(m, axis=1)
        delta = np.broadcast_to(np.max(e, axis=1), v.shape).copy()
    else:
        raise ValueError(reduce)
    return v, delta


def to_db(v, reduce, floor_db):
    c = 10.0 if reduce == MEAN_POWER else 20.0
    with np.errstate(divide="ignore"):
        return np.maximum(floor_db, c * np.log10(v))


def spectrum_reduce(iq, n, input_format=M.IQ_U8, kind=M.WINDOW_NONE, custom=None, half_band_shift=False, scale=1.0, hop=None, rows_out=1,
                    group=1, reduce=MEAN_POWER):
    """-> (v, delta): rows_out x n float64, the reduced value before unit and final rounding, and its tolerance."""
    mag, _ = M.spectrum(iq, n, input_format, kind, custom, half_band_shift, scale, hop, rows_out * group)
    return reduce_rows(mag, group, reduce)


def expected(v, reduce, unit, floor_db):
    """The float32 output the definition gives for v."""
    return (v if unit == LINEAR else to_db(v, reduce, floor_db)).astype(np.float32)


def _ulp32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def check(got, v, delta, reduce, unit, floor_db, what=""):
    """LINEAR: |got - v| <= delta + 2^-23 |v|.  DB: got within [dB(max(v - delta, 0)), dB(v + delta)], both ends clamped below by
    floor_db and widened by one float32 ulp of that end's value.  A bin whose v is NaN (non-finite cf32 input: the definition's sums,
    max and maximum all propagate it) must be NaN, whatever its payload; every other bin must be finite."""
    got = np.asarray(got, dtype=np.float64).reshape(v.shape)
    nan = np.isnan(v)
    assert np.all(np.isnan(got[nan])), f"{what}: {int((~np.isnan(got[nan])).sum())} bins that the definition makes NaN are not"
    assert np.all(np.isfinite(got[~nan])), f"{what}: non-finite bins (a row not written?)"
    if nan.any():                                    # the poisoned bins are settled (v = 1 exactly met): compare the others
        got, v, delta = np.where(nan, 1.0 if unit == LINEAR else 0.0, got), np.where(nan, 1.0, v), np.where(nan, 0.0, delta)
    if unit == LINEAR:
        err, bound = np.abs(got - v), delta + 2.0 ** -23 * np.abs(v)
        worst = np.unravel_index(np.argmax(err - bound), err.shape)
        print(f"{what}: max |got - v| = {err.max():.3e}, worst bin {worst}: err {err[worst]:.3e} vs bound {bound[worst]:.3e}")
        assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} bins outside the tolerance, worst {worst}: {err[worst]:.3e} > {bound[worst]:.3e}"
    else:
        lo = to_db(np.maximum(v - delta, 0.0), reduce, floor_db)
        hi = to_db(v + delta, reduce, floor_db)
        lo, hi = lo - _ulp32(lo), hi + _ulp32(hi)
        out = np.maximum(lo - got, got - hi)
        worst = np.unravel_index(np.argmax(out), out.shape)
        print(f"{what}: worst bin {worst}: got {got[worst]:.9g} dB, allowed [{lo[worst]:.9g}, {hi[worst]:.9g}]")
        assert np.all(out <= 0.0), f"{what}: {int((out > 0).sum())} bins outside the dB interval, worst {worst}: {got[worst]!r} not in [{lo[worst]!r}, {hi[worst]!r}]"
