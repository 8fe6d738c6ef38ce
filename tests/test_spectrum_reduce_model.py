"""The reducing form of the spectrum operator without a GPU: the numpy restatement of its definition (tests/spectrum_reduce_model.py)
against the operator's own model, a closed form and a plain loop, and the C ABI / binding surface of the new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import spectrum_model as M
import spectrum_reduce_model as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REDUCE_FUNCTIONS = ["sdrhip_spectrum_reduce_run_device", "sdrhip_spectrum_reduce_run", "sdrhip_spectrum_set_reduce_split",
                    "sdrhip_debug_spectrum_reduce_split_launches", "sdrhip_debug_spectrum_reduce_layer_launches"]


def test_group_of_one_mean_magnitude_is_the_operator():
    n, rows, hop = 64, 5, 37
    iq = np.random.default_rng(1).integers(0, 256, 2 * ((rows - 1) * hop + n), dtype=np.uint8)
    mag, out = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HAMMING, None, True, 0.75, hop, rows)
    v, delta = R.spectrum_reduce(iq, n, M.IQ_U8, M.WINDOW_HAMMING, None, True, 0.75, hop, rows, 1, R.MEAN_MAGNITUDE)
    assert np.array_equal(v, mag)
    assert np.array_equal(R.expected(v, R.MEAN_MAGNITUDE, R.LINEAR, -100.0), out)
    assert np.array_equal(delta, np.broadcast_to(1e-11 * mag.max(axis=1, keepdims=True), mag.shape))
    vmax, dmax = R.spectrum_reduce(iq, n, M.IQ_U8, M.WINDOW_HAMMING, None, True, 0.75, hop, rows, 1, R.MAX_MAGNITUDE)
    assert np.array_equal(vmax, mag) and np.array_equal(dmax, delta)


def test_mean_power_of_a_unit_tone_is_the_closed_form():
    """x[j] = exp(2 pi i k0 j / n), no window, scale 1 / n: every row has m[k0] = 1 and nothing elsewhere, so the mean power is 1 in
    bin k0 (0 dB) and the floor everywhere else."""
    n, k0, group, rows_out = 64, 5, 40, 2
    j = np.arange(rows_out * group * n)
    t = np.exp(2j * np.pi * k0 * j / n)
    iq = np.empty(2 * j.size, np.float32)
    iq[0::2], iq[1::2] = t.real, t.imag
    v, delta = R.spectrum_reduce(iq, n, M.IQ_CF32, M.WINDOW_NONE, None, False, 1.0 / n, n, rows_out, group, R.MEAN_POWER)
    assert v.shape == (rows_out, n)
    assert np.max(np.abs(v[:, k0] - 1.0)) <= 1e-6                   # float32 samples of the tone
    rest = np.delete(v, k0, axis=1)
    assert np.max(rest) <= 1e-12
    db = R.expected(v, R.MEAN_POWER, R.DB, -60.0)
    assert np.max(np.abs(db[:, k0])) <= 1e-5 and np.all(np.delete(db, k0, axis=1) == np.float32(-60.0))
    assert np.all(delta[:, k0] <= 3e-11) and np.all(delta >= 0)


@pytest.mark.parametrize("group", [1, 31, 32, 33, 70])
def test_chunked_order_is_the_plain_loop(group):
    rng = np.random.default_rng(group)
    x = rng.standard_normal((group, 3)) * 10.0 ** rng.integers(-8, 8, (group, 3))
    want = []
    for k in range(3):
        total, acc = 0.0, 0.0
        for r in range(group):
            if r and r % 32 == 0:
                total, acc = total + acc, 0.0
            acc = acc + float(x[r, k])
        want.append(total + acc)
    assert np.array_equal(R.chunked_sum(x), np.array(want))
    v, _ = R.reduce_rows(np.abs(x), group, R.MEAN_MAGNITUDE)
    assert np.array_equal(v[0], R.chunked_sum(np.abs(x)) / group)


def test_db_and_the_floor():
    v = np.array([[0.0, 1e-30, 1.0, 100.0]])
    assert np.array_equal(R.to_db(v, R.MEAN_POWER, -120.0), np.array([[-120.0, -120.0, 0.0, 20.0]]))
    assert np.array_equal(R.to_db(v, R.MAX_MAGNITUDE, -120.0), np.array([[-120.0, -120.0, 0.0, 40.0]]))
    R.check(np.array([[-120.0, -120.0, 0.0, 20.0]], np.float32), v, np.zeros_like(v), R.MEAN_POWER, R.DB, -120.0)
    with pytest.raises(AssertionError):
        R.check(np.array([[-120.0, -120.0, 1e-3, 20.0]], np.float32), v, np.zeros_like(v), R.MEAN_POWER, R.DB, -120.0)
    with pytest.raises(AssertionError):
        R.check(np.array([[0.0, 1e-30, 1.0 + 1e-6, 100.0]]), v, np.zeros_like(v), R.MEAN_POWER, R.LINEAR, -120.0)


def test_header_declares_and_library_exports_the_reduce_entry_points():
    """Fails on a tree without the reducing form."""
    text = open(os.path.join(ROOT, "include", "sdr_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in REDUCE_FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, code), f"{name} is not declared in sdr_hip.h"
    for macro, value in (("SDRHIP_REDUCE_MEAN_POWER", 0), ("SDRHIP_REDUCE_MEAN_MAGNITUDE", 1), ("SDRHIP_REDUCE_MAX_MAGNITUDE", 2),
                         ("SDRHIP_UNIT_LINEAR", 0), ("SDRHIP_UNIT_DB", 1)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), code), macro
    assert "chunks of 32 consecutive input rows" in text, "the header states the summation order"
    import sdr_amd.lib as L
    product = C.CDLL(L.LIB_PATH)
    for name in REDUCE_FUNCTIONS:
        assert hasattr(product, name), f"{name} is not exported"
        assert getattr(L.lib, name).argtypes is not None, f"{name} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_spectrum_reduce_split_launches.restype is C.c_longlong
    assert L.spectrum_reduce_split_launches() >= 0
    assert L.lib.sdrhip_debug_spectrum_reduce_layer_launches.restype is C.c_longlong and L.spectrum_reduce_layer_launches() >= 0
    for method in ("reduce", "reduce_device", "set_reduce_split"):
        assert hasattr(L.Spectrum, method), method
    assert (L.REDUCE_MEAN_POWER, L.REDUCE_MEAN_MAGNITUDE, L.REDUCE_MAX_MAGNITUDE) == (R.MEAN_POWER, R.MEAN_MAGNITUDE, R.MAX_MAGNITUDE)
    assert (L.UNIT_LINEAR, L.UNIT_DB) == (R.LINEAR, R.DB)
    hs = open(os.path.join(ROOT, "haskell", "SDR", "GPU.hs")).read()
    m = re.search(r'foreign import ccall safe "sdrhip_spectrum_reduce_run"\s+\w+\s*::(.*)', hs)
    assert m, "haskell/SDR/GPU.hs does not import sdrhip_spectrum_reduce_run"
    assert m.group(1).count("->") == 10, "ten arguments, as in the header"


def test_argument_errors_need_no_device():
    import sdr_amd.lib as L
    s = L.Spectrum(256)
    n_samples = (2 * 3 - 1) * 128 + 256
    iq = np.zeros(2 * n_samples, np.uint8)
    out = np.full(2 * 256, np.nan, np.float32)

    def run(n_samples=n_samples, hop=128, rows_out=2, group=3, reduce=L.REDUCE_MEAN_POWER, unit=L.UNIT_DB, floor_db=-100.0):
        return L.lib.sdrhip_spectrum_reduce_run(s.h, iq.ctypes.data, n_samples, hop, rows_out, group, reduce, unit, floor_db, out.ctypes.data)

    before = L.spectrum_fused_launches()
    for bad in (dict(n_samples=n_samples - 1), dict(group=0), dict(rows_out=0), dict(hop=0), dict(reduce=3), dict(reduce=-1), dict(unit=2),
                dict(floor_db=float("nan")), dict(floor_db=float("-inf")), dict(rows_out=1 << 16, group=1 << 15)):
        assert run(**bad) == -1, bad                             # SDRHIP_ERR_ARG
    assert L.spectrum_fused_launches() == before and np.all(np.isnan(out))
    with pytest.raises(L.SdrHipError):
        s.set_reduce_split(3)
    s.set_reduce_split(L.REDUCE_SPLIT_ALWAYS)
    s.set_reduce_split(L.REDUCE_SPLIT_AUTO)
