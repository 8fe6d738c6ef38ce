"""What tests/am_demod_cases.py reaches, shown on the CPU: the directed pairs have the bits the definition gives, ordinary data
already tells Data.Complex.magnitude from a correctly rounded hypot, and the wide-exponent stream tells it from the plain f32 formula
and holds subnormal inputs and outputs.  The device is held to the same table in tests/test_gpu_am_demod.py."""
import numpy as np

import agc_model
import am_demod_cases as AC


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _differ(a, b):
    return int((~AC.same(a, b)).sum())


def test_directed_pairs_have_the_expected_bits():
    z = AC.inputs()["directed"]
    m = AC.expected(z)
    assert m.dtype == np.float32 and m.size == len(AC.DIRECTED) == 27
    for (re, im, want), got in zip(AC.DIRECTED, m):
        if want is None:
            assert np.isnan(got), f"magnitude({re}, {im}) = {got!r}, expected NaN"
        else:
            assert _bits(got) == want, f"magnitude({re}, {im}) = {got!r} ({int(_bits(got)):#x}), expected {want:#x}"
    nonfinite = [(re, im, w) for re, im, w in AC.DIRECTED if not (np.isfinite(re) and np.isfinite(im))]
    assert len(nonfinite) == AC.N_NONFINITE
    for re, im, w in nonfinite:                           # a NaN part gives NaN; otherwise an infinite part gives +Inf
        assert (w is None) == (np.isnan(re) or np.isnan(im)) and (w is not None) == (w == AC.PINF)
    # the three consequences of the definition the issue names
    by = {(np.float32(re).item(), np.float32(im).item()): w for re, im, w in AC.DIRECTED if w is not None}
    assert by[(np.float32(1e-30).item(), 0.0)] == 0
    assert by[(np.float32(2.0 ** -149).item(), np.float32(2.0 ** -149).item())] == 1
    assert by[(AC.FLT_MAX, AC.FLT_MAX)] == AC.PINF and by[(AC.FLT_MAX, 1.0)] == 0x7F7FFFFF


def test_normal_stream_tells_magnitude_from_a_correctly_rounded_hypot():
    z = AC.inputs()["normal"]
    n = z.size
    assert n == 1 << 16
    re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    m = AC.expected(z)
    hyp = np.hypot(re, im)
    dbl = np.sqrt(re.astype(np.float64) ** 2 + im.astype(np.float64) ** 2).astype(np.float32)
    plain = np.sqrt(re * re + im * im)
    assert hyp.dtype == np.float32 and plain.dtype == np.float32
    d_hyp, d_dbl, d_plain = _differ(hyp, m), _differ(dbl, m), _differ(plain, m)
    print(f"    normal stream, {n} samples: hypot differs on {d_hyp}, the double root on {d_dbl}, the plain f32 formula on {d_plain}")
    # about one sample in six (the sum of the squares is rounded before the root): far more than a test could miss
    assert n // 8 < d_hyp < n // 4 and n // 8 < d_dbl < n // 4
    assert d_plain == 0                                    # nothing under- or overflows on ordinary data


def test_wide_stream_tells_magnitude_from_the_plain_formula_and_holds_subnormals():
    z = AC.inputs()["wide"]
    n = z.size
    re, im = np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)
    m = AC.expected(z)
    with np.errstate(all="ignore"):
        plain = np.sqrt(re * re + im * im)
    d_plain = _differ(plain, m)
    tiny = np.finfo(np.float32).tiny
    sub_in = int(((np.abs(re) < tiny) & (re != 0)).sum() + ((np.abs(im) < tiny) & (im != 0)).sum())
    sub_out = int(((m < tiny) & (m > 0)).sum())
    print(f"    wide stream, {n} samples: the plain f32 formula differs on {d_plain}; {sub_in} subnormal parts, {sub_out} subnormal outputs")
    assert d_plain > n // 3                               # almost half: one of the squares under- or overflows
    assert sub_in > 100 and sub_out > 10
    assert np.isfinite(m).all() and (m >= np.maximum(np.abs(re), np.abs(im)) * np.float32(0.999)).all()


def test_mixed_rows_hold_all_three_kinds_and_the_truth_is_elementwise():
    for n in (0, 1, 5, 27, 100, 1027):
        for seed in (0, 3):
            z = AC.mixed(n, seed)
            assert z.dtype == np.complex64 and z.size == n
            d = min(n, len(AC.DIRECTED))
            assert np.array_equal(z[:d].view(np.uint32), AC.inputs()["directed"][:d].view(np.uint32))
    z = AC.mixed(1027, 1)
    m = AC.expected(z)
    # element-wise: any slice's truth is the slice of the truth (what lets one reference serve every length and row)
    AC.assert_same(AC.expected(z[100:611]), m[100:611], "a slice")
    AC.assert_same(AC.expected(z.reshape(13, 79)), m, "a reshape")
    assert int(np.isnan(m).sum()) == 4 and int(np.isinf(m).sum()) == 4            # the seven Inf / NaN pairs and (FLT_MAX, FLT_MAX)
    assert agc_model.magnitude(np.float32(3), np.float32(4)) == np.float32(5)
