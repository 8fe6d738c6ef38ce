"""The inputs of the amDemod tests (sdrhip_am_demod_run / _run_rows / sdrhip_pipe_am_demod): a directed list, a seeded normal stream
and a seeded wide-exponent stream, all as complex64.  The truth is agc_model.magnitude on every sample, compared bit for bit with NaN
by position (`same`).  tests/test_am_demod_cases.py shows on the CPU what the table reaches; tests/test_gpu_am_demod.py runs it."""
import numpy as np

import agc_model

FLT_MAX = float(np.finfo(np.float32).max)
INF, NAN = float("inf"), float("nan")
PINF, QNAN = 0x7F800000, None           # expected bits; None = any NaN

# (re, im, expected bits): what the definition gives (k = the larger exponent, exponent 0 = 0); the CPU test holds the model to them
DIRECTED = [
    (0.0, 0.0, 0x00000000), (-0.0, 0.0, 0x00000000), (0.0, -0.0, 0x00000000), (-0.0, -0.0, 0x00000000),   # sqrt(+0) = +0
    (1.0, 0.0, 0x3F800000), (0.0, -1.0, 0x3F800000), (3.0, 4.0, 0x40A00000),
    (1e30, 1e30, 0x718ECC90),            # the plain formula overflows here
    (-1e30, 1e-30, 0x7149F2CA),          # the small part is scaled away: |-1e30|
    (1e-30, 1e-30, 0x0DE57822),          # the plain formula underflows to 0 here
    (1e-30, 0.0, 0x00000000),            # exponent 0 = 0 > exponent 1e-30, so k = 0 and the square underflows: the reference's +0
    (FLT_MAX, 0.0, 0x7F7FFFFF), (FLT_MAX, 1.0, 0x7F7FFFFF), (FLT_MAX, FLT_MAX, PINF),
    (2.0 ** -149, 0.0, 0x00000000),      # as (1e-30, 0)
    (2.0 ** -149, 2.0 ** -149, 0x00000001),           # sqrt(2) denormals round to one
    (3 * 2.0 ** -149, 4 * 2.0 ** -149, 0x00000005),
    (2.0 ** -126, 2.0 ** -126, 0x00B504F3), (2.0 ** -127, 2.0 ** -140, 0x00400000), (2.0 ** 64, 2.0 ** 64, 0x5FB504F3),
    # non-finite input is in contract: a NaN part gives NaN, otherwise an infinite part gives +Inf
    (INF, 0.0, PINF), (0.0, -INF, PINF), (INF, INF, PINF), (NAN, 0.0, QNAN), (0.0, NAN, QNAN), (NAN, INF, QNAN), (INF, NAN, QNAN),
]
N_NONFINITE = 7
N_STREAM = 1 << 16


def cplx(re, im):
    z = np.empty(np.shape(re), np.complex64)
    z.real, z.imag = re, im
    return z


def directed():
    a = np.array([(re, im) for re, im, _ in DIRECTED], np.float32)
    return cplx(a[:, 0], a[:, 1])


def normal(n=N_STREAM, seed=2024):
    """Ordinary data: both parts standard normal."""
    x = np.random.default_rng(seed).standard_normal((n, 2)).astype(np.float32)
    return cplx(x[:, 0], x[:, 1])


def wide(n=N_STREAM, seed=2025):
    """Parts +-2^[-140, 120] * [1, 2), the two exponents independent: subnormal parts, squares that under- and overflow."""
    rng = np.random.default_rng(seed)
    e = rng.integers(-140, 121, (n, 2))
    m = rng.uniform(1.0, 2.0, (n, 2))
    s = rng.choice([-1.0, 1.0], (n, 2))
    w = (s * np.ldexp(m, e)).astype(np.float32)
    return cplx(w[:, 0], w[:, 1])


_cache = {}


def inputs():
    """{name: complex64 stream}, computed once and shared: do not write to them."""
    if not _cache:
        _cache.update(directed=directed(), normal=normal(), wide=wide())
        for v in _cache.values():
            v.setflags(write=False)
    return _cache


def mixed(n, seed=0):
    """n samples for a device run: the directed list first (as far as it fits), then the normal and the wide stream alternating in
    runs of 5 samples from an offset of `seed` runs, so that every length, row and alignment case sees all three kinds."""
    i = inputs()
    out = np.empty(n, np.complex64)
    d = min(n, len(DIRECTED))
    out[:d] = i["directed"][:d]
    k = np.arange(n - d) + 5 * seed
    pick = (k // 5) % 2 == 0
    idx = k % N_STREAM
    out[d:] = np.where(pick, i["normal"][idx], i["wide"][idx])
    return out


def expected(z):
    """agc_model.magnitude of every sample of a complex64 array (any shape) -> float32."""
    z = np.asarray(z, np.complex64)
    with np.errstate(all="ignore"):
        return agc_model.magnitude(np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag))


def same(got, exp):
    """Bit for bit, NaN by position (a NaN's payload is unspecified) -> bool array."""
    got, exp = np.asarray(got, np.float32), np.asarray(exp, np.float32)
    return (got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))


def assert_same(got, exp, what):
    got, exp = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(exp, np.float32).ravel()
    assert got.shape == exp.shape, f"{what}: {got.size} floats, expected {exp.size}"
    bad = np.nonzero(~same(got, exp))[0]
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size}/{got.size} floats differ; first at {i}: {got[i]!r} ({got.view(np.uint32)[i]:#x}) vs "
                             f"{exp[i]!r} ({exp.view(np.uint32)[i]:#x})")
