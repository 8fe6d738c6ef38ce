"""agc / agcPipe (hs_sources/SDR/Util.hs:325-348) restated in numpy, float32 throughout, no fused multiply-add:

    c      = x[i] * state                            (both parts: the output sample)
    state' = state + mu * (reference - magnitude c)

`magnitude` is GHC base's Data.Complex.magnitude at Float (its SPECIALISE pragma covers Double only):

    k = max (exponent re) (exponent im)              exponent 0 = 0, otherwise frexp's exponent (denormals normalised)
    m = scaleFloat k (sqrt (sqr (scaleFloat (-k) re) + sqr (scaleFloat (-k) im)))

scaleFloat is ldexpf with one rounding; zero passes through unchanged.  No GHC was available to run the reference: the
model is a restatement of published `base` code ("argued-exact", as for fmDemod).

A Python loop over samples is slow, so the model steps many independent streams together: x has shape (streams, n)."""
import numpy as np


def magnitude(re, im):
    """float32 arrays -> float32 array."""
    re = np.asarray(re, dtype=np.float32)
    im = np.asarray(im, dtype=np.float32)
    _, er = np.frexp(re)
    _, ei = np.frexp(im)
    k = np.maximum(er, ei)
    a = np.ldexp(re, -k)
    b = np.ldexp(im, -k)
    m = np.ldexp(np.sqrt(a * a + b * b), k)
    assert m.dtype == np.float32
    return m


def agc(x, mu, reference, state=1.0, states_at=None):
    """x: complex64, shape (streams, n) or (n,).  state: a scalar or one value per stream.
    Returns (out complex64 of x's shape, final state float32 of shape (streams,) -- a scalar for 1-d x); with states_at (sample
    counts) a third value, {count: the state after that many samples}, so that one run serves every shorter length."""
    x = np.asarray(x)
    one = x.ndim == 1
    x = np.ascontiguousarray(x.reshape(1, -1) if one else x, dtype=np.complex64)
    streams, n = x.shape
    mu, reference = np.float32(mu), np.float32(reference)
    s = np.array(np.broadcast_to(np.asarray(state, dtype=np.float32), (streams,)), dtype=np.float32)
    xs = np.empty((n, 2, streams), np.float32)          # sample-major: one step reads and writes contiguous rows
    xs[:, 0, :] = x.real.T
    xs[:, 1, :] = x.imag.T
    out = np.empty_like(xs)
    marks = set(int(k) for k in states_at) if states_at is not None else set()
    snaps = {0: s.copy()} if 0 in marks else {}
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(n):
            c = xs[i] * s
            out[i] = c
            s = s + mu * (reference - magnitude(c[0], c[1]))
            if i + 1 in marks:
                snaps[i + 1] = s[0] if one else s.copy()
    assert s.dtype == np.float32 and out.dtype == np.float32
    res = np.empty((streams, n), np.complex64)
    res.real = out[:, 0, :].T
    res.imag = out[:, 1, :].T
    ret = (res[0], s[0]) if one else (res, s)
    return ret + (snaps,) if states_at is not None else ret


def interleaved(z):
    """complex64 (n,) -> float32 (2n,) as the device takes it."""
    return np.ascontiguousarray(z, dtype=np.complex64).view(np.float32)
