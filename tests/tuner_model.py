"""numpy float32 restatement of the tuner (include/sdr_hip.h, sdrhip_tuner_*).  TEST INFRASTRUCTURE ONLY.

    x[n] = input sample n;  o[n] = osc[n mod N], n = absolute stream index
    m[n] = (x.re*o.re - x.im*o.im, x.re*o.im + x.im*o.re)      Data.Complex's (*) at Float (GHC base), every op rounded, no FMA
    y    = the complex decimator's Pipe (oracle/pipes_model.py) on m

The (*) parity is argued from base's formula; no GHC ran."""
import numpy as np

from oracle import pipes_model as PM


def mix(x_iq, osc_iq, pos0=0):
    """x_iq: interleaved float32 samples, the first one at absolute stream index pos0; osc_iq: interleaved (re, im) table."""
    x = np.ascontiguousarray(x_iq, dtype=np.float32).reshape(-1, 2)
    o = np.ascontiguousarray(osc_iq, dtype=np.float32).reshape(-1, 2)
    idx = (int(pos0) + np.arange(x.shape[0], dtype=np.int64)) % o.shape[0]
    ore, oim = o[idx, 0], o[idx, 1]
    out = np.empty_like(x)
    # numpy evaluates each elementwise float32 product and sum on its own: nothing is fused
    out[:, 0] = x[:, 0] * ore - x[:, 1] * oim
    out[:, 1] = x[:, 0] * oim + x[:, 1] * ore
    return out.reshape(-1)


def mix_by_i_shortcut(x_iq):
    """'multiply by i = swap and negate' -- what a kernel may NOT do for the (0, 1) entries of a table: (-im, re)."""
    x = np.ascontiguousarray(x_iq, dtype=np.float32).reshape(-1, 2)
    return np.stack([-x[:, 1], x[:, 0]], axis=1).reshape(-1)


def shift_table(num, den):
    """exp(2 pi i ((num n) mod den) / den), n < den, float32 pairs: the octant reduction documented in sdr_hip.h."""
    num, den = int(num), int(den)
    n = np.arange(den, dtype=np.int64)
    r = (n * (num % den)) % den
    q = (4 * r) // den
    f = 4 * r - q * den
    c = np.ones(den, np.float32)
    s = np.zeros(den, np.float32)
    diag, low, high = 2 * f == den, (f > 0) & (2 * f < den), 2 * f > den
    c[diag] = s[diag] = np.float32(np.cos(np.float64(np.pi) * 0.25))
    phi = np.float64(np.pi) * (f[low].astype(np.float64) / np.float64(2 * den))
    c[low], s[low] = np.cos(phi).astype(np.float32), np.sin(phi).astype(np.float32)
    phi = np.float64(np.pi) * ((den - f[high]).astype(np.float64) / np.float64(2 * den))
    c[high], s[high] = np.sin(phi).astype(np.float32), np.cos(phi).astype(np.float32)
    zero = np.float32(0.0)
    nc, ns = zero - c, zero - s                 # -x, and +0 for x = 0
    re = np.select([q == 0, q == 1, q == 2], [c, ns, nc], s)
    im = np.select([q == 0, q == 1, q == 2], [s, c, ns], nc)
    return np.stack([re, im], axis=1).astype(np.float32).reshape(-1)


def tuner_expected(oracle, taps, order, factor, x, osc, seam, pos0=0, block_out=512):
    """The outputs of the stream whose sample pos0 is x[0] (interleaved float32), from output pos0 / factor on: the reference's
    firDecimator fed `seam`-sample buffers of the mixed stream (seam = 0: one buffer, every output One).  pos0 is a multiple
    of factor.  Only whole output blocks of block_out are yielded; with block_out = 1 every computable output comes back."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    assert pos0 % factor == 0
    m = mix(x, osc, pos0)
    model = PM.FilterModel(oracle, taps, order, complex_=True, factor=factor)
    if seam == 0:
        n = m.size // 2
        return model.one((n - model.num_coeffs) // factor + 1, m) if n >= model.num_coeffs else np.empty(0, np.float32)
    # the buffer pos0 lies in starts lead samples earlier: those samples are unknown (zeros here) and every output that starts
    # among them is dropped -- the outputs from pos0 / factor on never read them
    lead = pos0 % seam
    assert lead % factor == 0
    m = np.concatenate([np.zeros(2 * lead, np.float32), m])
    nblk = (m.size // 2) // seam
    blocks = [m[2 * seam * i:2 * seam * (i + 1)] for i in range(nblk)]
    rest = m[2 * seam * nblk:]
    if rest.size // 2 >= model.num_coeffs:
        blocks.append(rest)                      # a shorter last buffer: its own outputs are One, those before it Cross
    out, _ = PM.fir_decimator_pipe(model, blocks, block_out)
    y = np.concatenate(out) if out else np.empty(0, np.float32)
    return y[2 * (lead // factor):]
