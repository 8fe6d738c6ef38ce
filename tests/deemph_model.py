"""The model of de-emphasis (include/sdr_hip.h "de-emphasis"; sdr_amd/csrc/kernels_deemph.hip).  TEST INFRASTRUCTURE ONLY.

    y[i] = y[i-1] + alpha * (x[i] - y[i-1])        y[-1] = state

at numpy float32: three operations per sample, one per line, each rounded to nearest -- subtract, multiply, add.  The reference has no
de-emphasis, so this file is the definition's restatement, written as agc_model.py restates agc.  Vectorised across rows: 1024 rows cost
one walk.

wg_scheme restates what the one-workgroup route does with its chunks (speculate, then rounds of verification), to give the statistics
words the kernel reports; the OUTPUT never depends on the scheme."""
import math

import numpy as np

F = np.float32


def alpha_of(tau_seconds, sample_rate):
    """sdrhip_deemph_alpha's value, as a float32."""
    return F(1.0 - math.exp(-1.0 / (tau_seconds * sample_rate)))


def default_run_in(alpha):
    """ceil(40 / alpha) rounded up to a multiple of 4: the library's default run-in."""
    w = int(math.ceil(40.0 / float(F(alpha))))
    return (w + 3) & ~3


def step(x, y, alpha):
    with np.errstate(all="ignore"):
        d = x - y
        m = alpha * d
        return y + m


def deemph(x, alpha, state=0.0):
    """x: n floats, or rows x n; state: a float, or rows floats -> (out like x, final state(s))."""
    x = np.asarray(x, F)
    alpha = F(alpha)
    one = x.ndim == 1
    rows = np.atleast_2d(x)
    y = np.broadcast_to(np.asarray(state, F), (rows.shape[0],)).astype(F).copy()
    out = np.empty_like(rows)
    for i in range(rows.shape[1]):
        y = step(rows[:, i], y, alpha)
        assert y.dtype == F
        out[:, i] = y
    return (out[0], F(y[0])) if one else (out, y)


def same_bits(a, b):
    """bit for bit, NaN by position -> bool array"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def first_nan(out):
    bad = np.nonzero(np.isnan(out))[0]
    return int(bad[0]) if bad.size else None


def meet_index(x, alpha, state_a, state_b, start=0):
    """First i >= start at which the trajectory from state_a at sample 0 and the one from state_b at sample `start` hold the same
    bits after sample i; None if they never do inside x."""
    x = np.asarray(x, F)
    a, _ = deemph(x, alpha, state_a)
    b, _ = deemph(x[start:], alpha, state_b)
    eq = np.nonzero(a[start:].view(np.uint32) == b.view(np.uint32))[0]
    return int(eq[0]) + start if eq.size else None


def wg_chunk(n):
    c = max(16, (n + 1023) // 1024)
    return (c + 3) & ~3


def _walk_chunks(x, alpha, begins, ends, y):
    """the chunks [begins[k], ends[k]) walked side by side from the states y -> (their outputs as a list, their end states)"""
    y = y.astype(F).copy()
    span = int((ends - begins).max()) if begins.size else 0
    outs = np.zeros((begins.size, span), F)
    for t in range(span):
        i = begins + t
        live = i < ends
        xi = x[np.where(live, i, 0)]
        y = np.where(live, step(xi, y, alpha), y).astype(F)
        outs[:, t] = y
    return outs, y


def wg_scheme(x, alpha, state=0.0, run_in=0):
    """One row on the WG route -> (out, final, stats).  stats = (rounds that recomputed a chunk, 0, chunks whose start state was replaced
    summed over the rounds, chunks): the kernel's four words."""
    x = np.asarray(x, F)
    alpha = F(alpha)
    n = x.size
    W = default_run_in(alpha) if run_in <= 0 else (run_in + 3) & ~3
    C = wg_chunk(n)
    nch = (n + C - 1) // C
    begins = np.arange(nch, dtype=np.int64) * C
    ends = np.minimum(begins + C, n)
    exact = begins - W <= 0
    starts = np.where(exact, 0, begins - W)
    _, y_start = _walk_chunks(x, alpha, starts, begins, np.where(exact, F(state), F(0.0)))
    outs, y_end = _walk_chunks(x, alpha, begins, ends, y_start)
    y_start, y_end = y_start.view(np.uint32).copy(), y_end.view(np.uint32).copy()
    rounds = replaced = 0
    for _ in range(nch):
        prev = np.concatenate([[0], y_end[:-1]]).astype(np.uint32)
        redo = np.nonzero(~exact & (prev != y_start))[0]
        if redo.size == 0:
            break
        o, e = _walk_chunks(x, alpha, begins[redo], ends[redo], prev[redo].view(F))
        outs[redo, :o.shape[1]] = o
        new_end = y_end.copy()
        new_end[redo] = e.view(np.uint32)
        y_start[redo] = prev[redo]
        y_end = new_end
        rounds += 1
        replaced += int(redo.size)
    out = np.concatenate([outs[j, :ends[j] - begins[j]] for j in range(nch)]) if nch else np.zeros(0, F)
    return out, y_end[-1:].view(F)[0] if nch else F(state), (rounds, 0, replaced, nch)
