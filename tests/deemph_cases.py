"""The cases of the de-emphasis tests (tests/test_deemph_model.py, test_deemph_abi.py on the CPU; test_gpu_deemph.py,
test_gpu_deemph_stream_order.py on the device).  TEST INFRASTRUCTURE ONLY.

Rows.  ordinary: seeded noise, a sine in noise, 0.7 plus small noise, wide noise -- inputs on which two trajectories meet.  directed:
+-0, subnormals, a run of 3.3e38 followed by -3.3e38 (x - y overflows there), an Inf and a NaN; the first NaN of the OUTPUT is stated
here, not read from the model.  constant: 2.0 for a few samples, then exactly 0.5 for ever.  silent: noise, then exactly 0.  On the last
two a trajectory that starts from 0 inside the constant part never meets the true one (alpha < 1): the slow case of every route."""
import numpy as np

import deemph_model as DM

F = np.float32
# (tau, rate): broadcast FM at the audio rate, at a wideband rate, narrow-band voice, and the European constant
ALPHA_ARGS = [(75e-6, 48000.0), (50e-6, 48000.0), (750e-6, 8000.0), (75e-6, 256000.0)]
A48, A256, ONE = DM.alpha_of(75e-6, 48000.0), DM.alpha_of(75e-6, 256000.0), F(1.0)
ALPHAS = [A48, A256, ONE]                         # the GPU tests' alphas
ALPHA_IDS = ["75us-48k", "75us-256k", "alpha-1"]
WG_MAX = 65536                                     # what the WG route fits
WG_AUTO = 32768                                    # from here on auto takes LS when it has a workspace (the measured edge)
ORDINARY_KINDS = ("noise", "sine", "offset", "wide")

STEP_LEN = 37                                      # constant row: samples of 2.0 in front of the 0.5s
NOISE_LEN = 300                                    # silent row: samples of noise in front of the zeros
# directed row: where the pieces sit (all inside the first 2100 samples; a shorter row is a prefix)
BIG_AT, BIG_LEN, INF_AT, NAN_AT = 600, 400, 1500, 2000
SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-42, -3e-39, 1.1754942e-38, -1.1754944e-38, 1.0, -1.0, 0.0, -0.0, 5e-41, 0.5, -0.0, 0.0], F)


def ordinary(kind, n, seed):
    rng = np.random.default_rng(9100 + seed)
    t = np.arange(n)
    if kind == "noise":
        return rng.normal(0, 0.3, n).astype(F)
    if kind == "sine":
        return (0.6 * np.sin(2 * np.pi * 0.013 * t) + rng.normal(0, 0.05, n)).astype(F)
    if kind == "offset":
        return (0.7 + rng.normal(0, 1e-3, n)).astype(F)
    return rng.normal(0, 30.0, n).astype(F)


def ordinary_rows(rows, n, seed=0):
    """rows x n: the four kinds in turn, every row its own seed"""
    return np.stack([ordinary(ORDINARY_KINDS[r % 4], n, seed * 1000 + r) for r in range(rows)]) if rows else np.zeros((0, n), F)


def directed(n, variant="overflow", seed=0):
    """-> (row of n floats, index of the output's first NaN or None).  overflow: the whole row.  inf / nan: the row without the run of
    3.3e38, so that the Inf (the NaN) is the first thing that goes wrong.
    Why the index: from a finite state an Inf sample gives x - y = Inf, y = Inf, and the next finite sample Inf - Inf = NaN (one step
    later); after the run of 3.3e38 the state is near 3.3e38 for every alpha of the cases (0.95^400 < 1e-9), so -3.3e38 - y overflows to
    -Inf, y = -Inf, and the next sample gives NaN; a NaN sample gives NaN at once."""
    full = max(n, NAN_AT + 100)
    x = np.random.default_rng(9300 + seed).normal(0, 0.3, full).astype(F)
    x[:SPECIALS.size] = SPECIALS
    x[INF_AT] = np.inf
    x[NAN_AT] = np.nan
    if variant == "overflow":
        x[BIG_AT:BIG_AT + BIG_LEN] = F(3.3e38)
        x[BIG_AT + BIG_LEN] = F(-3.3e38)
        at = BIG_AT + BIG_LEN + 1
    elif variant == "inf":
        at = INF_AT + 1
    else:
        x[INF_AT] = F(0.25)
        at = NAN_AT
    return x[:n].copy(), (at if at < n else None)


def constant(n):
    x = np.full(n, 0.5, F)
    x[:min(STEP_LEN, n)] = 2.0
    return x


def silent(n, seed=0):
    x = np.zeros(n, F)
    k = min(NOISE_LEN, n)
    x[:k] = np.random.default_rng(9400 + seed).normal(0, 0.3, k).astype(F)
    return x


def lengths(alpha):
    """the n of the model comparison: the plan's edges for this alpha among them"""
    W = DM.default_run_in(alpha)
    return [0, 1, 7, 2 * W - 1, 2 * W, 2 * W + 1, 4096, 4097, WG_AUTO - 1, WG_AUTO, WG_MAX, WG_MAX + 1]
