"""One table of dcBlocker and agc cases for the CPU check (tests/test_iir_cases.py) and the GPU runs (tests/test_gpu_iir.py),
and a model of the scheme both operators run on the device (kernels_iir.hip, kernels_agc.hip): speculate per chunk, repair in
three parallel rounds, settle with a one-lane walk.

A case is an operator, a stream, a starting state, run_in, n (at most 2^16: the chunk floor is 256 samples, so that gives up to
256 chunks, and the walk is one lane -- larger sizes buy nothing) and what the case is there to reach.

The scheme model (scheme) takes the plan (chunks, C, W) the library reports (sdrhip_debug_dc_plan / sdrhip_debug_agc_plan) and
runs the SEQUENTIAL model -- the oracle's dcBlocker, agc_model.agc with the lanes as batch rows -- once per chunk from the
speculative start: state 0 for dcBlocker, the call's state for agc, W samples early.  It reports which chunks start from a state
that differs bitwise from the truth, the runs of such chunks and where each lane's trajectory meets the true one, and then plays
the three repair rounds and the walk on those states, which says what the statistics words of a launch must show.

NaN: two NaN states count as equal here (x86 and the GPU differ in a NaN's sign); a case where that happens at a chunk start
is flagged (nan_starts), and only the lower bounds on the statistics are asserted for it."""
import dataclasses
import functools

import numpy as np

import agc_model

ROUNDS = 3                      # DC_REPAIR_ROUNDS, AGC_REPAIR_ROUNDS
DC_STATE = (0.25, -0.5)         # (last_sample, last_output) of the dcBlocker cases, as in tests/test_dc_blocker.py


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    op: str                     # "dc" | "agc"
    stream: tuple               # (builder name, arguments...): see stream()
    n: int
    run_in: int                 # 0 = the default
    reach: str                  # what the case is there to reach
    state: tuple = DC_STATE     # dc: (last_sample, last_output); agc: (state,)
    mu: float = 0.0             # agc
    reference: float = 1.0      # agc
    nonfinite: bool = False     # the expected output holds Inf or NaN
    bitwise: bool = True        # False: the expected output holds NaN, positions are compared (value_classes.assert_same_classes)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Elementwise: the same float32 bits, or both NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return (_bits(a) == _bits(b)).reshape(a.shape) | (np.isnan(a) & np.isnan(b))


# ---- dcBlocker streams ----------------------------------------------------------------------------------------------------------
def dc_step(x, xp, y):
    """filter.c:152-161 on Python scalars: the f32 difference, then multiply and add in double (CPython does not contract), one
    rounding to f32."""
    d = np.float32(np.float32(x) - np.float32(xp))
    with np.errstate(over="ignore", invalid="ignore"):
        return np.float32(float(d) + 0.997 * float(y))


def cancellation(n, seed, state=DC_STATE):
    """Every second sample is x[i] = (float)(x[i-1] - 0.997 * y[i-1]): the step's two terms then cancel down to a sum of about
    2^-24 of either, where a fused multiply-add (one rounding instead of two) shows in the f32 result.  The samples between are
    uniform in (-1, 1), which kicks the state back to order 1.  Returns (x, y): y is the generator's own dcBlocker output."""
    rng = np.random.default_rng(seed)
    kicks = rng.uniform(-1, 1, n).astype(np.float32)
    x, y = np.empty(n, np.float32), np.empty(n, np.float32)
    xp, yp = np.float32(state[0]), np.float32(state[1])
    for i in range(n):
        xi = kicks[i] if i % 2 == 0 else np.float32(float(xp) - 0.997 * float(yp))
        yp = dc_step(xi, xp, yp)
        x[i], y[i], xp = xi, yp, xi
    return x, y


def _uniform(n, seed):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(np.float32)


POISON_AT = 24_001              # of the value-class streams: 60 % of the 40 000 outputs come before it
HOLD = 400                      # samples the cast-overflow stream rests at -3.3e38 before it jumps


def poisoned(n, seed, kind, at=POISON_AT):
    """Uniform samples with one value-class event at sample `at`.
       inf / ninf    one +-Inf sample: the difference is +-Inf, the next one -+Inf, the state NaN from at + 1 on
       nan           one NaN sample
       inf_inf       two +Inf samples: Inf - Inf
       diff_overflow 3e38 then -3e38: the f32 difference overflows to -Inf and the state stays -Inf: no NaN ever
       cast_overflow HOLD samples at -3.3e38, an ordinary one, then 3.3e38: both differences are finite and it is the f64 sum's
                     rounding to f32 that overflows; the state stays +Inf: no NaN ever
       subnormal     3000 subnormal samples (bit patterns 1 .. 0x7fffff, both signs) from `at` on: finite throughout"""
    x = _uniform(n, seed)
    rng = np.random.default_rng(seed + 1)
    if kind == "inf":
        x[at] = np.inf
    elif kind == "ninf":
        x[at] = -np.inf
    elif kind == "nan":
        x[at] = np.nan
    elif kind == "inf_inf":
        x[at:at + 2] = np.inf
    elif kind == "diff_overflow":
        x[at], x[at + 1] = 3.0e38, -3.0e38
    elif kind == "cast_overflow":
        x[at - HOLD:at] = -3.3e38
        x[at + 1] = 3.3e38
    elif kind == "subnormal":
        u = rng.integers(1, 0x800000, 3000, dtype=np.uint32) | (rng.integers(0, 2, 3000, dtype=np.uint32) << 31)
        x[at:at + 3000] = u.view(np.float32)
    else:
        raise ValueError(kind)
    return x


def fixed_point(n, noise_from=None, seed=0):
    """A constant input (equal to last_sample, so every difference is +0): the state is multiplied by 0.997 and rounded, decays
    from -0.5 into the subnormals and sticks at 166 units of 2^-149 (0.997 * 166 = 165.502 rounds back to 166).  A lane started
    from 0 stays at 0: the two never merge.  From noise_from on the samples are uniform: the first of them absorbs the
    difference and every trajectory is the true one from there."""
    x = np.full(n, 0.75, np.float32)
    if noise_from is not None:
        x[noise_from:] = _uniform(n - noise_from, seed)
    return x


# ---- agc streams ----------------------------------------------------------------------------------------------------------------
def _noise(n, seed, level=0.3):
    rng = np.random.default_rng(seed)
    return (level * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


RANGE_MU, RANGE_REF = 2.0 ** -101, 2.0 ** 90


def agc_range(n, seed):
    """|x| spread over 2^60 .. 2^100 (log-uniform) with mu = 2^-101: mu * |x| <= 1/2, so the state stays positive and finite.
    Wherever |x * state| > 2^64 a square overflows f32 and only the scaled magnitude is right.  Every 16th sample has a real part
    near 2^-140, every 64th both parts: their corrected parts are subnormal and frexpf has to normalise them."""
    rng = np.random.default_rng(seed)
    mag = np.ldexp(rng.uniform(1.0, 2.0, n), rng.integers(60, 100, n))
    ph = rng.uniform(0, 2 * np.pi, n)
    re, im = (mag * np.cos(ph)).astype(np.float32), (mag * np.sin(ph)).astype(np.float32)
    tiny = np.ldexp(rng.uniform(1.0, 2.0, n), -140).astype(np.float32) * rng.choice(np.array([-1, 1], np.float32), n)
    re[5::16] = tiny[5::16]
    im[37::64] = -tiny[37::64]
    return (re + 1j * im).astype(np.complex64)


SUB_MU, SUB_REF = 0.4 * 2.0 ** 127, 2.0 ** -130


def agc_subnormal_parts(n, seed):
    """Noise at level 0.3 * 2^-130 against a reference of 2^-130 and mu = 0.4 * 2^127: the state is of order 1, every corrected part
    is subnormal, and the magnitude -- exponents from frexpf of a subnormal, squares of the parts scaled up to order 1 -- decides
    the state.  (Squared where they stand, both parts underflow to 0.)"""
    return (_noise(n, seed).astype(np.complex128) * 2.0 ** -130).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _stream(key):
    kind, args = key[0], key[1:]
    if kind == "cancellation":
        return cancellation(*args)[0]
    if kind == "uniform":
        return _uniform(*args)
    if kind == "poisoned":
        return poisoned(*args)
    if kind == "fixed_point":
        return fixed_point(*args)
    if kind == "noise":
        return _noise(*args)
    if kind == "agc_range":
        return agc_range(*args)
    if kind == "agc_subnormal":
        return agc_subnormal_parts(*args)
    raise ValueError(kind)


def stream(case):
    """The case's input: float32 (n,) for dcBlocker, complex64 (n,) for agc.  Read-only, shared."""
    x = _stream(case.stream)[:case.n]
    assert x.size == case.n
    x.setflags(write=False)
    return x


# ---- the table ------------------------------------------------------------------------------------------------------------------
FIXED_POINT = float(np.array([166], np.uint32).view(np.float32)[0])        # 166 * 2^-149
N_CANCEL = 50_003
CANCEL = ("cancellation", N_CANCEL, 11)
UNIFORM = ("uniform", N_CANCEL, 12)
FIXED = ("fixed_point", N_CANCEL)


def _dc(name, strm, n, run_in, reach, **kw):
    return Case("dc/" + name, "dc", strm, n, run_in, reach, **kw)


def _agc(name, strm, n, run_in, reach, mu=0.4, reference=1.0, state=1.0):
    return Case("agc/" + name, "agc", strm, n, run_in, reach, state=(state,), mu=mu, reference=reference)


def _poison(kind, reach, bitwise):
    return _dc(kind, ("poisoned", 40_000, 20 + len(kind), kind), 40_000, 8192, reach, nonfinite=kind != "subnormal", bitwise=bitwise)


NOISE = ("noise", 8195, 31)
CASES = [
    # dcBlocker: the cancellation stream (a fused multiply-add shows on it) and a uniform one on the default plan and short run-ins
    _dc("cancel-default", CANCEL, N_CANCEL, 0, "cancellation stream, default run-in: nothing starts wrong; last chunk 83 = 20 * 4 + 3"),
    _dc("cancel-w64", CANCEL, 20_002, 64, "cancellation stream, run-in 64: lanes from 0 are an ulp off at some chunk starts; last chunk 34"),
    _dc("cancel-w8", CANCEL, 20_002, 8, "cancellation stream, run-in 8"),
    _dc("cancel-w24", CANCEL, 20_002, 24, "cancellation stream, run-in 24"),
    _dc("uniform-default", UNIFORM, 50_001, 0, "ordinary signal, default run-in: nothing starts wrong; last chunk 81 = 20 * 4 + 1"),
    _dc("uniform-w64", UNIFORM, 20_001, 64, "ordinary signal, run-in far too short: every lane starts wrong and stays wrong"),
    # value classes: the event at sample 24 001 of 40 000, run-in 8192 so that the finite part's chunks start right
    _poison("inf", "+Inf sample: NaN from the next sample to the end", False),
    _poison("ninf", "-Inf sample", False),
    _poison("nan", "NaN sample", False),
    _poison("inf_inf", "Inf - Inf", False),
    _poison("diff_overflow", "x[i] - x[i-1] overflows: sticky -Inf, no NaN, bit for bit", True),
    _poison("cast_overflow", "the f64 -> f32 rounding overflows: sticky +Inf, no NaN, bit for bit", True),
    _poison("subnormal", "subnormal samples: subnormal differences onto a normal state", True),
    _dc("fixed-point", FIXED, 40_003, 64, "sticks at 166 subnormal units, lanes from 0 stay 0: the walk runs to the last sample",
        state=(0.75, -0.5)),
    _dc("fixed-then-noise", ("fixed_point", 2051, 6 * 256 + 100, 5), 2051, 64,
        "starts on the fixed point; lanes from 0 never merge until noise begins inside chunk 6: the walk meets the stored trajectory there",
        state=(0.75, FIXED_POINT)),
    # plan edges: the route change at 2 W, short last chunks, run-ins that get rounded, a run-in the block does not cover
    _dc("n=2W-1", CANCEL, 127, 64, "one short of two run-ins: sequential"),
    _dc("n=2W", CANCEL, 128, 64, "two run-ins: one chunk"),
    _dc("n=2W+1", CANCEL, 129, 64, "one past"),
    _dc("n=2W,W=1024", UNIFORM, 2048, 1024, "two run-ins, eight chunks, four of them exact"),
    _dc("n=2W-1,W=1024", UNIFORM, 2047, 1024, "one short of it: sequential"),
    _dc("run_in=61", CANCEL, 2050, 61, "run-in rounded up to 64; last chunk of 2"),
    _dc("run_in=5", CANCEL, 1025, 5, "run-in rounded up to 8; last chunk of 1"),
    _dc("run_in=1000>n", CANCEL, 100, 1000, "a run-in longer than the block: sequential"),
    # agc
    _agc("noise-default", NOISE, 8195, 0, "noise, default run-in (328 at mu = 0.4): nothing starts wrong; last chunk 323 = 40 * 8 + 3"),
    _agc("noise-w512", NOISE, 8195, 512, "noise, an ample run-in: nothing starts wrong"),
    _agc("noise-w64", NOISE, 8194, 64, "noise, run-in 64; last chunk of 2"),
    _agc("noise-w24", NOISE, 8193, 24, "noise, run-in 24: some lanes have not merged; last chunk of 1"),
    _agc("noise-w8", NOISE, 8193, 8, "noise, run-in 8: most lanes have not merged"),
    _agc("slow", ("noise", 4097, 32), 4097, 8, "mu = 0.001 from state 5: no lane merges, the walk crosses every boundary", mu=0.001, state=5.0),
    _agc("range-w64", ("agc_range", 8194, 33), 8194, 64, "|x| in 2^60 .. 2^100, mu = 2^-101: squares overflow, parts subnormal",
         mu=RANGE_MU, reference=RANGE_REF),
    _agc("range-w2048", ("agc_range", 8194, 33), 8194, 2048, "the same on a long run-in", mu=RANGE_MU, reference=RANGE_REF),
    _agc("subnormal-parts", ("agc_subnormal", 8192, 34), 8192, 64, "every corrected part subnormal: frexpf must normalise",
         mu=SUB_MU, reference=SUB_REF),
    _agc("n=2W-1", NOISE, 127, 64, "one short of two run-ins: sequential"),
    _agc("n=2W", NOISE, 128, 64, "two run-ins: one chunk"),
    _agc("n=2W+1", NOISE, 129, 64, "one past"),
    _agc("run_in=61", NOISE, 2051, 61, "run-in rounded up to 64; last chunk of 3"),
    _agc("run_in=12", NOISE, 1029, 12, "run-in rounded up to 16; last chunk of 5"),
    _agc("run_in=1000>n", NOISE, 100, 1000, "a run-in longer than the block: sequential"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES) and all(c.n <= 1 << 16 for c in CASES)


# ---- the sequential models, as the scheme model needs them --------------------------------------------------------------------------
class _Dc:
    """states[i] = the state (last_output) before sample i; the output of sample i is states[i + 1]."""
    guess = np.float32(0.0)

    def __init__(self, case, oracle):
        self.x, self.oracle, self.ls = stream(case), oracle, case.state[0]
        self.out, fs, fo = oracle.dc_blocker(self.x, case.state[0], case.state[1])
        self.final = np.array([fs, fo], np.float32)
        self.states = np.concatenate([np.array([case.state[1]], np.float32), self.out])

    def walk(self, segs):
        """[(first sample, end, state before the first sample)] -> per segment, the state after each of its samples."""
        return [self.oracle.dc_blocker(self.x[a:b], float(self.x[a - 1]) if a else self.ls, float(s))[0] for a, b, s in segs]


class _Agc:
    def __init__(self, case, oracle=None):
        self.x, self.mu, self.ref = stream(case), case.mu, case.reference
        n = case.n
        self.out, fin, snaps = agc_model.agc(self.x, case.mu, case.reference, case.state[0], states_at=range(n + 1))
        self.states = np.array([np.ravel(snaps[k])[0] for k in range(n + 1)], np.float32)
        self.final = self.states[n:]
        self.guess = np.float32(case.state[0])

    def walk(self, segs):
        if not segs:
            return []
        L = max(b - a for a, b, _ in segs)
        rows = np.zeros((len(segs), L), np.complex64)          # zero padding: outputs past a row's end are ignored
        for r, (a, b, _) in enumerate(segs):
            rows[r, :b - a] = self.x[a:b]
        _, _, snaps = agc_model.agc(rows, self.mu, self.ref, np.array([s for _, _, s in segs], np.float32), states_at=range(1, L + 1))
        S = np.stack([snaps[k] for k in range(1, L + 1)])
        return [S[:b - a, r].copy() for r, (a, b, _) in enumerate(segs)]


@dataclasses.dataclass
class Scheme:
    chunks: int
    C: int
    W: int
    out: np.ndarray             # the expected output (dc: float32, agc: complex64)
    final: np.ndarray           # the expected final state (dc: 2 floats, agc: 1)
    wrong: np.ndarray           # per chunk: its lane reaches the chunk start in a state that is not the true one
    nan_starts: bool            # some lane and the truth are both NaN at a chunk start
    runs: list                  # [(first chunk, last chunk, [per chunk: the first sample whose state is the true one again, or None])]
    repaired: int               # chunks the three rounds recompute           (stats[2])
    left: int                   # chunks the settle pass still finds inconsistent (stats[0])
    rewritten: int              # samples the walk rewrites                   (stats[1]; a lower bound where NaN meets NaN)
    walks: list                 # [(first sample, end)] of the walk's stretches; end = where it met the stored trajectory, or n

    @property
    def n_wrong(self):
        return int(self.wrong.sum())

    @property
    def longest_run(self):
        return max((b - a + 1 for a, b, _ in self.runs), default=0)

    def never_merging_run(self, least):
        """A run of at least `least` wrong-start chunks each of which is still wrong at its end."""
        return any(b - a + 1 >= least and all(m is None for m in ms) for a, b, ms in self.runs)

    def describe(self):
        runs = "; ".join(f"chunks {a}-{b} merge at {['-' if m is None else m for m in ms]}" for a, b, ms in self.runs[:4])
        return (f"chunks {self.chunks} (C {self.C}, W {self.W}): {self.n_wrong} start wrong, longest run {self.longest_run}"
                f"{' [' + runs + (' ...' if len(self.runs) > 4 else '') + ']' if self.runs else ''}; rounds recompute {self.repaired}, "
                f"left to the walk {self.left}, walk {self.walks[:3]}{' ...' if len(self.walks) > 3 else ''} rewrites {self.rewritten}")


_MODELS = {}


def model(case, oracle):
    """The sequential truth of a case, computed once."""
    if case.name not in _MODELS:
        _MODELS[case.name] = (_Dc if case.op == "dc" else _Agc)(case, oracle)
    return _MODELS[case.name]


_SCHEMES = {}


def scheme(case, plan, oracle):
    """plan: (chunks, C, W) as the library's plan hook reports it for (case.n, case.run_in)."""
    key = (case.name, tuple(plan))
    if key not in _SCHEMES:
        _SCHEMES[key] = _scheme(case, model(case, oracle), *plan)
    return _SCHEMES[key]


def _scheme(case, m, chunks, C, W):
    n, T = case.n, m.states
    if chunks == 0:
        return Scheme(0, C, W, m.out, m.final, np.zeros(0, bool), False, [], 0, 0, 0, [])
    assert chunks == -(-n // C) and n >= 2 * W
    lo = [j * C for j in range(chunks)]
    hi = [min(b + C, n) for b in lo]
    exact = [b - W <= 0 for b in lo]                          # the lane starts at sample 0 from the call's state
    stored = T[1:].copy()                                     # the state after each sample, as the lanes leave it
    s_start, s_end = T[lo].copy(), T[hi].copy()
    spec = [j for j in range(chunks) if not exact[j]]
    for j, tr in zip(spec, m.walk([(lo[j] - W, hi[j], m.guess) for j in spec])):
        s_start[j], s_end[j] = tr[W - 1], tr[-1]
        stored[lo[j]:hi[j]] = tr[W:]
    wrong = ~same(s_start, T[lo])
    nan_starts = bool((np.isnan(s_start) & np.isnan(T[lo]))[spec].any()) if spec else False
    runs, j = [], 0
    while j < chunks:
        if not wrong[j]:
            j += 1
            continue
        a = j
        while j < chunks and wrong[j]:
            j += 1
        merges = []
        for k in range(a, j):
            hit = np.nonzero(same(stored[lo[k]:hi[k]], T[lo[k] + 1:hi[k] + 1]))[0]
            merges.append(int(lo[k] + hit[0]) if hit.size else None)
        runs.append((a, j - 1, merges))
    # the repair rounds: every chunk compares its start with its predecessor's end of the round before
    repaired = 0
    for _ in range(ROUNDS):
        prev = s_end.copy()
        todo = [j for j in spec if not same(s_start[j], prev[j - 1])]
        for j, tr in zip(todo, m.walk([(lo[j], hi[j], prev[j - 1]) for j in todo])):
            stored[lo[j]:hi[j]] = tr
            s_start[j], s_end[j] = prev[j - 1], tr[-1]
        repaired += len(todo)
    bad = [(not exact[j]) and not same(s_start[j], s_end[j - 1]) for j in range(chunks)]
    left, rewritten, walks = sum(bad), 0, []
    if case.op == "dc":                                       # k_dc_settle: from a bad chunk's start until the value equals what is stored
        reach = -1
        for j in range(1, chunks):
            if not bad[j] or lo[j] <= reach:
                continue
            i = lo[j]
            assert same(stored[i - 1], T[i]), "everything before the walk is final"
            hit = np.nonzero(same(stored[i:], T[i + 1:]))[0]
            end = i + int(hit[0]) if hit.size else n
            stored[i:end] = T[i + 1:end + 1]
            rewritten += end - i
            walks.append((i, end))
            reach = end
    else:                                                     # k_agc_settle: whole chunks, on while the next chunk's start is not the end just computed
        j = 1
        while j < chunks:
            if not bad[j] or same(s_start[j], s_end[j - 1]):
                j += 1
                continue
            a = j
            assert same(s_end[j - 1], T[lo[j]]), "everything before the walk is final"
            while True:
                s_start[j], s_end[j] = T[lo[j]], T[hi[j]]
                stored[lo[j]:hi[j]] = T[lo[j] + 1:hi[j] + 1]
                rewritten += hi[j] - lo[j]
                j += 1
                if j >= chunks or same(s_start[j], s_end[j - 1]):
                    break
            walks.append((lo[a], hi[j - 1]))
    assert same(stored, T[1:]).all(), "the scheme as modelled does not end on the sequential result"
    return Scheme(chunks, C, W, m.out, m.final, wrong, nan_starts, runs, repaired, left, rewritten, walks)


def plan_of(lib, case):
    """(chunks, C, W) from the library's plan hooks: no launch, no device."""
    return lib.dc_plan(case.n, case.run_in) if case.op == "dc" else lib.agc_plan(case.n, case.mu, case.run_in)
