"""The tables behind tests/test_gpu_rows_limits.py and tests/test_gpu_fir_rows_classes.py: the row forms at SDRHIP_ROWS_MAX = 1024
rows, at the lane cap of the agc / dcBlocker rows plan, and (the FIR rows) on the float32 value classes.  No pytest and no device
in here: tests/test_rows_limit_cases.py shows on the CPU, from the plan hooks and the models alone, what the tables reach.

A. agc / dcBlocker.  The rows plan is the one-row plan until rows * chunks passes 32768 lanes; from there the chunk grows (to a
multiple of 8 samples), the boundaries move, the last chunk shrinks to a few samples and the per-row statistics are no longer the
one-row call's.  The minimum chunk is 256 samples, so the smallest shapes that reach the cap are 1024 rows of 8192 samples (exactly
at it) and of 8193 (past it).  IIR_SHAPES states the plans as worked out by hand; the tests assert them through the hooks first.

The rows follow the recipe of test_gpu_rows._many (a seed, a level and a starting state per row; every eighth agc row silent, the
levels down to 0.01), with one addition: uniform dcBlocker rows started from zero W samples early never meet the stored trajectory
(the difference decays by 0.997 a sample: about 5000 samples to the last bit, a chunk is 264), so every 64th row from row 2 on is
iir_cases.fixed_point -- constant until three quarters of the row, lanes from 0 sit on 0 and the truth on 166 subnormal units, then
noise, which absorbs the difference at once: the settling walk meets the stored trajectory there, and starts again at the next
chunk the rounds did not reach.

B, C. The FIR rows: see FIR_1024 and CLASS_FAMILIES below."""
import dataclasses
import functools

import numpy as np

import agc_model
import fir_rows_cases as RC
import iir_cases as IC
import value_classes as VC

# ---- A: agc and dcBlocker rows at the lane cap ----------------------------------------------------------------------------------
RUN_IN, MU, REFERENCE = 64, 0.4, 1.0
LANE_CAP = 32768                # kAgcMaxLanes, kDcMaxLanes
AGC_LEVELS = (0.3, 0.05, 0.6, 0.01, 0.2, 0.1, 0.4, 0.0)


@dataclasses.dataclass(frozen=True)
class IirShape:
    rows: int
    n: int
    one_row: tuple              # (chunks, C, W) of the one-row plan, by hand
    plan: tuple                 # ... of the rows plan
    what: str

    @property
    def name(self):
        return f"{self.rows} rows x {self.n}"

    @property
    def grown(self):
        return self.plan != self.one_row

    @property
    def subset(self):
        """The checked rows: the first and the last, rows either side of a wave boundary of the packed lanes (32 chunks a row: two rows
        a wave; 63 chunks: lane 4032 = 63 * 64 opens row 64), one row of every agc level (rows 0 .. 7; row 7 silent) and the directed
        dcBlocker rows 2 and 66."""
        last = self.rows - 1
        return tuple(sorted({0, 1, 2, 3, 4, 5, 6, 7, 63, 64, 66, last // 2, last // 2 + 1, last - 1, last}))


IIR_SHAPES = [
    IirShape(1024, 8192, (32, 256, 64), (32, 256, 64), "exactly 32768 lanes: at the cap, not grown"),
    IirShape(1024, 8193, (33, 256, 64), (32, 264, 64), "grown; the last chunk is 9 samples"),
    IirShape(513, 16385, (65, 256, 64), (63, 264, 64), "grown; 32319 lanes; rows and chunks odd: every row boundary inside a wave"),
    IirShape(1024, 100, (0, 256, 64), (0, 256, 64), "the sequential walk, 1024 workgroups"),
]


def fixed_row(r):
    """dcBlocker: the directed rows (module docstring)."""
    return r % 64 == 2


@functools.lru_cache(maxsize=4)
def many(op, rows, n):
    """rows streams of n samples and their starting states: test_gpu_rows._many's recipe (the GPU tests assert that it is), and
    for dcBlocker the directed rows.  Read-only, shared."""
    if op == "dc":
        xs = [np.random.default_rng(500 + r).uniform(-1, 1, n).astype(np.float32) * np.float32(1 + r % 5) for r in range(rows)]
        states = [(0.01 * r - 0.3, 0.5 - 0.02 * r) for r in range(rows)]
        for r in range(rows):
            if fixed_row(r):
                xs[r] = IC.fixed_point(n, 3 * n // 4 + (r % 61 if n >= 1000 else 0), 500 + r)
                states[r] = (0.75, IC.FIXED_POINT)
    else:
        xs = [IC._noise(n, 600 + r, AGC_LEVELS[r % 8]) for r in range(rows)]
        states = [(1.0 + 0.03 * r,) for r in range(rows)]
    for x in xs:
        x.setflags(write=False)
    return xs, states


@dataclasses.dataclass
class Truth:
    outs: list                  # per row: the expected output as float32
    finals: np.ndarray          # [rows, 1 (agc) or 2 (dc)]
    states: object              # agc: [n + 1, rows], the state before each sample and after the last; dc: None (the output is it)


@functools.lru_cache(maxsize=4)
def _agc_truth(rows, n):
    xs, states = many("agc", rows, n)
    out, fin, snaps = agc_model.agc(np.stack(xs), MU, REFERENCE, np.array([s[0] for s in states], np.float32), states_at=range(n + 1))
    return Truth([np.ascontiguousarray(out[r]).view(np.float32) for r in range(rows)], fin.reshape(rows, 1).copy(),
                 np.stack([snaps[k] for k in range(n + 1)]))


_dc_truths = {}


def truth(op, shape, oracle):
    """The sequential models on every row, computed once: agc_model.agc vectorised over the rows, the oracle's dc_blocker per row."""
    if op == "agc":
        return _agc_truth(shape.rows, shape.n)
    key = (shape.rows, shape.n)
    if key not in _dc_truths:
        xs, states = many("dc", shape.rows, shape.n)
        res = [oracle.dc_blocker(x, *st) for x, st in zip(xs, states)]
        _dc_truths[key] = Truth([t[0] for t in res], np.array([t[1:] for t in res], np.float32), None)
    return _dc_truths[key]


class _AgcRow(IC._Agc):
    """iir_cases._Agc on a row of the vectorised truth (its state trajectory is already there)."""

    def __init__(self, x, state, out, states):
        self.x, self.mu, self.ref = x, MU, REFERENCE
        self.out, self.states, self.final, self.guess = out.view(np.complex64), states, states[-1:], np.float32(state[0])


class _DcRow(IC._Dc):
    def __init__(self, x, state, out, final, oracle):
        self.x, self.oracle, self.ls = x, oracle, state[0]
        self.out, self.final = out, final
        self.states = np.concatenate([np.array([state[1]], np.float32), out])


_schemes = {}


def row_scheme(op, shape, r, plan, oracle):
    """iir_cases' scheme model of row r under `plan` (chunks, C, W)."""
    key = (op, shape.rows, shape.n, r, tuple(plan))
    if key not in _schemes:
        xs, states = many(op, shape.rows, shape.n)
        t = truth(op, shape, oracle)
        if op == "agc":
            m = _AgcRow(xs[r], states[r], t.outs[r], np.ascontiguousarray(t.states[:, r]))
        else:
            m = _DcRow(xs[r], states[r], t.outs[r], t.finals[r], oracle)
        case = IC.Case(f"rows-limit/{op}/{shape.name}/{r}", op, ("rows-limit", op, shape.rows, shape.n, r), shape.n, RUN_IN, shape.what,
                       state=tuple(states[r]), mu=MU, reference=REFERENCE)
        _schemes[key] = IC._scheme(case, m, *plan)
    return _schemes[key]


def stats_of(s):
    """The four statistics words a launch must show for a row with this scheme."""
    return (s.left, s.rewritten, s.repaired, s.chunks)


def plans(lib, op, shape):
    """(rows plan, one-row plan) from the library's hooks: host arithmetic, no device."""
    if op == "dc":
        return lib.dc_rows_plan(shape.rows, shape.n, RUN_IN), lib.dc_plan(shape.n, RUN_IN)
    return lib.agc_rows_plan(shape.rows, shape.n, MU, RUN_IN), lib.agc_plan(shape.n, MU, RUN_IN)


FM_ROWS, FM_N = 1024, 1027

# ---- B: the FIR rows on the banked route with 1024 rows ---------------------------------------------------------------------------
# one family per kernel kind: the complex decimator, the chain's real resampler, the real symmetric filter
FIR_1024 = ("cdec AVX /4, 64 taps", "rres 3/10 AVX, the chain's taps", "rfilt sym SSE, the chain's audio taps")
FIR_PIPE_ROWS = (0, 1, 511, 1022, 1023)


def fir_1024_cases(f):
    """"tile + 1" outputs a row (two tiles: a full one and one output) with three seams inside the range, and "lane group - 1"
    outputs without a seam (1024 workgroups of mostly idle lanes, no fix-up launch)."""
    return [RC.Case(f, 1024, "tile + 1", "three", "zero", 1, f.out_blocks[0]), RC.Case(f, 1024, "lane group - 1", "none", "zero", 2, f.out_blocks[-1])]


def _seed(case, row, base):
    f = BASE_FAMILY.get(case.family.name, case.family)
    return base + 4096 * (RC.FAMILIES.index(f) * 8 + (RC.SIZES + ("short",)).index(case.size)) + 2048 * (case.seam_kind == "none") + row


def fir_row_stream(case, g, row, base=9000):
    """fir_rows_cases.row_stream for a case outside its table: the near stream of one row from element 0 to the end of its guaranteed
    range, seeded by the family, the size, the seam choice and the row."""
    f = case.family
    n = g.in_base + RC.need_inputs(f, g)
    x = RC.S.cfloat_block(n, seed=_seed(case, row, base)) if f.complex_ else RC.S.real_block(n, seed=_seed(case, row, base))
    x.setflags(write=False)
    return x


# ---- C: the FIR rows on value classes ---------------------------------------------------------------------------------------------
# Every banked family at two row lengths, each with seams and without, four rows a call:
#   short   the longest row the rows plan still gives U = 1 on a tile below plan_tile's (k_split_rows<..., U = 1, false> and a capped
#           NN exist in the row form only).  The longest, because a row this short holds few windows: a real filter's is 63 outputs,
#           and every segment and seam more that fits helps.  "rfilt AVX, 77 taps" (padded window 80, seam block at least 80) spans
#           142 inputs there, which cannot hold three seams (that takes more than 160): it runs with the two that fit.
#   long    "3 tiles - 1" outputs: plan_tile's tile and U, reached through k_split_rows.
# Row 0 is the unsalted stream.  Rows 1 .. 3 are slices of streams salted by value_classes.salt (lp = the family's window in input
# samples), cut so that a chosen segment lands on a chosen sample of the row: row 1 a sub_in_zero run (zeros, three
# subnormals in the middle) from a window's start on, its middle within a step of the first seam, row 2 an inf_re island and row 3 a nan island on the sample class_island() picks
# beside that seam.  A short row is a few windows long and cannot hold every class: the classes are spread over the rows.
AWKWARD = ("rfilt AVX, 77 taps", "cdec AVX /4, 64 taps")             # one real, one complex family also with level-1 taps
BASE_FAMILY = {}                # a derived family (awkward taps) -> the family of fir_rows_cases it was made from
TWO_SEAMS_ONLY = ("rfilt AVX, 77 taps", "rfilt AVX, 77 taps, level-1 taps")
CLASS_ROWS = 4


def _awkward(f):
    a = dataclasses.replace(f, name=f.name + ", level-1 taps", taps=lambda: VC.awkward_taps(f.taps(), 1))
    BASE_FAMILY[a.name] = f
    return a


CLASS_FAMILIES = [f for f in RC.FAMILIES if f.banked] + [_awkward(RC.BY_NAME[n]) for n in AWKWARD]


def short_outputs(lib, desc, f):
    """The longest row (a last cycle of one output) that plans U = 1 and fewer cycles a tile than the one-row lane-split kernel."""
    per_cycle = lib.fir_rows_plan(desc, 0, 1 << 20)["per_cycle"]
    for cycles in range(8 * (64 // f.M), 0, -1):
        n = (cycles - 1) * per_cycle + 1
        p = lib.fir_rows_plan(desc, 0, n, CLASS_ROWS, 0)
        if p["per_lane"] == 1 and p["cycles_per_tile"] < p["split_cycles_per_tile"]:
            return n
    raise AssertionError(f.name)


def class_cases(lib, f, desc=None):
    """-> [(case, geometry)]: short and long, with seams and without."""
    desc = desc if desc is not None else f.make(lib)
    n = short_outputs(lib, desc, f)
    cases = [RC.Case(f, CLASS_ROWS, "short", "three", "zero", 1, f.out_blocks[0], n_given=n),
             RC.Case(f, CLASS_ROWS, "short", "none", "zero", 2, f.out_blocks[-1], n_given=n),
             RC.Case(f, CLASS_ROWS, "3 tiles - 1", "three", "zero", 2, f.out_blocks[-1]),
             RC.Case(f, CLASS_ROWS, "3 tiles - 1", "none", "zero", 1, f.out_blocks[0])]
    out = [(c, RC.resolve(lib, c, desc)) for c in cases]
    c, g = out[0]
    if f.kind == "filter" and len(RC.seams_inside(f, g.k_begin, g.k_end, g.seam)) < 3:
        # a short filter row spans n - 1 + Lp inputs, under three seam blocks: from output seam - 1 on the range (seam - 1, ...)
        # holds one seam more than from output 0 on
        c = dataclasses.replace(c, first=g.seam - 1, seam_given=g.seam)
        out[0] = (c, RC.resolve(lib, c, desc))
    return out


def windows_holding(f, g, p):
    """Which outputs of the range read input sample p (the window of output m: the Lp // I samples from in_offset(m) on)."""
    m = np.arange(g.k_begin, g.k_end, dtype=np.int64)
    first = RC.SC.in_offset(m, f.I, f.D)
    return (first <= p) & (p < first + f.Lp // f.I)


def beside_a_seam(cross):
    """One outputs whose neighbour is Cross."""
    near = np.zeros_like(cross)
    near[1:] |= cross[:-1]
    near[:-1] |= cross[1:]
    return near & ~cross


def class_anchor(case, g):
    """The sample of the row the planted segments are aligned to: the first seam inside the range, or the middle of a seamless row."""
    f = case.family
    seams = RC.seams_inside(f, g.k_begin, g.k_end, g.seam)
    return seams[0] // f.I if seams else (g.in_base + RC.need_inputs(f, g)) // 2


def class_island(case, g):
    """The sample an Inf / NaN island is put on: within a window of the anchor, read by a Cross output and by a One output beside the
    seam (seamless: by two outputs at least), and among those samples the one the fewest outputs read -- a short filter row is
    shorter than two windows, and an island in its middle would make nearly every output NaN."""
    f = case.family
    lp, n = f.Lp // f.I, g.in_base + RC.need_inputs(f, g)
    anchor = class_anchor(case, g)
    cross = RC.cross_mask(f, g.k_begin, g.k_end, g.seam, case.out_block)
    near = beside_a_seam(cross)
    best = None
    for p in range(max(anchor - lp, 0), min(anchor + lp, n)):
        w = windows_holding(f, g, p)
        ok = (w & cross).any() and (w & near).any() if cross.any() else int(w.sum()) >= 2
        if ok and (best is None or int(w.sum()) < best[0]):
            best = (int(w.sum()), p)
    assert best is not None, case.name
    return best[1]


@functools.lru_cache(maxsize=None)
def _salted(width, lp, n, seed, large):
    base = RC.S.cfloat_block(n, seed=seed) if width == 2 else RC.S.real_block(n, seed=seed)
    x, table = VC.salt(base, width, lp, seed, large=large)
    x.setflags(write=False)
    return x, table


def class_rows(case, g):
    """-> (the rows' near streams, [(row, planted kind, sample of the row it was put on)])."""
    f = case.family
    w, lp = f.width, f.Lp // f.I
    n = g.in_base + RC.need_inputs(f, g)
    whole = -(-(n + 48 * lp + 64 + VC.BLOCK) // VC.BLOCK) * VC.BLOCK + 4 * lp + 8      # room for a pass behind any anchor, and a last
    anchor, island = class_anchor(case, g), class_island(case, g)                      # segment across the last 8192-sample edge
    # the zeros of the sub_in_zero run start where a window starts (the last one a window ahead of the anchor, or the first of the
    # range): that window reads lp zeros and nothing else, the next one the subnormals too
    first = RC.SC.in_offset(np.arange(g.k_begin, g.k_end), f.I, f.D)
    ahead = first[first <= anchor - lp]
    run = int(ahead[-1] if ahead.size else first[0])
    xs, planted = [fir_row_stream(case, g, 0, base=500_000)], []
    for row, kind, at in ((1, "sub_in_zero", run), (2, "inf_re", island), (3, "nan", island)):
        x, table = _salted(w, lp, whole, _seed(case, row, 500_000), (126, 127) if f.sym else (60, 62))
        seg = next(s for s in table if s["kind"] == kind and s["start"] >= max(at, 0))
        off = seg["start"] - at
        assert off >= 0 and off + n <= whole, (case.name, row, off, n, whole)
        xs.append(x[off * w:(off + n) * w])
        planted.append((row, kind, at))
    return xs, planted


_class_expected = {}


def class_expected(case, g, oracle):
    """-> (the rows' streams, what was planted, per row the outputs [k_begin, k_end) of the restated Pipe on that row's stream --
    cut into blocks of the seam, or one block -- as fir_rows_cases.pipe_expected builds them: no device code in it)."""
    if case.name not in _class_expected:
        xs, planted = class_rows(case, g)
        exp = [RC.pipe_expected(case, g, oracle, x) for x in xs]
        for e in exp:
            e.setflags(write=False)
        _class_expected[case.name] = (xs, planted, exp)
    return _class_expected[case.name]
