"""The table behind tests/test_gpu_tail_any_family.py: the general fused audio tail (k_audio_tail_rows_any, kernels_tail_any.hip) on
EVERY part of the family its predicate admits (audio_tail_any_fits) -- every coprime ratio I/D, every group length 8 .. 64, every
filter length 16 .. 128, the tap counts that decide how a Cross walk ends, the ten shapes whose y window fills the 5120 floats it
may take, and stream positions beyond 2^33 at a block that is no power of two.  tests/audio_tail_any_cases.py runs nine shapes of
that family; this table is derived from the restated predicate, not written out.  No pytest in here:
tests/test_tail_any_family_cases.py shows on the CPU, from the models alone, what the table reaches.

Tap sets.  Resampler: S.gauss_taps(n, 7000 + n) (seeded; the last taps are nonzero).  Audio filter: the symmetric halves
S.gauss_taps(h, 7600 + h), h = 8, 16 .. 64.

Expected values come from the restated Pipes only (oracle/pipes_model.py), through the helpers of tests/audio_tail_any_cases.py
(expected, expected_from, z_stream, filter_stream, padded): computed once, cached and read-only; no device run is a source of
expected values.

The reference's undefined zone.  firResampler asserts ("resample 1", Filter.hs:691) when, behind a buffer boundary, the first output
that starts in the new buffer does not fit in it.  Behind boundary k that output starts u_k = (-k B I) mod D upsampled units into
the buffer of B I, and it fits when u_k + numCoeffsR <= B I: block B asserts on a stream of n blocks exactly when some k in
1 .. n - 1 has u_k > B I - numCoeffsR (`asserts` below).  u_k < D, so the zone lies inside [numCoeffsR / I, (numCoeffsR + D - 1) / I):
up to ceil((D - 1) / I) blocks above the lowest one create admits, and not only the block with B I == numCoeffsR.  The tail's create
admits those blocks and the kernels serve them; there the table has no expected values and holds route against route."""
import dataclasses
import functools

import numpy as np

import audio_tail_any_cases as AC
import signals as S
import stream_slice_cases as SC

TILE, Q_MAX = AC.TILE, AC.Q_MAX
WINDOW_FLOATS, MAX_GROUP, MAX_FILTER, MAX_INTERP = AC.WINDOW_FLOATS, AC.MAX_GROUP, AC.MAX_FILTER, AC.MAX_INTERP
NLOOPS = tuple(range(8, MAX_GROUP + 1, 8))
LFS = tuple(range(16, MAX_FILTER + 1, 16))
ODD_BLOCK = 257                                       # a few hundred, odd, prime: no multiple of any I or of 8
FAR_BLOCKS = (250, 257)                               # neither divides 2^32
CUTS = (841, 1709)                                    # odd, and on no polyphase cycle of I = 2 .. 8
OFF_CYCLE = (829, 863)                                # q0 % I and q1 % I nonzero and different for I = 3 .. 8; spans the tile edge 840
FEW_START = 1003
EDGE_INTERPS = (1, 3, 5, 6, 8)
assert all(q % 2 == 1 and all(q % I for I in range(2, 9)) for q in CUTS)
assert all(OFF_CYCLE[0] % I and OFF_CYCLE[1] % I and OFF_CYCLE[0] % I != OFF_CYCLE[1] % I for I in range(3, 9))

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


@dataclasses.dataclass(frozen=True)
class Shape(AC.Shape):
    """audio_tail_any_cases.Shape on the family's seeded tap sets."""

    def resamp_taps(self):
        return _frozen(("r", self.ntaps), lambda: S.gauss_taps(self.ntaps, 7000 + self.ntaps))

    def audio_half(self):
        return _frozen(("h", self.nhalf), lambda: S.gauss_taps(self.nhalf, 7600 + self.nhalf))

    @property
    def nfc(self):                 # chunks of eight half-taps
        return self.nhalf // 8

    @property
    def row_stride(self):          # prepare_coeffs: the longest group, rounded up to the 8 lanes -- the group length itself
        return self.nloop

    @property
    def terms(self):               # products of an output at most
        return -(-self.ntaps // self.I)


def make_shape(I, D, ntaps, nhalf):
    return Shape(f"{I}/{D} x {ntaps}, {nhalf} half-taps", I, D, ntaps, nhalf)


# ---- the predicate, restated ---------------------------------------------------------------------------------------------------
def general_fits(shape, block, nhalf=None):
    """audio_tail_any_fits: AC.general_fits and the two clauses it leaves out (a tap count the kernel's LDS copy holds, group rows
    no shorter than the walk and no longer than the cap)."""
    return bool(AC.general_fits(shape, block, nhalf)) and 1 <= shape.ntaps <= MAX_GROUP * shape.I and shape.nloop <= shape.row_stride <= MAX_GROUP


def create_admits(shape, block, nhalf=None):
    """sdrhip_audio_tail_create's own condition on the block (audio_tail.cpp)."""
    lf = 2 * (nhalf or shape.nhalf)
    return block == 0 or (block * shape.I >= shape.rlp and shape.rlp >= shape.D and block >= lf)


def window_sum(I, D, nloop, lf):
    """The left side of the predicate's window bound: D (NC - 1) + premax + nloop + 8."""
    return D * (-(-(TILE + lf - 1) // I) - 1) + int(SC.in_offset(I - 1, I, D)) + nloop + 8


def fits(I, D, nloop, lf):
    """The shape part of the predicate for a ratio, a group length and a filter length (the tap count fills the groups)."""
    if nloop % 8 or lf % 16 or nloop < 8 or lf < 16:
        return False
    return general_fits(Shape("", I, D, I * nloop, lf // 2), 0)


@functools.lru_cache(maxsize=None)
def admitted(I, D):
    return tuple((nloop, lf) for nloop in NLOOPS for lf in LFS if fits(I, D, nloop, lf))


RATIOS = [(I, D) for I in range(1, MAX_INTERP + 2) for D in range(I + 1, 64) if admitted(I, D)]
MAX_D = {I: max(d for i, d in RATIOS if i == I) for I in sorted({i for i, _ in RATIOS})}
ADMITTED_GROUPS = {(I, nloop) for I, D in RATIOS for nloop, _ in admitted(I, D)}
ADMITTED_CHUNKS = {(I, lf // 16) for I, D in RATIOS for _, lf in admitted(I, D)}


def generic_ntaps(I, D, nloop):
    """A count inside the group length that is neither a multiple of I (for I > 1) nor one below a multiple of 8 I throughout."""
    n = I * nloop - 1 - (3 * D + nloop // 8) % 5
    assert I * (nloop - 8) < n <= I * nloop
    return n


# ---- the reference's undefined zone ---------------------------------------------------------------------------------------------
def asserts(shape, block, nblocks=0):
    """Does firResampler(block) assert on a stream of nblocks blocks (0: however long)?  See the module text."""
    slack = block * shape.I - shape.rlp
    ks = range(1, nblocks) if nblocks else range(1, shape.D + 1)
    return any((-k * block * shape.I) % shape.D > slack for k in ks)


def zone(shape, nblocks=0):
    """The blocks create admits at which the reference's Pipe is not defined."""
    return [b for b in range(shape.lowest_block, shape.lowest_block + shape.D) if asserts(shape, b, nblocks)]


def first_defined(shape):
    b = shape.lowest_block
    while asserts(shape, b):
        b += 1
    return b


# ---- the shapes -----------------------------------------------------------------------------------------------------------------
def _assign():
    """At least two (group length, filter length) per ratio, taken so that over the ratios of one I every admitted group length and
    every admitted chunk count runs: each ratio first takes its longest window among the picks that cover something new."""
    picks = {}
    for I in sorted(MAX_D):
        ds = [d for i, d in RATIOS if i == I]
        need_n = {n for i, n in ADMITTED_GROUPS if i == I}
        need_f = {f for i, f in ADMITTED_CHUNKS if i == I}
        rounds = 0
        while rounds < 2 or need_n or need_f:
            for D in ds:
                mine = picks.setdefault((I, D), [])
                cand = [c for c in admitted(I, D) if c not in mine]
                if not cand:
                    continue
                gain = lambda c: (c[0] in need_n) + (c[1] // 16 in need_f)                           # noqa: E731
                order = (lambda c: window_sum(I, D, *c)) if rounds == 0 else (lambda c: -((c[0] // 8 + 3 * (c[1] // 16) + D + rounds) % 11))
                best = max(cand, key=lambda c: (gain(c), order(c)))
                if rounds >= 2 and gain(best) == 0:
                    continue
                mine.append(best)
                need_n.discard(best[0])
                need_f.discard(best[1] // 16)
            rounds += 1
            assert rounds < 12, (I, need_n, need_f)
    return picks


ASSIGNED = _assign()
SHAPES, KINDS = {}, {}


def _add(shape, kind):
    SHAPES.setdefault(shape.name, shape)
    KINDS.setdefault(shape.name, set()).add(kind)
    return SHAPES[shape.name]


for (_I, _D), _combos in ASSIGNED.items():
    for _nloop, _lf in _combos:
        _add(make_shape(_I, _D, generic_ntaps(_I, _D, _nloop), _lf // 2), "ratio")

# one shape per I for the launches that are run once per I: the largest D, on its longest window
ONE_PER_I = {I: SHAPES[make_shape(I, MAX_D[I], generic_ntaps(I, MAX_D[I], ASSIGNED[I, MAX_D[I]][0][0]), ASSIGNED[I, MAX_D[I]][0][1] // 2).name]
             for I in sorted(MAX_D)}

# ---- tap-count edges: the largest ratio whose eight-float groups still span D (numCoeffsR = 8 I >= D) -------------------------------
# The counts up to I leave most z values zero (a group without a tap): those shapes take the largest such ratio that admits the
# longest filter, so that an audio output still sums enough nonzero products for the two summation orders to differ.
EDGE_KINDS = ("ntaps == I nloop", "ntaps == I nloop - (I - 1)", "ntaps a multiple of I, not of 8 I", "ntaps == I", "ntaps < I", "ntaps == 1")


def _edge_shapes():
    out = []
    for I in EDGE_INTERPS:
        counts = (("ntaps == I nloop", 24, 24 * I), ("ntaps == I nloop - (I - 1)", 16, 16 * I - (I - 1)),
                  ("ntaps a multiple of I, not of 8 I", 32, 29 * I), ("ntaps == I", 8, I), ("ntaps < I", 8, I // 2 + 1), ("ntaps == 1", 8, 1))
        for j, (kind, nloop, n) in enumerate(counts):
            if kind == "ntaps < I" and n >= I:
                continue                                                 # I = 1 has no such count
            if n <= I:
                D = max(d for i, d in RATIOS if i == I and d <= 8 * I and (nloop, MAX_FILTER) in admitted(I, d))
                lf = MAX_FILTER
            else:
                D = max(d for i, d in RATIOS if i == I and d <= 8 * I)
                lfs = [lf for nl, lf in admitted(I, D) if nl == nloop]
                assert lfs, (I, D, nloop)
                lf = lfs[(I + j) % len(lfs)]
            s = make_shape(I, D, n, lf // 2)
            assert s.nloop == nloop
            out.append((s, kind))
    return out


for _s, _kind in _edge_shapes():
    _add(_s, _kind)

# ---- window edges: every admitted (I, D, nloop, Lf) whose window sum is within 7 of the 5120 floats ----------------------------------
WINDOW_POINTS = [(I, D, nloop, lf) for I, D in RATIOS for nloop, lf in admitted(I, D) if window_sum(I, D, nloop, lf) >= WINDOW_FLOATS - 7]
WINDOW_EDGES = [_add(make_shape(I, D, generic_ntaps(I, D, nloop), lf // 2), "window edge") for I, D, nloop, lf in WINDOW_POINTS]
# the same shape with the next group length and with the next filter length: for the predicate only, never launched
WINDOW_NEIGHBOURS = {(I, D, nloop, lf): [p for p in ((I, D, nloop + 8, lf), (I, D, nloop, lf + 16)) if not fits(*p)] for I, D, nloop, lf in WINDOW_POINTS}

SALTED_KINDS = ("ntaps < I", "ntaps == I nloop - (I - 1)")


def is_fm_tail(s):
    """The shape k_audio_tail_rows is written for: on route 0 its rule comes before the general kernel's."""
    return (s.I, s.D, s.nloop, s.nhalf) == (3, 10, 64, 64)


# ---- the launches ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Launch(AC.Launch):
    shift: tuple = (0, 0)          # (outputs, inputs) a far launch is moved by
    zone: bool = False             # the block lies in the reference's undefined zone: route against route only
    route2: bool = False           # route 2 is held to the same expected values
    salted: bool = False           # one row with isolated +inf, -inf and NaN samples

    @property
    def far_shift(self):
        return self.shift


def far_shift(shape, block):
    """T = I block 2^k outputs and S = D block 2^k inputs, the smallest k with T > 2^33."""
    k = 0
    while (shape.I * block) << k <= 1 << 33:
        k += 1
    return (shape.I * block) << k, (shape.D * block) << k


def tile_bases(shape, q0, q1, T=0):
    """First audio output of every tile of the launch [T + q0, T + q1) (kernels_tail_any.hip: qa)."""
    qa0 = (T + q0) // shape.I * shape.I
    return [qa0 + TILE * t for t in range(-(-(T + q1 - qa0) // TILE))]


def _launches_of(s, idx):
    n, I = s.name, s.I
    b1 = first_defined(s)
    out = [
        Launch(f"{n}: [0, N) whole, block {b1}", s, b1, 0, Q_MAX, rows=1, exact=False, seamed=True),
        Launch(f"{n}: [0, N) whole, block {ODD_BLOCK}", s, ODD_BLOCK, 0, Q_MAX, rows=3, exact=False, seamed=True, route2=True),
        Launch(f"{n}: contiguous", s, 0, 1, Q_MAX, rows=33 if is_fm_tail(s) else 3),
        Launch(f"{n}: three runs", s, b1 if idx % 2 else ODD_BLOCK, 0, Q_MAX, rows=1 if idx % 2 else 3, cuts=CUTS, seamed=True),
        Launch(f"{n}: off-cycle start and end", s, b1, OFF_CYCLE[0], OFF_CYCLE[1], rows=3),
        Launch(f"{n}: fewer than I outputs", s, ODD_BLOCK, FEW_START, FEW_START + max(I - 1, 1), rows=1),
    ]
    if s is ONE_PER_I[I] or "window edge" in KINDS[n]:
        for off in range(4):                                             # every staging shift with the tile's window at its longest
            out.append(Launch(f"{n}: whole tile, y rows from {4 * off} bytes past a 16-byte boundary", s, b1 if off % 2 else ODD_BLOCK, 0, TILE,
                              rows=3, layout=(0, 0, off, (off + 1) % 4)))
    if s is ONE_PER_I[I]:
        out.append(Launch(f"{n}: 32 rows", s, ODD_BLOCK, 3, 1900, rows=32, exact=False, seamed=True))
        for block in FAR_BLOCKS:
            out.append(Launch(f"{n}: far, block {block}", s, block, 5, 700, rows=1, far=True, seamed=True, shift=far_shift(s, block)))
    if KINDS[n] & set(SALTED_KINDS):
        out.append(Launch(f"{n}: inf and nan samples", s, ODD_BLOCK, 0, Q_MAX, rows=1, exact=False, seamed=True, salted=True))
    z = zone(s)
    if z:
        out.append(Launch(f"{n}: inside the reference's undefined zone, block {z[0]}", s, z[0], 0, Q_MAX, rows=1, exact=False, zone=True))
    return out


LAUNCHES = {name: _launches_of(s, idx) for idx, (name, s) in enumerate(SHAPES.items())}
ALL_LAUNCHES = [c for cs in LAUNCHES.values() for c in cs]
assert len({c.name for c in ALL_LAUNCHES}) == len(ALL_LAUNCHES)


def padded_position(shape, block, k):
    """A y index behind buffer boundary k that a Cross output's grouped walk would multiply by a padded zero tap and its sequential
    walk never reads: the last float of the group walk of the first such output (a group shorter than nloop); None if there is none."""
    I, D = shape.I, shape.D
    for m in AC.resampler_cross(shape, block, max((k * block * I - shape.rlp) // D, 0), k * block * I // D + 1):
        fo = int(-(-m * D // I) * I - m * D)
        if (shape.ntaps - fo + I - 1) // I < shape.nloop:
            return shape.first_input(int(m)) + shape.nloop - 1
    return None


def salted_row(shape, block=ODD_BLOCK):
    """Row 0 of seed 5 with isolated +inf, -inf and NaN samples, one behind each of a few buffer boundaries of the resampler, where
    a Cross output's grouped walk would multiply it by a padded zero tap (0 * inf = NaN) and the sequential walk does not read it.
    With I = 1 and ntaps == nloop no tap is padded: the samples sit one input behind the boundary."""
    def make():
        y = AC.y_row(shape, 0, seed=5).copy()
        for j, k in enumerate((1, 2, 3, 5, 6, 8)):
            at = padded_position(shape, block, k)
            at = k * block + 1 if at is None else at
            if at < y.size:
                y[at] = (np.inf, -np.inf, np.nan)[j % 3]
        for j, k in enumerate((4, 7)):                                   # ... and two in the middle of a buffer, which every walk reads
            if k * block + 100 < y.size:
                y[k * block + 100] = (-np.inf, np.nan)[j]
        return y
    return _frozen(("salted", shape.name, block), make)


def salted_expected(oracle, shape, block=ODD_BLOCK):
    return _frozen(("salted*", shape.name, block), lambda: AC.expected_from(oracle, shape, salted_row(shape, block), block, 1.0)[:Q_MAX])


def few_terms(shape):
    """Up to three products sum to the same bits grouped ((a0 + a1) + (a2 + 0)) and in sequence: on finite streams such a resampler's
    Cross outputs equal their grouped values, and only non-finite input tells the walks apart."""
    return shape.terms <= 3
