"""The table behind tests/test_gpu_fir_rows.py: small shapes of the FIR row forms (sdrhip_filter_run_rows,
sdrhip_decimator_run_rows, sdrhip_resampler_run_rows), chosen so that every branch of the rows kernel is reached.  No pytest in
here: tests/test_fir_rows_cases.py shows on the CPU, from the model alone, what the table reaches.

A case is a family (descriptor), a number of rows, a per-row output count taken from the rows plan (so that it moves with the
plan), a seam choice, a position and a row layout.  Every dimension's values occur in every banked family; the full product does
not (it would be thousands of launches): the six slots of SLOTS pair the values, and the family's index rotates the rows so that
over the families every (rows, size) pair occurs.

Positions.  "zero": in_base 0.  "forty": the first window starts at d_in[1], with in_base 40 where the factor allows it (the first
output whose window starts at or behind input 41 is taken, and in_base is that start minus 1: 40 for filters, 43 for a decimator
by 4, ...).  "far": "forty" moved above 2^33 by the translation rule of tests/stream_slice_cases.py (S = n D B outB inputs,
T = S I / D outputs), so the near stream's answer is the far launch's.  With a seam the first output then moves forward, by as
little as it takes, until the range holds a Cross output.

Row layouts, in floats: (gap between input rows, gap between output rows, offset of the first input row, of the first output row
from a 256-byte boundary).  Complex rows take even numbers only (an odd stride is refused, and a base 4 bytes off would misalign
the (re, im) pairs themselves, which no operator of the library accepts): their bases are 8 bytes off, real rows' 4 and 8."""
import dataclasses
from typing import Callable

import numpy as np

from oracle import pipes_model as PM
import signals as S
import stream_slice_cases as SC

AVX, SSE, SCALAR = PM.ORDER_AVX, PM.ORDER_SSE, PM.ORDER_SCALAR
ROWS = (1, 3, 33)
_REAL = {SCALAR: 1, SSE: 4, AVX: 8}
_CPLX = {SCALAR: 1, SSE: 2, AVX: 4}


def _round_up(n, d):
    return -(-n // d) * d


@dataclasses.dataclass(frozen=True)
class Family:
    name: str
    kind: str                       # "filter" | "decimator" | "resampler"
    taps: Callable[[], np.ndarray]
    order: int = AVX
    complex_: bool = False
    sym: bool = False
    I: int = 1
    D: int = 1
    M: int = 8                      # partial sums per output = lanes per output of the tile kernel (0: not a banked shape)
    out_blocks: tuple = (0,)        # resamplers: the Pipe's output block sizes the cases alternate between

    @property
    def banked(self):
        return self.M > 0

    @property
    def width(self):
        return 2 if self.complex_ else 1

    @property
    def Lp(self):
        n = self.taps().size
        if self.kind == "resampler":
            return _round_up(n, self.I * _REAL[self.order])
        if self.sym:
            return 2 * n
        return _round_up(n, (_CPLX if self.complex_ else _REAL)[self.order])

    @property
    def chunks(self):
        """Chunks of M taps one output walks (kernels_split.hip: nch)."""
        if self.kind == "resampler":
            return _round_up(-(-self.taps().size // self.I), _REAL[self.order]) // self.M
        return (self.taps().size if self.sym else self.Lp) // self.M

    @property
    def min_seam(self):
        return -(-self.Lp // self.I)

    def make(self, hip):
        if self.kind == "filter":
            return hip.Filter(self.taps(), self.order, complex_=self.complex_, sym=self.sym)
        if self.kind == "decimator":
            return hip.Decimator(self.D, self.taps(), self.order, complex_=self.complex_, sym=self.sym)
        return hip.Resampler(self.I, self.D, self.taps(), self.order, self.complex_)

    def model(self, oracle):
        if self.kind == "resampler":
            return PM.ResamplerModel(oracle, self.I, self.D, self.taps(), self.order, self.complex_)
        return PM.FilterModel(oracle, self.taps(), self.order, complex_=self.complex_, sym=self.sym, factor=self.D)


def _g(n, seed):
    return lambda: S.gauss_taps(n, seed)


# chunk counts: complex 16 (exact) and 12; real 8 (exact: the guard-free instantiation where U = 2), 8 (symmetric), 10, 2 and 1
FAMILIES = [
    Family("cdec AVX /4, 64 taps", "decimator", _g(64, 604), complex_=True, D=4, M=4),
    Family("cdec SSE /3, 31 taps", "decimator", _g(31, 331), order=SSE, complex_=True, D=3, M=2),
    Family("rdec AVX /5, 61 taps", "decimator", _g(61, 561), D=5, M=8),
    Family("rfilt sym SSE, the chain's audio taps", "filter", S.taps_example_audio_filter_half, order=SSE, sym=True, M=4),
    Family("rfilt AVX, 77 taps", "filter", _g(77, 177), M=8),
    Family("cfilt AVX, 45 taps", "filter", _g(45, 145), complex_=True, M=4),
    Family("rres 3/10 AVX, the chain's taps", "resampler", S.taps_example_audio_resampler, I=3, D=10, M=8, out_blocks=(97, 1000)),
    Family("cres 7/9 SSE, 100 taps", "resampler", _g(100, 79), order=SSE, complex_=True, I=7, D=9, M=4, out_blocks=(97, 1000)),
    # padded length 12 within [D, D + I - 1]: every fifth seam of 4 inputs has no crossover (kernels.hpp seam_has_crossover)
    Family("rres 3/10 SSE, 10 taps", "resampler", _g(10, 310), order=SSE, I=3, D=10, M=4, out_blocks=(97, 1000)),
    # fallbacks: not banked shapes (the scalar order has no lanes to split; 97 polyphase groups are more than 64)
    Family("fallback: rdec scalar /3, 40 taps", "decimator", _g(40, 340), order=SCALAR, D=3, M=0),
    Family("fallback: rres 97/100 AVX, 1500 taps", "resampler", _g(1500, 197), I=97, D=100, M=0, out_blocks=(97, 1000)),
]
BY_NAME = {f.name: f for f in FAMILIES}

LAYOUTS_CPLX = [(0, 0, 0, 0), (2, 6, 0, 0), (6, 2, 2, 2)]
LAYOUTS_REAL = [(0, 0, 0, 0), (1, 3, 1, 2), (3, 1, 2, 1)]
SIZES = ("one", "lane group - 1", "tile", "tile + 1", "3 tiles - 1")
# (size, seam, position, layout); the rows rotate with the family
SLOTS = [
    ("one", "min", "zero", 0),
    ("lane group - 1", "none", "forty", 1),
    ("tile", "three", "zero", 2),
    ("tile + 1", "min", "far", 1),
    ("3 tiles - 1", "three", "forty", 0),
    ("tile", "none", "far", 2),
]
FALLBACK_SIZES = {"one": 1, "lane group - 1": 7, "tile": 100, "tile + 1": 101, "3 tiles - 1": 299}


@dataclasses.dataclass(frozen=True)
class Case:
    family: Family
    rows: int
    size: str
    seam_kind: str                  # "none" | "min" | "three"
    pos: str                        # "zero" | "forty" | "far"
    layout: int
    out_block: int = 0
    first: int = -1                 # >= 0: the first output, as given (the directed cases)
    n_given: int = 0
    seam_given: int = 0

    @property
    def name(self):
        return f"{self.family.name}: {self.rows} rows x {self.size}, seam {self.seam_kind}, {self.pos}, layout {self.layout}" + (
            f", out_block {self.out_block}" if self.out_block else "") + (f", from output {self.first}" if self.first >= 0 else "")

    @property
    def layout_floats(self):
        return (LAYOUTS_CPLX if self.family.complex_ else LAYOUTS_REAL)[self.layout]


def _cases():
    out = []
    for fi, f in enumerate(FAMILIES):
        for si, (size, seam, pos, layout) in enumerate(SLOTS):
            out.append(Case(f, ROWS[(si + fi) % 3], size, seam, pos, layout, f.out_blocks[si % len(f.out_blocks)]))
    chain = BY_NAME["rres 3/10 AVX, the chain's taps"]
    # directed: output 1843 = 19 * 97 opens an output block of 97, its window straddles the seam at 18432 = 96 * 192 (seam block 64),
    # where the Pipe does cross over, and its first input lies behind that seam (late_output_is_one): a One output ...
    out.append(Case(chain, 3, "40 outputs", "64", "zero", 1, 97, first=1830, n_given=40, seam_given=64))
    # ... and with unbounded output blocks the same output is Cross
    out.append(Case(chain, 3, "40 outputs", "64", "zero", 0, 0, first=1830, n_given=40, seam_given=64))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)


@dataclasses.dataclass(frozen=True)
class Geometry:
    """A case resolved against the rows plan: the NEAR launch (in_base, k_begin, k_end on the stream that starts at 0), the
    shift (S inputs, T outputs) of the launch actually made, the seam block, and the plan it was sized from."""
    in_base: int
    k_begin: int
    k_end: int
    seam: int
    S: int
    T: int
    tile: int                       # outputs of a full tile of a long row (0: fallback)
    plan: object                    # the rows plan of this very launch (None: fallback)

    @property
    def n(self):
        return self.k_end - self.k_begin


def cross_mask(f, a, b, seam, out_block):
    """The One / Cross decision of kernels.hpp for outputs [a, b) of the near stream."""
    if seam <= 0:
        return np.zeros(b - a, bool)
    return SC.is_cross(np.arange(a, b, dtype=np.int64), f.I, f.D, f.Lp, seam, out_block)


def seams_inside(f, a, b, seam):
    """Multiples of seam * I strictly inside the launch's window range (kernels.hpp seam_span), in upsampled units."""
    if seam <= 0:
        return []
    bi = seam * f.I
    v_lo, v_hi = a * f.D, (b - 1) * f.D + f.Lp
    return list(range((v_lo // bi + 1) * bi, v_hi, bi))


def resolve(L, case, desc=None):
    """-> Geometry.  L: sdr_amd.lib (the plan hook is host arithmetic: no device needed)."""
    f = case.family
    desc = desc if desc is not None else f.make(L)
    k0 = 0
    if case.pos != "zero":
        while SC.in_offset(k0, f.I, f.D) < 41:
            k0 += 1
    if case.first >= 0:
        k0 = case.first
    long_plan = L.fir_rows_plan(desc, k0, k0 + (1 << 20))
    assert (long_plan is not None) == f.banked, f.name
    if f.banked:
        tile = long_plan["split_cycles_per_tile"] * long_plan["per_cycle"]
        n = {"one": 1, "lane group - 1": 64 // f.M * long_plan["per_cycle"] - 1, "tile": tile, "tile + 1": tile + 1, "3 tiles - 1": 3 * tile - 1}.get(case.size, 0)
    else:
        tile, n = 0, FALLBACK_SIZES.get(case.size, 0)
    n = case.n_given or n
    if case.seam_given:
        seam = case.seam_given
    elif case.seam_kind == "none":
        seam = 0
    elif case.seam_kind == "min":
        seam = f.min_seam
    else:
        seam = max(f.min_seam, ((n - 1) * f.D + f.Lp) // (4 * f.I))
    if seam and case.first < 0:
        for _ in range(4 * seam * f.I):
            if cross_mask(f, k0, k0 + n, seam, case.out_block).any():
                break
            k0 += 1
    in_base = 0 if case.pos == "zero" else int(SC.in_offset(k0, f.I, f.D)) - 1
    S_, T_ = 0, 0
    if case.pos == "far":
        unit = f.D * max(seam, 1) * (case.out_block if case.out_block > 0 else 1)
        S_ = ((1 << 33) // unit + 1) * unit
        T_ = S_ * f.I // f.D
        assert T_ * f.D == S_ * f.I
    plan = L.fir_rows_plan(desc, T_ + k0, T_ + k0 + n, case.rows, seam) if f.banked else None
    return Geometry(in_base, k0, k0 + n, seam, S_, T_, tile, plan)


def need_inputs(f, g):
    """Stream elements a row holds from in_base on: the header's guaranteed range of the launch."""
    return int(SC.in_offset(g.k_end - 1, f.I, f.D)) + f.Lp // f.I - g.in_base


def row_stream(case, g, row, variant=0):
    """The near stream of one row from element 0 to the end of its guaranteed range (floats; complex: interleaved), seeded by the
    case and the row.  Never written to."""
    f = case.family
    n = g.in_base + need_inputs(f, g)
    seed = 7000 + 131 * CASES.index(case) + 17 * row + 1009 * variant
    x = S.cfloat_block(n, seed=seed) if f.complex_ else S.real_block(n, seed=seed)
    x.setflags(write=False)
    return x


def pipe_expected(case, g, oracle, x):
    """Outputs [k_begin, k_end) of the restated Pipe (oracle/pipes_model.py) on the near stream x of one row, computed as
    tests/test_gpu_stream_slices.py computes its expected values: the stream cut into blocks of the seam (one block for a contiguous
    stream), the Pipe's own One / Cross decisions.  The stream is extended by zeros so that the Pipe yields the block that holds the
    last output (it yields whole blocks only); outputs up to k_end - 1 do not read them."""
    f = case.family
    w = f.width
    model = f.model(oracle)
    assert model.num_coeffs == f.Lp
    # an unbounded output block: one that ends with the range, so that no output of the range opens a block
    pipe_out = case.out_block if case.out_block > 0 else g.k_end
    want = _round_up(g.k_end, pipe_out)
    have = x.size // w
    total = max(int(SC.in_offset(want, f.I, f.D)) + f.Lp // f.I + 1, have)
    if g.seam:
        total = _round_up(total, g.seam) + g.seam
    ext = np.concatenate([x, np.zeros((total - have) * w, np.float32)])
    blk = g.seam if g.seam else total
    blocks = [ext[i * blk * w:(i + 1) * blk * w] for i in range(total // blk)]
    if f.kind == "resampler":
        out, _ = PM.fir_resampler_pipe(model, blocks, pipe_out)
    else:
        out, _ = PM.fir_decimator_pipe(model, blocks, pipe_out)
    out = np.concatenate(out)
    assert out.size >= g.k_end * w, (case.name, out.size, g.k_end)
    return out[g.k_begin * w:g.k_end * w]


def pipe_cases():
    """The cases held to the restated Pipe as well: per family its case with three seams in a row that has the fewest rows, and the
    directed cases.  (A seam block just at the padded filter length is a launch the device operators define by the One / Cross rule,
    but with a factor above 1 not a Pipe the reference can run: firDecimator's own `assert`s fire on it, Filter.hs:574-611.)"""
    out = {}
    for c in sorted((c for c in CASES if c.seam_kind == "three"), key=lambda c: c.rows):
        out.setdefault(c.family.name, c)
    assert len(out) == len(FAMILIES) and all(c.rows <= 3 for c in out.values())
    return list(out.values()) + [c for c in CASES if c.first >= 0]
