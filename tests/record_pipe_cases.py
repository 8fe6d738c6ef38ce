"""The case table of the record-seam Pipe tests (tests/test_record_pipe_cases.py on the CPU, tests/test_gpu_record_pipes.py on the
device): which Filter / Decimator / Resampler records are driven through the restated Pipes (oracle/pipes_model.py), on which
blocks.  One table, so that what the CPU test proves about the inputs (which transitions and branches they reach) holds for the
inputs the device sees.  No device code here.

Per case: 12 seeded source blocks of random length, and every case runs at both output block sizes.  The lower bounds of the block
lengths are the shortest blocks on which none of the reference's `assert`s fire (Filter.hs:544-720): a block of only numCoeffs
elements trips "decimate 1" on the remainder of a crossover, numCoeffs == factor trips "decimate 3"."""
import functools
import zlib
from collections import namedtuple

import numpy as np

from oracle import pipes_model as PM
from oracle.oracle import round_up
import signals as S

ORDERS = {"scalar": PM.ORDER_SCALAR, "sse": PM.ORDER_SSE, "avx": PM.ORDER_AVX}
REAL_LANES = {"scalar": 1, "sse": 4, "avx": 8}
CPLX_LANES = {"scalar": 1, "sse": 2, "avx": 4}
NUM_BLOCKS = 12
OUT_BLOCKS = (97, 1000)

FIR_FACTORS = (1, 2, 3, 5, 8, 16)
FIR_TAPS = (5, 31, 64, 127)
SYM_HALVES = (8, 32, 64)
SYM_FACTORS = (1, 2, 3, 8)
RATIOS = ((3, 10), (2, 3), (5, 7), (7, 11), (1, 2), (3, 23), (13, 17))
MANY_GROUPS = (97, 100)            # more than 64 polyphase groups: the resampler's d_ext table
MANY_GROUPS_TAPS = (291, 500)

# kind: "fir" (factor 1 = Filter, else Decimator), "sym" (the symmetric real ones; ntaps = the half length) or "resampler"
Case = namedtuple("Case", "kind order cplx factor ntaps I D")


def case_id(c):
    data = "c" if c.cplx else "r"
    if c.kind == "resampler":
        return f"resampler-{c.order}-{data}-{c.I}_{c.D}-t{c.ntaps}"
    return f"{c.kind}-{c.order}-{data}-d{c.factor}-t{c.ntaps}"


def num_coeffs(c):
    """numCoeffsF / numCoeffsD / numCoeffsR: the padded length the Pipe sees (Filter.hs:167-175, 234-245, 322-331, 422)."""
    if c.kind == "sym":
        return 2 * c.ntaps
    if c.kind == "resampler":
        return round_up(c.ntaps, c.I * REAL_LANES[c.order])
    return round_up(c.ntaps, (CPLX_LANES if c.cplx else REAL_LANES)[c.order])


def family(c):
    """(operation, order, complex data): what the per-family conditions of the CPU test are counted over."""
    op = c.kind if c.kind == "resampler" else {"fir": "", "sym": "sym_"}[c.kind] + ("filter" if c.factor == 1 else "decimator")
    return op, c.order, c.cplx


def group_key(c):
    """(kind, order, complex data): one parametrised GPU test per key."""
    return c.kind, c.order, c.cplx


def _fir_cases():
    out = []
    for order in ORDERS:
        for cplx in (False, True):
            for factor in FIR_FACTORS:
                for ntaps in FIR_TAPS:
                    c = Case("fir", order, cplx, factor, ntaps, 1, factor)
                    if num_coeffs(c) > factor:
                        out.append(c)
    for order in ("sse", "avx"):
        for half in SYM_HALVES:
            for factor in SYM_FACTORS:
                out.append(Case("sym", order, False, factor, half, 1, factor))
    return out


def _resampler_cases():
    out = []
    for order in ORDERS:
        for cplx in (False, True):
            for I, D in RATIOS:
                for ntaps in (3 * I, 31, 191):
                    out.append(Case("resampler", order, cplx, 1, ntaps, I, D))
    for ntaps in MANY_GROUPS_TAPS:
        out.append(Case("resampler", "avx", False, 1, ntaps, *MANY_GROUPS))
    return out


FIR_CASES = tuple(_fir_cases())
RESAMPLER_CASES = tuple(_resampler_cases())
CASES = FIR_CASES + RESAMPLER_CASES
GROUPS = tuple(sorted({group_key(c) for c in CASES}))


def cases_of(key):
    return [c for c in CASES if group_key(c) == key]


def _seed(c, what):
    return zlib.crc32(f"{case_id(c)}/{what}".encode())


def taps(c):
    return S.gauss_taps(c.ntaps, _seed(c, "taps"))


def block_lengths(c):
    """NUM_BLOCKS lengths in elements: FIR in [numCoeffs + factor, 3 numCoeffs + factor + 200], resampler in
    [ceil(numCoeffsR / I) + D, 3 * that + 200]."""
    L = num_coeffs(c)
    if c.kind == "resampler":
        lo = PM.quot_up(L, c.I) + c.D
        hi = 3 * lo + 200
    else:
        lo, hi = L + c.factor, 3 * L + c.factor + 200
    return [int(n) for n in np.random.default_rng(_seed(c, "lengths")).integers(lo, hi + 1, NUM_BLOCKS)]


@functools.lru_cache(maxsize=None)
def blocks(c):
    """The case's source blocks (interleaved pairs for complex data), read-only: shared by every run of the case."""
    rng = np.random.default_rng(_seed(c, "blocks"))
    w = 2 if c.cplx else 1
    out = []
    for n in block_lengths(c):
        b = rng.uniform(-1.0, 1.0, n * w).astype(np.float32)
        b.setflags(write=False)
        out.append(b)
    return tuple(out)


def make_model(c, oracle, filter_cls=PM.FilterModel, resampler_cls=PM.ResamplerModel):
    """The case's record: the plain model by default, the device-backed one with tests/record_models.py's classes."""
    if c.kind == "resampler":
        return resampler_cls(oracle, c.I, c.D, taps(c), ORDERS[c.order], c.cplx)
    return filter_cls(oracle, taps(c), ORDERS[c.order], complex_=c.cplx, sym=c.kind == "sym", factor=c.factor)


def instrument(model, results=None):
    """Log every closure call of a record the way the Pipe made it: ("one", count, len(buf)[, dat]) /
    ("cross", count, len(last), len(next)[, dat]), lengths in elements.  -> the list the calls are appended to.
    results: a list that receives what each call returned (the vector; for a resampler the whole (vector, dat, offset))."""
    calls = []

    def keep(r):
        if results is not None:
            results.append(r)
        return r
    w = model.width
    one, cross = model.one, model.cross
    if isinstance(model, PM.ResamplerModel):
        def rec_one(dat, count, buf):
            calls.append(("one", count, buf.size // w, dat))
            return keep(one(dat, count, buf))

        def rec_cross(dat, count, last, nxt):
            calls.append(("cross", count, last.size // w, nxt.size // w, dat))
            return keep(cross(dat, count, last, nxt))
    else:
        def rec_one(count, buf):
            calls.append(("one", count, buf.size // w))
            return keep(one(count, buf))

        def rec_cross(count, last, nxt):
            calls.append(("cross", count, last.size // w, nxt.size // w))
            return keep(cross(count, last, nxt))
    model.one, model.cross = rec_one, rec_cross
    return calls


def run_pipe(c, model, out_block):
    """-> (yielded blocks, trace) of the case's Pipe over the case's blocks."""
    if c.kind == "resampler":
        return PM.fir_resampler_pipe(model, blocks(c), out_block)
    if c.factor == 1:
        return PM.fir_filter_pipe(model, blocks(c), out_block)
    return PM.fir_decimator_pipe(model, blocks(c), out_block)
