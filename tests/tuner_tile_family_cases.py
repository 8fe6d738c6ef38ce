"""The table behind tests/test_gpu_tuner_tile_family.py: the tuner tile kernels -- k_tuner_c4 and k_tuner_bank_c4 in its three output
forms -- on EVERY (factor, prepared length) their host predicate admits (tuner_fused_fits, kernels_tuner.hip: decimation 4 / 8 / 16,
a multiple of 4 taps in [8, 128], more taps than the factor: 31 + 30 + 28 = 89 shapes), on three seams and three input formats.  No
pytest in here: tests/test_tuner_tile_family_cases.py shows on the CPU, from the models alone, what the table reaches.

Taps.  (D, P) -> P seeded standard-normal coefficients / sqrt(n) (narrow_bank_cases._seeded_taps; seed 1000 D + P): every tap carries
weight.  For one length per branch of the dispatch (PADDED) also P - 1 and P - 3 coefficients: mkDecimatorC's zero padding under a
guarded walk.

Stream.  N = 2 OUTS + 77 outputs: a ragged third tile for both tile advances (OUTS, and OUTS - 2 of the fmDemod form).  Slices of
test_gpu_tuner.stream_u8() and tuner_i16_cases.stream_i16() from sample 0; cfloat input is oracle.convert_u8 of the u8 slice.

Channels.  Four: period 1000, the centre, the period-7 table of subnormals and signed zeros, period 5.  (510 D is a multiple of 5, so
period 5 meets every fmDemod-form tile at phase 0; 7 and 1000 divide no advance of either form, 5 none of the other two forms.)

Seams.  0: one buffer.  tight = ceil(P / D) D: one One output a buffer, every other output Cross; a tile spans many buffers.  wide =
the smallest multiple of D that is >= OUTS D + P: the launcher's in-tile condition holds, two seams in the stream -- the first behind
the first tile, so the Cross outputs lie in the second and third tiles of a launch from 0.

Expected rows come from tests/tuner_model.py alone (the restated firDecimator Pipe on the mixed stream), the envelope from
am_bank_cases.envelope, the phase from nfm_bank_cases.demod.  Each is computed once, cached and read-only; no device run is a source of
expected values.  TEST INFRASTRUCTURE ONLY."""
import os
import re

import numpy as np

import am_bank_cases as AC
import narrow_bank_cases as NBC
import nfm_bank_cases as NC
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from oracle import pipes_model as PM

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_amd", "csrc")

FACTORS = (4, 8, 16)
LENGTHS = tuple(range(8, 129, 4))
SHAPES = tuple((d, p) for d in FACTORS for p in LENGTHS if p > d)
FORMATS = AC.FORMATS                             # cf32, u8, i16
FORMS = ("iq", "env", "fm")

# name -> (D, TC, GUARD) of the instantiation launch_tuner_bank_c4_shape / launch_tuner_c4_shape pick
BRANCHES = {"D4": (4, 4, True), "D16/8": (16, 8, True), "D16/4": (16, 4, True), "D8 exact": (8, 8, False), "D8/8": (8, 8, True),
            "D8/4": (8, 4, True)}


def branch(d, p):
    """The dispatch rule of launch_tuner_bank_c4_shape, restated (tests/test_tuner_tile_family_cases.py holds it to the source)."""
    if d == 4:
        return "D4"
    if d == 16:
        return "D16/8" if p % 8 == 0 else "D16/4"
    if p == 128:
        return "D8 exact"
    return "D8/8" if p % 8 == 0 else "D8/4"


def admitted(d, p):
    """tuner_fused_fits' condition on the shape."""
    return d in (8, 4, 16) and 8 <= p <= 128 and p % 4 == 0 and p > d


# one length per branch that also runs with P - 1 and P - 3 coefficients, and on routes 2 and 0
PADDED = {"D4": 20, "D16/8": 40, "D16/4": 36, "D8 exact": 128, "D8/8": 24, "D8/4": 28}
PADDED_SHAPES = tuple((BRANCHES[b][0], p) for b, p in PADDED.items())
# (D, P, coefficients)
TAP_SETS = tuple((d, p, p) for d, p in SHAPES) + tuple((d, p, p - z) for d, p in PADDED_SHAPES for z in (1, 3))

OUTS = AC.tile_outputs()
ADV = NC.tile_advance()
assert ADV is not None and 0 < ADV < OUTS
N = 2 * OUTS + 77
SEAM_NAMES = ("none", "tight", "wide")

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def advance(form):
    return ADV if form == "fm" else OUTS


def tile_ranges(form):
    """The output ranges the three tiles of a launch of N outputs from 0 store."""
    a = advance(form)
    return [(0, a), (a, 2 * a), (2 * a, N)]


def taps(d, p, n=None):
    n = p if n is None else n
    return _frozen(("taps", d, p, n), lambda: NBC._seeded_taps(n, 1000 * d + p))


def tables():
    return _frozen("tables", lambda: tuple(BC.bank_tables(3)) + (T.osc_table(5),))


def seams(d, p):
    """(0, tight, wide)"""
    need = OUTS * d + p
    return (0, -(-p // d) * d, -(-need // d) * d)


def in_tile_condition(d, p, seam):
    """launch_tuner_bank_c4 / launch_tuner_c4: the Cross outputs of OUT_IQ / OUT_ENV may be computed in the tile (a tile spans less than
    one buffer)."""
    return seam >= OUTS * d + p


def n_samples(d, p, seam=0):
    """Samples the stream's N outputs read -- for the model with a seam: whole buffers of it (the Pipe yields nothing from a rest
    shorter than the filter; the device reads only the first (N - 1) D + P of them)."""
    n = (N - 1) * d + p
    return n if seam == 0 else -(-n // seam) * seam


def stream(fmt):
    """The whole seeded stream of a format; every shape reads a slice from sample 0."""
    return IC.stream_i16() if fmt == "i16" else T.stream_u8()


def converted(oracle, fmt, nsamp):
    src = stream(fmt)[:2 * nsamp]
    return (oracle.convert_i16 if fmt == "i16" else oracle.convert_u8)(src)


def expected_iq(oracle, d, p, n, channel, seam, fmt):
    """The channel's N complex outputs; cfloat input IS the converted u8, so it shares the u8 row."""
    i16 = fmt == "i16"

    def make():
        ns = n_samples(d, p, seam)
        assert ns <= stream(fmt).size // 2
        e = TM.tuner_expected(oracle, taps(d, p, n), PM.ORDER_AVX, d, converted(oracle, fmt, ns), tables()[channel], seam, 0, block_out=1)
        assert e.size >= 2 * N, (d, p, n, seam, e.size)
        return e[:2 * N].copy()
    return _frozen(("iq", d, p, n, channel, seam, i16), make)


def expected(oracle, form, d, p, n, channel, seam, fmt):
    """The channel's row in an output form, over the whole stream (fmDemod from the state (0, 0))."""
    if form == "iq":
        return expected_iq(oracle, d, p, n, channel, seam, fmt)
    fn = AC.envelope if form == "env" else (lambda iq: NC.demod(oracle, iq))
    return _frozen((form, d, p, n, channel, seam, fmt == "i16"), lambda: fn(expected_iq(oracle, d, p, n, channel, seam, fmt)))


def fm_state_before(oracle, d, p, n, channel, seam, fmt, k):
    """The fmDemod form's state in front of output k: the complex row's pair k - 1; (0, 0) in front of the stream."""
    if k == 0:
        return np.zeros(2, np.float32)
    return expected_iq(oracle, d, p, n, channel, seam, fmt)[2 * (k - 1):2 * k]


def cross_outputs(d, p, seam):
    return BC.straddlers(seam, N, p, d) if seam else np.zeros(0, np.int64)


def cuts(d, p, seam, fmt, form):
    """The cut run's two cuts.  The first: ON the first Cross output where the seam has one (33 where it has none) -- the second launch
    starts all-Cross at the tight seam, and at a residue inside its buffer at the wide one.  The second: one output past the second
    tile start of the launch that begins at the first cut (tiles count from a launch's first output).  u8 at factor 4 moves 8 bytes an
    output: an odd cut breaks the 16-byte alignment of the launch's first window, which route 1 rightly refuses -- both move to the next
    even output."""
    cr = cross_outputs(d, p, seam)
    c1 = int(cr[0]) if cr.size else 33
    c2 = c1 + advance(form) + 1
    if fmt == "u8" and d == 4:
        c1, c2 = c1 + c1 % 2, c2 + c2 % 2
    assert 0 < c1 < c2 < N
    return (c1, c2)


def launches(d, p, seam, fmt, form, cut):
    """[(k_begin, k_end)] of the one run or of the cut run."""
    edges = (0,) + (cuts(d, p, seam, fmt, form) if cut else ()) + (N,)
    return list(zip(edges[:-1], edges[1:]))


def has_seam(d, p, seam, k0, k1):
    """kernels.hpp's seam_span: a buffer boundary strictly inside the samples the launch [k0, k1) reads."""
    if seam == 0 or k1 <= k0:
        return False
    v_lo, v_hi = k0 * d, (k1 - 1) * d + p
    return (v_hi - 1) // seam >= v_lo // seam + 1


def fixup_launches(d, p, seam, ranges, in_tile_allowed):
    """Fix-up launches of OUT_IQ / OUT_ENV over these launches: one for every launch that reads across a boundary, unless its Cross
    outputs are computed in the tile (the default small_launch_outputs allows that for every launch this short; 0 never does)."""
    inl = in_tile_allowed and in_tile_condition(d, p, seam)
    return 0 if inl else sum(has_seam(d, p, seam, a, b) for a, b in ranges)


def dispatch_lines(name):
    """The five dispatch lines of launch_tuner_bank_c4_shape (name "tuner_bank") or launch_tuner_c4_shape ("tuner"), read from the code:
    [(condition, (D, TC, GUARD))] in the order they are tested.  A tree whose lines this pattern no longer matches must fail loudly."""
    src = open(os.path.join(CSRC, f"kernels_{name}.hip")).read()
    mac = "TUNER_BANK" if name == "tuner_bank" else "TUNER"
    call = mac + r"\((\d+), (\d+), (true|false)\);"
    pat = (r"    if \((g\.D == 4)\) " + call + r"\n"
           r"    else if \((g\.D == 16)\) \{ if \((P % 8 == 0)\) " + call + r" else " + call + r" \}\n"
           r"    else if \((P == 128)\) " + call + r"[^\n]*\n"
           r"    else if \((P % 8 == 0)\) " + call + r"\n"
           r"    else " + call + r"\n")
    m = re.search(pat, src)
    assert m is not None, f"kernels_{name}.hip: the dispatch lines were not found: update this pattern and branch()"
    g = m.groups()
    inst = lambda i: (int(g[i]), int(g[i + 1]), g[i + 2] == "true")                         # noqa: E731
    return [((g[0],), inst(1)), ((g[4], g[5]), inst(6)), ((g[4], "!" + g[5]), inst(9)), ((g[12],), inst(13)), ((g[16],), inst(17)),
            ((), inst(20))]


_COND = {"g.D == 4": lambda d, p: d == 4, "g.D == 16": lambda d, p: d == 16, "P % 8 == 0": lambda d, p: p % 8 == 0,
         "!P % 8 == 0": lambda d, p: p % 8 != 0, "P == 128": lambda d, p: p == 128}


def dispatched(lines, d, p):
    """The instantiation the source's lines pick for a shape: the first whose conditions hold (factor 16 is settled inside its braces:
    one of its two lines always holds)."""
    for conds, inst in lines:
        if all(_COND[c](d, p) for c in conds):
            return inst
    raise AssertionError((d, p))
