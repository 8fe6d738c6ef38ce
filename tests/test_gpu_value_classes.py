"""GPU parity of every FIR kernel family and route on the value classes the ordinary test signals never contain: signed zeros,
subnormals, tiny and huge normals, sums that overflow, infinities and NaN in the samples, runs of byte 128 (exactly +0) in u8 IQ,
and zero / subnormal / tiny / huge taps (tests/value_classes.py).  The kernels' shortcuts are exact only for some classes -- the
padding taps a u8 kernel skips (PSKIP), the guarded walk of shorter filters, the +0 a systolic partial starts from, taps / 128
for the u8-fused kernels, the symmetric pre-add -- and this file is where each of them meets the inputs that would show it.

Expected values come from the restated Pipes (oracle/pipes_model.py) or, without seams, from the plain oracle call; never from
the device.  Float input: NaN positions must agree and everything else bit for bit (value_classes.assert_same_classes); u8 input is
finite, so there plain bit equality holds and the expected output is shown to hold no NaN.  Where a route has a launch counter it is
asserted, so no case can quietly run on another kernel.

test_expected_outputs_on_the_cpu (no GPU) computes every case's expected output, checks the cap on its NaN share and that zeros,
subnormals, infinities and NaN all occur in it, and prints the shares."""
import functools

import numpy as np
import pytest

import signals as S
import tuned_chain_model as TCM
import tuner_model as TM
import value_classes as V
from conftest import assert_bit_equal
from oracle import pipes_model as PM
from oracle.oracle import duplicate

gpu = pytest.mark.gpu

B = 8192
NBLK = 6
GAIN = 0.2
SUBNORMALS = np.array([1e-42, -3e-39, -0.0, 1.0, 0.0, -0.0, 0.70710677, -0.70710677, -1.0, 1e-45, 2.5, -0.0, 1e-30, 3.0], np.float32)
LEVELS = {0: "ordinary taps", 1: "level-1 taps", 2: "level-2 taps"}
SYS_LEVELS = {0: "positive taps", 1: "level-1 taps"}
ALL = ("zero", "subnormal", "inf", "nan")


def _split(x, width, block):
    n = x.size // width
    return [x[i * block * width:(i + 1) * block * width] for i in range(n // block)]


def _pad(taps, mult):
    t = np.asarray(taps, np.float32)
    return np.concatenate([t, np.zeros(-t.size % mult, np.float32)])


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


# ---- the FIR cases: one table for the CPU check and the GPU runs ------------------------------------------------------------------
class Case:
    """One operator on one salted stream.  kind: dec / filt / res; inp: c (cfloat) / r (real) / u8; taps: the set as the constructor
    gets it; counter: which launch counter must move ("-name": must not move)."""

    def __init__(self, name, kind, inp, taps, order=PM.ORDER_AVX, factor=1, ratio=None, sym=False, nblk=NBLK, seams=(B, 0), small=0,
                 counters=(), large=(60, 62), every=1, even_cuts=False, cuts=None, seed=1):
        self.name, self.kind, self.inp, self.taps_fn, self.order, self.factor, self.ratio = name, kind, inp, taps, order, factor, ratio
        self.sym, self.nblk, self.seams, self.small, self.counters, self.large = sym, nblk, seams, small, counters, large
        self.every, self.even_cuts, self.cuts, self.seed = every, even_cuts, cuts, seed
        self.complex = inp in ("c", "u8")
        self.width = 2 if self.complex else 1

    def __repr__(self):
        return self.name

    @property
    def taps(self):
        return self.taps_fn()

    def lp(self):
        """The longest window in input samples."""
        t = self.taps
        if self.kind == "res":
            I = self.ratio[0]
            return -(-(-(-t.size // I)) // 8) * 8
        return 2 * t.size if self.sym else -(-t.size // 8) * 8

    @functools.lru_cache(maxsize=None)
    def stream(self):
        """(what the device gets, the same as float32, segment table)"""
        n = self.nblk * B
        if self.inp == "u8":
            u8, table = V.salt_u8(S.iq_u8(n, seed=4000 + self.seed), self.lp(), self.seed, self.every)
            x = _oracle().convert_u8(u8)
            u8.setflags(write=False)
            x.setflags(write=False)
            return u8, x, table
        base = S.cfloat_block(n, seed=4100 + self.seed) if self.complex else S.real_block(n, seed=4200 + self.seed)
        x, table = V.salt(base, self.width, self.lp(), self.seed, large=self.large, every=self.every)
        x.setflags(write=False)
        return x, x, table

    def model(self):
        o = _oracle()
        if self.kind == "res":
            return PM.ResamplerModel(o, self.ratio[0], self.ratio[1], self.taps, self.order, self.complex)
        return PM.FilterModel(o, self.taps, self.order, complex_=self.complex and not self.sym, sym=self.sym, factor=self.factor)

    @functools.lru_cache(maxsize=None)
    def expected(self, seam):
        _, x, _ = self.stream()
        m = self.model()
        if self.kind == "res":
            blocks, _ = PM.fir_resampler_pipe(m, _split(x, self.width, seam) if seam else [x], 512)
        elif seam:
            blocks, _ = PM.fir_decimator_pipe(m, _split(x, self.width, seam), 1024)
        else:
            blocks = [m.one((x.size // self.width - m.num_coeffs) // self.factor + 1, x)]
        e = np.concatenate(blocks)
        e.setflags(write=False)
        return e

    def need(self):
        return ("zero",) if self.inp == "u8" else ALL

    def descriptor(self, hip):
        if self.kind == "res":
            return hip.Resampler(self.ratio[0], self.ratio[1], self.taps, self.order, self.complex)
        if self.kind == "filt":
            return hip.Filter(self.taps, self.order, complex_=self.complex, sym=self.sym)
        return hip.Decimator(self.factor, self.taps, self.order, complex_=self.complex, sym=self.sym)


def _t127(level):
    return lambda: V.awkward_taps(S.taps_decim127(), level)


def _gauss(n, seed, level, last_zero=False, sigma=0.05):
    return lambda: V.awkward_taps(S.gauss_taps(n, seed, sigma), level, last_zero)


def _cases():
    c = []
    # the complex decimator by 8 with 127 taps, AVX order (k_decimate_c4): cfloat and u8, each tap level.  Level 2 has a tap below
    # 2^-119: the u8 launch must leave the taps / 128 kernels for the generic one and still give the same bits
    for level in (0, 1, 2):
        c.append(Case(f"c4 /8 127 taps cfloat, {LEVELS[level]}", "dec", "c", _t127(level), factor=8, small=None, even_cuts=True,
                      counters=("-tiled", "-generic_u8"), seed=10 + level))
        c.append(Case(f"c4 /8 127 taps u8, {LEVELS[level]}", "dec", "u8", _t127(level), factor=8, small=None, even_cuts=True,
                      counters=("-tiled", "generic_u8" if level == 2 else "-generic_u8"), seed=20 + level))
    # all taps positive: a window of -0 samples gives only -0 products, and the output is +0 because every partial sum starts from +0
    c.append(Case("c4 /8 127 positive taps cfloat", "dec", "c", lambda: np.abs(S.taps_decim127()), factor=8, small=None, even_cuts=True,
                  counters=("-tiled", "-generic_u8"), seed=13))
    # guarded and other instantiations (level-1 taps: zero taps inside, the last one nonzero)
    for factor, ntaps in ((4, 127), (16, 127), (8, 31), (8, 52), (8, 64), (8, 128)):
        for inp in ("c", "u8"):
            taps = _t127(1) if ntaps == 127 else _gauss(ntaps, 300 + ntaps, 1)
            c.append(Case(f"c4 /{factor} {ntaps} taps {inp}, level-1 taps", "dec", inp, taps, factor=factor, even_cuts=True,
                          counters=("-tiled", "-generic_u8"), seed=30 + factor + ntaps))
    # SSE and scalar orders of the complex decimator by 8
    c.append(Case("complex /8 127 taps cfloat, SSE order", "dec", "c", _t127(1), order=PM.ORDER_SSE, factor=8, even_cuts=True, seed=40))
    c.append(Case("complex /8 127 taps cfloat, scalar order", "dec", "c", _t127(1), order=PM.ORDER_SCALAR, factor=8, even_cuts=True, seed=41))
    # real decimators (kernels_decimate_real.hip).  The large segment reaches 2^127: a pair of them overflows in the symmetric
    # kernels' pre-add x[j] + x[2N-1-j] where the plain form's products stay finite
    for order, oname in ((PM.ORDER_AVX, "AVX"), (PM.ORDER_SSE, "SSE")):
        for factor, nblk in ((2, NBLK), (8, 2 * NBLK)):          # the kernel takes launches of at least 4096 outputs: by 8, 12 blocks
            for ntaps in (37, 128):
                c.append(Case(f"real /{factor} {ntaps} taps {oname}", "dec", "r", _gauss(ntaps, 400 + ntaps, 1), order=order, factor=factor,
                              nblk=nblk, counters=("real16",), large=(126, 127), seed=50 + factor + ntaps))
            for nhalf in (24, 64):
                c.append(Case(f"real symmetric /{factor} {nhalf} half-taps {oname}", "dec", "r", _gauss(nhalf, 500 + nhalf, 1), order=order,
                              factor=factor, sym=True, nblk=nblk, counters=("real16",), large=(126, 127), every=2, seed=60 + factor + nhalf))
    # the general tiled kernels (kernels_split.hip)
    c.append(Case("split real /5 31 taps", "dec", "r", _gauss(31, 601, 1), factor=5, counters=("tiled",), seed=70))
    c.append(Case("split complex /5 31 taps", "dec", "c", _gauss(31, 602, 1), factor=5, counters=("tiled",), seed=71))
    c.append(Case("split complex filter 77 taps SSE", "filt", "c", _gauss(77, 603, 1), order=PM.ORDER_SSE, nblk=4, counters=("tiled",), seed=72))
    c.append(Case("split real filter 75 taps SSE", "filt", "r", _gauss(75, 604, 1), order=PM.ORDER_SSE, nblk=4, counters=("tiled",), seed=73))
    # the fast real filters (k_fir_real8_fast)
    c.append(Case("fast real symmetric filter 64 half-taps AVX", "filt", "r", lambda: V.awkward_taps(S.taps_audio_half64(), 1), sym=True,
                  nblk=4, counters=("-tiled", "-real16"), large=(126, 127), every=2, seed=80))
    c.append(Case("fast real symmetric filter 64 half-taps SSE", "filt", "r", lambda: V.awkward_taps(S.taps_audio_half64(), 1), sym=True,
                  order=PM.ORDER_SSE, nblk=4, counters=("-tiled", "-real16"), large=(126, 127), every=2, seed=81))
    c.append(Case("fast real filter 80 taps AVX", "filt", "r", _gauss(80, 605, 1), nblk=4, counters=("-tiled", "-real16"), seed=82))
    # the generic kernel on the short-seamed-launch route (the library's default threshold; launches of at most 16384 outputs)
    c.append(Case("generic real filter 77 taps, short seamed launches", "filt", "r", _gauss(77, 606, 1), nblk=3, seams=(B,), small=None,
                  counters=("-tiled", "-real16", "-cycle"), cuts=(4097, 12288, -4099), seed=90))
    c.append(Case("generic real resampler 3/10 191 taps, short seamed launches", "res", "r", lambda: V.awkward_taps(S.taps_resamp191(), 1),
                  ratio=(3, 10), nblk=3, seams=(B,), small=None, counters=("-tiled", "-cycle"), seed=91))
    # resamplers
    c.append(Case("resampler 3/10 191 taps real AVX", "res", "r", lambda: V.awkward_taps(S.taps_resamp191(), 1), ratio=(3, 10),
                  counters=("-tiled", "-cycle"), seed=100))
    c.append(Case("resampler 3/10 31 taps real AVX", "res", "r", lambda: V.awkward_taps(S.taps_resamp31(), 1), ratio=(3, 10),
                  counters=("-tiled", "-cycle"), seed=101))
    c.append(Case("resampler 5/7 32 taps real (thread per cycle)", "res", "r", _gauss(32, 607, 1, sigma=0.3), ratio=(5, 7), counters=("cycle",), seed=102))
    c.append(Case("resampler 3/10 150 taps complex SSE", "res", "c", _gauss(150, 608, 1, sigma=0.3), ratio=(3, 10), order=PM.ORDER_SSE,
                  counters=("tiled",), seed=103))
    c.append(Case("resampler 3/10 150 taps complex AVX", "res", "c", _gauss(150, 609, 1, sigma=0.3), ratio=(3, 10), counters=("tiled",), seed=104))
    c.append(Case("resampler 97/100 1500 taps real (more than 64 groups)", "res", "r", _gauss(1500, 610, 1, sigma=0.3), ratio=(97, 100), nblk=1,
                  seams=(0,), seed=105))
    return c


CASES = _cases()
COUNTERS = {"tiled": "sdrhip_debug_tiled_launches", "real16": "sdrhip_debug_decimate_real16_launches",
            "cycle": "sdrhip_debug_resample_cycle_launches", "generic_u8": "sdrhip_debug_generic_u8_launches",
            "crossfix": "sdrhip_debug_decimator_crossfix_launches"}


def _check_expected(case, seam):
    """The conditions on the CPU side alone: the NaN cap (u8: no NaN at all) and the classes that must occur.  -> NaN share."""
    exp = case.expected(seam)
    what = f"{case.name}, seam {seam}"
    share = V.nan_share(exp)
    assert share <= (0.0 if case.inp == "u8" else 0.10), f"{what}: NaN share {share:.3f}"
    V.assert_not_vacuous(exp, what, case.need())
    return share


# ---- systolic inputs --------------------------------------------------------------------------------------------------------------
SYS_K = 64 * 240 * 4 + 247
SYS_NBLK = 61


@functools.lru_cache(maxsize=None)
def _systolic_stream(u8, strip_outs):
    """61 blocks, the first 60 salted once per block, plus a tail in the ragged last strip (its few outputs' windows overlap, so the classes share
    them: the first output's first 8 samples subnormal -- byte 127 / 129 for u8 --, then zeros through the second output's window,
    then a NaN).  Checked here: a zero run, a subnormal run and a NaN island each lie inside a whole strip and across a strip boundary."""
    n = SYS_NBLK * B
    lp = 128
    span = 8 * strip_outs
    nstrips = -(-SYS_K // strip_outs)
    t0 = span * (nstrips - 1)
    assert t0 + 8 + 136 + 1 <= 8 * (SYS_K - 1) + lp, "the tail does not fit the last strip's samples"
    if u8:
        base = S.iq_u8(n, seed=4300)
        head, table = V.salt_u8(base[:2 * (n - B)], lp, 7)           # the last block stays ordinary around the tail
        raw = np.concatenate([head, base[2 * (n - B):]])
        v = raw.reshape(-1, 2)
        v[t0:t0 + 8] = (127, 129)
        v[t0 + 8:t0 + 144] = 128
        kinds = ("silence",)
        x = _oracle().convert_u8(raw)
    else:
        base = S.cfloat_block(n, seed=4301)
        head, table = V.salt(base[:2 * (n - B)], 2, lp, 7)
        raw = np.concatenate([head, base[2 * (n - B):]])
        v = raw.reshape(-1, 2)
        v[t0:t0 + 8] = V._bits([0x00012345, 0x80054321])
        v[t0 + 8:t0 + 144] = 0.0
        v[t0 + 144] = V._bits([0x7FC00000, 0x7FC00000])
        kinds = ("pzero", "subnormal", "nan")
        x = raw
    for kind in kinds:
        segs = [s for s in table if s["kind"] == kind and s["start"] + s["len"] <= t0]
        inside = any(s["start"] // span == (s["start"] + s["len"] + lp - 1) // span for s in segs)
        # a run covers a strip's first sample; a lone sample lies in the lp samples two strips both read
        across = any((s["start"] - 1) // span != (s["start"] + s["len"] - 1) // span if s["len"] > 1 else s["start"] % span < lp for s in segs)
        assert inside and across, f"{kind}: inside a strip {inside}, across a boundary {across}"
    raw.setflags(write=False)
    x.setflags(write=False)
    return raw, x


@functools.lru_cache(maxsize=None)
def _systolic_expected(u8, strip_outs, level, seam):
    _, x = _systolic_stream(u8, strip_outs)
    taps = _systolic_taps(strip_outs, level)
    m = PM.FilterModel(_oracle(), taps, PM.ORDER_AVX, complex_=True, factor=8)
    if seam:
        blocks, _ = PM.fir_decimator_pipe(m, _split(x, 2, seam), 61)       # the Pipe yields whole output blocks only: small ones reach past K
        e = np.concatenate(blocks)[:2 * SYS_K]
    else:
        e = m.one(SYS_K, x)
    assert e.size == 2 * SYS_K
    e.setflags(write=False)
    return e


def _systolic_taps(strip_outs, level):
    """Level 0 here: the 127 taps made positive.  A window of -0 samples then gives nothing but -0 products, and only the +0 every
    partial sum starts from makes the output +0, as in the reference (mixed-sign taps hide a partial that starts from its first product)."""
    if level == 0:
        return np.abs(S.taps_decim127())
    return V.awkward_taps(S.taps_decim127() if strip_outs == 240 else S.taps_example_rf_decim(), level)


SYSTOLIC = [(u8, 240, level, seam) for u8 in (True, False) for level in (0, 1) for seam in (0, B)] + [(True, 248, 1, seam) for seam in (0, B)]


# ---- the FM chain on u8 silence ---------------------------------------------------------------------------------------------------
CHAIN_NBLK, MODEL_NBLK = 20, 60
SHIFT = ("shift -3/1000", lambda: TM.shift_table(-3, 1000))
QUARTER = ("shift 1/4", lambda: TM.shift_table(1, 4))


def _chain_taps(level):
    return (V.awkward_taps(S.taps_decim127(), level), V.awkward_taps(S.taps_resamp191(), level), V.awkward_taps(S.taps_audio_half64(), level))


@functools.lru_cache(maxsize=None)
def _chain_stream():
    u8, table = V.salt_u8(S.iq_u8_fm(MODEL_NBLK * B), 128, 9)
    assert sum(1 for s in table if s["kind"] == "silence" and s["start"] < CHAIN_NBLK * B) >= CHAIN_NBLK - 1
    u8.setflags(write=False)
    return u8


@functools.lru_cache(maxsize=None)
def _chain_expected(level, block, osc_name):
    """The audio of the first 20 blocks' run: a prefix of the first audio block of the restated Pipes on 60 blocks (block 8192), or
    the plain oracle calls on the 20 blocks as one buffer (block 0)."""
    o = _oracle()
    u8 = _chain_stream()
    dt, rt, at = _chain_taps(level)
    osc = {None: None, SHIFT[0]: SHIFT[1], QUARTER[0]: QUARTER[1]}[osc_name]
    osc = osc() if osc else None
    if block:
        blocks = [u8[2 * i * B:2 * (i + 1) * B] for i in range(MODEL_NBLK)]
        if osc is None:
            a = PM.fm_receiver(o, blocks, dt, 8, rt, 3, 10, at, GAIN, B)
        else:
            a = TCM.fm_receiver_tuned(o, blocks, osc, dt, 8, rt, 3, 10, at, GAIN, B, PM.ORDER_AVX)
        e = np.concatenate(a)
    else:
        x = o.convert_u8(u8[:2 * CHAIN_NBLK * B])
        if osc is not None:
            x = TM.mix(x, osc, 0)
        kd = (CHAIN_NBLK * B - 128) // 8 + 1
        y = o.fm_demod(o.decimate_rc(4, kd, 8, duplicate(_pad(dt, 4)), x))
        prep = o.prepare_coeffs(8, 3, 10, rt)
        nz = (kd * 3 - 192) // 10 + 1
        z, _ = o.resample_rr(8, nz, prep, 0, y)
        e = o.scale(GAIN, o.filter_sym_rr(8, nz - 127, at, z))
    e.setflags(write=False)
    return e


CHAIN_Q1 = (((CHAIN_NBLK * B - 128) // 8 + 1) * 3 - 192) // 10 + 1 - 127


# ---- the tuner on finite classes --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tuner_stream():
    x, _ = V.salt(S.cfloat_block(NBLK * B, seed=4400), 2, 128, 11, islands=False)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _tuner_expected(which, seam):
    osc = TM.shift_table(-3, 1000) if which == "shift" else SUBNORMALS
    e = TM.tuner_expected(_oracle(), S.taps_decim127(), PM.ORDER_AVX, 8, _tuner_stream(), osc, seam, 0, block_out=1)
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def _scale_stream():
    x, _ = V.salt(S.real_block(100001, seed=4500), 1, 16, 12)
    x.setflags(write=False)
    return x


# ---- the CPU side of every case, without a GPU ------------------------------------------------------------------------------------
def test_expected_outputs_on_the_cpu(oracle):
    """Every case's expected output once, here: its NaN share under the cap (the share is printed; the worst goes into LABNOTES), and
    zeros, subnormals, infinities and NaN all in it (u8 input: zeros, and no NaN)."""
    worst = (0.0, "")
    for case in CASES:
        for seam in case.seams:
            share = _check_expected(case, seam)
            print(f"NaN share {share:.4f}  {case.name}, seam {seam}")
            worst = max(worst, (share, case.name))
    for u8, strip_outs, level, seam in SYSTOLIC:
        e = _systolic_expected(u8, strip_outs, level, seam)
        what = f"systolic {'u8' if u8 else 'cfloat'}, strips of {strip_outs}, {SYS_LEVELS[level]}, seam {seam}"
        share = V.nan_share(e)
        print(f"NaN share {share:.4f}  {what}")
        assert share <= (0.0 if u8 else 0.10)
        V.assert_not_vacuous(e, what, ("zero",) if u8 else ALL)
        tail = e[2 * strip_outs * ((SYS_K - 1) // strip_outs):][:8]
        if not u8:
            assert V.classes_present(tail) == {"zero": True, "subnormal": True, "inf": False, "nan": True}, "the ragged strip's outputs"
            worst = max(worst, (share, what))
        else:
            assert V.classes_present(tail)["zero"]
    for level in (0, 1):
        for block in (B, 0):
            for name in (None, SHIFT[0], QUARTER[0]):
                e = _chain_expected(level, block, name)
                assert e.size >= CHAIN_Q1 and not np.isnan(e).any() and np.isfinite(e[:CHAIN_Q1]).all(), (level, block, name)
    for which in ("shift", "subnormals"):
        for seam in (B, 0):
            e = _tuner_expected(which, seam)
            assert np.isfinite(e).all()
            V.assert_not_vacuous(e, f"tuner, {which} table, seam {seam}", ("zero", "subnormal"))
    x = _scale_stream()
    exps = [oracle.scale(f, x) for f in V.SCALE_FACTORS]
    for f, e in zip(V.SCALE_FACTORS, exps):
        share = V.nan_share(e)
        print(f"NaN share {share:.4f}  scale by {f!r}")
        assert share <= 0.10
        worst = max(worst, (share, f"scale by {f!r}"))
    V.assert_not_vacuous(np.concatenate(exps), "scale, all factors")
    print(f"worst NaN share {worst[0]:.4f}: {worst[1]}")


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _dev():
    import gpu_util
    return gpu_util


def _run(desc, d_in, width, K, seam, cuts=(), u8=False, out_block=0):
    G = _dev()
    out = G.dev_empty_f32(K * width)
    edges = sorted(set([0] + [c for c in cuts if 0 < c < K] + [K]))
    kw = {"out_block": out_block} if out_block else {}
    for a, b in zip(edges[:-1], edges[1:]):
        (desc.run_u8 if u8 else desc.run)(G.ptr(d_in), 0, G.ptr(out) + 4 * width * a, a, b, seam, **kw)
    return G.to_host(out)


def _compare(case_is_u8, got, exp, what):
    if case_is_u8:
        assert not np.isnan(exp).any(), what
        assert_bit_equal(got, exp, what)
    else:
        V.assert_same_classes(got, exp, what)


def _counts(hip):
    return {k: int(getattr(hip.lib, f)()) for k, f in COUNTERS.items()}


def _fir_case_on_the_device(hip, case, small):
    G = _dev()
    prev = hip.set_small_launch_outputs(small) if small is not None else None
    try:
        raw, _, _ = case.stream()
        d_in = G.to_dev(raw)
        desc = case.descriptor(hip)
        u8 = case.inp == "u8"
        for seam in case.seams:
            _check_expected(case, seam)
            exp = case.expected(seam)
            K = exp.size // case.width
            ob = 512 if case.kind == "res" else 0
            before = _counts(hip)
            got = _run(desc, d_in, case.width, K, seam, (), u8, ob)
            after = _counts(hip)
            _compare(u8, got, exp, f"{case.name}, seam {seam}: one launch")
            cuts = [4098, (K - 4100) // 2 * 2] if case.even_cuts else [4097, K - 4099]    # even: 16-byte output starts keep a launch on k_decimate_c4
            if case.cuts:
                cuts = [c if c > 0 else K + c for c in case.cuts]
                one_launch_counts = False
            else:
                one_launch_counts = True
            before2 = _counts(hip)
            got = _run(desc, d_in, case.width, K, seam, cuts, u8, ob)
            after2 = _counts(hip)
            _compare(u8, got, exp, f"{case.name}, seam {seam}: cut at {cuts}")
            for name in case.counters:
                must, key = not name.startswith("-"), name.lstrip("-")
                pairs = [(before2, after2)] + ([(before, after)] if one_launch_counts else [])
                for b, a in pairs:
                    moved = a[key] - b[key]
                    assert (moved > 0) == must, f"{case.name}, seam {seam}: {COUNTERS[key]} moved by {moved}"
            if case.kind == "dec" and case.complex and case.order == PM.ORDER_AVX and case.factor in (4, 8, 16) and seam and small is not None \
                    and "generic_u8" not in case.counters:
                # the seam fix-up as a launch of its own exactly when the tile kernel does not compute the Cross outputs in place
                assert (after["crossfix"] - before["crossfix"] == 1) == (small == 0), f"{case.name}: fix-up launches, threshold {small}"
    finally:
        if prev is not None:
            hip.set_small_launch_outputs(prev)


def _ids(cases):
    return [c.name for c in cases]


C4_MAIN = [c for c in CASES if c.small is None and c.name.startswith("c4")]
OTHERS = [c for c in CASES if c not in C4_MAIN]


@gpu
@pytest.mark.parametrize("route", ["Cross outputs in the tile kernel", "tile kernel + fix-up launch"])
@pytest.mark.parametrize("case", C4_MAIN, ids=_ids(C4_MAIN))
def test_complex_decimator_by_8(hip, oracle, case, route):
    """k_decimate_c4 on cfloat (0 * Inf of the padding tap must be NaN) and on u8 (the padding tap's MACs are skipped; level-2 taps
    leave the taps / 128 kernels), under both settings of the short-seamed-launch threshold."""
    _fir_case_on_the_device(hip, case, -1 if route.startswith("Cross") else 0)


@gpu
@pytest.mark.parametrize("case", OTHERS, ids=_ids(OTHERS))
def test_fir_families(hip, oracle, case):
    """Guarded and exact-length instantiations, the other lane orders, the real decimators (plain and symmetric), the general tiled
    kernels, the fast real filters, the generic kernel on short seamed launches, and the resamplers."""
    _fir_case_on_the_device(hip, case, case.small)


@gpu
@pytest.mark.parametrize("u8,strip_outs,level,seam", SYSTOLIC)
def test_systolic_decimator(hip, oracle, u8, strip_outs, level, seam):
    """The register-resident kernel on whole strips, strip boundaries and the ragged last strip: against the oracle, and byte for
    byte (NaN payloads included: both are this GPU) against the tile kernel on the same launch."""
    G = _dev()
    import torch
    raw, _ = _systolic_stream(u8, strip_outs)
    exp = _systolic_expected(u8, strip_outs, level, seam)
    dec = hip.Decimator(8, _systolic_taps(strip_outs, level), hip.ORDER_AVX, complex_=True)
    d_in = G.to_dev(raw)
    prev = hip.set_small_launch_outputs(0)                   # seamed launches of this size: the fix-up outside the tile kernel
    mode = 1 if strip_outs == 240 else 2                     # the 64-tap instantiation is the library's own choice only
    outs = []
    try:
        for m in (mode, 0):
            hip.lib.sdrhip_debug_set_systolic(m)
            before = hip.lib.sdrhip_debug_systolic_launches()
            out = G.dev_empty_f32(2 * SYS_K)
            (dec.run_u8 if u8 else dec.run)(G.ptr(d_in), 0, G.ptr(out), 0, SYS_K, seam)
            torch.cuda.synchronize()
            assert hip.lib.sdrhip_debug_systolic_launches() - before == (1 if m else 0), f"set_systolic({m}): wrong kernel"
            outs.append(G.to_host(out))
    finally:
        hip.lib.sdrhip_debug_set_systolic(2)
        hip.set_small_launch_outputs(prev)
    what = f"systolic {'u8' if u8 else 'cfloat'}, strips of {strip_outs}, {SYS_LEVELS[level]}, seam {seam}"
    _compare(u8, outs[0], exp, what)
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), what + ": differs from the tile kernel"


@gpu
def test_fm_demod_fed_by_the_decimator_on_silence(hip, oracle):
    """sdrhip_fm_demod_run on the decimator's device output for the u8 silence stream: exact +0 pairs and the sums next to them."""
    G = _dev()
    case = next(c for c in CASES if c.name == "c4 /8 127 taps u8, ordinary taps")
    raw, x, _ = case.stream()
    m = case.model()
    blocks, _ = PM.fir_decimator_pipe(m, _split(x, 2, B), 1024)
    exp = np.concatenate(PM.fm_demod_pipe(oracle, blocks))
    K = exp.size
    assert not np.isnan(exp).any() and (np.concatenate(blocks).reshape(-1, 2) == 0).all(axis=1).sum() >= 16, "no silent decimated samples"
    d = G.dev_empty_f32(2 * K)
    case.descriptor(hip).run_u8(G.ptr(G.to_dev(raw)), 0, G.ptr(d), 0, K, B)
    y = G.dev_empty_f32(K)
    hip.check(hip.lib.sdrhip_fm_demod_run(None, G.ptr(d), 0, G.ptr(y), 0, K, 0.0, 0.0), "sdrhip_fm_demod_run")
    assert_bit_equal(G.to_host(y), exp, "fmDemod of the decimated silence stream")


def _chain_run(hip, ch, d_in, total, q1):
    import torch
    G = _dev()
    wsb = ch.workspace_bytes(total)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = G.dev_empty_f32(q1)
    ch.run(G.ptr(d_in), 0, total, G.ptr(out), 0, q1, G.ptr(ws), wsb)
    return G.to_host(out)


@gpu
@pytest.mark.parametrize("block", [B, 0])
@pytest.mark.parametrize("level", [0, 1])
def test_fm_chain_on_silence(hip, oracle, level, block):
    """20 blocks of FM-modulated u8 IQ with silent stretches (and runs of 0, 255, 127 / 129): the plain chain, the tuned chain and a
    2-station bank, on the one-kernel route and the stage route, against the restated Pipes and each other.  All finite: bit equality."""
    import torch
    G = _dev()
    total = CHAIN_NBLK * B
    d_in = G.to_dev(_chain_stream()[:2 * total])
    dt, rt, at = _chain_taps(level)
    tuned = {}
    for name, osc in ((None, None), (SHIFT[0], SHIFT[1]()), (QUARTER[0], QUARTER[1]())):
        exp = _chain_expected(level, block, name)[:CHAIN_Q1]
        assert not np.isnan(exp).any()
        ch = hip.FmChain(8, dt, 3, 10, rt, at, GAIN, block)
        if osc is not None:
            ch.set_tuner(osc)
        q0, q1, _ = ch.plan(0, total, total)
        assert (q0, q1) == (0, CHAIN_Q1)
        got = {}
        for route in ("small", "stage"):
            ch.set_small_chain(1 if route == "small" else 0)
            ch.set_fused_tail(0)
            n0 = hip.lib.sdrhip_debug_small_chain_launches()
            got[route] = _chain_run(hip, ch, d_in, total, q1)
            assert hip.lib.sdrhip_debug_small_chain_launches() - n0 == (1 if route == "small" else 0), f"{route} route: wrong kernel"
            assert_bit_equal(got[route], exp, f"{name or 'untuned'} chain, {LEVELS[level]}, block {block}, {route} route vs the CPU side")
        assert_bit_equal(got["small"], got["stage"], "one-kernel route vs stage route")
        tuned[name] = got["small"]
    bank = hip.FmBank(8, dt, 3, 10, rt, at, [SHIFT[1](), QUARTER[1]()], GAIN, block)
    bank.set_route(1)
    b0 = hip.fm_bank_launches()
    out = G.dev_empty_f32(2 * CHAIN_Q1)
    wsb = bank.workspace_bytes(total)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    bank.run(G.ptr(d_in), 0, total, G.ptr(out), CHAIN_Q1, 0, CHAIN_Q1, G.ptr(ws), wsb)
    rows = G.to_host(out).reshape(2, CHAIN_Q1)
    assert hip.fm_bank_launches() == b0 + 1, "one banked launch"
    assert_bit_equal(rows[0], tuned[SHIFT[0]], "bank station 0 vs its tuned chain")
    assert_bit_equal(rows[1], tuned[QUARTER[0]], "bank station 1 vs its tuned chain")


@gpu
@pytest.mark.parametrize("seam", [B, 0])
@pytest.mark.parametrize("which", ["shift", "subnormals"])
def test_tuner_on_finite_classes(hip, oracle, which, seam):
    """The tuner's header excludes non-finite input: the finite classes only, fused and two-pass routes, plain bit equality."""
    G = _dev()
    x = _tuner_stream()
    exp = _tuner_expected(which, seam)
    assert np.isfinite(exp).all()
    osc = TM.shift_table(-3, 1000) if which == "shift" else SUBNORMALS
    t = hip.Tuner(8, S.taps_decim127(), osc)
    K = exp.size // 2
    d_in = G.to_dev(x)
    for route in (hip.TUNER_ROUTE_FUSED, hip.TUNER_ROUTE_TWO_PASS):
        t.set_route(route)
        c0 = hip.tuner_fused_launches()
        got = _run(t, d_in, 2, K, seam, [4098, K - 4100])
        assert (hip.tuner_fused_launches() - c0 == 3) == (route == hip.TUNER_ROUTE_FUSED), f"route {route}: wrong kernel"
        assert_bit_equal(got, exp, f"tuner, {which} table, seam {seam}, route {route}")


@gpu
def test_scale(hip, oracle):
    G = _dev()
    x = _scale_stream()
    d_in = G.to_dev(x)
    for f in V.SCALE_FACTORS:
        exp = oracle.scale(f, x)
        out = G.dev_empty_f32(x.size)
        hip.check(hip.lib.sdrhip_scale_run(None, f, G.ptr(d_in), G.ptr(out), x.size), "sdrhip_scale_run")
        V.assert_same_classes(G.to_host(out), exp, f"sdrhip_scale_run by {f!r}")
        for sym in ("scale", "scaleSSE", "scaleAVX"):
            V.assert_same_classes(hip.DropIn.scale(sym, f, x), exp, f"{sym} by {f!r}")


@gpu
def test_convert_tx(hip, ref):
    """convertBladeRFTransmit: the restatement where the C cast is defined; where it is undefined behaviour, the answer of the x86
    build of the reference (live or recorded), which is what the kernel claims to give."""
    defined, wild = V.convert_tx_inputs()
    got = hip.DropIn.convert_tx(defined)
    assert got.dtype == np.int16
    assert_bit_equal(got, V.convert_tx_spec(defined), "convertBladeRFTransmit where the cast is defined")
    assert_bit_equal(hip.DropIn.convert_tx(wild), ref.convert_tx(wild), "convertBladeRFTransmit on +-1e6, +-3e9, +-Inf, NaN")
