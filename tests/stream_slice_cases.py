"""The table behind tests/test_gpu_stream_slices.py: one case per branch of fir_run / resamp_run_demod
(sdr_amd/csrc/abi_device.cpp), and the helper that runs a case on a SLICE of its stream placed far from the stream's start.
No pytest in here: tests/test_stream_slice_cases.py shows on the CPU that the table reaches what it is there for.

The translation rule.  The seam rule of kernels.hpp (is_cross, seam_has_crossover, late_output_is_one) and the resampler's
phase (in_offset, group) are periodic in the stream position: for a stage with interpolation I, decimation D (coprime), seam
block B and output block outB (1 where it is unbounded), an input shift S = n D B outB moves the outputs by T = S I / D, a
multiple of I (same groups), of outB (same output blocks) and, times D, of B I (same seams), with
in_offset(m + T) = in_offset(m) + S.  So the launch (in_base + S, k_begin + T, k_end + T) on the SAME buffer must give, bit
for bit, the outputs [k_begin, k_end) of the restated Pipe (oracle/pipes_model.py) on the stream that starts at 0.  Every
expected value is that Pipe's output on the near stream; nothing is taken from the device.

What the device buffer holds: exactly the inputs include/sdr_hip.h makes the caller guarantee, from the first window's first
input to the last window's end, inside a larger tensor with GUARD elements on either side.  Float guards are NaN, byte guards
the true stream's bytes XOR 0x80 (0x7f where the stream has none): a guard element that reaches an output breaks bit equality.
"""
import contextlib
import dataclasses
from typing import Callable, Tuple

import numpy as np

from oracle import pipes_model as PM
import signals as S

B = 8192
GUARD = 4096            # stream elements of guard on either side of a slice: vector loads that round down or run ahead stay inside
AVX, SSE, SCALAR = PM.ORDER_AVX, PM.ORDER_SSE, PM.ORDER_SCALAR


# ---- the seam rule of sdr_amd/csrc/kernels.hpp, restated on int64 arrays -------------------------------------------------
def in_offset(m, I, D):
    """First input element of stream output m (descriptors.hpp ResampDesc::in_offset; m D for filters / decimators)."""
    return -((-np.asarray(m, np.int64) * D) // I)


def seam_has_crossover(edge, I, D, Lp):
    edge = np.asarray(edge, np.int64)
    if I == 1:
        return np.ones(edge.shape, bool)
    m_star = np.where(edge >= Lp, (edge - Lp) // D + 1, 0)
    first_in = (m_star * D + I - 1) // I
    return first_in * I < edge


def late_output_is_one(m, edge, I, D, out_block):
    m = np.asarray(m, np.int64)
    if I == 1 or out_block <= 0:
        return np.zeros(m.shape, bool)
    first_in = (m * D + I - 1) // I
    return (m % out_block == 0) & (first_in * I >= edge)


def is_cross(m, I, D, Lp, seam, out_block):
    """Is stream output m computed in the sequential order (kernels.hpp is_cross, seam_block = seam > 0)?"""
    m = np.asarray(m, np.int64)
    seam_bi = seam * I
    v = m * D
    edge = (v // seam_bi + 1) * seam_bi
    return (v + Lp > edge) & ~late_output_is_one(m, edge, I, D, out_block) & seam_has_crossover(edge, I, D, Lp)


def input_range(I, D, Lp, a, b):
    """Inputs the caller of a launch of outputs [a, b) guarantees: from the first window's first input to the last window's end
    (a resampler's One output walks the Lp / I floats of a group row)."""
    return int(in_offset(a, I, D)), int(in_offset(b - 1, I, D)) + Lp // I


# ---- the table ------------------------------------------------------------------------------------------------------------
COUNTERS = {
    "tiled": "sdrhip_debug_tiled_launches",                  # kernels_split.hip
    "real16": "sdrhip_debug_decimate_real16_launches",       # kernels_decimate_real.hip
    "cycle": "sdrhip_debug_resample_cycle_launches",         # kernels_resample_cycle.hip
    "systolic": "sdrhip_debug_systolic_launches",            # kernels_systolic.hip
    "crossfix": "sdrhip_debug_decimator_crossfix_launches",  # the seam fix-up of launch_decimate_c4_fast as a launch of its own
    "generic_u8": "sdrhip_debug_generic_u8_launches",        # u8 launches no u8-fused tiled kernel took
}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str                     # "filter" | "decimator" | "resampler"
    taps: Callable[[], np.ndarray]
    order: int = AVX
    complex_: bool = False
    sym: bool = False
    u8: bool = False
    I: int = 1
    D: int = 1
    seam: int = B                   # the seam block: input blocks of the Pipe
    pipe_out: int = 1024            # the Pipe's output block size
    out_block: int = 0              # what the launch is told of it (resamplers; 0 for filters / decimators, where nothing depends on it)
    nblk: int = 6                   # the near stream: nblk blocks of `seam` elements
    small: int = 0                  # sdrhip_set_small_launch_outputs while the case runs: 0 = tiled kernels + seam launch, -1 = the default
    systolic: bool = False          # sdrhip_debug_set_systolic(1) while the case runs
    min_launch: int = 0             # outputs a launch needs to take the route
    route_seams: int = 1            # input blocks the route launch covers (two where the first boundary has no Cross outputs)
    span: int = 0                   # cap on the outputs of one run (0: the whole stream), for routes that only short launches take
    moves: Tuple[str, ...] = ()     # counters that the route launch must move ...
    still: Tuple[str, ...] = ()     # ... and must leave alone (where the route has no counter of its own, this is what shows
                                    # that no fallback with a counter took the launch)
    seed: int = 1

    @property
    def width(self):
        return 2 if self.complex_ else 1

    @property
    def shift_out_block(self):
        """outB of the translation rule: the output block where the seam rule looks at it, else 1."""
        return self.out_block if self.out_block > 0 else 1

    def make(self, hip):
        if self.family == "filter":
            return hip.Filter(self.taps(), self.order, complex_=self.complex_, sym=self.sym)
        if self.family == "decimator":
            return hip.Decimator(self.D, self.taps(), self.order, complex_=self.complex_, sym=self.sym)
        return hip.Resampler(self.I, self.D, self.taps(), self.order, self.complex_)

    def model(self, oracle):
        if self.family == "resampler":
            return PM.ResamplerModel(oracle, self.I, self.D, self.taps(), self.order, self.complex_)
        return PM.FilterModel(oracle, self.taps(), self.order, complex_=self.complex_, sym=self.sym, factor=self.D)

    def pipe(self, model, blocks):
        if self.family == "resampler":
            return PM.fir_resampler_pipe(model, blocks, self.pipe_out)
        return PM.fir_decimator_pipe(model, blocks, self.pipe_out)


def _g(n, seed):
    return lambda: S.gauss_taps(n, seed)


_NO_FALLBACK = ("tiled", "generic_u8")

CASES = [
    # ---- complex FIR -------------------------------------------------------------------------------------------------------
    # launch_decimate_c4_fast has no counter of its own: the fallbacks' counters stand still, and `crossfix` tells its two seam forms apart
    Case("c4 /8 cfloat, Cross in the tile kernel", "decimator", S.taps_decim127, complex_=True, D=8, small=-1,
         still=_NO_FALLBACK + ("crossfix",)),
    Case("c4 /8 u8, Cross in the tile kernel", "decimator", S.taps_decim127, complex_=True, u8=True, D=8, small=-1,
         still=_NO_FALLBACK + ("crossfix",)),
    Case("c4 /8 cfloat, fix-up launch", "decimator", S.taps_decim127, complex_=True, D=8, small=0,
         moves=("crossfix",), still=_NO_FALLBACK),
    Case("c4 /8 u8, fix-up launch", "decimator", S.taps_decim127, complex_=True, u8=True, D=8, small=0,
         moves=("crossfix",), still=_NO_FALLBACK),
    Case("c4 /4 cfloat (guarded 128-tap kernel)", "decimator", _g(77, 44), complex_=True, D=4, small=0,
         moves=("crossfix",), still=_NO_FALLBACK),
    # at the default scale, yet a fix-up launch: a tile of 512 outputs by 16 spans more than one 8192-sample block, so the tile kernel
    # cannot decide the Cross outputs itself (decimate_tile.hpp launch_c4)
    Case("c4 /16 u8 (guarded, 124 taps)", "decimator", _g(121, 45), complex_=True, u8=True, D=16, small=-1,
         moves=("crossfix",), still=_NO_FALLBACK),
    # the systolic walk: shape and strip cut of test_gpu_systolic.test_seamed_stream_cut_into_launches (seamed launches of up to
    # 5 * 32768 outputs stay on the tile kernel, so the stream is 240 blocks)
    Case("systolic /8 u8", "decimator", S.taps_decim127, complex_=True, u8=True, D=8, small=-1, systolic=True, nblk=240,
         pipe_out=4096, moves=("systolic",), still=_NO_FALLBACK),
    Case("systolic /8 cfloat", "decimator", S.taps_decim127, complex_=True, D=8, small=-1, systolic=True, nblk=240,
         pipe_out=4096, moves=("systolic",), still=_NO_FALLBACK),
    # launch_decimate_c_orders_fast, launch_filter_c4_tile, launch_filter_cplx4_fast: no counters of their own
    Case("c_orders /8 SSE cfloat", "decimator", S.taps_decim127, order=SSE, complex_=True, D=8, still=_NO_FALLBACK),
    Case("filter_c4_tile, 128 taps", "filter", _g(128, 428), complex_=True, pipe_out=4096, min_launch=16384, still=_NO_FALLBACK),
    Case("filter_cplx4_fast, 76 taps", "filter", _g(76, 376), complex_=True, still=_NO_FALLBACK),
    Case("fir_split complex /5, 31 taps", "decimator", _g(31, 36), complex_=True, D=5, min_launch=4096, moves=("tiled",)),
    # the generic kernels (launch_fir_cplx has no counter: the scalar order has no tiled kernel, kernels_split.hip real_order / cplx_order)
    Case("generic complex scalar /3 cfloat", "decimator", _g(77, 3), order=SCALAR, complex_=True, D=3, still=_NO_FALLBACK),
    Case("generic complex scalar /3 u8", "decimator", _g(77, 3), order=SCALAR, complex_=True, u8=True, D=3,
         moves=("generic_u8",), still=("tiled",)),
    # ---- real FIR ----------------------------------------------------------------------------------------------------------
    # a short seamed launch (<= 16384 outputs at the default scale) is the generic kernel's: no counter, the tiled ones stand still
    Case("short seamed real filter (generic kernel)", "filter", _g(77, 5), small=-1, span=12000, still=("tiled", "real16")),
    # launch_fir_real8_fast: no counter of its own
    Case("real8_fast symmetric AVX, 64 half-taps", "filter", S.taps_audio_half64, sym=True, still=("tiled", "real16")),
    Case("real8_fast SSE, 77 taps", "filter", _g(77, 5), order=SSE, still=("tiled", "real16")),
    Case("real16 /2 AVX", "decimator", _g(77, 91), D=2, min_launch=4096, moves=("real16",), still=("tiled",)),
    Case("real16 /16 symmetric SSE", "decimator", _g(64, 240), order=SSE, sym=True, D=16, nblk=20, min_launch=4096,
         moves=("real16",), still=("tiled",)),
    Case("fir_split real /5 SSE", "decimator", _g(31, 36), order=SSE, D=5, min_launch=4096, moves=("tiled",), still=("real16",)),
    Case("generic real scalar /7", "decimator", _g(77, 7), order=SCALAR, D=7, still=("tiled", "real16")),
    # ---- resamplers (out_block 512; two at 97, so that late_output_is_one meets a T that is no power of two) ----------------
    # launch_resample_3_10_fast / launch_resample3c_fast: no counters of their own
    Case("resample_3_10_fast real AVX", "resampler", S.taps_resamp191, I=3, D=10, pipe_out=512, out_block=512,
         still=("tiled", "cycle", "real16")),
    Case("resample_3_10_fast real SSE", "resampler", S.taps_resamp191, order=SSE, I=3, D=10, pipe_out=512, out_block=512,
         still=("tiled", "cycle", "real16")),
    Case("resample3c_fast complex AVX", "resampler", S.taps_resamp191, complex_=True, I=3, D=10, pipe_out=512, out_block=512,
         still=("tiled", "cycle")),
    Case("thread-per-cycle 5/7 real", "resampler", _g(191, 57), I=5, D=7, pipe_out=512, out_block=512, min_launch=4096,
         moves=("cycle",), still=("tiled",)),
    Case("thread-per-cycle 5/7 complex", "resampler", _g(191, 57), complex_=True, I=5, D=7, pipe_out=512, out_block=512,
         min_launch=4096, moves=("cycle",), still=("tiled",)),
    Case("resample_split 7/11 real", "resampler", _g(100, 81), I=7, D=11, pipe_out=512, out_block=512, min_launch=4096,
         moves=("tiled",), still=("cycle",)),
    # 97 polyphase groups: the per-group tables live in device memory and only the generic kernel reads them (no counter)
    Case("generic 97/100, 1500 taps", "resampler", _g(1500, 197), I=97, D=100, pipe_out=97, out_block=97,
         still=("tiled", "cycle", "real16")),
    Case("real decimator's kernel 1/8", "resampler", _g(120, 18), I=1, D=8, pipe_out=512, out_block=512, nblk=10, min_launch=4096,
         moves=("real16",), still=("tiled", "cycle")),
    # 44 blocks: output 234837 = 97 * 2421 is the first one that late_output_is_one keeps out of the Cross set (its virtual start is the
    # last zero-stuffed position before the boundary of block 43 and it opens an output block)
    Case("generic scalar 2/3 real", "resampler", _g(150, 23), order=SCALAR, I=2, D=3, pipe_out=97, out_block=97, nblk=44,
         still=("tiled", "cycle", "real16")),
    # 4 taps, shorter than D + I: at every third boundary the first output that no longer fits already starts in the next block and
    # the Pipe does not cross over (seam_has_crossover false)
    Case("generic scalar 2/3 real, 4 taps (seams without crossover)", "resampler", _g(4, 24), order=SCALAR, I=2, D=3, pipe_out=512,
         out_block=512, route_seams=2, still=("tiled", "cycle", "real16")),
    Case("generic scalar 2/3 complex", "resampler", _g(150, 23), order=SCALAR, complex_=True, I=2, D=3, pipe_out=512, out_block=512,
         still=("tiled", "cycle")),
    # a short seamed real launch (<= 65536 outputs at the default scale) is the generic kernel's
    Case("short seamed real resampler (generic kernel)", "resampler", S.taps_resamp191, I=3, D=10, pipe_out=512, out_block=512,
         small=-1, still=("tiled", "cycle", "real16")),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- the near stream and the model's answer on it ---------------------------------------------------------------------------
_near = {}


def near(case, oracle):
    """-> (raw, exp, trace, Lp): the near stream as the device takes it (u8 bytes or floats), the restated Pipe's outputs on it,
    the Pipe's (kind, count) trace and the Pipe-visible filter length.  Computed once per case and never written to."""
    if case.name not in _near:
        n = case.nblk * case.seam
        if case.u8:
            raw = S.iq_u8(n, seed=1000 + case.seed)
            x = oracle.convert_u8(raw)
        else:
            raw = x = S.cfloat_block(n, seed=2000 + case.seed) if case.complex_ else S.real_block(n, seed=3000 + case.seed)
        model = case.model(oracle)
        w = case.width
        blocks, trace = case.pipe(model, [x[i * case.seam * w:(i + 1) * case.seam * w] for i in range(case.nblk)])
        exp = np.concatenate(blocks)
        for a in (raw, exp):
            a.setflags(write=False)
        _near[case.name] = (raw, exp, trace, model.num_coeffs)
    return _near[case.name]


def cross_of_trace(trace, K):
    """The Pipe's own One / Cross decision for its first K outputs."""
    kinds = np.concatenate([np.full(n, kind == "cross") for kind, n in trace])
    return kinds[:K]


# ---- positions --------------------------------------------------------------------------------------------------------------
def shifts(case):
    """S: 0, the smallest multiple of D B outB above 2^33, the smallest above 2^40."""
    unit = case.D * case.seam * case.shift_out_block
    return [0] + [(bound // unit + 1) * unit for bound in (1 << 33, 1 << 40)]


def output_shift(case, s):
    assert (s * case.I) % case.D == 0
    return s * case.I // case.D


@dataclasses.dataclass(frozen=True)
class Position:
    label: str
    a: int          # outputs [a, b) of the near stream are launched
    b: int
    mis: int        # stream elements by which d_in[0] sits past a 16-byte aligned address


def positions(case, K):
    """The slice's first input in the near stream (delta = in_offset(a)): 0; the first window at or behind input 40; and the first
    at or behind input 41 with d_in[0] 3 floats (real data) / one sample (complex: 8 bytes, u8: 2 bytes) past a 16-byte
    aligned address -- the first window is then 4 bytes short of alignment for real data and off it for the others, however the
    factor divides the stream index.  The last output moves with the variant, so that the slice does not always end with the stream."""
    out = []
    for i, (label, target, mis) in enumerate((("delta 0", 0, 0), ("delta 40", 40, 0), ("delta 41, misaligned", 41, 1 if case.complex_ else 3))):
        a = 0
        while in_offset(a, case.I, case.D) < target:
            a += 1
        b = K - i
        if case.span:
            b = min(b, a + case.span)
        out.append(Position(label, a, b, mis))
    return out


def combos(case, K):
    """Every (S, position) of a case, numbered: the number moves the cuts (launch_edges)."""
    return [(s, pos, q) for q, (s, pos) in enumerate((s, pos) for s in shifts(case) for pos in positions(case, K))]


def launch_edges(case, a, b, q):
    """-> (edges, route): outputs [a, b) as three launches cut at odd places, and which of them must take the case's route.
    The route launch starts at `a` (aligned input and output, at least min_launch outputs, a seam inside); the cut behind it moves with q, so that
    over a case's nine combos the later launches start at nine consecutive outputs -- every starting group of a resampler with
    up to nine groups; the second launch is long enough for the tiled kernels too where the stream is.
    The systolic cases cut as their source test does: launch starts at even outputs (16-byte aligned), a long middle launch for the
    systolic kernel and a last one of 65536 outputs that stays on the tile kernel."""
    if case.systolic:
        c2 = b - 65536
        c2 -= (c2 - a) % 2
        edges, route = [a, a + 6, c2, b], 1
        assert c2 - (a + 6) > 5 * 32768
    else:
        assert a < 64
        # the same for every first output `a` of positions(), and long enough to have a seam inside (its fix-up is part of the route)
        c1 = 64 + max(case.min_launch, 1000, case.route_seams * case.seam * case.I // case.D + 64) + 5 + q
        c2 = c1 + max(case.min_launch + 3, ((b - c1) // 2) | 1)
        if c2 >= b:
            c2 = c1 + 7
        edges, route = [a, c1, c2, b], 0
    assert all(x < y for x, y in zip(edges[:-1], edges[1:])), (case.name, edges)
    return edges, route


# ---- the slice on the device ------------------------------------------------------------------------------------------------
def guarded_slice(raw, elems, lo, hi, u8):
    """Host image of stream elements [lo - GUARD, hi + GUARD) (`elems` array entries each): [lo, hi) as they are, the rest guards."""
    n = raw.size // elems
    assert 0 <= lo < hi <= n
    if u8:
        ext = np.full((n + 2 * GUARD) * elems, 0x7F, np.uint8)
        ext[GUARD * elems:(GUARD + n) * elems] = raw ^ np.uint8(0x80)
    else:
        ext = np.full((n + 2 * GUARD) * elems, np.nan, np.float32)
    ext[(GUARD + lo) * elems:(GUARD + hi) * elems] = raw[lo * elems:hi * elems]
    return ext[lo * elems:(hi + 2 * GUARD) * elems].copy()


def upload_slice(raw, elems, lo, hi, u8, mis=0):
    """-> (tensor to keep alive, device address of stream element lo).  The tensor's own start is 16-byte aligned (torch's allocator)
    and element lo sits GUARD + mis elements into it."""
    import torch
    host = guarded_slice(raw, elems, lo, hi, u8)
    whole = torch.full((mis * elems + host.size,), 0x7F if u8 else float("nan"), dtype=torch.uint8 if u8 else torch.float32, device="cuda")
    assert whole.data_ptr() % 16 == 0
    whole[mis * elems:].copy_(torch.from_numpy(host))
    return whole, whole.data_ptr() + whole.element_size() * elems * (mis + GUARD)


@contextlib.contextmanager
def route_knobs(hip, case):
    """The process-wide route switches a case runs under, put back afterwards."""
    prev = hip.set_small_launch_outputs(case.small)
    if case.systolic:
        hip.lib.sdrhip_debug_set_systolic(1)
    try:
        yield
    finally:
        hip.lib.sdrhip_debug_set_systolic(2)        # the library's own choice by launch size
        hip.set_small_launch_outputs(prev)


def counters(hip, names):
    return {n: int(getattr(hip.lib, COUNTERS[n])()) for n in names}


def run_case(hip, case, desc, raw, Lp, s, pos, q):
    """Outputs [T + a, T + b) of the stream shifted by s, from a buffer that holds only the slice the header guarantees.
    -> (outputs, counter deltas of the route launch)."""
    from gpu_util import dev_empty_f32, ptr, to_host
    w = case.width
    T = output_shift(case, s)
    lo, hi = input_range(case.I, case.D, Lp, pos.a, pos.b)
    keep, d_in = upload_slice(raw, 2 if (case.complex_ or case.u8) else 1, lo, hi, case.u8, pos.mis)
    out = dev_empty_f32((pos.b - pos.a) * w)
    edges, route = launch_edges(case, pos.a, pos.b, q)
    run = desc.run_u8 if case.u8 else desc.run
    kw = {"out_block": case.out_block} if case.family == "resampler" else {}
    watched = case.moves + case.still
    delta = {}
    for i, (k0, k1) in enumerate(zip(edges[:-1], edges[1:])):
        before = counters(hip, watched)
        run(d_in, lo + s, ptr(out) + 4 * w * (k0 - pos.a), T + k0, T + k1, case.seam, **kw)
        if i == route:
            after = counters(hip, watched)
            delta = {n: after[n] - before[n] for n in watched}
    got = to_host(out)
    del keep
    return got, delta
