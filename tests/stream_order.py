"""The gated run and its case table (tests/test_stream_order_cases.py on the CPU, tests/test_gpu_stream_order.py on the device).
TEST INFRASTRUCTURE ONLY.

What the other GPU tests cannot see.  They call an operator on the null stream with the input already in place and synchronise
straight after it, so a launch that went to another stream, an upload that was not finished when the first kernel started, a scratch
buffer reused too early or a host synchronisation inside a call that promises none all leave the result as it should be.  A GATED
run makes the order on `stream` the only thing that can produce the right answer:

  on a synchronised device   d_in holds POISON (another seeded stream of the same format and length), the outputs carry canaries,
                             workspaces and state buffers are filled with canary words;
  queued on a non-blocking   a bounded device delay; a device-to-device copy of the real input into d_in; the operator (or the
  stream S, with no host     whole call sequence); a copy of a second poison stream over d_in; copies of every output into
  synchronisation between    snapshot buffers.

A launch that is not ordered behind the copy on S reads poison; one that is not ordered before the second copy reads the other poison;
one that runs after the snapshot leaves canaries in it.  While the delay spins, S.query() is False: a call that synchronised the host
with S would have drained it, so "no host synchronisation" is asserted by the query straight after the call returns.

The expected values come from the CPU side the suite already has (the oracle, oracle/pipes_model.py, tuner_model, tuned_chain_model,
agc_model, spectrum_model, spectrum_reduce_model), never from a device run."""
import contextlib
import time

import numpy as np

import agc_model as AM
import signals as S
import spectrum_model as SM
import spectrum_reduce_model as SR
import tuned_chain_model as TCM
import tuner_model as TM
from oracle import pipes_model as PM

B = 8192
NBLK = 6
AVX, SSE, SCALAR = PM.ORDER_AVX, PM.ORDER_SSE, PM.ORDER_SCALAR
DELAY_MIN_MS, DELAY_MAX_MS = 20.0, 200.0


def seeded(fmt, n, seed):
    """n samples (complex for u8 / i16 / cf32, real for f32) of a seeded stream, as the array the device takes."""
    rng = np.random.default_rng(seed)
    if fmt == "u8":
        return rng.integers(0, 256, 2 * n, dtype=np.uint8)
    if fmt == "i16":
        return rng.integers(-32768, 32768, 2 * n).astype(np.int16)
    if fmt == "cf32":
        return rng.uniform(-1, 1, 2 * n).astype(np.float32)
    return rng.uniform(-1, 1, n).astype(np.float32)


def split(x, width, block):
    n = x.size // width
    return [x[i * block * width:(i + 1) * block * width] for i in range(n // block)]


def same_bits(a, b):
    """Bit for bit, NaN by position -> bool array."""
    a, b = np.ascontiguousarray(a, np.float32).ravel(), np.ascontiguousarray(b, np.float32).ravel()
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def cross_positions(trace):
    """Output indices the Pipe computed with the sequential (Cross) kernel, from a pipes_model trace."""
    pos, at = [], 0
    for kind, count in trace:
        if kind == "cross":
            pos += list(range(at, at + count))
        at += count
    return np.array(pos, dtype=np.int64)


class Case:
    """One operator call (or call sequence) on one input buffer.  The CPU side: stream(which), expected(oracle, x) -> {name: float32
    array}, cross(oracle) -> (outputs the sequential kernel computed, how many of them differ from the SIMD order) or None.  The
    device side: make(hip) -> a fresh descriptor (None for the operators without one), outputs() -> {name: floats},
    scratch(hip, obj) -> {name: bytes}, states() -> {name: float32 array}, call(hip, obj, stream, p_in, buf) queues the operator on
    the stream handle, knobs(hip) forces the route, counters -> {counter: (op, value)} over one call."""
    fmt, n, seed = "cf32", NBLK * B, 0
    nosync = True                   # after a warm-up run of the same shape the call makes no host synchronisation
    warm_on_stream = False          # ... of the same shape ON THE SAME STREAM
    tolerance = False               # True: the spectrum operator's tolerance contract, not bit parity
    counters = {}
    _cache = None

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return self.name

    def stream(self, which):
        """0 = the real input, 1 and 2 = the two poison streams."""
        return seeded(self.fmt, self.n, 7000 + 100 * self.seed + which)

    def floats(self, oracle, x):
        return oracle.convert_u8(x) if self.fmt == "u8" else oracle.convert_i16(x) if self.fmt == "i16" else x

    def expected(self, oracle, x):
        raise NotImplementedError

    def expected_real(self, oracle):
        if self._cache is None:
            e = self.expected(oracle, self.stream(0))
            for v in e.values():
                v.setflags(write=False)
            self._cache = e
        return self._cache

    def cross(self, oracle):
        return None

    def make(self, hip):
        return None

    def scratch(self, hip, obj):
        return {}

    def states(self):
        return {}

    def outputs(self, oracle):
        return {k: v.size for k, v in self.expected_real(oracle).items()}

    def knobs(self, hip):
        return contextlib.nullcontext()

    def check(self, got, exp, what, x=None):
        bad = np.nonzero(~same_bits(got, exp))[0]
        if bad.size:
            i = int(bad[0])
            g, e = np.asarray(got, np.float32).ravel(), np.asarray(exp, np.float32).ravel()
            raise AssertionError(f"{what}: {bad.size}/{e.size} floats differ; first at {i}: {g[i]!r} ({g.view(np.uint32)[i]:#x}) vs "
                                 f"{e[i]!r} ({e.view(np.uint32)[i]:#x})")


# ---- one-launch operators ------------------------------------------------------------------------------------------------------
class OneLaunch(Case):
    LAST = (0.25, -0.75)            # fmDemod's carried sample
    FACTOR = 0.2

    def __init__(self, op, fmt, seed):
        super().__init__(op)
        self.op, self.fmt, self.seed = op, fmt, seed
        self.n = NBLK * B + 5
        if op == "am_demod":
            self.counters = {"sdrhip_debug_am_demod_launches": ("==", 1)}

    def expected(self, oracle, x):
        if self.op == "scale":
            return {"out": oracle.scale(self.FACTOR, x)}
        if self.op == "convert_u8":
            return {"out": oracle.convert_u8(x)}
        if self.op == "convert_i16":
            return {"out": oracle.convert_i16(x)}
        if self.op == "fm_demod":
            return {"out": oracle.fm_demod(x, self.LAST)}
        with np.errstate(all="ignore"):
            return {"out": AM.magnitude(np.ascontiguousarray(x[0::2]), np.ascontiguousarray(x[1::2]))}

    def call(self, hip, obj, stream, p_in, buf):
        L, out = hip.lib, buf["out"].data_ptr()
        if self.op == "scale":
            hip.check(L.sdrhip_scale_run(stream, self.FACTOR, p_in, out, self.n), self.op)
        elif self.op == "convert_u8":
            hip.check(L.sdrhip_convert_u8_run(stream, p_in, out, 2 * self.n), self.op)
        elif self.op == "convert_i16":
            hip.check(L.sdrhip_convert_i16_run(stream, p_in, out, 2 * self.n), self.op)
        elif self.op == "fm_demod":
            hip.check(L.sdrhip_fm_demod_run(stream, p_in, 0, out, 0, self.n, self.LAST[0], self.LAST[1]), self.op)
        else:
            hip.check(L.sdrhip_am_demod_run(stream, p_in, out, self.n), self.op)


# ---- FIR stage operators ------------------------------------------------------------------------------------------------------
class Fir(Case):
    """A filter / decimator / resampler over NBLK blocks of B with seam B; outputs [0, K), K = the whole output blocks of 512 the
    reference's Pipe yields.  small: sdrhip_set_small_launch_outputs for the run; systolic: sdrhip_debug_set_systolic."""

    def __init__(self, name, kind, fmt, taps, seed, order=AVX, factor=1, ratio=None, sym=False, nblk=NBLK, small=None, systolic=None,
                 counters=None, min_outputs=0):
        super().__init__(name)
        self.kind, self.fmt, self.taps, self.seed, self.order, self.factor, self.ratio, self.sym = kind, fmt, taps, seed, order, factor, ratio, sym
        self.cplx = fmt != "f32"
        self.width = 2 if self.cplx else 1
        self.n = nblk * B
        self.small, self.systolic = small, systolic
        self.counters = counters or {}
        self.min_outputs = min_outputs
        self._trace = None

    def model(self, oracle):
        if self.kind == "res":
            return PM.ResamplerModel(oracle, self.ratio[0], self.ratio[1], self.taps(), self.order, self.cplx)
        return PM.FilterModel(oracle, self.taps(), self.order, complex_=self.cplx and not self.sym, sym=self.sym, factor=self.factor)

    def _pipe(self, oracle, x):
        m = self.model(oracle)
        blocks = split(self.floats(oracle, x), self.width, B)
        if self.kind == "res":
            return PM.fir_resampler_pipe(m, blocks, 512)
        return PM.fir_decimator_pipe(m, blocks, 512)

    def expected(self, oracle, x):
        out, trace = self._pipe(oracle, x)
        e = np.concatenate(out)
        assert e.size // self.width >= self.min_outputs
        return {"out": e}

    def cross(self, oracle, x=None):
        x = self.stream(0) if x is None else x
        out, trace = self._pipe(oracle, x)
        e = np.concatenate(out).reshape(-1, self.width)
        pos = cross_positions(trace)
        pos = pos[pos < e.shape[0]]
        m, f = self.model(oracle), self.floats(oracle, x)
        if self.kind == "res":
            simd = m.one((0, 0), e.shape[0], f)[0].reshape(-1, self.width)
        else:
            simd = m.one(e.shape[0], f).reshape(-1, self.width)
        differ = ~same_bits(simd[pos], e[pos]).reshape(-1, self.width).all(axis=1)
        return pos.size, int(differ.sum())

    def make(self, hip):
        if self.kind == "res":
            return hip.Resampler(self.ratio[0], self.ratio[1], self.taps(), self.order, self.cplx)
        if self.kind == "filt":
            return hip.Filter(self.taps(), self.order, complex_=self.cplx, sym=self.sym)
        return hip.Decimator(self.factor, self.taps(), self.order, complex_=self.cplx, sym=self.sym)

    @contextlib.contextmanager
    def knobs(self, hip):
        prev = hip.set_small_launch_outputs(self.small) if self.small is not None else None
        if self.systolic is not None:
            hip.lib.sdrhip_debug_set_systolic(self.systolic)
        try:
            yield
        finally:
            if self.systolic is not None:
                hip.lib.sdrhip_debug_set_systolic(2)
            if prev is not None:
                hip.set_small_launch_outputs(prev)

    def call(self, hip, obj, stream, p_in, buf):
        K = buf["out"].numel() // self.width
        if self.kind == "res":
            obj.run(p_in, 0, buf["out"].data_ptr(), 0, K, B, stream=stream, out_block=512)
        elif self.fmt == "u8":
            obj.run_u8(p_in, 0, buf["out"].data_ptr(), 0, K, B, stream=stream)
        else:
            obj.run(p_in, 0, buf["out"].data_ptr(), 0, K, B, stream=stream)


CROSSFIX, SYSTOLIC_CTR, TILED = "sdrhip_debug_decimator_crossfix_launches", "sdrhip_debug_systolic_launches", "sdrhip_debug_tiled_launches"
REAL16, CYCLE = "sdrhip_debug_decimate_real16_launches", "sdrhip_debug_resample_cycle_launches"
GENERIC_U8 = "sdrhip_debug_generic_u8_launches"
SYS_NBLK = 61                   # 64 * 240 * 4 outputs is the systolic kernel's minimum; 61 blocks give 61 440 + 512 and a ragged strip


def _gauss(n, seed, sigma=0.05):
    return lambda: S.gauss_taps(n, seed, sigma)


def fir_cases():
    c = []
    for fmt, seed in (("cf32", 1), ("u8", 2)):
        c.append(Fir(f"decimator /8 127 taps {fmt}, Cross outputs inside the tile kernel", "dec", fmt, S.taps_decim127, seed, factor=8, small=-1,
                     counters={CROSSFIX: ("==", 0), SYSTOLIC_CTR: ("==", 0), TILED: ("==", 0)}))
        c.append(Fir(f"decimator /8 127 taps {fmt}, tile kernel + fix-up launch", "dec", fmt, S.taps_decim127, seed, factor=8, small=0,
                     counters={CROSSFIX: ("==", 1), SYSTOLIC_CTR: ("==", 0), TILED: ("==", 0)}))
        # the scalar order has no tile kernel on u8 input: the generic kernel, which decides Cross per output (its counter: u8 only)
        c.append(Fir(f"decimator /8 127 taps {fmt}, scalar order", "dec", fmt, S.taps_decim127, seed, order=SCALAR, factor=8, small=0,
                     counters=dict({CROSSFIX: ("==", 0), SYSTOLIC_CTR: ("==", 0)}, **({GENERIC_U8: ("==", 1)} if fmt == "u8" else {}))))
        c.append(Fir(f"systolic decimator {fmt}, fix-up inside the launch", "dec", fmt, S.taps_decim127, seed + 2, factor=8, nblk=SYS_NBLK, small=0,
                     systolic=2, counters={CROSSFIX: ("==", 0), SYSTOLIC_CTR: ("==", 1)}, min_outputs=64 * 240 * 4 + 1))
        c.append(Fir(f"systolic decimator {fmt}, fix-up as a launch of its own", "dec", fmt, S.taps_decim127, seed + 2, factor=8, nblk=SYS_NBLK,
                     small=0, systolic=1, counters={CROSSFIX: ("==", 1), SYSTOLIC_CTR: ("==", 1)}, min_outputs=64 * 240 * 4 + 1))
    c.append(Fir("real symmetric filter 128 taps, fast filter + fix-up", "filt", "f32", S.taps_audio_half64, 5, sym=True, small=0,
                 counters={TILED: ("==", 0), REAL16: ("==", 0)}))
    c.append(Fir("real resampler 3/10 191 taps", "res", "f32", S.taps_resamp191, 6, ratio=(3, 10), small=0,
                 counters={TILED: ("==", 0), CYCLE: ("==", 0)}))
    c.append(Fir("real resampler 2/3 150 taps, cycle kernel", "res", "f32", _gauss(150, 611, 0.3), 7, ratio=(2, 3), small=0,
                 counters={CYCLE: (">=", 1)}))
    c.append(Fir("real decimator /4 128 taps", "dec", "f32", _gauss(128, 612), 8, factor=4, small=0, counters={REAL16: (">=", 1)}))
    c.append(Fir("split real decimator /5 31 taps", "dec", "f32", _gauss(31, 601), 9, factor=5, small=0, counters={TILED: (">=", 1)}))
    return c


# ---- dcBlocker and agc ------------------------------------------------------------------------------------------------------
class Iir(Case):
    """sdrhip_dc_blocker_run / sdrhip_agc_run: with a workspace (the speculating route: speculate, repair rounds, settle; the fourth
    statistics word says how many chunks it speculated on) or without one (the sequential walk)."""
    DC_STATE = (0.25, -0.5)
    MU, REFERENCE, AGC_STATE = 0.4, 1.0, 0.75

    def __init__(self, op, parallel, seed):
        super().__init__(f"{op}, {'speculating route with a workspace' if parallel else 'sequential walk, null workspace'}")
        self.op, self.parallel, self.seed = op, parallel, seed
        self.fmt = "f32" if op == "dc_blocker" else "cf32"
        self.n = 3 * B + 5
        self.run_in = 1024 if op == "dc_blocker" else 0

    def expected(self, oracle, x):
        if self.op == "dc_blocker":
            out, fs, fo = oracle.dc_blocker(x, *self.DC_STATE)
            return {"out": out, "final": np.array([fs, fo], np.float32)}
        out, fin = AM.agc(x.view(np.complex64), self.MU, self.REFERENCE, self.AGC_STATE)
        return {"out": AM.interleaved(out).copy(), "final": np.array([fin], np.float32)}

    def plan(self, hip):
        return hip.dc_plan(self.n, self.run_in) if self.op == "dc_blocker" else hip.agc_plan(self.n, self.MU, self.run_in)

    def scratch(self, hip, obj):
        if not self.parallel:
            return {}
        L = hip.lib
        return {"ws": L.sdrhip_dc_blocker_workspace_bytes(self.n) if self.op == "dc_blocker" else L.sdrhip_agc_workspace_bytes(self.n)}

    def call(self, hip, obj, stream, p_in, buf):
        ws = buf.get("ws")
        p_ws, b_ws = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
        if self.op == "dc_blocker":
            hip.check(hip.lib.sdrhip_dc_blocker_run(stream, p_in, buf["out"].data_ptr(), self.n, self.DC_STATE[0], self.DC_STATE[1],
                                                    buf["final"].data_ptr(), p_ws, b_ws, self.run_in), self.op)
        else:
            hip.check(hip.lib.sdrhip_agc_run(stream, p_in, buf["out"].data_ptr(), self.n, self.MU, self.REFERENCE, self.AGC_STATE,
                                             buf["final"].data_ptr(), p_ws, b_ws, self.run_in), self.op)

    def after(self, hip, buf):
        """the route's own counter: the chunks the launch speculated on, in the workspace's fourth statistics word"""
        if self.parallel:
            chunks = self.plan(hip)[0]
            assert chunks > 0, f"{self.name}: the plan takes the sequential walk at n = {self.n}"
            assert hip.dc_stats(buf["ws"])[3] == chunks, f"{self.name}: speculated on {hip.dc_stats(buf['ws'])[3]} chunks, planned {chunks}"


class IirRows(Case):
    """Two consecutive pushes of the row forms, 3 rows, the state passing through device memory: d_final of the first push is
    d_state of the second, and d_final aliases d_state, as the header allows.  Both pushes are queued behind one gate."""
    ROWS = 3
    MU, REFERENCE = 0.4, 1.0

    def __init__(self, op, parallel, seed):
        super().__init__(f"{op} rows, two pushes, {'workspace' if parallel else 'null workspace'}, d_final == d_state")
        self.op, self.parallel, self.seed = op, parallel, seed
        self.fmt = "f32" if op == "dc_blocker" else "cf32"
        self.half = B + 3 if op == "agc" else 3 * B + 1          # samples per row and push
        self.n = self.ROWS * 2 * self.half                       # the input holds the rows one after the other, each two pushes long
        self.run_in = 1024 if op == "dc_blocker" else 0
        self.width = 1 if op == "dc_blocker" else 2
        self.counters = {"sdrhip_debug_rows_launches": ("==", 10 if parallel else 2)}     # 5 per call with chunks, 1 on the sequential walk

    def state0(self):
        if self.op == "dc_blocker":
            return np.array([0.25, -0.5, -0.125, 0.375, 0.0, 0.0], np.float32)
        return np.array([0.75, 1.0, 1.5], np.float32)

    def states(self):
        return {"state": self.state0()}

    def expected(self, oracle, x):
        rows = x.reshape(self.ROWS, -1)
        if self.op == "agc":
            o, fin = AM.agc(rows.view(np.complex64), self.MU, self.REFERENCE, self.state0())
            return {"out": np.ascontiguousarray(o).view(np.float32).ravel().copy(), "state": np.asarray(fin, np.float32).copy()}
        outs, fins = [], []
        for r in range(self.ROWS):
            o, fs, fo = oracle.dc_blocker(rows[r], *self.state0()[2 * r:2 * r + 2])
            outs.append(o)
            fins += [fs, fo]
        return {"out": np.concatenate(outs), "state": np.array(fins, np.float32)}

    def scratch(self, hip, obj):
        if not self.parallel:
            return {}
        L = hip.lib
        f = L.sdrhip_dc_blocker_rows_workspace_bytes if self.op == "dc_blocker" else L.sdrhip_agc_rows_workspace_bytes
        return {"ws": f(self.ROWS, self.half)}

    def call(self, hip, obj, stream, p_in, buf):
        ws = buf.get("ws")
        p_ws, b_ws = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
        stride = 2 * self.half * self.width
        st = buf["state"].data_ptr()
        for push in range(2):
            off = 4 * push * self.half * self.width
            if self.op == "dc_blocker":
                hip.check(hip.lib.sdrhip_dc_blocker_run_rows(stream, p_in + off, stride, buf["out"].data_ptr() + off, stride, self.ROWS, self.half,
                                                             st, st, p_ws, b_ws, self.run_in), self.name)
            else:
                hip.check(hip.lib.sdrhip_agc_run_rows(stream, p_in + off, stride, buf["out"].data_ptr() + off, stride, self.ROWS, self.half, self.MU,
                                                      self.REFERENCE, st, st, p_ws, b_ws, self.run_in), self.name)


class DemodRows(Case):
    """fmDemod / amDemod rows: 3 rows in one launch; fmDemod with its carried samples in device memory, d_last_out == d_last_iq."""
    ROWS = 3

    def __init__(self, op, seed):
        super().__init__(f"{op} rows")
        self.op, self.seed = op, seed
        self.m = B + 7
        self.n = self.ROWS * self.m
        self.counters = {"sdrhip_debug_rows_launches": ("==", 1)} if op == "fm_demod" else {"sdrhip_debug_am_demod_launches": ("==", 1)}

    def states(self):
        return {"last": np.array([0.25, -0.75, 0.0, 0.0, -0.5, 0.125], np.float32)} if self.op == "fm_demod" else {}

    def expected(self, oracle, x):
        rows = x.reshape(self.ROWS, -1)
        if self.op == "fm_demod":
            last = self.states()["last"]
            out = np.concatenate([oracle.fm_demod(rows[r], (float(last[2 * r]), float(last[2 * r + 1]))) for r in range(self.ROWS)])
            return {"out": out, "last": np.concatenate([rows[r][-2:] for r in range(self.ROWS)])}
        with np.errstate(all="ignore"):
            return {"out": AM.magnitude(np.ascontiguousarray(x[0::2]), np.ascontiguousarray(x[1::2]))}

    def call(self, hip, obj, stream, p_in, buf):
        if self.op == "fm_demod":
            hip.check(hip.lib.sdrhip_fm_demod_run_rows(stream, p_in, 2 * self.m, 0, buf["out"].data_ptr(), self.m, self.ROWS, 0, self.m,
                                                       buf["last"].data_ptr(), buf["last"].data_ptr()), self.name)
        else:
            hip.check(hip.lib.sdrhip_am_demod_run_rows(stream, p_in, 2 * self.m, buf["out"].data_ptr(), self.m, self.ROWS, self.m), self.name)


class FirRows(Case):
    """sdrhip_{filter,decimator,resampler}_run_rows on 3 rows, route 1 (one banked launch and one fix-up launch for all rows) and route
    2 (the one-row operator row by row on the caller's stream).  Each row is a stream of its own, NBLK blocks with seam B."""
    ROWS = 3
    FIR_LAUNCHES, FIR_FIXUPS = "sdrhip_debug_fir_rows_launches", "sdrhip_debug_fir_rows_fixups"

    def __init__(self, one, route):
        super().__init__(f"rows x3 of [{one.name}], route {route}")
        self.one, self.route = one, route
        self.fmt, self.seed = one.fmt, one.seed + 40
        self.n = self.ROWS * one.n
        self.counters = {self.FIR_LAUNCHES: ("==", 1), self.FIR_FIXUPS: ("==", 1)} if route == 1 else {self.FIR_LAUNCHES: ("==", 0), self.FIR_FIXUPS: ("==", 0)}

    def _rows(self, x):
        return x.reshape(self.ROWS, -1)

    def cross(self, oracle):
        """every row is a seamed stream of its own, with other seeds than the one-row case: the shares summed over the rows"""
        parts = [self.one.cross(oracle, np.ascontiguousarray(r)) for r in self._rows(self.stream(0))]
        return sum(p[0] for p in parts), sum(p[1] for p in parts)

    def expected(self, oracle, x):
        return {"out": np.concatenate([self.one.expected(oracle, np.ascontiguousarray(r))["out"] for r in self._rows(x)])}

    def make(self, hip):
        return self.one.make(hip)

    def knobs(self, hip):
        return self.one.knobs(hip)

    def call(self, hip, obj, stream, p_in, buf):
        w = self.one.width
        K = buf["out"].numel() // (self.ROWS * w)
        kw = {"out_block": 512} if self.one.kind == "res" else {}
        obj.run_rows(p_in, buf["out"].data_ptr(), 0, K, in_base=0, seam_block=B, route=self.route, stream=stream, in_stride=self.one.n * w,
                     out_stride=K * w, rows=self.ROWS, **kw)


# ---- the tuner family ------------------------------------------------------------------------------------------------------
def osc(period):
    return TM.shift_table(-3, period)


SUBNORMALS = np.array([1e-42, -3e-39, -0.0, 1.0, 0.0, -0.0, 0.70710677, -0.70710677, -1.0, 1e-45, 2.5, -0.0, 1e-30, 3.0], np.float32)
BANK_TABLES = [osc(1000), np.array([1.0, 0.0], np.float32), SUBNORMALS]
TUNER_FUSED, TUNER_I16, BANK_LAUNCHES = "sdrhip_debug_tuner_fused_launches", "sdrhip_debug_tuner_i16_launches", "sdrhip_debug_tuner_bank_launches"
# samples a two-pass chunk mixes: 1486 outputs, so K = 6129 outputs make 5 mix + decimate pairs; an even count keeps every pair's first
# output 16-byte aligned, so each pair's decimator is the tile kernel whose fix-up launches the library counts
TUNER_CHUNK = 12008


def tuner_outputs(oracle, case, x, table, seam):
    return TM.tuner_expected(oracle, S.taps_decim127(), getattr(case, "order", AVX), 8, case.floats(oracle, x), table, seam, 0, block_out=1)


def straddlers(n_out, seam=B, lp=128, factor=8):
    v = np.arange(n_out, dtype=np.int64) * factor
    return np.nonzero((v // seam) != ((v + lp - 1) // seam))[0]


def two_pass_chunks(K=(NBLK * B - 128) // 8 + 1):
    """[k_begin, k_end) of the mix + decimate pairs tuner_two_pass makes of outputs [0, K) at TUNER_CHUNK (tuner.cpp)"""
    per = (TUNER_CHUNK - 128) // 8 + 1
    return [(a, min(a + per, K)) for a in range(0, K, per)]


def two_pass_seamed_chunks():
    cross = straddlers((NBLK * B - 128) // 8 + 1)
    return sum(1 for a, b in two_pass_chunks() if ((cross >= a) & (cross < b)).any())


class Tuner(Case):
    def __init__(self, fmt, route, seed, small=0):
        two = route == 2
        super().__init__(f"tuner {fmt}, " + (f"two-pass route in chunks of {TUNER_CHUNK}" if two else
                                             "fused route, " + ("tile kernel + fix-up launch" if small == 0 else "Cross outputs inside")))
        self.fmt, self.route, self.seed, self.small = fmt, route, seed, small
        self.table = osc(1000)
        if two:
            # every mix + decimate pair whose chunk holds a seam launches the tile decimator's fix-up kernel (small = 0): the library's
            # count of those launches measures the pairs the call made
            self.counters = {TUNER_FUSED: ("==", 0), TUNER_I16: ("==", 0), CROSSFIX: ("==", two_pass_seamed_chunks()), TILED: ("==", 0)}
        else:
            self.counters = {TUNER_FUSED: ("==", 0 if fmt == "i16" else 1), TUNER_I16: ("==", 1 if fmt == "i16" else 0)}

    def expected(self, oracle, x):
        return {"out": tuner_outputs(oracle, self, x, self.table, B)}

    def cross(self, oracle):
        x = self.stream(0)
        e, simd = tuner_outputs(oracle, self, x, self.table, B).reshape(-1, 2), tuner_outputs(oracle, self, x, self.table, 0).reshape(-1, 2)
        pos = straddlers(e.shape[0])
        return pos.size, int((~same_bits(e[pos], simd[pos]).reshape(-1, 2).all(axis=1)).sum())

    def make(self, hip):
        t = hip.Tuner(8, S.taps_decim127(), self.table)
        t.set_route(self.route)
        return t

    @contextlib.contextmanager
    def knobs(self, hip):
        prev = hip.set_small_launch_outputs(self.small)
        chunk = hip.set_tuner_chunk(TUNER_CHUNK) if self.route == 2 else None
        try:
            yield
        finally:
            if chunk is not None:
                hip.set_tuner_chunk(chunk)
            hip.set_small_launch_outputs(prev)

    def call(self, hip, obj, stream, p_in, buf):
        K = buf["out"].numel() // 2
        run = {"cf32": obj.run, "u8": obj.run_u8, "i16": obj.run_i16}[self.fmt]
        run(p_in, 0, buf["out"].data_ptr(), 0, K, B, stream=stream)


class TunerBank(Case):
    def __init__(self, fmt, route, seed, small=0):
        super().__init__(f"tuner bank x3 {fmt}, " + ("banked launch + fix-up launch" if route == 1 and small == 0 else
                                                     "banked launch, Cross outputs inside" if route == 1 else
                                                     f"route 2, SSE order: each channel's tuner leases a lane, chunks of {TUNER_CHUNK}"))
        self.fmt, self.route, self.seed, self.small = fmt, route, seed, small
        # route 2 runs K tuners on `auto`, which take their fused kernel wherever it fits: the SSE order has none, so each of them
        # goes two-pass and leases a lane of its own
        self.order = AVX if route == 1 else SSE
        self.counters = {BANK_LAUNCHES: ("==", 1)} if route == 1 else {BANK_LAUNCHES: ("==", 0), TUNER_FUSED: ("==", 0), TUNER_I16: ("==", 0)}

    def expected(self, oracle, x):
        return {"out": np.concatenate([tuner_outputs(oracle, self, x, t, B) for t in BANK_TABLES])}

    def cross(self, oracle):
        x = self.stream(0)
        total = differ = 0
        for t in BANK_TABLES:
            e, simd = tuner_outputs(oracle, self, x, t, B).reshape(-1, 2), tuner_outputs(oracle, self, x, t, 0).reshape(-1, 2)
            pos = straddlers(e.shape[0])
            total += pos.size
            differ += int((~same_bits(e[pos], simd[pos]).reshape(-1, 2).all(axis=1)).sum())
        return total, differ

    def make(self, hip):
        b = hip.TunerBank(8, S.taps_decim127(), BANK_TABLES, self.order)
        b.set_route(self.route)
        return b

    @contextlib.contextmanager
    def knobs(self, hip):
        prev = hip.set_small_launch_outputs(self.small)
        chunk = hip.set_tuner_chunk(TUNER_CHUNK) if self.route == 2 else None
        try:
            yield
        finally:
            if chunk is not None:
                hip.set_tuner_chunk(chunk)
            hip.set_small_launch_outputs(prev)

    def call(self, hip, obj, stream, p_in, buf):
        K = buf["out"].numel() // (2 * len(BANK_TABLES))
        run = {"cf32": obj.run, "u8": obj.run_u8, "i16": obj.run_i16}[self.fmt]
        run(p_in, 0, buf["out"].data_ptr(), 2 * K, 0, K, B, stream=stream)


# ---- the FM chain and the FM bank ------------------------------------------------------------------------------------------------------
CHAIN_NBLK, MODEL_NBLK = 20, 60
GAIN = 0.2
# the audio a run over the first 20 blocks can write: a prefix of the first audio block the restated Pipes yield on 60 blocks
CHAIN_Q1 = (((CHAIN_NBLK * B - 128) // 8 + 1) * 3 - 192) // 10 + 1 - 127


def model_blocks(x, fmt):
    """The 20 blocks the device gets, and 40 seeded blocks behind them that no output of the run reads: the Pipes need 60 to yield."""
    tail = seeded(fmt, (MODEL_NBLK - CHAIN_NBLK) * B, 6800)
    return split(np.concatenate([x, tail]), 2, B)
SMALL_CHAIN, SMALL_TUNED, FM_BANK, FM_BANK_I16 = ("sdrhip_debug_small_chain_launches", "sdrhip_debug_small_chain_tuned_launches",
                                                  "sdrhip_debug_fm_bank_launches", "sdrhip_debug_fm_bank_i16_launches")


class Chain(Case):
    """FmChain.run over 20 blocks of u8 IQ: the one-kernel route, the stage route and the stage route with the fused tail, with and
    without a tuner.  The real stream is an FM signal, the poison streams are noise."""
    fmt, n = "u8", CHAIN_NBLK * B

    def __init__(self, route, tuned, seed):
        super().__init__(f"FM chain, {route}, {'tuned' if tuned else 'untuned'}")
        self.route, self.tuned, self.seed = route, tuned, seed
        small = 1 if route == "one kernel" else 0
        self.counters = {SMALL_CHAIN: ("==", small)}
        if tuned:
            self.counters[SMALL_TUNED] = ("==", small)

    def stream(self, which):
        return S.iq_u8_fm(self.n, seed=4400 + self.seed) if which == 0 else super().stream(which)

    def expected(self, oracle, x):
        blocks = model_blocks(x, "u8")
        args = (S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(), GAIN, B)
        if self.tuned:
            out = TCM.fm_receiver_tuned(oracle, blocks, osc(1000), *args)
        else:
            out = PM.fm_receiver(oracle, blocks, *args)
        return {"out": np.concatenate(out)[:CHAIN_Q1].copy()}

    def make(self, hip):
        ch = hip.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), GAIN, B)
        if self.tuned:
            ch.set_tuner(osc(1000))
        ch.set_small_chain(1 if self.route == "one kernel" else 0)
        ch.set_fused_tail(1 if self.route == "fused tail" else 0)
        return ch

    def scratch(self, hip, obj):
        return {"ws": obj.workspace_bytes(self.n)}

    # The library counts the one-kernel launches only.  Which of the other two routes ran is read from the chain's per-stage timing,
    # switched on for the synchronous run alone (its events are extra work on the stream): a stage that launched nothing reports 0 ms.
    RAN = {"one kernel": {"fused_chain"}, "stage kernels": {"decimate", "resample", "filter"}, "fused tail": {"decimate", "fused_tail"}}

    def sync_begin(self, hip, obj):
        obj.enable_timing(True)

    def sync_end(self, hip, obj):
        ms, runs = obj.read_timing()
        obj.enable_timing(False)
        ran = {k for k, v in ms.items() if v > 0.0}
        assert runs == 1 and ran == self.RAN[self.route], f"{self.name}: the stages that launched were {sorted(ran)}"

    def call(self, hip, obj, stream, p_in, buf):
        q1 = buf["out"].numel()
        assert obj.plan(0, self.n, self.n)[:2] == (0, q1), "the model's prefix is not the run's plan"
        obj.run(p_in, 0, self.n, buf["out"].data_ptr(), 0, q1, buf["ws"].data_ptr(), buf["ws"].numel(), stream=stream)


class FmBank(Case):
    """FmBank.run, 2 stations: the banked one-kernel launch and the station-by-station route on the caller's workspace."""
    n = CHAIN_NBLK * B
    TABLES = [osc(1000), TM.shift_table(1, 4)]

    def __init__(self, fmt, route, seed):
        super().__init__(f"FM bank x2 {fmt}, {'banked launch' if route == 1 else 'station by station'}")
        self.fmt, self.route, self.seed = fmt, route, seed
        self.counters = {FM_BANK: ("==", 1 if route == 1 else 0), FM_BANK_I16: ("==", 1 if route == 1 and fmt == "i16" else 0)}

    def stream(self, which):
        if which:
            return super().stream(which)
        u8 = S.iq_u8_fm(self.n, seed=4500 + self.seed)
        return u8 if self.fmt == "u8" else ((u8.astype(np.int16) - 128) * 16).astype(np.int16)

    def expected(self, oracle, x):
        args = (S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(), GAIN, B)
        rows = []
        blocks = model_blocks(x, self.fmt)
        for t in self.TABLES:
            if self.fmt == "u8":
                rows.append(np.concatenate(TCM.fm_receiver_tuned(oracle, blocks, t, *args))[:CHAIN_Q1])
            else:
                import fm_bank_i16_cases as FI
                assert FI.GAIN == GAIN
                rows.append(FI.tail_from_d(oracle, FI.receiver_stages(oracle, blocks, t)[1])[:CHAIN_Q1])
        return {"out": np.concatenate(rows)}

    def make(self, hip):
        b = hip.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), self.TABLES, GAIN, B)
        b.set_route(self.route)
        return b

    def scratch(self, hip, obj):
        return {"ws": max(obj.workspace_bytes(self.n), 16)}

    def call(self, hip, obj, stream, p_in, buf):
        q1 = buf["out"].numel() // len(self.TABLES)
        assert obj.plan(0, self.n, self.n)[:2] == (0, q1), "the model's prefix is not the run's plan"
        run = obj.run if self.fmt == "u8" else obj.run_i16
        run(p_in, 0, self.n, buf["out"].data_ptr(), q1, 0, q1, buf["ws"].data_ptr(), buf["ws"].numel(), stream=stream)


# ---- the spectrum operator ------------------------------------------------------------------------------------------------------
SPECTRUM_FUSED, SPECTRUM_SPLIT = "sdrhip_debug_spectrum_fused_launches", "sdrhip_debug_spectrum_reduce_split_launches"


class Spectrum(Case):
    """sdrhip_spectrum_run_device / sdrhip_spectrum_reduce_run_device on u8 IQ.  Tolerance contract (spectrum_reduce_model.check);
    the gated result is also compared bit for bit with the same call made synchronously.  The hipFFT routes and the reductions through
    layers keep one scratch buffer behind `last_stream`, so a run on another stream than the last may block the host (sdr_hip.h):
    warm_on_stream has the warm-up repeated on the gated stream, and the no-host-synchronisation assertion is made from there."""
    fmt = "u8"

    def __init__(self, name, n, rows, route, seed, group=0, reduce=SR.MEAN_POWER, unit=SR.LINEAR, split=1, counters=None):
        super().__init__(name)
        self.size, self.rows, self.route, self.seed, self.group, self.reduce, self.unit, self.split = n, rows, route, seed, group, reduce, unit, split
        self.n = n * rows * max(group, 1)
        self.tolerance = True
        # the routes through the object's one work buffer promise no host synchronisation only while the stream stays the same: their
        # warm-up is repeated on the gated stream
        self.warm_on_stream = not (route == 1 and group <= 32)
        self.counters = counters or {}
        self.floor_db = -120.0

    def model(self, x):
        if self.group:
            return SR.spectrum_reduce(x, self.size, SM.IQ_U8, SM.WINDOW_HANNING, None, True, 1.0, None, self.rows, self.group, self.reduce)
        mag, _ = SM.spectrum(x, self.size, SM.IQ_U8, SM.WINDOW_HANNING, None, True, 1.0, None, self.rows)
        return mag, 1e-11 * np.max(mag, axis=1, keepdims=True) * np.ones_like(mag)

    def expected(self, oracle, x):
        v, _ = self.model(x)
        return {"out": SR.expected(v, self.reduce, self.unit, self.floor_db).ravel()}

    def check(self, got, exp, what, x=None):
        v, delta = self.model(self.stream(0) if x is None else x)
        SR.check(got, v, delta, self.reduce if self.group else SR.MEAN_MAGNITUDE, self.unit, self.floor_db, what)

    def within(self, got, x):
        """bool per bin: got inside the tolerance of the model on stream x (the CPU file's 'a stray launch would show')"""
        v, delta = self.model(x)
        g = np.asarray(got, np.float64).reshape(v.shape)
        return np.abs(g - v) <= delta + 2.0 ** -23 * np.abs(v)

    def make(self, hip):
        s = hip.Spectrum(self.size, hip.IQ_U8, hip.WINDOW_HANNING, True, 1.0)
        s.set_route(self.route)
        if self.group:
            s.set_reduce_split(self.split)
        return s

    def call(self, hip, obj, stream, p_in, buf):
        if self.group:
            obj.reduce_device(p_in, self.n, buf["out"].data_ptr(), self.group, self.reduce, self.unit, self.floor_db, rows_out=self.rows, stream=stream)
        else:
            obj.run_device(p_in, self.n, buf["out"].data_ptr(), rows=self.rows, stream=stream)


def spectrum_cases():
    return [
        Spectrum("spectrum n = 256, one kernel", 256, 12, 1, 1, counters={SPECTRUM_FUSED: ("==", 1)}),
        Spectrum("spectrum n = 1000, hipFFT route", 1000, 5, 2, 2, counters={SPECTRUM_FUSED: ("==", 0)}),
        Spectrum("spectrum reduce n = 256, group 70: layers + finalise", 256, 3, 1, 3, group=70, split=1,
                 counters={SPECTRUM_FUSED: ("==", 1), SPECTRUM_SPLIT: ("==", 0)}),
        Spectrum("spectrum reduce n = 256, group 70, forced split", 256, 3, 1, 3, group=70, split=2,
                 counters={SPECTRUM_FUSED: ("==", 1), SPECTRUM_SPLIT: ("==", 1)}),
        Spectrum("spectrum reduce n = 1000, group 40, hipFFT route", 1000, 2, 2, 4, group=40, reduce=SR.MEAN_MAGNITUDE,
                 counters={SPECTRUM_FUSED: ("==", 0), SPECTRUM_SPLIT: ("==", 0)}),
    ]


# ---- the table ------------------------------------------------------------------------------------------------------
def _table():
    c = fir_cases()
    c += [OneLaunch(op, fmt, 10 + i) for i, (op, fmt) in enumerate((("fm_demod", "cf32"), ("scale", "f32"), ("convert_u8", "u8"),
                                                                    ("convert_i16", "i16"), ("am_demod", "cf32")))]
    c += [Iir(op, par, 20 + i) for i, (op, par) in enumerate((("dc_blocker", True), ("dc_blocker", False), ("agc", True), ("agc", False)))]
    c += [IirRows(op, par, 24 + i) for i, (op, par) in enumerate((("dc_blocker", True), ("agc", True), ("dc_blocker", False)))]
    c += [IirRows("agc", False, 29)]
    c += [DemodRows("fm_demod", 27), DemodRows("am_demod", 28)]
    by = {x.name: x for x in c}
    for one in ("real symmetric filter 128 taps, fast filter + fix-up", "decimator /8 127 taps cf32, tile kernel + fix-up launch",
                "real resampler 3/10 191 taps"):
        c += [FirRows(by[one], route) for route in (1, 2)]
    c += [Tuner(fmt, 1, 30 + i) for i, fmt in enumerate(("cf32", "u8", "i16"))]
    c += [Tuner("cf32", 1, 33, small=-1), Tuner("cf32", 2, 34), Tuner("u8", 2, 35)]
    c += [TunerBank(fmt, 1, 36 + i) for i, fmt in enumerate(("cf32", "u8", "i16"))]
    c += [TunerBank("u8", 1, 39, small=-1), TunerBank("u8", 2, 40), TunerBank("i16", 2, 41)]
    c += [Chain(route, tuned, 42 + i) for i, (route, tuned) in enumerate((("one kernel", False), ("stage kernels", False), ("fused tail", False),
                                                                         ("one kernel", True), ("stage kernels", True)))]
    c += [Chain("fused tail", True, 52)]
    c += [FmBank(fmt, route, 47 + i) for i, (fmt, route) in enumerate((("u8", 1), ("u8", 2), ("i16", 1), ("i16", 2)))]
    c += spectrum_cases()
    assert len({x.name for x in c}) == len(c)
    return c


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
# the seamed cases whose Cross outputs come from a sequential kernel of their own.  Not among them: the scalar order, whose SIMD order
# IS the sequential order (no Cross output can differ, and its route has no fix-up launch that could be overwritten: the counter says so)
SEAMED = [c for c in CASES if type(c).cross is not Case.cross and getattr(c, "order", AVX) != SCALAR]

# a fresh descriptor's FIRST EVER run is the gated one: tap, table, window and twiddle uploads against a kernel on a non-blocking stream
FIRST_RUN = ["real symmetric filter 128 taps, fast filter + fix-up", "decimator /8 127 taps cf32, tile kernel + fix-up launch",
             "decimator /8 127 taps u8, tile kernel + fix-up launch", "real resampler 3/10 191 taps", "tuner u8, fused route, tile kernel + fix-up launch",
             f"tuner cf32, two-pass route in chunks of {TUNER_CHUNK}", "tuner bank x3 u8, banked launch + fix-up launch", "FM chain, one kernel, tuned",
             "FM chain, stage kernels, untuned", "FM bank x2 u8, banked launch", "FM bank x2 u8, station by station", "spectrum n = 256, one kernel",
             "spectrum n = 1000, hipFFT route"]
# one descriptor, two gated streams from one host thread: S1 (long delay) queued first, S2 (a quarter of it) second, so the device
# runs them in the reverse of call order; the pattern S1, S2, S1 for the tuner and the spectrum operator
TWO_STREAMS = [(f"tuner cf32, two-pass route in chunks of {TUNER_CHUNK}", 3), (f"tuner bank x3 u8, route 2, SSE order: each channel's tuner leases a lane, chunks of {TUNER_CHUNK}", 2),
               ("spectrum n = 1000, hipFFT route", 3), ("spectrum reduce n = 256, group 70: layers + finalise", 2),
               ("decimator /8 127 taps u8, tile kernel + fix-up launch", 2), ("FM bank x2 u8, station by station", 2)]
# the case with the most launches behind one gate: its host queueing time sets the delay
MOST_LAUNCHES = f"tuner bank x3 u8, route 2, SSE order: each channel's tuner leases a lane, chunks of {TUNER_CHUNK}"


# ---- the device side ------------------------------------------------------------------------------------------------------
CANARY_BYTE = 0xA5


class Gate:
    """The session's gate: the streams the control picked, the calibrated delay, the figures for the notebook."""

    def __init__(self, hip):
        import torch
        self.torch, self.hip = torch, hip
        self.cycles_per_ms = self._calibrate_sleep()
        self.delay_ms = DELAY_MIN_MS
        self.queue_ms = None
        self.s1 = self.s2 = None
        self.log = []

    def _calibrate_sleep(self):
        torch = self.torch
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        cycles = 2_000_000
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        assert ms > 0.01, f"torch.cuda._sleep({cycles}) took {ms} ms: the delay cannot be calibrated"
        return cycles / ms

    def sleep(self, ms):
        self.torch.cuda._sleep(int(ms * self.cycles_per_ms))

    def set_delay(self, queue_ms):
        self.queue_ms = queue_ms
        self.delay_ms = min(DELAY_MAX_MS, max(DELAY_MIN_MS, 100.0 * queue_ms))
        self.log.append(f"host queueing time of the case with the most launches: {queue_ms:.3f} ms; delay {self.delay_ms:.1f} ms "
                        f"({self.cycles_per_ms:.0f} sleep cycles per ms)")

    # -- the control: a one-kernel operator queued on ANOTHER stream than the gated one must overtake the gate
    def _control(self, s, other):
        torch, hip = self.torch, self.hip
        import gpu_util as G
        n, f = 1 << 16, 0.2
        real, p1, p2 = (seeded("f32", n, 6900 + i) for i in range(3))
        from oracle.oracle import Oracle
        exp = Oracle().scale(f, real)
        d_real, d_in, d_p2 = G.to_dev(real), G.to_dev(p1), G.to_dev(p2)
        out, snap = G.dev_empty_f32(n), G.dev_empty_f32(n)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            self.sleep(self.delay_ms)
            d_in.copy_(d_real, non_blocking=True)
        hip.check(hip.lib.sdrhip_scale_run(other.cuda_stream if other is not None else None, f, d_in.data_ptr(), out.data_ptr(), n), "control")
        with torch.cuda.stream(s):
            d_in.copy_(d_p2, non_blocking=True)
            snap.copy_(out, non_blocking=True)
        s.synchronize()
        torch.cuda.synchronize()
        return not bool(same_bits(G.to_host(snap), exp).all())

    def pick_streams(self):
        torch = self.torch
        cands = [torch.cuda.Stream() for _ in range(4)]
        for i, s in enumerate(cands):
            if not self._control(s, None):
                self.log.append(f"control: candidate stream {i}: a launch on the null stream did NOT overtake the gate")
                continue
            for j, t in enumerate(cands):
                if j != i and self._control(s, t) and self._control(t, s):
                    self.s1, self.s2 = s, t
                    self.log.append(f"control: gated stream = candidate {i}; a one-kernel operator queued on the null stream and on candidate {j} "
                                    f"overtook the gate (snapshot differs from the expected output), and candidate {i} overtook a gate on {j}")
                    return
            self.log.append(f"control: candidate stream {i}: no second stream overtook the gate")
        raise AssertionError("the gated-stream harness sees nothing: on none of 4 fresh streams did a launch queued on the null stream and on "
                             "a second stream overtake the gate (do the streams share one hardware queue?)\n" + "\n".join(self.log))


def alloc(gate, hip, case, obj, oracle):
    """-> {name: tensor}: outputs between guard bands with canaries, scratch filled with canary bytes, states with their initial values"""
    import gpu_util as G
    torch = gate.torch
    buf = {}
    for name, floats in case.outputs(oracle).items():
        if name not in case.states():
            buf[name] = G.dev_empty_f32(floats)
    for name, nbytes in case.scratch(hip, obj).items():
        buf[name] = torch.full((max(int(nbytes), 16),), CANARY_BYTE, dtype=torch.uint8, device="cuda")
    for name, init in case.states().items():
        st = G.dev_empty_f32(init.size)
        st.copy_(torch.from_numpy(init))
        buf[name] = st
    return buf


def counter_values(hip, case):
    return {k: int(getattr(hip.lib, k)()) for k in case.counters}


def assert_counters(case, before, after, calls=1):
    for k, (op, v) in case.counters.items():
        moved = after[k] - before[k]
        ok = moved == v * calls if op == "==" else moved >= v * calls
        assert ok, f"{case.name}: {k} moved by {moved} over {calls} call(s), expected {op} {v} per call"


def sync_run(gate, hip, case, obj, oracle, d_real):
    """The same call made synchronously on the null stream on the real input: the warm-up, the counters, the reference device result."""
    import gpu_util as G
    torch = gate.torch
    buf = alloc(gate, hip, case, obj, oracle)
    d_in = d_real.clone()
    torch.cuda.synchronize()
    before = counter_values(hip, case)
    if hasattr(case, "sync_begin"):
        case.sync_begin(hip, obj)
    case.call(hip, obj, None, d_in.data_ptr(), buf)
    torch.cuda.synchronize()
    if hasattr(case, "sync_end"):
        case.sync_end(hip, obj)
    assert_counters(case, before, counter_values(hip, case))
    if hasattr(case, "after"):
        case.after(hip, buf)
    return {k: G.to_host(buf[k]).copy() for k in case.outputs(oracle)}


def warm_run(gate, hip, case, obj, oracle, stream, d_real):
    """One more run of the same shape on `stream`, then a synchronised device: for the cases whose promise holds while the stream stays."""
    buf = alloc(gate, hip, case, obj, oracle)
    d_in = d_real.clone()
    gate.torch.cuda.synchronize()
    case.call(hip, obj, stream.cuda_stream, d_in.data_ptr(), buf)
    gate.torch.cuda.synchronize()


class Queued:
    """One gated run, queued: finish() waits for its stream and returns the snapshots."""

    def __init__(self, gate, stream, snaps, busy, queue_ms, buf):
        self.gate, self.stream, self.snaps, self.busy, self.queue_ms, self.buf = gate, stream, snaps, busy, queue_ms, buf

    def finish(self):
        import gpu_util as G
        self.stream.synchronize()
        return {k: G.to_host(v).copy() for k, v in self.snaps.items()}


def gated_run(gate, hip, case, obj, oracle, stream=None, delay_ms=None, prepared=None, record=None, wait=None):
    """Queue one gated run of `case` on `stream` (default: the session's gated stream) -> Queued.  prepared = what prepare() returned
    on a synchronised device, so that several gated runs can be queued back to back.  record: an event recorded on the stream when
    the gate has opened and the real input is in place; wait: open this run's gate on such an event of another stream instead of
    on a delay of its own, so that the two operators start together."""
    torch = gate.torch
    stream = stream or gate.s1
    delay_ms = gate.delay_ms if delay_ms is None else delay_ms
    buf, d_in, snaps, d_real, d_p2 = prepared
    with torch.cuda.stream(stream):
        if wait is not None:
            stream.wait_event(wait)
        else:
            gate.sleep(delay_ms)
        t0 = time.perf_counter()
        d_in.copy_(d_real, non_blocking=True)
        if record is not None:
            record.record(stream)
        case.call(hip, obj, stream.cuda_stream, d_in.data_ptr(), buf)
        busy = not stream.query()
        d_in.copy_(d_p2, non_blocking=True)
        for k, s in snaps.items():
            s.copy_(buf[k], non_blocking=True)
        queue_ms = (time.perf_counter() - t0) * 1e3
    return Queued(gate, stream, snaps, busy, queue_ms, buf)


def prepare(gate, hip, case, obj, oracle, real=None):
    """On a synchronised device: d_in with poison, canaried outputs and snapshots, canary-filled scratch, states."""
    import gpu_util as G
    torch = gate.torch
    real = case.stream(0) if real is None else real
    d_real, d_in, d_p2 = G.to_dev(real), G.to_dev(case.stream(1)), G.to_dev(case.stream(2))
    buf = alloc(gate, hip, case, obj, oracle)
    snaps = {k: G.dev_empty_f32(v) for k, v in case.outputs(oracle).items()}
    torch.cuda.synchronize()
    return buf, d_in, snaps, d_real, d_p2
