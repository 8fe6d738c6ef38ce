"""GPU parity of the AM bank's Pipe (sdrhip_pipe_am_bank): host cfloat / u8 / int16 IQ blocks in, every channel's audio blocks out.
Every channel's blocks are compared, bit for bit over the whole stream, against the model (tests/pipe_am_bank_cases.py: the restated
Pipe on the mixed stream at the pushes' own boundaries, magnitude, the oracle's dcBlocker), which is independent of the product.  Every
pop goes into a buffer of NaN canaries whose words around each row must be canaries afterwards.
Shape: 127 taps (128 prepared), factor 8, AVX order, the tables of the tuner bank's tests."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import pipe_am_bank_cases as PC
import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
from conftest import assert_bit_equal
from gpu_util import CANARY

pytestmark = pytest.mark.gpu

B, LP, D = PC.B, PC.LP, PC.D
NBLK = 19                                      # 19 blocks: two submissions of 16 coalesced blocks, seven of 3
_f32p = C.POINTER(C.c_float)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PUSH = {"cf32": ("sdrhip_pipe_push", _f32p), "u8": ("sdrhip_pipe_push_u8", C.POINTER(C.c_uint8)), "i16": ("sdrhip_pipe_push_i16", C.POINTER(C.c_int16))}


def tables_for(nch):
    return [T.osc_table(1000), T.osc_table(5)] if nch == 2 else BC.bank_tables(nch)


def am_bank(hip, tables, dc=True, factor=8, taps=None):
    return hip.AmBank(hip.TunerBank(factor, S.taps_decim127() if taps is None else taps, tables), dc_block=dc)


class AmPipe:
    """The Pipe through the raw C calls: every pop goes into canaries and the words around each row are checked."""

    def __init__(self, hip, am, block_out, fmt):
        self.hip, self.bo, self.fmt = hip, block_out, fmt
        self.p = hip.Pipe.am_bank(am, block_out, input_u8=fmt == "u8", input_i16=fmt == "i16")
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []

    def _pop(self, ready):
        self.counts.append(ready)
        if ready <= 0:
            return
        n, gap = ready * self.bo, 5
        stride = n + gap
        buf = np.full(8 + self.rows * stride, CANARY, np.uint32)
        out = buf[8:].view(np.float32)
        nb = self.hip.check(self.hip.lib.sdrhip_pipe_pop_rows(self.p.h, out.ctypes.data_as(_f32p), stride, ready), "sdrhip_pipe_pop_rows")
        assert nb == ready
        r = buf[8:].reshape(self.rows, stride)
        assert (buf[:8] == CANARY).all() and (r[:, n:] == CANARY).all(), "a pop wrote outside its rows"
        for j in range(self.rows):
            self.got[j].append(r[j, :n].copy())

    def push(self, blk, via_buffer=False):
        name, ptr_t = PUSH[self.fmt]
        n = blk.size // 2
        if via_buffer:
            view = self.p.input_buffer(n)
            view[:] = blk
            blk = view
        else:
            blk = np.ascontiguousarray(blk)
        self._pop(self.hip.check(getattr(self.hip.lib, name)(self.p.h, blk.ctypes.data_as(ptr_t), n), name))

    def flush(self):
        self._pop(self.hip.check(self.hip.lib.sdrhip_pipe_flush(self.p.h), "sdrhip_pipe_flush"))

    def restore(self, state):
        self._pop(self.hip.check(self.hip.lib.sdrhip_pipe_restore(self.p.h, state, C.c_size_t(len(state))), "sdrhip_pipe_restore"))

    def row(self, j):
        return np.concatenate(self.got[j]).view(np.float32) if self.got[j] else np.empty(0, np.float32)


def counters(hip):
    """(envelope tile, all-Cross envelope, amDemod, banked tuner, all-Cross tuner) launches"""
    return np.array([hip.am_bank_launches(), hip.am_bank_cross_launches(), hip.lib.sdrhip_debug_am_demod_launches(),
                     hip.tuner_bank_launches(), hip.tuner_bank_cross_launches()])


def check_rows(oracle, ap, tables, fmt, sizes, dc, nsamples, what, **kw):
    for j, t in enumerate(tables):
        exp = PC.expected(oracle, t, fmt, sizes, dc, nsamples, **kw)
        got = ap.row(j)
        assert got.size > 0 and got.size % ap.bo == 0 and got.size <= exp.size
        assert_bit_equal(got, exp[:got.size], f"{what}: channel {j} against the model")


# ---- uniform pushes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3, 16])
@pytest.mark.parametrize("nch", [1, 2, 3, 32])
def test_uniform_pushes(hip, oracle, nch, group):
    """`group` 8192-sample blocks per submission, the three input types, block_size_out 1000 and 1024: exactly one envelope tile launch
    per submission, no all-Cross launch, no amDemod and no tuner bank launch."""
    tables = tables_for(nch)
    sizes = [B] * NBLK
    for fmt in PC.FORMATS:
        blocks = PC.cut(PC.stream(fmt, NBLK * B), sizes)
        for bo in (1000, 1024):
            ap = AmPipe(hip, am_bank(hip, tables), bo, fmt)
            assert ap.rows == nch
            ap.p.set_adaptive(0)
            if group > 1:
                ap.p.set_coalesce(group)
            c0 = counters(hip)
            for blk in blocks:
                ap.push(blk)
            ap.flush()
            what = f"{nch} channels, {group} blocks per submission, {fmt}, block_size_out {bo}"
            assert tuple(counters(hip) - c0) == (-(-NBLK // group), 0, 0, 0, 0), what
            assert sum(ap.counts) == ap.row(0).size // bo == ((NBLK * B - LP) // D + 1) // bo, what + ": blocks per channel"
            check_rows(oracle, ap, tables, fmt, sizes, True, NBLK * B, what)


# ---- ragged pushes -----------------------------------------------------------------------------------------------------------------
def ragged_sizes(n=20, seed=5):
    """Three equal blocks (so that coalescing has something to stage), then seeded sizes in [LP, 3 B], odd ones included."""
    rng = np.random.default_rng(seed)
    return [B, B, B] + [int(v) for v in rng.integers(LP, 3 * B + 1, n)]


@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
@pytest.mark.parametrize("fmt", PC.FORMATS)
def test_ragged_pushes(hip, oracle, fmt, mode):
    """Per ragged submission ONE all-Cross envelope launch and ONE envelope tile launch for all channels; every third push goes
    through input_buffer."""
    sizes = ragged_sizes()
    total = 28 * B
    assert sum(sizes) <= total and any(s % 2 for s in sizes[3:])
    tables = tables_for(3)
    ap = AmPipe(hip, am_bank(hip, tables), 1000, fmt)
    if mode == "plain":
        ap.p.set_adaptive(0)
    elif mode == "coalesce 7":
        ap.p.set_coalesce(7)
    else:
        ap.p.set_adaptive(32)
    blocks = PC.cut(PC.stream(fmt, total), sizes)
    for i, blk in enumerate(blocks[:3]):
        ap.push(blk, via_buffer=(i == 1))
    c0 = counters(hip)
    ap.push(blocks[3])                                  # ends the uniform run: what is still staged goes out, then the ragged block
    c1 = counters(hip)
    assert c1[1] - c0[1] == 1 and 1 <= c1[0] - c0[0] <= 2 and (c1[2:] == c0[2:]).all(), mode
    for i, blk in enumerate(blocks[4:]):
        ap.push(blk, via_buffer=(i % 3 == 0))
        c2 = counters(hip)
        assert tuple(c2 - c1) == (1, 1, 0, 0, 0), f"{mode}: ragged push {i + 4} of {blk.size // 2} samples"
        c1 = c2
    ap.flush()
    assert (counters(hip) == c1).all(), "flush launched although nothing was staged"
    check_rows(oracle, ap, tables, fmt, sizes, True, total, f"ragged pushes, {mode}, {fmt}")


# ---- ordering ----------------------------------------------------------------------------------------------------------------------
def test_two_hundred_pushes_in_flight_keep_the_dc_blocker_in_order(hip, oracle):
    """200 one-block pushes of 1024 samples made as fast as the host can (four submissions in flight, results popped only at the
    end of each push): dcBlocker of submission i starts from the state submission i - 1 left on the device."""
    n, nb = 1024, 200
    tables = tables_for(3)
    sizes = [n] * nb
    for fmt in ("u8", "cf32"):
        ap = AmPipe(hip, am_bank(hip, tables), 128, fmt)
        ap.p.set_adaptive(0)
        c0 = counters(hip)
        for blk in PC.cut(PC.stream(fmt, nb * n), sizes):
            ap.push(blk)
        ap.flush()
        assert tuple(counters(hip) - c0) == (nb, 0, 0, 0, 0)
        check_rows(oracle, ap, tables, fmt, sizes, True, nb * n, f"200 pushes, {fmt}")


# ---- no output ---------------------------------------------------------------------------------------------------------------------
def test_pushes_without_an_output_launch_nothing(hip, oracle):
    tables = tables_for(3)
    for fmt in PC.FORMATS:
        s = PC.stream(fmt, NBLK * B)
        ap = AmPipe(hip, am_bank(hip, tables), 1000, fmt)
        ap.p.set_coalesce(4)                                 # three pushes are staged: no submission, no launch
        c0 = counters(hip)
        for blk in PC.cut(s, [B, B, B]):
            ap.push(blk)
        assert (counters(hip) == c0).all() and ap.counts == [0, 0, 0]
        ap.flush()
        assert tuple(counters(hip) - c0) == (1, 0, 0, 0, 0)
        c1 = counters(hip)
        name, ptr_t = PUSH[fmt]
        short = np.ascontiguousarray(s[:2 * (LP - 1)])
        assert getattr(hip.lib, name)(ap.p.h, short.ctypes.data_as(ptr_t), LP - 1) == -1
        assert b"shorter than the filter" in hip.lib.sdrhip_last_error()
        assert (counters(hip) == c1).all()
        ap.p.set_coalesce(0)
        ap.p.set_adaptive(0)
        ap.push(s[2 * 3 * B:2 * 4 * B])
        ap.flush()
        check_rows(oracle, ap, tables, fmt, [B] * 4, True, NBLK * B, f"after a refused push, {fmt}")


# ---- calls -------------------------------------------------------------------------------------------------------------------------
def test_the_wrong_push_call_is_refused(hip):
    am = am_bank(hip, tables_for(2))
    data = {f: np.ascontiguousarray(PC.stream(f, B)) for f in PC.FORMATS}
    c0 = counters(hip)
    for fmt in PC.FORMATS:
        p = hip.Pipe.am_bank(am, 1000, input_u8=fmt == "u8", input_i16=fmt == "i16")
        for other in PC.FORMATS:
            if other == fmt:
                continue
            name, ptr_t = PUSH[other]
            assert getattr(hip.lib, name)(p.h, data[other].ctypes.data_as(ptr_t), B) == -1, f"{other} blocks into a {fmt} pipe"
            assert name.encode() + b":" in hip.lib.sdrhip_last_error()
            with pytest.raises(hip.SdrHipError):
                p.push(data[other])
        assert p.flush() == []
    assert (counters(hip) == c0).all()


def test_pop_against_pop_rows(hip, oracle):
    blocks = PC.cut(PC.stream("cf32", NBLK * B), [B] * 4)
    t1 = tables_for(1)
    p = hip.Pipe.am_bank(am_bank(hip, t1), 1000)
    p.set_adaptive(0)
    assert p.rows == 1
    for blk in blocks:
        hip.check(hip.lib.sdrhip_pipe_push(p.h, np.ascontiguousarray(blk).ctypes.data_as(_f32p), B), "push")
    ready = hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush")
    assert ready == 4
    got = []
    for k in range(ready):
        if k % 2:
            got.append(p.pop_rows(1).reshape(-1))
        else:
            o = np.empty(1000, np.float32)
            assert hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(_f32p), 1000) == 1000
            got.append(o)
    assert_bit_equal(np.concatenate(got), PC.expected(oracle, t1[0], "cf32", [B] * 4, True, NBLK * B)[:4000], "pop and pop_rows, one channel")
    # three rows: pop is refused and pops nothing; a short row_stride is refused with nothing written
    tables = tables_for(3)
    q = hip.Pipe.am_bank(am_bank(hip, tables), 1000)
    q.set_adaptive(0)
    for blk in blocks:
        hip.check(hip.lib.sdrhip_pipe_push(q.h, np.ascontiguousarray(blk).ctypes.data_as(_f32p), B), "push")
    assert hip.check(hip.lib.sdrhip_pipe_flush(q.h), "flush") == 4
    o = np.full(3 * 4000, CANARY, np.uint32)
    assert hip.lib.sdrhip_pipe_pop(q.h, o.view(np.float32).ctypes.data_as(_f32p), 4000) == -1
    assert b"sdrhip_pipe_pop" in hip.lib.sdrhip_last_error() and (o == CANARY).all()
    assert hip.lib.sdrhip_pipe_pop_rows(q.h, o.view(np.float32).ctypes.data_as(_f32p), 4 * 1000 - 1, 4) == -1
    assert b"sdrhip_pipe_pop_rows" in hip.lib.sdrhip_last_error() and (o == CANARY).all()
    assert hip.check(hip.lib.sdrhip_pipe_poll(q.h), "poll") == 4, "a refused pop took blocks"
    rows = q.pop_rows(4)
    assert rows.shape == (3, 4, 1000)
    for j, t in enumerate(tables):
        assert_bit_equal(rows[j].reshape(-1), PC.expected(oracle, t, "cf32", [B] * 4, True, NBLK * B)[:4000], f"pop_rows: channel {j}")


# ---- save / restore ----------------------------------------------------------------------------------------------------------------
def test_save_and_restore(hip, oracle):
    """Save after 5 of 40 pushes (2048-sample blocks) and restore over a second pipe: the rest of the stream is the model's; every
    refusal leaves the pipe unchanged."""
    tables = tables_for(3)
    taps = S.taps_decim127()
    sizes = [2048] * 40
    for fmt in PC.FORMATS:
        kw = dict(input_u8=fmt == "u8", input_i16=fmt == "i16")
        am = am_bank(hip, tables)
        blocks = PC.cut(PC.stream(fmt, 40 * 2048), sizes)
        a = AmPipe(hip, am, 1000, fmt)
        for blk in blocks[:5]:
            a.push(blk)
        state = a.p.save()
        b = AmPipe(hip, am, 1000, fmt)

        def refused(pipe, st, what):
            assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
            assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what

        refused(b.p, state[:-1], "a truncated state")
        refused(b.p, state[:-25], "a state cut inside its dcBlocker floats")
        refused(b.p, state[:60], "a state cut inside its header")
        refused(hip.Pipe.am_bank(am_bank(hip, tables[:2]), 1000, **kw), state, "another row count")
        other = dict(input_u8=fmt != "u8", input_i16=False)
        refused(hip.Pipe.am_bank(am, 1000, **other), state, "another input type")
        refused(hip.Pipe.am_bank(am, 1024, **kw), state, "another block_size_out")
        refused(hip.Pipe.am_bank(am_bank(hip, tables, factor=16), 1000, **kw), state, "another factor")
        refused(hip.Pipe.am_bank(am_bank(hip, tables, taps=S.gauss_taps(64, 104)), 1000, **kw), state, "another tap count")
        refused(hip.Pipe.am_bank(am_bank(hip, tables, dc=False), 1000, **kw), state, "another dc_block")
        tb = hip.Pipe.tuner_bank(am.tuner_bank, 1000, **kw)
        refused(tb, state, "another kind")
        tb.push(blocks[0])
        refused(b.p, tb.save(), "a tuner bank pipe's state")
        assert hip.lib.sdrhip_pipe_poll(b.p.h) == 0
        b.restore(state)                                     # ... and after all those refusals the pipe is as fresh as it was
        for blk in blocks[5:]:
            a.push(blk)
            b.push(blk)
        a.flush()
        b.flush()
        check_rows(oracle, a, tables, fmt, sizes, True, 40 * 2048, f"the saved pipe, {fmt}")
        nb_before = sum(a.counts[:5])
        for j in range(3):
            assert_bit_equal(b.row(j), a.row(j)[nb_before * 1000:], f"restored pipe, {fmt}: channel {j}")


def test_saved_states_of_every_existing_kind_keep_their_bytes(hip):
    states = PC.existing_kind_states(hip)
    assert set(states) == set(PC.PARENT_STATE_SHA256) and len(states) == 9
    for kind, st in states.items():
        assert hashlib.sha256(st).hexdigest() == PC.PARENT_STATE_SHA256[kind], f"the saved state of a {kind} pipe changed"


# ---- no dcBlocker ------------------------------------------------------------------------------------------------------------------
def test_without_dc_block_the_rows_are_the_envelope(hip, oracle):
    tables = tables_for(3)
    for fmt in PC.FORMATS:
        for sizes, total in (([B] * NBLK, NBLK * B), (ragged_sizes(), 28 * B)):
            ap = AmPipe(hip, am_bank(hip, tables, dc=False), 1000, fmt)
            ap.p.set_adaptive(0)
            for blk in PC.cut(PC.stream(fmt, total), sizes):
                ap.push(blk)
            ap.flush()
            check_rows(oracle, ap, tables, fmt, sizes, False, total, f"dc_block 0, {fmt}, {'uniform' if sizes[3] == B else 'ragged'}")


def test_a_bank_the_fused_launch_does_not_serve(hip, oracle):
    """Factor 5 has no tile kernel: the Pipe goes through the tuner bank and amDemod's rows form, same model."""
    tables = tables_for(2)
    am = hip.AmBank(hip.TunerBank(5, S.taps_decim127(), tables), dc_block=True)
    sizes = [4000, 4000, 4000, 5001, 2999]
    ap = AmPipe(hip, am, 200, "u8")
    ap.p.set_adaptive(0)
    c0 = counters(hip)
    for blk in PC.cut(PC.stream("u8", 20000), sizes):
        ap.push(blk)
    ap.flush()
    d = counters(hip) - c0
    assert d[0] == 0 and d[2] == len(sizes)
    check_rows(oracle, ap, tables, "u8", sizes, True, 20000, "factor 5", factor=5)


# ---- the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [[], ["--no-dc"], ["--s16"], ["--s16", "--no-dc"]])
def test_airband_replay_example(hip, args, tmp_path):
    """examples/airband_replay.c against the same Pipe driven from the binding: one f32 file per channel."""
    exe = os.path.join(ROOT, "examples", "bin", "airband_replay")
    assert os.path.exists(exe), "build() makes the examples"
    fmt = "i16" if "--s16" in args else "u8"
    s = PC.stream(fmt, 6 * B)
    cap, tp = tmp_path / "capture.bin", tmp_path / "taps.f32"
    s.tofile(cap)
    S.taps_decim127().tofile(tp)
    chans = [(1, 64), (-3, 64), (0, 1)]
    r = subprocess.run([exe, str(cap), str(tp), str(tmp_path / "out"), "--channels", ",".join(f"{a}/{b}" for a, b in chans)] + args,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tables = [hip.tuner_shift_table(a, b) for a, b in chans]
    am = hip.AmBank(hip.TunerBank(8, S.taps_decim127(), tables), dc_block="--no-dc" not in args)
    p = hip.Pipe.am_bank(am, 1024, input_u8=fmt == "u8", input_i16=fmt == "i16")
    outs = []
    for blk in PC.cut(s, [B] * 6):
        outs += p.push(blk)
    outs += p.flush()
    want = np.concatenate(outs, axis=1)
    assert want.shape == (3, ((6 * B - LP) // D + 1) // 1024 * 1024)
    for j in range(3):
        got = np.fromfile(str(tmp_path / f"out.ch{j}.f32"), np.float32)
        assert_bit_equal(got, want[j], f"airband_replay {' '.join(args)}: channel {j}")
