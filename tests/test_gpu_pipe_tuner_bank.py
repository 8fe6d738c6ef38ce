"""GPU parity of the tuner bank's Pipe (sdrhip_pipe_tuner_bank): host cfloat / u8 IQ blocks in, every channel's blocks out.

The definition is the expected value everywhere: row j equals, bit for bit, the blocks of a one-row Pipe.tuner over
Tuner(factor, taps, tables[j]) of the same block_size_out fed the same blocks at the same boundaries (a u8 pipe's twin is fed
(u - 128) / 128 as float32, which is exact).  For two channels the rows are also held to the restated Pipe on the mixed stream
(tests/tuner_model.py + oracle/pipes_model.py), which is independent of the product.  Everything is compared as uint32, and every
pop goes into a buffer of NaN canaries whose words around each row must be canaries afterwards.

Shape: 127 taps (128 prepared), factor 8, AVX order, 8192-sample blocks, block_size_out 1000 and 1024, the tables of the bank's own
tests (tests/tuner_bank_cases.py: neighbours never share a period; the {1, 0} table and the subnormal / -0 table among them).

What the issue asked for and this shape cannot show: a ragged submission with m_split == m_done.  m_done = floor((E - Lp) / D) + 1
and m_split = ceil(E / D) for a boundary at sample E; with Lp > D (every shape the banked kernel serves: 128 > 8) m_done <
m_split always -- 15 Cross outputs where 8 divides E, 16 elsewhere.  The branch is reached with a filter shorter than the
decimation step (8 taps / 16), which test_ragged_pushes_without_a_cross_part does; the 127-tap series asserts that both Cross
counts (15, and the maximum 16) occurred."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import numpy as np
import pytest

import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import CANARY
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, LP, D = 8192, 128, 8
NBLK = 19                                      # 19 blocks: two submissions of 16 coalesced blocks, seven of 3
_f32p = C.POINTER(C.c_float)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_cache = {}


def stream_u8(nsamples=NBLK * B):
    """Seeded u8 IQ with 127 / 128 / 129 forced into a few dozen positions, block edges included (128 converts to +0)."""
    key = ("u8", nsamples)
    if key not in _cache:
        rng = np.random.default_rng(20240607)
        u = rng.integers(0, 256, 2 * nsamples, dtype=np.uint8)
        pos = np.concatenate([rng.integers(0, 2 * nsamples, 48), np.arange(2 * B - 4, 2 * B + 4)])
        u[pos] = rng.integers(127, 130, pos.size).astype(np.uint8)
        u.setflags(write=False)
        _cache[key] = u
    return _cache[key]


def to_f32(u8):
    return (u8.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0)       # exact: sdr_hip.h


def tables_for(nch):
    return [T.osc_table(1000), T.osc_table(5)] if nch == 2 else BC.bank_tables(nch)


def cut(u8, sizes):
    """The stream as blocks of these sizes (samples)."""
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] * 2 <= u8.size
    return [u8[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:])]


def one_row_expected(hip, table, sizes, block_out, factor=8, taps=None, order=PM.ORDER_AVX, u8=None, state=None):
    """The definition: Pipe.tuner over a Tuner with this table, fed the float blocks (computed once per case, shared, never
    written).  state: restore it first (not cached)."""
    u8 = stream_u8() if u8 is None else u8
    taps = S.taps_decim127() if taps is None else taps
    key = ("exp", np.asarray(table, np.float32).tobytes(), tuple(int(s) for s in sizes), block_out, factor, taps.tobytes(), order, u8.tobytes()[:64],
           u8.size)
    if state is None and key in _cache:
        return _cache[key]
    p = hip.Pipe.tuner(hip.Tuner(factor, taps, table, order), block_out)
    p.set_adaptive(0)
    outs = list(p.restore(state)) if state is not None else []
    for blk in cut(u8, sizes):
        outs += p.push(to_f32(blk))
    outs += p.flush()
    e = np.concatenate(outs) if outs else np.empty(0, np.float32)
    e.setflags(write=False)
    if state is None:
        _cache[key] = e
    return e


class BankPipe:
    """The bank's Pipe through the raw C calls: every pop goes into canaries and the words around each row are checked."""

    def __init__(self, hip, bank, block_out, u8):
        self.hip, self.bo, self.u8 = hip, block_out, u8
        self.p = hip.Pipe.tuner_bank(bank, block_out, input_u8=u8)
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []                                   # blocks per channel each call returned

    def _pop(self, ready):
        self.counts.append(ready)
        if ready <= 0:
            return
        n, gap = ready * 2 * self.bo, 6
        stride = n + gap
        buf = np.full(8 + self.rows * stride, CANARY, np.uint32)
        out = buf[8:].view(np.float32)
        nb = self.hip.check(self.hip.lib.sdrhip_pipe_pop_rows(self.p.h, out.ctypes.data_as(_f32p), stride, ready), "sdrhip_pipe_pop_rows")
        assert nb == ready
        r = buf[8:].reshape(self.rows, stride)
        assert (buf[:8] == CANARY).all() and (r[:, n:] == CANARY).all(), "a pop wrote outside its rows"
        assert not (r[:, :n] == CANARY).all(axis=1).any(), "a popped row was not written"
        for j in range(self.rows):
            self.got[j].append(r[j, :n].copy())

    def push(self, blk, via_buffer=False):
        if via_buffer:
            view = self.p.input_buffer(blk.size // 2)
            assert view.dtype == (np.uint8 if self.u8 else np.float32)
            view[:] = blk if self.u8 else to_f32(blk)
            if self.u8:
                rc = self.hip.lib.sdrhip_pipe_push_u8(self.p.h, view.ctypes.data_as(C.POINTER(C.c_uint8)), blk.size // 2)
            else:
                rc = self.hip.lib.sdrhip_pipe_push(self.p.h, view.ctypes.data_as(_f32p), blk.size // 2)
        elif self.u8:
            b = np.ascontiguousarray(blk)
            rc = self.hip.lib.sdrhip_pipe_push_u8(self.p.h, b.ctypes.data_as(C.POINTER(C.c_uint8)), b.size // 2)
        else:
            f = to_f32(blk)
            rc = self.hip.lib.sdrhip_pipe_push(self.p.h, f.ctypes.data_as(_f32p), f.size // 2)
        self._pop(self.hip.check(rc, "push"))

    def flush(self):
        self._pop(self.hip.check(self.hip.lib.sdrhip_pipe_flush(self.p.h), "sdrhip_pipe_flush"))

    def restore(self, state):
        self._pop(self.hip.check(self.hip.lib.sdrhip_pipe_restore(self.p.h, state, C.c_size_t(len(state))), "sdrhip_pipe_restore"))

    def row(self, j):
        return np.concatenate(self.got[j]).view(np.float32) if self.got[j] else np.empty(0, np.float32)


def counters(hip):
    return np.array([hip.tuner_bank_launches(), hip.tuner_bank_cross_launches(), hip.tuner_fused_launches()])


def check_rows(hip, bp, tables, sizes, block_out, what, **kw):
    for j, t in enumerate(tables):
        exp = one_row_expected(hip, t, sizes, block_out, **kw)
        assert exp.size > 0
        assert_bit_equal(bp.row(j), exp, f"{what}: channel {j} vs its one-row Pipe.tuner")


# ---- the definition ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3, 16])
@pytest.mark.parametrize("nch", [1, 2, 3, 32])
def test_definition(hip, oracle, nch, group):
    """`group` 8192-sample blocks per submission (set_coalesce; 1: every push), cfloat and u8, block_size_out 1000 and 1024: exactly
    one banked launch per submission, none of the tuners' own, no cross launch.  One channel is banked by force (auto sends one
    channel to its tuner: tests/test_gpu_tuner_bank.py)."""
    tables = tables_for(nch)
    sizes = [B] * NBLK
    blocks = cut(stream_u8(), sizes)
    for u8 in (False, True):
        for bo in (1000, 1024):
            bank = hip.TunerBank(8, S.taps_decim127(), tables)
            if nch == 1:
                bank.set_route(bank.ROUTE_BANKED)
            bp = BankPipe(hip, bank, bo, u8)
            assert bp.rows == nch
            bp.p.set_adaptive(0)
            if group > 1:
                bp.p.set_coalesce(group)
            c0 = counters(hip)
            for blk in blocks:
                bp.push(blk)
            bp.flush()
            what = f"{nch} channels, {group} blocks per submission, {'u8' if u8 else 'cfloat'}, block_size_out {bo}"
            assert tuple(counters(hip) - c0) == (-(-NBLK // group), 0, 0), what + ": (banked, cross, tuners' own) launches"
            assert sum(bp.counts) == bp.row(0).size // (2 * bo) == ((NBLK * B - LP) // D + 1) // bo, what + ": blocks per channel"
            check_rows(hip, bp, tables, sizes, bo, what)
            if nch == 2 and group == 3 and bo == 1000:
                x = to_f32(stream_u8())
                for j, t in enumerate(tables):
                    m = TM.mix(x, t)
                    model = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=8)
                    out, _ = PM.fir_decimator_pipe(model, [m[2 * B * i:2 * B * (i + 1)] for i in range(NBLK)], bo)
                    assert_bit_equal(bp.row(j), np.concatenate(out), what + f": channel {j} vs the restated Pipe")


# ---- ragged pushes -----------------------------------------------------------------------------------------------------------------
def ragged_sizes(lo=LP, hi=3 * B, n=20, seed=5):
    """Three equal blocks (so that coalescing has something to stage), then seeded sizes in [lo, hi], odd ones included."""
    rng = np.random.default_rng(seed)
    return [B, B, B] + [int(v) for v in rng.integers(lo, hi + 1, n)]


def cross_counts(sizes, lp=LP, d=D):
    """fir_submit's arithmetic restated: Cross outputs of the submission of each block (index 0: none, nothing precedes it)."""
    out, e = [], 0
    for n in sizes:
        m_done = (e - lp) // d + 1 if e >= lp else 0
        m_split = max(-(-e // d), m_done)
        out.append(m_split - m_done)
        e += n
    return out


@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
@pytest.mark.parametrize("u8", [False, True], ids=["cfloat", "u8"])
def test_ragged_pushes(hip, oracle, u8, mode):
    """Per ragged submission: ONE cross launch for all channels and ONE banked launch, none of the tuners' own -- odd sizes
    included, because the copy lands where the banked launch's first window is 16-byte aligned.  Every third push goes through
    input_buffer."""
    sizes = ragged_sizes()
    big = stream_u8(28 * B)
    assert sum(sizes) <= 28 * B and any(s % 2 for s in sizes[3:]) and any(s % 8 == 0 for s in sizes[3:-1])
    ncross = cross_counts(sizes)
    ragged = ncross[3:]
    assert min(ragged) == 15 and max(ragged) == 16 == -(-LP // D), "the seed shows both Cross counts, the maximal one included"
    tables = tables_for(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    bp = BankPipe(hip, bank, 1000, u8)
    if mode == "plain":
        bp.p.set_adaptive(0)
    elif mode == "coalesce 7":
        bp.p.set_coalesce(7)
    else:
        bp.p.set_adaptive(32)
    blocks = cut(big, sizes)
    for i, blk in enumerate(blocks[:3]):
        bp.push(blk, via_buffer=(i == 1))
    c0 = counters(hip)
    bp.push(blocks[3])                                  # ends the uniform run: what is still staged goes out, then the ragged block
    c1 = counters(hip)
    assert c1[1] - c0[1] == 1 and c1[2] == c0[2] and 1 <= c1[0] - c0[0] <= 2, mode
    for i, blk in enumerate(blocks[4:]):
        bp.push(blk, via_buffer=(i % 3 == 0))
        c2 = counters(hip)
        assert tuple(c2 - c1) == (1, 1, 0), f"{mode}: ragged push {i + 4} of {blk.size // 2} samples: (banked, cross, tuners' own) launches"
        c1 = c2
    bp.flush()
    assert (counters(hip) == c1).all(), "flush launched although nothing was staged"
    check_rows(hip, bp, tables, sizes, 1000, f"ragged pushes, {mode}, {'u8' if u8 else 'cfloat'}", u8=big)
    if not u8 and mode == "plain":
        x = to_f32(big)
        for j, t in enumerate(tables[:2]):
            m = TM.mix(x, t)
            edges = np.concatenate([[0], np.cumsum(sizes)])
            model = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=8)
            out, _ = PM.fir_decimator_pipe(model, [m[2 * a:2 * b] for a, b in zip(edges[:-1], edges[1:])], 1000)
            assert_bit_equal(bp.row(j), np.concatenate(out), f"ragged pushes: channel {j} vs the restated Pipe")


def test_ragged_pushes_without_a_cross_part(hip):
    """8 taps / 16: where a boundary E has E mod 16 in [8, 15] no output straddles it (m_split == m_done) and the submission
    launches no cross kernel; elsewhere it launches one.  (No banked kernel serves this shape: the One part goes channel by channel.)"""
    taps = S.gauss_taps(8, 48)
    sizes = [B, 8200, 8195, 8192 + 9, 8192 + 7, 4099, 8192 + 12]
    ncross = cross_counts(sizes, lp=8, d=16)
    assert 0 in ncross[1:] and 1 in ncross[1:]
    tables = tables_for(3)
    bank = hip.TunerBank(16, taps, tables)
    for u8 in (False, True):
        bp = BankPipe(hip, bank, 100, u8)
        bp.p.set_adaptive(0)
        for i, blk in enumerate(cut(stream_u8(), sizes)):
            c0 = counters(hip)
            bp.push(blk)
            d = counters(hip) - c0
            assert d[0] == 0 and d[1] == (1 if i > 0 and ncross[i] > 0 else 0), f"push {i}: {ncross[i]} Cross outputs"
        bp.flush()
        check_rows(hip, bp, tables, sizes, 100, f"8 taps / 16, {'u8' if u8 else 'cfloat'}", factor=16, taps=taps)


# ---- no output ---------------------------------------------------------------------------------------------------------------------
def test_pushes_without_an_output_launch_nothing(hip):
    tables = tables_for(3)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    u = stream_u8()
    for u8 in (False, True):
        bp = BankPipe(hip, bank, 1000, u8)
        bp.p.set_coalesce(4)                                 # three pushes are staged: no submission, no launch
        c0 = counters(hip)
        for blk in cut(u, [B, B, B]):
            bp.push(blk)
        assert (counters(hip) == c0).all() and bp.counts == [0, 0, 0]
        bp.flush()
        assert tuple(counters(hip) - c0) == (1, 0, 0)
        # a push shorter than the filter: refused by name, nothing staged -- the stream goes on as if it had not happened
        c1 = counters(hip)
        short = u[:2 * (LP - 1)]
        if u8:
            rc = hip.lib.sdrhip_pipe_push_u8(bp.p.h, short.ctypes.data_as(C.POINTER(C.c_uint8)), LP - 1)
        else:
            f = to_f32(short)
            rc = hip.lib.sdrhip_pipe_push(bp.p.h, f.ctypes.data_as(_f32p), LP - 1)
        assert rc == -1 and b"shorter than the filter" in hip.lib.sdrhip_last_error()
        assert (counters(hip) == c1).all()
        bp.p.set_coalesce(0)
        bp.p.set_adaptive(0)
        bp.push(u[2 * 3 * B:2 * 4 * B])
        bp.flush()
        check_rows(hip, bp, tables, [B] * 4, 1000, f"after a refused push, {'u8' if u8 else 'cfloat'}")


# ---- other factors -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor,ntaps", [(4, 127), (16, 127), (8, 64)])
def test_other_factors_and_a_64_tap_filter(hip, factor, ntaps):
    """Uniform and ragged pushes; the bits are asserted, and for factors 8 and 16 the routes too (factor 4 at an odd output falls
    back to the bank's channel-by-channel run)."""
    taps = S.taps_decim127() if ntaps == 127 else S.gauss_taps(ntaps, 40 + ntaps)
    tables = tables_for(3)
    bank = hip.TunerBank(factor, taps, tables)
    for sizes in ([4096] * 6, [4096, 4096, 5001, 4099, 6000, 700, 4100]):
        for u8 in (False, True):
            bp = BankPipe(hip, bank, 1000 if factor == 4 else 300, u8)
            bp.p.set_adaptive(0)
            c0 = counters(hip)
            for blk in cut(stream_u8(), sizes):
                bp.push(blk)
            bp.flush()
            d = counters(hip) - c0
            if factor != 4:
                ragged = len(sizes) - 2 if len(set(sizes)) > 1 else 0       # every push from the first of another size on
                assert tuple(d) == (len(sizes), ragged, 0), f"factor {factor}, {ntaps} taps, sizes {sizes}"
            check_rows(hip, bp, tables, sizes, bp.bo, f"factor {factor}, {ntaps} taps, {'u8' if u8 else 'cfloat'}, sizes {sizes}", factor=factor,
                       taps=taps)


# ---- pop calls ---------------------------------------------------------------------------------------------------------------------
def test_pop_against_pop_rows(hip):
    u = stream_u8()
    blocks = cut(u, [B] * 4)
    # a one-channel bank: pop and pop_rows alternate on one pipe, and both give the one-row tuner Pipe's blocks
    t1 = tables_for(1)
    p = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), t1), 1000)
    p.set_adaptive(0)
    assert p.rows == 1
    ready = 0
    for blk in blocks:
        f = to_f32(blk)
        ready = hip.check(hip.lib.sdrhip_pipe_push(p.h, f.ctypes.data_as(_f32p), B), "push")
    ready = hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush")
    assert ready == 4
    got = []
    for k in range(ready):
        if k % 2:
            got.append(p.pop_rows(1).reshape(-1))
        else:
            o = np.empty(2000, np.float32)
            assert hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(_f32p), 1000) == 1000
            got.append(o)
    assert_bit_equal(np.concatenate(got), one_row_expected(hip, t1[0], [B] * 4, 1000), "pop and pop_rows on a one-channel bank")
    assert p.pop_rows(3).shape == (1, 0, 2000)

    # three rows: pop is refused and pops nothing; a short row_stride is refused with nothing written
    tables = tables_for(3)
    q = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), tables), 1000, input_u8=True)
    q.set_adaptive(0)
    assert q.rows == 3
    for blk in blocks:
        hip.check(hip.lib.sdrhip_pipe_push_u8(q.h, np.ascontiguousarray(blk).ctypes.data_as(C.POINTER(C.c_uint8)), B), "push_u8")
    assert hip.check(hip.lib.sdrhip_pipe_flush(q.h), "flush") == 4
    o = np.full(3 * 8000, CANARY, np.uint32)
    assert hip.lib.sdrhip_pipe_pop(q.h, o.view(np.float32).ctypes.data_as(_f32p), 4000) == -1
    assert b"sdrhip_pipe_pop" in hip.lib.sdrhip_last_error() and (o == CANARY).all()
    assert hip.lib.sdrhip_pipe_pop_rows(q.h, o.view(np.float32).ctypes.data_as(_f32p), 4 * 2000 - 2, 4) == -1
    assert b"sdrhip_pipe_pop_rows" in hip.lib.sdrhip_last_error() and (o == CANARY).all()
    assert hip.check(hip.lib.sdrhip_pipe_poll(q.h), "poll") == 4, "a refused pop took blocks"
    rows = q.pop_rows(4)
    assert rows.shape == (3, 4, 2000)
    for j, t in enumerate(tables):
        assert_bit_equal(rows[j].reshape(-1), one_row_expected(hip, t, [B] * 4, 1000), f"pop_rows: channel {j}")

    # an existing decimator Pipe: pop_rows gives pop's blocks
    x = to_f32(u[:2 * 4 * B])
    outs = []
    for use_rows in (False, True):
        dp = hip.Pipe("decimator", hip.Decimator(8, S.taps_decim127(), hip.ORDER_AVX, complex_=True), 1000)
        dp.set_adaptive(0)
        assert dp.rows == 1
        ready = 0
        for i in range(4):
            hip.check(hip.lib.sdrhip_pipe_push(dp.h, x[2 * B * i:].ctypes.data_as(_f32p), B), "push")
        ready = hip.check(hip.lib.sdrhip_pipe_flush(dp.h), "flush")
        assert ready == 4
        outs.append(dp.pop_rows(4).reshape(-1) if use_rows else np.concatenate(dp._pop(4)))
    assert_bit_equal(outs[1], outs[0], "pop_rows on a decimator Pipe")


# ---- type mismatches ---------------------------------------------------------------------------------------------------------------
def test_the_wrong_push_call_is_refused(hip):
    tables = tables_for(2)
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    u = stream_u8()[:2 * B]
    f = to_f32(u)
    pu, pf = hip.Pipe.tuner_bank(bank, 1000, input_u8=True), hip.Pipe.tuner_bank(bank, 1000)
    c0 = counters(hip)
    assert hip.lib.sdrhip_pipe_push(pu.h, f.ctypes.data_as(_f32p), B) == -1 and b"sdrhip_pipe_push:" in hip.lib.sdrhip_last_error()
    assert hip.lib.sdrhip_pipe_push_u8(pf.h, u.ctypes.data_as(C.POINTER(C.c_uint8)), B) == -1
    assert b"sdrhip_pipe_push_u8" in hip.lib.sdrhip_last_error()
    assert not hip.lib.sdrhip_pipe_input_buffer(pu.h, B) and b"sdrhip_pipe_input_buffer" in hip.lib.sdrhip_last_error()
    assert not hip.lib.sdrhip_pipe_input_buffer_u8(pf.h, B) and b"sdrhip_pipe_input_buffer_u8" in hip.lib.sdrhip_last_error()
    tp = hip.Pipe.tuner(hip.Tuner(8, S.taps_decim127(), tables[0]), 1000)
    assert hip.lib.sdrhip_pipe_push_u8(tp.h, u.ctypes.data_as(C.POINTER(C.c_uint8)), B) == -1
    for p, bad in ((pu, f), (pf, u), (tp, u)):
        with pytest.raises(hip.SdrHipError):
            p.push(bad)
    # nothing was staged: a flush launches nothing and yields nothing
    for p in (pu, pf, tp):
        assert p.flush() == []
    assert (counters(hip) == c0).all()


# ---- save / restore ----------------------------------------------------------------------------------------------------------------
def test_save_and_restore(hip):
    """Save after 5 of 40 pushes (2048-sample blocks) and restore into a second pipe: the rest of the stream is bit-equal; every
    refusal leaves the pipe unchanged."""
    tables = tables_for(3)
    taps = S.taps_decim127()
    bank = hip.TunerBank(8, taps, tables)
    sizes = [2048] * 40
    blocks = cut(stream_u8(), sizes)
    for u8 in (False, True):
        a = BankPipe(hip, bank, 1000, u8)
        for blk in blocks[:5]:
            a.push(blk)
        state = a.p.save()
        version, = struct.unpack_from("<I", state, 4)
        assert version == 2
        b = BankPipe(hip, bank, 1000, u8)

        def refused(pipe, st, what):
            assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
            assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what

        refused(b.p, state[:-1], "a truncated state")
        refused(b.p, state[:60], "a state cut inside its header")
        refused(hip.Pipe.tuner_bank(hip.TunerBank(8, taps, tables[:2]), 1000, input_u8=u8), state, "another row count")
        refused(hip.Pipe.tuner_bank(bank, 1000, input_u8=not u8), state, "another input type")
        refused(hip.Pipe.tuner_bank(bank, 1024, input_u8=u8), state, "another block_size_out")
        refused(hip.Pipe.tuner_bank(hip.TunerBank(16, taps, tables), 1000, input_u8=u8), state, "another factor")
        refused(hip.Pipe.tuner_bank(hip.TunerBank(8, S.gauss_taps(64, 104), tables), 1000, input_u8=u8), state, "another tap count")
        refused(hip.Pipe.tuner(hip.Tuner(8, taps, tables[0]), 1000), state, "a one-row pipe")
        one = hip.Pipe.tuner(hip.Tuner(8, taps, tables[0]), 1000)
        one.push(to_f32(blocks[0]))
        refused(b.p, one.save(), "a one-row pipe's state")
        assert hip.lib.sdrhip_pipe_poll(b.p.h) == 0
        b.restore(state)                                     # ... and after all those refusals the pipe is as fresh as it was
        for blk in blocks[5:]:
            a.push(blk)
            b.push(blk)
        a.flush()
        b.flush()
        check_rows(hip, a, tables, sizes, 1000, f"the saved pipe, {'u8' if u8 else 'cfloat'}")
        nb_before = sum(a.counts[:5])
        for j in range(3):
            assert_bit_equal(b.row(j), a.row(j)[nb_before * 2000:], f"restored pipe, {'u8' if u8 else 'cfloat'}: channel {j}")


def tuner_pipe_state(hip):
    """The state of Pipe.tuner(Tuner(8, taps_decim127, osc_table(1000)), 1000) after five 8192-sample pushes of stream_u8() and a
    flush whose five blocks were popped: position, history and the 105 outputs that fill no block yet."""
    p = hip.Pipe.tuner(hip.Tuner(8, S.taps_decim127(), T.osc_table(1000)), 1000)
    p.set_adaptive(0)
    n = 0
    for blk in cut(stream_u8(), [B] * 5):
        n += len(p.push(to_f32(blk)))
    n += len(p.flush())
    assert n == 5
    return p.save()


# sha256 of tuner_pipe_state(hip) with `hip` bound to a build of the PARENT commit's tree (its sdr_amd/lib.py over its libsdr_hip.so),
# printed on an MI355X by a throw-away script that imported this function
PARENT_TUNER_PIPE_STATE_SHA256 = "a1a39d0ce950351923c6a1667c6f464467a48bb89ff5663f48abaf9c583ac3f9"      # 2136 bytes


def test_a_one_row_tuner_pipe_state_is_byte_for_byte_the_parent_trees(hip):
    state = tuner_pipe_state(hip)
    assert struct.unpack_from("<I", state, 4)[0] == 1
    assert hashlib.sha256(state).hexdigest() == PARENT_TUNER_PIPE_STATE_SHA256


# ---- far position ------------------------------------------------------------------------------------------------------------------
def moved(state, samples, factor=8):
    """The state `samples` further down the stream: E_prev (offset 48) and m_done (offset 56) of the header."""
    e_prev, m_done = struct.unpack_from("<qq", state, 48)
    assert samples % factor == 0
    return state[:48] + struct.pack("<qq", e_prev + samples, m_done + samples // factor) + state[64:]


def test_far_stream_position(hip):
    """A state moved to just above 2^33 samples (2^33 is a multiple of the block size, so the seams stay where they were), periods
    1000 and 5 in one bank: each channel's phase is a 64-bit reduction of its own, and the rows equal the one-row Pipes restored to
    the same position."""
    tables = [T.osc_table(1000), T.osc_table(5)]
    taps = S.taps_decim127()
    bank = hip.TunerBank(8, taps, tables)
    sizes = [B] * 6
    blocks = cut(stream_u8(), sizes)
    far = 1 << 33
    assert far % 1000 != 0 and far % 5 != 0
    for u8 in (False, True):
        a = BankPipe(hip, bank, 1000, u8)
        a.p.set_adaptive(0)
        a.push(blocks[0])
        a.flush()                                            # (every ready block popped: the state holds the 9 outputs that fill none)
        st = moved(a.p.save(), far)
        b = BankPipe(hip, bank, 1000, u8)
        b.p.set_adaptive(0)
        b.restore(st)
        c0 = counters(hip)
        for blk in blocks[1:]:
            b.push(blk)
        b.flush()
        assert tuple(counters(hip) - c0) == (5, 0, 0)
        for j, t in enumerate(tables):
            one = hip.Pipe.tuner(hip.Tuner(8, taps, t), 1000)
            one.set_adaptive(0)
            one.push(to_f32(blocks[0]))
            one.flush()
            exp = one_row_expected(hip, t, sizes[1:], 1000, u8=stream_u8()[2 * B:], state=moved(one.save(), far))
            assert exp.size >= 4 * 2000
            assert_bit_equal(b.row(j), exp, f"far position, {'u8' if u8 else 'cfloat'}: channel {j}")


# ---- the example -------------------------------------------------------------------------------------------------------------------
def test_channel_replay_example(hip, tmp_path):
    exe = os.path.join(ROOT, "examples", "bin", "channel_replay")
    if not os.path.exists(exe):
        from sdr_amd import build as Bd
        Bd.build_examples()
    assert os.path.exists(exe)
    n = 6 * B + 1234                                     # five whole pushes and a ragged rest
    u = stream_u8()[:2 * n]
    cap, tp = tmp_path / "capture.u8", tmp_path / "taps.f32"
    u.tofile(cap)
    S.taps_decim127().tofile(tp)
    r = subprocess.run([exe, str(cap), str(tp), str(tmp_path / "out"), "--channels", "1/4,-3/1000,0/1", "--block-out", "500"],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tables = [hip.tuner_shift_table(1, 4), hip.tuner_shift_table(-3, 1000), hip.tuner_shift_table(0, 1)]
    p = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), tables), 500, input_u8=True)
    p.set_adaptive(0)
    outs = []
    for blk in cut(u, [B] * 6 + [1234]):
        outs += p.push(blk)
    outs += p.flush()
    rows = np.concatenate(outs, axis=1)
    assert rows.shape == (3, ((n - LP) // D + 1) // 500 * 1000)
    for j in range(3):
        assert_bit_equal(np.fromfile(tmp_path / f"out.ch{j}.cf32", np.float32), rows[j], f"channel_replay: channel {j}")
