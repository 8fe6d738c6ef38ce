"""GPU parity of the narrow-band FM bank's Pipe (sdrhip_pipe_nfm_bank): host cfloat / u8 / int16 IQ blocks in, every channel's
demodulated blocks out.  Every channel's blocks are compared, bit for bit over the whole stream, against the model: the restated
firDecimator Pipe on the mixed stream at the pushes' own boundaries (tests/pipe_am_bank_cases.py's streams and cuts), then
oracle.fm_demod from (0, 0) over the whole row -- independent of the product.  Every pop goes into a buffer of NaN canaries.
Shape: 127 taps (128 prepared), factor 8, AVX order, the tables of the tuner bank's tests."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import pipe_am_bank_cases as PC
import signals as S
import test_gpu_pipe_am_bank as PA
import test_gpu_tuner as T
import tuner_model as TM
from conftest import assert_bit_equal
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, LP, D = PC.B, PC.LP, PC.D
NBLK = 19                                      # 19 blocks: two submissions of 16 coalesced blocks, seven of 3
_cache = {}


def nfm_bank(hip, tables, factor=8, order=None, taps=None):
    taps = S.taps_decim127() if taps is None else taps
    tb = hip.TunerBank(factor, taps, tables) if order is None else hip.TunerBank(factor, taps, tables, order)
    return hip.NfmBank(tb)


class NfmPipe(PA.AmPipe):
    """PA.AmPipe's raw-call pushes and canary pops over Pipe.nfm_bank."""

    def __init__(self, hip, bank, block_out, fmt):
        self.hip, self.bo, self.fmt = hip, block_out, fmt
        self.p = hip.Pipe.nfm_bank(bank, block_out, input_u8=fmt == "u8", input_i16=fmt == "i16")
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []


def counters(hip):
    """(fmDemod-form tile, all-Cross fmDemod-form, rows, banked tuner, all-Cross tuner, envelope tile) launches"""
    return np.array([hip.nfm_bank_launches(), hip.nfm_bank_cross_launches(), hip.lib.sdrhip_debug_rows_launches(),
                     hip.tuner_bank_launches(), hip.tuner_bank_cross_launches(), hip.am_bank_launches()])


def expected(oracle, table, fmt, sizes, nsamples, factor=8, order=PM.ORDER_AVX):
    key = (np.asarray(table, np.float32).tobytes(), "i16" if fmt == "i16" else "u8", tuple(int(v) for v in sizes), nsamples, factor, order)
    if key not in _cache:
        m = TM.mix(PC.converted(oracle, fmt, nsamples), table)
        model = PM.FilterModel(oracle, S.taps_decim127(), order, complex_=True, factor=factor)
        out, _ = PM.fir_decimator_pipe(model, PC.cut(m, sizes), 1)
        e = oracle.fm_demod(np.concatenate(out), last=(0.0, 0.0))
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


def check_rows(oracle, ap, tables, fmt, sizes, nsamples, what, **kw):
    for j, t in enumerate(tables):
        exp = expected(oracle, t, fmt, sizes, nsamples, **kw)
        got = ap.row(j)
        assert got.size > 0 and got.size % ap.bo == 0 and got.size <= exp.size
        assert_bit_equal(got, exp[:got.size], f"{what}: channel {j} against the model")


@pytest.mark.parametrize("group", [1, 3, 16])
@pytest.mark.parametrize("nch", [1, 2, 3, 32])
def test_uniform_pushes(hip, oracle, nch, group):
    """`group` 8192-sample blocks per submission: exactly one fmDemod-form tile launch per submission and no other launch."""
    tables = PA.tables_for(nch)
    sizes = [B] * NBLK
    for fmt in PC.FORMATS:
        blocks = PC.cut(PC.stream(fmt, NBLK * B), sizes)
        for bo in (1000, 1024):
            ap = NfmPipe(hip, nfm_bank(hip, tables), bo, fmt)
            assert ap.rows == nch
            ap.p.set_adaptive(0)
            if group > 1:
                ap.p.set_coalesce(group)
            c0 = counters(hip)
            for blk in blocks:
                ap.push(blk)
            ap.flush()
            what = f"{nch} channels, {group} blocks per submission, {fmt}, block_size_out {bo}"
            assert tuple(counters(hip) - c0) == (-(-NBLK // group), 0, 0, 0, 0, 0), what
            assert sum(ap.counts) == ap.row(0).size // bo == ((NBLK * B - LP) // D + 1) // bo, what + ": blocks per channel"
            check_rows(oracle, ap, tables, fmt, sizes, NBLK * B, what)


@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
@pytest.mark.parametrize("fmt", PC.FORMATS)
def test_ragged_pushes(hip, oracle, fmt, mode):
    """Per ragged submission ONE all-Cross launch and ONE tile launch for all channels; every third push goes through input_buffer."""
    sizes = PA.ragged_sizes()
    total = 28 * B
    tables = PA.tables_for(3)
    ap = NfmPipe(hip, nfm_bank(hip, tables), 1000, fmt)
    if mode == "plain":
        ap.p.set_adaptive(0)
    elif mode == "coalesce 7":
        ap.p.set_coalesce(7)
    else:
        ap.p.set_adaptive(32)
    blocks = PC.cut(PC.stream(fmt, total), sizes)
    for i, blk in enumerate(blocks[:3]):
        ap.push(blk, via_buffer=(i == 1))
    ap.flush()
    c0 = counters(hip)
    for i, blk in enumerate(blocks[3:]):
        ap.push(blk, via_buffer=(i % 3 == 0))
    ap.flush()
    d = counters(hip) - c0
    if mode == "plain":
        assert tuple(d) == (len(sizes) - 3, len(sizes) - 3, 0, 0, 0, 0), f"{fmt}, {mode}: {d}"
    assert not d[2:].any()
    check_rows(oracle, ap, tables, fmt, sizes, total, f"ragged, {fmt}, {mode}")


def test_two_hundred_pushes_in_flight(hip, oracle):
    """200 one-block pushes of 1024 samples, four in flight: the state ping-pong under load."""
    n, nb = 1024, 200
    tables = PA.tables_for(3)
    sizes = [n] * nb
    ap = NfmPipe(hip, nfm_bank(hip, tables), 1000, "u8")
    ap.p.set_adaptive(0)
    c0 = counters(hip)
    for blk in PC.cut(PC.stream("u8", nb * n), sizes):
        ap.push(blk)
    ap.flush()
    assert tuple(counters(hip) - c0) == (nb, 0, 0, 0, 0, 0)
    check_rows(oracle, ap, tables, "u8", sizes, nb * n, "200 pushes")


def test_staged_and_short_pushes_and_wrong_calls(hip, oracle):
    tables = PA.tables_for(3)
    ap = NfmPipe(hip, nfm_bank(hip, tables), 1000, "u8")
    ap.p.set_adaptive(0)
    ap.p.set_coalesce(4)
    blocks = PC.cut(PC.stream("u8", 4 * B), [B] * 4)
    c0 = counters(hip)
    for blk in blocks[:3]:
        ap.push(blk)
    assert not (counters(hip) - c0).any() and sum(ap.counts) == 0, "staged pushes launch nothing"
    ap.push(blocks[3])
    ap.flush()
    assert tuple(counters(hip) - c0) == (1, 0, 0, 0, 0, 0)
    short = np.full(2 * 100, 128, np.uint8)
    assert hip.lib.sdrhip_pipe_push_u8(ap.p.h, short.ctypes.data_as(C.POINTER(C.c_uint8)), 100) == -1, "a push shorter than the filter"
    f = np.zeros(2 * B, np.float32)
    assert hip.lib.sdrhip_pipe_push(ap.p.h, f.ctypes.data_as(C.POINTER(C.c_float)), B) == -1 and b"u8" in hip.lib.sdrhip_last_error()
    i16 = np.zeros(2 * B, np.int16)
    assert hip.lib.sdrhip_pipe_push_i16(ap.p.h, i16.ctypes.data_as(C.POINTER(C.c_int16)), B) == -1
    out = np.full(3 * 1000, np.nan, np.float32)
    assert hip.lib.sdrhip_pipe_pop_rows(ap.p.h, out.ctypes.data_as(C.POINTER(C.c_float)), 999, 1) == -1 and np.isnan(out).all(), "a short row_stride"


def test_pop_against_pop_rows(hip, oracle):
    t = [T.osc_table(1000)]
    blocks = PC.cut(PC.stream("u8", 3 * B), [B] * 3)
    a, b = NfmPipe(hip, nfm_bank(hip, t), 1000, "u8"), hip.Pipe.nfm_bank(nfm_bank(hip, t), 1000, input_u8=True)
    for blk in blocks:
        a.push(blk)
    a.flush()
    for blk in blocks:
        assert hip.lib.sdrhip_pipe_push_u8(b.h, np.ascontiguousarray(blk).ctypes.data_as(C.POINTER(C.c_uint8)), B) >= 0
    ready = hip.check(hip.lib.sdrhip_pipe_flush(b.h), "sdrhip_pipe_flush")
    got = []
    for _ in range(ready):
        o = np.empty(1000, np.float32)
        assert hip.lib.sdrhip_pipe_pop(b.h, o.ctypes.data_as(C.POINTER(C.c_float)), 1000) == 1000
        got.append(o)
    assert_bit_equal(np.concatenate(got), a.row(0), "pop against pop_rows")


def test_save_and_restore(hip, oracle):
    """Save after 5 of 40 ragged pushes, restore over a second pipe and continue; every restore refusal leaves the pipe unchanged."""
    rng = np.random.default_rng(11)
    sizes = [int(v) for v in rng.integers(LP, 2 * B + 1, 40)]
    total = sum(sizes)
    tables = PA.tables_for(3)
    bank = nfm_bank(hip, tables)
    blocks = PC.cut(PC.stream("i16", total), sizes)
    first = NfmPipe(hip, bank, 1000, "i16")
    for blk in blocks[:5]:
        first.push(blk)
    state = first.p.save()
    first._pop(hip.check(hip.lib.sdrhip_pipe_poll(first.p.h), "sdrhip_pipe_poll"))
    second = NfmPipe(hip, bank, 1000, "i16")

    def refused(pipe, st, what):
        assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
        assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what

    # the state of this pipe into pipes of another kind, row count, input type, block_size_out, factor and tap count: each is
    # refused, and each refused pipe is UNCHANGED -- it then yields what a fresh twin of it yields from the same pushes
    am = hip.AmBank(bank.tuner_bank, dc_block=False)
    makers = {"another kind (AM bank)": lambda: hip.Pipe.am_bank(am, 1000, input_i16=True),
              "another kind (tuner bank)": lambda: hip.Pipe.tuner_bank(bank.tuner_bank, 1000, input_i16=True),
              "another row count": lambda b=nfm_bank(hip, tables[:2]): hip.Pipe.nfm_bank(b, 1000, input_i16=True),
              "another input type": lambda: hip.Pipe.nfm_bank(bank, 1000, input_u8=True),
              "another block_size_out": lambda: hip.Pipe.nfm_bank(bank, 1024, input_i16=True),
              "another factor": lambda b=nfm_bank(hip, tables, factor=16): hip.Pipe.nfm_bank(b, 1000, input_i16=True),
              "another tap count": lambda b=nfm_bank(hip, tables, taps=S.gauss_taps(64, 104)): hip.Pipe.nfm_bank(b, 1000, input_i16=True)}
    for what, make in makers.items():
        p, twin = make(), make()
        refused(p, state, what)
        assert hip.lib.sdrhip_pipe_poll(p.h) == 0, what
        feed = PC.cut(PC.stream("u8" if p.input_u8 else "i16", 3 * B), [B, 5000, B])
        got, ref = [], []
        for blk in feed:
            got += p.push(blk)
            ref += twin.push(blk)
        got += p.flush()
        ref += twin.flush()
        assert len(got) == len(ref) > 0, what
        assert_bit_equal(np.concatenate(got, axis=-1), np.concatenate(ref, axis=-1), what + ": the refused pipe against a fresh twin")
    # states that are not this pipe's, and truncated ones, into the pipe that then takes the good state and finishes the stream
    tb = hip.Pipe.tuner_bank(bank.tuner_bank, 1000, input_i16=True)
    tb.push(blocks[0])
    refused(second.p, tb.save(), "a tuner bank pipe's state")
    ab = hip.Pipe.am_bank(am, 1000, input_i16=True)
    ab.push(blocks[0])
    refused(second.p, ab.save(), "an AM bank pipe's state")
    for cut_at in (len(state) - 1, len(state) - 24, len(state) - 25, 100, 60):
        refused(second.p, state[:cut_at], f"a state truncated to {cut_at} of {len(state)} bytes")
    assert hip.lib.sdrhip_pipe_poll(second.p.h) == 0
    second.restore(state)
    second.got = [list(g) for g in first.got]
    for blk in blocks[5:]:
        second.push(blk)
    second.flush()
    check_rows(oracle, second, tables, "i16", sizes, total, "restored after 5 of 40 pushes")


def test_older_state_formats_keep_their_bytes(hip):
    for kind, state in PC.existing_kind_states(hip).items():
        assert hashlib.sha256(state).hexdigest() == PC.PARENT_STATE_SHA256[kind], f"the saved state of a {kind} pipe changed"


def test_a_factor_5_bank_goes_through_the_composed_calls(hip, oracle):
    tables = [T.osc_table(1000), T.osc_table(5)]
    sizes = [B, B, B, 5000, 7001, B]
    total = sum(sizes)
    ap = NfmPipe(hip, nfm_bank(hip, tables, factor=5, order=hip.ORDER_SSE), 1000, "u8")
    ap.p.set_adaptive(0)
    c0 = counters(hip)
    for blk in PC.cut(PC.stream("u8", total), sizes):
        ap.push(blk)
    ap.flush()
    d = counters(hip) - c0
    assert d[0] == 0 and d[2] >= len(sizes), f"the fallback did not go through fmDemod's rows form: {d}"
    check_rows(oracle, ap, tables, "u8", sizes, total, "factor 5, SSE order", factor=5, order=PM.ORDER_SSE)


@pytest.mark.parametrize("args", [[], ["--s16"]], ids=["u8", "s16"])
def test_nfm_replay_example(hip, args, tmp_path):
    """examples/nfm_replay.c against the same Pipe driven from the binding: one f32 file per channel."""
    from sdr_amd import build as Bld
    Bld.build_examples()                                      # (a no-op where build() has made it already)
    exe = os.path.join(PA.ROOT, "examples", "bin", "nfm_replay")
    assert os.path.exists(exe)
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
    p = hip.Pipe.nfm_bank(nfm_bank(hip, tables), 1024, input_u8=fmt == "u8", input_i16=fmt == "i16")
    outs = []
    for blk in PC.cut(s, [B] * 6):
        outs += p.push(blk)
    outs += p.flush()
    want = np.concatenate(outs, axis=1)
    assert want.shape == (3, ((6 * B - LP) // D + 1) // 1024 * 1024)
    for j in range(3):
        got = np.fromfile(str(tmp_path / f"out.ch{j}.f32"), np.float32)
        assert_bit_equal(got, want[j], f"nfm_replay {' '.join(args)}: channel {j}")
