"""GPU parity of the narrow-channel bank's Pipe (sdrhip_pipe_narrow_bank): host cfloat / u8 / int16 IQ blocks in, every channel's
    firDecimator deci1 block_mid >-> firDecimator deci2 block_size_out >-> magnitude | fmDemod [>-> dcBlockingFilter]
blocks out.  Every channel's blocks are held, bit for bit, to the model (the restated Pipes alone: the first firDecimator at the
pushes' own boundaries yielding blocks of block_mid, the second on those blocks, then the demodulator models) and to the same stages
driven through the host: a tuner-bank Pipe with block_size_out = block_mid, K one-row Pipe("decimator") objects and the map Pipes.
Every pop goes into a buffer of NaN canaries whose words around each row must be canaries afterwards.
Shape: stage 1 127 taps / 8; stage 2 the 24 / 4 and 61 / 5 decimators of tests/narrow_bank_cases.py."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import agc_model as AM
import narrow_bank_cases as NB
import pipe_am_bank_cases as PC
import signals as S
import test_gpu_pipe_am_bank as TA
import tuner_model as TM
from conftest import assert_bit_equal
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B = PC.B
ENV, FM = NB.ENV, NB.FM
KINDS = [(ENV, True), (ENV, False), (FM, False)]
KIND_IDS = ["env-dc", "env", "fm"]
BO = 100                                       # block_size_out: the 19-block stream yields 48 blocks of it at factor 4
NBLK = TA.NBLK
_cache = {}


def make_bank(hip, tables, shape, form, dc):
    taps, d2, _ = NB.SHAPES[shape]
    return hip.NarrowBank(hip.TunerBank(8, S.taps_decim127(), tables), hip.Decimator(d2, taps, complex_=True), form, dc)


class NarrowPipe(TA.AmPipe):
    """The Pipe through the raw C calls (tests/test_gpu_pipe_am_bank.py's harness: pops into canaries)."""

    def __init__(self, hip, bank, block_mid, block_out, fmt):
        self.hip, self.bo, self.fmt = hip, block_out, fmt
        self.p = hip.Pipe.narrow_bank(bank, block_mid, block_out, input_u8=fmt == "u8", input_i16=fmt == "i16")
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []


def model(oracle, table, fmt, sizes, nsamples, shape, block_mid, form, dc):
    """The channel's demodulated stream from the restated Pipes alone, in whole blocks of BO as the second firDecimator yields them."""
    key = (np.asarray(table, np.float32).tobytes(), "i16" if fmt == "i16" else "u8", tuple(int(v) for v in sizes), nsamples, shape, block_mid)
    if key not in _cache:
        taps2, d2, _ = NB.SHAPES[shape]
        m = TM.mix(PC.converted(oracle, fmt, nsamples), table)
        m1 = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=8)
        mid, _ = PM.fir_decimator_pipe(m1, PC.cut(m, sizes), block_mid)
        m2 = PM.FilterModel(oracle, taps2, PM.ORDER_AVX, complex_=True, factor=d2)
        out, _ = PM.fir_decimator_pipe(m2, mid, BO)
        iq2 = np.concatenate(out)
        iq2.setflags(write=False)
        _cache[key] = iq2
    if key + (form, dc) not in _cache:
        y = NB.demodulate(oracle, _cache[key], form, dc)
        y.setflags(write=False)
        _cache[key + (form, dc)] = y
    return _cache[key + (form, dc)]


def narrow_runs(submissions, shape, block_mid):
    """How many of these submissions (samples each) complete stage-2 outputs: those at which the outputs that the WHOLE blocks of
    block_mid stage-1 outputs so far allow move on.  Each of them is exactly one narrow launch."""
    _, d2, lp2 = NB.SHAPES[shape]
    seen, done, runs = 0, 0, 0
    for n in submissions:
        seen += n
        m = (seen - 128) // 8 + 1 if seen >= 128 else 0
        n1 = m // block_mid * block_mid
        ready = (n1 - lp2) // d2 + 1 if n1 >= lp2 else 0
        runs += ready > done
        done = max(done, ready)
    return runs


def host_chain(hip, bank, block_mid, block_out, fmt, blocks, rows):
    """{row: stream} through the host: Pipe.tuner_bank(block_mid), then per row Pipe("decimator") and the map Pipes."""
    tb = hip.Pipe.tuner_bank(bank.tuner_bank, block_mid, input_u8=fmt == "u8", input_i16=fmt == "i16")
    mids = []
    for blk in blocks:
        mids += tb.push(blk)
    mids += tb.flush()
    out = {}
    for j in rows:
        dp = hip.Pipe("decimator", bank.decimator, block_out)
        mp = hip.Pipe("fm_demod") if bank.form == FM else hip.Pipe.am_demod()
        dcp = hip.Pipe("dc_blocker") if bank.dc_block else None
        def through(pipe, blks):
            got = []
            for blk in blks:
                got += pipe.push(np.ascontiguousarray(blk))
            return got + pipe.flush()                # (a Pipe keeps submissions in flight: its last blocks come with the flush)

        ys = through(mp, through(dp, [mid[j] for mid in mids]))
        if dcp:
            ys = through(dcp, ys)
        out[j] = np.concatenate(ys) if ys else np.empty(0, np.float32)
    return out


def check(hip, oracle, ap, bank, tables, shape, block_mid, fmt, sizes, blocks, nsamples, what, host_rows=(0,)):
    host = host_chain(hip, bank, block_mid, ap.bo, fmt, blocks, host_rows)
    for j, t in enumerate(tables):
        exp = model(oracle, t, fmt, sizes, nsamples, shape, block_mid, bank.form, bank.dc_block)
        got = ap.row(j)
        assert got.size > 0 and got.size % ap.bo == 0 and got.size <= exp.size, f"{what}: channel {j}: {got.size} outputs"
        assert exp.size - got.size < ap.bo + block_mid, f"{what}: channel {j}: the pipe is more than a block behind the model"
        assert_bit_equal(got, exp[:got.size], f"{what}: channel {j} against the model")
        if j in host:
            assert host[j].size == got.size, f"{what}: channel {j}: {got.size} outputs, the stages through the host yield {host[j].size}"
            assert_bit_equal(got, host[j], f"{what}: channel {j} against the stages driven through the host")


def counters(hip):
    """(narrow kernel, banked tuner, all-Cross tuner, FIR rows tile, amDemod) launches"""
    return np.array([hip.narrow_bank_launches(), hip.tuner_bank_launches(), hip.tuner_bank_cross_launches(), hip.fir_rows_launches(),
                     hip.am_demod_launches()])


# ---- uniform pushes ----------------------------------------------------------------------------------------------------------------
MIDS = ((1024, "24/4"), (1000, "61/5"))


@pytest.mark.parametrize("group", [1, 3, 16])
@pytest.mark.parametrize("nch", [1, 2, 32])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=KIND_IDS)
def test_uniform_pushes(hip, oracle, kind, nch, group):
    """`group` 8192-sample blocks per submission, the three input types, block_mid 1024 (24 / 4) and 1000 (61 / 5): one banked tuner
    launch per submission (one channel: its tuner's, none banked), EXACTLY one narrow launch per submission that completes stage-2
    outputs and none for the others, no all-Cross launch and none of the composed route's launches."""
    form, dc = KINDS[kind]
    tables = TA.tables_for(nch)
    sizes = [B] * NBLK
    subs = [B * min(group, NBLK - i) for i in range(0, NBLK, group)]
    for fmt in PC.FORMATS:
        blocks = PC.cut(PC.stream(fmt, NBLK * B), sizes)
        for block_mid, shape in MIDS:
            bank = make_bank(hip, tables, shape, form, dc)
            ap = NarrowPipe(hip, bank, block_mid, BO, fmt)
            assert ap.rows == nch
            ap.p.set_adaptive(0)
            if group > 1:
                ap.p.set_coalesce(group)
            c0 = counters(hip)
            for blk in blocks:
                ap.push(blk)
            ap.flush()
            d = counters(hip) - c0
            want = narrow_runs(subs, shape, block_mid)
            what = f"{fmt}, block_mid {block_mid}, {shape}, {group} per submission"
            assert len(subs) - 1 <= want <= len(subs), what
            assert tuple(d) == (want, len(subs) if nch > 1 else 0, 0, 0, 0), f"{what}: launches {d}, {want} narrow runs expected"
            check(hip, oracle, ap, bank, tables, shape, block_mid, fmt, sizes, blocks, NBLK * B, "uniform, " + what, host_rows=(0, nch - 1))


# ---- ragged pushes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=KIND_IDS)
def test_ragged_pushes(hip, oracle, kind, mode):
    """Seeded block sizes, odd ones included: per ragged submission ONE all-Cross tuner launch and ONE banked launch, and at most one
    narrow launch; every third push goes through input_buffer.  Stage 2 sees blocks of block_mid whatever the pushes are."""
    form, dc = KINDS[kind]
    fmt = PC.FORMATS[kind]
    sizes = TA.ragged_sizes()
    total = 28 * B
    tables = TA.tables_for(3)
    bank = make_bank(hip, tables, "61/5", form, dc)
    ap = NarrowPipe(hip, bank, 1000, BO, fmt)
    if mode == "plain":
        ap.p.set_adaptive(0)
    elif mode == "coalesce 7":
        ap.p.set_coalesce(7)
    else:
        ap.p.set_adaptive(32)
    blocks = PC.cut(PC.stream(fmt, total), sizes)
    for i, blk in enumerate(blocks[:4]):
        ap.push(blk, via_buffer=(i == 1))
    c1 = counters(hip)
    for i, blk in enumerate(blocks[4:]):
        ap.push(blk, via_buffer=(i % 3 == 0))
        c2 = counters(hip)
        d = c2 - c1
        assert d[1] == 1 and d[2] == 1 and d[0] <= 1 and d[3] == 0, f"{mode}: ragged push {i + 4} of {blk.size // 2} samples: {d}"
        c1 = c2
    ap.flush()
    assert (counters(hip) == c1).all(), "flush launched although nothing was staged"
    check(hip, oracle, ap, bank, tables, "61/5", 1000, fmt, sizes, blocks, total, f"ragged pushes, {mode}, {fmt}")


def test_pushes_that_complete_no_stage_two_output(hip, oracle):
    """Pushes of 2048 samples are 256 stage-1 outputs: three of four complete no block of 1024 and run the bank part only."""
    tables = TA.tables_for(2)
    sizes = [2048] * 40
    for kind, fmt in zip(range(3), PC.FORMATS):
        form, dc = KINDS[kind]
        bank = make_bank(hip, tables, "24/4", form, dc)
        ap = NarrowPipe(hip, bank, 1024, BO, fmt)
        ap.p.set_adaptive(0)
        blocks = PC.cut(PC.stream(fmt, 40 * 2048), sizes)
        moved = []
        for blk in blocks:
            c0 = counters(hip)
            ap.push(blk)
            ap.flush()
            moved.append(int((counters(hip) - c0)[0]))
        assert set(moved) == {0, 1} and 8 <= sum(moved) <= 10, moved
        check(hip, oracle, ap, bank, tables, "24/4", 1024, fmt, sizes, blocks, 40 * 2048, f"short pushes, {fmt}", host_rows=(0, 1))


def test_a_second_decimator_the_fused_launch_does_not_serve(hip, oracle):
    """An SSE-order decimator2: the Pipe's narrow runs take the composed calls (decimator rows, demodulator rows), no narrow launch,
    and every block equals the same stages driven through the host."""
    tables = TA.tables_for(2)
    taps, d2, _ = NB.SHAPES["24/4"]
    sizes = [B] * 8
    for kind, fmt in zip(range(3), PC.FORMATS):
        form, dc = KINDS[kind]
        bank = hip.NarrowBank(hip.TunerBank(8, S.taps_decim127(), tables), hip.Decimator(d2, taps, hip.ORDER_SSE, complex_=True), form, dc)
        ap = NarrowPipe(hip, bank, 1024, BO, fmt)
        ap.p.set_adaptive(0)
        blocks = PC.cut(PC.stream(fmt, 8 * B), sizes)
        c0 = counters(hip)
        rows0 = hip.rows_launches()
        for blk in blocks:
            ap.push(blk)
        ap.flush()
        d = counters(hip) - c0
        want = narrow_runs(sizes, "24/4", 1024)
        assert want == 7, "the first block of 8192 samples completes no block of 1024 stage-1 outputs"
        assert d[0] == 0 and d[1] == 8 and d[2] == 0, f"{fmt}: launches {d}"
        assert (d[4] == want) if form == ENV else (hip.rows_launches() - rows0 >= want), f"{fmt}: the demodulator's rows form runs once per narrow run"
        host = host_chain(hip, bank, 1024, BO, fmt, blocks, (0, 1))
        for j in range(2):
            got = ap.row(j)
            assert got.size == host[j].size > 0
            assert_bit_equal(got, host[j], f"SSE-order second decimator, {fmt}: channel {j} against the stages driven through the host")


# ---- calls -------------------------------------------------------------------------------------------------------------------------
def test_create_refusals(hip):
    bank = make_bank(hip, TA.tables_for(2), "61/5", ENV, True)
    for what, args in (("a null bank", (None, 1024, BO, 0)), ("block_mid shorter than filter + factor", (bank.h, 68, BO, 0)),
                       ("block_size_out 0", (bank.h, 1024, 0, 0)), ("input_type 3", (bank.h, 1024, BO, 3))):
        h = C.c_void_p(0xdead)
        assert hip.lib.sdrhip_pipe_narrow_bank(C.byref(h), *args) == -1 and not h.value, what
        assert b"sdrhip_pipe_narrow_bank" in hip.lib.sdrhip_last_error(), what
    assert hip.lib.sdrhip_pipe_narrow_bank(None, bank.h, 1024, BO, 0) == -1
    assert hip.Pipe.narrow_bank(bank, 69, BO).rows == 2


def test_the_wrong_push_call_is_refused(hip):
    bank = make_bank(hip, TA.tables_for(2), "24/4", FM, False)
    data = {f: np.ascontiguousarray(PC.stream(f, B)) for f in PC.FORMATS}
    c0 = counters(hip)
    for fmt in PC.FORMATS:
        p = hip.Pipe.narrow_bank(bank, 1024, BO, input_u8=fmt == "u8", input_i16=fmt == "i16")
        for other in PC.FORMATS:
            if other == fmt:
                continue
            name, ptr_t = TA.PUSH[other]
            assert getattr(hip.lib, name)(p.h, data[other].ctypes.data_as(ptr_t), B) == -1, f"{other} blocks into a {fmt} pipe"
            assert name.encode() + b":" in hip.lib.sdrhip_last_error()
            with pytest.raises(hip.SdrHipError):
                p.push(data[other])
        assert p.flush() == []
    assert (counters(hip) == c0).all()


def test_pop_against_pop_rows(hip, oracle):
    blocks = PC.cut(PC.stream("cf32", NBLK * B), [B] * 4)
    t1 = TA.tables_for(1)
    bank = make_bank(hip, t1, "24/4", FM, False)
    p = hip.Pipe.narrow_bank(bank, 1024, BO)
    q = NarrowPipe(hip, bank, 1024, BO, "cf32")
    for blk in blocks[:-1]:
        q.push(blk)
        assert hip.check(hip.lib.sdrhip_pipe_push(p.h, np.ascontiguousarray(blk).ctypes.data_as(TA._f32p), blk.size // 2), "push") >= 0
    q.flush()
    ready = hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush")
    assert ready == sum(q.counts) > 3
    one = []
    for _ in range(ready):
        o = np.empty(BO, np.float32)
        assert hip.check(hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(TA._f32p), BO), "pop") == BO
        one.append(o)
    assert_bit_equal(np.concatenate(one), q.row(0), "pop against pop_rows")
    # a pipe of more than one row has no sdrhip_pipe_pop
    p2 = hip.Pipe.narrow_bank(make_bank(hip, TA.tables_for(2), "24/4", FM, False), 1024, BO)
    o = np.empty(BO, np.float32)
    assert hip.lib.sdrhip_pipe_pop(p2.h, o.ctypes.data_as(TA._f32p), BO) == -1


# ---- save / restore ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2], ids=KIND_IDS)
def test_save_and_restore(hip, oracle, kind):
    """Save after 5 of 40 pushes (2048-sample blocks: the carried complex rows hold a quarter of a block of 1024) and restore over a
    second pipe: the rest of the stream is the model's; every refusal leaves the pipe unchanged."""
    form, dc = KINDS[kind]
    tables = TA.tables_for(3)
    sizes = [2048] * 40
    for fmt in PC.FORMATS:
        kw = dict(input_u8=fmt == "u8", input_i16=fmt == "i16")
        bank = make_bank(hip, tables, "24/4", form, dc)
        blocks = PC.cut(PC.stream(fmt, 40 * 2048), sizes)
        a = NarrowPipe(hip, bank, 1024, BO, fmt)
        for blk in blocks[:5]:
            a.push(blk)
        state = a.p.save()
        b = NarrowPipe(hip, bank, 1024, BO, fmt)

        def refused(pipe, st, what):
            assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
            assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what

        refused(b.p, state[:-1], "a truncated state")
        refused(b.p, state[:-(3 * 256 * 8 + 9)], "a state cut inside its state floats")
        refused(b.p, state[:60], "a state cut inside its header")
        refused(hip.Pipe.narrow_bank(make_bank(hip, tables[:2], "24/4", form, dc), 1024, BO, **kw), state, "another row count")
        refused(hip.Pipe.narrow_bank(bank, 1024, BO, input_u8=fmt != "u8", input_i16=False), state, "another input type")
        refused(hip.Pipe.narrow_bank(bank, 1024, BO + 4, **kw), state, "another block_size_out")
        refused(hip.Pipe.narrow_bank(bank, 1000, BO, **kw), state, "another block_mid")
        refused(hip.Pipe.narrow_bank(make_bank(hip, tables, "61/5", form, dc), 1024, BO, **kw), state, "another second decimator")
        taps = NB.SHAPES["24/4"][0]
        d2 = hip.NarrowBank(bank.tuner_bank, hip.Decimator(4, taps[:20], complex_=True), form, dc)
        refused(hip.Pipe.narrow_bank(d2, 1024, BO, **kw), state, "another tap count of the second decimator")
        d3 = hip.NarrowBank(bank.tuner_bank, hip.Decimator(8, taps, complex_=True), form, dc)
        refused(hip.Pipe.narrow_bank(d3, 1024, BO, **kw), state, "another factor of the second decimator")
        oform, odc = KINDS[(kind + 1) % 3]
        refused(hip.Pipe.narrow_bank(make_bank(hip, tables, "24/4", oform, odc), 1024, BO, **kw), state, "another form or dc_block")
        s16 = hip.NarrowBank(hip.TunerBank(16, S.taps_decim127(), tables), bank.decimator, form, dc)
        refused(hip.Pipe.narrow_bank(s16, 1024, BO, **kw), state, "another first factor")
        tb = hip.Pipe.tuner_bank(bank.tuner_bank, BO, **kw)
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
        check(hip, oracle, a, bank, tables, "24/4", 1024, fmt, sizes, blocks, 40 * 2048, f"the saved pipe, {fmt}")
        nb_before = sum(a.counts[:5])
        for j in range(3):
            assert_bit_equal(b.row(j), a.row(j)[nb_before * BO:], f"restored pipe, {fmt}: channel {j}")


def test_saved_states_of_every_existing_kind_keep_their_bytes(hip):
    states = PC.existing_kind_states(hip)
    assert set(states) == set(PC.PARENT_STATE_SHA256) and len(states) == 9
    for kind, st in states.items():
        assert hashlib.sha256(st).hexdigest() == PC.PARENT_STATE_SHA256[kind], f"the saved state of a {kind} pipe changed"


# ---- examples ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("example,form,dc", [("airband_replay", ENV, True), ("nfm_replay", FM, False)])
@pytest.mark.parametrize("args", [[], ["--block-mid", "1000", "--s16"]], ids=["mid 1024, u8", "mid 1000, s16"])
def test_replay_examples_with_narrow(hip, example, form, dc, args, tmp_path):
    """examples/<example> --narrow TAPS2.f32 D2 [--block-mid N] against the same Pipe driven from the binding: one f32 file per channel."""
    from sdr_amd import build as Bld
    Bld.build_examples()                                      # (a no-op where build() has made it already)
    exe = os.path.join(TA.ROOT, "examples", "bin", example)
    assert os.path.exists(exe)
    fmt = "i16" if "--s16" in args else "u8"
    nblk = 12
    s = PC.stream(fmt, nblk * B)
    cap, tp, tp2 = tmp_path / "capture.bin", tmp_path / "taps.f32", tmp_path / "taps2.f32"
    s.tofile(cap)
    S.taps_decim127().tofile(tp)
    t2, d2, _ = NB.SHAPES["61/5"]
    t2.tofile(tp2)
    chans = [(1, 64), (-3, 64), (0, 1)]
    r = subprocess.run([exe, str(cap), str(tp), str(tmp_path / "out"), "--channels", ",".join(f"{a}/{b}" for a, b in chans), "--block-out", "200",
                        "--narrow", str(tp2), str(d2)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tables = [hip.tuner_shift_table(a, b) for a, b in chans]
    mid = 1000 if "--block-mid" in args else 1024
    p = hip.Pipe.narrow_bank(make_bank(hip, tables, "61/5", form, dc), mid, 200, input_u8=fmt == "u8", input_i16=fmt == "i16")
    outs = []
    for blk in PC.cut(s, [B] * nblk):
        outs += p.push(blk)
    outs += p.flush()
    want = np.concatenate(outs, axis=1)
    assert want.shape[0] == 3 and want.shape[1] >= 2000 and want.shape[1] % 200 == 0
    for j in range(3):
        got = np.fromfile(str(tmp_path / f"out.ch{j}.f32"), np.float32)
        assert_bit_equal(got, want[j], f"{example} --narrow {' '.join(args)}: channel {j}")
    # --narrow excludes --audio
    r = subprocess.run([exe, str(cap), str(tp), str(tmp_path / "o2"), "--channels", "0/1", "--narrow", str(tp2), str(d2), "--audio", str(tp), str(tp)],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--narrow" in r.stderr
