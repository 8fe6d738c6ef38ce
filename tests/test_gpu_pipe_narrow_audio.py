"""GPU parity of the narrow-channel bank's Pipe with the audio tail behind it (sdrhip_pipe_narrow_bank_audio): host cfloat / u8 / int16
IQ blocks in, every channel's
    firDecimator deci1 block_mid >-> firDecimator deci2 block >-> magnitude | fmDemod [>-> dcBlockingFilter]
    >-> firResampler(block) >-> firFilter(block) >-> (* gain)
audio blocks out.  Every channel's blocks are held, bit for bit,
  (a) to the restated Pipes end to end: tests/test_gpu_pipe_narrow_bank.py's model of the demodulated stream (tuner model, two
      decimator Pipes, demodulator, dcBlocker) through tests/audio_tail_any_cases.py's resampler and filter Pipes and the scale;
  (b) to Pipe.narrow_bank with block_size_out = block, popped through the host into a Pipe("resampler") and a Pipe("filter") per
      channel, and scaled.
Combinations (block_mid, second decimator, ratio, block): (1024, 24/4, 4/5 x 63, 256) and (1000, 61/5, 2/5 x 127, 200).  With mode 1
the launches are counted exactly: one launch of the general kernel for every submission that completes audio outputs, none of
k_audio_tail_rows and none of the row forms.  Every pop goes into canaries (tests/test_gpu_pipe_am_bank.py's harness)."""
import ctypes as C

import numpy as np
import pytest

import audio_tail_any_cases as AC
import narrow_bank_cases as NB
import pipe_am_bank_cases as PC
import signals as S
import test_gpu_pipe_am_bank as TA
import test_gpu_pipe_narrow_bank as TN
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

B = PC.B
NBLK = TA.NBLK
GAIN = 0.5
COMBOS = {"4/5": (1024, "24/4", AC.SHAPES["4/5 x 63"], 256), "2/5": (1000, "61/5", AC.SHAPES["2/5 x 127"], 200)}
KINDS, KIND_IDS = TN.KINDS, TN.KIND_IDS


def make_tail(hip, shape, block, mode=1, order=None):
    t = hip.AudioTail(shape.I, shape.D, shape.resamp_taps(), shape.audio_half(), gain=GAIN, block=block,
                      order=hip.ORDER_AVX if order is None else order)
    t.set_general(mode)
    return t


class NarrowAudioPipe(TA.AmPipe):
    def __init__(self, hip, bank, tail, block_mid, fmt):
        self.hip, self.bo, self.fmt = hip, tail.block, fmt
        self.p = hip.Pipe.narrow_bank_audio(bank, tail, block_mid, input_u8=fmt == "u8", input_i16=fmt == "i16")
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []


def counters(hip):
    """(general tail kernel, k_audio_tail_rows, narrow kernel, banked tuner, all-Cross tuner, FIR rows tile + fix-up) launches"""
    return np.array([hip.audio_tail_general_launches(), hip.audio_tail_launches(), hip.narrow_bank_launches(), hip.tuner_bank_launches(),
                     hip.tuner_bank_cross_launches(), hip.fir_rows_launches() + hip.fir_rows_fixups()])


def progress(tail, submissions, shape2, block_mid):
    """Per submission (samples each): (stage-2 outputs ready, audio outputs ready) afterwards."""
    _, d2, lp2 = NB.SHAPES[shape2]
    seen, out = 0, []
    for n in submissions:
        seen += n
        m = (seen - 128) // 8 + 1 if seen >= 128 else 0
        n1 = m // block_mid * block_mid
        a2 = (n1 - lp2) // d2 + 1 if n1 >= lp2 else 0
        out.append((a2, tail.ready(a2)))
    return out


def runs_of(tail, submissions, shape2, block_mid):
    """(narrow launches, tail launches) these submissions make: a submission that completes stage-2 outputs is one narrow launch, one
    that completes audio outputs one tail run."""
    a2s = [0] + [a for a, _ in progress(tail, submissions, shape2, block_mid)]
    qs = [0] + [q for _, q in progress(tail, submissions, shape2, block_mid)]
    return sum(b > a for a, b in zip(a2s[:-1], a2s[1:])), sum(b > a for a, b in zip(qs[:-1], qs[1:]))


def model(oracle, table, fmt, sizes, nsamples, combo, form, dc):
    """(a): the channel's audio from the restated Pipes alone."""
    block_mid, shape2, shape, block = COMBOS[combo]
    y = TN.model(oracle, table, fmt, sizes, nsamples, shape2, block_mid, form, dc)
    return AC.expected_from(oracle, shape, np.ascontiguousarray(y), block, GAIN)


def host_chain(hip, oracle, bank, tail_shape, block, block_mid, fmt, blocks, rows, order=None):
    """(b): {row: audio} through the host: Pipe.narrow_bank(block), then per row Pipe("resampler"), Pipe("filter") and the scale."""
    order = hip.ORDER_AVX if order is None else order
    nb = hip.Pipe.narrow_bank(bank, block_mid, block, input_u8=fmt == "u8", input_i16=fmt == "i16")
    ys = []
    for blk in blocks:
        ys += nb.push(blk)
    ys += nb.flush()
    res = hip.Resampler(tail_shape.I, tail_shape.D, tail_shape.resamp_taps(), order)
    fil = hip.Filter(tail_shape.audio_half(), order, sym=True)
    out = {}
    for j in rows:
        def through(pipe, blks):
            got = []
            for b in blks:
                got += pipe.push(np.ascontiguousarray(b))
            return got + pipe.flush()
        a = through(hip.Pipe("filter", fil, block), through(hip.Pipe("resampler", res, block), [y[j] for y in ys]))
        out[j] = oracle.scale(np.float32(GAIN), np.concatenate(a)) if a else np.empty(0, np.float32)
    return out


def check(hip, oracle, ap, bank, tables, combo, fmt, sizes, blocks, nsamples, what, host_rows=(0,), against_model=True, order=None):
    block_mid, shape2, shape, block = COMBOS[combo]
    host = host_chain(hip, oracle, bank, shape, block, block_mid, fmt, blocks, host_rows, order)
    for j, t in enumerate(tables):
        got = ap.row(j)
        assert got.size >= 3 * block and got.size % block == 0, f"{what}: channel {j}: {got.size} outputs"
        if against_model:
            exp = model(oracle, t, fmt, sizes, nsamples, combo, bank.form, bank.dc_block)
            # the model's demodulated stream ends on a whole block of its own second decimator (100 outputs): it determines at most
            # 100 * I / D audio outputs fewer than the pipe has seen, and the pipe yields whole blocks only
            n = min(got.size, exp.size)
            assert n >= got.size - block and exp.size - got.size < 2 * block, f"{what}: channel {j}: {got.size} outputs, the model {exp.size}"
            assert_bit_equal(got[:n], exp[:n], f"{what}: channel {j} against the restated Pipes")
        if j in host:
            # a Pipe yields whole blocks only, so driven through the host the tail sees the stage-2 outputs a block at a time and lags the
            # fused Pipe (which takes every stage-2 output as it comes) by up to that block's audio outputs and the filter's own block
            assert got.size - 3 * block <= host[j].size <= got.size and host[j].size % block == 0 and host[j].size >= 2 * block, \
                f"{what}: channel {j}: {got.size} outputs, the stages through the host yield {host[j].size}"
            assert_bit_equal(got[:host[j].size], host[j], f"{what}: channel {j} against the narrow Pipe and the tail's Pipes driven through the host")


# ---- uniform pushes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 3, 16])
@pytest.mark.parametrize("nch", [1, 2, 32])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=KIND_IDS)
def test_uniform_pushes_mode_1_with_exact_launch_counts(hip, oracle, kind, nch, group):
    form, dc = KINDS[kind]
    tables = TA.tables_for(nch)
    sizes = [B] * NBLK
    subs = [B * min(group, NBLK - i) for i in range(0, NBLK, group)]
    for fmt in PC.FORMATS:
        blocks = PC.cut(PC.stream(fmt, NBLK * B), sizes)
        for combo, (block_mid, shape2, shape, block) in COMBOS.items():
            bank = TN.make_bank(hip, tables, shape2, form, dc)
            tail = make_tail(hip, shape, block)
            ap = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)
            assert ap.rows == nch
            ap.p.set_adaptive(0)
            if group > 1:
                ap.p.set_coalesce(group)
            c0 = counters(hip)
            for blk in blocks:
                ap.push(blk)
            ap.flush()
            d = counters(hip) - c0
            narrow, tails = runs_of(tail, subs, shape2, block_mid)
            what = f"{fmt}, {combo}, block_mid {block_mid}, block {block}, {group} per submission"
            assert tails >= 1 and tuple(d) == (tails, 0, narrow, len(subs) if nch > 1 else 0, 0, 0), f"{what}: launches {d}, {narrow} narrow and {tails} tail runs expected"
            assert ap.row(0).size == progress(tail, subs, shape2, block_mid)[-1][1] // block * block, what
            check(hip, oracle, ap, bank, tables, combo, fmt, sizes, blocks, NBLK * B, "uniform, " + what, host_rows=(0, nch - 1))


@pytest.mark.parametrize("mode", [2, "sse"], ids=["mode 2", "an SSE tail"])
def test_the_composed_tail_inside_the_pipe(hip, oracle, mode):
    """Mode 2, and a tail in the SSE order (which the general kernel does not serve, whatever the mode): the composition inside the
    Pipe, no launch of either fused tail kernel."""
    tables = TA.tables_for(2)
    sizes = [B] * NBLK
    for kind, fmt in zip(range(3), PC.FORMATS):
        form, dc = KINDS[kind]
        combo = "4/5" if kind != 1 else "2/5"
        block_mid, shape2, shape, block = COMBOS[combo]
        blocks = PC.cut(PC.stream(fmt, NBLK * B), sizes)
        bank = TN.make_bank(hip, tables, shape2, form, dc)
        order = hip.ORDER_SSE if mode == "sse" else None
        tail = make_tail(hip, shape, block, 1 if mode == "sse" else 2, order)
        assert tail.general_fits() == (mode != "sse")
        ap = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)
        ap.p.set_adaptive(0)
        c0 = counters(hip)
        for blk in blocks:
            ap.push(blk)
        ap.flush()
        d = counters(hip) - c0
        assert d[0] == 0 and d[1] == 0 and d[2] == runs_of(tail, sizes, shape2, block_mid)[0], f"{fmt}: launches {d}"
        check(hip, oracle, ap, bank, tables, combo, fmt, sizes, blocks, NBLK * B, f"composed tail ({mode}), {fmt}", host_rows=(0, 1),
              against_model=mode != "sse", order=order)


# ---- ragged and short pushes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=KIND_IDS)
def test_ragged_pushes(hip, oracle, kind, mode):
    """Seeded block sizes, odd ones included; every third push goes through input_buffer.  At most one narrow launch and one tail
    launch per push."""
    form, dc = KINDS[kind]
    fmt = PC.FORMATS[kind]
    sizes = TA.ragged_sizes()
    total = 28 * B
    tables = TA.tables_for(3)
    combo = "2/5"
    block_mid, shape2, shape, block = COMBOS[combo]
    bank = TN.make_bank(hip, tables, shape2, form, dc)
    tail = make_tail(hip, shape, block)
    ap = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)
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
        assert d[0] <= 1 and d[1] == 0 and d[2] <= 1 and d[5] == 0, f"{mode}: ragged push {i + 4} of {blk.size // 2} samples: {d}"
        c1 = c2
    ap.flush()
    assert (counters(hip) == c1).all(), "flush launched although nothing was staged"
    check(hip, oracle, ap, bank, tables, combo, fmt, sizes, blocks, total, f"ragged pushes, {mode}, {fmt}")


def test_pushes_of_2048_samples_with_both_kinds_of_quiet_submission(hip, oracle):
    """2048 samples are 256 stage-1 outputs: three of four pushes complete no block of 1024 and run the bank part only; with a tail
    block of 256 a submission that completes 256 stage-2 outputs can complete no audio block -- and with the lowest-rate tail (2/5) some
    complete stage-2 outputs and no audio OUTPUT at all: no tail launch."""
    tables = TA.tables_for(2)
    sizes = [2048] * 40
    seen = set()
    for kind, fmt in zip(range(3), PC.FORMATS):
        form, dc = KINDS[kind]
        combo = "4/5" if kind != 1 else "2/5"
        block_mid, shape2, shape, block = COMBOS[combo]
        bank = TN.make_bank(hip, tables, shape2, form, dc)
        tail = make_tail(hip, shape, block)
        ap = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)
        ap.p.set_adaptive(0)
        blocks = PC.cut(PC.stream(fmt, 40 * 2048), sizes)
        prog = [(0, 0)] + progress(tail, sizes, shape2, block_mid)
        for i, blk in enumerate(blocks):
            c0 = counters(hip)
            ap.push(blk)
            ap.flush()
            d = counters(hip) - c0
            want = (int(prog[i + 1][1] > prog[i][1]), 0, int(prog[i + 1][0] > prog[i][0]))
            assert tuple(d[:3]) == want and d[5] == 0, f"{fmt}, push {i}: launches {d}, expected (tail, -, narrow) {want}"
            seen.add(want)
        check(hip, oracle, ap, bank, tables, combo, fmt, sizes, blocks, 40 * 2048, f"short pushes, {fmt}", host_rows=(0, 1))
    assert seen == {(0, 0, 0), (0, 0, 1), (1, 0, 1)}, f"no stage-2 output / stage-2 output but no audio / both: {seen}"


def test_200_pushes_in_flight(hip, oracle):
    """200 pushes of 1024 samples without a poll in between (the engine keeps up to four submissions in flight and harvests as it
    goes): every block arrives, in order."""
    tables = TA.tables_for(2)
    sizes = [1024] * 200
    combo = "4/5"
    block_mid, shape2, shape, block = COMBOS[combo]
    fmt = "u8"
    bank = TN.make_bank(hip, tables, shape2, NB.FM, False)
    tail = make_tail(hip, shape, block)
    ap = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)
    blocks = PC.cut(PC.stream(fmt, 200 * 1024), sizes)
    for blk in blocks:
        ap.push(blk)
    ap.flush()
    check(hip, oracle, ap, bank, tables, combo, fmt, sizes, blocks, 200 * 1024, "200 pushes in flight", host_rows=(0, 1))


# ---- calls -------------------------------------------------------------------------------------------------------------------------
def test_create_refusals(hip):
    block_mid, shape2, shape, block = COMBOS["2/5"]
    bank = TN.make_bank(hip, TA.tables_for(2), shape2, NB.ENV, True)
    tail = make_tail(hip, shape, block)
    tail0 = make_tail(hip, shape, 0)
    for what, args in (("a null bank", (None, tail.h, 1000, 0)), ("a null tail", (bank.h, None, 1000, 0)), ("a tail of block 0", (bank.h, tail0.h, 1000, 0)),
                       ("block_mid shorter than filter + factor", (bank.h, tail.h, 68, 0)), ("input_type 3", (bank.h, tail.h, 1000, 3))):
        h = C.c_void_p(0xdead)
        assert hip.lib.sdrhip_pipe_narrow_bank_audio(C.byref(h), *args) == -1 and not h.value, what
        assert b"sdrhip_pipe_narrow_bank_audio" in hip.lib.sdrhip_last_error(), what
    assert hip.lib.sdrhip_pipe_narrow_bank_audio(None, bank.h, tail.h, 1000, 0) == -1
    assert hip.Pipe.narrow_bank_audio(bank, tail, 69).rows == 2


def test_the_wrong_push_call_is_refused(hip):
    block_mid, shape2, shape, block = COMBOS["4/5"]
    bank = TN.make_bank(hip, TA.tables_for(2), shape2, NB.FM, False)
    tail = make_tail(hip, shape, block)
    data = {f: np.ascontiguousarray(PC.stream(f, B)) for f in PC.FORMATS}
    c0 = counters(hip)
    for fmt in PC.FORMATS:
        p = hip.Pipe.narrow_bank_audio(bank, tail, block_mid, input_u8=fmt == "u8", input_i16=fmt == "i16")
        for other in PC.FORMATS:
            if other == fmt:
                continue
            name, ptr_t = TA.PUSH[other]
            assert getattr(hip.lib, name)(p.h, data[other].ctypes.data_as(ptr_t), B) == -1, f"{other} blocks into a {fmt} pipe"
            assert name.encode() + b":" in hip.lib.sdrhip_last_error()
        assert p.flush() == []
    assert (counters(hip) == c0).all()


def test_pop_against_pop_rows(hip, oracle):
    block_mid, shape2, shape, block = COMBOS["4/5"]
    blocks = PC.cut(PC.stream("cf32", NBLK * B), [B] * NBLK)
    bank = TN.make_bank(hip, TA.tables_for(1), shape2, NB.FM, False)
    tail = make_tail(hip, shape, block)
    p = hip.Pipe.narrow_bank_audio(bank, tail, block_mid)
    q = NarrowAudioPipe(hip, bank, tail, block_mid, "cf32")
    for blk in blocks:
        q.push(blk)
        assert hip.check(hip.lib.sdrhip_pipe_push(p.h, np.ascontiguousarray(blk).ctypes.data_as(TA._f32p), blk.size // 2), "push") >= 0
    q.flush()
    ready = hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush")
    assert ready == sum(q.counts) > 3
    one = []
    for _ in range(ready):
        o = np.empty(block, np.float32)
        assert hip.check(hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(TA._f32p), block), "pop") == block
        one.append(o)
    assert_bit_equal(np.concatenate(one), q.row(0), "pop against pop_rows")
    p2 = hip.Pipe.narrow_bank_audio(TN.make_bank(hip, TA.tables_for(2), shape2, NB.FM, False), tail, block_mid)
    o = np.empty(block, np.float32)
    assert hip.lib.sdrhip_pipe_pop(p2.h, o.ctypes.data_as(TA._f32p), block) == -1


# ---- save / restore ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2], ids=KIND_IDS)
def test_save_and_restore(hip, oracle, kind):
    """Save after 5 of 40 pushes (2048-sample blocks: both carries hold elements) and restore over a second pipe: the rest of the stream
    is the first pipe's and the model's; every refusal leaves the pipe fresh."""
    form, dc = KINDS[kind]
    tables = TA.tables_for(3)
    sizes = [2048] * 40
    combo = "4/5"
    block_mid, shape2, shape, block = COMBOS[combo]
    fmt = PC.FORMATS[kind]
    kw = dict(input_u8=fmt == "u8", input_i16=fmt == "i16")
    bank = TN.make_bank(hip, tables, shape2, form, dc)
    tail = make_tail(hip, shape, block)
    blocks = PC.cut(PC.stream(fmt, 40 * 2048), sizes)
    a = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)
    for blk in blocks[:5]:
        a.push(blk)
    state = a.p.save()
    a2, q = progress(tail, sizes[:5], shape2, block_mid)[-1]
    assert a2 > 0 and q > 0 and a2 > tail.first_input(q), "both carries hold elements at the save"
    b = NarrowAudioPipe(hip, bank, tail, block_mid, fmt)

    def refused(pipe, st, what):
        assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
        assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what

    refused(b.p, state[:-1], "a truncated state")
    refused(b.p, state[:-(3 * (a2 - tail.first_input(q)) * 4 + 9)], "a state cut inside its audio record")
    refused(b.p, state[:60], "a state cut inside its header")
    plain = hip.Pipe.narrow_bank(bank, block_mid, block, **kw)
    refused(plain, state, "a tailed state on a plain narrow pipe")
    plain2 = hip.Pipe.narrow_bank(bank, block_mid, block, **kw)
    for blk in blocks[:5]:
        plain2.push(blk)
    plain_state = plain2.save()
    refused(b.p, plain_state, "a plain narrow pipe's state on a tailed pipe")
    assert plain.restore(plain_state) is not None                                 # ... which its own kind of pipe takes
    other = make_tail(hip, AC.SHAPES["3/5 x 71"], block)
    refused(hip.Pipe.narrow_bank_audio(bank, other, block_mid, **kw), state, "another tail shape")
    half32 = hip.AudioTail(shape.I, shape.D, shape.resamp_taps(), S.taps_audio_half32(), gain=GAIN, block=block)
    refused(hip.Pipe.narrow_bank_audio(bank, half32, block_mid, **kw), state, "another audio filter length")
    refused(hip.Pipe.narrow_bank_audio(TN.make_bank(hip, tables[:2], shape2, form, dc), tail, block_mid, **kw), state, "another row count")
    refused(hip.Pipe.narrow_bank_audio(bank, tail, block_mid, input_u8=fmt != "u8", input_i16=False), state, "another input type")
    refused(hip.Pipe.narrow_bank_audio(bank, tail, 1000, **kw), state, "another block_mid")
    refused(hip.Pipe.narrow_bank_audio(bank, make_tail(hip, shape, 200), block_mid, **kw), state, "another block")
    refused(hip.Pipe.narrow_bank_audio(TN.make_bank(hip, tables, "61/5", form, dc), tail, block_mid, **kw), state, "another second decimator")
    oform, odc = KINDS[(kind + 1) % 3]
    refused(hip.Pipe.narrow_bank_audio(TN.make_bank(hip, tables, shape2, oform, odc), tail, block_mid, **kw), state, "another form or dc_block")
    assert hip.lib.sdrhip_pipe_poll(b.p.h) == 0
    b.restore(state)                                     # ... and after all those refusals the pipe is as fresh as it was
    for blk in blocks[5:]:
        a.push(blk)
        b.push(blk)
    a.flush()
    b.flush()
    check(hip, oracle, a, bank, tables, combo, fmt, sizes, blocks, 40 * 2048, f"the saved pipe, {fmt}")
    nb_before = sum(a.counts[:5])
    for j in range(3):
        assert_bit_equal(b.row(j), a.row(j)[nb_before * block:], f"restored pipe, {fmt}: channel {j}")


def test_a_plain_narrow_pipe_writes_the_state_it_always_wrote(hip):
    """The narrow record's last field is 0 for a plain narrow pipe, and its state's size is the parent's layout's (the hashes of every
    existing kind's state are held by tests/test_gpu_pipe_narrow_bank.py and tests/test_gpu_pipe_state_bytes.py)."""
    tables = TA.tables_for(2)
    bank = TN.make_bank(hip, tables, "24/4", NB.FM, False)
    p = hip.Pipe.narrow_bank(bank, 1024, 100)
    for blk in PC.cut(PC.stream("cf32", 5 * 2048), [2048] * 5):
        p.push(blk)
    st = p.save()
    # [... | PipeStateNarrow (3 int64, 6 int32) | 2 K state floats | K x y_n complex stage-1 outputs]: m = 1265 stage-1 outputs, one
    # block of 1024 seen, a_done = 251 stage-2 outputs done, the carry reaches back to output 1004
    y_n = 1265 - 4 * 251
    rec = st[-(48 + 2 * 2 * 4 + 2 * y_n * 8):][:48]
    a_done, yn, mid = np.frombuffer(rec[:24], np.int64)
    d2, lp2, form, dcb, nf, has_tail = np.frombuffer(rec[24:], np.int32)
    assert (a_done, yn, mid, d2, lp2, form, dcb, nf, has_tail) == (251, y_n, 1024, 4, 24, NB.FM, 0, 4, 0)


# ---- the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc,combo,args", [("am", True, "4/5", []), ("nfm", False, "2/5", ["--s16"])], ids=["am --dc, 4/5, u8", "nfm, 2/5, s16"])
def test_narrow_audio_replay(hip, form, dc, combo, args, tmp_path):
    """examples/narrow_audio_replay against the same Pipe driven from the binding: one f32 audio file per channel."""
    import os
    import subprocess
    from sdr_amd import build as Bld
    Bld.build_examples()                                      # (a no-op where build() has made it already)
    exe = os.path.join(TA.ROOT, "examples", "bin", "narrow_audio_replay")
    assert os.path.exists(exe)
    block_mid, shape2, shape, block = COMBOS[combo]
    fmt = "i16" if "--s16" in args else "u8"
    nblk = 12
    s = PC.stream(fmt, nblk * B)
    cap, tp, tp2, tr, th = (tmp_path / n for n in ("capture.bin", "taps.f32", "taps2.f32", "resamp.f32", "half.f32"))
    s.tofile(cap)
    S.taps_decim127().tofile(tp)
    t2, d2, _ = NB.SHAPES[shape2]
    t2.tofile(tp2)
    shape.resamp_taps().tofile(tr)
    shape.audio_half().tofile(th)
    chans = [(1, 64), (-3, 64), (0, 1)]
    cmd = [exe, str(cap), str(tp), str(tmp_path / "out"), "--channels", ",".join(f"{a}/{b}" for a, b in chans), "--form", form,
           "--narrow", str(tp2), str(d2), "--block-mid", str(block_mid), "--audio", str(tr), str(th), "--ratio", f"{shape.I}/{shape.D}",
           "--gain", str(GAIN), "--block", str(block)] + (["--dc"] if dc else []) + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tables = [hip.tuner_shift_table(a, b) for a, b in chans]
    bank = TN.make_bank(hip, tables, shape2, NB.FM if form == "nfm" else NB.ENV, dc)
    tail = make_tail(hip, shape, block, mode=0)
    p = hip.Pipe.narrow_bank_audio(bank, tail, block_mid, input_u8=fmt == "u8", input_i16=fmt == "i16")
    outs = []
    for blk in PC.cut(s, [B] * nblk):
        outs += p.push(blk)
    outs += p.flush()
    want = np.concatenate(outs, axis=1)
    assert want.shape[0] == 3 and want.shape[1] >= 3 * block and want.shape[1] % block == 0
    for j in range(3):
        got = np.fromfile(str(tmp_path / f"out.ch{j}.f32"), np.float32)
        assert_bit_equal(got, want[j], f"narrow_audio_replay --form {form} {' '.join(args)}: channel {j}")
    # what it requires: both stages, a form, a down-sampling ratio
    for bad in (cmd[:cmd.index("--audio")], cmd[:cmd.index("--form")] + cmd[cmd.index("--form") + 2:], cmd + ["--ratio", "5/4"]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "narrow_audio_replay" in r.stderr, bad
