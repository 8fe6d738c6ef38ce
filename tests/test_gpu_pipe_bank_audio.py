"""GPU parity of the audio Pipes of the two banks (sdrhip_pipe_am_bank_audio, sdrhip_pipe_nfm_bank_audio): host cfloat / u8 / int16 IQ
blocks in, every channel's AUDIO blocks out.

Every row's audio blocks are held, bit for bit, to the composition driven through the host: the existing bank Pipe (Pipe.am_bank /
Pipe.nfm_bank) with block_size_out = block, then per channel a one-row Pipe.fir_resampler and Pipe.fir_filter with the same block,
then one float32 multiply by the gain -- fed the blocks the bank Pipe yields.  Those Pipes are pinned by their own suites.  Two AM
channels are also held to the restated Pipes end to end (tests/pipe_am_bank_cases.py, then tests/audio_tail_cases.py): no device code
in those expected values.  Every pop goes into a buffer of NaN canaries whose words around each row must be canaries afterwards.
Shape: 127 decimator taps, factor 8 or 16, the FM tail (3/10 with 191 taps, 2 x 64 audio taps), gain -0.5."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import audio_tail_cases as AC
import pipe_am_bank_cases as PC
import signals as S
import test_gpu_pipe_am_bank as TA
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

B = PC.B
GAIN = np.float32(-0.5)
_f32p = C.POINTER(C.c_float)
KINDS = ("am dc", "am", "nfm")


def make_bank(hip, kind, tables, factor=8, taps=None):
    tb = hip.TunerBank(factor, S.taps_decim127() if taps is None else taps, tables)
    return hip.NfmBank(tb) if kind == "nfm" else hip.AmBank(tb, dc_block=kind == "am dc")


def make_tail(hip, block, route=0, rt=None, ah=None):
    t = hip.AudioTail(3, 10, AC.resamp_taps() if rt is None else rt, AC.audio_half() if ah is None else ah, gain=float(GAIN), block=block)
    t.set_route(route)
    return t


def bank_pipe(hip, kind, bank, block, fmt):
    make = hip.Pipe.nfm_bank if kind == "nfm" else hip.Pipe.am_bank
    return make(bank, block, input_u8=fmt == "u8", input_i16=fmt == "i16")


class AudioPipe(TA.AmPipe):
    """The audio Pipe through the raw C calls (tests/test_gpu_pipe_am_bank.py's harness: pops into canaries)."""

    def __init__(self, hip, kind, bank, tail, fmt):
        self.hip, self.bo, self.fmt = hip, tail.block, fmt
        make = hip.Pipe.nfm_bank_audio if kind == "nfm" else hip.Pipe.am_bank_audio
        self.p = make(bank, tail, input_u8=fmt == "u8", input_i16=fmt == "i16")
        self.rows = self.p.rows
        self.got = [[] for _ in range(self.rows)]
        self.counts = []


def demod_rows(hip, kind, bank, block, fmt, blocks):
    """Every row's demodulated blocks as the existing bank Pipe yields them for these pushes: a list of [K, block] arrays."""
    bp = bank_pipe(hip, kind, bank, block, fmt)
    out = []
    for blk in blocks:
        out += bp.push(blk)
    return out + bp.flush()


def host_composition(hip, ys, rows, block):
    """{row: audio} of the chosen rows: their demodulated blocks through one-row firResampler and firFilter Pipes, then * gain."""
    res, fil = hip.Resampler(3, 10, AC.resamp_taps()), hip.Filter(AC.audio_half(), sym=True)
    out = {}
    for j in rows:
        rp, fp = hip.Pipe("resampler", res, block), hip.Pipe("filter", fil, block)
        zs = []
        for y in ys:
            zs += rp.push(y[j])
        zs += rp.flush()
        a = []
        for z in zs:
            a += fp.push(z)
        a += fp.flush()
        out[j] = np.concatenate(a) * GAIN if a else np.empty(0, np.float32)
    return out


def device_composition(hip, ys, block):
    """Every row's audio blocks by ONE composed run (route 2, pinned by tests/test_gpu_audio_tail.py) over the demodulated rows."""
    import gpu_util
    y = np.ascontiguousarray(np.concatenate(ys, axis=1))
    tail = make_tail(hip, block, route=2)
    n = tail.ready(y.shape[1]) // block * block
    d_y, d_a = gpu_util.to_dev(y), gpu_util.dev_empty_f32(y.shape[0] * max(n, 1)).view(y.shape[0], max(n, 1))
    if n:
        import torch
        ws = torch.empty(tail.workspace_bytes(y.shape[0], y.shape[1]), dtype=torch.uint8, device="cuda")
        tail.run_rows(d_y, d_a[:, :n], 0, n, workspace=ws)
    return gpu_util.to_host(d_a)[:, :n].copy()


def check(hip, ap, kind, bank, fmt, blocks, block, what, host_rows=None):
    """The Pipe's rows against the composition.  The bank Pipe with block_size_out = block hands the stages behind it whole blocks
    only, so driven through the host the composition lags the audio Pipe (which takes every demodulated output as it comes) by up
    to a block of demodulated outputs: every block it yields is compared.  The demodulated STREAM does not depend on block_size_out
    (the same Pipe with blocks of 8 gives all of it but the last 7 outputs), and the composed run over that stream gives every audio
    block the Pipe can have yielded, but for a last one those 7 outputs complete."""
    ys = demod_rows(hip, kind, bank, block, fmt, blocks)
    dev = device_composition(hip, demod_rows(hip, kind, bank, 8, fmt, blocks), block)
    assert dev.shape[1] > 0 and dev.shape[1] % block == 0, what
    host_rows = range(ap.rows) if host_rows is None else host_rows
    host = host_composition(hip, ys, host_rows, block) if ys else {}
    for j in range(ap.rows):
        got = ap.row(j)
        assert got.size - dev.shape[1] in (0, block), f"{what}: channel {j}: {got.size} audio outputs, the composition yields {dev.shape[1]}"
        assert_bit_equal(got[:dev.shape[1]], dev[j], f"{what}: channel {j} against the composed run over the bank Pipe's stream")
        if j in host:
            assert host[j].size <= got.size and host[j].size % block == 0
            assert_bit_equal(got[:host[j].size], host[j], f"{what}: channel {j} against the Pipes driven through the host")
    assert np.isfinite(ap.row(0)).all() and np.abs(ap.row(0)).max() > 0
    return min(len(h) for h in host.values()) if host else 0


def bank_counters(hip, kind):
    if kind == "nfm":
        return np.array([hip.nfm_bank_launches(), hip.nfm_bank_cross_launches()])
    return np.array([hip.am_bank_launches(), hip.am_bank_cross_launches()])


# (kind, channels, input type, factor, source blocks per submission)
UNIFORM = [("am dc", 2, "u8", 8, 1), ("am", 2, "cf32", 8, 3), ("nfm", 2, "i16", 8, 1), ("am dc", 2, "i16", 16, 16), ("nfm", 2, "u8", 16, 3),
           ("nfm", 2, "cf32", 16, 1), ("am dc", 1, "cf32", 16, 3), ("nfm", 1, "u8", 8, 16), ("am", 32, "i16", 8, 1), ("nfm", 32, "u8", 16, 16),
           ("am dc", 32, "u8", 16, 3)]


@pytest.mark.parametrize("kind,nch,fmt,factor,group", UNIFORM, ids=[f"{k}, {n} ch, {f}, /{d}, {g} per submission" for k, n, f, d, g in UNIFORM])
def test_uniform_pushes(hip, kind, nch, fmt, factor, group):
    """8192-sample blocks, audio block 8192, the tail on route 1: the bank Pipe's launch counts, ONE tail launch per submission that
    completes audio and none otherwise."""
    block = 8192
    nblk = 57 * factor // 8                 # 7 whole blocks of 8192 demodulated outputs, 2 of z: the host-driven composition yields a block too
    tables = TA.tables_for(nch)
    bank = make_bank(hip, kind, tables, factor)
    tail = make_tail(hip, block, route=1)
    blocks = PC.cut(PC.stream(fmt, nblk * B), [B] * nblk)
    ap = AudioPipe(hip, kind, bank, tail, fmt)
    assert ap.rows == nch
    ap.p.set_adaptive(0)
    if group > 1:
        ap.p.set_coalesce(group)
    c0, f0, r0 = bank_counters(hip, kind), hip.audio_tail_launches(), hip.fir_rows_launches()
    with_audio, m, a = 0, 0, 0
    for i, blk in enumerate(blocks):
        ap.push(blk)
        if (i + 1) % group == 0:
            m2 = ((i + 1) * B - PC.LP) // factor + 1
            a2 = tail.ready(m2)
            with_audio += a2 > a
            m, a = m2, a2
    ap.flush()
    if nblk % group:
        a2 = tail.ready((nblk * B - PC.LP) // factor + 1)
        with_audio += a2 > a
    what = f"{kind}, {nch} channels, {fmt}, factor {factor}, {group} blocks per submission"
    subs = -(-nblk // group)
    assert tuple(bank_counters(hip, kind) - c0) == (subs, 0), what
    assert hip.audio_tail_launches() - f0 == with_audio and 0 < with_audio <= subs and hip.fir_rows_launches() == r0, what
    assert check(hip, ap, kind, bank, fmt, blocks, block, what, host_rows=None if nch <= 2 else (0, 17, 31)) >= block
    assert sum(c for c in ap.counts if c > 0) == ap.row(0).size // block >= 1


def test_on_auto_the_pipe_takes_the_fused_kernel_where_the_rule_says(hip):
    """The Pipes' runs read padded y rows behind a carried history (the "y-strided" layout of tools/audio_tail_bench.py): on auto a
    submission that completes 153 .. 314574 audio outputs per row takes the fused kernel, one that completes fewer the composition."""
    tables = TA.tables_for(3)
    block = 8192
    for kind, fmt, factor, n in (("nfm", "u8", 8, B), ("am dc", "i16", 16, B), ("am", "cf32", 16, 3 * B)):
        bank, tail = make_bank(hip, kind, tables, factor), make_tail(hip, block, route=0)
        nblk = 12
        ap = AudioPipe(hip, kind, bank, tail, fmt)
        ap.p.set_adaptive(0)
        done, seen = 0, set()
        for i, blk in enumerate(PC.cut(PC.stream(fmt, nblk * n), [n] * nblk)):
            f0, r0 = hip.audio_tail_launches(), hip.fir_rows_launches()
            ap.push(blk)
            a = tail.ready(((i + 1) * n - PC.LP) // factor + 1)
            fused, composed = hip.audio_tail_launches() - f0, hip.fir_rows_launches() - r0
            want = "none" if a == done else "fused" if 153 <= a - done <= 314574 else "composed"
            assert (fused, composed) == {"none": (0, 0), "fused": (1, 0), "composed": (0, 2)}[want], \
                f"{kind}, {fmt}, factor {factor}, push {i}: {a - done} audio outputs, {fused} fused launches, {composed} row-form launches"
            seen.add(want)
            done = a
        assert "fused" in seen and (factor == 8 or n > B or "composed" in seen), seen
        ap.flush()


def test_block_1000_takes_the_composed_route(hip):
    tables = TA.tables_for(3)
    for kind, fmt in (("am dc", "u8"), ("nfm", "cf32")):
        bank, tail = make_bank(hip, kind, tables), make_tail(hip, 1000)
        assert not tail.fused_fits()
        blocks = PC.cut(PC.stream(fmt, 12 * B), [B] * 12)
        ap = AudioPipe(hip, kind, bank, tail, fmt)
        ap.p.set_adaptive(0)
        f0, r0 = hip.audio_tail_launches(), hip.fir_rows_launches()
        for blk in blocks:
            ap.push(blk)
        ap.flush()
        assert hip.audio_tail_launches() == f0 and hip.fir_rows_launches() > r0
        check(hip, ap, kind, bank, fmt, blocks, 1000, f"block 1000, {kind}, {fmt}")


@pytest.mark.parametrize("mode", ["plain", "coalesce 7", "adaptive 32"])
@pytest.mark.parametrize("kind,fmt", [("am dc", "u8"), ("nfm", "i16"), ("am", "cf32")])
def test_ragged_pushes(hip, kind, fmt, mode):
    """Seeded block sizes, odd ones included, every third push through input_buffer; auto route, audio block 1500 (composed) and the
    smallest block the fused kernel takes."""
    sizes = TA.ragged_sizes(n=36, seed=11)
    total = 2 * sum(sizes) // 2
    tables = TA.tables_for(3)
    for block in (1500, AC.MIN_BLOCK):
        bank, tail = make_bank(hip, kind, tables), make_tail(hip, block)
        ap = AudioPipe(hip, kind, bank, tail, fmt)
        if mode == "plain":
            ap.p.set_adaptive(0)
        elif mode == "coalesce 7":
            ap.p.set_coalesce(7)
        else:
            ap.p.set_adaptive(32)
        blocks = PC.cut(PC.stream(fmt, total), sizes)
        for i, blk in enumerate(blocks):
            ap.push(blk, via_buffer=(i % 3 == 1))
        ap.flush()
        check(hip, ap, kind, bank, fmt, blocks, block, f"ragged pushes, {mode}, {kind}, {fmt}, block {block}")


def test_pushes_that_complete_no_audio_launch_no_tail(hip):
    """Blocks of 2048 samples at factor 16 are 128 demodulated outputs: the first three pushes complete no audio output (488 inputs are
    one receptive field), the bank part still runs; later pushes alternate."""
    tables = TA.tables_for(3)
    for kind, fmt in (("nfm", "u8"), ("am dc", "i16")):
        bank, tail = make_bank(hip, kind, tables, 16), make_tail(hip, 512, route=2)
        n, nb = 2048, 40
        blocks = PC.cut(PC.stream(fmt, nb * n), [n] * nb)
        ap = AudioPipe(hip, kind, bank, tail, fmt)
        ap.p.set_adaptive(0)
        done = 0
        for i, blk in enumerate(blocks):
            c0, r0 = bank_counters(hip, kind), hip.fir_rows_launches()
            ap.push(blk)
            a = tail.ready(((i + 1) * n - PC.LP) // 16 + 1)
            assert (bank_counters(hip, kind) - c0)[0] == 1, f"push {i}: the bank part runs whether audio completes or not"
            assert (hip.fir_rows_launches() > r0) == (a > done), f"push {i}: {a - done} audio outputs completed"
            if i < 3:
                assert a == 0
            done = a
        ap.flush()
        check(hip, ap, kind, bank, fmt, blocks, 512, f"small pushes, {kind}, {fmt}")


def test_two_hundred_pushes_in_flight(hip):
    n, nb = 1024, 200
    tables = TA.tables_for(3)
    for kind, fmt, route in (("am dc", "u8", 1), ("nfm", "cf32", 0)):
        bank, tail = make_bank(hip, kind, tables), make_tail(hip, AC.MIN_BLOCK, route=route)
        blocks = PC.cut(PC.stream(fmt, nb * n), [n] * nb)
        ap = AudioPipe(hip, kind, bank, tail, fmt)
        ap.p.set_adaptive(0)
        for blk in blocks:
            ap.push(blk)
        ap.flush()
        check(hip, ap, kind, bank, fmt, blocks, AC.MIN_BLOCK, f"200 pushes, {kind}, {fmt}")


def test_the_wrong_push_call_is_refused_and_the_state_size_is_exact(hip):
    tables = TA.tables_for(2)
    data = {f: np.ascontiguousarray(PC.stream(f, B)) for f in PC.FORMATS}
    for kind in ("am dc", "nfm"):
        bank, tail = make_bank(hip, kind, tables), make_tail(hip, 1000)
        for fmt in PC.FORMATS:
            ap = AudioPipe(hip, kind, bank, tail, fmt)
            for other in PC.FORMATS:
                if other == fmt:
                    continue
                name, ptr_t = TA.PUSH[other]
                assert getattr(hip.lib, name)(ap.p.h, data[other].ctypes.data_as(ptr_t), B) == -1, f"{other} blocks into a {fmt} pipe"
                assert name.encode() + b":" in hip.lib.sdrhip_last_error()
                with pytest.raises(hip.SdrHipError):
                    ap.p.push(data[other])
                buf = {"cf32": hip.lib.sdrhip_pipe_input_buffer, "u8": hip.lib.sdrhip_pipe_input_buffer_u8, "i16": hip.lib.sdrhip_pipe_input_buffer_i16}
                assert not buf[other](ap.p.h, 16) and buf[fmt](ap.p.h, 16)
            assert ap.p.flush() == []
            # a fresh pipe: the bank Pipe's state, the audio record (two int64, four int32) and no carried rows; after a push, K rows of them
            fresh = ap.p.save()
            twin = bank_pipe(hip, kind, bank, 1000, fmt).save()
            assert len(fresh) == len(twin) + 32
            ap.push(data[fmt])
            hip.lib.sdrhip_pipe_state_bytes.restype = C.c_size_t
            hip.lib.sdrhip_pipe_state_bytes.argtypes = [C.c_void_p]
            nbytes = hip.lib.sdrhip_pipe_state_bytes(ap.p.h)
            st = ap.p.save()
            m = (B - PC.LP) // 8 + 1
            carried = m - tail.first_input(tail.ready(m))
            assert len(st) == nbytes and 0 < carried <= tail.max_halo()
            bp = bank_pipe(hip, kind, bank, 1000, fmt)
            bp.push(data[fmt])
            bp.flush()
            # (the bank Pipe alone has yielded 1000 of its 1009 outputs as a block; the audio Pipe holds 157 audio outputs that fill no block)
            a = tail.ready(m)
            assert len(st) - 32 - 4 * 2 * carried - 4 * 2 * a == len(bp.save()) - 4 * 2 * (m - m // 1000 * 1000)


def test_pop_against_pop_rows(hip):
    blocks = PC.cut(PC.stream("cf32", 24 * B), [B] * 24)
    bank, tail = make_bank(hip, "am dc", TA.tables_for(1)), make_tail(hip, 1000)
    ap = AudioPipe(hip, "am dc", bank, tail, "cf32")
    p = ap.p
    assert p.rows == 1
    for blk in blocks:
        hip.check(hip.lib.sdrhip_pipe_push(p.h, np.ascontiguousarray(blk).ctypes.data_as(_f32p), B), "push")
    ready = hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush")
    assert ready == tail.ready((24 * B - PC.LP) // 8 + 1) // 1000 >= 6
    for k in range(ready):
        if k % 2:
            ap.got[0].append(p.pop_rows(1).reshape(-1))
        else:
            o = np.empty(1000, np.float32)
            assert hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(_f32p), 999) == -1
            assert hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(_f32p), 1000) == 1000
            ap.got[0].append(o)
    check(hip, ap, "am dc", bank, "cf32", blocks, 1000, "pop and pop_rows, one channel")
    bank3 = make_bank(hip, "nfm", TA.tables_for(3))
    q = AudioPipe(hip, "nfm", bank3, tail, "cf32")
    for blk in blocks[:8]:
        hip.check(hip.lib.sdrhip_pipe_push(q.p.h, np.ascontiguousarray(blk).ctypes.data_as(_f32p), B), "push")
    n = hip.check(hip.lib.sdrhip_pipe_flush(q.p.h), "flush")
    o = np.full(3 * n * 1000, TA.CANARY, np.uint32)
    assert n >= 2 and hip.lib.sdrhip_pipe_pop(q.p.h, o.view(np.float32).ctypes.data_as(_f32p), n * 1000) == -1 and (o == TA.CANARY).all()
    assert q.p.pop_rows(n).shape == (3, n, 1000)


def test_save_and_restore(hip):
    """Save after 5 of 40 pushes (2048-sample blocks) and restore into a twin: the rest of the stream is the composition's; every
    refusal leaves the pipe as fresh as it was: a pipe of each refused class is then driven beside a fresh twin of itself."""
    tables = TA.tables_for(3)
    sizes = [2048] * 40
    block = 700
    for kind, fmt in (("am dc", "u8"), ("nfm", "i16"), ("am", "cf32")):
        kw = dict(input_u8=fmt == "u8", input_i16=fmt == "i16")
        bank, tail = make_bank(hip, kind, tables), make_tail(hip, block)
        audio = hip.Pipe.nfm_bank_audio if kind == "nfm" else hip.Pipe.am_bank_audio
        blocks = PC.cut(PC.stream(fmt, 40 * 2048), sizes)
        a = AudioPipe(hip, kind, bank, tail, fmt)
        for blk in blocks[:5]:
            a.push(blk)
        state = a.p.save()
        b = AudioPipe(hip, kind, bank, tail, fmt)

        def refused(pipe, st, what):
            assert hip.lib.sdrhip_pipe_restore(pipe.h, st, C.c_size_t(len(st))) == -1, what
            assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), what

        def drive(pipe):
            """24 pushes of the stream in the pipe's own input type -> every block it yields, [rows, floats]"""
            f2 = "u8" if pipe.input_u8 else "i16" if pipe.input_i16 else "cf32"
            outs = []
            for blk in PC.cut(PC.stream(f2, 40 * 2048), sizes)[:24]:
                outs += pipe.push(blk)
            outs += pipe.flush()
            assert outs, "24 pushes yield at least one block"
            return np.concatenate(outs, axis=1)

        def refused_then_fresh(make, st, what):
            """restore refuses `st` on make()'s pipe, and that pipe then yields what a fresh twin yields"""
            pipe, twin = make(), make()
            refused(pipe, st, what)
            assert hip.lib.sdrhip_pipe_poll(pipe.h) == 0, what
            assert_bit_equal(drive(pipe).ravel(), drive(twin).ravel(), f"{what}: the refused pipe against a fresh twin, {kind}, {fmt}")

        refused(b.p, state[:-1], "a truncated state")
        refused(b.p, state[:-4 * 3 * 100], "a state cut inside its carried rows")
        refused(b.p, state[:60], "a state cut inside its header")
        refused_then_fresh(lambda: audio(bank, tail, **kw), state[:-1], "a truncated state")
        refused_then_fresh(lambda: audio(make_bank(hip, kind, tables[:2]), tail, **kw), state, "another row count")
        refused_then_fresh(lambda: audio(bank, tail, input_u8=fmt != "u8", input_i16=False), state, "another input type")
        refused_then_fresh(lambda: audio(bank, make_tail(hip, block + 1), **kw), state, "another block")
        refused_then_fresh(lambda: audio(make_bank(hip, kind, tables, factor=16), tail, **kw), state, "another factor")
        refused_then_fresh(lambda: audio(make_bank(hip, kind, tables, taps=S.gauss_taps(64, 104)), tail, **kw), state, "another tap count")
        other_kind = "am dc" if kind == "nfm" else "nfm"
        other_audio = hip.Pipe.nfm_bank_audio if other_kind == "nfm" else hip.Pipe.am_bank_audio
        refused_then_fresh(lambda: other_audio(make_bank(hip, other_kind, tables), tail, **kw), state, "another kind")
        refused_then_fresh(lambda: bank_pipe(hip, kind, bank, block, fmt), state, "the bank Pipe without audio")
        if kind != "nfm":
            refused_then_fresh(lambda: audio(make_bank(hip, "am" if kind == "am dc" else "am dc", tables), tail, **kw), state, "another dc_block")
        t25 = hip.AudioTail(2, 5, AC.resamp_taps(), AC.audio_half(), gain=float(GAIN), block=block)
        refused_then_fresh(lambda: audio(bank, t25, **kw), state, "another resampler ratio")
        refused_then_fresh(lambda: audio(bank, make_tail(hip, block, rt=S.taps_resamp31()), **kw), state, "another resampler tap count")
        refused_then_fresh(lambda: audio(bank, make_tail(hip, block, ah=S.taps_audio_half32()), **kw), state, "another audio tap count")
        bp = bank_pipe(hip, kind, bank, block, fmt)
        bp.push(blocks[0])
        refused(b.p, bp.save(), "a bank Pipe's state")
        assert hip.lib.sdrhip_pipe_poll(b.p.h) == 0
        b.restore(state)                                     # ... and after all those refusals the pipe is as fresh as it was
        for blk in blocks[5:]:
            a.push(blk)
            b.push(blk)
        a.flush()
        b.flush()
        check(hip, a, kind, bank, fmt, blocks, block, f"the saved pipe, {kind}, {fmt}")
        nb_before = sum(c for c in a.counts[:5] if c > 0)
        for j in range(3):
            assert_bit_equal(b.row(j), a.row(j)[nb_before * block:], f"restored pipe, {kind}, {fmt}: channel {j}")


def test_saved_states_of_every_older_kind_keep_their_bytes(hip):
    states = PC.existing_kind_states(hip)
    assert set(states) == set(PC.PARENT_STATE_SHA256)
    for kind, st in states.items():
        assert hashlib.sha256(st).hexdigest() == PC.PARENT_STATE_SHA256[kind], f"the saved state of a {kind} pipe changed"


def test_two_channels_against_the_restated_pipes_end_to_end(hip, oracle):
    """u8 IQ -> mix, firDecimator Pipe, magnitude, dcBlocker (tests/pipe_am_bank_cases.py) -> firResampler, firFilter, gain
    (tests/audio_tail_cases.py), every stage the model's."""
    tables = TA.tables_for(2)
    nblk, block = 30, 8192
    sizes = [B] * nblk
    for dc in (True, False):
        kind = "am dc" if dc else "am"
        bank, tail = make_bank(hip, kind, tables), make_tail(hip, block)
        ap = AudioPipe(hip, kind, bank, tail, "u8")
        for blk in PC.cut(PC.stream("u8", nblk * B), sizes):
            ap.push(blk)
        ap.flush()
        for j, t in enumerate(tables):
            y = PC.expected(oracle, t, "u8", sizes, dc, nblk * B)
            exp = AC.expected_from(oracle, y, block, GAIN)
            got = ap.row(j)
            assert got.size == exp.size // block * block >= block
            assert_bit_equal(got, exp[:got.size], f"end to end against the models, dc_block {dc}, channel {j}")


# ---- the examples ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exe_name,args", [("nfm_replay", []), ("nfm_replay", ["--s16", "--ratio", "3/10", "--gain", "-0.5"]),
                                           ("airband_replay", ["--gain", "-0.5"]), ("airband_replay", ["--s16", "--no-dc"])])
def test_replay_examples_with_audio(hip, exe_name, args, tmp_path):
    """examples/nfm_replay.c and examples/airband_replay.c with --audio against the same Pipe driven from the binding."""
    import os
    import subprocess
    exe = os.path.join(TA.ROOT, "examples", "bin", exe_name)
    assert os.path.exists(exe), "build() makes the examples"
    fmt = "i16" if "--s16" in args else "u8"
    nblk, block = 24, 1024
    s = PC.stream(fmt, nblk * B)
    cap, tp, rp, hp = tmp_path / "capture.bin", tmp_path / "taps.f32", tmp_path / "resamp.f32", tmp_path / "half.f32"
    s.tofile(cap)
    S.taps_decim127().tofile(tp)
    AC.resamp_taps().tofile(rp)
    AC.audio_half().tofile(hp)
    chans = [(1, 64), (-3, 64), (0, 1)]
    r = subprocess.run([exe, str(cap), str(tp), str(tmp_path / "out"), "--channels", ",".join(f"{a}/{b}" for a, b in chans), "--block-out", str(block),
                        "--audio", str(rp), str(hp)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    tables = [hip.tuner_shift_table(a, b) for a, b in chans]
    tb = hip.TunerBank(8, S.taps_decim127(), tables)
    gain = -0.5 if "--gain" in args else 1.0
    tail = hip.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), gain=gain, block=block)
    if exe_name == "nfm_replay":
        p = hip.Pipe.nfm_bank_audio(hip.NfmBank(tb), tail, input_u8=fmt == "u8", input_i16=fmt == "i16")
    else:
        p = hip.Pipe.am_bank_audio(hip.AmBank(tb, dc_block="--no-dc" not in args), tail, input_u8=fmt == "u8", input_i16=fmt == "i16")
    outs = []
    for blk in PC.cut(s, [B] * nblk):
        outs += p.push(blk)
    outs += p.flush()
    want = np.concatenate(outs, axis=1)
    assert want.shape == (3, tail.ready((nblk * B - PC.LP) // 8 + 1) // block * block) and want.shape[1] >= 6 * block
    for j in range(3):
        got = np.fromfile(str(tmp_path / f"out.ch{j}.f32"), np.float32)
        assert_bit_equal(got, want[j], f"{exe_name} --audio {' '.join(args)}: channel {j}")
