"""GPU parity of a bank's host-block stream on 16-bit signed IQ (sdrhip_fm_stream_create_bank_i16): int16 host blocks in, every
station's audio blocks out.  Definition: station j's blocks are those of sdrhip_fm_bank_run_i16's hand-driven composition
(test_gpu_fm_bank_i16.compose) run over the whole stream -- whatever the push sizes, coalescing, adaptive submission or route.
Expected values are never taken from a bank or its stream."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fm_bank_i16_cases as FC
import signals as S
import test_gpu_fm_bank_i16 as FB
import test_gpu_tuned_chain as T
from conftest import assert_bit_equal
from gpu_util import ptr

pytestmark = pytest.mark.gpu

B = FC.B
ERR_ARG = -1
RAGGED = [1, 3, 2, 16, 5, 1, 1, 7, 16, 4, 2, 1, 9, 16, 12]


def _rows(got, K, block_out=B):
    for g in got:
        assert g.shape == (K, block_out) and g.dtype == np.float32
    return np.concatenate(got, axis=1) if got else np.zeros((K, 0), np.float32)


def _check(hip, names, rows, total, what, block=B):
    q1 = FB._bank(hip, names[:1], block).ready(total)
    for j, name in enumerate(names):
        ref = FB.compose(hip, name, ptr(FB.dev()), 0, 0, q1, block=block)
        assert rows.shape[1] <= ref.size
        FB.same_bits(rows[j], ref[:rows.shape[1]], f"{what}: station {j} ({name}) vs the hand-driven composition")


def _push_all(st, i16, sizes, inplace_every=0, unit=B):
    got, pos = [], 0
    for k, n in enumerate(sizes):
        chunk = i16[2 * pos * unit:2 * (pos + n) * unit]
        if inplace_every and k % inplace_every == 0:
            view = st.input_buffer_i16(n * unit)[:chunk.size]
            view[:] = chunk
            got += st.push_i16(view)
        else:
            got += st.push_i16(chunk)
        pos += n
    return got


def _submissions_with_output(bank, sizes, unit=B):
    n, count = 0, 0
    for s in sizes:
        count += bank.ready((n + s) * unit) > bank.ready(n * unit)
        n += s
    return count


# ---- uniform pushes ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks_per_push", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 2, 32])
def test_uniform_pushes(hip, K, blocks_per_push):
    """96 source blocks, audio blocks of 8192; adaptive submission off, so every push is a submission: exactly one banked int16
    launch per submission that completes an output, and no launch of the chains' own (neither the one-kernel chain nor the tuner)."""
    names = {1: ["shift 1/65536"], 2: ["shift 1/4", "shift -3/1000"], 32: [FC.NAMES[j % len(FC.NAMES)] for j in range(32)]}[K]
    nblk = FC.NBLK
    i16 = FC.stream()
    bank = FB._bank(hip, names)
    _check(hip, names, np.zeros((K, 0), np.float32), nblk * B, "references first")      # their launches stay out of the counts
    st = hip.FmStream(bank, blocks_per_push * B, B, input_i16=True)
    assert st.rows() == K
    st.set_adaptive(0)
    sizes = [blocks_per_push] * (nblk // blocks_per_push)
    c0 = FB.counters(hip)
    got = _push_all(st, i16, sizes) + st.flush()
    c1 = FB.counters(hip)
    assert c1[0] - c0[0] == c1[1] - c0[1] == _submissions_with_output(bank, sizes) == len(sizes)
    assert c1[2:] == c0[2:], "a bank's stream launched a chain's or a tuner's kernel"
    rows = _rows(got, K)
    assert rows.shape[1] == bank.ready(nblk * B) // B * B == 3 * B
    _check(hip, names, rows, nblk * B, f"{K} stations, {blocks_per_push} blocks per push")


# ---- ragged pushes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [None, ("coalesce", 7), ("adaptive", 32)], ids=["plain", "coalesce 7", "adaptive 32"])
def test_ragged_pushes(hip, setting):
    names = ["shift 1/4", "random, period 5", "shift -3/1000"]
    nblk = FC.NBLK
    assert sum(RAGGED) == nblk and any(s % 2 for s in RAGGED)
    st = hip.FmStream(FB._bank(hip, names), 16 * B, B, input_i16=True)
    if setting:
        getattr(st, "set_" + setting[0])(setting[1] * B)
    rows = _rows(_push_all(st, FC.stream(), RAGGED, inplace_every=3) + st.flush(), 3)
    assert rows.shape[1] == 3 * B
    _check(hip, names, rows, nblk * B, f"ragged pushes ({setting})")


def test_pushes_that_complete_no_output(hip):
    """Seam block 1024, pushes of 1024 samples: the first three complete no output (no launch, nothing to pop)."""
    names = ["shift -3/1000", "shift 1/4"]
    unit, npush, block_out = 1024, 40, 64
    bank = FB._bank(hip, names, unit)
    assert [bank.ready(k * unit) for k in range(1, 5)] == [0, 0, 0, 3]
    i16 = FC.stream(5)
    _check(hip, names, np.zeros((2, 0), np.float32), npush * unit, "references first", block=unit)
    st = hip.FmStream(bank, unit, block_out, input_i16=True)
    st.set_adaptive(0)
    assert st.flush() == []
    c0 = FB.counters(hip)
    got = []
    for k in range(3):
        got += st.push_i16(i16[2 * k * unit:2 * (k + 1) * unit])
    got += st.poll()
    assert got == [] and FB.counters(hip) == c0, "a push that completes no output launched something"
    for k in range(3, npush):
        got += st.push_i16(i16[2 * k * unit:2 * (k + 1) * unit])
    got += st.flush()
    assert hip.fm_bank_i16_launches() - c0[1] == _submissions_with_output(bank, [1] * npush, unit) == npush - 3
    rows = _rows(got, 2, block_out)
    assert rows.shape[1] == bank.ready(npush * unit) // block_out * block_out > 20 * block_out
    _check(hip, names, rows, npush * unit, "1024-sample pushes", block=unit)


# ---- the wrong call ----------------------------------------------------------------------------------------------------------------
def test_wrong_push_call(hip):
    names = ["shift 1/4", "shift -3/1000"]
    i16 = FC.stream(2)
    u8 = T.stream_u8(2)
    s16 = hip.FmStream(FB._bank(hip, names), 2 * B, 256, input_i16=True)
    s8 = hip.FmStream(FB._bank(hip, names), 2 * B, 256)
    lib = hip.lib
    assert lib.sdrhip_fm_stream_push(s16.h, u8.ctypes.data_as(C.POINTER(C.c_uint8)), B) == ERR_ARG
    assert b"int16" in lib.sdrhip_last_error()
    assert not lib.sdrhip_fm_stream_input_buffer(s16.h) and b"int16" in lib.sdrhip_last_error()
    assert lib.sdrhip_fm_stream_push_i16(s8.h, i16.ctypes.data_as(C.c_void_p), B) == ERR_ARG
    assert b"u8" in lib.sdrhip_last_error()
    assert not lib.sdrhip_fm_stream_input_buffer_i16(s8.h) and b"u8" in lib.sdrhip_last_error()
    with pytest.raises(hip.SdrHipError):
        hip.FmStream(T._chain(hip, FC.table("shift 1/4")), 2 * B, 256, input_i16=True)
    # nothing was staged: a flush yields nothing, and both streams work on
    assert s16.flush() == [] and s8.flush() == []
    rows = _rows(s16.push_i16(i16[:4 * B]) + s16.flush(), 2, 256)
    assert rows.shape[1] > 0
    _check(hip, names, rows, 2 * B, "an int16 stream that refused a u8 push")
    assert len(s8.push(u8[:4 * B]) + s8.flush()) > 0


# ---- save and restore --------------------------------------------------------------------------------------------------------------
def test_save_and_restore(hip):
    names = ["shift -3/1000", "shift 1/4", "random, period 5"]
    nblk, block_out = 40, 2048
    i16 = FC.stream(nblk)
    first = hip.FmStream(FB._bank(hip, names), 8 * B, block_out, input_i16=True)
    got = _push_all(first, i16, [1] * 5)
    state = first.save()
    assert hip.lib.sdrhip_fm_stream_state_bytes(first.h) == len(state)
    version, = np.frombuffer(state, np.uint32, 1, 4)
    n_seen, q_done, _, hist_n, pending = (int(v) for v in np.frombuffer(state, np.int64, 5, 8))
    assert version == 3 and np.frombuffer(state, np.int64, 1, 64)[0] == 3, "an int16 state has its own version and carries the row count"
    assert n_seen == 5 * B and q_done == first.chain.ready(5 * B)
    assert len(state) == 64 + 8 + 4 * hist_n + 3 * 4 * pending, "the history is int16 IQ, 4 bytes a sample"
    hist = np.frombuffer(state, np.int16, 2 * hist_n, 72)
    assert np.array_equal(hist, i16[2 * (5 * B - hist_n):2 * 5 * B]), "the history holds the stream's last samples as they came"
    del first
    second = hip.FmStream(FB._bank(hip, names), 8 * B, block_out, input_i16=True)
    got += second.restore(state)
    got += _push_all(second, i16[2 * 5 * B:], [1] * (nblk - 5)) + second.flush()
    rows = _rows(got, 3, block_out)
    assert rows.shape[1] == second.chain.ready(nblk * B) // block_out * block_out
    _check(hip, names, rows, nblk * B, "saved after 5 of 40 pushes, restored over a second bank")

    def refuses(st, blob, what):
        rc = hip.lib.sdrhip_fm_stream_restore(st.h, blob, len(blob))
        assert rc == ERR_ARG and b"sdrhip_fm_stream_restore" in hip.lib.sdrhip_last_error(), what

    # a u8 state on an int16 stream and the reverse; u8 states keep their versions
    u8 = T.stream_u8(nblk)
    u8_first = hip.FmStream(FB._bank(hip, names), 8 * B, block_out)
    T._push_all(u8_first, u8, [1] * 5)
    u8_state = u8_first.save()
    assert np.frombuffer(u8_state, np.uint32, 1, 4)[0] == 2
    one8 = hip.FmStream(FB._bank(hip, names[:1]), 8 * B, block_out)
    T._push_all(one8, u8, [1] * 5)
    assert np.frombuffer(one8.save(), np.uint32, 1, 4)[0] == 1, "a one-row u8 state keeps its version"
    s16 = hip.FmStream(FB._bank(hip, names), 8 * B, block_out, input_i16=True)
    refuses(s16, u8_state, "a u8 state on an int16 stream")
    s8 = hip.FmStream(FB._bank(hip, names), 8 * B, block_out)
    refuses(s8, state, "an int16 state on a u8 stream")
    two = hip.FmStream(FB._bank(hip, names[:2]), 8 * B, block_out, input_i16=True)
    refuses(two, state, "a 3-station state into a 2-station stream")
    refuses(s16, state[:-4], "a truncated state")
    refuses(s16, state[:68], "a state cut inside its row count")
    # the refusing streams work on, and s16 takes the state it was refused a truncated copy of
    rows = _rows(_push_all(two, i16, [2] * 10) + two.flush(), 2, block_out)
    _check(hip, names[:2], rows, 20 * B, "a stream that refused a state")
    assert len(s8.restore(u8_state)) == 0
    assert len(s16.restore(state)) == 0


# ---- pop ---------------------------------------------------------------------------------------------------------------------------
def test_pop_against_pop_rows_on_one_station(hip):
    name = "shift -3/1000"
    nblk = 56
    i16 = FC.stream(nblk)
    outs = {}
    for how in ("pop", "pop_rows"):
        st = hip.FmStream(FB._bank(hip, [name]), 16 * B, 2048, input_i16=True)
        assert st.rows() == 1
        got, pos = [], 0
        for n in RAGGED[:10] + [0]:
            chunk = np.ascontiguousarray(i16[2 * pos * B:2 * (pos + n) * B])
            ready = hip.lib.sdrhip_fm_stream_push_i16(st.h, chunk.ctypes.data_as(C.c_void_p), chunk.size // 2) if n else hip.lib.sdrhip_fm_stream_flush(st.h)
            assert ready >= 0, hip.lib.sdrhip_last_error()
            pos += n
            if how == "pop":
                for _ in range(ready):
                    o = np.empty(2048, np.float32)
                    assert hip.lib.sdrhip_fm_stream_pop(st.h, o.ctypes.data_as(C.POINTER(C.c_float)), 2048) == 2048
                    got.append(o)
            else:
                blocks = st.pop_rows(ready + 2)
                assert blocks.shape == (1, ready, 2048)
                got += list(blocks[0])
        outs[how] = np.concatenate(got)
    assert outs["pop"].size == FB._bank(hip, [name]).ready(nblk * B) // 2048 * 2048
    assert_bit_equal(outs["pop"], outs["pop_rows"], "pop vs pop_rows")
    _check(hip, [name], outs["pop"][None, :], nblk * B, "one station through pop")


# ---- the example -------------------------------------------------------------------------------------------------------------------
def test_fm_replay_s16(tmp_path, hip):
    """fm_replay --s16 with two stations against the binding's stream on the same capture."""
    import test_gpu_examples as E
    E._ensure_exe()
    nblk = 60
    names = ["shift 1/4", "shift -3/1000"]
    cap = tmp_path / "capture.s16"
    FC.stream(nblk).tofile(cap)
    S.taps_decim127().tofile(str(cap) + ".decim.f32")
    S.taps_resamp191().tofile(str(cap) + ".resamp.f32")
    S.taps_audio_half64().tofile(str(cap) + ".audio_half.f32")
    out = tmp_path / "audio.f32"
    r = subprocess.run([E.EXE, "--s16", "--stations", "1/4,-3/1000", str(cap), str(out), "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(out), "with --stations the audio goes to <file>.<station>"
    st = hip.FmStream(FB._bank(hip, names), 4 * B, B, input_i16=True)
    rows = _rows(_push_all(st, FC.stream(nblk), [4] * (nblk // 4)) + st.flush(), 2)
    assert rows.shape[1] >= B
    for j in range(2):
        got = np.fromfile(f"{out}.{j}", np.float32)
        assert got.size >= rows.shape[1] and got.size % B == 0
        FB.same_bits(got[:rows.shape[1]], rows[j], f"fm_replay --s16, station {j}")
    _check(hip, names, rows, nblk * B, "the binding's stream")
    # one {1, 0} station when no station is given
    r = subprocess.run([E.EXE, "--s16", str(cap), str(out), "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    got = np.fromfile(out, np.float32)
    _check(hip, ["identity"], got[None, :B], nblk * B, "fm_replay --s16 without stations")
