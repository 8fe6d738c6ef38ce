"""GPU parity of a bank's host-block stream (sdrhip_fm_stream_create_bank): host blocks in, every station's audio blocks out.
The definition is the whole specification: station j's blocks are, bit for bit, those of an FmStream over a tuned chain of the
bank's arguments with table j, fed the same samples -- whatever the push sizes, coalescing, adaptive submission or route.  Expected
values are never taken from a bank's stream: they are the tuned chains' own runs over the whole device buffer
(test_gpu_fm_bank.chain_ref) cut into blocks, FmStreams over tuned chains, or the restated Pipes (test_gpu_tuned_chain.model).
Chain arguments, tables and the input stream are those of tests/test_gpu_tuned_chain.py / tests/test_gpu_fm_bank.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import signals as S
import test_gpu_fm_bank as FB
import test_gpu_tuned_chain as T
from conftest import assert_bit_equal
from gpu_util import to_dev

pytestmark = pytest.mark.gpu

B = T.B
ERR_ARG = -1
RAGGED = [1, 3, 2, 16, 5, 1, 1, 7, 16, 4, 2, 1, 9, 16, 12]
_cache = {}


def _small(hip):
    return hip.lib.sdrhip_debug_small_chain_launches()


def _rows(got, K, block_out=B):
    """The list a bank stream's calls return -> [K, blocks * block_out]"""
    for g in got:
        assert g.shape == (K, block_out) and g.dtype == np.float32
    return np.concatenate(got, axis=1) if got else np.zeros((K, 0), np.float32)


def _check(hip, names, rows, d_in, total, what, block=B, **kw):
    """Every station's audio against its tuned chain's run over the whole buffer (the refs are computed once per table and run)."""
    q1 = FB._bank(hip, names[:1], block).ready(total)
    for j, name in enumerate(names):
        ref = FB.chain_ref(hip, name, d_in, 0, total, 0, q1, block=block, **kw)
        assert rows.shape[1] <= ref.size
        assert_bit_equal(rows[j], ref[:rows.shape[1]], f"{what}: station {j} ({name}) vs its tuned chain")


def _submissions_with_output(bank, sizes, unit=B):
    n, count = 0, 0
    for s in sizes:
        count += bank.ready((n + s) * unit) > bank.ready(n * unit)
        n += s
    return count


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blocks_per_push", [1, 3, 16])
@pytest.mark.parametrize("K", [1, 2, 3, 32])
def test_definition(hip, K, blocks_per_push):
    """96 source blocks, audio blocks of 8192.  Every push is a submission here (adaptive submission off), so the banked launches
    can be counted: one per submission that completes an output, and none of the chains' own kernels."""
    names = {1: ["shift 1/65536"], 2: ["shift 1/4", "shift -3/1000"], 3: ["shift -3/1000", "shift 5/8313", "shift -3/1000"],
             32: [FB.NAMES[j % len(FB.NAMES)] for j in range(32)]}[K]
    nblk = 96
    u8 = T.stream_u8(nblk)
    bank = FB._bank(hip, names)
    st = hip.FmStream(bank, blocks_per_push * B, B)
    assert st.rows() == K
    st.set_adaptive(0)
    sizes = [blocks_per_push] * (nblk // blocks_per_push)
    b0, c0 = hip.fm_bank_launches(), _small(hip)
    got = T._push_all(st, u8, sizes) + st.flush()
    assert hip.fm_bank_launches() - b0 == _submissions_with_output(bank, sizes) == len(sizes)
    assert _small(hip) == c0, "a bank's stream launched a chain's kernel"
    rows = _rows(got, K)
    assert rows.shape[1] == bank.ready(nblk * B) // B * B == 3 * B
    _check(hip, names, rows, T.stream_dev(), nblk * B, f"{K} stations, {blocks_per_push} blocks per push")
    if K == 3:
        assert not np.array_equal(rows[0], rows[1]), "two stations with different tables gave the same audio"


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
def test_against_the_restated_pipes(hip, oracle):
    names = ["shift 1/4", "shift -3/1000"]
    nblk = 96
    st = hip.FmStream(FB._bank(hip, names), 4 * B, B)
    rows = _rows(T._push_all(st, T.stream_u8(nblk), [4] * (nblk // 4)) + st.flush(), 2)
    for j, name in enumerate(names):
        exp = T.model(oracle, name)
        assert exp.size == 2 * B <= rows.shape[1]
        assert_bit_equal(rows[j][:exp.size], exp, f"station {j} ({name}) vs the restated Pipes")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setting", [None, ("coalesce", 7), ("adaptive", 32)], ids=["plain", "coalesce 7", "adaptive 32"])
def test_ragged_pushes(hip, setting):
    names = ["shift 1/4", "random, period 5", "shift -3/1000"]
    nblk = 96
    assert sum(RAGGED) == nblk
    st = hip.FmStream(FB._bank(hip, names), 16 * B, B)
    if setting:
        getattr(st, "set_" + setting[0])(setting[1] * B)
    rows = _rows(T._push_all(st, T.stream_u8(nblk), RAGGED, inplace_every=3) + st.flush(), 3)
    assert rows.shape[1] == 3 * B
    _check(hip, names, rows, T.stream_dev(), nblk * B, f"ragged pushes ({setting})")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_pushes_that_complete_no_output(hip):
    """Seam block 1024, pushes of 1024 samples: the first three complete no output (no launch, nothing to pop), the fourth
    completes 3.  Audio blocks of 64 floats."""
    names = ["shift -3/1000", "shift 1/4"]
    unit, npush, block_out = 1024, 40, 64
    bank = FB._bank(hip, names, unit)
    assert [bank.ready(k * unit) for k in range(1, 5)] == [0, 0, 0, 3]
    u8 = T.stream_u8(5)
    st = hip.FmStream(bank, unit, block_out)
    st.set_adaptive(0)
    assert hip.lib.sdrhip_fm_stream_flush(st.h) == 0 and st.flush() == [], "flush of an empty stream"
    b0, c0 = hip.fm_bank_launches(), _small(hip)
    got = []
    for k in range(3):
        got += st.push(u8[2 * k * unit:2 * (k + 1) * unit])
    got += st.poll()
    assert got == [] and hip.fm_bank_launches() == b0 and _small(hip) == c0, "a push that completes no output launched something"
    for k in range(3, npush):
        got += st.push(u8[2 * k * unit:2 * (k + 1) * unit])
    got += st.flush()
    assert hip.fm_bank_launches() - b0 == _submissions_with_output(bank, [1] * npush, unit) == npush - 3
    rows = _rows(got, 2, block_out)
    assert rows.shape[1] == bank.ready(npush * unit) // block_out * block_out > 20 * block_out
    _check(hip, names, rows, T.stream_dev(), npush * unit, "1024-sample pushes", block=unit)


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def _long_stream():
    """600 source blocks: the module's 300-block stream twice over (uploaded once)."""
    if "u8" not in _cache:
        u8 = np.concatenate([T.stream_u8(300), T.stream_u8(300)])
        _cache["dev"] = to_dev(u8)
        u8.setflags(write=False)
        _cache["u8"] = u8
    return _cache["u8"], _cache["dev"]


LONG_SIZES = [1, 208, 3, 208, 16, 1, 163]


def test_past_the_banked_rectangle_and_the_direct_bound(hip):
    """max_block of 208 source blocks is past the direct bound: two slots, and the 208-block pushes go through the copy engines.
    They are also longer than 39322 outputs per station, so the bank runs them (and the 163-block push) station by station, on
    the stations' own one-kernel chains; the small pushes between them are one copy and one banked launch each."""
    names = ["shift -3/1000", "shift 1/4"]
    nblk = sum(LONG_SIZES)
    assert nblk == 600
    u8, d = _long_stream()
    bank = FB._bank(hip, names)
    long_pushes = [s for s in LONG_SIZES if bank.ready(s * B) > 39322]
    assert long_pushes == [208, 208, 163]
    st = hip.FmStream(bank, 208 * B, B)
    b0, c0 = hip.fm_bank_launches(), _small(hip)
    rows = _rows(T._push_all(st, u8, LONG_SIZES, inplace_every=3) + st.flush(), 2)
    assert hip.fm_bank_launches() - b0 == len(LONG_SIZES) - len(long_pushes), "the small pushes go banked, the long ones do not"
    assert _small(hip) - c0 == 2 * len(long_pushes), "a long push is one run of each station's own chain"
    assert rows.shape[1] == bank.ready(nblk * B) // B * B == 22 * B
    _check(hip, names, rows, d, nblk * B, "600 blocks over two routes", key="600 blocks")


def test_route_switch_on_a_chain_stream(hip):
    """The same sizes on an FmStream over a tuned chain: in place, slot-stream copy and copy engines in one stream."""
    name = "shift -3/1000"
    u8, d = _long_stream()
    st = hip.FmStream(FB._chain(hip, name), 208 * B, B)
    assert st.rows() == 1
    got = T._push_all(st, u8, LONG_SIZES, inplace_every=3) + st.flush()
    assert all(g.shape == (B,) for g in got)
    _check(hip, [name], np.concatenate(got)[None, :], d, 600 * B, "chain stream, 600 blocks over three routes", key="600 blocks")
    assert len(got) == 22


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_forced_routes(hip):
    names = ["shift 5/8313", "shift 1/4", "identity"]
    nblk = 56
    bank = FB._bank(hip, names)
    bank.set_route(2)
    st = hip.FmStream(bank, 16 * B, 2048)
    b0, c0 = hip.fm_bank_launches(), _small(hip)
    rows = _rows(T._push_all(st, T.stream_u8(nblk), RAGGED[:10], inplace_every=3) + st.flush(), 3, 2048)
    assert sum(RAGGED[:10]) == nblk and hip.fm_bank_launches() == b0 and _small(hip) > c0
    assert rows.shape[1] == bank.ready(nblk * B) // 2048 * 2048
    _check(hip, names, rows, T.stream_dev(), nblk * B, "route 2 under the stream")
    # route 1 where the banked launch does not fit (a seam block below the one-kernel chain's range): the push fails
    unit = 160
    bank = FB._bank(hip, names[:2], unit)
    bank.set_route(1)
    st = hip.FmStream(bank, 64 * unit, 256)
    with pytest.raises(hip.SdrHipError):
        st.push(T.stream_u8(2)[:2 * 64 * unit])
    assert b"sdrhip_fm_bank_run" in hip.lib.sdrhip_last_error()
    assert hip.fm_bank_launches() == b0
    assert st.pop_rows(4).shape == (2, 0, 256), "a refused push left audio to pop"
    del st                                                     # still destroyable


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_save_and_restore(hip):
    names = ["shift -3/1000", "shift 1/4", "random, period 5"]
    nblk, block_out = 40, 2048
    u8 = T.stream_u8(nblk)
    first = hip.FmStream(FB._bank(hip, names), 8 * B, block_out)
    got = T._push_all(first, u8, [1] * 5)
    state = first.save()                                       # (binds state_bytes / save / restore on first use)
    assert hip.lib.sdrhip_fm_stream_state_bytes(first.h) == len(state), "state_bytes is what save used"
    # the header's fields: magic, version, then N, q_done, head_cap, hist_n, pending (int64 each), ...: 64 bytes; a state of
    # several rows carries the row count behind it, then the history (2 bytes a sample) and every row's audio not yet popped
    version, = np.frombuffer(state, np.uint32, 1, 4)
    n_seen, q_done, _, hist_n, pending = (int(v) for v in np.frombuffer(state, np.int64, 5, 8))
    assert version == 2 and np.frombuffer(state, np.int64, 1, 64)[0] == 3, "a multi-row state has its own version and carries the row count"
    assert n_seen == 5 * B and q_done == first.chain.ready(5 * B)
    assert pending + sum(g.shape[1] for g in got) == q_done and 0 < pending % block_out < block_out, "every station has a remainder in the state"
    assert len(state) == 64 + 8 + 2 * hist_n + 3 * 4 * pending
    chain_st = hip.FmStream(FB._chain(hip, names[0]), 8 * B, block_out)
    T._push_all(chain_st, u8, [1] * 5)
    chain_state = chain_st.save()
    assert np.frombuffer(chain_state, np.uint32, 1, 4)[0] == 1, "a one-row state keeps its version"
    del first
    second = hip.FmStream(FB._bank(hip, names), 8 * B, block_out)
    got += second.restore(state)
    got += T._push_all(second, u8[2 * 5 * B:], [1] * (nblk - 5)) + second.flush()
    rows = _rows(got, 3, block_out)
    assert rows.shape[1] == second.chain.ready(nblk * B) // block_out * block_out
    _check(hip, names, rows, T.stream_dev(), nblk * B, "saved after 5 of 40 pushes, restored over a second bank")

    # refusals: another station count, a chain's stream, another block_out, a truncated state -- and the refusing stream works on
    def refuses(st, blob, what):
        rc = hip.lib.sdrhip_fm_stream_restore(st.h, blob, len(blob))
        assert rc == ERR_ARG and b"sdrhip_fm_stream_restore" in hip.lib.sdrhip_last_error(), what

    two = hip.FmStream(FB._bank(hip, names[:2]), 8 * B, block_out)
    refuses(two, state, "a 3-station state into a 2-station stream")
    one = hip.FmStream(FB._chain(hip, names[0]), 8 * B, block_out)
    refuses(one, state, "a 3-station state into a chain's stream")
    other = hip.FmStream(FB._bank(hip, names), 8 * B, 4096)
    refuses(other, state, "another block_out")
    three = hip.FmStream(FB._bank(hip, names), 8 * B, block_out)
    refuses(three, state[:-4], "a truncated state")
    refuses(three, state[:68], "a state cut inside its row count")
    refuses(three, chain_state, "a chain stream's state into a 3-station stream")
    got1 = T._push_all(one, u8, [2] * 10) + one.flush()
    _check(hip, names[:1], np.concatenate(got1)[None, :], T.stream_dev(), 20 * B, "a chain's stream that refused a state")
    for st, nm in ((two, names[:2]), (three, names)):
        rows = _rows(T._push_all(st, u8, [2] * 10) + st.flush(), len(nm), block_out)
        _check(hip, nm, rows, T.stream_dev(), 20 * B, "a stream that refused a state")
    # ... and takes the state it was refused a truncated copy of
    four = hip.FmStream(FB._bank(hip, names), 8 * B, block_out)
    refuses(four, state[:-4], "a truncated state")
    assert len(four.restore(state)) == 0


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def _raw_push(hip, st, chunk):
    chunk = np.ascontiguousarray(chunk)
    rc = hip.lib.sdrhip_fm_stream_push(st.h, chunk.ctypes.data_as(C.POINTER(C.c_uint8)), chunk.size // 2)
    assert rc >= 0, hip.lib.sdrhip_last_error()
    return rc


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_one_row(hip):
    """A bank of one station is a one-row stream: sdrhip_fm_stream_pop serves it, and it equals the FmStream over the tuned chain."""
    name = "shift -3/1000"
    nblk = 56
    u8 = T.stream_u8(nblk)
    ref = hip.FmStream(FB._chain(hip, name), 16 * B, 2048)
    exp = T._push_all(ref, u8, RAGGED[:10]) + ref.flush()
    assert len(exp) == ref.chain.ready(nblk * B) // 2048
    for how in ("pop", "pop_rows"):
        st = hip.FmStream(FB._bank(hip, [name]), 16 * B, 2048)
        assert st.rows() == 1
        got, pos = [], 0
        for n in RAGGED[:10] + [0]:                                # 0: the flush
            ready = _raw_push(hip, st, u8[2 * pos * B:2 * (pos + n) * B]) if n else hip.lib.sdrhip_fm_stream_flush(st.h)
            pos += n
            if how == "pop":
                for _ in range(ready):
                    o = np.empty(2048, np.float32)
                    assert hip.lib.sdrhip_fm_stream_pop(st.h, _fp(o), 2048) == 2048
                    got.append(o)
            else:
                blocks = st.pop_rows(ready + 2)
                assert blocks.shape == (1, ready, 2048)
                got += list(blocks[0])
        assert len(got) == len(exp)
        assert_bit_equal(np.concatenate(got), np.concatenate(exp), f"one-station bank stream through {how} vs the chain's FmStream")
    # pop_rows on a chain's stream: one row
    st = hip.FmStream(FB._chain(hip, name), 16 * B, 2048)
    for i in range(2):
        _raw_push(hip, st, u8[2 * 16 * B * i:2 * 16 * B * (i + 1)])
    ready = hip.lib.sdrhip_fm_stream_flush(st.h)
    assert 2 < ready <= len(exp)
    assert_bit_equal(st.pop_rows(ready)[0].reshape(-1), np.concatenate(exp[:ready]), "pop_rows on a chain's stream")

    three = hip.FmStream(FB._bank(hip, [name, "shift 1/4", name]), 16 * B, 2048)
    for i in range(2):
        _raw_push(hip, three, u8[2 * 16 * B * i:2 * 16 * B * (i + 1)])
    ready = hip.lib.sdrhip_fm_stream_flush(three.h)
    assert ready > 2
    o = np.full(3 * 2 * 2048, 7.0, np.float32)
    assert hip.lib.sdrhip_fm_stream_pop(three.h, _fp(o), o.size) == ERR_ARG and b"sdrhip_fm_stream_pop" in hip.lib.sdrhip_last_error()
    assert hip.lib.sdrhip_fm_stream_pop_rows(three.h, _fp(o), 2 * 2048 - 1, 2) == ERR_ARG, "row_stride too small for max_blocks"
    assert b"sdrhip_fm_stream_pop_rows" in hip.lib.sdrhip_last_error()
    assert (o == 7.0).all() and hip.lib.sdrhip_fm_stream_poll(three.h) == ready, "a refused pop wrote or popped something"
    rows = three.pop_rows(ready)
    assert rows.shape == (3, ready, 2048)
    for j in (0, 2):
        assert_bit_equal(rows[j].reshape(-1), np.concatenate(exp[:ready]), f"row {j} of three vs the chain's FmStream")
    assert not np.array_equal(rows[0], rows[1])


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def test_fm_replay_stations(tmp_path, oracle):
    import test_gpu_examples as E
    E._ensure_exe()
    nblk = 96
    cap = tmp_path / "capture.u8"
    T.stream_u8(nblk).tofile(cap)
    S.taps_decim127().tofile(str(cap) + ".decim.f32")
    S.taps_resamp191().tofile(str(cap) + ".resamp.f32")
    S.taps_audio_half64().tofile(str(cap) + ".audio_half.f32")
    out = tmp_path / "audio.f32"
    r = subprocess.run([E.EXE, "--stations", "1/4,-3/1000", str(cap), str(out), "4"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert not os.path.exists(out), "with --stations the audio goes to <file>.<station>"
    for j, name in enumerate(["shift 1/4", "shift -3/1000"]):
        got = np.fromfile(f"{out}.{j}", np.float32)
        exp = T.model(oracle, name)
        assert got.size >= exp.size == 2 * B and got.size % B == 0
        assert_bit_equal(got[:exp.size], exp, f"fm_replay --stations, station {j} ({name})")
    r = subprocess.run([E.EXE, "--stations", "1/4,,3/8", str(cap), str(out)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--stations" in r.stderr
