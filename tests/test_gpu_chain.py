"""GPU parity: the whole FM receiver (examples/fm/fm.hs:34-41) as one device-resident
chain vs the restated Pipes, single launch and sharded with a right halo."""
import struct

import numpy as np
import pytest

from conftest import assert_bit_equal
from oracle import pipes_model as PM
import signals as S
from gpu_util import to_dev, dev_empty_f32, ptr, to_host
import torch

pytestmark = pytest.mark.gpu

# SDRHIP_SWEEP_SCALE=20 turns the seeded random sweeps into a soak test (more trials, same seeds first)
SWEEP_SCALE = max(1, int(__import__("os").environ.get("SDRHIP_SWEEP_SCALE", "1")))
SWEEP_SEED = int(__import__("os").environ.get("SDRHIP_SWEEP_SEED", "0"))        # other seeds for soak runs

B = 8192


def _chain(hip, gain=0.2, block=B, order=None):
    return hip.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), gain, block,
                       hip.ORDER_AVX if order is None else order)


def _model(oracle, u8, nblk, gain=0.2, block=B, order=PM.ORDER_AVX):
    blocks = [u8[2 * i * block:2 * (i + 1) * block] for i in range(nblk)]
    out = PM.fm_receiver(oracle, blocks, S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(),
                         gain, block, order)
    return np.concatenate(out) if out else np.zeros(0, np.float32)


def _run(hip, chain, u8_dev, s0, n_in, q0, q1):
    ws_bytes = chain.workspace_bytes(n_in)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = dev_empty_f32(q1 - q0)
    chain.run(ptr(u8_dev), s0, n_in, ptr(out), q0, q1, ptr(ws), ws_bytes)
    return to_host(out)


@pytest.mark.parametrize("fm_signal", [False, True])
def test_chain_matches_pipes(hip, oracle, fm_signal):
    # every Pipe only yields full 8192-blocks: 90 input blocks -> 11 decimator blocks -> 3 resampler blocks -> 2 audio blocks
    nblk = 90
    u8 = (S.iq_u8_fm if fm_signal else S.iq_u8)(nblk * B)
    exp = _model(oracle, u8, nblk)
    assert exp.size == 2 * B
    chain = _chain(hip)
    total = nblk * B
    q0, q1, halo = chain.plan(0, total, total)
    assert q0 == 0 and halo == 0 and q1 >= exp.size
    got = _run(hip, chain, to_dev(u8), 0, total, 0, q1)
    assert_bit_equal(got[: exp.size], exp, "chain vs pipes")


def test_chain_sharded_equals_single(hip, oracle):
    """Shards + right halo (what each GPU does after the halo exchange) reproduce the single stream."""
    nblk = 40
    total = nblk * B
    u8 = S.iq_u8(total)
    chain = _chain(hip)
    Q0, Q1, _ = chain.plan(0, total, total)
    full = _run(hip, chain, to_dev(u8), 0, total, Q0, Q1)
    max_halo = chain.max_halo()
    assert 0 < max_halo < 8192
    for nshards in (2, 4, 5):
        S_len = total // nshards // 8 * 8
        pieces = []
        for r in range(nshards):
            s0 = r * S_len
            s1 = total if r == nshards - 1 else (r + 1) * S_len
            q0, q1, halo = chain.plan(s0, s1, total)
            assert halo <= max_halo
            n_in = min(total, s1 + halo) - s0
            shard = to_dev(u8[2 * s0: 2 * (s0 + n_in)])
            pieces.append((q0, q1, _run(hip, chain, shard, s0, n_in, q0, q1)))
        assert pieces[0][0] == Q0 and pieces[-1][1] == Q1
        for (a0, a1, _), (b0, b1, _) in zip(pieces[:-1], pieces[1:]):
            assert a1 == b0
        got = np.concatenate([p[2] for p in pieces])
        assert_bit_equal(got, full, f"{nshards} shards")


def test_chain_contiguous_and_orders(hip, oracle):
    """block = 0 (no seams) and the SSE order."""
    total = 30 * B
    u8 = S.iq_u8(total)
    # SSE order with seams vs the model
    exp = _model(oracle, u8, 30, gain=None, order=PM.ORDER_SSE)
    chain = _chain(hip, gain=1.0, order=hip.ORDER_SSE)
    q0, q1, _ = chain.plan(0, total, total)
    got = _run(hip, chain, to_dev(u8), 0, total, q0, q1)
    assert_bit_equal(got[: exp.size], exp, "SSE chain")
    # contiguous: equals the stage-by-stage C kernels on whole buffers
    chain0 = _chain(hip, gain=1.0, block=0)
    q0, q1, _ = chain0.plan(0, total, total)
    got = _run(hip, chain0, to_dev(u8), 0, total, q0, q1)
    x = oracle.convert_u8(u8)
    h = np.concatenate([S.taps_decim127(), np.zeros(1, np.float32)])
    K = (total - 128) // 8 + 1
    d = oracle.decimate_rc(4, K, 8, np.repeat(h, 2), x)
    y = oracle.fm_demod(d)
    prep = oracle.prepare_coeffs(8, 3, 10, S.taps_resamp191())
    M = (K * 3 - 192) // 10 + 1
    z, _ = oracle.resample_rr(8, M, prep, 0, y)
    a = oracle.filter_sym_rr(8, M - 127, S.taps_audio_half64(), z)
    assert q1 == a.size
    assert_bit_equal(got, a, "contiguous chain")


def test_chain_rejects_missing_halo(hip):
    chain = _chain(hip)
    total = 20 * B
    u8 = to_dev(S.iq_u8(total))
    q0, q1, halo = chain.plan(0, total // 2, total)
    assert halo > 0
    ws = torch.empty(chain.workspace_bytes(total), dtype=torch.uint8, device="cuda")
    out = dev_empty_f32(q1 - q0)
    with pytest.raises(hip.SdrHipError):
        chain.run(ptr(u8), 0, total // 2, ptr(out), q0, q1, ptr(ws), ws.numel())  # halo not provided


@pytest.mark.parametrize("blocks_per_push", [1, 3, 16])
def test_fm_stream_matches_pipes(hip, oracle, blocks_per_push):
    """Host-block streaming front end (pinned, double-buffered, three streams): source blocks in, the
    reference's audio blocks out, however many source blocks one push carries."""
    nblk = 96
    u8 = S.iq_u8_fm(nblk * B)
    exp = _model(oracle, u8, nblk)
    assert exp.size == 2 * B
    chain = _chain(hip)
    st = hip.FmStream(chain, blocks_per_push * B, B)
    got = []
    for i in range(0, nblk, blocks_per_push):
        got += st.push(u8[2 * i * B: 2 * (i + blocks_per_push) * B])
    got += st.flush()
    # the stream yields an audio block as soon as its receptive field is complete, i.e. sometimes a push earlier than the
    # four chained Pipes (each of which waits for a full 8192-block of ITS input); the sequence of blocks is the same
    assert len(got) >= 2
    assert_bit_equal(np.concatenate(got[:2]), exp, "fm stream vs pipes")
    with pytest.raises(hip.SdrHipError):
        st.push(u8[: 2 * (B - 8)])          # not a whole source block: the seams would be somewhere else


def test_fm_stream_large_copying_pushes_equal_small_ones(hip):
    """Round 5: a push of 4 MiB or more (chain.cpp: CopyPool::kMinBytes) from caller memory is copied into the pinned staging buffer by the caller and three helper
    threads (chain.cpp: CopyPool); the audio must be what 16-block pushes give -- including a push whose length is not a multiple of
    the helpers' 1 MiB pieces, from an unaligned address, and a last short one."""
    nblk = 1536 + 700 + 37
    raw = np.empty(2 * nblk * B + 3, np.uint8)
    u8 = raw[3:]                                   # unaligned caller memory
    u8[:] = S.iq_u8(nblk * B)
    chain = _chain(hip)
    ref_st = hip.FmStream(chain, 16 * B, B)
    ref = []
    for i in range(0, nblk, 16):
        ref += ref_st.push(u8[2 * i * B: 2 * min(nblk, i + 16) * B])
    ref += ref_st.flush()
    st = hip.FmStream(chain, 1536 * B, B)
    got = []
    at = 0
    for n in (1536, 700, 37):                      # 24 MiB, 10.9 MiB (pieces do not divide it), 0.6 MiB (plain memcpy)
        got += st.push(u8[2 * at * B: 2 * (at + n) * B])
        at += n
    got += st.flush()
    assert len(got) == len(ref) and len(got) > 60
    assert_bit_equal(np.concatenate(got), np.concatenate(ref), "large copying pushes vs 16-block pushes")


def test_fm_stream_long_run_equals_chain(hip, oracle):
    """Many pushes: the streamed audio equals one device-resident chain run over the same samples."""
    nblk = 512
    total = nblk * B
    u8 = S.iq_u8(total)
    chain = _chain(hip)
    _, q1, _ = chain.plan(0, total, total)
    chain.set_small_chain(0)                    # the resident run on the STAGE kernels: 512 blocks are inside the one-kernel chain's
    full = _run(hip, chain, to_dev(u8), 0, total, 0, q1)   # automatic range since round 5, and the pushes below take it on their own
    chain.set_small_chain(2)
    st = hip.FmStream(chain, 8 * B, B)
    got = []
    for i in range(0, nblk, 8):
        if i % 16:
            got += st.push(u8[2 * i * B: 2 * (i + 8) * B])
        else:                                   # zero-copy: fill the pinned staging buffer in place
            view = st.input_buffer(8 * B)
            view[:] = u8[2 * i * B: 2 * (i + 8) * B]
            got += st.push_inplace(view)
    got += st.flush()
    got = np.concatenate(got)
    assert got.size == q1 // B * B
    assert_bit_equal(got, full[: got.size], "streamed vs resident")


def test_chain_split_at_ready(hip, oracle):
    """Overlapping the halo exchange: a shard's outputs [q0, ready(s1)) need only its own samples (computed here from a
    buffer whose halo region is still garbage), the rest run once the halo is in; together they equal the unsplit run."""
    nblk = 48
    total = nblk * B
    u8 = S.iq_u8(total)
    chain = _chain(hip)
    S_len = total // 3 // 8 * 8
    halo_cap = (chain.max_halo() + 7) // 8 * 8
    for r in range(2):
        s0, s1 = r * S_len, (r + 1) * S_len
        q0, q1, halo = chain.plan(s0, s1, -1)
        q_mid = max(q0, min(q1, chain.ready(s1)))
        assert q0 < q_mid < q1 and q1 - q_mid < 400
        assert chain.plan(s0, s1, -1)[2] > 0 and chain.plan(s0, s1 - 0, -1)[0] == q0
        n_in = S_len + halo_cap
        ref = _run(hip, chain, to_dev(u8[2 * s0: 2 * (s0 + n_in)]), s0, n_in, q0, q1)
        poisoned = u8[2 * s0: 2 * (s0 + n_in)].copy()
        poisoned[2 * S_len:] = 255                                  # the halo has not arrived yet
        part_a = _run(hip, chain, to_dev(poisoned), s0, n_in, q0, q_mid)
        part_b = _run(hip, chain, to_dev(u8[2 * s0: 2 * (s0 + n_in)]), s0, n_in, q_mid, q1)
        assert_bit_equal(np.concatenate([part_a, part_b]), ref, f"shard {r}")
    # ready() is the inverse of the receptive-field end
    for n in (0, 100, 5000, 8192, 123456):
        k = chain.ready(n)
        if k > 0:
            assert chain.plan(0, n, -1)[1] >= 0
        q0, q1, h = chain.plan(0, max(n, 1), -1)
        assert k <= q1


@pytest.mark.parametrize("coalesce_blocks", [4, 16])
def test_fm_stream_coalesce(hip, oracle, coalesce_blocks):
    """Coalescing 8192-sample pushes inside the operator changes when the audio appears, not what it is."""
    nblk = 100
    u8 = S.iq_u8_fm(nblk * B)
    exp = _model(oracle, u8, nblk)
    chain = _chain(hip)
    st = hip.FmStream(chain, B, B)
    st.set_coalesce(coalesce_blocks * B)
    got = []
    for i in range(nblk):
        if i % 3 == 0:
            view = st.input_buffer(B)
            view[:] = u8[2 * i * B: 2 * (i + 1) * B]
            got += st.push_inplace(view)
        else:
            got += st.push(u8[2 * i * B: 2 * (i + 1) * B])
    got += st.flush()
    got = np.concatenate(got)
    assert got.size >= exp.size
    assert_bit_equal(got[: exp.size], exp, "coalesced stream")
    with pytest.raises(hip.SdrHipError):
        st.push(u8[: 2 * B])
        st.set_coalesce(2 * B)                     # samples staged: refuse


@pytest.mark.parametrize("cap_blocks", [2, 8, 32])
def test_fm_stream_adaptive(hip, oracle, cap_blocks):
    """Adaptive submission (pushes are staged while the slot ahead is still running and leave as one launch when it frees up):
    how the pushes are grouped depends on timing, the audio does not -- fast pushes, pushes with pauses, lent buffers."""
    import time
    nblk = 300
    u8 = S.iq_u8_fm(nblk * B)
    exp = _model(oracle, u8, nblk)
    chain = _chain(hip)
    st = hip.FmStream(chain, B, B)
    st.set_adaptive(cap_blocks * B)
    got = []
    for i in range(nblk):
        if i % 3 == 0:
            view = st.input_buffer(B)
            view[:] = u8[2 * i * B: 2 * (i + 1) * B]
            got += st.push_inplace(view)
        else:
            got += st.push(u8[2 * i * B: 2 * (i + 1) * B])
        if i % 50 == 49:
            time.sleep(0.002)                      # the GPU catches up: the next pushes go out one by one again
    got += st.flush()
    got = np.concatenate(got)
    assert got.size >= exp.size
    assert_bit_equal(got[: exp.size], exp, "adaptive stream")
    st.set_adaptive(0)
    with pytest.raises(hip.SdrHipError):
        st.set_adaptive(B)                         # less than two pushes
    with pytest.raises(hip.SdrHipError):
        st.push(u8[: 2 * B])
        st.flush()
        st.push(u8[: 2 * B])
        st.set_adaptive(4 * B)                     # samples may be staged / in flight: only refused while staged
        st.set_coalesce(4 * B)
        st.push(u8[: 2 * B])
        st.set_adaptive(4 * B)                     # staged now: refuse


def test_fm_stream_poll_delivers_a_push_without_another_push(hip, oracle):
    """A real-time caller: push one source block, poll a little later -- the audio that push completed is there, no further
    push and no flush needed (sdrhip_fm_stream_poll); the block sequence is the resident run's."""
    import time
    nblk = 100
    u8 = S.iq_u8_fm(nblk * B)
    exp = _model(oracle, u8, nblk)
    chain = _chain(hip)
    st = hip.FmStream(chain, B, 512)
    got, late = [], 0
    for i in range(nblk):
        got += st.push(u8[2 * i * B: 2 * (i + 1) * B])
        have = sum(len(b) for b in got)
        # the audio outputs whose last input sample has arrived: chain.ready(N)
        want = (chain.ready((i + 1) * B) // 512) * 512
        deadline = time.time() + 2.0
        while have < want and time.time() < deadline:
            got += st.poll()
            have = sum(len(b) for b in got)
        late += have < want
    assert late == 0, "poll did not deliver the audio of a finished push"
    got += st.flush()
    got = np.concatenate(got)
    m = min(got.size, exp.size)
    assert exp.size >= 16384 and m == exp.size
    assert_bit_equal(got[:m], exp[:m], "polled stream")


def test_chain_random_sweep(hip, oracle):
    """Seeded random receivers (decimation, tap counts, resampling ratio, gain, source block size, SIMD order): the
    device-resident chain in one launch, the same chain sharded in three, and the host-block stream operator all give the
    audio of the restated reference pipeline."""
    rng = np.random.default_rng(4242 + SWEEP_SEED)
    ran = 0
    for trial in range(24 * SWEEP_SCALE):
        order = [PM.ORDER_AVX, PM.ORDER_SSE][rng.integers(0, 2)]
        simd = 8 if order == PM.ORDER_AVX else 4
        block = int(rng.choice([2048, 4096, 8192]))
        factor = int(rng.integers(2, 17))
        n_decim = int(rng.integers(factor + 4, 200))
        while True:
            I, D = int(rng.integers(1, 6)), int(rng.integers(2, 16))
            if D > I and np.gcd(I, D) == 1:
                break
        n_resamp = int(rng.integers(max(D, 2 * I), 40 * I + D))
        n_half = simd * int(rng.integers(1, 12))
        gain = float(np.float32(rng.uniform(0.05, 3.0)))
        decim_taps, resamp_taps, half = S.gauss_taps(n_decim, 1000 + trial), S.gauss_taps(n_resamp, 2000 + trial), S.gauss_taps(n_half, 3000 + trial, 0.2)
        # enough source blocks for a few audio blocks
        per_audio = block * factor * D / I
        nblk = int(3.3 * per_audio / block) + 4
        if nblk * block > 6_000_000:
            continue
        u8 = S.iq_u8(nblk * block, seed=5000 + trial)
        blocks = [u8[2 * i * block: 2 * (i + 1) * block] for i in range(nblk)]
        try:
            exp = PM.fm_receiver(oracle, blocks, decim_taps, factor, resamp_taps, I, D, half, gain, block, order)
        except PM.PipeAssert:
            continue
        if not exp:
            continue
        exp = np.concatenate(exp)
        label = f"trial {trial}: /{factor} {n_decim} taps, {I}/{D} {n_resamp} taps, {n_half} half taps, block {block}, order {order}"
        chain = hip.FmChain(factor, decim_taps, I, D, resamp_taps, half, gain, block, order)
        total = nblk * block
        q0, q1, halo = chain.plan(0, total, total)
        assert q0 == 0 and halo == 0 and q1 >= exp.size, label
        d_u8 = to_dev(u8)
        got = _run(hip, chain, d_u8, 0, total, 0, q1)
        assert_bit_equal(got[: exp.size], exp, label + " (one launch)")
        # three shards with right halos
        S_len = total // 3 // 8 * 8
        pieces = []
        for r in range(3):
            s0 = r * S_len
            s1 = total if r == 2 else (r + 1) * S_len
            a, b, h = chain.plan(s0, s1, total)
            n_in = min(total, s1 + h) - s0
            pieces.append(_run(hip, chain, to_dev(u8[2 * s0: 2 * (s0 + n_in)]), s0, n_in, a, b))
        assert_bit_equal(np.concatenate(pieces), got, label + " (3 shards)")
        # host-block stream operator: random push sizes (1-4 source blocks), random coalescing, zero-copy now and then
        st = hip.FmStream(chain, 4 * block, block)
        if rng.integers(0, 2):
            st.set_coalesce(int(rng.integers(1, 9)) * block)
        outs, i = [], 0
        while i < nblk:
            k = min(int(rng.integers(1, 5)), nblk - i)
            chunk = u8[2 * i * block: 2 * (i + k) * block]
            if rng.integers(0, 3) == 0:
                view = st.input_buffer(4 * block)[: chunk.size]
                view[:] = chunk
                outs += st.push_inplace(view)
            else:
                outs += st.push(chunk)
            i += k
        outs += st.flush()
        outs = np.concatenate(outs) if outs else np.zeros(0, np.float32)
        assert outs.size >= exp.size and outs.size % block == 0, label
        assert_bit_equal(outs[: exp.size], exp, label + " (stream)")
        ran += 1
    print(f"chain sweep: {ran} random receivers compared")
    assert ran >= 12


def test_fm_stream_coalesce_ragged_inplace(hip, oracle):
    """Zero-copy pushes of 1-3 source blocks with a coalescing target that is not a multiple of any of them: the staging
    buffer always has room for a whole push behind what is already staged."""
    nblk = 120
    u8 = S.iq_u8(nblk * B)
    exp = _model(oracle, u8, nblk)
    chain = _chain(hip)
    st = hip.FmStream(chain, 3 * B, B)
    st.set_coalesce(7 * B)
    got, i, k = [], 0, 0
    while i < nblk:
        n = min([1, 3, 2, 3][k % 4], nblk - i)
        k += 1
        view = st.input_buffer(3 * B)[: 2 * n * B]
        view[:] = u8[2 * i * B: 2 * (i + n) * B]
        got += st.push_inplace(view)
        i += n
    got += st.flush()
    got = np.concatenate(got)
    assert got.size >= exp.size
    assert_bit_equal(got[: exp.size], exp, "ragged coalesced zero-copy stream")


@pytest.mark.parametrize("block", [B, 0, 3 * B])
def test_fused_tail_equals_stage_kernels(hip, oracle, block):
    """kernels_tail.hip (fmDemod -> resampler -> filter in one kernel, Cross outputs decided in-kernel) against the three
    stage kernels + their seam fix-ups: whole runs, runs that start and end mid-tile, short runs inside one tile."""
    nblk = 70
    total = nblk * B
    u8 = S.iq_u8_fm(total)
    d = to_dev(u8)
    ch = _chain(hip, block=block)
    ch.set_small_chain(0)                      # this test is about the tail kernels: not the one-kernel chain
    q0, q1, _ = ch.plan(0, total, total)
    rng = np.random.default_rng(77 + SWEEP_SEED)
    ranges = [(0, q1), (0, 2046), (0, 2047), (1, 700), (2047, 2047 + 4093), (q1 - 5000, q1)]
    for _ in range(6 * SWEEP_SCALE):
        a = int(rng.integers(0, q1 - 10))
        ranges.append((a, int(min(q1, a + rng.integers(1, 9000)))))
    for a, b in ranges:
        ch.set_fused_tail(0)
        ref = _run(hip, ch, d, 0, total, a, b)
        ch.set_fused_tail(1)
        got = _run(hip, ch, d, 0, total, a, b)
        assert_bit_equal(got, ref, f"fused tail, block {block}, outputs [{a},{b})")
    if block == B:
        exp = _model(oracle, u8, nblk)
        ch.set_fused_tail(1)
        got = _run(hip, ch, d, 0, total, 0, q1)
        assert exp.size >= B
        assert_bit_equal(got[: exp.size], exp, "fused tail vs restated pipes")


@pytest.mark.parametrize("nblk", [300, 600, 900, 1100])
def test_small_chain_automatic_range_equals_stage_kernels(hip, nblk):
    """the one-kernel chain's automatic bound moved from ~256 to ~900 source blocks (chain.cpp: small-chain bound) -- every
    default run in between now takes kernels_small.hip.  The library's own choice (mode 2) against the stage kernels (mode 0), bit for
    bit, at sizes inside and just past the new range: seamed (8192-sample blocks) and unseamed, from the stream start and as a shard
    that starts inside the stream (s0 > 0, right halo only, a resampler phase that is not 0)."""
    total = nblk * B
    u8 = S.iq_u8(total + 8 * B)
    for block in (B, 0):
        ch = _chain(hip, block=block)
        for s0 in (0, 37 * B + 4096):
            n_in = total
            q0, q1, _ = ch.plan(s0, s0 + n_in, s0 + n_in)           # the stream ends where the resident samples end
            shard = to_dev(u8[2 * 0: 2 * n_in]) if s0 == 0 else to_dev(u8[2 * 4096: 2 * (4096 + n_in)])
            ch.set_small_chain(0)
            n0 = hip.lib.sdrhip_debug_small_chain_launches()
            ref = _run(hip, ch, shard, s0, n_in, q0, q1)
            assert hip.lib.sdrhip_debug_small_chain_launches() == n0, "mode 0 must never take the one-kernel chain"
            ch.set_small_chain(2)
            got = _run(hip, ch, shard, s0, n_in, q0, q1)
            took = hip.lib.sdrhip_debug_small_chain_launches() - n0
            assert took == (1 if nblk <= 800 else took), "runs of up to ~900 source blocks are the one-kernel chain's by default"
            assert_bit_equal(got, ref, f"automatic route vs stage kernels, {nblk} blocks, seam block {block}, s0 {s0} (one-kernel chain launches: {took})")


@pytest.mark.parametrize("block", [B, 0, 3 * B, 1000, 200])
def test_small_chain_equals_stage_kernels(hip, oracle, block):
    """kernels_small.hip (the WHOLE chain in one kernel: convert + decimator, fmDemod, resampler, filter, Cross outputs of
    every stage decided in-kernel) against the stage kernels + their seam fix-ups: whole runs, runs that start and end
    mid-tile, one-output runs, every tile size, shards that start inside the stream (s0 > 0, right halo only)."""
    nblk = 70
    total = nblk * B
    u8 = S.iq_u8_fm(total) if block != 1000 else S.iq_u8(total)
    d = to_dev(u8)
    ch = _chain(hip, block=block)
    q0, q1, _ = ch.plan(0, total, total)
    rng = np.random.default_rng(177 + SWEEP_SEED)
    ranges = [(0, q1), (0, 159), (0, 160), (1, 2), (2, 700), (158, 158 + 4093), (q1 - 5000, q1), (q1 - 1, q1)]
    for _ in range(6 * SWEEP_SCALE):
        a = int(rng.integers(0, q1 - 10))
        ranges.append((a, int(min(q1, a + rng.integers(1, 9000)))))
    tiles = [0, 159, 96, 48, 3]
    for i, (a, b) in enumerate(ranges):
        ch.set_small_chain(0)
        ref = _run(hip, ch, d, 0, total, a, b)
        n0 = hip.lib.sdrhip_debug_small_chain_launches()
        ch.set_small_chain(1, 0, tiles[i % len(tiles)])
        got = _run(hip, ch, d, 0, total, a, b)
        assert hip.lib.sdrhip_debug_small_chain_launches() == n0 + 1, "the one-kernel chain did not take the run"
        assert_bit_equal(got, ref, f"one-kernel chain, block {block}, tile {tiles[i % len(tiles)]}, outputs [{a},{b})")
    # shards: only [s0, s1 + halo) resident, global indices
    for nshards in (3, 7):
        S_len = total // nshards // 8 * 8
        for r in range(nshards):
            s0 = r * S_len
            s1 = total if r == nshards - 1 else (r + 1) * S_len
            a, b, halo = ch.plan(s0, s1, total)
            n_in = min(total, s1 + halo) - s0
            shard = to_dev(u8[2 * s0: 2 * (s0 + n_in)])
            ch.set_small_chain(0)
            ref = _run(hip, ch, shard, s0, n_in, a, b)
            ch.set_small_chain(1)
            got = _run(hip, ch, shard, s0, n_in, a, b)
            assert_bit_equal(got, ref, f"one-kernel chain, block {block}, shard {r} of {nshards}")
    if block == B:
        exp = _model(oracle, u8, nblk)
        ch.set_small_chain(1)
        got = _run(hip, ch, d, 0, total, 0, q1)
        assert exp.size >= B
        assert_bit_equal(got[: exp.size], exp, "one-kernel chain vs restated pipes")


def test_small_chain_on_eight_shards_of_2_to_the_20(hip, oracle):
    """BASELINE configs[4]'s geometry on one device: 8 shards of exactly 2^20 samples (+ right halo), each through the
    one-kernel chain (the route sdrhip_fm_chain_run takes by itself at this size), bit-equal to the single stream on the
    stage kernels -- and, over the first blocks, to the restated Pipes."""
    S_len, nshards = 1 << 20, 8
    chain = _chain(hip)
    chain.set_small_chain(2)                   # the default (auto) route, whatever the environment asks for
    halo_cap = chain.halo_samples()
    total = nshards * S_len + halo_cap
    u8 = S.iq_u8(total)
    d = to_dev(u8)
    ref_chain = _chain(hip)
    ref_chain.set_small_chain(0)
    Q0, _, _ = chain.plan(0, S_len, -1)
    _, Q1, _ = chain.plan((nshards - 1) * S_len, nshards * S_len, -1)
    full = _run(hip, ref_chain, d, 0, total, Q0, Q1)
    pieces = []
    for r in range(nshards):
        s0, s1 = r * S_len, (r + 1) * S_len
        a, b, halo = chain.plan(s0, s1, -1)
        assert halo <= halo_cap
        shard = to_dev(u8[2 * s0: 2 * (s1 + halo_cap)])
        n0 = hip.lib.sdrhip_debug_small_chain_launches()
        pieces.append((a, b, _run(hip, chain, shard, s0, S_len + halo_cap, a, b)))
        assert hip.lib.sdrhip_debug_small_chain_launches() == n0 + 1, "a 2^20-sample shard must take the one-kernel route by itself"
    assert pieces[0][0] == Q0 and pieces[-1][1] == Q1
    for (a0, a1, _), (b0, b1, _) in zip(pieces[:-1], pieces[1:]):
        assert a1 == b0
    assert_bit_equal(np.concatenate([p[2] for p in pieces]), full, "8 shards of 2^20 samples")
    nblk = 90
    exp = _model(oracle, u8[: 2 * nblk * B], nblk)
    assert_bit_equal(full[: exp.size], exp, "single stream vs restated pipes")


def _timed(chain, run):
    """run() with per-stage timing on -> (its result, stage -> ms, runs); a stage that did not run reads 0"""
    chain.enable_timing(True)
    try:
        out = run()
        torch.cuda.synchronize()
        stage_ms, runs = chain.read_timing()
    finally:
        chain.enable_timing(False)
    return out, stage_ms, runs


@pytest.mark.parametrize("block,forced", [(160, "small_chain"), (1000, "fused_tail")])
def test_forced_fused_route_that_does_not_fit_runs_the_stage_kernels_with_timing_on(hip, block, forced):
    """A fused kernel forced on (mode 1) on a chain it does not fit falls through to the next route, and the per-stage timing books
    what ran: nothing under the kernel that did not run, and the event pool is left fit for a second timed run.
    Seam block 160: below the one-kernel chain's 192, and below one tile of the fused tail, which auto mode asks for on the
    600-output range.  Seam block 1000: below the fused tail's 2046 + 4 + 128."""
    total = 16 * B
    d = to_dev(S.iq_u8_fm(total))
    ch = _chain(hip, block=block)
    for a, b in [(0, 600), (100, 2000)]:
        ch.set_small_chain(0)
        ch.set_fused_tail(0)
        ref = _run(hip, ch, d, 0, total, a, b)
        if forced == "small_chain":
            ch.set_small_chain(1)
            ch.set_fused_tail(2)
        else:
            ch.set_fused_tail(1)
        n0 = hip.lib.sdrhip_debug_small_chain_launches()
        for attempt in (1, 2):                                  # the second round: the first left the recorder consistent
            got, ms, runs = _timed(ch, lambda: _run(hip, ch, d, 0, total, a, b))
            what = f"forced {forced} on seam block {block}, outputs [{a},{b}), timed run {attempt}: {ms}"
            assert runs == 1, what
            assert ms["fused_chain"] == 0 and ms["fused_tail"] == 0, what
            assert ms["decimate"] > 0 and ms["resample"] > 0 and ms["filter"] > 0, what
            assert_bit_equal(got, ref, what)
        assert hip.lib.sdrhip_debug_small_chain_launches() == n0, "the one-kernel chain must not launch on a seam it does not fit"


def test_chain_run_as_hipgraph(hip, oracle):
    """sdrhip_fm_chain_graph_*: one run with fixed arguments captured into a hipGraph replays to the same audio, for as many
    launches as wanted and after the input changes under it."""
    nblk = 40
    total = nblk * B
    ch = _chain(hip)
    u8 = S.iq_u8_fm(total)
    d = to_dev(u8)
    q0, q1, _ = ch.plan(0, total, total)
    ws_bytes = ch.workspace_bytes(total)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    ref = _run(hip, ch, d, 0, total, q0, q1)
    out = dev_empty_f32(q1 - q0)
    g = hip.FmGraph(ch, ptr(d), 0, total, ptr(out), q0, q1, ptr(ws), ws_bytes)
    st = torch.cuda.current_stream()
    for _ in range(3):
        out.zero_()
        g.launch(st.cuda_stream)
        torch.cuda.synchronize()
        assert_bit_equal(to_host(out), ref, "graph replay")
    # new samples in the same buffer: the graph reads the buffer, not a snapshot
    u8b = S.iq_u8(total)
    d.copy_(torch.from_numpy(u8b).cuda())
    refb = _run(hip, ch, d, 0, total, q0, q1)
    g.launch(st.cuda_stream)
    torch.cuda.synchronize()
    assert_bit_equal(to_host(out), refb, "graph replay on new input")
    with pytest.raises(hip.SdrHipError):
        ch.enable_timing(True)
        try:
            hip.FmGraph(ch, ptr(d), 0, total, ptr(out), q0, q1, ptr(ws), ws_bytes)
        finally:
            ch.enable_timing(False)


# A stream whose largest push (8 blocks) runs in place: four slots, adaptive submission by default (piles of up to 64 blocks).
_IN_PLACE_PUSHES = ([3, 8, 1, 5, 8, 2, 8, 1], 13)      # 468 blocks per phase: two batches of 210 blocks and a remainder
_THRESHOLD_PHASES = {
    "large_pushes": [(None, [1, 1, 7, 200, 1, 16, 1, 199, 230, 7, 1, 2, 200, 1], 3)],
    "coalesce_above": [(("coalesce", 210),) + _IN_PLACE_PUSHES],
    "adaptive_above": [(("adaptive", 256),) + _IN_PLACE_PUSHES],
    "adaptive_off": [(("adaptive", 0),) + _IN_PLACE_PUSHES],
    "switched": [(("coalesce", 210),) + _IN_PLACE_PUSHES, (("coalesce", 0),) + _IN_PLACE_PUSHES,
                 (("adaptive", 256),) + _IN_PLACE_PUSHES, (("adaptive", 0),) + _IN_PLACE_PUSHES,
                 (("coalesce", 205),) + _IN_PLACE_PUSHES],
}


@pytest.mark.parametrize("phases", sorted(_THRESHOLD_PHASES))
def test_fm_stream_crosses_the_in_place_threshold(hip, oracle, phases):
    """sdrhip_fm_stream across the 200-block bound (carried tail included) between the slot-stream copy and the three-stream
    copy path, against one device-resident run.  large_pushes: pushes of 1 block (the kernel reads the pinned buffer in place),
    7, 16 and 199 blocks (one pass over the link on the slot's own stream, then the one-kernel chain on device memory), 200 and
    230 blocks (three-stream copy path, stage kernels) in one stream of two slots.  The others push 1 to 8 blocks into a stream
    whose largest push runs in place -- four slots, adaptive by default -- in phases that each end with a flush: set_coalesce
    batches of 203-210 blocks take the copy engines with four slots, set_adaptive piles of up to 256 blocks cross the bound
    depending on timing, set_adaptive(0) sends every push alone, and `switched` changes the setting between flushes in both
    directions across the bound."""
    plan = _THRESHOLD_PHASES[phases]
    total = sum(sum(pattern) * reps for _, pattern, reps in plan) * B
    u8 = S.iq_u8_fm(total)
    chain = _chain(hip)
    _, q1, _ = chain.plan(0, total, total)
    full = _run(hip, chain, to_dev(u8), 0, total, 0, q1)
    st = hip.FmStream(chain, (230 if phases == "large_pushes" else 8) * B, B)
    got, pos = [], 0
    for setting, pattern, reps in plan:
        if setting is not None:
            getattr(st, "set_" + setting[0])(setting[1] * B)
        for rep in range(reps):
            for k, n in enumerate(pattern):
                chunk = u8[2 * pos * B: 2 * (pos + n) * B]
                if (k + rep) % 2:
                    view = st.input_buffer(n * B)
                    view[: chunk.size] = chunk
                    got += st.push_inplace(view[: chunk.size])
                else:
                    got += st.push(chunk)
                pos += n
        got += st.flush()
    got = np.concatenate(got)
    assert got.size == q1 // B * B
    assert_bit_equal(got, full[: got.size], f"{phases}: mixed in-place / copied pushes vs resident")


@pytest.mark.parametrize("blocks_per_push", [1, 5])
def test_fm_stream_save_and_restore(hip, oracle, blocks_per_push):
    """Checkpoint / resume (sdrhip_fm_stream_save / _restore): a stream saved after some pushes, destroyed, restored into a
    fresh operator (over a fresh chain object with the same taps) and fed the rest yields the uninterrupted stream's audio."""
    nblk = 40
    u8 = S.iq_u8_fm(nblk * B)
    chain = _chain(hip)
    whole = hip.FmStream(chain, 8 * B, 2048)
    exp = []
    for i in range(0, nblk, blocks_per_push):
        exp += whole.push(u8[2 * i * B: 2 * (i + blocks_per_push) * B])
    exp += whole.flush()
    exp = np.concatenate(exp)

    first = hip.FmStream(chain, 8 * B, 2048)
    got = []
    cut = 15 if blocks_per_push == 5 else 17
    for i in range(0, cut, blocks_per_push):
        got += first.push(u8[2 * i * B: 2 * (i + blocks_per_push) * B])
    state = first.save()
    assert len(state) < 64 * 1024 + 4 * 2048 * 8, "the state is the position, ~4k samples of history and the unpopped audio"
    # the layout: StreamStateHeader (64 bytes), the history (u8 IQ samples), the audio not yet popped
    assert struct.calcsize("<IIqqqqqiiq") == 64
    magic, version, n, q_done, head_cap, hist_n, pending, block_out, chain_block, _ = struct.unpack_from("<IIqqqqqiiq", state)
    assert (magic, version, n, q_done, block_out, chain_block) == (0x53444d46, 1, cut * B, chain.ready(cut * B), 2048, B)
    assert 0 < hist_n <= head_cap and pending == q_done - 2048 * len(got)
    assert len(state) == 64 + 2 * hist_n + 4 * pending
    del first
    chain2 = _chain(hip)
    second = hip.FmStream(chain2, 8 * B, 2048)
    got += second.restore(state)
    with pytest.raises(hip.SdrHipError):
        hip.FmStream(chain2, 8 * B, 2048).restore(state[: 40])       # truncated
    with pytest.raises(hip.SdrHipError):
        second.restore(state)                                        # only into a stream that has not been pushed to
    for i in range(cut, nblk, blocks_per_push):
        got += second.push(u8[2 * i * B: 2 * (i + blocks_per_push) * B])
    got += second.flush()
    got = np.concatenate(got)
    assert_bit_equal(got, exp, "saved + restored stream vs uninterrupted")
    other = hip.FmStream(chain2, 8 * B, 4096)
    with pytest.raises(hip.SdrHipError):
        other.restore(state)                             # another output block size


def test_fm_stream_many_mixed_pushes(hip):
    """A long stream of pushes of mixed sizes -- one block (fused tail, in place), a few (stage kernels, in place, the two
    compute streams in turn), 200 and 230 blocks (copy engines) -- zero-copy and memcpy pushes interleaved: every audio sample
    equals the device-resident run over the whole stream.  (What a race between consecutive pushes on the two compute streams,
    or a stale workspace / history, would break.)"""
    rng = np.random.default_rng(515 + SWEEP_SEED)
    choices = np.array([1, 1, 1, 2, 3, 7, 16, 80, 200, 230, 1, 2])
    pattern = rng.choice(choices, size=min(300 * SWEEP_SCALE, 6000))
    nblk = int(pattern.sum())
    total = nblk * B
    u8 = torch.randint(0, 256, (2 * total,), dtype=torch.uint8)
    chain = _chain(hip)
    _, q1, _ = chain.plan(0, total, total)
    ref = _run(hip, chain, u8.cuda(), 0, total, 0, q1)
    st = hip.FmStream(_chain(hip), 230 * B, B)
    host = u8.numpy()
    got, pos = [], 0
    for k, n in enumerate(pattern):
        chunk = host[2 * pos * B: 2 * (pos + n) * B]
        if k % 3 == 1:
            view = st.input_buffer(n * B)
            view[: chunk.size] = chunk
            got += st.push_inplace(view[: chunk.size])
        else:
            got += st.push(chunk)
        pos += n
    got += st.flush()
    got = np.concatenate(got)
    assert got.size == q1 // B * B
    assert_bit_equal(got, ref[: got.size], "mixed pushes vs resident run")


@pytest.mark.parametrize("nblk", [40, 1200])
def test_two_runs_in_flight_equal_the_single_stream(hip, nblk):
    """sdrhip_fm_chain_set_overlap (round 4): consecutive runs alternate between two internal streams and workspace halves.
    Seven back-to-back runs over three different inputs, audio double-buffered as the contract asks, the input of a run produced
    on the caller's stream right before it -- bit-equal with the same runs one at a time.  nblk = 40: the one-kernel chain;
    1200: the stage kernels (systolic decimator, fmDemod, resampler, filter and their seam fix-ups)."""
    total = nblk * B
    chain = _chain(hip)
    q0, q1, _ = chain.plan(0, total, total)
    gen = torch.Generator(device="cuda").manual_seed(5)
    inputs = [torch.randint(0, 256, (2 * total,), dtype=torch.uint8, device="cuda", generator=gen) for _ in range(3)]
    refs = [torch.from_numpy(_run(hip, chain, x, 0, total, q0, q1)).cuda() for x in inputs]
    chain.set_overlap(True)
    ws_bytes = chain.workspace_bytes(total)
    assert ws_bytes >= 2 * (chain.workspace_bytes(total) // 2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    audio = [dev_empty_f32(q1 - q0) for _ in range(2)]          # (between guard bands: gpu_util)
    stage = torch.empty_like(inputs[0])
    st = torch.cuda.current_stream()
    checked = 0
    order = [0, 1, 2, 2, 0, 1, 0]
    for k, which in enumerate(order):
        # the previous-but-one run's audio is complete on this stream now: check it before its buffer is reused
        if k >= 2:
            assert torch.equal(audio[k % 2].view(torch.int32), refs[order[k - 2]].view(torch.int32)), f"run {k - 2}"
            checked += 1
        stage_k = stage if k % 2 == 0 else inputs[which]          # every other run reads an input copied in just before it
        if k % 2 == 0:
            stage.copy_(inputs[which])
        chain.run(ptr(stage_k), 0, total, ptr(audio[k % 2]), q0, q1, ptr(ws), ws_bytes, stream=st.cuda_stream)
        if k % 2 == 0 and k + 2 < len(order):
            # `stage` is overwritten two runs later: that copy is queued on the caller's stream, which by then waits for this run
            pass
    chain.join(st.cuda_stream)
    n = len(order)
    assert torch.equal(audio[(n - 1) % 2].view(torch.int32), refs[order[n - 1]].view(torch.int32))
    assert torch.equal(audio[(n - 2) % 2].view(torch.int32), refs[order[n - 2]].view(torch.int32))
    assert checked == n - 2
    chain.set_overlap(False)
    again = _run(hip, chain, inputs[1], 0, total, q0, q1)
    assert np.array_equal(again.view(np.int32), refs[1].cpu().numpy().view(np.int32))
