"""GPU parity of the FM chain with a tuner (sdrhip_fm_chain_set_tuner): a periodic oscillator mixed in between convert and the
decimator, on every route of the chain -- stage kernels (the tuner's tile kernel, or the mix into the workspace and the stock
decimator), decimator + fused tail, and the tuned one-kernel chain (kernels_small.hip) -- against

  * the restated Pipes with the oscillator stage (tests/tuned_chain_model.py), and
  * the defining identity: sdrhip_tuner_run_u8 -> sdrhip_fm_demod_run -> sdrhip_resampler_run -> sdrhip_filter_run ->
    sdrhip_scale_run driven by hand over the same ranges,

bit for bit.  The chain is that of tests/test_gpu_chain.py: /8 with 127 taps, 3/10 with 191 taps, 64 half taps, gain 0.2."""
import numpy as np
import pytest
import torch

import signals as S
import tuned_chain_model as TCM
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B = 8192
GAIN = 0.2
NLOOP = 64                  # floats a resampler output walks (191 taps in 3 groups, padded): the chain's reach in y


def _random5():
    return np.random.default_rng(20250).uniform(-1.5, 1.5, 10).astype(np.float32)


# 8313 is coprime to the one-kernel chain's tile span of 8312 samples; 5 and 1000 divide neither a tile nor a block
TABLES = {
    "shift 1/4": lambda: TM.shift_table(1, 4),
    "shift -3/1000": lambda: TM.shift_table(-3, 1000),
    "shift 5/8313": lambda: TM.shift_table(5, 8312 + 1),
    "random, period 5": _random5,
    "shift 1/65536": lambda: TM.shift_table(1, 65536),
}
# test_gpu_tuner.py::test_user_table_with_subnormals_and_negative_zeros
SUBNORMALS = np.array([1e-42, -3e-39, -0.0, 1.0, 0.0, -0.0, 0.70710677, -0.70710677, -1.0, 1e-45, 2.5, -0.0, 1e-30, 3.0, -0.0, -0.0],
                      np.float32)[:14]
IDENTITY = np.array([1.0, 0.0], np.float32)

_cache = {}


def table(name):
    if ("osc", name) not in _cache:
        t = TABLES[name]()
        t.setflags(write=False)
        _cache[("osc", name)] = t
    return _cache[("osc", name)]


def stream_u8(nblk=300):
    """One stream for the whole module (uploaded once); tests take prefixes and slices of it.  FM-modulated: the audio is not noise."""
    if "u8" not in _cache:
        u8 = S.iq_u8_fm(300 * B)
        _cache["u8_dev"] = to_dev(u8)
        u8.setflags(write=False)
        _cache["u8"] = u8
    return _cache["u8"][:2 * nblk * B]


def stream_dev():
    stream_u8()
    return _cache["u8_dev"]


def model(oracle, name, nblk=96):
    """The restated Pipes on the first 96 source blocks: 2 audio blocks (computed once per table, shared, never written)."""
    key = ("model", name, nblk)
    if key not in _cache:
        u8 = stream_u8(nblk)
        blocks = [u8[2 * i * B:2 * (i + 1) * B] for i in range(nblk)]
        out = TCM.fm_receiver_tuned(oracle, blocks, table(name), S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(),
                                    GAIN, B, PM.ORDER_AVX)
        e = np.concatenate(out)
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


def _chain(hip, osc=None, block=B, order=None):
    ch = hip.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), GAIN, block,
                     hip.ORDER_AVX if order is None else order)
    if osc is not None:
        ch.set_tuner(osc)
    return ch


ROUTES = ("stage", "tail", "small")


def _route(ch, route):
    """stage: the stage kernels; tail: decimator + fused tail wherever it fits; small: the one-kernel chain wherever it fits."""
    ch.set_small_chain(1 if route == "small" else 0)
    ch.set_fused_tail(1 if route == "tail" else 0)


def _run(hip, chain, d_in, s0, n_in, q0, q1):
    ws_bytes = chain.workspace_bytes(n_in)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = dev_empty_f32(q1 - q0)
    chain.run(ptr(d_in), s0, n_in, ptr(out), q0, q1, ptr(ws), ws_bytes)
    return to_host(out)


def _small_fits(block):
    """fm_chain_small_fits for this chain on aligned input: a contiguous stream, or seam blocks of 192 .. 2^26 samples."""
    return block == 0 or 192 <= block <= 1 << 26


def _compose(hip, d_in, s0, q0, q1, osc, block, order=None, decim_taps=None):
    """The defining identity, by hand: the tuner's decimator outputs, then the existing operators over the chain's ranges."""
    order = hip.ORDER_AVX if order is None else order
    t = hip.Tuner(8, S.taps_decim127() if decim_taps is None else decim_taps, osc, order)
    res = hip.Resampler(3, 10, S.taps_resamp191(), order)
    filt = hip.Filter(S.taps_audio_half64(), order, sym=True)
    m1 = q1 + filt.num_coeffs - 1
    ky0, ky1 = res.in_offset(q0), res.in_offset(m1 - 1) + NLOOP
    kd0, kd1 = max(ky0 - 1, 0), ky1
    d = dev_empty_f32(2 * (kd1 - kd0))
    t.run_u8(ptr(d_in), s0, ptr(d), kd0, kd1, block)
    y = dev_empty_f32(ky1 - ky0)
    hip.check(hip.lib.sdrhip_fm_demod_run(None, ptr(d), kd0, ptr(y), ky0, ky1, 0.0, 0.0), "sdrhip_fm_demod_run")
    z = dev_empty_f32(m1 - q0)
    res.run(ptr(y), ky0, ptr(z), q0, m1, block, out_block=block)
    a = dev_empty_f32(q1 - q0)
    filt.run(ptr(z), q0, ptr(a), q0, q1, block)
    out = dev_empty_f32(q1 - q0)
    hip.check(hip.lib.sdrhip_scale_run(None, GAIN, ptr(a), ptr(out), q1 - q0), "sdrhip_scale_run")
    return to_host(out)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shift 1/4", "shift -3/1000"])
def test_stage_route_against_the_model(hip, oracle, name):
    """90 blocks as test_chain_matches_pipes (2 audio blocks), the one-kernel chain and the fused tail off."""
    nblk = 90
    exp = model(oracle, name)
    assert exp.size == 2 * B
    ch = _chain(hip, table(name))
    assert ch.tuner_period() == table(name).size // 2
    _route(ch, "stage")
    total = nblk * B
    q0, q1, halo = ch.plan(0, total, total)
    assert q0 == 0 and halo == 0 and q1 >= exp.size
    c0, t0 = hip.small_chain_tuned_launches(), hip.tuner_fused_launches()
    got = _run(hip, ch, stream_dev(), 0, total, 0, q1)
    assert hip.small_chain_tuned_launches() == c0 and hip.tuner_fused_launches() == t0 + 1, "aligned input: the tuner's tile kernel"
    assert_bit_equal(got[:exp.size], exp, f"{name}: stage kernels vs the restated Pipes")


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [B, 0, 3 * B])
def test_defining_identity_on_the_device(hip, block):
    nblk = 40
    total = nblk * B
    d = stream_dev()
    for name in TABLES:
        osc = table(name)
        ch = _chain(hip, osc, block)
        q0, q1, _ = ch.plan(0, total, total)
        exp = _compose(hip, d, 0, q0, q1, osc, block)
        for route in ROUTES:
            _route(ch, route)
            assert_bit_equal(_run(hip, ch, d, 0, total, q0, q1), exp, f"{name}, block {block}, {route} route vs the operators by hand")
        # a range inside the stream, from an output that starts no polyphase cycle
        a, b = 1000, 3001
        exp = _compose(hip, d, 0, a, b, osc, block)
        for route in ROUTES:
            _route(ch, route)
            assert_bit_equal(_run(hip, ch, d, 0, total, a, b), exp, f"{name}, block {block}, {route} route, outputs [{a},{b})")


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block", [B, 0, 3 * B, 1000, 200, 160])
def test_routes_are_bit_equal(hip, block):
    """The one-kernel chain and the fused tail forced on against the stage kernels.  The tuned one-kernel chain must launch exactly
    where fm_chain_small_fits holds: seam blocks 1000 and 200 are inside its range (>= 192; at 200 a tile meets 41 buffer boundaries
    and the owners walk their Cross outputs), as test_small_chain_equals_stage_kernels asserts for the untuned kernel; 160 is the
    seam block below it, where a forced one-kernel chain falls through to the stage kernels."""
    d = stream_dev()
    # 3 blocks: one tile with a ragged end; 300 blocks: many tiles; [1000, 3001) and [q1 - 2000, q1): q0 not a multiple of 3
    for name in TABLES:
        ch = _chain(hip, table(name), block)
        for nblk in (3, 300):
            total = nblk * B
            _, q1, _ = ch.plan(0, total, total)
            ranges = [(0, q1)] if nblk == 3 else [(0, q1), (1000, 3001), (q1 - 2000, q1)]
            for a, b in ranges:
                assert a % 3 != 0 or a == 0
                _route(ch, "stage")
                c0 = hip.small_chain_tuned_launches()
                ref = _run(hip, ch, d, 0, total, a, b)
                _route(ch, "tail")
                tail = _run(hip, ch, d, 0, total, a, b)
                assert hip.small_chain_tuned_launches() == c0, "the one-kernel chain launched while it was switched off"
                _route(ch, "small")
                n0 = hip.lib.sdrhip_debug_small_chain_launches()
                small = _run(hip, ch, d, 0, total, a, b)
                what = f"{name}, block {block}, {nblk} blocks, outputs [{a},{b})"
                assert hip.small_chain_tuned_launches() - c0 == (1 if _small_fits(block) else 0), what + ": wrong route"
                assert hip.lib.sdrhip_debug_small_chain_launches() - n0 == (1 if _small_fits(block) else 0), what
                assert_bit_equal(tail, ref, what + ": fused tail vs stage kernels")
                assert_bit_equal(small, ref, what + ": one-kernel chain vs stage kernels")
        if name == "shift -3/1000":
            # every tile size of the one-kernel chain: the phase of a tile's first sample follows the tile stride
            total = 300 * B
            _, q1, _ = ch.plan(0, total, total)
            _route(ch, "stage")
            ref = _run(hip, ch, d, 0, total, 158, 158 + 4093)
            for tile in (159, 96, 48, 3):
                ch.set_small_chain(1, 0, tile)
                assert_bit_equal(_run(hip, ch, d, 0, total, 158, 158 + 4093), ref, f"block {block}, tile of {tile} outputs")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["small", "stage"])
@pytest.mark.parametrize("name", ["shift -3/1000", "random, period 5"])
def test_cuts_and_shards(hip, name, route):
    """One stream of 40 blocks as 1 run and as 4 shards with right halos (each shard a buffer of its own, global indices): the
    oscillator phase follows s0."""
    nblk = 40
    total = nblk * B
    u8 = stream_u8(nblk)
    ch = _chain(hip, table(name))
    _route(ch, route)
    Q0, Q1, _ = ch.plan(0, total, total)
    full = _run(hip, ch, stream_dev(), 0, total, Q0, Q1)
    nshards = 4
    S_len = (total // nshards // 8 - 1) * 8              # 81912: a shard starts at no multiple of either period
    assert S_len % 1000 != 0 and S_len % 5 != 0 and S_len % 8 == 0
    pieces, prev = [], Q0
    for r in range(nshards):
        s0 = r * S_len
        s1 = total if r == nshards - 1 else (r + 1) * S_len
        q0, q1, halo = ch.plan(s0, s1, total)
        assert q0 == prev and halo <= ch.max_halo()
        prev = q1
        n_in = min(total, s1 + halo) - s0
        pieces.append(_run(hip, ch, to_dev(u8[2 * s0:2 * (s0 + n_in)]), s0, n_in, q0, q1))
    assert prev == Q1
    assert_bit_equal(np.concatenate(pieces), full, f"{name}, {route} route: 4 shards vs one run")


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_far_stream_position(hip):
    """s0 = 2^34 + 8 * 12345: the buffer holds only the run's 6 blocks.  Pins the 64-bit part of the phase on every route (the host's
    one modulo per launch); test_gpu_tuner.py::test_far_stream_position holds the tuner itself to the model there."""
    s0 = 2 ** 34 + 8 * 12345
    assert s0 % 8 == 0 and s0 % B == 456 and s0 % 1000 == 944
    n_in = 6 * B
    osc = table("shift -3/1000")
    d = to_dev(stream_u8(6))
    ch = _chain(hip, osc)
    q0, q1, halo = ch.plan(s0, s0 + n_in, s0 + n_in)
    assert halo == 0 and q1 - q0 > 1500 and q0 > 2 ** 29
    exp = _compose(hip, d, s0, q0, q1, osc, B)
    c0 = hip.small_chain_tuned_launches()
    for route in ROUTES:
        _route(ch, route)
        assert_bit_equal(_run(hip, ch, d, s0, n_in, q0, q1), exp, f"far position, {route} route vs the operators by hand")
    assert hip.small_chain_tuned_launches() == c0 + 1
    # the same samples at the stream's start give other audio: the position reached the oscillator
    near = _run(hip, ch, d, 0, n_in, *ch.plan(0, n_in, n_in)[:2])
    assert not np.array_equal(near[:1000], exp[:1000])


# ---- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_subnormal_entries_and_signed_zeros(hip):
    """A table no shortcut survives.  With a subnormal entry ((u - 128) / 128) * o and (u - 128) * o round differently: the tuned
    one-kernel chain converts in full and reads the unscaled taps."""
    nblk = 6
    total = nblk * B
    d = stream_dev()
    for block in (B, 0):
        ch = _chain(hip, SUBNORMALS, block)
        q0, q1, _ = ch.plan(0, total, total)
        exp = _compose(hip, d, 0, q0, q1, SUBNORMALS, block)
        c0 = hip.small_chain_tuned_launches()
        for route in ROUTES:
            _route(ch, route)
            assert_bit_equal(_run(hip, ch, d, 0, total, q0, q1), exp, f"subnormal table, block {block}, {route} route")
        assert hip.small_chain_tuned_launches() == c0 + 1
    # a decimator of 128 taps: its last prepared tap is no padding, which selects the kernel instantiation that skips no MAC
    taps128 = S.gauss_taps(128, 128128)
    osc = table("random, period 5")
    ch = hip.FmChain(8, taps128, 3, 10, S.taps_resamp191(), S.taps_audio_half64(), GAIN, B)
    ch.set_tuner(osc)
    q0, q1, _ = ch.plan(0, total, total)
    exp = _compose(hip, d, 0, q0, q1, osc, B, decim_taps=taps128)
    c0 = hip.small_chain_tuned_launches()
    for route in ROUTES:
        _route(ch, route)
        assert_bit_equal(_run(hip, ch, d, 0, total, q0, q1), exp, f"128-tap decimator, {route} route")
    assert hip.small_chain_tuned_launches() == c0 + 1


# ---- 7 ---------------------------------------------------------------------------------------------------------------------------
def test_identity_table_is_the_untuned_chain(hip):
    nblk = 40
    total = nblk * B
    d = stream_dev()
    plain, tuned = _chain(hip), _chain(hip, IDENTITY)
    q0, q1, _ = plain.plan(0, total, total)
    for route in ROUTES:
        _route(plain, route)
        _route(tuned, route)
        c0 = hip.small_chain_tuned_launches()
        ref = _run(hip, plain, d, 0, total, q0, q1)
        assert hip.small_chain_tuned_launches() == c0, "an untuned chain launched the tuned kernel"
        assert_bit_equal(_run(hip, tuned, d, 0, total, q0, q1), ref, f"table (1, +0), {route} route vs the untuned chain")
        assert hip.small_chain_tuned_launches() - c0 == (1 if route == "small" else 0)


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------
def test_a_chain_that_lost_its_tuner(hip):
    nblk = 40
    total = nblk * B
    d = stream_dev()
    never, had = _chain(hip), _chain(hip, table("shift 1/4"))
    q0, q1, _ = never.plan(0, total, total)
    tuned_audio = _run(hip, had, d, 0, total, q0, q1)
    assert had.workspace_bytes(total) > never.workspace_bytes(total)
    had.set_tuner(None)
    assert had.tuner_period() == 0
    for n in (0, B, total, 1 << 27):
        assert had.workspace_bytes(n) == never.workspace_bytes(n)
    for route in ROUTES + ("auto",):
        for ch in (never, had):
            if route == "auto":
                ch.set_small_chain(2)
                ch.set_fused_tail(2)
            else:
                _route(ch, route)
        c0, n0, t0 = hip.small_chain_tuned_launches(), hip.lib.sdrhip_debug_small_chain_launches(), hip.tuner_fused_launches()
        ref = _run(hip, never, d, 0, total, q0, q1)
        n1 = hip.lib.sdrhip_debug_small_chain_launches()
        got = _run(hip, had, d, 0, total, q0, q1)
        assert hip.lib.sdrhip_debug_small_chain_launches() - n1 == n1 - n0 == (1 if route in ("small", "auto") else 0), route
        assert hip.small_chain_tuned_launches() == c0 and hip.tuner_fused_launches() == t0, "no tuner, no tuner kernels"
        assert_bit_equal(got, ref, f"tuner removed, {route} route vs a chain that never had one")
    assert not np.array_equal(tuned_audio, ref)
    had.set_tuner(table("shift 1/4"))                      # ... and back
    had.set_small_chain(2)
    had.set_fused_tail(2)
    assert_bit_equal(_run(hip, had, d, 0, total, q0, q1), tuned_audio, "tuner set again")


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------
def _push_all(st, u8, sizes, inplace_every=0):
    got, pos = [], 0
    for k, n in enumerate(sizes):
        chunk = u8[2 * pos * B:2 * (pos + n) * B]
        if inplace_every and k % inplace_every == 0:
            view = st.input_buffer(n * B)[:chunk.size]
            view[:] = chunk
            got += st.push_inplace(view)
        else:
            got += st.push(chunk)
        pos += n
    return got


@pytest.mark.parametrize("blocks_per_push", [1, 3, 16])
def test_fm_stream_against_the_model(hip, oracle, blocks_per_push):
    """A lone block is read in place over the link by the kernel itself, 3 and 16 blocks are copied to the device on the slot's stream:
    one launch of the tuned one-kernel chain either way."""
    nblk = 96
    name = "shift -3/1000"
    exp = model(oracle, name)
    u8 = stream_u8(nblk)
    st = hip.FmStream(_chain(hip, table(name)), blocks_per_push * B, B)
    c0 = hip.small_chain_tuned_launches()
    got = _push_all(st, u8, [blocks_per_push] * (nblk // blocks_per_push)) + st.flush()
    assert hip.small_chain_tuned_launches() > c0
    assert len(got) >= 2
    assert_bit_equal(np.concatenate(got[:2]), exp, f"tuned fm stream, {blocks_per_push} blocks per push, vs the restated Pipes")


def test_fm_stream_ragged_pushes_and_coalescing(hip, oracle):
    nblk = 96
    name = "shift 1/4"
    exp = model(oracle, name)
    u8 = stream_u8(nblk)
    sizes = [1, 3, 2, 16, 5, 1, 1, 7, 16, 4, 2, 1, 9, 16, 12]
    assert sum(sizes) == nblk
    for setting in (None, ("coalesce", 7), ("adaptive", 32)):
        st = hip.FmStream(_chain(hip, table(name)), 16 * B, B)
        if setting:
            getattr(st, "set_" + setting[0])(setting[1] * B)
        got = _push_all(st, u8, sizes, inplace_every=3) + st.flush()
        assert len(got) >= 2
        assert_bit_equal(np.concatenate(got[:2]), exp, f"ragged tuned stream ({setting}) vs the restated Pipes")


def test_fm_stream_save_and_restore(hip):
    """Saved after 5 blocks (40960 samples: no multiple of 1000), restored into a fresh stream over a second tuned chain: the phase
    is a closed form of the saved position, the state layout is the untuned stream's."""
    nblk = 40
    name = "shift -3/1000"
    u8 = stream_u8(nblk)
    whole = hip.FmStream(_chain(hip, table(name)), 8 * B, 2048)
    exp = np.concatenate(_push_all(whole, u8, [1] * nblk) + whole.flush())
    first = hip.FmStream(_chain(hip, table(name)), 8 * B, 2048)
    got = _push_all(first, u8, [1] * 5)
    state = first.save()
    plain = hip.FmStream(_chain(hip), 8 * B, 2048)
    _push_all(plain, u8, [1] * 5)
    assert len(state) == len(plain.save())
    del first
    second = hip.FmStream(_chain(hip, table(name)), 8 * B, 2048)
    got += second.restore(state)
    got += _push_all(second, u8[2 * 5 * B:], [1] * (nblk - 5)) + second.flush()
    assert_bit_equal(np.concatenate(got), exp, "tuned stream saved and restored vs uninterrupted")


# ---- 10 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["small", "stage"])
def test_graph_replays_a_tuned_run(hip, route):
    nblk = 40
    total = nblk * B
    d = stream_dev()
    ch = _chain(hip, table("shift 5/8313"))
    _route(ch, route)
    q0, q1, _ = ch.plan(0, total, total)
    ref = _run(hip, ch, d, 0, total, q0, q1)
    ws_bytes = ch.workspace_bytes(total)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    out = dev_empty_f32(q1 - q0)
    g = hip.FmGraph(ch, ptr(d), 0, total, ptr(out), q0, q1, ptr(ws), ws_bytes)
    st = torch.cuda.current_stream()
    for i in range(2):
        out.zero_()
        g.launch(st.cuda_stream)
        torch.cuda.synchronize()
        assert_bit_equal(to_host(out), ref, f"{route} route, graph launch {i}")


@pytest.mark.parametrize("route", ["small", "stage"])
def test_two_runs_in_flight_on_a_tuned_chain(hip, route):
    """set_overlap(1): 4 consecutive runs over the 4 quarters of one stream (each with its right halo) alternate between the two
    lanes and workspace halves; together they are the single stream's audio."""
    nblk = 40
    total = nblk * B
    d = stream_dev()
    ch = _chain(hip, table("shift -3/1000"))
    _route(ch, route)
    Q0, Q1, _ = ch.plan(0, total, total)
    full = _run(hip, ch, d, 0, total, Q0, Q1)
    ch.set_overlap(True)
    ws_bytes = ch.workspace_bytes(total)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    st = torch.cuda.current_stream()
    S_len = total // 4
    outs = []
    for r in range(4):
        s0, s1 = r * S_len, (r + 1) * S_len
        q0, q1, halo = ch.plan(s0, s1, total)
        out = dev_empty_f32(q1 - q0)                      # an audio buffer per run
        ch.run(ptr(d) + 2 * s0, s0, min(total, s1 + halo) - s0, ptr(out), q0, q1, ptr(ws), ws_bytes, stream=st.cuda_stream)
        outs.append(out)
    ch.join(st.cuda_stream)
    got = np.concatenate([to_host(o) for o in outs])
    ch.set_overlap(False)
    assert_bit_equal(got, full, f"{route} route: 4 runs, two in flight, vs the single stream")


# ---- 11 --------------------------------------------------------------------------------------------------------------------------
def test_reference_example_taps(hip, oracle):
    """The reference example's own taps (51 / 31 / 64): the one-kernel chain does not fit 56 prepared taps, and the tuner's tile
    kernel walks them four at a time.  90 blocks, as test_stage_route_against_the_model: 40 blocks are 12288 resampler outputs, one
    block of them, and the audio filter's Pipe yields its first 8192-sample block only once a second one has arrived."""
    nblk = 90
    total = nblk * B
    hd, hr, ha = S.taps_example_rf_decim(), S.taps_example_audio_resampler(), S.taps_example_audio_filter_half()
    osc = table("shift 1/4")
    u8 = stream_u8(nblk)
    blocks = [u8[2 * i * B:2 * (i + 1) * B] for i in range(nblk)]
    exp = np.concatenate(TCM.fm_receiver_tuned(oracle, blocks, osc, hd, 8, hr, 3, 10, ha, GAIN, B, PM.ORDER_AVX))
    assert exp.size == 2 * B
    ch = hip.FmChain(8, hd, 3, 10, hr, ha, GAIN, B)
    ch.set_tuner(osc)
    q0, q1, _ = ch.plan(0, total, total)
    assert q0 == 0 and q1 >= exp.size
    for route in ("stage", "small"):                       # forced on, the one-kernel chain falls through to the stage kernels
        _route(ch, route)
        c0, t0 = hip.small_chain_tuned_launches(), hip.tuner_fused_launches()
        got = _run(hip, ch, stream_dev(), 0, total, 0, q1)
        assert hip.small_chain_tuned_launches() == c0 and hip.tuner_fused_launches() == t0 + 1
        assert_bit_equal(got[:exp.size], exp, f"example taps, {route} requested, vs the restated Pipes")


# ---- the mix into the workspace --------------------------------------------------------------------------------------------------
def test_input_that_is_not_16_byte_aligned_mixes_into_the_workspace(hip):
    """d_in 2 bytes off a 16-byte boundary: neither the one-kernel chain nor the tuner's tile kernel can load it; the run mixes into
    the start of the workspace and the stock decimator runs on that.  Same bits."""
    nblk = 12
    total = nblk * B
    u8 = stream_u8(nblk)
    shifted = to_dev(np.concatenate([np.zeros(2, np.uint8), u8]))[2:]
    assert ptr(shifted) % 16 == 2
    for name in ("shift -3/1000", "random, period 5"):
        for block in (B, 0):
            ch = _chain(hip, table(name), block)
            q0, q1, _ = ch.plan(0, total, total)
            _route(ch, "stage")
            ref = _run(hip, ch, stream_dev(), 0, total, q0, q1)
            for route in ("stage", "small", "tail"):
                _route(ch, route)
                c0, t0 = hip.small_chain_tuned_launches(), hip.tuner_fused_launches()
                got = _run(hip, ch, shifted, 0, total, q0, q1)
                assert hip.small_chain_tuned_launches() == c0 and hip.tuner_fused_launches() == t0, "an unaligned run took a tile kernel"
                assert_bit_equal(got, ref, f"{name}, block {block}, {route} requested: unaligned input vs aligned")


def test_other_orders_and_factors_mix_into_the_workspace(hip):
    """The SSE order has no tuned tile kernel: mix + the stock decimator, against the operators by hand in that order."""
    nblk = 12
    total = nblk * B
    osc = table("shift -3/1000")
    ch = _chain(hip, osc, order=hip.ORDER_SSE)
    q0, q1, _ = ch.plan(0, total, total)
    t0 = hip.tuner_fused_launches()
    got = _run(hip, ch, stream_dev(), 0, total, q0, q1)
    exp = _compose(hip, stream_dev(), 0, q0, q1, osc, B, hip.ORDER_SSE)
    assert hip.tuner_fused_launches() == t0
    assert_bit_equal(got, exp, "SSE order, tuned chain vs the operators by hand")
