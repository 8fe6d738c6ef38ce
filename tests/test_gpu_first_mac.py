"""The first multiply-add of every lane partial is one fma onto a literal +0 (sdr_amd/csrc/first_mac.hpp) in the three kernels of a
full-size FM pass: the systolic decimator, the packed walk of the 3/10 resampler's tile kernel, the fast real FIR filter.  That is
the reference's `+0 + round(a * b)` bit for bit -- unless a kernel took the shortcut `partial = product`, which leaves -0 where the
reference has +0.  So every case here feeds inputs whose FIRST products are -0 (a zero sample under a negative tap) and compares
every result bit with the oracle through view(int32): the sign of zero counts.

test_inputs_on_the_cpu (no GPU) shows for each case that the inputs do produce -0 first products, that the oracle's outputs hold no
-0, and, where the reference build (oracle/_ref) is present, that it agrees with the oracle."""
import functools

import numpy as np
import pytest

import signals as S
from conftest import assert_bit_equal
from oracle.oracle import duplicate

gpu = pytest.mark.gpu

NEG_ZERO = np.uint32(0x80000000)
K2_K = 64 * 240 * 4 + 37               # the smallest launch the systolic kernel takes, plus a ragged strip
K5_K = 2 * 1024 + 37                   # two tiles of the filter kernel and a ragged one
K4_K = 3 * 768 + 100                   # three tiles of the resampler's tile kernel (256 cycles of 3 outputs) and a ragged one
K4_STARTS = (0, 1, 2)                  # first output's polyphase group: 1 and 2 put outputs in front of the first whole cycle
GAIN = 0.2
CHAIN_TOTAL = 60000                    # samples of the chain case: 2100 audio outputs, past K5_K


@functools.lru_cache(maxsize=None)
def _oracle():
    from oracle.oracle import Oracle
    return Oracle()


def _frozen(a):
    a.setflags(write=False)
    return a


def _neg_zero_count(a):
    return int((np.ascontiguousarray(a, np.float32).view(np.uint32) == NEG_ZERO).sum())


# ---- K2: the systolic decimator ----------------------------------------------------------------------------------------------------
def _neg8_taps():
    """127 taps, the first eight negative and the rest positive: the first products of all four partials of an output (taps 0 .. 3)
    are -0 under a zero sample, and nothing later in the partial is"""
    t = np.abs(S.taps_decim127())
    t[:8] = -t[:8]
    return t


K2_CASES = {"random input, the chain's taps": ("random", S.taps_decim127),
            "random input, first eight taps negative": ("random", _neg8_taps),
            "all-128 input, all taps negative": ("silence", lambda: -np.abs(S.taps_decim127()))}


@functools.lru_cache(maxsize=None)
def _k2_raw(kind):
    n = 8 * (K2_K - 1) + 128
    if kind == "silence":
        return _frozen(np.full(2 * n, 128, np.uint8))
    raw = S.iq_u8(n, seed=5100).copy()
    raw[3::4] = 128                      # every fourth byte: converts to exactly +0.0
    return _frozen(raw)


@functools.lru_cache(maxsize=None)
def _k2_expected(name):
    kind, taps = K2_CASES[name]
    h = np.concatenate([taps(), np.zeros(1, np.float32)])
    return _frozen(_oracle().decimate_rc(4, K2_K, 8, duplicate(h), _oracle().convert_u8(_k2_raw(kind))))


def _k2_first_products(name):
    """partial k of output o starts with tap k times sample 8 o + k (k = 0 .. 3), re and im"""
    kind, taps = K2_CASES[name]
    x = _oracle().convert_u8(_k2_raw(kind)).reshape(-1, 2)
    h = taps()
    return np.stack([x[k:8 * K2_K:8] * h[k] for k in range(4)])


# ---- K5: the fast real filter -------------------------------------------------------------------------------------------------------
def _half_neg8():
    h = S.taps_audio_half64().copy()
    h[:8] = -np.abs(h[:8])
    return h


K5_CASES = ("zeros", "zeros sprinkled in")


@functools.lru_cache(maxsize=None)
def _k5_input(name):
    n = K5_K + 127
    if name == "zeros":
        return _frozen(np.zeros(n, np.float32))
    x = S.real_block(n, seed=5200).copy()
    x[::3] = 0.0
    x[700:1000] = 0.0                    # whole windows of zeros: the pair sums x[o + k] + x[o + 127 - k] are +0
    x[1500:1500 + 64] = -x[1500 + 127:1500 + 63:-1]      # and a window whose pair sums cancel
    return _frozen(x)


@functools.lru_cache(maxsize=None)
def _k5_expected(name):
    return _frozen(_oracle().filter_sym_rr(8, K5_K, _half_neg8(), _k5_input(name)))


def _k5_first_products(name):
    x, h = _k5_input(name), _half_neg8()
    o = np.arange(K5_K)
    return np.stack([h[k] * (x[o + k] + x[o + 127 - k]) for k in range(8)])


# ---- K4: the resampler's tile kernel -----------------------------------------------------------------------------------------------
K4_CASES = {"zeros, all taps negative": ("zeros", lambda: -np.abs(S.taps_resamp191())),
            "zeros sprinkled in, the chain's taps": ("sprinkled", S.taps_resamp191)}


@functools.lru_cache(maxsize=None)
def _k4_input(kind):
    n = -(-(max(K4_STARTS) + K4_K) * 10 // 3) + 64 + 16
    if kind == "zeros":
        return _frozen(np.zeros(n, np.float32))
    x = S.real_block(n, seed=5300).copy()
    x[::3] = 0.0
    x[3000:3200] = 0.0
    return _frozen(x)


def _k4_offset(m):
    return -((-m * 10) // 3)


@functools.lru_cache(maxsize=None)
def _k4_prep(name):
    return _oracle().prepare_coeffs(8, 3, 10, K4_CASES[name][1]())


@functools.lru_cache(maxsize=None)
def _k4_expected(name, start):
    x = _k4_input(K4_CASES[name][0])
    out, _ = _oracle().resample_rr(8, K4_K, _k4_prep(name), start % 3, x[_k4_offset(start):])
    return _frozen(out)


def _k4_first_products(name, start):
    """lane partial j of output m starts with tap j of m's polyphase row times input in_offset(m) + j (j = 0 .. 7)"""
    x, rows = _k4_input(K4_CASES[name][0]), _k4_prep(name)["groups"]
    m = np.arange(start, start + K4_K)
    off = -((-m * 10) // 3)
    return np.stack([rows[m % 3, j] * x[off + j] for j in range(8)])


# ---- the chain's stage route: the only way to the filter kernel's fused gain ------------------------------------------------------
def _chain_taps():
    return -np.abs(S.taps_decim127()), -np.abs(S.taps_resamp191()), _half_neg8()


@functools.lru_cache(maxsize=None)
def _chain_expected():
    o = _oracle()
    dt, rt, at = _chain_taps()
    x = o.convert_u8(np.full(2 * CHAIN_TOTAL, 128, np.uint8))
    kd = (CHAIN_TOTAL - 128) // 8 + 1
    y = o.fm_demod(o.decimate_rc(4, kd, 8, duplicate(np.concatenate([dt, np.zeros(1, np.float32)])), x))
    nz = (kd * 3 - 192) // 10 + 1
    z, _ = o.resample_rr(8, nz, o.prepare_coeffs(8, 3, 10, rt), 0, y)
    return _frozen(o.scale(GAIN, o.filter_sym_rr(8, nz - 127, at, z)))


# ---- the CPU side ------------------------------------------------------------------------------------------------------------------
def test_inputs_on_the_cpu(oracle):
    from oracle.oracle import Ref, have_ref
    ref = Ref() if have_ref() else None
    for name, (kind, taps) in K2_CASES.items():
        n0 = _neg_zero_count(_k2_first_products(name))
        exp = _k2_expected(name)
        print(f"K2, {name}: {n0} first products are -0")
        assert n0 >= 1, f"K2, {name}: no -0 first product"
        assert _neg_zero_count(exp) == 0, f"K2, {name}: the oracle's output holds -0"
        if kind == "silence":
            assert not exp.view(np.uint32).any(), "all-128 input: every output is +0.0"
        if ref is not None:
            h = np.concatenate([taps(), np.zeros(1, np.float32)])
            assert_bit_equal(ref.decim("decimateAVXRC", K2_K, 8, duplicate(h), oracle.convert_u8(_k2_raw(kind)), True), exp, f"K2, {name}: reference build")
    for name in K5_CASES:
        n0 = _neg_zero_count(_k5_first_products(name))
        exp = _k5_expected(name)
        print(f"K5, {name}: {n0} first products are -0")
        assert n0 >= 1, f"K5, {name}: no -0 first product"
        assert _neg_zero_count(exp) == 0, f"K5, {name}: the oracle's output holds -0"
        if ref is not None:
            assert_bit_equal(ref.filt("filterAVXSymmetricRR", K5_K, _half_neg8(), _k5_input(name)), exp, f"K5, {name}: reference build")
    for name, (kind, _) in K4_CASES.items():
        for start in K4_STARTS:
            n0 = _neg_zero_count(_k4_first_products(name, start))
            exp = _k4_expected(name, start)
            print(f"K4, {name}, first output {start}: {n0} first products are -0")
            assert n0 >= 1, f"K4, {name}, first output {start}: no -0 first product"
            assert _neg_zero_count(exp) == 0, f"K4, {name}: the oracle's output holds -0"
            if ref is not None:
                got, _ = ref.resample("resampleAVXRR", K4_K, _k4_prep(name), start % 3, _k4_input(kind)[_k4_offset(start):])
                assert_bit_equal(got, exp, f"K4, {name}, first output {start}: reference build")
    exp = _chain_expected()
    assert exp.size >= K5_K and not exp.view(np.uint32).any(), "the chain on silence: every audio sample is +0.0"


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------
def _same_bits(got, exp, what):
    a, b = np.ascontiguousarray(got, np.float32).view(np.int32), np.ascontiguousarray(exp, np.float32).view(np.int32)
    assert a.shape == b.shape, what
    bad = np.nonzero(a != b)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} differ, first at {int(bad[0])}: {int(a[bad[0]]):#x} vs {int(b[bad[0]]):#x}"


@gpu
@pytest.mark.parametrize("name", list(K2_CASES))
def test_systolic_decimator(hip, oracle, name):
    import gpu_util as G
    kind, taps = K2_CASES[name]
    exp = _k2_expected(name)
    dec = hip.Decimator(8, taps(), hip.ORDER_AVX, complex_=True)
    d_in = G.to_dev(_k2_raw(kind))
    out = G.dev_empty_f32(2 * K2_K)
    hip.lib.sdrhip_debug_set_systolic(1)
    try:
        before = hip.lib.sdrhip_debug_systolic_launches()
        dec.run_u8(G.ptr(d_in), 0, G.ptr(out), 0, K2_K, 0)
        got = G.to_host(out)
        assert hip.lib.sdrhip_debug_systolic_launches() == before + 1, "the systolic kernel did not take the launch"
    finally:
        hip.lib.sdrhip_debug_set_systolic(2)
    _same_bits(got, exp, f"systolic decimator, {name}")
    if kind == "silence":
        assert not got.view(np.uint32).any(), "all-128 input: every output must be +0.0 (0x00000000)"


@gpu
@pytest.mark.parametrize("name", K5_CASES)
def test_fast_real_filter(hip, oracle, name):
    import gpu_util as G
    f = hip.Filter(_half_neg8(), hip.ORDER_AVX, sym=True)
    out = G.dev_empty_f32(K5_K)
    before = hip.lib.sdrhip_debug_tiled_launches()
    f.run(G.ptr(G.to_dev(_k5_input(name))), 0, G.ptr(out), 0, K5_K, 0)
    got = G.to_host(out)
    assert hip.lib.sdrhip_debug_tiled_launches() == before, "the general tiled kernel took the launch"
    _same_bits(got, _k5_expected(name), f"symmetric filter, {name}")


@gpu
@pytest.mark.parametrize("start", K4_STARTS)
@pytest.mark.parametrize("name", list(K4_CASES))
def test_resampler_tile_kernel(hip, oracle, name, start):
    import gpu_util as G
    kind, taps = K4_CASES[name]
    r = hip.Resampler(3, 10, taps(), hip.ORDER_AVX)
    assert r.group(start) == start % 3 and r.in_offset(start) == _k4_offset(start)
    out = G.dev_empty_f32(K4_K)
    before = (hip.lib.sdrhip_debug_tiled_launches(), hip.lib.sdrhip_debug_resample_cycle_launches())
    r.run(G.ptr(G.to_dev(_k4_input(kind))), 0, G.ptr(out), start, start + K4_K, 0)
    got = G.to_host(out)
    assert (hip.lib.sdrhip_debug_tiled_launches(), hip.lib.sdrhip_debug_resample_cycle_launches()) == before, "not the 3/10 tile kernel"
    _same_bits(got, _k4_expected(name, start), f"resampler, {name}, first output {start}")


@gpu
def test_chain_stage_route_on_silence(hip, oracle):
    """The filter kernel with its fused gain runs only inside the chain: all-128 input, negative first taps in all three filters,
    the stage kernels.  Every audio sample is +0.0."""
    import torch
    import gpu_util as G
    exp = _chain_expected()
    dt, rt, at = _chain_taps()
    ch = hip.FmChain(8, dt, 3, 10, rt, at, GAIN, 0)
    q0, q1, _ = ch.plan(0, CHAIN_TOTAL, CHAIN_TOTAL)
    assert (q0, q1) == (0, exp.size)
    ch.set_small_chain(0)
    ch.set_fused_tail(0)
    wsb = ch.workspace_bytes(CHAIN_TOTAL)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = G.dev_empty_f32(q1)
    n0 = hip.lib.sdrhip_debug_small_chain_launches()
    ch.run(G.ptr(G.to_dev(np.full(2 * CHAIN_TOTAL, 128, np.uint8))), 0, CHAIN_TOTAL, G.ptr(out), 0, q1, G.ptr(ws), wsb)
    got = G.to_host(out)
    assert hip.lib.sdrhip_debug_small_chain_launches() == n0, "the one-kernel route took the run"
    _same_bits(got, exp, "chain on silence, stage route")
    assert not got.view(np.uint32).any()
