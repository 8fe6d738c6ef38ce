"""The audio tail (sdrhip_audio_tail_*) on a host without a GPU: the names are declared, exported and bound; create refuses what
its two stages refuse; ready / first_input / max_halo are the FM chain's arithmetic without its decimator and fmDemod; every
refusal of run_rows comes back as SDRHIP_ERR_ARG under the function's own name before any pointer is looked at or any device work
is done (the pointers handed in here point nowhere, and there is no device); the route-1 fit edge lies where fm_tail_fused_fits puts
it.  What the tail COMPUTES is held to the restated Pipes on the device (tests/test_gpu_audio_tail.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import audio_tail_cases as AC
import signals as S

OK, ERR_ARG = 0, -1
NEW_SYMBOLS = ["sdrhip_audio_tail_create", "sdrhip_audio_tail_destroy", "sdrhip_audio_tail_ready", "sdrhip_audio_tail_first_input",
               "sdrhip_audio_tail_max_halo", "sdrhip_audio_tail_workspace_bytes", "sdrhip_audio_tail_run_rows", "sdrhip_audio_tail_set_route",
               "sdrhip_debug_audio_tail_launches", "sdrhip_audio_tail_block", "sdrhip_audio_tail_fused_fits"]
P = [0x10000, 0x20000, 0x30000]                          # never dereferenced: every call below is refused (or empty) first
NAME = b"sdrhip_audio_tail_run_rows"


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def fm_tail(L, block=8192, gain=0.5):
    return L.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), gain=gain, block=block)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.audio_tail_launches() >= 0
    for m in ("ready", "first_input", "workspace_bytes", "run_rows", "set_route", "max_halo"):
        assert callable(getattr(L.AudioTail, m))
    assert (L.AUDIO_TAIL_AUTO, L.AUDIO_TAIL_FUSED, L.AUDIO_TAIL_COMPOSED) == (0, 1, 2)


def test_create_destroy_and_what_create_refuses(L):
    t = fm_tail(L)
    assert t.h and L.lib.sdrhip_audio_tail_block(t.h) == 8192
    t.close()
    assert not t.h
    r, a = AC.resamp_taps(), AC.audio_half()
    h = C.c_void_p()

    def create(order=L.ORDER_AVX, I=3, D=10, nr=r.size, na=a.size, block=8192, out=C.byref(h)):
        return L.lib.sdrhip_audio_tail_create(out, order, I, D, L._fp(r), nr, L._fp(a), na, 1.0, block)
    assert create(out=None) == ERR_ARG
    assert create(block=-1) == ERR_ARG and not h
    assert create(order=7) == ERR_ARG and not h                       # what sdrhip_resampler_create refuses
    assert create(I=0) == ERR_ARG and create(D=0) == ERR_ARG and create(nr=0) == ERR_ARG
    assert create(na=0) == ERR_ARG and not h                          # what sdrhip_filter_sym_create refuses
    assert create(block=127) == ERR_ARG and not h                     # shorter than the audio filter (128)
    assert create(block=128) == OK and h
    L.lib.sdrhip_audio_tail_destroy(h)
    L.lib.sdrhip_audio_tail_destroy(None)
    # a block shorter than the resampler's filter: 31 taps at 3/10 in the SSE order are 36 prepared taps = 12 inputs; the filter 2 x 4 taps
    h = C.c_void_p()
    r31, a4 = S.taps_resamp31(), S.taps_audio_half32()[:4]
    assert L.lib.sdrhip_audio_tail_create(C.byref(h), L.ORDER_SSE, 3, 10, L._fp(r31), r31.size, L._fp(a4), 4, 1.0, 11) == ERR_ARG and not h
    assert L.lib.sdrhip_audio_tail_create(C.byref(h), L.ORDER_SSE, 3, 10, L._fp(r31), r31.size, L._fp(a4), 4, 1.0, 12) == OK
    L.lib.sdrhip_audio_tail_destroy(h)


def test_plan_functions_are_monotone_consistent_and_the_chains(L):
    t = fm_tail(L)
    # the chain with the same tail behind a decimator by Dd with Ld prepared taps: y index k is sample (k - 1) Dd + Ld
    for Dd, dtaps in ((8, S.taps_decim127()), (4, S.gauss_taps(64, 5))):
        chain = L.FmChain(Dd, dtaps, 3, 10, AC.resamp_taps(), AC.audio_half(), gain=0.5, block=8192)
        Ld = -(-dtaps.size // 4) * 4
        ready_t, ready_c = L.lib.sdrhip_audio_tail_ready, L.lib.sdrhip_fm_chain_ready
        for n_y in range(1, 100001):                               # every input count up to 10^5
            assert ready_t(t.h, n_y) == ready_c(chain.h, (n_y - 1) * Dd + Ld), (Dd, n_y)
        assert ready_t(t.h, 0) == 0 == ready_c(chain.h, 0)
        # first_input against the chain's plan: the first sample audio output q reads is decimator output first_input(q) - 1 (fmDemod
        # looks one back), so the outputs that start at or behind sample s are those from the first q with (first_input(q) - 1) Dd >= s
        for q in list(range(1, 400)) + [29999]:
            q0, q1, halo = chain.plan((t.first_input(q) - 1) * Dd, (t.first_input(q) - 1) * Dd + 1)
            assert q0 <= q and t.first_input(q0) == t.first_input(q), (Dd, q)
    assert t.ready(0) == 0 and t.ready(-1) == -1 and L.lib.sdrhip_audio_tail_ready(None, 5) == -1
    assert t.first_input(-1) == -1 and L.lib.sdrhip_audio_tail_first_input(None, 0) == -1
    assert L.lib.sdrhip_audio_tail_max_halo(None) == -1
    # against the table's own arithmetic, all of 0 .. 10^5 inputs: ready(n) = #{q : end_input(q) <= n}
    ends = np.array([AC.end_input(q) for q in range(30100)], np.int64)
    assert (np.diff(ends) >= 0).all()
    want = np.searchsorted(ends, np.arange(100001), side="right")
    got = np.array([t.ready(n_y) for n_y in range(0, 100001, 7)] + [t.ready(100000)])
    assert (got == np.concatenate([want[::7], want[-1:]])).all()
    assert (np.diff(got[:-1]) >= 0).all()
    span = t.max_halo()
    prev = -1
    for q in list(range(0, 3000)) + [10 ** 6, 3 * 2 ** 30 + 5]:
        f = t.first_input(q)
        assert f == -(-10 * q // 3) and f >= prev
        prev = f if q < 3000 else prev
        if q < 29000:
            assert f == AC.first_input(q) and t.ready(f + span) > q and t.ready(AC.end_input(q)) == q + 1 and t.ready(AC.end_input(q) - 1) <= q
    assert span == max(AC.end_input(q) - AC.first_input(q) for q in range(30)) == 424 + 64


def test_workspace_bytes(L):
    t = fm_tail(L)
    assert t.workspace_bytes(0, 1000) == 0 and t.workspace_bytes(1025, 1000) == 0 and t.workspace_bytes(1, -1) == 0
    assert L.lib.sdrhip_audio_tail_workspace_bytes(None, 1, 1000) == 0
    for rows in (1, 3, 32):
        prev = 0
        for n_y in (0, 488, 8192, 28000, 10 ** 6):
            b = t.workspace_bytes(rows, n_y)
            nz = max(0, (n_y * 3 - AC.RLP) // 10 + 1) if n_y * 3 >= AC.RLP else 0
            # room for every row's z outputs and filter outputs of any range inside n_y inputs, 16-byte aligned rows
            assert b >= rows * 4 * (-(-nz // 4) * 4 + max(nz - 127, 0)) and b % (16 * rows) == 0 and b >= prev
            assert b == rows * t.workspace_bytes(1, n_y) and b <= rows * 4 * (2 * (0.3 * n_y + 8))
            prev = b


def call(L, t, **kw):
    a = dict(d_y=P[0], y_stride=AC.N_Y, y_base=0, n_y=AC.N_Y, d_audio=P[1], audio_stride=AC.Q_MAX, rows=3, q0=0, q1=AC.Q_MAX,
             ws=P[2], ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = 1 << 30 if t is None else t.workspace_bytes(max(1, min(a["rows"], 1024)), a["n_y"])
    h = t.h if t is not None else None
    return L.lib.sdrhip_audio_tail_run_rows(h, None, a["d_y"], a["y_stride"], a["y_base"], a["n_y"], a["d_audio"], a["audio_stride"],
                                            a["rows"], a["q0"], a["q1"], a["ws"], a["ws_bytes"])


def refused(L, t, what, **kw):
    rc = call(L, t, **kw)
    assert rc == ERR_ARG, f"{what} is not refused (rc {rc})"
    assert NAME in L.lib.sdrhip_last_error(), f"{what}: {L.lib.sdrhip_last_error()!r}"


@pytest.mark.parametrize("route", [0, 1, 2])
def test_every_refusal_comes_before_any_pointer_is_looked_at(L, route):
    t = fm_tail(L)
    t.set_route(route)
    refused(L, None, "a null handle")
    for rows in (0, -1, 1025):
        refused(L, t, f"rows = {rows}", rows=rows)
    refused(L, t, "a receptive field that ends one sample behind the buffer", n_y=AC.N_Y - 1)
    refused(L, t, "a receptive field that starts before y_base", y_base=AC.first_input(5) + 1, q0=5, n_y=AC.N_Y)
    refused(L, t, "q1 < q0", q0=10, q1=9)
    refused(L, t, "a negative output", q0=-1)
    refused(L, t, "audio_stride one short", audio_stride=AC.Q_MAX - 1)
    refused(L, t, "y_stride shorter than the readable span", y_stride=AC.N_Y - 1)
    refused(L, t, "a negative stride", y_stride=-AC.N_Y)
    refused(L, t, "in place", d_audio=P[0])
    refused(L, t, "null d_y", d_y=None)
    refused(L, t, "null d_audio", d_audio=None)
    if route != 1:
        refused(L, t, "a null workspace", ws=None)
        refused(L, t, "a workspace one byte short", ws_bytes=t.workspace_bytes(3, AC.N_Y) - 1)
    # with one row the strides' lengths are not looked at; an empty range is fine and touches nothing, whatever else is passed
    assert call(L, t, rows=1, y_stride=0, audio_stride=0, q0=7, q1=7) == OK
    assert call(L, t, q0=7, q1=7, d_y=None, d_audio=None, ws=None, ws_bytes=0, n_y=0) == OK
    refused(L, t, "an empty range with rows = 0", q0=7, q1=7, rows=0)
    refused(L, None, "an empty range on a null handle", q0=7, q1=7)


def test_set_route_refuses_and_route_1_is_refused_where_it_does_not_fit(L):
    t = fm_tail(L)
    for route in (-1, 3):
        assert L.lib.sdrhip_audio_tail_set_route(t.h, route) == ERR_ARG
    assert L.lib.sdrhip_audio_tail_set_route(None, 1) == ERR_ARG
    # the fit edge, from the predicate (kernels_tail.hip fm_tail_fused_fits, restated in the case table)
    edge = AC.MIN_BLOCK
    assert AC.fused_fits(edge) and not AC.fused_fits(edge - 1)
    for block, fits in ((0, True), (edge, True), (edge - 1, False), (8192, True), (1024, False), (1 << 28, True), ((1 << 28) + 1, False)):
        tb = fm_tail(L, block=block)
        assert tb.fused_fits() == fits == AC.fused_fits(block), block
        tb.set_route(1)
        if fits:
            assert call(L, tb, q0=7, q1=7) == OK
        else:
            refused(L, tb, f"route 1 with block {block}")
            assert b"route 1" in L.lib.sdrhip_last_error()
            assert call(L, tb, q0=7, q1=7) == OK                # an empty range: nothing to route
    # another shape: 2/3 with 31 taps in the SSE order, 8 half-taps
    other = L.AudioTail(2, 3, S.taps_resamp31(), S.taps_audio_half32()[:8], gain=1.0, block=0, order=L.ORDER_SSE)
    assert not other.fused_fits()
    other.set_route(1)
    n_y = 4000
    q1 = other.ready(n_y)
    assert q1 > 2000
    rc = L.lib.sdrhip_audio_tail_run_rows(other.h, None, P[0], n_y, 0, n_y, P[1], q1, 3, 0, q1, None, 0)
    assert rc == ERR_ARG and b"route 1" in L.lib.sdrhip_last_error()
    # the AVX order with the FM taps but 32 half-taps is not the kernel's shape either
    assert not L.AudioTail(3, 10, AC.resamp_taps(), S.taps_audio_half32(), block=0).fused_fits()
    assert not L.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), block=0, order=L.ORDER_SSE).fused_fits()
