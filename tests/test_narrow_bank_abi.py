"""The narrow-channel bank (sdrhip_narrow_bank_*) on a host without a GPU: the names are declared, exported and bound; create, destroy,
the getters, stage1_range and workspace_bytes work without a device; every refusal returns SDRHIP_ERR_ARG with its function named in
sdrhip_last_error before any device work.  What a bank COMPUTES is held to the models and to the composed calls on the device
(tests/test_gpu_narrow_bank.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import narrow_bank_cases as NB
import signals as S
import tuner_model as TM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_narrow_bank_create", "sdrhip_narrow_bank_destroy", "sdrhip_narrow_bank_channels", "sdrhip_narrow_bank_set_route",
               "sdrhip_narrow_bank_workspace_bytes", "sdrhip_narrow_bank_stage1_range", "sdrhip_narrow_bank_run", "sdrhip_narrow_bank_run_u8",
               "sdrhip_narrow_bank_run_i16", "sdrhip_debug_narrow_bank_launches", "sdrhip_debug_narrow_bank_tile", "sdrhip_pipe_narrow_bank"]
A16 = 0x10000                                                    # a 16-byte aligned address that is never dereferenced
S0, S1 = 0x20000, 0x20000 + 24                                   # two state arrays of 3 pairs, back to back
DC = 0x30000


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _tables():
    return [TM.shift_table(1, 4), TM.shift_table(-3, 1000), np.array([1.0, 0.0], np.float32)]


def _bank(L, shape="24/4", form=NB.FM, dc=False, order=None, nch=3):
    taps, d2, _ = NB.SHAPES[shape]
    tb = L.TunerBank(8, S.taps_decim127(), _tables()[:nch])
    dec = L.Decimator(d2, taps, L.ORDER_AVX if order is None else order, complex_=True)
    return L.NarrowBank(tb, dec, form, dc)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_narrow_bank_launches.restype is C.c_longlong and L.lib.sdrhip_narrow_bank_workspace_bytes.restype is C.c_size_t
    assert L.narrow_bank_launches() >= 0
    assert (L.NARROW_ENV, L.NARROW_FM) == (NB.ENV, NB.FM)
    assert L.narrow_bank_tile(L.NARROW_ENV) == NB.TILE and L.narrow_bank_tile(L.NARROW_FM) == NB.TILE - 1 and L.narrow_bank_tile(2) == 0


def test_create_refusals_and_getters_without_a_device(L):
    tb = L.TunerBank(8, S.taps_decim127(), _tables())
    taps, d2, _ = NB.SHAPES["61/5"]
    dec = L.Decimator(d2, taps, complex_=True)
    real = L.Decimator(d2, taps, complex_=False)
    for form, dc in ((L.NARROW_ENV, 0), (L.NARROW_ENV, 1), (L.NARROW_FM, 0)):
        nb = L.NarrowBank(tb, dec, form, dc)
        assert nb.channels == 3
    L.lib.sdrhip_narrow_bank_destroy(None)                       # harmless
    assert L.lib.sdrhip_narrow_bank_channels(None) == ERR_ARG
    for what, args in (("a null tuner bank", (None, dec.h, 0, 0)), ("a null decimator", (tb.h, None, 0, 0)),
                       ("a decimator on real data", (tb.h, real.h, 0, 0)), ("form 2", (tb.h, dec.h, 2, 0)), ("form -1", (tb.h, dec.h, -1, 0)),
                       ("dc_block 2", (tb.h, dec.h, 0, 2)), ("dc_block with fmDemod", (tb.h, dec.h, 1, 1))):
        h = C.c_void_p(0xdead)                                   # a refused create must overwrite it with null
        assert L.lib.sdrhip_narrow_bank_create(C.byref(h), *args) == ERR_ARG and not h.value, what
        assert b"sdrhip_narrow_bank_create" in L.lib.sdrhip_last_error(), what
    assert L.lib.sdrhip_narrow_bank_create(None, tb.h, dec.h, 0, 0) == ERR_ARG


def test_stage1_range(L):
    for shape, (_, d2, lp2) in NB.SHAPES.items():
        nb = _bank(L, shape)
        for k0, k1 in ((0, 1), (0, 0), (7, 7), (7, 9), (601, 1271), (3 * 2 ** 30 + 5, 3 * 2 ** 30 + 5 + 300)):
            assert nb.stage1_range(k0, k1) == NB.stage1_range(shape, k0, k1), (shape, k0, k1)
        j0, j1 = C.c_int64(0), C.c_int64(0)
        for bad in ((-1, 3), (5, 4), (0, 2 ** 31 - 1)):
            assert L.lib.sdrhip_narrow_bank_stage1_range(nb.h, *bad, C.byref(j0), C.byref(j1)) == ERR_ARG
            assert b"sdrhip_narrow_bank_stage1_range" in L.lib.sdrhip_last_error()
        assert L.lib.sdrhip_narrow_bank_stage1_range(None, 0, 1, C.byref(j0), C.byref(j1)) == ERR_ARG
        assert L.lib.sdrhip_narrow_bank_stage1_range(nb.h, 0, 1, None, C.byref(j1)) == ERR_ARG


def test_workspace_bytes(L):
    assert L.lib.sdrhip_narrow_bank_workspace_bytes(None, 100) == 0

    def r4(n):
        return (n + 3) // 4 * 4

    for shape, (_, d2, lp2) in NB.SHAPES.items():
        for form, dc in ((NB.ENV, False), (NB.ENV, True), (NB.FM, False)):
            nb = _bank(L, shape, form, dc)
            for bad in (0, -1, 2 ** 31 - 1, (2 ** 31 - 1) // d2 + 1):
                assert nb.workspace_bytes(bad) == 0, (shape, bad)
            for n in (1, 2, 255, 256, 257, 1271):
                n1 = (n - 1) * d2 + lp2
                dcb = 3 * 4 * r4(n) + L.lib.sdrhip_dc_blocker_rows_workspace_bytes(3, n) if dc else 0
                r1 = 3 * 2 * 4 * r4(n1) + dcb                          # the stage-1 complex rows, each 16-byte aligned
                r2 = r1 + 3 * 2 * 4 * r4(n)                            # ... and the stage-2 complex rows
                for route, want in ((1, r1), (2, r2), (0, r2)):
                    nb.set_route(route)
                    assert nb.workspace_bytes(n) == want, (shape, form, dc, n, route)
                assert 0 < r1 <= r2


def test_routes_and_host_side_run_errors(L):
    n = 100
    for form, dc in ((NB.FM, False), (NB.ENV, False), (NB.ENV, True)):
        nb = _bank(L, "24/4", form, dc)
        assert L.lib.sdrhip_narrow_bank_set_route(None, 0) == ERR_ARG
        for bad in (3, -1):
            assert L.lib.sdrhip_narrow_bank_set_route(nb.h, bad) == ERR_ARG
            assert b"sdrhip_narrow_bank_set_route" in L.lib.sdrhip_last_error()
        st = (S0, S1) if form == NB.FM else (None, None)
        dcs = DC if dc else None
        # refused before any device work: no pointer is dereferenced (the addresses are made up)
        for run in (L.lib.sdrhip_narrow_bank_run, L.lib.sdrhip_narrow_bank_run_u8, L.lib.sdrhip_narrow_bank_run_i16):
            for route in (1, 2, 0):
                nb.set_route(route)
                ws = nb.workspace_bytes(n)

                def refused(what, *args):
                    assert run(*args) == ERR_ARG, f"route {route}: {what}"
                    assert b"sdrhip_narrow_bank_run" in L.lib.sdrhip_last_error(), what

                refused("null bank", None, None, A16, 0, A16, n, 0, n, 0, 0, *st, dcs, A16, ws)
                refused("out_stride < k_end - k_begin", nb.h, None, A16, 0, A16, n - 1, 0, n, 0, 0, *st, dcs, A16, ws)
                refused("k_end < k_begin", nb.h, None, A16, 0, A16, n, n, 0, 0, 0, *st, dcs, A16, ws)
                refused("negative k_begin", nb.h, None, A16, 0, A16, n, -1, n - 1, 0, 0, *st, dcs, A16, ws)
                refused("a window before d_in", nb.h, None, A16, 8, A16, n, 0, n, 0, 0, *st, dcs, A16, ws)
                refused("a window before d_in, far", nb.h, None, A16, 601 * 4 * 8 + 8, A16, n, 601, 601 + n, 0, 0, *st, dcs, A16, ws)
                refused("seam_block shorter than the first filter", nb.h, None, A16, 0, A16, n, 0, n, 127, 0, *st, dcs, A16, ws)
                refused("seam_block2 shorter than the second filter", nb.h, None, A16, 0, A16, n, 0, n, 0, 23, *st, dcs, A16, ws)
                refused("seam_block2 of 1", nb.h, None, A16, 0, A16, n, 0, n, 8192, 1, *st, dcs, A16, ws)
                refused("a negative seam_block2", nb.h, None, A16, 0, A16, n, 0, n, 0, -1, *st, dcs, A16, ws)
                refused("null input", nb.h, None, None, 0, A16, n, 0, n, 0, 0, *st, dcs, A16, ws)
                refused("null output", nb.h, None, A16, 0, None, n, 0, n, 0, 0, *st, dcs, A16, ws)
                refused("an output off a float's alignment", nb.h, None, A16, 0, A16 + 2, n, 0, n, 0, 0, *st, dcs, A16, ws)
                refused("a workspace one byte short", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, *st, dcs, A16, ws - 1)
                refused("a null workspace", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, *st, dcs, None, ws)
                refused("a workspace off 16 bytes", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, *st, dcs, A16 + 8, ws)
                refused("a run whose stage-1 range passes 2^31 - 2 outputs", nb.h, None, A16, 0, A16, 2 ** 31, 0, 2 ** 30, 0, 0, *st, dcs, A16,
                        2 ** 40)
                if form == NB.FM:
                    for what, a, b in (("the same array", S0, S0), ("one pair apart", S0, S0 + 8), ("d_final in front, overlapping", S0 + 20, S0),
                                       ("the last float shared", S0, S0 + 20)):
                        refused("overlapping state arrays: " + what, nb.h, None, A16, 0, A16, n, 0, n, 0, 0, a, b, None, A16, ws)
                    refused("overlapping state arrays on an empty range", nb.h, None, A16, 0, A16, n, 7, 7, 0, 0, S0, S0, None, A16, ws)
                    refused("a dc state with fmDemod", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, S0, S1, DC, A16, ws)
                    refused("a state array off a float's alignment", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, S0 + 2, S1, None, A16, ws)
                else:
                    refused("d_state with the envelope form", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, S0, None, dcs, A16, ws)
                    refused("d_final with the envelope form", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, None, S1, dcs, A16, ws)
                    refused("the dc state does not match dc_block", nb.h, None, A16, 0, A16, n, 0, n, 0, 0, None, None, None if dc else DC, A16, ws)
                # an empty range with nothing to copy: no workspace, no pointers
                assert run(nb.h, None, None, 0, None, 0, 7, 7, 0, 0, None, None, dcs, None, 0) == 0
            # route 1 forced on a run the kernel does not serve
            nb.set_route(1)
            ws = nb.workspace_bytes(n)
            assert run(nb.h, None, A16, 0, A16, n, 0, n, 0, 1 << 30, *st, dcs, A16, ws) == ERR_ARG, "seam_block2 2^30"
            assert b"sdrhip_narrow_bank_run: the fused route" in L.lib.sdrhip_last_error()
        # the tuner bank forced onto ITS banked route on an input it does not fit: refused by the narrow bank's first call
        nb.set_route(2)
        nb.tuner_bank.set_route(1)
        ws = nb.workspace_bytes(n)
        assert L.lib.sdrhip_narrow_bank_run(nb.h, None, A16 + 8, 0, A16, n, 0, n, 0, 0, *st, dcs, A16, ws) == ERR_ARG
        assert b"sdrhip_tuner_bank_run" in L.lib.sdrhip_last_error()
    # int16 IQ off its 4-byte samples
    nb = _bank(L)
    ws = nb.workspace_bytes(n)
    assert L.lib.sdrhip_narrow_bank_run_i16(nb.h, None, A16 + 2, 0, A16, n, 0, n, 0, 0, S0, S1, None, A16, ws) == ERR_ARG
    assert b"int16" in L.lib.sdrhip_last_error()


def test_route_one_refuses_the_shapes_it_does_not_serve(L):
    """The SSE order, a factor above 16 and more than 128 prepared taps: SDRHIP_ERR_ARG on route 1, whatever the pointers are."""
    n = 40
    taps24 = NB.SHAPES["24/4"][0]
    long_taps = np.ones(132, np.float32)
    for what, dec in (("SSE order", L.Decimator(4, taps24, L.ORDER_SSE, complex_=True)), ("scalar order", L.Decimator(4, taps24, L.ORDER_SCALAR, complex_=True)),
                      ("factor 17", L.Decimator(17, taps24, complex_=True)), ("132 taps", L.Decimator(4, long_taps, complex_=True))):
        nb = L.NarrowBank(L.TunerBank(8, S.taps_decim127(), _tables()), dec, L.NARROW_ENV)
        nb.set_route(1)
        ws = max(nb.workspace_bytes(n), 16)
        assert L.lib.sdrhip_narrow_bank_run(nb.h, None, A16, 0, A16, n, 0, n, 0, 0, None, None, None, A16, ws) == ERR_ARG, what
        assert b"sdrhip_narrow_bank_run: the fused route" in L.lib.sdrhip_last_error(), what


def test_the_pipes_create_refusals_come_before_any_device_work(L):
    """sdrhip_pipe_narrow_bank: a null bank, a block_mid shorter than the second filter plus its factor (the reference's `assert
    "decimate 1"`), a block_size_out below 1 and an input type out of range are refused before the engine creates a stream."""
    nb = _bank(L, "61/5", NB.ENV, True)
    for what, args in (("a null bank", (None, 1024, 100, 0)), ("block_mid 68 < 64 + 5", (nb.h, 68, 100, 0)), ("block_size_out 0", (nb.h, 1024, 0, 0)),
                       ("input_type 3", (nb.h, 1024, 100, 3)), ("input_type -1", (nb.h, 1024, 100, -1))):
        h = C.c_void_p(0xdead)
        assert L.lib.sdrhip_pipe_narrow_bank(C.byref(h), *args) == ERR_ARG and not h.value, what
        assert b"sdrhip_pipe_narrow_bank" in L.lib.sdrhip_last_error(), what
    assert L.lib.sdrhip_pipe_narrow_bank(None, nb.h, 1024, 100, 0) == ERR_ARG
