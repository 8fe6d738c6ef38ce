"""The AM bank (sdrhip_am_bank_*) on a host without a GPU: the names are declared, exported and bound; create, destroy and the getters
work without a device; every refusal returns SDRHIP_ERR_ARG with its function named in sdrhip_last_error before any device work.
What a bank COMPUTES is held to the models and to the composed calls on the device (tests/test_gpu_am_bank.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_model as TM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_am_bank_create", "sdrhip_am_bank_destroy", "sdrhip_am_bank_channels", "sdrhip_am_bank_set_route",
               "sdrhip_am_bank_workspace_bytes", "sdrhip_am_bank_run", "sdrhip_am_bank_run_u8", "sdrhip_am_bank_run_i16",
               "sdrhip_debug_am_bank_launches", "sdrhip_debug_am_bank_fixup_launches"]
A16 = 0x10000                                                    # a 16-byte aligned address that is never dereferenced


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _tables():
    return [TM.shift_table(1, 4), TM.shift_table(-3, 1000), np.array([1.0, 0.0], np.float32)]


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_am_bank_launches.restype is C.c_longlong and L.lib.sdrhip_am_bank_workspace_bytes.restype is C.c_size_t
    assert L.am_bank_launches() >= 0 and L.am_bank_fixup_launches() >= 0


def test_create_destroy_and_getters_without_a_device(L):
    tb = L.TunerBank(8, S.taps_decim127(), _tables())
    for dc in (True, False):
        am = L.AmBank(tb, dc_block=dc)
        assert am.channels == 3 and am.dc_block is dc
    L.lib.sdrhip_am_bank_destroy(None)                           # harmless
    assert L.lib.sdrhip_am_bank_channels(None) == ERR_ARG

    def refused(what, *args):
        h = C.c_void_p(0xdead)                                   # a refused create must overwrite it with null
        assert L.lib.sdrhip_am_bank_create(C.byref(h), *args) == ERR_ARG, what
        assert not h.value, what + ": a refused create must leave *b null"
        assert b"sdrhip_am_bank_create" in L.lib.sdrhip_last_error(), what

    refused("a null bank", None, 1)
    for bad in (-1, 2, 7):
        refused(f"dc_block {bad}", tb.h, bad)
    assert L.lib.sdrhip_am_bank_create(None, tb.h, 1) == ERR_ARG and b"sdrhip_am_bank_create" in L.lib.sdrhip_last_error()


def test_workspace_bytes(L):
    tb = L.TunerBank(8, S.taps_decim127(), _tables())
    on, off = L.AmBank(tb, True), L.AmBank(tb, False)
    assert L.lib.sdrhip_am_bank_workspace_bytes(None, 100) == 0
    for bad in (0, -1, 2 ** 31 - 1):
        assert on.workspace_bytes(bad) == 0
    for n in (1, 511, 512, 5105):
        rows = 3 * 4 * ((n + 3) // 4 * 4)
        # the complex rows; with dc_block the envelope rows and dcBlocker's own workspace behind them
        assert off.workspace_bytes(n) == 2 * rows
        assert on.workspace_bytes(n) == 3 * rows + L.lib.sdrhip_dc_blocker_rows_workspace_bytes(3, n)


def test_routes_and_host_side_run_errors(L):
    tb = L.TunerBank(8, S.taps_decim127(), _tables())
    am = L.AmBank(tb, True)
    plain = L.AmBank(tb, False)
    assert L.lib.sdrhip_am_bank_set_route(None, 0) == ERR_ARG
    for bad in (3, -1):
        assert L.lib.sdrhip_am_bank_set_route(am.h, bad) == ERR_ARG
        assert b"sdrhip_am_bank_set_route" in L.lib.sdrhip_last_error()
    n = 100
    ws = am.workspace_bytes(n)
    # refused before any device work: no pointer is dereferenced (the addresses below are made up)
    for run in (L.lib.sdrhip_am_bank_run, L.lib.sdrhip_am_bank_run_u8, L.lib.sdrhip_am_bank_run_i16):
        for route in (1, 2, 0):
            am.set_route(route)
            plain.set_route(route)

            def refused(what, *args):
                assert run(*args) == ERR_ARG, f"route {route}: {what}"
                assert b"sdrhip_am_bank_run" in L.lib.sdrhip_last_error(), what

            refused("null bank", None, None, A16, 0, A16, n, 0, n, 0, A16, A16, ws)
            refused("out_stride < k_end - k_begin", am.h, None, A16, 0, A16, n - 1, 0, n, 0, A16, A16, ws)
            refused("k_end < k_begin", am.h, None, A16, 0, A16, n, n, 0, 0, A16, A16, ws)
            refused("negative k_begin", am.h, None, A16, 0, A16, n, -1, n - 1, 0, A16, A16, ws)
            refused("a window before d_in", am.h, None, A16, 8, A16, n, 0, n, 0, A16, A16, ws)
            refused("a seam block shorter than the filter", am.h, None, A16, 0, A16, n, 0, n, 127, A16, A16, ws)
            refused("a null state with dc_block", am.h, None, A16, 0, A16, n, 0, n, 0, None, A16, ws)
            refused("a state without dc_block", plain.h, None, A16, 0, A16, n, 0, n, 0, A16, A16, ws)
            refused("null input", am.h, None, None, 0, A16, n, 0, n, 0, A16, A16, ws)
            refused("null output", am.h, None, A16, 0, None, n, 0, n, 0, A16, A16, ws)
            refused("an output off a float's alignment", am.h, None, A16, 0, A16 + 2, n, 0, n, 0, A16, A16, ws)
            need = ws if route != 1 else ws - 3 * 2 * 4 * n     # route 1 asks for no complex rows
            refused("a workspace one byte short", am.h, None, A16, 0, A16, n, 0, n, 0, A16, A16, need - 1)
            refused("a null workspace", am.h, None, A16, 0, A16, n, 0, n, 0, A16, None, ws)
            refused("a workspace off 16 bytes", am.h, None, A16, 0, A16, n, 0, n, 0, A16, A16 + 8, ws)
            if route != 1:
                refused("a workspace one byte short without dc_block", plain.h, None, A16, 0, A16, n, 0, n, 0, None, A16,
                        plain.workspace_bytes(n) - 1)
            assert run(am.h, None, None, 0, None, 0, 7, 7, 0, A16, None, 0) == 0        # no outputs: nothing to do
        # route 1 forced on a shape the banked launch refuses: every output Cross, an input 8 bytes off 16
        am.set_route(1)
        for what, d_in, seam in (("seam_block -1", A16, -1), ("a first window off 16 bytes", A16 + 8, 0)):
            if run is L.lib.sdrhip_am_bank_run_i16 and d_in != A16:
                d_in = A16 + 4
            assert run(am.h, None, d_in, 0, A16, n, 0, n, seam, A16, A16, ws) == ERR_ARG, what
            assert b"sdrhip_am_bank_run: the fused route" in L.lib.sdrhip_last_error(), what
    # int16 IQ off its 4-byte samples
    am.set_route(0)
    assert L.lib.sdrhip_am_bank_run_i16(am.h, None, A16 + 2, 0, A16, n, 0, n, 0, A16, A16, ws) == ERR_ARG
    assert b"int16" in L.lib.sdrhip_last_error()
    # a shape the banked launch never serves (factor 5): route 1 refuses whatever the pointers are
    other = L.AmBank(L.TunerBank(5, S.taps_decim127(), _tables()[:2], L.ORDER_SSE), False)
    other.set_route(1)
    assert L.lib.sdrhip_am_bank_run(other.h, None, A16, 0, A16, n, 0, n, 0, None, None, 0) == ERR_ARG
    assert b"sdrhip_am_bank_run: the fused route" in L.lib.sdrhip_last_error()
    # one channel has no second row to overlap: any stride passes and the call stops at the null pointers
    one = L.AmBank(L.TunerBank(8, S.taps_decim127(), _tables()[:1]), False)
    assert L.lib.sdrhip_am_bank_run(one.h, None, None, 0, None, 3, 0, n, 0, None, None, 0) == ERR_ARG
    assert b"d_in != nullptr" in L.lib.sdrhip_last_error()
