"""The narrow-band FM bank (sdrhip_nfm_bank_*) on a host without a GPU: the names are declared, exported and bound; create, destroy
and the getters work without a device; every refusal returns SDRHIP_ERR_ARG with its function named in sdrhip_last_error before any
device work.  What a bank COMPUTES is held to the models and to the composed calls on the device (tests/test_gpu_nfm_bank.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_model as TM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_nfm_bank_create", "sdrhip_nfm_bank_destroy", "sdrhip_nfm_bank_channels", "sdrhip_nfm_bank_set_route",
               "sdrhip_nfm_bank_workspace_bytes", "sdrhip_nfm_bank_run", "sdrhip_nfm_bank_run_u8", "sdrhip_nfm_bank_run_i16",
               "sdrhip_debug_nfm_bank_launches", "sdrhip_debug_nfm_bank_cross_launches"]
A16 = 0x10000                                                    # a 16-byte aligned address that is never dereferenced
S0, S1 = 0x20000, 0x20000 + 24                                   # two state arrays of 3 pairs, back to back


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
    assert L.lib.sdrhip_debug_nfm_bank_launches.restype is C.c_longlong and L.lib.sdrhip_nfm_bank_workspace_bytes.restype is C.c_size_t
    assert L.nfm_bank_launches() >= 0 and L.nfm_bank_cross_launches() >= 0


def test_create_destroy_and_getters_without_a_device(L):
    tb = L.TunerBank(8, S.taps_decim127(), _tables())
    nb = L.NfmBank(tb)
    assert nb.channels == 3
    L.lib.sdrhip_nfm_bank_destroy(None)                          # harmless
    assert L.lib.sdrhip_nfm_bank_channels(None) == ERR_ARG
    h = C.c_void_p(0xdead)                                       # a refused create must overwrite it with null
    assert L.lib.sdrhip_nfm_bank_create(C.byref(h), None) == ERR_ARG and not h.value
    assert b"sdrhip_nfm_bank_create" in L.lib.sdrhip_last_error()
    assert L.lib.sdrhip_nfm_bank_create(None, tb.h) == ERR_ARG and b"sdrhip_nfm_bank_create" in L.lib.sdrhip_last_error()


def test_workspace_bytes(L):
    nb = L.NfmBank(L.TunerBank(8, S.taps_decim127(), _tables()))
    assert L.lib.sdrhip_nfm_bank_workspace_bytes(None, 100) == 0
    for bad in (0, -1, 2 ** 31 - 1):
        assert nb.workspace_bytes(bad) == 0
    for n in (1, 511, 512, 5105):
        assert nb.workspace_bytes(n) == 3 * 2 * 4 * ((n + 3) // 4 * 4)       # the complex rows, each 16-byte aligned


def test_routes_and_host_side_run_errors(L):
    nb = L.NfmBank(L.TunerBank(8, S.taps_decim127(), _tables()))
    assert L.lib.sdrhip_nfm_bank_set_route(None, 0) == ERR_ARG
    for bad in (3, -1):
        assert L.lib.sdrhip_nfm_bank_set_route(nb.h, bad) == ERR_ARG
        assert b"sdrhip_nfm_bank_set_route" in L.lib.sdrhip_last_error()
    n = 100
    ws = nb.workspace_bytes(n)
    # refused before any device work: no pointer is dereferenced (the addresses below are made up)
    for run in (L.lib.sdrhip_nfm_bank_run, L.lib.sdrhip_nfm_bank_run_u8, L.lib.sdrhip_nfm_bank_run_i16):
        for route in (1, 2, 0):
            nb.set_route(route)

            def refused(what, *args):
                assert run(*args) == ERR_ARG, f"route {route}: {what}"
                assert b"sdrhip_nfm_bank_run" in L.lib.sdrhip_last_error(), what

            refused("null bank", None, None, A16, 0, A16, n, 0, n, 0, S0, S1, A16, ws)
            refused("out_stride < k_end - k_begin", nb.h, None, A16, 0, A16, n - 1, 0, n, 0, S0, S1, A16, ws)
            refused("k_end < k_begin", nb.h, None, A16, 0, A16, n, n, 0, 0, S0, S1, A16, ws)
            refused("negative k_begin", nb.h, None, A16, 0, A16, n, -1, n - 1, 0, S0, S1, A16, ws)
            refused("a window before d_in", nb.h, None, A16, 8, A16, n, 0, n, 0, S0, S1, A16, ws)
            refused("a seam block shorter than the filter", nb.h, None, A16, 0, A16, n, 0, n, 127, S0, S1, A16, ws)
            refused("null input", nb.h, None, None, 0, A16, n, 0, n, 0, S0, S1, A16, ws)
            refused("null output", nb.h, None, A16, 0, None, n, 0, n, 0, S0, S1, A16, ws)
            refused("an output off a float's alignment", nb.h, None, A16, 0, A16 + 2, n, 0, n, 0, S0, S1, A16, ws)
            for what, a, b in (("the same array", S0, S0), ("one pair apart", S0, S0 + 8), ("d_final in front, overlapping", S0 + 20, S0),
                               ("the last float shared", S0, S0 + 20)):
                refused("overlapping state arrays: " + what, nb.h, None, A16, 0, A16, n, 0, n, 0, a, b, A16, ws)
            refused("overlapping state arrays on an empty range", nb.h, None, A16, 0, A16, n, 7, 7, 0, S0, S0, A16, ws)
            if route != 1:
                refused("a workspace one byte short", nb.h, None, A16, 0, A16, n, 0, n, 0, S0, S1, A16, ws - 1)
                refused("a null workspace", nb.h, None, A16, 0, A16, n, 0, n, 0, S0, S1, None, ws)
                refused("a workspace off 16 bytes", nb.h, None, A16, 0, A16, n, 0, n, 0, S0, S1, A16 + 8, ws)
            assert run(nb.h, None, None, 0, None, 0, 7, 7, 0, None, None, None, 0) == 0        # no outputs, no d_final: nothing to do
        # route 1 forced on a shape the fused launch refuses: every output Cross, a seam of 2^30, an input 8 bytes off 16
        nb.set_route(1)
        for what, d_in, seam in (("seam_block -1", A16, -1), ("seam_block 2^30", A16, 1 << 30), ("a first window off 16 bytes", A16 + 8, 0)):
            if run is L.lib.sdrhip_nfm_bank_run_i16 and d_in != A16:
                d_in = A16 + 4
            assert run(nb.h, None, d_in, 0, A16, n, 0, n, seam, S0, S1, None, 0) == ERR_ARG, what
            assert b"sdrhip_nfm_bank_run: the fused route" in L.lib.sdrhip_last_error(), what
    # int16 IQ off its 4-byte samples
    nb.set_route(0)
    assert L.lib.sdrhip_nfm_bank_run_i16(nb.h, None, A16 + 2, 0, A16, n, 0, n, 0, S0, S1, A16, ws) == ERR_ARG
    assert b"int16" in L.lib.sdrhip_last_error()
    # a shape the fused launch never serves (factor 5): route 1 refuses whatever the pointers are
    other = L.NfmBank(L.TunerBank(5, S.taps_decim127(), _tables()[:2], L.ORDER_SSE))
    other.set_route(1)
    assert L.lib.sdrhip_nfm_bank_run(other.h, None, A16, 0, A16, n, 0, n, 0, None, None, None, 0) == ERR_ARG
    assert b"sdrhip_nfm_bank_run: the fused route" in L.lib.sdrhip_last_error()
    # one channel has no second row to overlap: any stride passes and the call stops at the null pointers
    one = L.NfmBank(L.TunerBank(8, S.taps_decim127(), _tables()[:1]))
    assert L.lib.sdrhip_nfm_bank_run(one.h, None, None, 0, None, 3, 0, n, 0, None, None, None, 0) == ERR_ARG
    assert b"d_in != nullptr" in L.lib.sdrhip_last_error()
