"""The receiver bank (sdrhip_fm_bank_*) on a host without a GPU: the names are declared, exported and bound; create refuses every
bad argument before any device work; planning and sizing are the tuned chain's of the same arguments.  What a bank COMPUTES is
held to tuned chains on the device (tests/test_gpu_fm_bank.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_model as TM

B = 8192
ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_fm_bank_create", "sdrhip_fm_bank_destroy", "sdrhip_fm_bank_stations", "sdrhip_fm_bank_period", "sdrhip_fm_bank_plan",
               "sdrhip_fm_bank_ready", "sdrhip_fm_bank_max_halo", "sdrhip_fm_bank_workspace_bytes", "sdrhip_fm_bank_run",
               "sdrhip_fm_bank_set_route", "sdrhip_debug_fm_bank_launches"]


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _tables():
    return [TM.shift_table(1, 4), TM.shift_table(-3, 1000), np.array([1.0, 0.0], np.float32)]


def _bank(L, tables=None, block=B):
    return L.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), _tables() if tables is None else tables, 0.2, block)


def _tuned_chain(L, osc, block=B):
    ch = L.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, block)
    ch.set_tuner(osc)
    return ch


def _create(L, tables, periods=None, stations=None, handle=True, null_tables=False, null_periods=False):
    """sdrhip_fm_bank_create by hand -> (rc, handle).  tables: arrays or None (a null table pointer)."""
    a, b, c = S.taps_decim127(), S.taps_resamp191(), S.taps_audio_half64()
    n = max(len(tables), 1)
    ptrs = (C.POINTER(C.c_float) * n)(*[_fp(t) if t is not None else C.POINTER(C.c_float)() for t in tables])
    per = (C.c_int * n)(*(periods if periods is not None else [0 if t is None else t.size // 2 for t in tables]))
    h = C.c_void_p()
    rc = L.lib.sdrhip_fm_bank_create(C.byref(h) if handle else None, L.ORDER_AVX, 8, _fp(a), a.size, 3, 10, _fp(b), b.size, _fp(c), c.size,
                                     C.c_float(0.2), B, len(tables) if stations is None else stations,
                                     None if null_tables else ptrs, None if null_periods else per)
    return rc, h


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_fm_bank_launches.restype is C.c_longlong
    assert L.fm_bank_launches() >= 0
    header = open(os.path.join(os.path.dirname(L.HERE), "include", "sdr_hip.h")).read()
    assert "#define SDRHIP_FM_BANK_MAX_STATIONS 32" in header
    hs = open(os.path.join(os.path.dirname(L.HERE), "haskell", "SDR", "GPU.hs")).read()
    for n in NEW_SYMBOLS:
        assert f'"{n}"' in hs, f"haskell/SDR/GPU.hs does not import {n}"


def test_create_refuses_bad_arguments(L):
    ok = _tables()

    def refused(what, *args, **kw):
        rc, h = _create(L, *args, **kw)
        assert rc == ERR_ARG, what
        assert not h.value, what + ": a refused create must hand out no bank"
        assert b"sdrhip_fm_bank_create" in L.lib.sdrhip_last_error(), what

    rc, h = _create(L, ok)
    assert rc == 0 and h.value
    L.lib.sdrhip_fm_bank_destroy(h)
    refused("no stations", [], stations=0)
    refused("a negative count", ok, stations=-1)
    one = TM.shift_table(1, 4)
    refused("33 stations", [one] * 33)
    rc, h = _create(L, [one] * 32)                              # ... and 32 are a bank
    assert rc == 0
    L.lib.sdrhip_fm_bank_destroy(h)
    refused("a null table pointer", [ok[0], None, ok[2]], periods=[4, 4, 1])
    refused("a null table array", ok, null_tables=True)
    refused("a null period array", ok, null_periods=True)
    for bad in (0, -1, 65537):
        refused(f"period {bad}", ok, periods=[4, bad, 1])
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 3, 1999):
            t = ok[1].copy()
            t[at] = bad
            refused(f"{bad} at {at}", [ok[0], t, ok[2]])
    rc, _ = _create(L, ok, handle=False)
    assert rc == ERR_ARG and b"sdrhip_fm_bank_create" in L.lib.sdrhip_last_error()
    big = np.zeros(2 * 65536, np.float32)                       # the longest table
    rc, h = _create(L, [big])
    assert rc == 0
    assert L.lib.sdrhip_fm_bank_period(h, 0) == 65536
    L.lib.sdrhip_fm_bank_destroy(h)
    with pytest.raises(L.SdrHipError):
        _bank(L, [np.zeros(3, np.float32)])                     # not whole pairs


def test_chain_arguments_are_the_chains(L):
    """Chain arguments exactly as sdrhip_fm_chain_create: what a chain refuses, a bank refuses (a block shorter than a stage's
    filter, test_abi.py::test_chain_planning_on_the_host), and the smallest block a chain takes, a bank takes."""
    with pytest.raises(L.SdrHipError):
        _tuned_chain(L, _tables()[0], block=100)
    with pytest.raises(L.SdrHipError):
        _bank(L, block=100)
    assert _bank(L, block=128).stations() == 3 and _bank(L, block=0).stations() == 3
    with pytest.raises(L.SdrHipError):
        L.FmBank(8, S.taps_decim127(), 10, 3, S.taps_resamp191(), S.taps_audio_half64(), _tables())


def test_stations_and_periods(L):
    bank = _bank(L)
    assert bank.stations() == 3
    assert [bank.period(j) for j in range(3)] == [4, 1000, 1]
    for j in (-1, 3):
        assert L.lib.sdrhip_fm_bank_period(bank.h, j) == ERR_ARG
    assert L.lib.sdrhip_fm_bank_stations(None) == ERR_ARG and L.lib.sdrhip_fm_bank_period(None, 0) == ERR_ARG
    # the tables were copied: the caller's arrays may go
    t = [x.copy() for x in _tables()]
    bank = _bank(L, t)
    for x in t:
        x[:] = np.nan
    del t
    assert [bank.period(j) for j in range(3)] == [4, 1000, 1]


def test_planning_and_sizes_are_the_tuned_chains(L):
    total = 100 * B
    for block in (B, 0):
        bank = _bank(L, block=block)
        ch = _tuned_chain(L, _tables()[1], block)
        for s0, s1, tot in ((0, total, total), (0, total, -1), (5 * B, 9 * B, total), (8 * 4321, 8 * 9876, total), (total, total, total),
                            (2 ** 33 + 8, 2 ** 33 + 6 * B, 2 ** 33 + 6 * B)):
            assert bank.plan(s0, s1, tot) == ch.plan(s0, s1, tot), (s0, s1, tot)
        for n in (0, 127, 5000, B, 20 * B, 1 << 20, 2 ** 33):
            assert bank.ready(n) == ch.ready(n), n
        assert bank.max_halo() == ch.max_halo() and 3000 < bank.max_halo() < 5000
        for n in (0, B, 20 * B, 1 << 20, 1 << 27):
            assert bank.workspace_bytes(n) == int(ch.workspace_bytes(n)) > 0, n
        assert bank.workspace_bytes(-1) == 0
    assert L.lib.sdrhip_fm_bank_ready(None, B) == -1 and L.lib.sdrhip_fm_bank_max_halo(None) == -1
    assert L.lib.sdrhip_fm_bank_workspace_bytes(None, B) == 0
    q = C.c_int64()
    assert L.lib.sdrhip_fm_bank_plan(None, 0, B, B, C.byref(q), C.byref(q), C.byref(q)) == ERR_ARG


def test_null_handles_and_host_side_run_errors(L):
    L.lib.sdrhip_fm_bank_destroy(None)                          # harmless
    bank = _bank(L)
    assert L.lib.sdrhip_fm_bank_set_route(None, 0, 0, 0) == ERR_ARG
    for bad in ((3, 0, 0), (-1, 0, 0), (0, -1, 0), (0, 0, -1)):
        assert L.lib.sdrhip_fm_bank_set_route(bank.h, *bad) == ERR_ARG, bad
    bank.set_route(1, 1000, 96)
    bank.set_route()
    # refused before any device work: no pointer is looked at
    assert L.lib.sdrhip_fm_bank_run(None, None, None, 0, B, None, 100, 0, 100, None, 0) == ERR_ARG
    assert b"sdrhip_fm_bank_run" in L.lib.sdrhip_last_error()
    assert L.lib.sdrhip_fm_bank_run(bank.h, None, None, 0, B, None, 99, 0, 100, None, 0) == ERR_ARG      # audio_stride < q1 - q0
    assert b"sdrhip_fm_bank_run" in L.lib.sdrhip_last_error()
    assert L.lib.sdrhip_fm_bank_run(bank.h, None, None, 0, B, None, 100, 100, 0, None, 0) == ERR_ARG     # q1 < q0
    assert L.lib.sdrhip_fm_bank_run(bank.h, None, None, 0, B, None, 0, 7, 7, None, 0) == 0               # no outputs: nothing to do
