"""The tuner bank (sdrhip_tuner_bank_*) on a host without a GPU: the names are declared, exported and bound; create, destroy and the
getters work without a device; create refuses every bad argument under its own name and hands out no bank; the run refuses what it
can before any device work.  What a bank COMPUTES is held to the model and to tuners on the device (tests/test_gpu_tuner_bank.py);
that its expected outputs reach the cases they exist for is shown here from the model alone."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_bank_cases as BC
import tuner_model as TM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_tuner_bank_create", "sdrhip_tuner_bank_destroy", "sdrhip_tuner_bank_channels", "sdrhip_tuner_bank_period",
               "sdrhip_tuner_bank_num_coeffs", "sdrhip_tuner_bank_factor", "sdrhip_tuner_bank_run", "sdrhip_tuner_bank_run_u8",
               "sdrhip_tuner_bank_set_route", "sdrhip_debug_tuner_bank_launches"]


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


def _create(L, tables, periods=None, channels=None, handle=True, null_tables=False, null_periods=False, order=None, factor=8, taps=None):
    """sdrhip_tuner_bank_create by hand -> (rc, handle).  tables: arrays or None (a null table pointer)."""
    a = S.taps_decim127() if taps is None else taps
    n = max(len(tables), 1)
    ptrs = (C.POINTER(C.c_float) * n)(*[_fp(t) if t is not None else C.POINTER(C.c_float)() for t in tables])
    per = (C.c_int * n)(*(periods if periods is not None else [0 if t is None else t.size // 2 for t in tables]))
    h = C.c_void_p(0xdead)                                       # a refused create must overwrite it with null
    rc = L.lib.sdrhip_tuner_bank_create(C.byref(h) if handle else None, L.ORDER_AVX if order is None else order, factor,
                                        _fp(a) if a is not None else None, a.size if a is not None else 0,
                                        len(tables) if channels is None else channels,
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
    assert L.lib.sdrhip_debug_tuner_bank_launches.restype is C.c_longlong
    assert L.tuner_bank_launches() >= 0
    header = open(os.path.join(os.path.dirname(L.HERE), "include", "sdr_hip.h")).read()
    assert "#define SDRHIP_TUNER_BANK_MAX_CHANNELS 32" in header


def test_create_destroy_and_getters_without_a_device(L):
    bank = L.TunerBank(8, S.taps_decim127(), _tables())
    assert bank.channels == 3 and [bank.period(j) for j in range(3)] == [4, 1000, 1]
    assert (bank.factor, bank.num_coeffs) == (8, 128)
    for j in (-1, 3):
        assert L.lib.sdrhip_tuner_bank_period(bank.h, j) == ERR_ARG
        assert b"sdrhip_tuner_bank_period" in L.lib.sdrhip_last_error()
    for fn in ("channels", "num_coeffs", "factor"):
        assert getattr(L.lib, "sdrhip_tuner_bank_" + fn)(None) == ERR_ARG
    assert L.lib.sdrhip_tuner_bank_period(None, 0) == ERR_ARG
    L.lib.sdrhip_tuner_bank_destroy(None)                        # harmless
    # getters are the tuner's of the same arguments, for other shapes too
    for factor, taps, order in ((4, S.gauss_taps(52, 92), L.ORDER_AVX), (5, S.taps_decim127(), L.ORDER_SSE), (16, S.gauss_taps(31, 71), L.ORDER_SCALAR)):
        bank = L.TunerBank(factor, taps, _tables()[:2], order)
        t = L.Tuner(factor, taps, _tables()[0], order)
        assert (bank.factor, bank.num_coeffs, bank.channels) == (t.factor, t.num_coeffs, 2)
    # the tables were copied: the caller's arrays may go
    t = [x.copy() for x in _tables()]
    bank = L.TunerBank(8, S.taps_decim127(), t)
    for x in t:
        x[:] = np.nan
    del t
    assert [bank.period(j) for j in range(3)] == [4, 1000, 1]
    # 32 channels and the longest table are a bank
    rc, h = _create(L, [TM.shift_table(1, 4)] * 32)
    assert rc == 0 and L.lib.sdrhip_tuner_bank_channels(h) == 32
    L.lib.sdrhip_tuner_bank_destroy(h)
    rc, h = _create(L, [np.zeros(2 * 65536, np.float32)])
    assert rc == 0 and L.lib.sdrhip_tuner_bank_period(h, 0) == 65536
    L.lib.sdrhip_tuner_bank_destroy(h)


def test_create_refuses_bad_arguments(L):
    ok = _tables()

    def refused(what, *args, **kw):
        rc, h = _create(L, *args, **kw)
        assert rc == ERR_ARG, what
        assert not h.value, what + ": a refused create must leave *b null"
        assert b"sdrhip_tuner_bank_create" in L.lib.sdrhip_last_error(), what + f": {L.lib.sdrhip_last_error()!r}"

    refused("no channels", [], channels=0)
    refused("a negative count", ok, channels=-1)
    refused("33 channels", [ok[0]] * 33)
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
    # whatever sdrhip_tuner_create refuses: the decimator's own refusals (an unknown order, factor 0, no taps)
    for what, kw in (("order 7", dict(order=7)), ("factor 0", dict(factor=0)), ("no taps", dict(taps=np.empty(0, np.float32)))):
        h = C.c_void_p()
        a = kw.get("taps", S.taps_decim127())
        o = TM.shift_table(1, 4)
        rc = L.lib.sdrhip_tuner_create(C.byref(h), kw.get("order", L.ORDER_AVX), kw.get("factor", 8), _fp(a), a.size, _fp(o), 4)
        assert rc == ERR_ARG and not h.value, what + ": the tuner takes it, so this is no case"
        refused(what, ok, **kw)
    rc, _ = _create(L, ok, handle=False)
    assert rc == ERR_ARG and b"sdrhip_tuner_bank_create" in L.lib.sdrhip_last_error()
    with pytest.raises(L.SdrHipError):
        L.TunerBank(8, S.taps_decim127(), [np.zeros(3, np.float32)])       # not whole pairs


def test_routes_and_host_side_run_errors(L):
    bank = L.TunerBank(8, S.taps_decim127(), _tables())
    assert L.lib.sdrhip_tuner_bank_set_route(None, 0) == ERR_ARG
    for bad in (3, -1):
        assert L.lib.sdrhip_tuner_bank_set_route(bank.h, bad) == ERR_ARG
        assert b"sdrhip_tuner_bank_set_route" in L.lib.sdrhip_last_error()
    for route in (1, 2, 0):
        bank.set_route(route)
    # refused before any device work: no pointer is looked at
    for run in (L.lib.sdrhip_tuner_bank_run, L.lib.sdrhip_tuner_bank_run_u8):
        def refused(what, *args):
            assert run(*args) == ERR_ARG, what
            assert b"sdrhip_tuner_bank_run" in L.lib.sdrhip_last_error(), what
        refused("null bank", None, None, None, 0, None, 200, 0, 100, 0)
        refused("out_stride < 2 (k_end - k_begin)", bank.h, None, None, 0, None, 198, 0, 100, 0)
        refused("odd out_stride", bank.h, None, None, 0, None, 201, 0, 100, 0)
        refused("k_end < k_begin", bank.h, None, None, 0, None, 200, 100, 0, 0)
        refused("negative k_begin", bank.h, None, None, 0, None, 200, -1, 99, 0)
        refused("a window before d_in", bank.h, None, None, 8, None, 200, 0, 100, 0)
        refused("a seam block shorter than the filter", bank.h, None, None, 0, None, 200, 0, 100, 127)
        refused("null pointers", bank.h, None, None, 0, None, 200, 0, 100, 0)
        assert run(bank.h, None, None, 0, None, 0, 7, 7, 0) == 0           # no outputs: nothing to do
    one = L.TunerBank(8, S.taps_decim127(), _tables()[:1])
    # one channel has no second row to overlap, but its stride is still even
    assert L.lib.sdrhip_tuner_bank_run(one.h, None, None, 0, None, 3, 0, 100, 0) == ERR_ARG
    assert b"odd" in L.lib.sdrhip_last_error()
    assert L.lib.sdrhip_tuner_bank_run(one.h, None, None, 0, None, 0, 0, 100, 0) == ERR_ARG        # ... and then stops at the null pointers
    assert b"d_in != nullptr" in L.lib.sdrhip_last_error()


def test_the_expected_outputs_reach_the_cases_they_exist_for(oracle):
    """From the model alone (as tests/test_record_pipe_cases.py does for the Pipes): at seam 8192 every channel of the 32-channel
    bank has Cross outputs -- outputs that differ from the seamless stream's -- in every launch of the cut, so both the in-tile and
    the fix-up path are compared on each row; and the channels' phases at the cuts differ from channel 0's, so a kernel that took
    channel 0's period, offset or phase for every row would be caught at every cut."""
    tables = BC.bank_tables(32)
    periods = [t.size // 2 for t in tables]
    assert all(a != b for a, b in zip(periods[:-1], periods[1:])), "neighbouring channels never share a period"
    assert 1 in periods and 7 in periods and len(set(periods)) == 7 + 1
    edges = [0] + BC.CUTS + [BC.K_ALL]
    cross = BC.straddlers(BC.B, BC.K_ALL)
    assert cross.size == 15 * (BC.NBLK - 1) and cross[0] == 1009 and cross[14] == 1023
    with_cross = [(a, b) for a, b in zip(edges[:-1], edges[1:]) if ((cross >= a) & (cross < b)).any()]
    assert with_cross == [(1009, 1024), (1024, 3000), (3000, BC.K_ALL)]       # one launch is nothing but a seam's Cross outputs
    for n_out in (4097, 4608):
        assert (cross < n_out).sum() == 15 * 4
    for j in range(32):
        seamed, plain = BC.expected(oracle, tables[j], BC.B), BC.expected(oracle, tables[j], 0)
        assert seamed.size == plain.size == 2 * BC.K_ALL
        diff = np.nonzero((seamed.view(np.uint32) != plain.view(np.uint32)).reshape(-1, 2).any(axis=1))[0]
        assert set(diff) <= set(cross), f"channel {j}: an output that is no straddler depends on the seam"
        for a, b in with_cross:
            assert ((diff >= a) & (diff < b)).any(), f"channel {j}: launch [{a}, {b}) has no Cross output that shows in the bits"
    phases = [[(8 * c) % p for c in BC.CUTS] for p in periods]
    assert any(ph != phases[0] for ph in phases[1:]), "no channel's phase at a cut differs from channel 0's"
    far = [(8 * (BC.FAR_K0 + c)) % p for p in (1000, 5) for c in [0] + BC.FAR_CUTS]
    assert far[:3] != far[3:] and all(f != 0 for f in far), "the far position selects a phase of its own in both channels"
    # and rows differ: a row copied from its neighbour would not pass
    e0, e1 = BC.expected(oracle, tables[0], BC.B), BC.expected(oracle, tables[1], BC.B)
    assert not np.array_equal(e0, e1)
