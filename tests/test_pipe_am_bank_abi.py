"""The AM bank's Pipe (sdrhip_pipe_am_bank) on a host without a GPU: the names are declared, exported and bound, and create refuses
every bad argument under its own name, before any device work, handing out no pipe.  What the Pipe COMPUTES is held to the model on
the device (tests/test_gpu_pipe_am_bank.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_model as TM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_pipe_am_bank", "sdrhip_debug_am_bank_cross_launches"]


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _bank(L, dc=True):
    tables = [TM.shift_table(1, 4), TM.shift_table(-3, 1000), np.array([1.0, 0.0], np.float32)]
    return L.AmBank(L.TunerBank(8, S.taps_decim127(), tables), dc_block=dc)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_am_bank_cross_launches.restype is C.c_longlong and L.am_bank_cross_launches() >= 0
    assert callable(L.Pipe.am_bank)


def test_create_refuses_bad_arguments_before_any_device_work(L):
    am = _bank(L)

    def refused(what, *args):
        h = C.c_void_p(0xdead)                                   # a refused create must overwrite it with null
        assert L.lib.sdrhip_pipe_am_bank(C.byref(h), *args) == ERR_ARG, what
        assert not h.value, what + ": a refused create must leave *p null"
        assert b"sdrhip_pipe_am_bank" in L.lib.sdrhip_last_error(), what

    refused("a null bank", None, 1000, 0)
    for bad in (0, -1):
        refused(f"block_size_out {bad}", am.h, bad, 0)
    for bad in (-1, 3, 7):
        refused(f"input_type {bad}", am.h, 1000, bad)
    assert L.lib.sdrhip_pipe_am_bank(None, am.h, 1000, 0) == ERR_ARG and b"sdrhip_pipe_am_bank" in L.lib.sdrhip_last_error()
    with pytest.raises(ValueError):
        L.Pipe.am_bank(am, 1000, input_u8=True, input_i16=True)


def test_the_kind_is_the_last_of_the_enum():
    """Saved states hold the kind's number: the ten kinds up to the AM bank's keep theirs, 0 .. 9, the AM bank's being the last of
    them, and every kind behind them has a number of its own."""
    from pipe_kind_table import KIND_NUMBERS, pipe_kind_table
    table = pipe_kind_table()
    assert table[:10] == [(k, n) for k, n in KIND_NUMBERS.items() if n <= 9] and table[9] == ("PK_AM_BANK", 9)
    assert len({n for _, n in table}) == len(table) == len({k for k, _ in table}), "a number or a name stands twice"
    assert all(n >= 10 for _, n in table[10:])
