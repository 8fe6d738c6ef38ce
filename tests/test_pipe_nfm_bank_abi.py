"""The narrow-band FM bank's Pipe (sdrhip_pipe_nfm_bank) on a host without a GPU: the name is declared, exported and bound, every
create refusal comes before any device work and leaves *p null, and the kind table of pipe.hpp gives the older kinds their numbers and this one the
next.  What the pipe COMPUTES is held to the models on the device (tests/test_gpu_pipe_nfm_bank.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_model as TM

ERR_ARG = -1


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _bank(L):
    tables = [TM.shift_table(1, 4), TM.shift_table(-3, 1000), np.array([1.0, 0.0], np.float32)]
    return L.NfmBank(L.TunerBank(8, S.taps_decim127(), tables))


def test_the_symbol_is_declared_exported_and_bound(L):
    from test_abi import declared_functions
    assert "sdrhip_pipe_nfm_bank" in declared_functions()
    assert hasattr(C.CDLL(L.LIB_PATH), "sdrhip_pipe_nfm_bank")
    assert L.lib.sdrhip_pipe_nfm_bank.argtypes is not None and callable(L.Pipe.nfm_bank)


def test_create_refuses_bad_arguments_before_any_device_work(L):
    nb = _bank(L)

    def refused(what, *args):
        h = C.c_void_p(0xdead)                                   # a refused create must overwrite it with null
        assert L.lib.sdrhip_pipe_nfm_bank(C.byref(h), *args) == ERR_ARG, what
        assert not h.value, what + ": a refused create must leave *p null"
        assert b"sdrhip_pipe_nfm_bank" in L.lib.sdrhip_last_error(), what

    refused("a null bank", None, 1000, 0)
    for bad in (0, -1):
        refused(f"block_size_out {bad}", nb.h, bad, 0)
    for bad in (-1, 3, 7):
        refused(f"input_type {bad}", nb.h, 1000, bad)
    assert L.lib.sdrhip_pipe_nfm_bank(None, nb.h, 1000, 0) == ERR_ARG and b"sdrhip_pipe_nfm_bank" in L.lib.sdrhip_last_error()
    with pytest.raises(ValueError):
        L.Pipe.nfm_bank(nb, 1000, input_u8=True, input_i16=True)


def test_the_kind_line_is_unchanged_and_the_new_kind_stands_behind_it():
    """The kind table (sdr_amd/csrc/pipe.hpp) as written: the ten older kinds keep 0 .. 9, the waterfall's is 10 and this Pipe's 11."""
    from pipe_kind_table import KIND_NUMBERS, pipe_kind_table
    table = pipe_kind_table()
    assert table[:12] == [(k, n) for k, n in KIND_NUMBERS.items() if n <= 11]
    assert dict(table)["PK_SPECTRUM"] == 10 and dict(table)["PK_NFM_BANK"] == 11
