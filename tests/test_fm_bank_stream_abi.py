"""The bank's host-block front end (sdrhip_fm_stream_create_bank, _rows, _pop_rows) on a host without a GPU: the names are
declared, exported, bound and imported by the Haskell module; create refuses every bad argument before any device work, naming the
call; the two row calls refuse a null stream.  What a bank's stream COMPUTES is held to tuned chains and to streams over tuned
chains on the device (tests/test_gpu_fm_bank_stream.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuner_model as TM

B = 8192
ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_fm_stream_create_bank", "sdrhip_fm_stream_rows", "sdrhip_fm_stream_pop_rows"]


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _bank(L, block=B):
    tables = [TM.shift_table(1, 4), TM.shift_table(-3, 1000)]
    return L.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), tables, 0.2, block)


def test_new_symbols_are_declared_exported_bound_and_imported(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    hs = open(os.path.join(os.path.dirname(L.HERE), "haskell", "SDR", "GPU.hs")).read()
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
        assert f'"{n}"' in hs, f"haskell/SDR/GPU.hs does not import {n}"
    assert hasattr(L.FmStream, "rows") and hasattr(L.FmStream, "pop_rows")
    header = open(os.path.join(os.path.dirname(L.HERE), "include", "sdr_hip.h")).read()
    assert "no host-block stream front end" not in " ".join(header.split()).replace("* ", "")


def test_create_bank_refuses_bad_arguments_before_device_work(L):
    bank = _bank(L)
    create = L.lib.sdrhip_fm_stream_create_bank

    def refused(what, *args):
        assert create(*args) == ERR_ARG, what
        assert b"sdrhip_fm_stream_create_bank" in L.lib.sdrhip_last_error(), what

    h = C.c_void_p()
    refused("a null bank", C.byref(h), None, B, B)
    assert not h.value
    refused("a null out-pointer", None, bank.h, B, B)
    refused("max_block_samples that is no multiple of the seam block", C.byref(h), bank.h, B + 8, B)
    refused("max_block_samples 0", C.byref(h), bank.h, 0, B)
    refused("block_size_out 0", C.byref(h), bank.h, B, 0)
    refused("block_size_out < 0", C.byref(h), bank.h, B, -5)
    assert not h.value, "a refused create handed out a stream"
    # the same refusals, at the same point, as the chain's create
    chain = L.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, B)
    for args in ((B + 8, B), (0, B), (B, 0)):
        assert L.lib.sdrhip_fm_stream_create(C.byref(h), chain.h, *args) == ERR_ARG
        assert create(C.byref(h), bank.h, *args) == ERR_ARG
    with pytest.raises(L.SdrHipError):
        L.FmStream(bank, B + 8, B)
    # a contiguous bank (block 0) takes any push size in its argument check; 1000-sample blocks want multiples of 1000
    odd = _bank(L, block=1000)
    refused("8192 samples on a 1000-sample seam block", C.byref(h), odd.h, B, B)


def test_row_calls_refuse_a_null_stream(L):
    out = np.zeros(4, np.float32)
    assert L.lib.sdrhip_fm_stream_rows(None) == ERR_ARG
    assert b"sdrhip_fm_stream_rows" in L.lib.sdrhip_last_error()
    assert L.lib.sdrhip_fm_stream_pop_rows(None, out.ctypes.data_as(C.POINTER(C.c_float)), 4, 1) == ERR_ARG
    assert b"sdrhip_fm_stream_pop_rows" in L.lib.sdrhip_last_error()
    assert (out == 0).all()
