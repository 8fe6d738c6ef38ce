"""The audio Pipes of the two banks (sdrhip_pipe_am_bank_audio, sdrhip_pipe_nfm_bank_audio) on a host without a GPU: the names are
declared, exported and bound, create refuses every bad argument under its own name before any device work, handing out no pipe, and
the kind numbers stand behind the older ones.  A pipe itself needs a device (its engine creates streams): the wrong push call for each
input type, the state's size and what the Pipes COMPUTE are held on the device (tests/test_gpu_pipe_bank_audio.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import audio_tail_cases as AC
import signals as S
import tuner_model as TM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_pipe_am_bank_audio", "sdrhip_pipe_nfm_bank_audio", "sdrhip_audio_tail_shape"]


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _tuner_bank(L):
    tables = [TM.shift_table(1, 4), TM.shift_table(-3, 1000), np.array([1.0, 0.0], np.float32)]
    return L.TunerBank(8, S.taps_decim127(), tables)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert callable(L.Pipe.am_bank_audio) and callable(L.Pipe.nfm_bank_audio)


def test_the_tail_s_shape_is_what_a_saved_state_records(L):
    t = L.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), block=8192)
    shape = (C.c_int32 * 4)()
    assert L.lib.sdrhip_audio_tail_shape(t.h, shape) == 0 and list(shape) == [3, 10, AC.RLP, AC.LF]
    assert L.lib.sdrhip_audio_tail_shape(None, shape) == ERR_ARG and L.lib.sdrhip_audio_tail_shape(t.h, None) == ERR_ARG


@pytest.mark.parametrize("which", ["am", "nfm"])
def test_create_refuses_bad_arguments_before_any_device_work(L, which):
    tb = _tuner_bank(L)
    bank = L.AmBank(tb, dc_block=True) if which == "am" else L.NfmBank(tb)
    fn = L.lib.sdrhip_pipe_am_bank_audio if which == "am" else L.lib.sdrhip_pipe_nfm_bank_audio
    name = f"sdrhip_pipe_{which}_bank_audio".encode()
    tail = L.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), block=8192)
    contiguous = L.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), block=0)

    def refused(what, *args):
        h = C.c_void_p(0xdead)                                   # a refused create must overwrite it with null
        assert fn(C.byref(h), *args) == ERR_ARG, what
        assert not h.value, what + ": a refused create must leave *p null"
        assert name in L.lib.sdrhip_last_error(), what

    refused("a null bank", None, tail.h, 0)
    refused("a null tail", bank.h, None, 0)
    refused("a tail of block 0", bank.h, contiguous.h, 0)
    for bad in (-1, 3, 7):
        refused(f"input_type {bad}", bank.h, tail.h, bad)
    assert fn(None, bank.h, tail.h, 0) == ERR_ARG and name in L.lib.sdrhip_last_error()
    make = L.Pipe.am_bank_audio if which == "am" else L.Pipe.nfm_bank_audio
    with pytest.raises(ValueError):
        make(bank, tail, input_u8=True, input_i16=True)
    with pytest.raises(L.SdrHipError):
        make(bank, contiguous)


def test_the_kind_numbers_stand_behind_the_older_ones():
    """Saved states hold the kind's number: the ten oldest kinds keep 0 .. 9, the waterfall's (10) and the narrow-band FM bank's (11)
    follow, the two audio kinds come behind those (12, 13), and the narrow bank's (14) is the last."""
    from pipe_kind_table import KIND_NUMBERS, pipe_kind_table
    table = pipe_kind_table()
    assert table == list(KIND_NUMBERS.items()), "the whole table, name by name and number by number, in the order of the numbers"
    assert dict(table)["PK_AM_BANK_AUDIO"] == 12 and dict(table)["PK_NFM_BANK_AUDIO"] == 13
