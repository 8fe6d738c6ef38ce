"""16-bit signed IQ into the FM bank and its stream (sdrhip_fm_bank_run_i16, sdrhip_fm_stream_create_bank_i16, _push_i16,
_input_buffer_i16 and the launch counter) on a host without a GPU: the five names are declared with the issue's C types, exported,
bound and imported by the Haskell module with the header's arity; the run call and the stream's create refuse what they can before
any device work.  A bank is created, planned and sized without a GPU.  What the calls COMPUTE is held to the hand-driven composition
and the restated Pipes on the device (tests/test_gpu_fm_bank_i16.py, tests/test_gpu_fm_bank_stream_i16.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fm_bank_i16_cases as FC
import signals as S
from test_pipe_tuner_bank_abi import _header_signature

ERR_ARG = -1
NEW = {
    "sdrhip_fm_bank_run_i16": ("int", ["sdrhip_fm_bank *", "void *", "const int16_t *", "int64_t", "int64_t", "float *", "int64_t", "int64_t",
                                       "int64_t", "void *", "size_t"]),
    "sdrhip_debug_fm_bank_i16_launches": ("long long", []),
    "sdrhip_fm_stream_create_bank_i16": ("int", ["sdrhip_fm_stream **", "sdrhip_fm_bank *", "int", "int"]),
    "sdrhip_fm_stream_push_i16": ("int", ["sdrhip_fm_stream *", "const int16_t *", "int"]),
    "sdrhip_fm_stream_input_buffer_i16": ("int16_t *", ["sdrhip_fm_stream *"]),
}
B = FC.B


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _bank(L, names, block=B):
    return L.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), [FC.table(n) for n in names], FC.GAIN, block)


def _hs_arity(hs, name):
    """the number of arguments of the foreign import of `name` (arrows of its type, the result excluded)"""
    m = re.search(r'foreign import ccall safe "' + name + r'"\s+\w+\s*::\s*(.*)', hs)
    assert m, f"haskell/SDR/GPU.hs does not import {name}"
    return len(re.findall(r"->", m.group(1)))


def test_new_symbols_are_declared_exported_bound_and_imported(L):
    root = os.path.dirname(L.HERE)
    header = open(os.path.join(root, "include", "sdr_hip.h")).read()
    hs = open(os.path.join(root, "haskell", "SDR", "GPU.hs")).read()
    product = C.CDLL(L.LIB_PATH)
    for name, (ret, params) in NEW.items():
        assert _header_signature(header, name) == (ret, params), f"{name}: sdr_hip.h declares {_header_signature(header, name)}"
        assert hasattr(product, name), f"{name} is not exported"
        bound = getattr(L.lib, name)
        assert bound.argtypes is not None and len(bound.argtypes) == len(params), f"{name} is not bound in sdr_amd/lib.py"
        assert _hs_arity(hs, name) == len(params), f"{name}: GPU.hs imports it with another arity"
    assert L.lib.sdrhip_debug_fm_bank_i16_launches.restype is C.c_longlong
    assert callable(L.fm_bank_i16_launches) and L.fm_bank_i16_launches() == 0
    assert hasattr(L.FmBank, "run_i16") and hasattr(L.FmStream, "push_i16") and hasattr(L.FmStream, "input_buffer_i16")
    assert not hasattr(product, "sdrhip_fm_chain_run_i16"), "int16 reaches the FM side through the bank only"


def test_run_refuses_before_any_device_work(L):
    names = ["shift 1/4", "shift -3/1000", "identity"]
    bank = _bank(L, names)
    total = 20 * B
    q0, q1, halo = bank.plan(0, total, total)
    assert (q0, q1, halo) == (0, 5994, 0) and bank.workspace_bytes(total) > 0       # planned and sized without a GPU
    n = q1 - q0
    run = L.lib.sdrhip_fm_bank_run_i16
    buf = np.zeros(64, np.int16)
    out = np.zeros(16, np.float32)
    p_in, p_out = buf.ctypes.data, out.ctypes.data
    p_in += (-p_in) % 16

    def refused(what, *args, msg=b"sdrhip_fm_bank_run"):
        assert run(*args) == ERR_ARG, what
        assert msg in L.lib.sdrhip_last_error(), (what, L.lib.sdrhip_last_error())

    for route in (0, 1, 2):
        bank.set_route(route)
        refused("null bank", None, None, p_in, 0, total, p_out, n, q0, q1, None, 0)
        refused("rows would overlap", bank.h, None, p_in, 0, total, p_out, n - 1, q0, q1, None, 0)
        refused("q1 < q0", bank.h, None, p_in, 0, total, p_out, n, 10, 5, None, 0)
        refused("negative s0", bank.h, None, p_in, -4, total, p_out, n, q0, q1, None, 0)
        refused("null input", bank.h, None, None, 0, total, p_out, n, q0, q1, None, 0)
        refused("null output", bank.h, None, p_in, 0, total, None, n, q0, q1, None, 0)
        refused("2 bytes past a sample boundary", bank.h, None, p_in + 2, 0, total, p_out, n, q0, q1, None, 0, msg=b"multiple of 4")
        refused("a receptive field outside d_in", bank.h, None, p_in, 0, total - B, p_out, n, q0, q1, None, 0, msg=b"need samples")
        assert run(bank.h, None, None, 0, 0, None, 0, 7, 7, None, 0) == 0           # no outputs: nothing to do
    # route 1 forced where the banked launch does not fit: input 4 bytes past a 16-byte boundary, s0 no multiple of 4, a seam
    # block below the kernel's range
    bank.set_route(1)
    refused("route 1, input 4 bytes past a 16-byte boundary", bank.h, None, p_in + 4, 0, total, p_out, n, q0, q1, None, 0, msg=b"does not fit")
    Q0, Q1, _ = bank.plan(2, total, total)
    refused("route 1, s0 = 2", bank.h, None, p_in, 2, total - 2, p_out, Q1 - Q0, Q0, Q1, None, 0, msg=b"does not fit")
    b160 = _bank(L, names[:2], 160)
    b160.set_route(1)
    refused("route 1, seam block 160", b160.h, None, p_in, 0, total, p_out, n, q0, q1, None, 0, msg=b"does not fit")
    # route 2 / auto without a workspace, and with one too small
    for route in (0, 2):
        bank.set_route(route)
        refused(f"route {route}, no workspace", bank.h, None, p_in + 4, 0, total, p_out, n, q0, q1, None, 0)
        refused(f"route {route}, a workspace of 4096 bytes", bank.h, None, p_in + 4, 0, total, p_out, n, q0, q1, p_out, 4096, msg=b"workspace")
    assert (out == 0).all() and L.fm_bank_i16_launches() == 0
    with pytest.raises(L.SdrHipError):
        _bank(L, names, 100)                                    # shorter than the decimator's taps: no bank at all


def test_stream_create_refuses_before_any_device_work(L):
    bank = _bank(L, ["shift 1/4", "shift -3/1000"])
    create = L.lib.sdrhip_fm_stream_create_bank_i16
    h = C.c_void_p()
    assert create(None, bank.h, B, B) == ERR_ARG and b"sdrhip_fm_stream_create_bank_i16" in L.lib.sdrhip_last_error()
    for what, args in (("a null bank", (None, B, B)), ("max_block_samples 0", (bank.h, 0, B)), ("block_size_out 0", (bank.h, B, 0)),
                       ("max_block_samples no multiple of the seam block", (bank.h, B + 4, B))):
        assert create(C.byref(h), *args) == ERR_ARG, what
        assert b"sdrhip_fm_stream_create_bank_i16" in L.lib.sdrhip_last_error(), what
    s = np.zeros(8, np.int16)
    assert L.lib.sdrhip_fm_stream_push_i16(None, s.ctypes.data, 4) == ERR_ARG and b"sdrhip_fm_stream_push_i16" in L.lib.sdrhip_last_error()
    assert not L.lib.sdrhip_fm_stream_input_buffer_i16(None) and b"sdrhip_fm_stream_input_buffer_i16" in L.lib.sdrhip_last_error()
    with pytest.raises(L.SdrHipError):
        L.FmStream(object(), B, B, input_i16=True)              # int16 reaches the FM side through a bank
