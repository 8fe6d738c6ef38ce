"""The tuner bank's Pipe (sdrhip_pipe_tuner_bank, _rows, _push_u8, _input_buffer_u8, _pop_rows and the cross-launch counter) on a
host without a GPU: the names are declared, exported, bound and imported by the Haskell module with the header's arity and C types;
create refuses every bad argument before any device work, naming the call; the row and u8 calls refuse a null pipe.  What the Pipe
COMPUTES is held to one-row tuner Pipes on the device (tests/test_gpu_pipe_tuner_bank.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import signals as S
import tuner_model as TM

ERR_ARG = -1
# name -> (C return type, C parameter types) as sdr_hip.h declares them
NEW = {
    "sdrhip_pipe_tuner_bank": ("int", ["sdrhip_pipe **", "const sdrhip_tuner_bank *", "int", "int"]),
    "sdrhip_pipe_rows": ("int", ["const sdrhip_pipe *"]),
    "sdrhip_pipe_push_u8": ("int", ["sdrhip_pipe *", "const uint8_t *", "int"]),
    "sdrhip_pipe_input_buffer_u8": ("uint8_t *", ["sdrhip_pipe *", "int"]),
    "sdrhip_pipe_pop_rows": ("int", ["sdrhip_pipe *", "float *", "int64_t", "int"]),
    "sdrhip_debug_tuner_bank_cross_launches": ("long long", []),
}
HS_TYPE = {"int": "CInt", "int64_t": "Int64", "long long": "CLLong", "float *": "Ptr CFloat", "const uint8_t *": "Ptr CUChar",
           "uint8_t *": "Ptr CUChar", "sdrhip_pipe *": "Ptr SdrPipe", "const sdrhip_pipe *": "Ptr SdrPipe",
           "sdrhip_pipe **": "Ptr (Ptr SdrPipe)", "const sdrhip_tuner_bank *": "Ptr SdrTunerBank"}


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def _root(L):
    return os.path.dirname(L.HERE)


def _header_signature(header, name):
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*\b" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"{name} is not declared in sdr_hip.h"

    def norm(t):
        t = re.sub(r"\s+", " ", t.strip())
        t = re.sub(r"\s*\*", " *", t)
        return re.sub(r"\* \*", "**", t)

    params = [] if m.group(2).strip() in ("", "void") else [norm(re.sub(r"\b[A-Za-z_][A-Za-z0-9_]*$", "", q.strip())) for q in m.group(2).split(",")]
    return norm(m.group(1)), params


def test_new_symbols_are_declared_exported_bound_and_imported(L):
    header = open(os.path.join(_root(L), "include", "sdr_hip.h")).read()
    hs = open(os.path.join(_root(L), "haskell", "SDR", "GPU.hs")).read()
    product = C.CDLL(L.LIB_PATH)
    for name, (ret, params) in NEW.items():
        assert _header_signature(header, name) == (ret, params), f"{name}: sdr_hip.h declares {_header_signature(header, name)}"
        assert hasattr(product, name), f"{name} is not exported"
        bound = getattr(L.lib, name)
        assert bound.argtypes is not None and len(bound.argtypes) == len(params), f"{name} is not bound in sdr_amd/lib.py with {len(params)} arguments"
        m = re.search(r'foreign import ccall safe "' + name + r'"\s+\w+\s*::(.*)', hs)
        assert m, f"haskell/SDR/GPU.hs does not import {name}"
        want = [HS_TYPE[p] for p in params] + [f"IO {HS_TYPE[ret]}" if " " not in HS_TYPE[ret] else f"IO ({HS_TYPE[ret]})"]
        assert [t.strip() for t in m.group(1).split("->")] == want, f"{name}: GPU.hs imports it as {m.group(1).strip()}"
    assert L.lib.sdrhip_debug_tuner_bank_cross_launches.restype is C.c_longlong
    assert hasattr(L.Pipe, "tuner_bank") and hasattr(L.Pipe, "rows") and hasattr(L.Pipe, "pop_rows")
    assert callable(L.tuner_bank_cross_launches) and L.tuner_bank_cross_launches() == 0
    assert os.path.exists(os.path.join(_root(L), "examples", "channel_replay.c"))


def test_create_refuses_bad_arguments_before_device_work(L):
    bank = L.TunerBank(8, S.taps_decim127(), [TM.shift_table(1, 4), TM.shift_table(-3, 1000)])       # host code only
    create = L.lib.sdrhip_pipe_tuner_bank

    def refused(what, *args):
        assert create(*args) == ERR_ARG, what
        assert b"sdrhip_pipe_tuner_bank" in L.lib.sdrhip_last_error(), what

    h = C.c_void_p()
    refused("a null out-pointer", None, bank.h, 1024, 0)
    for what, args in (("a null bank", (None, 1024, 0)), ("block_size_out 0", (bank.h, 0, 0)), ("block_size_out < 0", (bank.h, -5, 1)),
                       ("input_u8 2", (bank.h, 1024, 2)), ("input_u8 -1", (bank.h, 1024, -1))):
        h.value = 0xdead
        refused(what, C.byref(h), *args)
        assert not h.value, what + ": a refused create handed out a pipe"
    with pytest.raises(L.SdrHipError):
        L.Pipe.tuner_bank(bank, 0)
    with pytest.raises(L.SdrHipError):
        L.Pipe.tuner_bank(bank, 1024, input_u8=2)


def test_row_and_u8_calls_refuse_a_null_pipe(L):
    out = np.zeros(4, np.float32)
    u = np.zeros(8, np.uint8)
    for name, call in (("sdrhip_pipe_rows", lambda: L.lib.sdrhip_pipe_rows(None)),
                       ("sdrhip_pipe_pop_rows", lambda: L.lib.sdrhip_pipe_pop_rows(None, out.ctypes.data_as(C.POINTER(C.c_float)), 4, 1)),
                       ("sdrhip_pipe_push_u8", lambda: L.lib.sdrhip_pipe_push_u8(None, u.ctypes.data_as(C.POINTER(C.c_uint8)), 4))):
        assert call() == ERR_ARG, name
        assert name.encode() in L.lib.sdrhip_last_error(), name
    assert not L.lib.sdrhip_pipe_input_buffer_u8(None, 4) and b"sdrhip_pipe_input_buffer_u8" in L.lib.sdrhip_last_error()
    assert (out == 0).all()
