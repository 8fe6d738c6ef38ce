"""16-bit signed IQ into the tuner family (sdrhip_tuner_run_i16, sdrhip_tuner_bank_run_i16, sdrhip_pipe_tuner_bank_i16, _push_i16,
_input_buffer_i16 and the launch counter) on a host without a GPU: the names are declared with the issue's C types, exported, bound
and imported by the Haskell module; the run calls and the pipe's create refuse what they can before any device work; the int16 stream
of the GPU tests holds the values it exists for, and the subnormal table meets zeros of both signs and subnormals on it.  What the
calls COMPUTE is held to the model on the device (tests/test_gpu_tuner_i16.py); the wrong push / input_buffer call for a pipe's type
needs a pipe, which needs a device's streams, so it is there too."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import signals as S
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from test_pipe_tuner_bank_abi import _header_signature

ERR_ARG = -1
RUN = ["int64_t", "float *", "int64_t", "int64_t", "int64_t"]
NEW = {
    "sdrhip_tuner_run_i16": ("int", ["const sdrhip_tuner *", "void *", "const int16_t *"] + RUN),
    "sdrhip_tuner_bank_run_i16": ("int", ["const sdrhip_tuner_bank *", "void *", "const int16_t *", "int64_t", "float *", "int64_t", "int64_t",
                                          "int64_t", "int64_t"]),
    "sdrhip_pipe_tuner_bank_i16": ("int", ["sdrhip_pipe **", "const sdrhip_tuner_bank *", "int"]),
    "sdrhip_pipe_push_i16": ("int", ["sdrhip_pipe *", "const int16_t *", "int"]),
    "sdrhip_pipe_input_buffer_i16": ("int16_t *", ["sdrhip_pipe *", "int"]),
    "sdrhip_debug_tuner_i16_launches": ("long long", []),
}
HS_IMPORTED = ["sdrhip_tuner_run_i16", "sdrhip_tuner_bank_run_i16", "sdrhip_pipe_tuner_bank_i16", "sdrhip_pipe_push_i16", "sdrhip_pipe_input_buffer_i16",
               "sdrhip_debug_tuner_i16_launches"]


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def test_new_symbols_are_declared_exported_and_bound(L):
    root = os.path.dirname(L.HERE)
    header = open(os.path.join(root, "include", "sdr_hip.h")).read()
    hs = open(os.path.join(root, "haskell", "SDR", "GPU.hs")).read()
    product = C.CDLL(L.LIB_PATH)
    for name, (ret, params) in NEW.items():
        assert _header_signature(header, name) == (ret, params), f"{name}: sdr_hip.h declares {_header_signature(header, name)}"
        assert hasattr(product, name), f"{name} is not exported"
        bound = getattr(L.lib, name)
        assert bound.argtypes is not None and len(bound.argtypes) == len(params), f"{name} is not bound in sdr_amd/lib.py"
    for name in HS_IMPORTED:
        assert re.search(r'foreign import ccall safe "' + name + r'"', hs), f"haskell/SDR/GPU.hs does not import {name}"
    assert L.lib.sdrhip_debug_tuner_i16_launches.restype is C.c_longlong
    assert callable(L.tuner_i16_launches) and L.tuner_i16_launches() == 0
    assert hasattr(L.Tuner, "run_i16") and hasattr(L.TunerBank, "run_i16")


def test_the_run_calls_refuse_before_any_device_work(L):
    taps = S.taps_decim127()
    bank = L.TunerBank(8, taps, [TM.shift_table(1, 4), TM.shift_table(-3, 1000), BC.IDENTITY])
    run = L.lib.sdrhip_tuner_bank_run_i16

    def refused(what, *args):
        assert run(*args) == ERR_ARG, what
        assert b"sdrhip_tuner_bank_run" in L.lib.sdrhip_last_error(), what

    # no pointer is looked at: they are all null
    refused("null bank", None, None, None, 0, None, 200, 0, 100, 0)
    refused("a row too short with more than one channel", bank.h, None, None, 0, None, 198, 0, 100, 0)
    refused("odd out_stride", bank.h, None, None, 0, None, 201, 0, 100, 0)
    refused("k_end < k_begin", bank.h, None, None, 0, None, 200, 100, 0, 0)
    refused("a first window before d_in", bank.h, None, None, 8, None, 200, 0, 100, 0)
    refused("a seam block shorter than the filter", bank.h, None, None, 0, None, 200, 0, 100, 127)
    refused("null pointers", bank.h, None, None, 0, None, 200, 0, 100, 0)
    assert run(bank.h, None, None, 0, None, 0, 7, 7, 0) == 0               # no outputs: nothing to do
    one = L.TunerBank(8, taps, [TM.shift_table(1, 4)])
    assert run(one.h, None, None, 0, None, 3, 0, 100, 0) == ERR_ARG and b"odd" in L.lib.sdrhip_last_error()
    # an int16 buffer 2 bytes off a sample boundary is refused on every route, before the device is touched
    buf = np.zeros(4096, np.int16)
    out = np.zeros(8, np.float32)
    odd = buf.ctypes.data + 2
    for route in (0, 1, 2):
        bank.set_route(route)
        assert run(bank.h, None, odd, 0, out.ctypes.data, 2, 0, 1, 0) == ERR_ARG, f"route {route}"
        assert b"multiple of 4" in L.lib.sdrhip_last_error()
    assert (out == 0).all()

    t = L.Tuner(8, taps, TM.shift_table(1, 4))
    trun = L.lib.sdrhip_tuner_run_i16
    for what, args in (("null tuner", (None, None, None, 0, None, 0, 100, 0)),
                       ("a first window before d_in", (t.h, None, None, 8, None, 0, 100, 0)),
                       ("a seam block shorter than the filter", (t.h, None, None, 0, None, 0, 100, 127)),
                       ("k_end < k_begin", (t.h, None, None, 0, None, 100, 0, 0)),
                       ("null pointers", (t.h, None, None, 0, None, 0, 100, 0))):
        assert trun(*args) == ERR_ARG, what
        assert b"tuner_run" in L.lib.sdrhip_last_error(), what
    assert trun(t.h, None, None, 0, None, 7, 7, 0) == 0
    for route in (0, 1, 2):
        t.set_route(route)
        assert trun(t.h, None, odd, 0, out.ctypes.data, 0, 1, 0) == ERR_ARG and b"multiple of 4" in L.lib.sdrhip_last_error()


def test_pipe_create_refuses_bad_arguments_before_device_work(L):
    bank = L.TunerBank(8, S.taps_decim127(), [TM.shift_table(1, 4), TM.shift_table(-3, 1000)])
    create = L.lib.sdrhip_pipe_tuner_bank_i16
    h = C.c_void_p()
    assert create(None, bank.h, 1024) == ERR_ARG and b"sdrhip_pipe_tuner_bank_i16" in L.lib.sdrhip_last_error()
    for what, args in (("a null bank", (None, 1024)), ("block_size_out 0", (bank.h, 0)), ("block_size_out < 0", (bank.h, -5))):
        h.value = 0xdead
        assert create(C.byref(h), *args) == ERR_ARG, what
        assert b"sdrhip_pipe_tuner_bank_i16" in L.lib.sdrhip_last_error(), what
        assert not h.value, what + ": a refused create handed out a pipe"
    with pytest.raises(L.SdrHipError):
        L.Pipe.tuner_bank(bank, 0, input_i16=True)
    with pytest.raises(ValueError):
        L.Pipe.tuner_bank(bank, 1024, input_u8=True, input_i16=True)
    # null pipes
    s = np.zeros(8, np.int16)
    assert L.lib.sdrhip_pipe_push_i16(None, s.ctypes.data_as(C.POINTER(C.c_int16)), 4) == ERR_ARG
    assert b"sdrhip_pipe_push_i16" in L.lib.sdrhip_last_error()
    assert not L.lib.sdrhip_pipe_input_buffer_i16(None, 4) and b"sdrhip_pipe_input_buffer_i16" in L.lib.sdrhip_last_error()


def test_the_stream_and_the_expected_outputs_reach_the_cases_they_exist_for(oracle):
    s = IC.stream_i16()
    assert s.dtype == np.int16 and s.size == 2 * IC.NBLK * IC.B
    for v in IC.FORCED:
        assert (s == v).sum() >= 3, f"the stream holds {v}"
    for e in range(IC.B, IC.NBLK * IC.B, IC.B):
        assert set(int(v) for v in s[2 * e - 5:2 * e + 5]) <= set(IC.FORCED), f"the elements around block edge {e}"
    real = s[2 * 2 * IC.B:2 * 3 * IC.B]
    mag = np.abs(real.astype(np.int32))
    assert (mag > 2048).sum() <= 16 and (mag >= 2000).any(), "block 2 is a BladeRF's real range but for the forced +-32768"
    rest = np.concatenate([s[:2 * 2 * IC.B], s[2 * 3 * IC.B:]]).astype(np.int32)
    assert rest.min() == -32768 and rest.max() == 32767 and (np.abs(rest) > 16384).mean() > 0.4
    # the conversion is s * 2^-11 over the whole range, exact, and 0 -> +0
    x = oracle.convert_i16(s)
    assert np.array_equal(x.view(np.uint32), (s.astype(np.float32) * np.float32(2.0 ** -11)).view(np.uint32))
    every = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    assert np.array_equal(oracle.convert_i16(every).view(np.uint32), (every.astype(np.float64) / 2048.0).astype(np.float32).view(np.uint32))
    assert oracle.convert_i16(np.zeros(2, np.int16)).view(np.uint32).tolist() == [0, 0]
    # the subnormal table: zeros of both signs and subnormals among the MIXED samples, which is where a loader that scaled the table
    # or the taps instead of the sample would go wrong.  (Not among the outputs: a sum of 128 products that starts at +0 is never -0,
    # and on a full-range stream it is neither zero nor subnormal -- the u8 stream's expected outputs hold none either.)  The seam
    # shows in the bits of the outputs
    for seam in (0, IC.B):
        e = IC.expected(oracle, BC.SUBNORMALS, seam)
        assert e.size == 2 * IC.K_ALL
    m = TM.mix(x, BC.SUBNORMALS).view(np.uint32)
    assert (m == 0).any() and (m == 0x80000000).any(), "the mixed stream holds zeros of both signs"
    mag = m & 0x7FFFFFFF
    assert ((mag > 0) & (mag < 0x00800000)).any(), "the mixed stream holds subnormals"
    e = IC.expected(oracle, BC.SUBNORMALS, IC.B).view(np.uint32)
    emag = e & 0x7FFFFFFF
    assert np.isfinite(e.view(np.float32)).all() and (emag > 0).any()
    cross = BC.straddlers(IC.B, IC.K_ALL)
    plain = IC.expected(oracle, BC.SUBNORMALS, 0).view(np.uint32)
    diff = np.nonzero((e != plain).reshape(-1, 2).any(axis=1))[0]
    assert diff.size > 0 and set(diff) <= set(cross)
