"""The waterfall Pipe (sdrhip_pipe_spectrum) and int16 input of the spectrum operator (SDRHIP_IQ_I16) on a host without a GPU: the
names are declared, exported and bound, sdrhip_spectrum_create takes the new format and still refuses an unknown one, and the Pipe's
create refuses every bad argument under its own name, before any device work, handing out no pipe -- the carried tail's 4 MiB cap on
both sides of its edge.  What they COMPUTE is held to the operator on the device (tests/test_gpu_spectrum_i16.py,
tests/test_gpu_pipe_spectrum.py)."""
import ctypes as C
import os

import pytest

import spectrum_pipe_model as SP

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_pipe_spectrum"]


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert callable(L.Pipe.spectrum) and L.IQ_I16 == 2
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sdr_hip.h")).read()
    assert "#define SDRHIP_IQ_I16  2" in hdr


def test_spectrum_create_takes_int16_and_refuses_an_unknown_format(L):
    s = L.Spectrum(256, L.IQ_I16, L.WINDOW_HANNING, True, 1.0)
    assert L.lib.sdrhip_spectrum_size(s.h) == 256
    for bad in (7, 3, -1):
        h = C.c_void_p(0xdead)
        assert L.lib.sdrhip_spectrum_create(C.byref(h), 256, bad, 0, None, 0, 1.0) == ERR_ARG, f"format {bad}"
        assert not h.value


def test_pipe_create_refuses_bad_arguments_before_any_device_work(L):
    spec = L.Spectrum(64, L.IQ_U8)

    def refused(what, *args):
        h = C.c_void_p(0xdead)                                   # a refused create must overwrite it with null
        assert L.lib.sdrhip_pipe_spectrum(C.byref(h), *args) == ERR_ARG, what
        assert not h.value, what + ": a refused create must leave *p null"
        assert b"sdrhip_pipe_spectrum" in L.lib.sdrhip_last_error(), what

    ok = (64, 1, L.REDUCE_MEAN_MAGNITUDE, L.UNIT_LINEAR, -200.0)
    refused("a null spectrum object", None, *ok)
    assert L.lib.sdrhip_pipe_spectrum(None, spec.h, *ok) == ERR_ARG and b"sdrhip_pipe_spectrum" in L.lib.sdrhip_last_error()
    for hop in (0, -1):
        refused(f"hop {hop}", spec.h, hop, 1, 1, 0, -200.0)
    for group in (0, -3):
        refused(f"group {group}", spec.h, 64, group, 1, 0, -200.0)
    for reduce in (-1, 3):
        refused(f"reduce {reduce}", spec.h, 64, 1, reduce, 0, -200.0)
    for unit in (-1, 2):
        refused(f"unit {unit}", spec.h, 64, 1, 1, unit, -200.0)
    for floor_db in (float("inf"), float("-inf"), float("nan")):
        refused(f"floor_db {floor_db}", spec.h, 64, 1, 1, 1, floor_db)


@pytest.mark.parametrize("fmt", ["u8", "cf32", "i16"])
def test_the_tail_cap_on_both_sides_of_its_edge(L, fmt):
    """((group - 1) * hop + n - 1) * sample_bytes > 4 MiB is refused; equal to 4 MiB is not refused FOR THAT REASON (without a device the
    accepted create goes on to make streams and may fail there, with another code or message)."""
    n, group = 64, 2
    spec = L.Spectrum(n, {"u8": L.IQ_U8, "cf32": L.IQ_CF32, "i16": L.IQ_I16}[fmt])
    sb = SP.SAMPLE_BYTES[fmt]
    hop_edge = SP.TAIL_CAP_BYTES // sb - (n - 1)                  # (group - 1) * hop + n - 1 == 4 MiB / sample_bytes exactly
    assert ((group - 1) * hop_edge + n - 1) * sb == SP.TAIL_CAP_BYTES
    h = C.c_void_p(0xdead)
    assert L.lib.sdrhip_pipe_spectrum(C.byref(h), spec.h, hop_edge + 1, group, 1, 0, -200.0) == ERR_ARG
    assert not h.value and b"4 MiB" in L.lib.sdrhip_last_error()
    # a huge group or hop must not overflow its way past the check
    for hop, g in ((1 << 62, 2), (1 << 40, 1 << 30), (3, 2147483647)):
        h = C.c_void_p(0xdead)
        assert L.lib.sdrhip_pipe_spectrum(C.byref(h), spec.h, hop, g, 1, 0, -200.0) == ERR_ARG, (hop, g)
        assert not h.value and b"4 MiB" in L.lib.sdrhip_last_error()
    h = C.c_void_p(0xdead)
    rc = L.lib.sdrhip_pipe_spectrum(C.byref(h), spec.h, hop_edge, group, 1, 0, -200.0)
    if rc == 0:
        L.lib.sdrhip_pipe_destroy(h)
    else:
        assert not h.value and b"4 MiB" not in L.lib.sdrhip_last_error(), "the edge itself is inside the cap"


def test_the_binding_refuses_an_array_of_another_dtype(L):
    """Pipe.push looks at the dtype before it calls the library (as the AM bank Pipe's binding): checked on the class, without a pipe."""
    import numpy as np

    class Fake(L.Pipe):
        def __init__(self, u8, i16):
            self.input_u8, self.input_i16 = u8, i16

        def __del__(self):
            pass

    for u8, i16, good in ((True, False, np.uint8), (False, True, np.int16), (False, False, np.float32)):
        p = Fake(u8, i16)
        p._wrong_dtype(np.zeros(4, good), "Pipe.push")
        for bad in (np.uint8, np.int16, np.float32):
            if bad is not good:
                with pytest.raises(L.SdrHipError):
                    p._wrong_dtype(np.zeros(4, bad), "Pipe.push")
