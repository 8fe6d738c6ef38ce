"""The tuner without a GPU: the header and the library's exports, sdrhip_tuner_shift_table (pure host code) against the numpy
restatement of its documented reduction (tests/tuner_model.py), the mix's signed zeros by hand, and the argument errors that are
raised before any device work."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tuner_model as TM
from conftest import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("sdrhip_tuner_create", "sdrhip_tuner_num_coeffs", "sdrhip_tuner_factor", "sdrhip_tuner_period", "sdrhip_tuner_destroy",
                "sdrhip_tuner_run", "sdrhip_tuner_run_u8", "sdrhip_tuner_shift_table", "sdrhip_tuner_set_route",
                "sdrhip_debug_tuner_fused_launches", "sdrhip_pipe_tuner")
ERR_ARG = -1

SHIFTS = [(1, 2), (1, 4), (3, 4), (1, 8), (3, 8), (1, 5), (2, 5), (7, 1000), (1, 8192), (4095, 8192), (1, 65536), (-1, 4)]


def _f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as B
    if not os.path.exists(B.LIB):
        B.build()
    import sdr_amd.lib as lib
    return lib


def test_header_declares_and_library_exports_the_tuner(L):
    with open(os.path.join(ROOT, "include", "sdr_hip.h")) as f:
        header = f.read()
    product = C.CDLL(L.LIB_PATH)
    for sym in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % sym, header), f"{sym} is not declared in include/sdr_hip.h"
        assert hasattr(product, sym), f"{sym} is not exported by {os.path.basename(L.LIB_PATH)}"


@pytest.mark.parametrize("num,den", SHIFTS)
def test_shift_table_matches_the_documented_reduction(L, num, den):
    got = L.tuner_shift_table(num, den)
    assert got.shape == (2 * den,)
    assert_bit_equal(got, TM.shift_table(num, den), f"shift table ({num}, {den})")
    # within an ulp or so of the plain double evaluation, and on the unit circle
    n = np.arange(den, dtype=np.int64)
    z = np.exp(2j * np.pi * ((n * (num % den)) % den) / den)
    assert np.max(np.abs(got.reshape(-1, 2).astype(np.float64) - np.stack([z.real, z.imag], axis=1))) < 1.2e-7


def test_quarter_and_half_band_tables_are_the_references(L):
    """quarterBandUp / halfBandUp (Util.hs:263-285): 1 :+ 0, 0 :+ 1, (-1) :+ 0, 0 :+ (-1) and 1, -1 -- every zero +0."""
    assert_bit_equal(L.tuner_shift_table(1, 4), _f32([0x3F800000, 0, 0, 0x3F800000, 0xBF800000, 0, 0, 0xBF800000]), "(1, 4)")
    assert_bit_equal(L.tuner_shift_table(1, 2), _f32([0x3F800000, 0, 0xBF800000, 0]), "(1, 2)")
    assert_bit_equal(L.tuner_shift_table(-1, 4), _f32([0x3F800000, 0, 0, 0xBF800000, 0xBF800000, 0, 0, 0x3F800000]), "(-1, 4)")


@pytest.mark.parametrize("num,den", [(1, 8), (3, 8), (4095, 8192), (1, 65536)])
def test_quarter_turns_are_exact_and_odd_eighths_symmetric(L, num, den):
    t = L.tuner_shift_table(num, den).reshape(-1, 2)
    r = (np.arange(den, dtype=np.int64) * num) % den
    quarter = (4 * r) % den == 0
    b = t[quarter].view(np.uint32)
    assert np.all((b == 0x3F800000) | (b == 0xBF800000) | (b == 0)), "a multiple of a quarter turn is not (+-1, +0) / (+0, +-1)"
    eighth = ((8 * r) % den == 0) & ~quarter
    assert eighth.any()
    assert np.all(np.abs(t[eighth, 0]) == np.abs(t[eighth, 1])) and np.all(np.abs(t[eighth, 0]) == np.float32(np.sqrt(0.5)))


def test_mix_signed_zeros_by_hand():
    """The (1, 4) table on samples with +-0 components, starting at stream position 0.  Each expected value is the formula
    (a*c - b*d, a*d + b*c) worked out by hand in IEEE arithmetic: x * (+0) keeps x's sign on the zero, (+0) - (+0) = +0,
    (-0) - (+0) = -0, (+0) + (-0) = +0, (-0) + (-0) = -0."""
    P0, N0, TWO = 0x00000000, 0x80000000, 0x40000000
    x = _f32([P0, P0,      # n = 0, o = ( 1, +0): (+0*1 - +0*+0, +0*+0 + +0*1)  = (+0 - +0, +0 + +0)   = (+0, +0)
              N0, P0,      # n = 1, o = (+0,  1): (-0*+0 - +0*1, -0*1 + +0*+0)  = (-0 - +0, -0 + +0)   = (-0, +0)
              P0, N0,      # n = 2, o = (-1, +0): (+0*-1 - -0*+0, +0*+0 + -0*-1) = (-0 - -0, +0 + +0)  = (+0, +0)
              N0, N0,      # n = 3, o = (+0, -1): (-0*+0 - -0*-1, -0*-1 + -0*+0) = (-0 - +0, +0 + -0)  = (-0, +0)
              N0, TWO,     # n = 4, o = ( 1, +0): (-0*1 - 2*+0, -0*+0 + 2*1)    = (-0 - +0, -0 + 2)    = (-0, 2)
              TWO, N0,     # n = 5, o = (+0,  1): (2*+0 - -0*1, 2*1 + -0*+0)    = (+0 - -0, 2 + -0)    = (+0, 2)
              N0, N0,      # n = 6, o = (-1, +0): (-0*-1 - -0*+0, -0*+0 + -0*-1) = (+0 - -0, -0 + +0)  = (+0, +0)
              P0, TWO])    # n = 7, o = (+0, -1): (+0*+0 - 2*-1, +0*-1 + 2*+0)  = (+0 + 2, -0 + +0)    = (2, +0)
    exp = _f32([P0, P0, N0, P0, P0, P0, N0, P0, N0, TWO, P0, TWO, P0, P0, TWO, P0])
    osc = TM.shift_table(1, 4)
    assert_bit_equal(TM.mix(x, osc, 0), exp, "mix with signed zeros")
    # the phase follows the ABSOLUTE position: the same samples four and five positions on
    assert_bit_equal(TM.mix(x, osc, 4), exp, "mix, one period later")
    assert_bit_equal(TM.mix(x[2:], osc, 1), exp[2:], "mix from position 1")


def test_multiply_by_i_shortcut_changes_bits():
    """Why the device computes every mix in full: for an oscillator entry (+0, 1) the shortcut `x * i = (-im, re)` and the
    formula differ in the sign of zero -- and the parity contract compares bits."""
    x = _f32([0x40000000, 0x00000000])                      # (2, +0)
    full = TM.mix(x, _f32([0x00000000, 0x3F800000]), 0)     # (2*+0 - +0*1, 2*1 + +0*+0) = (+0 - +0, 2 + +0) = (+0, 2)
    short = TM.mix_by_i_shortcut(x)                         # (-(+0), 2) = (-0, 2)
    assert_bit_equal(full, _f32([0x00000000, 0x40000000]), "the formula")
    assert_bit_equal(short, _f32([0x80000000, 0x40000000]), "the shortcut")
    assert full.view(np.uint32)[0] != short.view(np.uint32)[0]
    assert np.array_equal(full, short)                      # equal as numbers, different as bits


def test_argument_errors_need_no_device(L):
    lib = L.lib
    taps = np.ones(16, np.float32)
    osc = TM.shift_table(1, 4)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    h = C.c_void_p()
    for period in (0, -3, 65537):
        assert lib.sdrhip_tuner_create(C.byref(h), L.ORDER_AVX, 8, fp(taps), taps.size, fp(osc), period) == ERR_ARG
        assert not h
    assert lib.sdrhip_tuner_create(C.byref(h), L.ORDER_AVX, 8, fp(taps), taps.size, None, 4) == ERR_ARG
    assert lib.sdrhip_tuner_create(C.byref(h), L.ORDER_AVX, 8, None, taps.size, fp(osc), 4) == ERR_ARG
    assert lib.sdrhip_tuner_create(C.byref(h), 7, 8, fp(taps), taps.size, fp(osc), 4) == ERR_ARG
    assert lib.sdrhip_tuner_create(None, L.ORDER_AVX, 8, fp(taps), taps.size, fp(osc), 4) == ERR_ARG
    # null handles
    assert lib.sdrhip_tuner_num_coeffs(None) == ERR_ARG and lib.sdrhip_tuner_factor(None) == ERR_ARG and lib.sdrhip_tuner_period(None) == ERR_ARG
    assert lib.sdrhip_tuner_run(None, None, None, 0, None, 0, 8, 0) == ERR_ARG
    assert lib.sdrhip_tuner_run_u8(None, None, None, 0, None, 0, 8, 0) == ERR_ARG
    assert lib.sdrhip_tuner_set_route(None, 0) == ERR_ARG
    assert lib.sdrhip_pipe_tuner(C.byref(C.c_void_p()), None, 512) == ERR_ARG
    assert lib.sdrhip_tuner_shift_table(1, 0, fp(osc)) == ERR_ARG and lib.sdrhip_tuner_shift_table(1, 4, None) == ERR_ARG
    # a descriptor is host data until its first run: created, queried and refused here without a device
    t = L.Tuner(8, taps, osc)
    assert (t.num_coeffs, t.period, t.factor) == (16, 4, 8) and lib.sdrhip_tuner_factor(t.h) == 8
    assert L.Tuner(8, np.ones(13, np.float32), osc, L.ORDER_AVX).num_coeffs == 16 and L.Tuner(8, np.ones(13, np.float32), osc, L.ORDER_SSE).num_coeffs == 14
    one = C.c_void_p(256)                                   # never dereferenced: every call below is refused first
    assert lib.sdrhip_tuner_run(t.h, None, one, 0, one, 0, 8, 15) == ERR_ARG        # seam block shorter than the filter
    assert lib.sdrhip_tuner_run_u8(t.h, None, one, 0, one, 0, 8, 15) == ERR_ARG
    assert lib.sdrhip_tuner_run(t.h, None, one, 8, one, 0, 8, 0) == ERR_ARG         # first window before d_in
    assert lib.sdrhip_tuner_run(t.h, None, one, 0, one, 8, 0, 0) == ERR_ARG         # k_end < k_begin
    assert lib.sdrhip_tuner_run(t.h, None, None, 0, one, 0, 8, 0) == ERR_ARG        # null input
    assert lib.sdrhip_tuner_run(t.h, None, one, 0, one, 5, 5, 0) == 0               # an empty range is no work
    assert lib.sdrhip_tuner_set_route(t.h, 3) == ERR_ARG and lib.sdrhip_tuner_set_route(t.h, -1) == ERR_ARG
    for r in (2, 1, 0):
        assert lib.sdrhip_tuner_set_route(t.h, r) == 0
    t.close()
