"""The general fused audio tail (sdrhip_audio_tail_general_fits / _set_general / sdrhip_debug_audio_tail_general_launches) on a host
without a GPU: the names are declared, exported and bound; the predicate says yes to every shape the kernel must serve, with 64, 32
and 8 half-taps and at every block the tail's create admits, and no to the outsiders; set_general refuses what it must; the existing
routes keep their meaning (route 3 is still refused, fused_fits is still k_audio_tail_rows' fit).  What the kernel COMPUTES is held
to the restated Pipes on the device (tests/test_gpu_audio_tail_any.py)."""
import ctypes as C
import os

import numpy as np
import pytest

import audio_tail_any_cases as AC
import signals as S

OK, ERR_ARG = 0, -1
NEW_SYMBOLS = ["sdrhip_audio_tail_general_fits", "sdrhip_audio_tail_set_general", "sdrhip_debug_audio_tail_general_launches",
               "sdrhip_pipe_narrow_bank_audio"]
P = [0x10000, 0x20000, 0x30000]                          # never dereferenced: every call below is refused (or empty) first


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def tail(L, shape, block=0, nhalf=None, order=None):
    half = {64: S.taps_audio_half64(), 32: S.taps_audio_half32(), 8: S.taps_audio_half32()[:8]}[nhalf or shape.nhalf]
    return L.AudioTail(shape.I, shape.D, shape.resamp_taps(), half, gain=1.0, block=block, order=L.ORDER_AVX if order is None else order)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.audio_tail_general_launches() >= 0
    for m in ("general_fits", "set_general"):
        assert callable(getattr(L.AudioTail, m))
    assert callable(L.Pipe.narrow_bank_audio)
    assert (L.AUDIO_TAIL_GENERAL_AUTO, L.AUDIO_TAIL_GENERAL_ALWAYS, L.AUDIO_TAIL_GENERAL_NEVER) == (0, 1, 2)


@pytest.mark.parametrize("shape", list(AC.SHAPES.values()), ids=list(AC.SHAPES))
def test_every_must_serve_shape_fits_with_64_32_and_8_half_taps(L, shape):
    for nhalf in AC.HALF_COUNTS:
        lowest = max(-(-shape.rlp // shape.I), 2 * nhalf)
        for block in (0, lowest, 128, 129, 200, 250, 256, 1000, 8192, 1 << 27):
            if block and block < lowest:
                continue
            t = tail(L, shape, block, nhalf)
            assert t.general_fits() and AC.general_fits(shape, block, nhalf), (shape.name, nhalf, block)
            shp = (C.c_int32 * 4)()
            assert L.lib.sdrhip_audio_tail_shape(t.h, shp) == OK and list(shp) == [shape.I, shape.D, shape.rlp, 2 * nhalf]
        assert not tail(L, shape, (1 << 27) + 1, nhalf).general_fits(), "positions inside a buffer are 32-bit"
        # there is no tighter lower bound than create's: one below it there is no tail to ask
        h = C.c_void_p()
        r, a = shape.resamp_taps(), S.taps_audio_half64()[:nhalf] if nhalf == 64 else S.taps_audio_half32()[:nhalf]
        assert L.lib.sdrhip_audio_tail_create(C.byref(h), L.ORDER_AVX, shape.I, shape.D, L._fp(r), r.size, L._fp(a), a.size, 1.0, lowest - 1) == ERR_ARG
    # only the FM shape with 64 half-taps is k_audio_tail_rows': fused_fits keeps its meaning
    assert tail(L, shape, 0).fused_fits() == (shape.name == "3/10 x 191")
    assert not tail(L, shape, 256).fused_fits()


def test_the_outsiders(L):
    s45 = AC.SHAPES["4/5 x 63"]
    assert not tail(L, s45, 0, order=L.ORDER_SSE).general_fits(), "the SSE order"
    h64, h32 = S.taps_audio_half64(), S.taps_audio_half32()

    def make(I, D, ntaps, half, block=0):
        taps = (I * S.windowed_sinc(ntaps, 1.0 / max(I, D))).astype(np.float32)
        return L.AudioTail(I, D, taps, half, gain=1.0, block=block)
    assert make(8, 9, 511, h64).general_fits() and not make(9, 10, 511, h64).general_fits(), "interpolation 9"
    assert make(1, 5, 63, h64).general_fits() and not make(1, 5, 71, h64).general_fits(), "a 72-float polyphase group"
    assert make(4, 5, 255, h64).general_fits() and not make(4, 5, 263, h64).general_fits(), "a 72-float polyphase group, I = 4"
    # a longer filter: the AVX order takes half-taps in eights, so the first length behind 128 prepared taps is 144 (136 is refused
    # by the filter's own create)
    half72 = np.concatenate([h64, h32[:8]])
    assert not make(4, 5, 63, half72).general_fits(), "a 144-tap filter"
    h = C.c_void_p()
    r = s45.resamp_taps()
    half68 = np.concatenate([h64, h32[:4]])
    assert L.lib.sdrhip_audio_tail_create(C.byref(h), L.ORDER_AVX, 4, 5, L._fp(r), r.size, L._fp(half68), 68, 1.0, 0) == ERR_ARG and not h
    # numCoeffsR < decimation: create allows it on a contiguous stream only (1/9 with 7 taps: 8 prepared taps)
    assert not make(1, 9, 7, h64).general_fits(), "Lp < D"
    assert make(1, 5, 7, h64).general_fits()
    # interpolation and decimation with a common factor: the polyphase cycle is shorter than I outputs
    assert not make(2, 4, 63, h64).general_fits() and not make(6, 8, 63, h32).general_fits()
    # a y window longer than a tile's: decimation / interpolation beyond about 5
    assert make(1, 5, 39, h64).general_fits() and not make(1, 6, 39, h64).general_fits() and not make(3, 16, 191, h64).general_fits()
    assert L.lib.sdrhip_audio_tail_general_fits(None) == ERR_ARG


def test_set_general_refuses_and_the_routes_keep_their_meaning(L):
    t = tail(L, AC.SHAPES["4/5 x 63"], 256)
    for mode in (-1, 3, 7):
        assert L.lib.sdrhip_audio_tail_set_general(t.h, mode) == ERR_ARG
        assert b"sdrhip_audio_tail_set_general" in L.lib.sdrhip_last_error()
    assert L.lib.sdrhip_audio_tail_set_general(None, 1) == ERR_ARG
    for mode in (0, 1, 2):
        assert L.lib.sdrhip_audio_tail_set_general(t.h, mode) == OK
    for route in (-1, 3):
        assert L.lib.sdrhip_audio_tail_set_route(t.h, route) == ERR_ARG
    # route 1 is k_audio_tail_rows or a refusal, whatever the general mode says; every refusal comes before any pointer is looked at
    n_y = 4000
    q1 = t.ready(n_y)
    assert q1 > 2000 and not t.fused_fits() and t.general_fits()
    for mode in (0, 1, 2):
        t.set_general(mode)
        t.set_route(1)
        rc = L.lib.sdrhip_audio_tail_run_rows(t.h, None, P[0], n_y, 0, n_y, P[1], q1, 3, 0, q1, None, 0)
        assert rc == ERR_ARG and b"route 1" in L.lib.sdrhip_last_error()
        # routes 0 and 2 ask for the workspace whichever way auto goes, the general kernel included
        for route in (0, 2):
            t.set_route(route)
            c0 = L.audio_tail_general_launches()
            for ws, nbytes in ((None, 0), (P[2], t.workspace_bytes(3, n_y) - 1)):
                rc = L.lib.sdrhip_audio_tail_run_rows(t.h, None, P[0], n_y, 0, n_y, P[1], q1, 3, 0, q1, ws, nbytes)
                assert rc == ERR_ARG and b"sdrhip_audio_tail_run_rows" in L.lib.sdrhip_last_error(), (mode, route)
            rc = L.lib.sdrhip_audio_tail_run_rows(t.h, None, P[0], n_y, 0, n_y - 1, P[1], q1, 3, 0, q1, P[2], 1 << 30)
            assert rc == ERR_ARG, "a receptive field behind the buffer"
            assert L.lib.sdrhip_audio_tail_run_rows(t.h, None, None, 0, 0, 0, None, 0, 3, 7, 7, None, 0) == OK      # an empty range
            assert L.audio_tail_general_launches() == c0


def test_the_narrow_audio_pipe_refuses_before_the_engine_creates_a_stream(L):
    """sdrhip_pipe_narrow_bank_audio: a null bank, a null tail, a tail of block 0, a block_mid shorter than the second filter plus its
    factor and an input type out of range are refused -- under the call's own name, *p = NULL -- on a host without a device."""
    import narrow_bank_cases as NB
    taps, d2, lp2 = NB.SHAPES["61/5"]
    tb = L.TunerBank(8, S.taps_decim127(), [L.tuner_shift_table(1, 64), L.tuner_shift_table(-3, 64)])
    nb = L.NarrowBank(tb, L.Decimator(d2, taps, complex_=True), NB.ENV, True)
    s25 = AC.SHAPES["2/5 x 127"]
    t200, t0 = tail(L, s25, 200), tail(L, s25, 0)
    assert lp2 + d2 == 69
    for what, args in (("a null bank", (None, t200.h, 1000, 0)), ("a null tail", (nb.h, None, 1000, 0)), ("a tail of block 0", (nb.h, t0.h, 1000, 0)),
                       ("block_mid 68 < 64 + 5", (nb.h, t200.h, 68, 0)), ("input_type 3", (nb.h, t200.h, 1000, 3)),
                       ("input_type -1", (nb.h, t200.h, 1000, -1))):
        h = C.c_void_p(0xdead)
        assert L.lib.sdrhip_pipe_narrow_bank_audio(C.byref(h), *args) == ERR_ARG and not h.value, what
        assert b"sdrhip_pipe_narrow_bank_audio" in L.lib.sdrhip_last_error(), what
    assert L.lib.sdrhip_pipe_narrow_bank_audio(None, nb.h, t200.h, 1000, 0) == ERR_ARG
