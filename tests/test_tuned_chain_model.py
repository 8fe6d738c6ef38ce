"""The FM chain with a tuner, without a GPU: the restated Pipes with the oscillator stage (tests/tuned_chain_model.py) against the
plain receiver, and the C ABI of sdrhip_fm_chain_set_tuner on a chain created on the host."""
import ctypes as C
import os

import numpy as np
import pytest

import signals as S
import tuned_chain_model as TCM
import tuner_model as TM
from conftest import assert_bit_equal
from oracle import pipes_model as PM

B = 8192
NBLK = 24
# 24 source blocks are 7372 resampler outputs: less than one 8192-sample audio block.  fm_receiver's `block` is the blockSizeOut of
# its four Pipes, whatever the source delivers; at 512 the same 24 source blocks of 8192 samples yield 13 audio blocks.
BLOCK_OUT = 512
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _blocks():
    u8 = S.iq_u8_fm(NBLK * B)
    return [u8[2 * i * B:2 * (i + 1) * B] for i in range(NBLK)]


def _cat(blocks):
    return np.concatenate(blocks) if blocks else np.zeros(0, np.float32)


def _tuned(oracle, osc, **kw):
    return _cat(TCM.fm_receiver_tuned(oracle, _blocks(), osc, S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(),
                                      0.2, BLOCK_OUT, PM.ORDER_AVX, **kw))


def _plain(oracle):
    """The untuned receiver on the same 24 blocks (computed once, shared, never written)."""
    if "plain" not in _cache:
        e = _cat(PM.fm_receiver(oracle, _blocks(), S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(), 0.2, BLOCK_OUT, PM.ORDER_AVX))
        e.setflags(write=False)
        _cache["plain"] = e
    return _cache["plain"]


def test_identity_table_is_the_plain_receiver(oracle):
    """(1, +0): a converted u8 sample is never -0, so x*1 - y*0 and x*0 + y*1 give x and y back, bit for bit."""
    exp = _plain(oracle)
    assert exp.size == 13 * BLOCK_OUT
    assert_bit_equal(_tuned(oracle, np.array([1.0, 0.0], np.float32)), exp, "identity table vs fm_receiver")


def test_quarter_band_shift_changes_the_audio(oracle):
    got = _tuned(oracle, TM.shift_table(1, 4))
    exp = _plain(oracle)
    assert got.shape == exp.shape
    assert (got.view(np.uint32) != exp.view(np.uint32)).mean() > 0.5


def test_phase_follows_the_absolute_stream_index(oracle):
    """Period 1000 does not divide the 8192-sample block: every block starts at another phase.  Mixing block by block equals mixing
    the whole stream once."""
    osc = TM.shift_table(-3, 1000)
    assert B % 1000 != 0
    by_block = _tuned(oracle, osc)
    whole = _tuned(oracle, osc, mix_whole_stream=True)
    assert by_block.size > 0
    assert_bit_equal(by_block, whole, "mixed per block vs mixed as one stream")
    # ... and it is not what a table restarted at every block would give
    restarted = [TM.mix(S.cfloat_block(B, seed=3), osc, 0), TM.mix(S.cfloat_block(B, seed=3), osc, B)]
    assert not np.array_equal(restarted[0], restarted[1])


# ---- the C ABI, on a host without a GPU as well --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


NEW_SYMBOLS = ["sdrhip_fm_chain_set_tuner", "sdrhip_fm_chain_tuner_period", "sdrhip_debug_small_chain_tuned_launches"]


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
    assert L.lib.sdrhip_debug_small_chain_tuned_launches.restype is C.c_longlong
    assert L.small_chain_tuned_launches() >= 0


def _chain(L):
    return L.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, B)


def test_set_tuner_argument_errors(L):
    ERR_ARG = -1
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ch = _chain(L)
    ok = TM.shift_table(1, 4)
    f = L.lib.sdrhip_fm_chain_set_tuner
    assert f(None, fp(ok), 4) == ERR_ARG                                  # a null chain
    assert b"sdrhip_fm_chain_set_tuner" in L.lib.sdrhip_last_error()
    assert f(ch.h, None, 4) == ERR_ARG                                    # a null table with a period
    assert f(ch.h, fp(ok), 0) == ERR_ARG                                  # a table without one
    assert f(ch.h, fp(ok), -1) == ERR_ARG
    big = np.zeros(2 * 65537, np.float32)
    assert f(ch.h, fp(big), 65537) == ERR_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for at in (0, 3, 7):
            t = ok.copy()
            t[at] = bad
            assert f(ch.h, fp(t), 4) == ERR_ARG, (bad, at)
    assert ch.tuner_period() == 0, "a refused table must leave the chain as it was"
    assert L.lib.sdrhip_fm_chain_tuner_period(None) == ERR_ARG
    with pytest.raises(L.SdrHipError):
        ch.set_tuner(np.zeros(3, np.float32))                             # not whole pairs
    assert f(ch.h, fp(big), 65536) == 0 and ch.tuner_period() == 65536   # the longest table


def test_tuner_period_and_workspace_on_the_host(L):
    """Set, replace and remove on a chain that never saw a device: the period is reported, a tuned chain reserves the mixed samples
    (8 bytes per input sample) and a chain that lost its tuner sizes its workspace as one that never had one."""
    ch, never = _chain(L), _chain(L)
    sizes = (0, B, 1 << 20)
    plain = [int(never.workspace_bytes(n)) for n in sizes]
    assert ch.tuner_period() == 0
    ch.set_tuner(TM.shift_table(1, 4))
    assert ch.tuner_period() == 4
    tuned = [int(ch.workspace_bytes(n)) for n in sizes]
    for n, a, b in zip(sizes, plain, tuned):
        assert b >= a + 8 * n, (n, a, b)
    ch.set_overlap(True)
    assert [int(ch.workspace_bytes(n)) for n in sizes] == [2 * ((b + 255) // 256 * 256) for b in tuned]
    ch.set_overlap(False)
    ch.set_tuner(TM.shift_table(-3, 1000))
    assert ch.tuner_period() == 1000
    # planning is counted in input samples: the tuner changes none of it
    total = 40 * B
    assert ch.plan(0, total, total) == never.plan(0, total, total) and ch.max_halo() == never.max_halo()
    assert ch.plan(5 * B, 9 * B, total) == never.plan(5 * B, 9 * B, total) and ch.halo_samples() == never.halo_samples()
    ch.set_tuner(None)
    assert ch.tuner_period() == 0
    assert [int(ch.workspace_bytes(n)) for n in sizes] == plain
    # a first stage that converts into the workspace anyway (decimation 5): the tuned chain mixes into the same region
    d5 = L.FmChain(5, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, B)
    before = [int(d5.workspace_bytes(n)) for n in sizes]
    d5.set_tuner(TM.shift_table(1, 4))
    assert [int(d5.workspace_bytes(n)) for n in sizes] == before
