"""The cases of the 16-bit tests (tests/test_tuner_i16_abi.py, tests/test_gpu_tuner_i16.py): the
geometry of tests/test_gpu_tuner.py / tests/tuner_bank_cases.py -- 5 blocks of 8192 samples, 127 taps / 8, 5105 outputs -- on an int16
stream, and each table's expected outputs from the model (tests/tuner_model.py) on the stream oracle.convert_i16 makes of it, computed
once, shared and never written.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import signals as S
import tuner_bank_cases as BC
import tuner_model as TM
from oracle import pipes_model as PM

B, NBLK, CUTS, K_ALL = BC.B, BC.NBLK, BC.CUTS, BC.K_ALL
FORCED = (-32768, 32767, 0, 1, -1, 2047, -2047, 2048, -2048)

_cache = {}


def stream_i16(nsamples=NBLK * B, seed=1601):
    """Seeded int16 IQ, uniform over the whole int16 range, block 2 drawn from -2048 .. 2047 (a BladeRF's real range), and FORCED put
    into a few dozen positions: the five elements either side of every block edge, the first and last elements and seeded ones."""
    key = ("i16", nsamples, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        s = rng.integers(-32768, 32768, 2 * nsamples, dtype=np.int64).astype(np.int16)
        if nsamples >= 3 * B:
            s[2 * 2 * B:2 * 3 * B] = rng.integers(-2048, 2048, 2 * B).astype(np.int16)
        pos = [int(p) for p in rng.integers(0, 2 * nsamples, 36)]
        for e in range(B, nsamples, B):
            pos += list(range(2 * e - 5, 2 * e + 5))
        pos += [0, 1, 2, 2 * nsamples - 2, 2 * nsamples - 1]
        for i, p in enumerate(pos):
            s[p] = FORCED[i % len(FORCED)]
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def expected(oracle, table, seam, factor=8, taps=None, i16=None, pos0=0):
    """Every output of the int16 stream (default: the 5-block one through the /8 tuner of 127 taps) with this table."""
    i16 = stream_i16() if i16 is None else i16
    taps = S.taps_decim127() if taps is None else taps
    key = ("exp", np.asarray(table, np.float32).tobytes(), seam, factor, taps.tobytes(), i16.size, i16[:64].tobytes(), pos0)
    if key not in _cache:
        e = TM.tuner_expected(oracle, taps, PM.ORDER_AVX, factor, oracle.convert_i16(i16), table, seam, pos0, block_out=1)
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]
