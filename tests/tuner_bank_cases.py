"""The cases of the tuner bank's tests (tests/test_tuner_bank_abi.py, tests/test_gpu_tuner_bank.py): the stream, cuts and tables of
tests/test_gpu_tuner.py arranged as banks, and each table's expected outputs from the model (tests/tuner_model.py), computed once,
shared and never written.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import signals as S
import test_gpu_tuner as T
import tuner_model as TM
from oracle import pipes_model as PM

B, NBLK, CUTS, PERIODS = T.B, T.NBLK, T.CUTS, T.PERIODS
K_ALL = (NBLK * B - 128) // 8 + 1                 # 5105 outputs: ten tiles of 512, the last ragged
IDENTITY = np.array([1.0, 0.0], np.float32)       # a channel on the centre frequency
# the table of test_gpu_tuner.py::test_user_table_with_subnormals_and_negative_zeros (period 7)
SUBNORMALS = np.array([1e-42, -3e-39, -0.0, 1.0, 0.0, -0.0, 0.70710677, -0.70710677, -1.0, 1e-45, 2.5, -0.0, 1e-30, 3.0], np.float32)
FAR_K0 = 3 * 2 ** 30 + 5
FAR_CUTS = [1000, 1019]


def bank_tables(nch):
    """1 channel: period 1000.  3: period 1000, the centre, the subnormal table.  More: the periods of test_gpu_tuner.py in turn, so
    that neighbouring channels never share a period, with the centre as channel 3 and the subnormal table as channel 10."""
    if nch == 1:
        return [T.osc_table(1000)]
    ts = [T.osc_table(PERIODS[j % len(PERIODS)]) for j in range(nch)]
    if nch == 3:
        return [T.osc_table(1000), IDENTITY, SUBNORMALS]
    ts[3], ts[10] = IDENTITY, SUBNORMALS
    return ts


_cache = {}


def expected(oracle, table, seam):
    """Every output of the 5-block u8 stream through a /8 tuner of 127 taps with this table."""
    key = (np.asarray(table, np.float32).tobytes(), seam)
    if key not in _cache:
        x = oracle.convert_u8(T.stream_u8())
        e = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, x, table, seam, 0, block_out=1)
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


def straddlers(seam, n_out, lp=128, factor=8):
    """Outputs below n_out whose window crosses a multiple of seam: the Cross outputs of the stream."""
    m = np.arange(n_out, dtype=np.int64)
    v = m * factor
    return m[(v // seam) != ((v + lp - 1) // seam)]
