"""The cases of the AM bank's tests (tests/test_am_bank_cases.py, tests/test_gpu_am_bank.py): the streams, cuts and tables of
tests/tuner_bank_cases.py and tests/tuner_i16_cases.py, and each channel's expected audio from the models alone -- the restated Pipe on
the stream mixed with the channel's table (tests/tuner_model.py), then agc_model.magnitude (Data.Complex.magnitude at Float), then
the oracle's dcBlocker from (0, 0) -- computed once, shared and never written.  TEST INFRASTRUCTURE ONLY."""
import os
import re

import numpy as np

import agc_model as AM
import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from oracle import pipes_model as PM

B, NBLK, CUTS, K_ALL = BC.B, BC.NBLK, BC.CUTS, BC.K_ALL
FORMATS = ("cf32", "u8", "i16")
ODD_CUTS = [1, 1009, 1024, 3001]                 # cuts at odd outputs: the rows of the later launches start 4 bytes off 8-byte alignment
K0_CROSS = 1009                                  # the first Cross output of the seamed stream: a run of ONE output there is all Cross
# samples of the non-finite case: re = +Inf (at a phase where no entry of the period-1000 and period-5 tables has a zero part), im = NaN
INF_AT, NAN_AT = 3001, 20003


def tile_outputs():
    """T::OUTS of the bank's tile kernel, read from the code: NT threads x R outputs."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_amd", "csrc", "kernels_tuner_bank.hip")).read()
    m = re.search(r"constexpr int R = (\d+), NT = (\d+);", src)
    return int(m.group(1)) * int(m.group(2))


OUTS = tile_outputs()
COUNTS = [1, OUTS - 1, OUTS, OUTS + 1, 3 * OUTS - 1]

_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def envelope(iq):
    iq = np.asarray(iq, np.float32)
    return AM.magnitude(iq[0::2], iq[1::2])


def expected_iq(oracle, table, seam, fmt):
    """The tuner bank's expected complex row: cfloat input is the converted u8 stream, so it shares the u8 row."""
    return IC.expected(oracle, table, seam) if fmt == "i16" else BC.expected(oracle, table, seam)


def expected_env(oracle, table, seam, fmt):
    key = ("env", np.asarray(table, np.float32).tobytes(), seam, fmt == "i16")
    if key not in _cache:
        _cache[key] = _frozen(envelope(expected_iq(oracle, table, seam, fmt)))
    return _cache[key]


def expected_audio(oracle, table, seam, fmt):
    """dcBlocker of the envelope over the WHOLE stream from (0, 0): (audio, final lastSample, final lastOutput)."""
    key = ("dc", np.asarray(table, np.float32).tobytes(), seam, fmt == "i16")
    if key not in _cache:
        y, fs, fo = oracle.dc_blocker(expected_env(oracle, table, seam, fmt), 0.0, 0.0)
        _cache[key] = (_frozen(y), np.float32(fs), np.float32(fo))
    return _cache[key]


def expected(oracle, table, seam, fmt, dc):
    return expected_audio(oracle, table, seam, fmt)[0] if dc else expected_env(oracle, table, seam, fmt)


def state_before(oracle, table, seam, fmt, k):
    """dcBlocker's (lastSample, lastOutput) in front of output k of the stream."""
    if k == 0:
        return np.zeros(2, np.float32)
    return np.array([expected_env(oracle, table, seam, fmt)[k - 1], expected_audio(oracle, table, seam, fmt)[0][k - 1]], np.float32)


def nonfinite_stream(oracle):
    """The converted u8 stream with re = +Inf at sample INF_AT and im = NaN at sample NAN_AT."""
    if "nf" not in _cache:
        x = oracle.convert_u8(T.stream_u8()).copy()
        x[2 * INF_AT] = np.inf
        x[2 * NAN_AT + 1] = np.nan
        _cache["nf"] = _frozen(x)
    return _cache["nf"]


def nonfinite_expected(oracle, table, seam, dc):
    key = ("nfe", np.asarray(table, np.float32).tobytes(), seam)
    if key not in _cache:
        iq = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, nonfinite_stream(oracle), table, seam, 0, block_out=1)
        env = envelope(iq)
        _cache[key] = (_frozen(env), _frozen(oracle.dc_blocker(env, 0.0, 0.0)[0]))
    return _cache[key][1 if dc else 0]


SPARSE_SAMPLES = 2 * B
SPARSE_OUT = (SPARSE_SAMPLES - 128) // 8 + 1     # 2033 outputs


def sparse_stream():
    """cfloat, two blocks: (1, 0) at every 7th sample of the first 6000 -- where the subnormal table (period 7) holds its entry 0,
    (1e-42, -3e-39) -- and at every sample = 2 (mod 7) of samples 6000 .. 9000 -- entry 2, (0, -0); zeros elsewhere.  Every product under
    the FIR sum is subnormal or a signed zero."""
    if "sparse" not in _cache:
        x = np.zeros(2 * SPARSE_SAMPLES, np.float32)
        x[2 * np.arange(0, 6000, 7)] = 1.0
        x[2 * np.arange(6001 - 6001 % 7 + 2, 9000, 7)] = -1.0
        _cache["sparse"] = _frozen(x)
    return _cache["sparse"]


def sparse_expected_iq(oracle, table, seam):
    key = ("sparse", np.asarray(table, np.float32).tobytes(), seam)
    if key not in _cache:
        _cache[key] = _frozen(TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, sparse_stream(), table, seam, 0, block_out=1))
    return _cache[key]


def window_outputs(sample, n_out=K_ALL, lp=128, factor=8):
    """Outputs whose 128-sample window holds this sample."""
    m = np.arange(n_out, dtype=np.int64)
    return m[(m * factor <= sample) & (sample < m * factor + lp)]
