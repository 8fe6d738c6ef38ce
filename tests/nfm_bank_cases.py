"""The cases of the narrow-band FM bank's tests (tests/test_nfm_bank_cases.py, tests/test_gpu_nfm_bank.py, tests/test_gpu_pipe_nfm_bank.py):
the streams, cuts and tables of tests/tuner_bank_cases.py, tests/tuner_i16_cases.py and tests/am_bank_cases.py, and each channel's
expected output from the models alone -- the restated firDecimator Pipe on the stream mixed with the channel's table
(tests/tuner_model.py), then oracle.fm_demod -- computed once, shared and never written.  fmDemod carries only the last sample, so
a launch over [k0, k1) from the state y[k0 - 1] is the slice [k0, k1) of fm_demod over the whole row.  TEST INFRASTRUCTURE ONLY."""
import os
import re

import numpy as np

import am_bank_cases as AC
import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from oracle import pipes_model as PM

B, NBLK, K_ALL = BC.B, BC.NBLK, BC.K_ALL
FORMATS = AC.FORMATS
LP = 128                                         # the 127 taps, prepared


def tile_outputs():
    """T::OUTS of the bank's tile kernel, read from the code."""
    return AC.tile_outputs()


def tile_advance():
    """Outputs an OUT_FM tile advances by, read from the code: T::OUTS - (the overlap)."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "sdr_amd", "csrc", "kernels_tuner_bank.hip")).read()
    m = re.search(r"tile_advance\(\) \{ return OUT == OUT_FM \? T::OUTS - (\d+) : T::OUTS; \}", src)
    if m is None:
        # a tree without the fmDemod form (the model-only tests hold there too) has no advance to read; a tree WITH it whose line this
        # pattern no longer matches must not quietly fall back to a number written here
        assert "OUT_FM" not in src, "kernels_tuner_bank.hip has the OUT_FM form but tile_advance() was not found: update this pattern"
        return None
    return tile_outputs() - int(m.group(1))


OUTS = tile_outputs()
ADV = tile_advance() or OUTS - 2                 # (on a tree without the form: the issue's design, for the model-only tests)
# a launch end at advance - 1, advance, advance + 1, the tile's output count and two advances + 1 (and the one-output launch)
COUNTS = [1, ADV - 1, ADV, ADV + 1, OUTS, 2 * ADV + 1]
ODD_CUTS3 = [1009, 3001]                         # the whole stream as three runs
ODD_CUTS5 = [1, 1009, 1023, 3001]                # ... and as five: a run of ONE output, a run that is all Cross at seam B
# the +-1 table: +1 on entries 0 .. 7, -1 on 8 .. 15.  At factor 8 a constant input gives y[k] = -y[k - 1] exactly
PM1 = np.array([1.0, 0.0] * 8 + [-1.0, 0.0] * 8, np.float32)
# the directed u8 stream: the seeded one with a silent stretch (byte 128: all-zero windows) at the launch's start and across the
# first tile edge, and a constant stretch (200, 128) across the second tile edge
SILENT = [(0, 600), (ADV * 8 - 180, ADV * 8 + 320)]
CONST = (2 * ADV * 8 - 260, 2 * ADV * 8 + 340)

_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def directed_u8():
    if "du8" not in _cache:
        u = T.stream_u8().copy()
        for a, b in SILENT:
            u[2 * a:2 * b] = 128
        u[2 * CONST[0]:2 * CONST[1]:2] = 200
        u[2 * CONST[0] + 1:2 * CONST[1]:2] = 128
        _cache["du8"] = _frozen(u)
    return _cache["du8"]


def directed_tables():
    return [PM1, BC.IDENTITY, T.osc_table(1000)]


def inside(stretch, factor=8, lp=LP):
    """Outputs whose whole window lies in the sample stretch [a, b)."""
    a, b = stretch
    return np.arange(-(-a // factor), (b - lp) // factor + 1)


def expected_iq(oracle, table, seam, fmt, factor=8, stream="seeded"):
    """Channel's complex row: the tuner model on oracle.convert_u8 / convert_i16 of the stream (cfloat input IS the converted u8)."""
    key = ("iq", np.asarray(table, np.float32).tobytes(), seam, fmt == "i16", factor, stream)
    if key not in _cache:
        if stream == "seeded" and factor == 8:
            _cache[key] = AC.expected_iq(oracle, table, seam, fmt)
        else:
            x = oracle.convert_i16(IC.stream_i16()) if fmt == "i16" else oracle.convert_u8(directed_u8() if stream == "directed" else T.stream_u8())
            _cache[key] = _frozen(TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, factor, x, table, seam, 0, block_out=1))
    return _cache[key]


def demod(oracle, iq, state=(0.0, 0.0)):
    return oracle.fm_demod(iq, last=(float(state[0]), float(state[1])))


def expected(oracle, table, seam, fmt, factor=8, stream="seeded"):
    """fmDemod of the channel's row over the WHOLE stream from (0, 0)."""
    key = ("fm", np.asarray(table, np.float32).tobytes(), seam, fmt == "i16", factor, stream)
    if key not in _cache:
        _cache[key] = _frozen(demod(oracle, expected_iq(oracle, table, seam, fmt, factor, stream)))
    return _cache[key]


def state_before(oracle, table, seam, fmt, k, factor=8, stream="seeded"):
    """The channel's decimated output k - 1 as (re, im): the state in front of output k; (0, 0) in front of the stream."""
    if k == 0:
        return np.zeros(2, np.float32)
    return expected_iq(oracle, table, seam, fmt, factor, stream)[2 * (k - 1):2 * k]


def nonfinite_expected(oracle, table, seam):
    """The converted u8 stream with re = +Inf at sample AC.INF_AT and im = NaN at AC.NAN_AT: (complex row, its fmDemod)."""
    key = ("nf", np.asarray(table, np.float32).tobytes(), seam)
    if key not in _cache:
        iq = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, AC.nonfinite_stream(oracle), table, seam, 0, block_out=1)
        _cache[key] = (_frozen(iq), _frozen(demod(oracle, iq)))
    return _cache[key]
