"""The cases of the narrow-channel bank's tests (tests/test_narrow_bank_cases.py, tests/test_gpu_narrow_bank.py): stage 1 is the
128-tap / 8 fixture with the streams and tables of tests/tuner_bank_cases.py, tests/tuner_i16_cases.py and tests/am_bank_cases.py;
stage 2 is one of three seeded real-tap decimators on complex data.  Each channel's expected row comes from the models alone -- the
restated firDecimator Pipe (oracle/pipes_model.py) on the stream mixed with the channel's table (tests/tuner_model.py), the same
Pipe once more on that row in blocks of seam_block2, then agc_model.magnitude [and the oracle's dcBlocker] or oracle.fm_demod --
computed once, shared and never written.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import am_bank_cases as AC
import nfm_bank_cases as NC
import signals as S
import tuner_bank_cases as BC
import tuner_model as TM
from oracle import pipes_model as PM

B, K_ALL = BC.B, BC.K_ALL                        # stage 1: 8192-sample blocks, 5105 outputs of the 5-block stream
D1, LP1 = 8, 128
FORMATS = AC.FORMATS
ENV, FM = 0, 1
TILE = 256                                       # threads = outputs a tile of k_narrow_rows computes (the FM form advances by TILE - 1)


def _seeded_taps(n, seed):
    r = np.random.RandomState(seed)
    return (r.standard_normal(n) / np.sqrt(n)).astype(np.float32)


# name -> (taps, D2, Lp2): 24 / 4; 61 / 5 (prepared to 64: an odd factor and padded zero taps); 128 / 16 (the fused route's limit)
SHAPES = {"24/4": (_seeded_taps(24, 2401), 4, 24), "61/5": (_seeded_taps(61, 6105), 5, 64), "128/16": (_seeded_taps(128, 12816), 16, 128)}
for _t in SHAPES.values():
    _t[0].setflags(write=False)
# (seam_block, seam_block2) pairs: seam_block2 counts stage-1 outputs; B / D1 = 1024 is the first Pipe's own block, 1000 a block the
# second factor does not divide evenly into windows, "Lp" = the second filter's length: all but one output a block is Cross
SEAM_PAIRS = [(0, 0), (B, 1024), (B, 1000), (0, "Lp"), (B, "Lp")]

_cache = {}


def _frozen(a):
    a.setflags(write=False)
    return a


def seam2_of(shape, seam2):
    return SHAPES[shape][2] if seam2 == "Lp" else seam2


def n_out(shape, n1=K_ALL):
    _, d2, lp2 = SHAPES[shape]
    return (n1 - lp2) // d2 + 1


def stage1_range(shape, k0, k1):
    _, d2, lp2 = SHAPES[shape]
    return (k0 * d2, k0 * d2) if k1 == k0 else (k0 * d2, (k1 - 1) * d2 + lp2)


def decimate2(oracle, shape, iq1, seam2, pos0=0):
    """Stage 2 over the complex row iq1 whose element 0 is stage-1 output pos0 (a multiple of D2): the outputs from pos0 / D2 on,
    the Pipe fed seam2-element buffers (0: one buffer).  tests/tuner_model.py's block cut without its mixer."""
    taps, d2, _ = SHAPES[shape]
    assert pos0 % d2 == 0
    model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=d2)
    m = np.ascontiguousarray(iq1, np.float32)
    if seam2 == 0:
        n = m.size // 2
        return model.one((n - model.num_coeffs) // d2 + 1, m) if n >= model.num_coeffs else np.empty(0, np.float32)
    lead = pos0 % seam2
    assert lead % d2 == 0
    m = np.concatenate([np.zeros(2 * lead, np.float32), m])
    nblk = (m.size // 2) // seam2
    blocks = [m[2 * seam2 * i:2 * seam2 * (i + 1)] for i in range(nblk)]
    rest = m[2 * seam2 * nblk:]
    if rest.size // 2 >= model.num_coeffs:
        blocks.append(rest)
    try:
        out, _ = PM.fir_decimator_pipe(model, blocks, 1)
    except PM.PipeAssert:
        # the reference's Pipe asserts (Filter.hs:586): after a crossover the rest of the next buffer is shorter than the filter.  With
        # blocks of exactly Lp2 that is every factor that does not divide Lp2 -- the 61 / 5 shape.  The product defines such a run by
        # the One / Cross rule all the same; the tests hold its routes to each other there, not to the model
        return None
    y = np.concatenate(out) if out else np.empty(0, np.float32)
    return y[2 * (lead // d2):]


def expected_iq2(oracle, table, shape, seam, seam2, fmt, stream="seeded"):
    """The channel's stage-2 complex row over the whole stream."""
    s2 = seam2_of(shape, seam2)
    key = ("iq2", np.asarray(table, np.float32).tobytes(), shape, seam, s2, fmt == "i16", stream)
    if key not in _cache:
        iq1 = NC.expected_iq(oracle, table, seam, fmt, 8, stream)
        y = decimate2(oracle, shape, iq1, s2)
        _cache[key] = None if y is None else _frozen(y)
    return _cache[key]


def model_defined(shape, seam2):
    """Whether the reference's Pipe runs blocks of seam_block2 through this shape without asserting."""
    _, d2, lp2 = SHAPES[shape]
    s2 = seam2_of(shape, seam2)
    return s2 == 0 or s2 >= lp2 + d2 or s2 % d2 == 0


def demodulate(oracle, iq2, form, dc, fm_state=(0.0, 0.0), dc_state=(0.0, 0.0)):
    if form == FM:
        return NC.demod(oracle, iq2, fm_state)
    env = AC.envelope(iq2)
    return oracle.dc_blocker(env, float(dc_state[0]), float(dc_state[1]))[0] if dc else env


def expected(oracle, table, shape, seam, seam2, fmt, form, dc=False, stream="seeded"):
    """The channel's demodulated row over the WHOLE stream from zero states."""
    key = ("out", np.asarray(table, np.float32).tobytes(), shape, seam, seam2_of(shape, seam2), fmt == "i16", form, bool(dc), stream)
    if key not in _cache:
        iq2 = expected_iq2(oracle, table, shape, seam, seam2, fmt, stream)
        _cache[key] = None if iq2 is None else _frozen(demodulate(oracle, iq2, form, dc))
    return _cache[key]


def fm_state_before(oracle, table, shape, seam, seam2, fmt, k):
    if k == 0:
        return np.zeros(2, np.float32)
    return expected_iq2(oracle, table, shape, seam, seam2, fmt)[2 * (k - 1):2 * k]


def dc_state_before(oracle, table, shape, seam, seam2, fmt, k):
    """dcBlocker's (lastSample, lastOutput) in front of output k."""
    if k == 0:
        return np.zeros(2, np.float32)
    env = expected(oracle, table, shape, seam, seam2, fmt, ENV, False)
    aud = expected(oracle, table, shape, seam, seam2, fmt, ENV, True)
    return np.array([env[k - 1], aud[k - 1]], np.float32)


def cross2(shape, seam2, n=None):
    """Stage-2 outputs below n whose window crosses a multiple of seam_block2: the Cross outputs of stage 2."""
    _, d2, lp2 = SHAPES[shape]
    s2 = seam2_of(shape, seam2)
    n = n_out(shape) if n is None else n
    if s2 == 0:
        return np.empty(0, np.int64)
    return BC.straddlers(s2, n, lp2, d2)


def far_case(oracle, shape, seam, seam2, tables, k_begin, fmt_stream_u8):
    """Stage-2 outputs from k_begin on, computed from a u8 slice whose sample 0 is stream sample in_base = k_begin D2 D1:
    -> (in_base, [per channel stage-2 complex rows])."""
    _, d2, _ = SHAPES[shape]
    s2 = seam2_of(shape, seam2)
    j0 = k_begin * d2
    in_base = j0 * D1
    rows = []
    for t in tables:
        iq1 = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, D1, oracle.convert_u8(fmt_stream_u8), t, seam, in_base, block_out=1)
        rows.append(decimate2(oracle, shape, iq1, s2, j0))
    return in_base, rows
