"""The cases of the FM bank's 16-bit tests (tests/test_fm_bank_i16_cases.py, tests/test_gpu_fm_bank_i16.py,
tests/test_gpu_fm_bank_stream_i16.py): the chain of tests/test_gpu_tuned_chain.py -- /8 with 127 taps, 3/10 with 191 taps, 64 half
taps, gain 0.2, block 8192 -- on ONE int16 stream, tuner_i16_cases.stream_i16 at 96 blocks (seeded, full range, one block in
+-2048, the FORCED values around every block edge); tests take prefixes and slices of it.  The model is tuned_chain_model's
fm_receiver_tuned restated for oracle.convert_i16 blocks.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import signals as S
import tuner_i16_cases as IC
import tuner_model as TM
from oracle import pipes_model as PM

B = 8192
NBLK = 96
GAIN = 0.2
NLOOP = 64                      # floats a resampler output walks
LF = 128                        # the audio filter's taps
IDENTITY = np.array([1.0, 0.0], np.float32)
# test_gpu_tuner.py::test_user_table_with_subnormals_and_negative_zeros
SUBNORMALS = np.array([1e-42, -3e-39, -0.0, 1.0, 0.0, -0.0, 0.70710677, -0.70710677, -1.0, 1e-45, 2.5, -0.0, 1e-30, 3.0], np.float32)

_cache = {}


def stream(nblk=NBLK):
    """The first nblk blocks of THE stream (the FORCED positions are those of the 96-block stream)."""
    return IC.stream_i16(NBLK * B)[:2 * nblk * B]


def _random5():
    return np.random.default_rng(20250).uniform(-1.5, 1.5, 10).astype(np.float32)


TABLES = {
    "shift 1/4": lambda: TM.shift_table(1, 4),
    "shift -3/1000": lambda: TM.shift_table(-3, 1000),
    "shift 5/8313": lambda: TM.shift_table(5, 8312 + 1),
    "random, period 5": _random5,
    "shift 1/65536": lambda: TM.shift_table(1, 65536),
    "subnormals": lambda: SUBNORMALS.copy(),
    "identity": lambda: IDENTITY.copy(),
    "overflow": lambda: overflow_table(),
}
NAMES = list(TABLES)[:7]


def table(name):
    if ("osc", name) not in _cache:
        t = np.ascontiguousarray(TABLES[name](), np.float32)
        t.setflags(write=False)
        _cache[("osc", name)] = t
    return _cache[("osc", name)]


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def receiver_stages(oracle, i16_blocks, osc_iq, block=B, with_osc=True):
    """fm_receiver_tuned on int16 buffers: P.map convertCBladeRF >-> P.map (zipWith (*) osc) >-> firDecimator >-> ...
    -> (mixed buffers, decimated blocks).  with_osc=False: the plain receiver, no oscillator stage at all."""
    iq = [oracle.convert_i16(b) for b in i16_blocks]
    mixed, pos = [], 0
    for b in iq:
        mixed.append(TM.mix(b, osc_iq, pos) if with_osc else b)
        pos += b.size // 2
    deci = PM.FilterModel(oracle, S.taps_decim127(), PM.ORDER_AVX, complex_=True, factor=8)
    d_blocks, _ = PM.fir_decimator_pipe(deci, mixed, block)
    return mixed, d_blocks


def tail_from_d(oracle, d_blocks, block=B):
    """fmDemod >-> firResampler >-> firFilter >-> (* gain) on decimated blocks -> the audio, concatenated."""
    y_blocks = PM.fm_demod_pipe(oracle, d_blocks)
    resp = PM.ResamplerModel(oracle, 3, 10, S.taps_resamp191(), PM.ORDER_AVX)
    z_blocks, _ = PM.fir_resampler_pipe(resp, y_blocks, block)
    filt = PM.FilterModel(oracle, S.taps_audio_half64(), PM.ORDER_AVX, sym=True)
    a_blocks, _ = PM.fir_filter_pipe(filt, z_blocks, block)
    a_blocks = [oracle.scale(GAIN, a) for a in a_blocks]
    return np.concatenate(a_blocks) if a_blocks else np.empty(0, np.float32)


def model(oracle, name, nblk=NBLK, with_osc=True):
    """The restated Pipes on the first nblk source blocks of the stream (whole audio blocks only), computed once and shared."""
    key = ("model", name, nblk, with_osc)
    if key not in _cache:
        s = stream(nblk)
        blocks = [s[2 * i * B:2 * (i + 1) * B] for i in range(nblk)]
        _, d_blocks = receiver_stages(oracle, blocks, table(name), B, with_osc)
        e = tail_from_d(oracle, d_blocks)
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


# ---- the skip predicates -----------------------------------------------------------------------------------------------------------
FLT_MAX = float(np.finfo(np.float32).max)


def chain_says_no_overflow(osc):
    """sdrhip_fm_chain_set_tuner's predicate, decided under |x| <= 1 (converted u8)."""
    o = np.asarray(osc, np.float64).reshape(-1, 2)
    return bool((np.abs(o[:, 0]) + np.abs(o[:, 1]) <= FLT_MAX).all())


def i16_says_no_overflow(osc):
    """the int16 run's: converted int16 reaches |x| = 16."""
    o = np.asarray(osc, np.float64).reshape(-1, 2)
    return bool((16.0 * (np.abs(o[:, 0]) + np.abs(o[:, 1])) <= FLT_MAX).all())


# ---- the overflow case -------------------------------------------------------------------------------------------------------------
# Sample OV_N of the stream is (.., -32768) -- the last sample of block 23, one of the FORCED positions -- and the decimator output
# OV_K = (OV_N - 127) / 8 is the one whose window [8 k, 8 k + 128) meets it under tap 127 only, the zero tap create pads the 127 taps
# with.  OV_K mod 10 == 0: y[OV_K] is the last y of a resampler window of group 1 (start 10 c + 4, 64 long ... the model tells).
OV_N = 24 * B - 1
OV_K = (OV_N - 127) // 8
OV_PERIOD = 65536
OV_NBLK = 60                    # blocks of the stream the overflow model runs on: the Pipes then yield one audio block
OVERFLOW_RANGE = (7000, 7700)   # the audio outputs the GPU test runs: 3/80 of OV_N is 7373
# (q0, q1, seam block, FIR stages with Cross outputs in the range: d / r / f) of the GPU tests' runs
CHECKED_RANGES = [(0, 5994, B, "dr"), (1000, 3001, B, "dr"), (0, 2000, B, "d"), (158, 4251, B, "dr"), (0, 2 * B, B, "drf"),
                  (0, 5994, 192, "drf"), (0, 5994, 200, "drf"), (1000, 3001, 192, "drf"), OVERFLOW_RANGE + (B, "d")]


def overflow_table():
    """period 65536, 1 + 0i everywhere but one entry near 3e37 at OV_N mod 65536: every 65536 samples it meets the last sample of a block again (whether those
    overflow is in the model)."""
    t = np.zeros(2 * OV_PERIOD, np.float32)
    t[0::2] = 1.0
    t[2 * (OV_N % OV_PERIOD)] = 3e37
    return t


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def ranges(q0, q1):
    """The stage ranges of audio outputs [q0, q1) (chain.cpp's plan_run)."""
    m1 = q1 + LF - 1
    in_off = lambda m: -((-10 * m) // 3)
    ky0, ky1 = in_off(q0), in_off(m1 - 1) + NLOOP
    kd0, kd1 = max(ky0 - 1, 0), ky1
    return dict(m1=m1, ky0=ky0, ky1=ky1, kd0=kd0, kd1=kd1, n_lo=kd0 * 8, n_hi=(kd1 - 1) * 8 + 128)


def cross_counts(q0, q1, block=B):
    """How many Cross outputs of each FIR stage the run [q0, q1) computes: (decimator, resampler, filter)."""
    r = ranges(q0, q1)
    k = np.arange(r["kd0"], r["kd1"], dtype=np.int64)
    dec = int((((8 * k) % block) + 128 > block).sum())
    m = np.arange(q0, r["m1"], dtype=np.int64)
    v = (10 * m) % (3 * block)                       # window start inside its buffer, upsampled units (192 taps)
    res = int((v + 192 > 3 * block).sum())
    q = np.arange(q0, q1, dtype=np.int64)
    fil = int(((q % block) + LF > block).sum())
    return dec, res, fil


def forced_in(q0, q1, s0=0, value=-32768, i16=None):
    """Does the receptive field of [q0, q1) hold `value` at one of the stream's FORCED positions around a block edge?"""
    i16 = stream() if i16 is None else i16
    r = ranges(q0, q1)
    for e in range(B, NBLK * B, B):
        for el in range(2 * e - 5, 2 * e + 5):
            if 2 * (r["n_lo"] - s0) <= el < 2 * (r["n_hi"] - s0) and el < i16.size and i16[el] == value:
                return True
    return False
