"""The table behind tests/test_gpu_tail_family.py: the kernels specialised for the tail `y -> firResampler 3/10 -> symmetric firFilter
(2 x 64 taps) * gain` -- k_fm_tail, the one-kernel chain in its four forms, k_audio_tail_rows -- on EVERY resampler tap count their
host predicate admits (fm_tail_shape_ok, kernels_tail.hip: 169 .. 192 taps, which prepare to 3 groups of 64 floats, 192 taps), and on
block sizes that are odd, 1 and 2 modulo 3, and no multiple of 8.  No pytest in here: tests/test_tail_family_cases.py shows on the CPU,
from the models alone, what the table reaches.

Tap sets.  Count n in COUNTS: S.gauss_taps(n, 7000 + n) (seeded; the last taps are nonzero).  ANCHOR: S.taps_resamp191(), the set every
earlier test of these kernels uses -- its expectations here are those of tests/audio_tail_cases.py, bit for bit.  EDGES: 168 and 193
taps, one short and one past the family (56-float groups / 168 taps, 72-float groups / 216 taps): no fused kernel may take them.

Expected values come from the restated Pipes only (oracle/pipes_model.py): the composition of tests/audio_tail_cases.py for rows,
PM.fm_receiver for chains, the oscillator stage of tests/tuner_model.py in front of it for banks.  Each is computed once, cached and
read-only; no device run is a source of expected values."""
import dataclasses

import numpy as np

from oracle import pipes_model as PM
from oracle.oracle import round_up
import audio_tail_cases as AC
import signals as S
import stream_slice_cases as SC
import tuner_model as TM

I, D = AC.I, AC.D
LF, TILE, Q_MAX = AC.LF, AC.TILE, AC.Q_MAX
NLOOP, RLP = AC.NLOOP, AC.RLP

COUNTS = tuple(range(169, 193))
ANCHOR = "anchor"
EDGES = (168, 193)
TAP_SETS = COUNTS + (ANCHOR,)

# 7314 is the smallest block the fused tail fits (audio_tail_cases.MIN_BLOCK); its neighbours are odd / 1 mod 3 and 2 mod 3
BLOCKS = (0, 8192, AC.MIN_BLOCK + 1, AC.MIN_BLOCK + 2, 8191)
ODD1, EVEN2, ODD8 = BLOCKS[2], BLOCKS[3], BLOCKS[4]
assert ODD1 % 2 == 1 and ODD1 % 3 == 1 and EVEN2 % 3 == 2 and ODD8 % 2 == 1 and ODD8 % 8 != 0 and ODD8 % 3 != 0
assert all(AC.fused_fits(b) for b in BLOCKS) and not AC.fused_fits(AC.MIN_BLOCK - 1)

# ---- rows (k_audio_tail_rows) ----------------------------------------------------------------------------------------------------
ROWS = 3
ROWS_ALL_BLOCKS = (169, 170, 171, 190, 192)          # counts that run every block; the others run 8192 and ODD1
ROWS_CUTS = (2047, 6001)
# [0, Q_MAX) holds the FIRST buffer boundary of the filter only, and every tile below it starts inside the first buffer, where a
# position modulo the block is the position itself.  The long cases reach past the second boundary (2 * block <= 16384): there the
# kernels' `qa % seam` and `(30 c0) % (3 seam)` are real reductions.  Their second launch starts at Q_LONG_START on a buffer that holds
# exactly its receptive field, so its tiles lie elsewhere than those of the launch from 0.
Q_LONG = 2 * 8192 + 300
Q_LONG_START = 8500                                    # past the first boundary of every block, not on a polyphase cycle
ROWS_LONG_CASES = [(key, block) for key in (169, 192) for block in (AC.MIN_BLOCK + 1, AC.MIN_BLOCK + 2, 8191)]

# ---- chains (k_fm_tail, k_fm_chain_small, the stage kernels) -------------------------------------------------------------------------
CHAIN_COUNTS = (169, 170, 171, 180, 190, 192)
CHAIN_BLOCKS = (8192, ODD1, EVEN2, ODD8)
CHAIN_NBLK = 70                                       # source blocks of `block` samples: the Pipes yield one audio block
GAIN = 0.2
DECIM = 8
DECIM_COUNTS = (125, 126, 128)                        # beside S.taps_decim127(): all prepare to 128 taps
DECIM_CASE = (170, ODD1)
# as the long rows cases: 100 source blocks yield two audio blocks, the second behind the filter's second boundary
CHAIN_LONG_NBLK = 100
CHAIN_LONG_CASES = [(170, ODD8), (192, ODD1)]

# ---- banks (the bank and int16-bank forms of k_fm_chain_small) --------------------------------------------------------------------------
BANK_COUNTS = (169, 192)
BANK_BLOCKS = (8192, ODD8)
STATIONS = ("shift -3/1000", "shift 5/8313")

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        v = make()
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
        _cache[key] = v
    return _cache[key]


# ---- the tap sets -------------------------------------------------------------------------------------------------------------------
def resamp_taps(key):
    if key == ANCHOR:
        return _frozen(("taps", key), S.taps_resamp191)
    return _frozen(("taps", key), lambda: S.gauss_taps(int(key), 7000 + int(key)))


def ntaps(key):
    return resamp_taps(key).size


def audio_half():
    return AC.audio_half()


def decim_taps(n=127):
    if n == 127:
        return _frozen(("decim", n), S.taps_decim127)
    return _frozen(("decim", n), lambda: S.gauss_taps(n, 7500 + n))


def table(name):
    num, den = {"shift -3/1000": (-3, 1000), "shift 5/8313": (5, 8313)}[name]
    return _frozen(("osc", name), lambda: TM.shift_table(num, den))


# ---- what a tap count implies (FilterInternal.hs:297-319, restated as arithmetic) -------------------------------------------------------
def nloop_of(n):
    """Floats a polyphase group walks: the longest group, rounded up to the 8 lanes."""
    return round_up(-(-n // I), 8)


def rlp_of(n):
    """numCoeffsR, Filter.hs:422."""
    return round_up(n, I * 8)


def group_nonzero(n):
    """Taps of the set that land in group 0, 1, 2: group g holds the taps of one residue modulo 3."""
    off = [0, 2, 1]                                    # offsets of the 3/10 walk: group g starts at tap off[g]
    return tuple((n - o + I - 1) // I for o in off)


def cross_terms(n):
    """Terms of a sequential (Cross) output by filter offset fo = 0, 1, 2: taps fo, fo + 3, ... < n."""
    return tuple((n - fo + 2) // 3 for fo in range(3))


def in_family(n):
    """fm_tail_shape_ok for a 3/10 resampler of n taps in the AVX order with 64 half-taps."""
    return nloop_of(n) == NLOOP and rlp_of(n) <= 3 * NLOOP and n <= rlp_of(n)


def end_input(q, n):
    """One past the last y index audio output q of a tail of n resampler taps reads."""
    return int(SC.in_offset(q + LF - 1, I, D)) + nloop_of(n)


# ---- rows: the composition on seeded y streams -------------------------------------------------------------------------------------------
N_Y_MAX = end_input(Q_MAX - 1, max(EDGES))
N_Y_LONG = end_input(Q_LONG - 1, max(COUNTS))


def y_row(row, long=False):
    """audio_tail_cases' row, with a few seeded samples more behind it for the 72-float groups of 193 taps; long: a seeded row of its
    own for the outputs [0, Q_LONG)."""
    def make():
        if long:
            return S.real_block(N_Y_LONG, seed=9800 + row)
        y = AC.y_row(row)
        return np.concatenate([y, S.real_block(N_Y_MAX - y.size, seed=9700 + row)])
    return _frozen(("y", row, long), make)


def _blocks(x, block):
    return [x[i:i + block] for i in range(0, x.size - block + 1, block)]


def z_stream(oracle, taps, y, block):
    """The resampler Pipe's output stream (whole blocks only) for y cut into blocks of `block` (0: one block, every output One)."""
    model = PM.ResamplerModel(oracle, I, D, taps, PM.ORDER_AVX)
    assert model.num_coeffs == rlp_of(taps.size)
    if block == 0:
        out, _ = PM.fir_resampler_pipe(model, [y], (y.size * I - model.num_coeffs) // D + 1)
    else:
        out, _ = PM.fir_resampler_pipe(model, _blocks(y, block), block)
    return np.concatenate(out)


def tail_streams(oracle, taps, y, block):
    """-> (z, audio before the gain): firResampler(block) >-> firFilter(block) on the y stream; zeros are appended so that the Pipes
    (whole blocks only) yield the blocks that hold every output the stream itself determines -- those are cut off again."""
    n = taps.size
    q = np.arange(0, y.size, dtype=np.int64)
    n_ok = int(np.count_nonzero(SC.in_offset(q + LF - 1, I, D) + nloop_of(n) <= y.size))
    if block:
        up = lambda k: -(-k // block) * block                           # noqa: E731
        pad = up(-(-(up(up(n_ok) + LF - 1) * D) // I) + nloop_of(n) + 1) + block
        y = np.concatenate([y, np.zeros(pad - y.size, np.float32)])
    z = z_stream(oracle, taps, y, block)
    a = AC.filter_stream(oracle, z, block)
    assert a.size >= n_ok, (a.size, n_ok, block)
    return z[:n_ok + LF - 1], a[:n_ok]


def rows_streams(oracle, key, row, block, long=False):
    """(z, audio before the gain) of row `row` under tap set `key`: computed once."""
    def make():
        taps = resamp_taps(key)
        z, a = tail_streams(oracle, taps, y_row(row, long)[:end_input((Q_LONG if long else Q_MAX) - 1, taps.size)], block)
        z.setflags(write=False)
        a.setflags(write=False)
        return z, a
    return _frozen(("rows", key, row, block, long), make)


def rows_expected(oracle, key, row, block, gain=1.0, long=False):
    def make():
        n = Q_LONG if long else Q_MAX
        e = oracle.scale(np.float32(gain), rows_streams(oracle, key, row, block, long)[1])
        assert e.size >= n
        return e[:n]
    return _frozen(("rows*", key, row, block, float(np.float32(gain)), long), make)


def rows_blocks(key):
    return BLOCKS if key in ROWS_ALL_BLOCKS else (8192, ODD1)


ROWS_CASES = [(key, block) for key in TAP_SETS for block in rows_blocks(key)]


# ---- the seam rule on the tail's two stages, and the sequential kernel restated ----------------------------------------------------------
def resampler_cross(block, a, b, rlp=RLP):
    m = np.arange(a, b, dtype=np.int64)
    return m[SC.is_cross(m, I, D, rlp, block, block)] if block else m[:0]


def filter_cross(block, a, b):
    return AC.filter_cross(block, a, b)


def decimator_cross(block, a, b, lp=128):
    k = np.arange(a, b, dtype=np.int64)
    return k[SC.is_cross(k, 1, DECIM, lp, block, block)] if block else k[:0]


def sequential_z(taps, y, m, terms=None, behind=0.0):
    """Resampler output m in the sequential order of resampleCrossHighLevel (FilterInternal.hs:410-423): taps fo, fo + 3, ... from +0,
    every product and sum rounded.  terms: term count by filter offset (default: the set's own, cross_terms); a walk that runs past the
    set's last tap reads `behind` there -- the device's plain tap buffer ends at the last tap, so what lies behind it is not a tap."""
    n = taps.size
    v = D * int(m)
    pos = (v + I - 1) // I
    fo = pos * I - v
    nterms = cross_terms(n)[fo] if terms is None else terms[fo]
    t = np.concatenate([taps, np.full(max(0, fo + I * nterms - n), behind, np.float32)])
    r = np.float32(0.0)
    for l in range(nterms):
        r = np.float32(r + np.float32(y[pos + l] * t[fo + I * l]))
    return r


# ---- chains -----------------------------------------------------------------------------------------------------------------------------
def chain_u8(block, nblk=CHAIN_NBLK):
    return _frozen(("u8", block, nblk), lambda: S.iq_u8_fm(nblk * block))


def _source_blocks(x, block, per_sample=2):
    w = per_sample * block
    return [x[w * i:w * (i + 1)] for i in range(x.size // w)]


def chain_expected(oracle, key, block, decim=127, nblk=CHAIN_NBLK):
    """PM.fm_receiver on nblk source blocks of `block` samples (every Pipe's block is `block`): the whole audio blocks."""
    def make():
        out = PM.fm_receiver(oracle, _source_blocks(chain_u8(block, nblk), block), decim_taps(decim), DECIM, resamp_taps(key), I, D, audio_half(),
                             GAIN, block, PM.ORDER_AVX)
        return np.concatenate(out) if out else np.zeros(0, np.float32)
    return _frozen(("chain", key, block, decim, nblk), make)


def chain_stage_ranges(q0, q1, n=191):
    """The stage ranges of audio outputs [q0, q1) (chain.cpp's plan_run): z outputs [q0, m1), y and d outputs [kd0, ky1)."""
    m1 = q1 + LF - 1
    ky0, ky1 = int(SC.in_offset(q0, I, D)), int(SC.in_offset(m1 - 1, I, D)) + nloop_of(n)
    return dict(m1=m1, ky0=ky0, ky1=ky1, kd0=max(ky0 - 1, 0), kd1=ky1)


CHAIN_CASES = [(key, block) for key in CHAIN_COUNTS for block in CHAIN_BLOCKS]


# ---- banks ------------------------------------------------------------------------------------------------------------------------------
def bank_stream(fmt, block):
    """fmt "u8": the chains' FM stream; "i16": seeded interleaved int16 over the whole range."""
    if fmt == "u8":
        return chain_u8(block)
    return _frozen(("i16", block), lambda: np.random.default_rng(1700 + block).integers(-32768, 32768, 2 * CHAIN_NBLK * block,
                                                                                         dtype=np.int64).astype(np.int16))


def bank_expected(oracle, fmt, name, key, block):
    """The restated receiver with the oscillator stage (tests/tuned_chain_model.py), for either input format: P.map convert >->
    P.map (zipWith (*) osc) >-> firDecimator >-> fmDemod >-> firResampler >-> firFilter >-> P.map (* gain)."""
    def make():
        convert = oracle.convert_u8 if fmt == "u8" else oracle.convert_i16
        mixed, pos = [], 0
        for b in _source_blocks(bank_stream(fmt, block), block):
            mixed.append(TM.mix(convert(b), table(name), pos))
            pos += block
        deci = PM.FilterModel(oracle, decim_taps(), PM.ORDER_AVX, complex_=True, factor=DECIM)
        d_blocks, _ = PM.fir_decimator_pipe(deci, mixed, block)
        y_blocks = PM.fm_demod_pipe(oracle, d_blocks)
        z_blocks, _ = PM.fir_resampler_pipe(PM.ResamplerModel(oracle, I, D, resamp_taps(key), PM.ORDER_AVX), y_blocks, block)
        a_blocks, _ = PM.fir_filter_pipe(PM.FilterModel(oracle, audio_half(), PM.ORDER_AVX, sym=True), z_blocks, block)
        return np.concatenate([oracle.scale(GAIN, a) for a in a_blocks]) if a_blocks else np.zeros(0, np.float32)
    return _frozen(("bank", fmt, name, key, block), make)


BANK_CASES = [(fmt, key, block) for fmt in ("u8", "i16") for key in BANK_COUNTS for block in BANK_BLOCKS]


# ---- the predicate's edges --------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Edge:
    ntaps: int
    nloop: int
    rlp: int


EDGE_SHAPES = tuple(Edge(n, nloop_of(n), rlp_of(n)) for n in EDGES)
EDGE_BLOCK = 8192
