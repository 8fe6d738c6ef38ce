"""The table behind tests/test_gpu_audio_tail_any.py: the audio tail over rows on the general fused kernel (k_audio_tail_rows_any,
sdrhip_audio_tail_set_general) -- every down-sampling shape the kernel must serve, with 64, 32 and 8 half-taps of a symmetric
filter.  No pytest in here: tests/test_audio_tail_any_cases.py shows on the CPU, from the models alone, what the table reaches.

Every row is one seeded y stream from stream element 0; the expected audio of a (shape, row, block, gain) is the restated Pipes'
composition (oracle/pipes_model.py): firResampler(block) >-> firFilter(block) >-> (* gain) on the y stream cut into blocks of
`block` (one block for a contiguous stream), computed once and shared -- exactly as tests/audio_tail_cases.py builds it.  A launch is
a range [q0, q1) of audio outputs, given a buffer that holds exactly its receptive field or the stream from 0.

The far launches move a near launch by T = I * 2^30 outputs and S = D * 2^30 inputs: multiples of the blocks that are moved (0 and
256) in outputs, in inputs and in upsampled units, so the near stream's answer is the far launch's, One / Cross decisions included.
For 3/10 the far launch starts at output 3 * 2^30 + 5."""
import dataclasses

import numpy as np

from oracle import pipes_model as PM
import signals as S
import stream_slice_cases as SC

TILE = 840                     # audio outputs of one workgroup (kernels.hpp kTailAnyTileOutputs)
Q_MAX = 2 * TILE + 1 + 360     # a few thousand outputs per row: 2 A + 1 and a range behind it
WINDOW_FLOATS, MAX_GROUP, MAX_FILTER, MAX_INTERP = 5120, 64, 128, 8


@dataclasses.dataclass(frozen=True)
class Shape:
    name: str
    I: int
    D: int
    ntaps: int
    nhalf: int

    @property
    def rlp(self):                 # numCoeffsR = roundUp(ntaps, I * 8)
        return -(-self.ntaps // (self.I * 8)) * self.I * 8

    @property
    def nloop(self):               # floats a polyphase group walks: roundUp(ceil(ntaps / I), 8)
        return -(-(-(-self.ntaps // self.I)) // 8) * 8

    @property
    def lf(self):
        return 2 * self.nhalf

    @property
    def lowest_block(self):        # what sdrhip_audio_tail_create admits, and the predicate has no tighter bound
        return max(-(-self.rlp // self.I), self.lf)

    def resamp_taps(self):
        if (self.I, self.D, self.ntaps) == (3, 10, 191):
            return S.taps_resamp191()
        return (self.I * S.windowed_sinc(self.ntaps, 1.0 / max(self.I, self.D))).astype(np.float32)

    def audio_half(self):
        return {64: S.taps_audio_half64(), 32: S.taps_audio_half32(), 8: S.taps_audio_half32()[:8]}[self.nhalf]

    def first_input(self, q):
        return int(SC.in_offset(q, self.I, self.D))

    def end_input(self, q):
        """One past the last y index audio output q reads."""
        return int(SC.in_offset(q + self.lf - 1, self.I, self.D)) + self.nloop

    @property
    def n_y(self):
        return self.end_input(Q_MAX - 1)


SHAPES = {s.name: s for s in (
    Shape("4/5 x 63", 4, 5, 63, 64), Shape("3/5 x 71", 3, 5, 71, 32), Shape("2/5 x 127", 2, 5, 127, 64), Shape("2/3 x 47", 2, 3, 47, 8),
    Shape("3/4 x 95", 3, 4, 95, 32), Shape("7/8 x 255", 7, 8, 255, 64), Shape("8/9 x 511", 8, 9, 511, 8), Shape("1/5 x 39", 1, 5, 39, 64),
    Shape("3/10 x 191", 3, 10, 191, 64))}
FM = SHAPES["3/10 x 191"]
# the prepared lengths the issue names
assert [s.rlp for s in SHAPES.values()] == [64, 72, 128, 48, 96, 280, 512, 40, 192]
# every must-serve shape with every half-tap count (the ABI test asks the predicate about all 27)
HALF_COUNTS = (64, 32, 8)
SEAMED_BLOCKS = (200, 250, 256, 1000)


def general_fits(shape, block, nhalf=None):
    """kernels_tail_any.hip audio_tail_any_fits, restated (AVX orders, real data, a symmetric filter are the caller's)."""
    lf = 2 * (nhalf or shape.nhalf)
    I, D = shape.I, shape.D
    if not (1 <= I <= MAX_INTERP and D > I and np.gcd(I, D) == 1):
        return False
    if not (8 <= shape.nloop <= MAX_GROUP and shape.rlp >= D and 16 <= lf <= MAX_FILTER and lf % 16 == 0):
        return False
    premax = int(SC.in_offset(I - 1, I, D))
    nc = -(-(TILE + lf - 1) // I)
    if D * (nc - 1) + premax + shape.nloop + 8 > WINDOW_FLOATS:
        return False
    return block == 0 or (block * I >= shape.rlp and block >= lf and block <= 1 << 27)


def y_row(shape, row, seed=0):
    y = S.real_block(shape.n_y, seed=9300 + 37 * row + 1013 * seed + 7 * shape.ntaps)
    y.setflags(write=False)
    return y


def _blocks(x, block):
    return [x[i:i + block] for i in range(0, x.size - block + 1, block)]


def z_stream(oracle, shape, y, block):
    """The resampler Pipe's output stream (whole blocks only) for y cut into blocks of `block` (0: one block, every output One)."""
    model = PM.ResamplerModel(oracle, shape.I, shape.D, shape.resamp_taps(), PM.ORDER_AVX)
    assert model.num_coeffs == shape.rlp
    if block == 0:
        nz = (y.size * shape.I - shape.rlp) // shape.D + 1
        out, _ = PM.fir_resampler_pipe(model, [y], nz)
    else:
        out, _ = PM.fir_resampler_pipe(model, _blocks(y, block), block)
    return np.concatenate(out)


def filter_stream(oracle, shape, z, block):
    model = PM.FilterModel(oracle, shape.audio_half(), PM.ORDER_AVX, sym=True)
    assert model.num_coeffs == shape.lf
    if block == 0:
        out, _ = PM.fir_filter_pipe(model, [z], z.size - shape.lf + 1)
    else:
        out, _ = PM.fir_filter_pipe(model, _blocks(z, block), block)
    return np.concatenate(out)


def padded(shape, y, block, n_ok):
    """y with the zeros appended that make the Pipes (whole blocks only) yield the blocks holding outputs [0, n_ok)."""
    if not block:
        return y
    up = lambda n: -(-n // block) * block                               # noqa: E731
    pad = up(-(-(up(up(n_ok) + shape.lf - 1) * shape.D) // shape.I) + shape.nloop + 1) + block
    return np.concatenate([y, np.zeros(max(pad - y.size, 0), np.float32)])


def expected_from(oracle, shape, y, block, gain):
    """Audio outputs [0, ...) of the composition on one y stream: those the stream itself determines."""
    n_ok = 0
    while shape.end_input(n_ok) <= y.size:
        n_ok += 1
    a = filter_stream(oracle, shape, z_stream(oracle, shape, padded(shape, y, block, n_ok), block), block)
    assert a.size >= n_ok, (a.size, n_ok, block)
    return oracle.scale(np.float32(gain), a[:n_ok])


_cache = {}


def expected(oracle, shape, row, block, gain=1.0, seed=0):
    key = (shape.name, row, block, float(np.float32(gain)), seed)
    if key not in _cache:
        e = expected_from(oracle, shape, y_row(shape, row, seed), block, gain)
        assert e.size >= Q_MAX
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


# ---- the seam rule on the tail's two stages -----------------------------------------------------------------------------------
def resampler_cross(shape, block, a, b):
    """z outputs in [a, b) the resampler Pipe computes sequentially (seam and output block both `block`)."""
    m = np.arange(a, b, dtype=np.int64)
    return m[SC.is_cross(m, shape.I, shape.D, shape.rlp, block, block)] if block else m[:0]


def filter_cross(shape, block, a, b):
    q = np.arange(a, b, dtype=np.int64)
    return q[SC.is_cross(q, 1, 1, shape.lf, block, block)] if block else q[:0]


def late_first_outputs(shape, block, a, b):
    """z outputs in [a, b) whose window straddles a seam, that open an output block and whose first input lies behind the seam
    (kernels.hpp late_output_is_one)."""
    if not block:
        return np.zeros(0, np.int64)
    m = np.arange(a, b, dtype=np.int64)
    v = m * shape.D
    edge = (v // (block * shape.I) + 1) * (block * shape.I)
    return m[(v + shape.rlp > edge) & SC.late_output_is_one(m, edge, shape.I, shape.D, block)]


def boundaries_in_tile(shape, block, tile):
    """(resampler, filter) buffer boundaries strictly inside the window ranges of tile `tile` of a launch from output 0."""
    qa, qb = tile * TILE, (tile + 1) * TILE
    v_lo, v_hi = qa * shape.D, (qb + shape.lf - 2) * shape.D + shape.rlp
    r = (v_hi - 1) // (block * shape.I) - v_lo // (block * shape.I)
    f = (qb - 1 + shape.lf - 1) // block - qa // block
    return r, f


# ---- the launches ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Launch:
    name: str
    shape: Shape
    block: int
    q0: int
    q1: int
    rows: int = 3
    exact: bool = True             # the buffer holds exactly the receptive field (y_base = first_input(q0)); else the stream from 0
    far: bool = False
    seamed: bool = False           # made to hold Cross outputs of BOTH stages
    cuts: tuple = ()
    layout: tuple = (0, 0, 0, 0)   # floats: gap between y rows, between audio rows, offset of the first y row, of the first audio row
    gain: float = 1.0

    @property
    def z_range(self):
        return self.q0, self.q1 + self.shape.lf - 1

    @property
    def far_shift(self):
        return (self.shape.I << 30, self.shape.D << 30) if self.far else (0, 0)


def _launches():
    out = []
    every = (0,) + SEAMED_BLOCKS
    for k, s in enumerate(SHAPES.values()):
        n = s.name
        ends = sorted({1, 2, s.I, s.I + 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1})
        for j, end in enumerate(ends):
            out.append(Launch(f"{n}: [0, {end})", s, every[(j + k) % 5], 0, end, rows=1 if end < 4 else 3, exact=j % 2 == 0, seamed=False))
        for j, q0 in enumerate(sorted({0, 1, s.I - 1, 601, TILE})):
            out.append(Launch(f"{n}: from {q0}", s, every[(j + k + 2) % 5], q0, q0 + 300))
        for block in (0, 256):
            out.append(Launch(f"{n}: far, block {block}", s, block, 5, 700, far=True, seamed=block > 0))
        b3 = SEAMED_BLOCKS[k % 4]
        out.append(Launch(f"{n}: [0, N) whole, block {b3}", s, b3, 0, Q_MAX, exact=False, seamed=True))
        out.append(Launch(f"{n}: three runs", s, SEAMED_BLOCKS[(k + 1) % 4], 0, Q_MAX, cuts=(841, 1705), seamed=True))
        out.append(Launch(f"{n}: five runs", s, SEAMED_BLOCKS[(k + 2) % 4], 7, Q_MAX, cuts=(99, 1001, 1003, 1999), seamed=True))
        out.append(Launch(f"{n}: the lowest block", s, s.lowest_block, 0, Q_MAX, rows=1, seamed=True))
    pick = list(SHAPES.values())
    for j, rows in enumerate((1, 3, 32)):
        for s in (pick[j], pick[j + 4]):
            out.append(Launch(f"{s.name}: {rows} rows, block 200", s, 200, 3, 1900, rows=rows, exact=False, seamed=True))
    for j, (gy, ga) in enumerate(((0, 0), (1, 1), (5, 5), (1, 5), (5, 0))):
        s = pick[(2 * j + 1) % 9]
        out.append(Launch(f"{s.name}: strides n + {gy} / n + {ga}", s, 256, 500, 1400, layout=(gy, ga, 0, 0), seamed=True))
    for off in (1, 2, 3):
        for s in (pick[off], pick[off + 5]):
            out.append(Launch(f"{s.name}: y base {4 * off} bytes past a 16-byte boundary", s, 250, 500 + off, 1400,
                              layout=(0, 0, off, (off + 1) % 4), seamed=True))
    for j, gain in enumerate((-0.5, float(np.float32(1e-41)))):
        for s in (pick[3 * j], pick[3 * j + 2]):
            out.append(Launch(f"{s.name}: gain {gain!r}", s, 1000, 500, 1400, gain=gain, seamed=True))
    # On route 0 the rule of k_audio_tail_rows comes first: it takes a contiguous stream of its own shape inside its sweep (1 .. 32 rows
    # of 153 .. 314574 outputs).  Those launches get 33 rows, so that mode 1 reaches the general kernel on the FM shape too.
    return [dataclasses.replace(c, rows=33) if c.shape.name == "3/10 x 191" and c.block == 0 and c.q1 - c.q0 >= 153 else c for c in out]


LAUNCHES = _launches()
assert len({c.name for c in LAUNCHES}) == len(LAUNCHES)
