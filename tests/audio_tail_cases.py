"""The table behind tests/test_gpu_audio_tail.py: the audio tail over rows (sdrhip_audio_tail_run_rows) on the FM fixture taps --
a 3/10 resampler of 191 taps (64-float polyphase groups, 192 prepared taps) and 64 half-taps of a symmetric filter, the shape the
fused kernel serves.  No pytest in here: tests/test_audio_tail_cases.py shows on the CPU, from the models alone, what the table
reaches.

Every row is one seeded y stream of N_Y samples from stream element 0; the expected audio of a (row, block, gain) is the restated
Pipes' composition (oracle/pipes_model.py): firResampler(block) >-> firFilter(block) >-> (* gain) on the y stream cut into blocks
of `block` (one block for a contiguous stream), computed once and shared.  A launch is a range [q0, q1) of audio outputs, given a
buffer that holds exactly its receptive field (y_base = the first input of q0) or the stream from 0.

The far launches move a near launch by T = 3 * 2^30 outputs and S = 10 * 2^30 inputs: both multiples of the block sizes that are
moved (0 and 8192), so the near stream's answer is the far launch's, One / Cross decisions included."""
import dataclasses
import functools

import numpy as np

from oracle import pipes_model as PM
import signals as S
import stream_slice_cases as SC

I, D = 3, 10
NLOOP = 64                     # floats a polyphase group walks
RLP = 192                      # numCoeffsR = roundUp(191, 3 * 8)
LF = 128                       # numCoeffsF of the symmetric filter
TILE = 2046                    # audio outputs of one workgroup of the fused kernel (kernels.hpp kTailTileOutputs)
NZ_TILE = 3 * ((TILE + LF - 1 + 2) // 3)
Q_MAX = 8400
FAR_T, FAR_S = 3 << 30, 10 << 30


def resamp_taps():
    return S.taps_resamp191()


def audio_half():
    return S.taps_audio_half64()


def first_input(q):
    return int(SC.in_offset(q, I, D))


def end_input(q):
    """One past the last y index audio output q reads."""
    return int(SC.in_offset(q + LF - 1, I, D)) + NLOOP


N_Y = end_input(Q_MAX - 1)


def fused_fits(block):
    """kernels_tail.hip fm_tail_fused_fits for 192 prepared taps: a buffer of the Pipes is longer than a tile."""
    return block == 0 or not (block * 3 < 10 * NZ_TILE + RLP or block < TILE + 4 + LF or block > (1 << 28))


MIN_BLOCK = next(b for b in range(LF, 1 << 16) if fused_fits(b))
BLOCKS = (0, 8192, MIN_BLOCK, 1024)


def y_row(row, seed=0):
    y = S.real_block(N_Y, seed=9100 + 37 * row + 1013 * seed)
    y.setflags(write=False)
    return y


def _blocks(x, block):
    return [x[i:i + block] for i in range(0, x.size - block + 1, block)]


def z_stream(oracle, y, block):
    """The resampler Pipe's output stream (whole blocks only) for y cut into blocks of `block` (0: one block, every output One)."""
    model = PM.ResamplerModel(oracle, I, D, resamp_taps(), PM.ORDER_AVX)
    assert model.num_coeffs == RLP
    if block == 0:
        nz = (y.size * I - RLP) // D + 1
        out, _ = PM.fir_resampler_pipe(model, [y], nz)
    else:
        out, _ = PM.fir_resampler_pipe(model, _blocks(y, block), block)
    return np.concatenate(out)


def filter_stream(oracle, z, block):
    model = PM.FilterModel(oracle, audio_half(), PM.ORDER_AVX, sym=True)
    assert model.num_coeffs == LF
    if block == 0:
        out, _ = PM.fir_filter_pipe(model, [z], z.size - LF + 1)
    else:
        out, _ = PM.fir_filter_pipe(model, _blocks(z, block), block)
    return np.concatenate(out)


def expected_from(oracle, y, block, gain):
    """Audio outputs [0, ...) of the composition on one y stream; zeros are appended so that the Pipes (which yield whole blocks
    only) yield the blocks that hold the outputs the stream itself determines -- those are cut off again."""
    n_ok = 0
    while end_input(n_ok) <= y.size:
        n_ok += 1
    if block:
        up = lambda n: -(-n // block) * block                           # noqa: E731
        pad = up(-(-(up(up(n_ok) + LF - 1) * D) // I) + NLOOP + 1) + block
        y = np.concatenate([y, np.zeros(pad - y.size, np.float32)])
    a = filter_stream(oracle, z_stream(oracle, y, block), block)
    assert a.size >= n_ok, (a.size, n_ok, block)
    return oracle.scale(np.float32(gain), a[:n_ok])


_cache = {}


def expected(oracle, row, block, gain=1.0, seed=0):
    key = (row, block, float(np.float32(gain)), seed)
    if key not in _cache:
        e = expected_from(oracle, y_row(row, seed), block, gain)
        assert e.size >= Q_MAX
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


# ---- the seam rule on the tail's two stages -----------------------------------------------------------------------------------
def resampler_cross(block, a, b):
    """z outputs in [a, b) the resampler Pipe computes sequentially (seam and output block both `block`)."""
    m = np.arange(a, b, dtype=np.int64)
    return m[SC.is_cross(m, I, D, RLP, block, block)] if block else m[:0]


def filter_cross(block, a, b):
    q = np.arange(a, b, dtype=np.int64)
    return q[SC.is_cross(q, 1, 1, LF, block, block)] if block else q[:0]


def late_first_outputs(block, a, b):
    """z outputs in [a, b) whose window straddles a seam, that open an output block and whose first input lies behind the seam
    (kernels.hpp late_output_is_one).  With seam block = output block = B and 3/10 there is none: m = k B gives a window start
    10 k B = B (k mod 3) modulo 3 B, never 1 or 2 short of a multiple of 3 B."""
    if not block:
        return np.zeros(0, np.int64)
    m = np.arange(a, b, dtype=np.int64)
    v = m * D
    edge = (v // (block * I) + 1) * (block * I)
    return m[(v + RLP > edge) & SC.late_output_is_one(m, edge, I, D, block)]


# ---- the launches ---------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Launch:
    name: str
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
        return self.q0, self.q1 + LF - 1


def _launches():
    out = []
    for end in (1, 2, 3, 4, 2045, 2046, 2047, 4093):
        out.append(Launch(f"[0, {end})", 8192 if end % 2 else 0, 0, end, rows=1 if end < 4 else 3, exact=end % 3 != 0))
    for q0 in (1, 2, 3 * 200 + 1, 2046):
        out.append(Launch(f"from {q0}", 0 if q0 % 2 else 8192, q0, q0 + 700))
    for block in (0, 8192):
        out.append(Launch(f"far, block {block}", block, 5, 2300, far=True))
    out.append(Launch("far across both seams", 8192, 2300, Q_MAX, far=True, seamed=True))
    for rows in (1, 3, 32):
        out.append(Launch(f"both seams, {rows} rows", 8192, 0, Q_MAX, rows=rows, exact=False, seamed=True))
    out.append(Launch("both seams, the smallest fitting block", MIN_BLOCK, 0, Q_MAX, seamed=True))
    out.append(Launch("a tile boundary on a seam, the smallest fitting block", MIN_BLOCK, 2046 * 3, Q_MAX, seamed=True))
    out.append(Launch("block 1024: composed only", 1024, 0, 2500, seamed=True))
    out.append(Launch("three runs", 8192, 0, Q_MAX, cuts=(2047, 6001), seamed=True))
    out.append(Launch("five runs", 8192, 7, Q_MAX, cuts=(100, 2460, 2461, 8065), seamed=True))
    for k, (gy, ga) in enumerate(((0, 0), (1, 1), (5, 5), (1, 5))):
        out.append(Launch(f"strides n + {gy} / n + {ga}", 8192, 2000, 2700, layout=(gy, ga, 0, 0)))
    for off in (1, 2, 3):
        out.append(Launch(f"y base {4 * off} bytes past a 16-byte boundary", 8192, 2000 + off, 2700, layout=(0, 0, off, (off + 1) % 4)))
    for gain in (-0.5, float(np.float32(1e-41))):
        out.append(Launch(f"gain {gain!r}", 8192, 2000, 2700, gain=gain))
    return out


LAUNCHES = _launches()
assert len({c.name for c in LAUNCHES}) == len(LAUNCHES)
