"""The seeded inputs the squelch tests share (tests/test_squelch_cases.py states, from the model alone, what they must contain;
tests/test_gpu_squelch.py runs them on the device).  TEST INFRASTRUCTURE ONLY.

A detector row is built block by block from a pattern of three classes: L (a level under the lower threshold), M (between the two) and
H (over the upper one).  Its samples are +-amp * (1 .. 1.05), so that even a block of ONE sample falls into its class; a complex
detector splits the amplitude 0.8 / 0.6 between re and im.  With the thresholds 0.25 and 1.0 the same rows serve both polarities:
opening above 1.0 (a carrier squelch) and opening below 0.25 (an FM quieting squelch)."""
import numpy as np

import squelch_model as SM

F = np.float32
# openings, closings, between-levels met open and shut, and for either polarity a stretch without an opening that outlasts the hang
PATTERN = "LLMHMMLLLLLMHHLMLLLLLLLHLLLLLLLL" + "HMMHMMMMLL"
GATE_BLOCKS = 2 * len(PATTERN)                     # a gate case holds the whole pattern at any shift
AMP = {"L": 0.2, "M": 0.7, "H": 1.5}
LOW, HIGH = 0.25, 1.0
ABOVE = dict(open_level=HIGH, close_level=LOW, open_above=1)       # opens on H, closes on L
BELOW = dict(open_level=LOW, close_level=HIGH, open_above=0)       # opens on L, closes on H
POLARITIES = {"above": ABOVE, "below": BELOW}
WG, LS = SM.WG, SM.LS
BLOCK_DETS = (1, 3, 255, 256, 257, 1000, 1024, 4097)
BLOCK_SIGS = (1, 5, 256, 1000)
N_BLOCKS = (0, 1, 2, 63, 64, 65, 1024, 1025)
HANGS = (0, 1, 3)
# every carried-in state, out-of-range ones included: det 0 / 1 / other, hang_left below, inside and above 0 .. hang
STATES_IN = [(0, 0), (1, 0), (0, 1), (1, 3), (0, 3), (0, 2), (7, 1), (-1, 2), (0, -5), (0, 1 << 30), (1, -1), (0, 100)]
SPECIALS = np.array([0x7FC12345, 0xFFC00001, 0x7F800001, 0x80000000, 0x00000001, 0x7F800000, 0xFF800000, 0x807FFFFF], np.uint32)


def classes(n_blocks, shift=0):
    return "".join(PATTERN[(b + shift) % len(PATTERN)] for b in range(n_blocks))


def detector(rows, n_blocks, block_det, det_complex, seed):
    """rows x (n_blocks * block_det [* 2]) floats; row r follows the pattern shifted by 5 r blocks"""
    rng = np.random.default_rng(seed)
    amp = np.array([[AMP[c] for c in classes(n_blocks, 5 * r)] for r in range(rows)], F).reshape(rows, n_blocks)
    shape = (rows, n_blocks, block_det)
    mag = np.repeat(amp[:, :, None], block_det, axis=2) * rng.uniform(1.0, 1.05, shape)
    if not det_complex:
        return (mag * rng.choice([-1.0, 1.0], shape)).astype(F).reshape(rows, n_blocks * block_det)
    out = np.empty((rows, n_blocks, block_det, 2), F)
    out[..., 0] = mag * 0.8 * rng.choice([-1.0, 1.0], shape)
    out[..., 1] = mag * 0.6 * rng.choice([-1.0, 1.0], shape)
    return out.reshape(rows, n_blocks * block_det * 2)


def signal(rows, n, seed):
    """rows x n floats of noise with NaN payloads, a signalling NaN, -0, subnormals and infinities sprinkled in: the copy is of bits"""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (rows, n)).astype(F)
    u = x.view(np.uint32)
    if n:
        k = max(1, n // 7)
        pos = rng.integers(0, n, (rows, k))
        for r in range(rows):
            u[r, pos[r]] = SPECIALS[rng.integers(0, SPECIALS.size, k)]
    return x


def equality_case():
    """-> (det 1 x (8 * 256), block index b, its level L): quiet blocks and one block of unit noise whose level the thresholds sit on"""
    rng = np.random.default_rng(771)
    det = (0.05 * rng.uniform(-1, 1, (1, 8 * 256))).astype(F)
    b = 3
    det[0, b * 256:(b + 1) * 256] = rng.uniform(-1, 1, 256).astype(F)
    L = SM.levels(det, False, 256)[0, b]
    return det, b, L


def value_class_case():
    """-> det 1 x (6 * 256), real: blocks {ordinary H, one NaN sample, overflow in the sum, subnormal samples, powers that are subnormal,
    ordinary L}"""
    rng = np.random.default_rng(772)
    det = np.zeros((6, 256), F)
    det[0] = 1.5 * rng.choice([-1.0, 1.0], 256)
    det[1] = 1.5 * rng.choice([-1.0, 1.0], 256)
    det[1, 77] = np.nan
    det[2] = F(1.5e19) * rng.choice([-1.0, 1.0], 256).astype(F)       # each power is finite (2.25e38), their sum is not
    det[3] = F(1e-40) * rng.choice([-1.0, 1.0], 256).astype(F)        # subnormal samples: every power is +0
    det[4] = F(2.0 ** -70) * rng.choice([-1.0, 1.0], 256).astype(F)   # powers 2^-140: the level is subnormal
    det[5] = 0.2 * rng.choice([-1.0, 1.0], 256)
    return det.reshape(1, -1)


def states_array(rows, seed):
    rng = np.random.default_rng(seed)
    idx = rng.permutation(len(STATES_IN))
    return np.array([STATES_IN[idx[r % len(STATES_IN)]] for r in range(rows)], np.int32)
