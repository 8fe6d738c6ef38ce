"""The model of the squelch (include/sdr_hip.h "squelch"; sdr_amd/csrc/kernels_squelch.hip).  TEST INFRASTRUCTURE ONLY.

A gate decision per block: the level of a block is the mean power of its `block_det` detector samples, summed in a stated order
(256 slots, then a fold by halves); a gate with two levels and a hang walks the blocks of a row; the block's `block_sig` signal floats
are copied bit for bit where the gate is open and are +0.0 where it is shut.  numpy float32, every operation rounded, no FMA.  The
reference has no squelch, so this file is the definition's restatement, as deemph_model.py is de-emphasis'.  Vectorised across rows.

gate_walk is the definition (sequential over the blocks); gate_scan is the two-max-scan form the kernels use, held against it by
tests/test_squelch_model.py."""
import numpy as np

F = np.float32
SLOTS = 256


def powers(det, det_complex):
    """det: (..., m) floats (real) or (..., 2m) interleaved (complex) -> (..., m) float32 powers."""
    det = np.asarray(det, F)
    with np.errstate(all="ignore"):
        if not det_complex:
            return det * det
        a = det[..., 0::2] * det[..., 0::2]
        b = det[..., 1::2] * det[..., 1::2]
        return a + b


def levels(det, det_complex, block_det, n_blocks=None):
    """det: rows x (n_blocks * block_det [* 2]) floats (or one row) -> rows x n_blocks float32 levels (or one row of them)."""
    det = np.asarray(det, F)
    one = det.ndim == 1
    rows = np.atleast_2d(det)
    c = 2 if det_complex else 1
    if n_blocks is None:
        n_blocks = rows.shape[1] // (block_det * c)
    p = powers(rows[:, :n_blocks * block_det * c], det_complex).reshape(rows.shape[0], n_blocks, block_det)
    padded = -(-block_det // SLOTS) * SLOTS
    q = np.zeros((rows.shape[0], n_blocks, padded), F)               # +0 padding changes no bit: no p is negative, no sum is -0
    q[:, :, :block_det] = p
    q = q.reshape(rows.shape[0], n_blocks, padded // SLOTS, SLOTS)
    with np.errstate(all="ignore"):
        slot = q[:, :, 0, :].copy()
        for k in range(1, padded // SLOTS):
            slot = slot + q[:, :, k, :]
        w = SLOTS // 2
        while w >= 1:
            slot = slot[:, :, :w] + slot[:, :, w:2 * w]
            w //= 2
        inv = F(1.0 / block_det)
        lv = slot[:, :, 0] * inv
    assert lv.dtype == F
    return lv[0] if one else lv


def level_plain(det_block, det_complex):
    """One block's level by a plain Python loop in the stated order (no padding: an empty slot is +0)."""
    m = np.asarray(det_block).size // (2 if det_complex else 1)
    with np.errstate(all="ignore"):
        return F(sum_plain(det_block, det_complex) * F(1.0 / m))


def sum_plain(det_block, det_complex):
    """slot[0] behind the fold, by a plain Python loop: the level before its division"""
    det_block = np.asarray(det_block, F)
    m = det_block.size // (2 if det_complex else 1)
    slot = [None] * SLOTS
    with np.errstate(all="ignore"):
        for i in range(m):
            if det_complex:
                a = det_block[2 * i] * det_block[2 * i]
                b = det_block[2 * i + 1] * det_block[2 * i + 1]
                p = F(a + b)
            else:
                p = F(det_block[i] * det_block[i])
            j = i % SLOTS
            slot[j] = p if slot[j] is None else F(slot[j] + p)
        slot = [F(0.0) if s is None else s for s in slot]
        w = SLOTS // 2
        while w >= 1:
            for j in range(w):
                slot[j] = F(slot[j] + slot[j + w])
            w //= 2
        return slot[0]


def clamp_state(state, hang):
    det, left = int(state[0]), int(state[1])
    return (1 if det != 0 else 0), min(max(left, 0), hang)


def wants(level, open_level, close_level, open_above):
    """-> (want_open, want_close) bool arrays; a NaN level wants neither"""
    level = np.asarray(level, F)
    with np.errstate(invalid="ignore"):
        if open_above:
            return level >= F(open_level), level < F(close_level)
        return level <= F(open_level), level > F(close_level)


def gate_walk(lv, open_level, close_level, hang, open_above, state=(0, 0)):
    """THE DEFINITION.  lv: one row's levels -> (gates uint8, (det, hang_left))."""
    det, left = clamp_state(state, hang)
    wo, wc = wants(lv, open_level, close_level, open_above)
    gates = np.zeros(len(lv), np.uint8)
    for b in range(len(lv)):
        if wo[b]:
            det = 1
        elif wc[b]:
            det = 0
        if det:
            left = hang
            gates[b] = 1
        elif left > 0:
            left -= 1
            gates[b] = 1
    return gates, (det, left)


def gate_scan(lv, open_level, close_level, hang, open_above, state=(0, 0)):
    """The same by two max-scans, as the kernels compute it."""
    det_in, left_in = clamp_state(state, hang)
    n = len(lv)
    if n == 0:
        return np.zeros(0, np.uint8), (det_in, left_in)
    wo, wc = wants(lv, open_level, close_level, open_above)
    b = np.arange(n, dtype=np.int64)
    dec = np.where(wo, 1, np.where(wc, 0, -1))
    key = np.where(dec >= 0, 2 * b + np.maximum(dec, 0), -1)
    last = np.maximum.accumulate(key)
    det = np.where(last < 0, det_in, last & 1)
    last_open = np.maximum.accumulate(np.where(det == 1, b, -1))
    gates = np.where(last_open >= 0, b - last_open <= hang, b < left_in).astype(np.uint8)
    if det[-1]:
        fin = (1, hang)
    elif last_open[-1] >= 0:
        fin = (0, max(0, hang - (n - 1 - int(last_open[-1]))))
    else:
        fin = (0, max(0, left_in - n))
    return gates, fin


def squelch(det, det_complex, block_det, sig, block_sig, open_level, close_level, hang, open_above, states=None, n_blocks=None):
    """det: rows x floats; sig: rows x (n_blocks * block_sig) floats, or None (detect-only); states: rows x 2 int32 or None.
    -> (out like sig or None, final rows x 2 int32, levels rows x n_blocks, gates rows x n_blocks uint8)."""
    det = np.atleast_2d(np.asarray(det, F))
    rows = det.shape[0]
    c = 2 if det_complex else 1
    if n_blocks is None:
        n_blocks = det.shape[1] // (block_det * c)
    lv = levels(det, det_complex, block_det, n_blocks).reshape(rows, n_blocks)
    states = np.zeros((rows, 2), np.int32) if states is None else np.asarray(states, np.int32).reshape(rows, 2)
    gates = np.zeros((rows, n_blocks), np.uint8)
    final = np.zeros((rows, 2), np.int32)
    for r in range(rows):
        gates[r], final[r] = gate_walk(lv[r], open_level, close_level, hang, open_above, states[r])
    out = None
    if sig is not None:
        sig = np.atleast_2d(np.asarray(sig, F))[:, :n_blocks * block_sig]
        mask = np.repeat(gates, block_sig, axis=1).astype(bool)
        out = np.where(mask, sig.view(np.uint32), np.uint32(0)).astype(np.uint32).view(F)
    return out, final, lv, gates


def same_bits(a, b):
    """bit for bit -> bool array"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return a.view(np.uint32) == b.view(np.uint32)


def same_levels(a, b):
    """bit for bit, NaN by position -> bool array"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


# ---- the auto rule, restated (sdr_hip.h "squelch") ---------------------------------------------------------------------------------
WG, LS = 1, 2
WG_BLOCKS = 1024
WG_BYTES = 256 * 1024


def route(n_blocks, block_det, det_complex, block_sig, has_workspace):
    """block_sig = 0: detect-only"""
    row_bytes = 4 * n_blocks * (block_det * (2 if det_complex else 1) + block_sig)
    if n_blocks <= WG_BLOCKS and row_bytes <= WG_BYTES:
        return WG
    return LS if has_workspace else WG
