"""Conditions on the INPUTS of the squelch tests (tests/squelch_cases.py), from the model alone: a gate case that never opens, never
closes or never hangs would let a broken gate pass.  These hold on any tree that has the model."""
import numpy as np
import pytest

import squelch_cases as SC
import squelch_model as SM

F = np.float32


def _trace(lv, hang, pol, state=(0, 0)):
    """the sequential walk with its inner values: per block (det before, det after, between, gate)"""
    det, left = SM.clamp_state(state, hang)
    wo, wc = SM.wants(lv, pol["open_level"], pol["close_level"], pol["open_above"])
    rows = []
    for b in range(len(lv)):
        before = det
        det = 1 if wo[b] else 0 if wc[b] else det
        if det:
            left, gate = hang, 1
        elif left > 0:
            left, gate = left - 1, 1
        else:
            gate = 0
        rows.append((before, det, not (wo[b] or wc[b]), gate))
    return rows


@pytest.mark.parametrize("pol", list(SC.POLARITIES), ids=list(SC.POLARITIES))
@pytest.mark.parametrize("hang", [1, 3])
@pytest.mark.parametrize("block_det,det_complex", [(1, False), (3, True), (256, False), (257, True), (1000, False)])
def test_every_gate_case_opens_closes_hangs_and_meets_a_between_level_both_ways(pol, hang, block_det, det_complex):
    rows = 3
    det = SC.detector(rows, SC.GATE_BLOCKS, block_det, det_complex, 100 + block_det)
    lv = SM.levels(det, det_complex, block_det)
    for r in range(rows):
        t = _trace(lv[r], hang, SC.POLARITIES[pol])
        gates = SM.gate_walk(lv[r], hang=hang, **SC.POLARITIES[pol])[0]
        assert [x[3] for x in t] == gates.tolist()
        assert any(a == 0 and b == 1 for a, b, _, _ in t), "no opening"
        assert any(a == 1 and b == 0 for a, b, _, _ in t), "no closing"
        assert any(b == 0 and g == 1 for _, b, _, g in t), "no block held open by the hang alone"
        assert any(g0 == 1 and g1 == 0 for g0, g1 in zip(gates[:-1], gates[1:])), "the gate never shuts"
        assert any(btw and a == 1 for a, _, btw, _ in t), "no between-level met while open"
        assert any(btw and a == 0 for a, _, btw, _ in t), "no between-level met while closed"
    assert not np.array_equal(lv[0], lv[1])


def test_the_classes_hold_for_every_block_length_and_both_detectors():
    for bd in SC.BLOCK_DETS:
        for cplx in (False, True):
            lv = SM.levels(SC.detector(2, len(SC.PATTERN), bd, cplx, 3), cplx, bd)
            for r in range(2):
                for b, c in enumerate(SC.classes(len(SC.PATTERN), 5 * r)):
                    v = lv[r, b]
                    assert (v < 0.9 * SC.LOW) if c == "L" else (1.1 * SC.LOW < v < 0.9 * SC.HIGH) if c == "M" else v > 1.1 * SC.HIGH, (bd, cplx, r, b, c, v)


def test_the_equality_case_sits_on_the_level_and_one_ulp_to_either_side():
    det, b, L = SC.equality_case()
    lv = SM.levels(det, False, 256)[0]
    assert lv[b].view(np.uint32) == L.view(np.uint32) and L > 0.2 and (np.delete(lv, b) < 0.01).all()
    up, down = np.nextafter(L, F(np.inf)), np.nextafter(L, F(-np.inf))
    assert up.view(np.uint32) == L.view(np.uint32) + 1 and down.view(np.uint32) == L.view(np.uint32) - 1
    hit = np.zeros(8, np.uint8)
    hit[b] = 1
    # opening above: >= opens on equality and one ulp under the level; > would not open on equality
    for open_level, want in ((L, hit), (down, hit), (up, 0 * hit)):
        g, _ = SM.gate_walk(lv, open_level, 0.01, 0, 1)
        assert np.array_equal(g, want)
    # opening below (every quiet block is open; the loud one decides): <= keeps the gate open on equality, and one ulp over it
    for open_level, want in ((L, 1), (up, 1), (down, 0)):
        g, _ = SM.gate_walk(lv, open_level, open_level, 0, 0)
        assert g[b] == want and g[:b].all()
    # the close level: < and > are strict, so equality does not close an open gate
    for close_level, want in ((L, 1), (up, 0)):
        g, _ = SM.gate_walk(lv[b:b + 1], F(10.0), close_level, 0, 1, state=(1, 0))
        assert g[0] == want


def test_the_value_class_case_holds_a_nan_an_overflow_and_subnormals():
    det = SC.value_class_case()
    lv = SM.levels(det, False, 256)[0]
    tiny = np.finfo(F).tiny
    assert lv[0] > 2 and np.isnan(lv[1]) and np.isposinf(lv[2]) and np.isfinite(det[0, 2 * 256:3 * 256] ** 2).all()
    assert lv[3].view(np.uint32) == 0 and (np.abs(det[0, 3 * 256:4 * 256]) < tiny).all()
    assert 0 < lv[4] < tiny and lv[5] < SC.LOW
    g, f = SM.gate_walk(lv, hang=0, **SC.ABOVE)
    assert g.tolist() == [1, 1, 1, 0, 0, 0]           # the NaN level leaves det as it was; +Inf opens
    g, f = SM.gate_walk(lv, hang=0, **SC.BELOW)
    assert g.tolist() == [0, 0, 0, 1, 1, 1]


def test_the_signal_rows_hold_bits_that_arithmetic_would_change():
    x = SC.signal(3, 1000, 9).view(np.uint32)
    for s in SC.SPECIALS:
        assert (x == s).any(), hex(int(s))
    assert len({tuple(s) for s in SC.STATES_IN}) == len(SC.STATES_IN) and any(s[1] < 0 for s in SC.STATES_IN) and any(s[0] not in (0, 1) for s in SC.STATES_IN)
