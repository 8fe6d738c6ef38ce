"""The squelch model against itself (tests/squelch_model.py): the two-scan form of the gate, which the kernels compute, equals the
sequential walk that defines it; the vectorised 256-slot level equals a plain loop in the stated order; zero padding changes no bit;
consecutive calls that hand the state on give the bits of one call."""
import numpy as np
import pytest

import squelch_cases as SC
import squelch_model as SM

F = np.float32


def _random_levels(rng, n):
    lv = rng.choice(np.array([0.0, 0.1, 0.25, 0.5, 1.0, 2.0, np.nan, np.inf], F), n)
    return lv.astype(F)


def test_the_scan_form_is_the_sequential_form():
    rng = np.random.default_rng(5)
    seen_final = set()
    for case in range(3000):
        n = int(rng.choice([0, 1, 2, 3, 5, 8, 13, 40]))
        lv = _random_levels(rng, n)
        hang = int(rng.choice([0, 1, 3, n + 2, 1000]))
        state = SC.STATES_IN[case % len(SC.STATES_IN)]
        for pol in SC.POLARITIES.values():
            g1, f1 = SM.gate_walk(lv, hang=hang, state=state, **pol)
            g2, f2 = SM.gate_scan(lv, hang=hang, state=state, **pol)
            assert np.array_equal(g1, g2) and tuple(f1) == tuple(f2), (lv, hang, state, pol, g1, g2, f1, f2)
            seen_final.add(tuple(int(v) for v in f1))
    assert len(seen_final) > 6


def test_a_carried_in_det_of_one_opens_nothing_behind_a_close_at_block_zero():
    """the case that tells the two readings of `last_open` apart: state {1, 0}, the first block closes, hang 3"""
    lv = np.array([0.1, 0.1], F)
    for fn in (SM.gate_walk, SM.gate_scan):
        g, f = fn(lv, hang=3, state=(1, 0), **SC.ABOVE)
        assert g.tolist() == [0, 0] and tuple(f) == (0, 0)
        g, f = fn(lv, hang=3, state=(1, 2), **SC.ABOVE)
        assert g.tolist() == [1, 1] and tuple(f) == (0, 0)


@pytest.mark.parametrize("det_complex", [False, True], ids=["real", "complex"])
def test_the_level_is_the_plain_loop_in_the_stated_order(det_complex):
    rng = np.random.default_rng(6)
    c = 2 if det_complex else 1
    for m in SC.BLOCK_DETS:
        x = (rng.normal(0, 1, (2, 3 * m * c)) * rng.choice([1e-3, 1.0, 300.0], (2, 3 * m * c))).astype(F)
        lv = SM.levels(x, det_complex, m)
        assert lv.shape == (2, 3) and lv.dtype == F
        for r in range(2):
            for b in range(3):
                want = SM.level_plain(x[r, b * m * c:(b + 1) * m * c], det_complex)
                assert lv[r, b].view(np.uint32) == want.view(np.uint32), (m, r, b, lv[r, b], want)
    # the order matters: a plain left-to-right sum gives other bits on at least one of these blocks
    x = rng.normal(0, 1, 4097).astype(F)
    seq = F(0)
    for v in x * x:
        seq = F(seq + v)
    assert F(seq * F(1.0 / 4097)).view(np.uint32) != SM.levels(x, False, 4097)[0].view(np.uint32)


def test_zero_padding_changes_no_bit():
    rng = np.random.default_rng(7)
    for det_complex in (False, True):
        c = 2 if det_complex else 1
        for m in (1, 3, 255, 257, 1000):
            x = rng.normal(0, 1, m * c).astype(F)
            for pad_to in (-(-m // 256) * 256, -(-m // 256) * 256 + 256):
                padded = np.zeros(pad_to * c, F)
                padded[:m * c] = x
                a, b = SM.sum_plain(x, det_complex), SM.sum_plain(padded, det_complex)
                assert a.view(np.uint32) == b.view(np.uint32), (m, pad_to)
    # -0 samples: their powers are +0, and so is the level
    assert SM.levels(np.full(300, -0.0, F), False, 300)[0].view(np.uint32) == 0


@pytest.mark.parametrize("pol", list(SC.POLARITIES), ids=list(SC.POLARITIES))
def test_consecutive_calls_are_one_call(pol):
    rows, nb, bd, bs = 3, SC.GATE_BLOCKS, 5, 7
    det = SC.detector(rows, nb, bd, True, 11)
    sig = SC.signal(rows, nb * bs, 12)
    for hang in (0, 1, 3, nb + 1):
        for st in ([(0, 0)] * rows, SC.states_array(rows, 13)):
            whole = SM.squelch(det, True, bd, sig, bs, hang=hang, states=st, **SC.POLARITIES[pol])
            for cuts in ([0, 20, 50, nb], [0, 1, 2, 40, 41, nb]):
                state, outs, lvs, gts = st, [], [], []
                for a, b in zip(cuts[:-1], cuts[1:]):
                    o, state, lv, g = SM.squelch(det[:, a * bd * 2:b * bd * 2], True, bd, sig[:, a * bs:b * bs], bs, hang=hang, states=state,
                                                 **SC.POLARITIES[pol])
                    outs.append(o), lvs.append(lv), gts.append(g)
                assert SM.same_bits(np.concatenate(outs, 1), whole[0]).all()
                assert np.array_equal(state, whole[1])
                assert SM.same_levels(np.concatenate(lvs, 1), whole[2]).all() and np.array_equal(np.concatenate(gts, 1), whole[3])


def test_the_output_is_a_copy_of_bits_or_plus_zero():
    det = SC.detector(1, SC.GATE_BLOCKS, 4, False, 14)
    sig = SC.signal(1, SC.GATE_BLOCKS * 4, 15)
    out, _, _, gates = SM.squelch(det, False, 4, sig, 4, hang=1, **SC.ABOVE)
    mask = np.repeat(gates, 4, axis=1).astype(bool)
    assert (out.view(np.uint32)[mask] == sig.view(np.uint32)[mask]).all() and (out.view(np.uint32)[~mask] == 0).all()
    assert mask.any() and (~mask).any() and np.isnan(out).any()
