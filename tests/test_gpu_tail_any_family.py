"""GPU: the general fused audio tail (k_audio_tail_rows_any) on every part of the family its predicate admits.

For every launch of tests/tail_any_family_cases.py -- 109 coprime ratios with two and more (group length, filter length) each, the
tap-count edges, the ten shapes whose y window fills its 5120 floats on all four row alignments, launches that start and end off a
polyphase cycle, launches of fewer than I outputs, 32 rows, positions beyond 2^33 at blocks 250 and 257, rows with isolated
non-finite samples -- route 0 with mode 1 is held bit for bit, NaN by position, to the restated Pipes' composition
(oracle/pipes_model.py): no device code in the expected values.  One launch a shape holds route 2 to the same values.  At a block
inside the reference's undefined zone (tail_any_family_cases.asserts) there are no expected values: mode 1 is held to route 2 and
to mode 2 on route 0, at most once a shape.  Launch counters: a mode-1 run is exactly one launch of the general kernel a run, none
of k_audio_tail_rows and none of the row forms.  The y rows hold exactly what the launch may read, NaN between and around them; the
audio buffer starts as canaries and every float outside the rows' outputs is a canary afterwards.
tests/test_tail_any_family_cases.py shows on the CPU what the table reaches."""
import collections

import numpy as np
import pytest

import audio_tail_any_cases as AC
import tail_any_family_cases as FC
from conftest import assert_bit_equal
from test_gpu_audio_tail_any import run, tail_of

pytestmark = pytest.mark.gpu

SHAPES = list(FC.SHAPES.values())
_compared = collections.Counter()


def _expected_rows(oracle, case):
    s = case.shape
    if case.salted:
        return [FC.salted_row(s, case.block)], [FC.salted_expected(oracle, s, case.block)[case.q0:case.q1]]
    return ([AC.y_row(s, r) for r in range(case.rows)], [AC.expected(oracle, s, r, case.block, case.gain)[case.q0:case.q1] for r in range(case.rows)])


@pytest.mark.parametrize("shape", SHAPES, ids=[s.name for s in SHAPES])
def test_mode_1_against_the_restated_pipes(hip, oracle, shape):
    for case in FC.LAUNCHES[shape.name]:
        tail = tail_of(hip, shape, case.block, case.gain)
        assert tail.general_fits() and FC.general_fits(shape, case.block), case.name
        runs = len(case.cuts) + 1
        what = f"{case.name}, mode 1"
        if case.zone:
            ys = [AC.y_row(shape, r) for r in range(case.rows)]
        else:
            ys, exp = _expected_rows(oracle, case)
        outs, delta = run(hip, tail, shape, ys, case.q0, case.q1, 1, 0, case.exact, case.layout, case.cuts, case.far_shift, what)
        assert delta == (runs, 0, 0), f"{what}: launches (general, k_audio_tail_rows, row forms) {delta}"
        against = []
        if case.zone:
            against = [(2, 0), (1, 2)]                       # mode 2 inside route 0 and route 2 itself: the composition
        elif case.route2:
            against = [(1, 2)]
        comps = {}
        for mode, route in against:
            comp, d2 = run(hip, tail, shape, ys, case.q0, case.q1, mode, route, case.exact, case.layout, case.cuts, case.far_shift, what)
            assert d2[0] == 0 and d2[1] == 0 and d2[2] >= 2 * runs, f"{what}: mode {mode}, route {route}: {d2}"
            comps[mode, route] = comp
        if case.zone:
            for (mode, route), comp in comps.items():
                for r in range(case.rows):
                    assert_bit_equal(outs[r], comp[r], f"{what}, row {r} against mode {mode} on route {route}")
            _compared["zone", shape.I, shape.nloop, shape.nfc] += 1
            continue
        if not case.salted:
            assert all(np.isfinite(e).all() for e in exp) and (case.q1 - case.q0 < 8 or all(np.abs(e).max() > 0 for e in exp)), what
        for r in range(len(ys)):
            assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the restated Pipes")
            for (mode, route), comp in comps.items():
                assert_bit_equal(comp[r], exp[r], f"{case.name}, route {route}, row {r} against the restated Pipes")
        _compared["models", shape.I, shape.nloop, shape.nfc] += 1


def test_the_counts_the_family_was_compared_on():
    """Runs behind the table: what was compared, for the record."""
    total = collections.Counter()
    for (kind, I, nloop, nfc), n in _compared.items():
        total[kind] += n
        total[kind, "I", I] += n
        total[kind, "nloop", nloop] += n
        total[kind, "nfc", nfc] += n
    for kind in ("models", "zone"):
        print(f"    launch sets equal, {kind}: {total[kind]}")
        for axis, values in (("I", range(1, 9)), ("nloop", FC.NLOOPS), ("nfc", range(1, 9))):
            print(f"      by {axis}: " + ", ".join(f"{v}: {total[kind, axis, v]}" for v in values))
    if sum(_compared.values()) == len(FC.ALL_LAUNCHES):                  # the whole file ran: every part of the family was compared
        assert all(total["models", "I", I] > 0 for I in range(1, 9))
        assert all(total["models", "nloop", n] > 0 for n in FC.NLOOPS) and all(total["models", "nfc", f] > 0 for f in range(1, 9))
        assert total["zone"] == sum(1 for c in FC.ALL_LAUNCHES if c.zone)
