"""The CPU side of the gated-stream cases (tests/stream_order.py): what a gated run can show, checked before it costs GPU time.

For every case: the expected output exists and is finite where the operator's contract is bit parity; a stray launch would show
-- the output the models give for either poison stream equals the real stream's, bit for bit, at no more than 1 % of the outputs
(the spectrum operator: lies inside the real stream's tolerance at no more than 1 % of the bins); and in every seamed case at least
half of the Cross outputs differ between the sequential order and the SIMD order, so a fix-up that ran early and was overwritten by
the tile kernel would show as well.  Both shares are printed per case."""
import numpy as np
import pytest

import stream_order as SO


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("case", SO.CASES, ids=_ids(SO.CASES))
def test_a_stray_launch_would_show(oracle, case):
    exp = case.expected_real(oracle)
    assert set(case.states()) <= set(exp), "a state buffer without an expected final value"
    for name, e in exp.items():
        assert e.dtype == np.float32 and e.size > 0, name
        if not case.tolerance:
            assert np.isfinite(e).all(), f"{case.name}: non-finite expected {name}"
    for which in (1, 2):
        x = case.stream(which)
        assert x.dtype == case.stream(0).dtype and x.shape == case.stream(0).shape, "poison of another format or length"
        if case.tolerance:
            same = case.within(case.expected(oracle, x)["out"], case.stream(0))
            share = float(np.mean(same))
            print(f"{case.name}: poison {which}: {share:.4%} of the bins inside the real stream's tolerance")
            assert share <= 0.01
            continue
        poison = case.expected(oracle, x)
        for name, e in exp.items():
            if e.size < 100:                    # final states: a handful of floats, all of them must differ
                same = SO.same_bits(poison[name], e)
                print(f"{case.name}: poison {which}: {name}: {int(same.sum())} of {e.size} floats equal")
                assert not same.any(), f"{case.name}: {name} of poison stream {which} equals the real stream's"
                continue
            share = float(np.mean(SO.same_bits(poison[name], e)))
            print(f"{case.name}: poison {which}: {name}: {share:.4%} of the outputs equal the real stream's")
            assert share <= 0.01, f"{case.name}: {name}: a launch that read poison stream {which} would go unseen at {share:.2%} of the outputs"


@pytest.mark.parametrize("case", SO.SEAMED, ids=_ids(SO.SEAMED))
def test_an_overwritten_fix_up_would_show(oracle, case):
    total, differ = case.cross(oracle)
    print(f"{case.name}: {differ} of {total} Cross outputs differ between the sequential and the SIMD order ({differ / max(total, 1):.1%})")
    assert total > 0, "a seamed case without Cross outputs"
    assert 2 * differ >= total


def test_the_lists_name_cases():
    for name in SO.FIRST_RUN + [n for n, _ in SO.TWO_STREAMS] + [SO.MOST_LAUNCHES]:
        assert name in SO.BY_NAME, name
    kinds = {type(SO.BY_NAME[n]).__name__ + ":" + SO.BY_NAME[n].fmt for n in SO.FIRST_RUN}
    # one first-run case per descriptor type; the decimator on cfloat and on u8 (the scaled taps)
    assert {"Fir:f32", "Fir:cf32", "Fir:u8", "Tuner:u8", "TunerBank:u8", "Chain:u8", "FmBank:u8", "Spectrum:u8"} <= kinds


def test_the_two_pass_cases_make_at_least_three_pairs():
    """the plan; the GPU cases measure it: each pair whose chunk holds a seam moves the fix-up launch counter"""
    assert len(SO.two_pass_chunks()) >= 3 and SO.two_pass_seamed_chunks() >= 3
