"""The de-emphasis model on its own (tests/deemph_model.py, tests/deemph_cases.py): no library, no device.

What the kernels' design rests on is restated here on the CPU: on ordinary inputs two trajectories of the rounded recurrence meet
within the default run-in, 40 / alpha samples; on an exactly constant input they never do; the one-workgroup scheme then reports
{0, 0, 0, chunks}, and non-zero repair words on the two stall rows; and the directed row's first NaN sits where the cases say."""
import numpy as np
import pytest

import deemph_cases as DC
import deemph_model as DM

F = np.float32
MEET_ALPHAS = [DM.alpha_of(*a) for a in DC.ALPHA_ARGS] + [DC.ONE]


def test_the_model_is_the_three_rounded_operations_in_order():
    x = DC.ordinary("noise", 200, 1)
    a = DC.A48
    y, want = F(0.375), []
    for v in x:
        d = F(v - y)
        m = F(a * d)
        y = F(y + m)
        want.append(y)
    out, fin = DM.deemph(x, a, 0.375)
    assert np.array_equal(out.view(np.uint32), np.array(want, F).view(np.uint32)) and fin.view(np.uint32) == want[-1].view(np.uint32)
    # a fused multiply-add would differ somewhere on this row: the definition is observable
    y, fused = 0.375, []
    for v in x:
        y = float(F(np.float64(y) + np.float64(a) * np.float64(F(v - F(y)))))
        fused.append(y)
    assert not np.array_equal(np.array(fused, F).view(np.uint32), out.view(np.uint32))
    rows, fins = DM.deemph(np.stack([x, x[::-1]]), a, np.array([0.375, -1.0], F))
    assert np.array_equal(rows[0].view(np.uint32), out.view(np.uint32)) and rows.shape == (2, 200) and fins.shape == (2,)
    o0, f0 = DM.deemph(np.zeros(0, F), a, 0.375)
    assert o0.size == 0 and f0 == F(0.375)


@pytest.mark.parametrize("alpha", MEET_ALPHAS, ids=lambda a: f"{float(a):.4f}")
def test_trajectories_meet_within_the_default_run_in_on_ordinary_rows(alpha):
    """true state against 0: bit-equal after at most 40 / alpha samples (the default run-in is that bound, rounded up to 4)"""
    bound = 40.0 / float(alpha)
    rng = np.random.default_rng(77)
    worst = 0.0
    n = int(bound) + 64
    for seed in range(12):
        for kind in DC.ORDINARY_KINDS:
            x = DC.ordinary(kind, n, seed)
            at = DM.meet_index(x, alpha, F(rng.normal(0, 2)), F(0.0))
            assert at is not None and at + 1 <= bound, f"{kind} seed {seed}: met after {at} samples, bound {bound:.1f}"
            worst = max(worst, (at + 1) * float(alpha))
    print(f"alpha {float(alpha):.4f}: the slowest meeting took {worst:.1f} / alpha samples (default run-in: 40 / alpha)")
    assert DM.default_run_in(alpha) >= bound and DM.default_run_in(alpha) % 4 == 0


@pytest.mark.parametrize("alpha", [DC.A48, DC.A256], ids=DC.ALPHA_IDS[:2])
def test_trajectories_never_meet_on_the_stall_rows(alpha):
    """A lane that starts from 0 inside the constant part (as a chunk's run-in does) against the true trajectory: never bit-equal."""
    n = 6000
    assert DM.meet_index(DC.constant(n), alpha, F(0.0), F(0.0), start=DC.STEP_LEN) is None
    assert DM.meet_index(DC.silent(n), alpha, F(0.0), F(0.0), start=DC.NOISE_LEN) is None


def test_alpha_one_copies_its_input_and_meets_at_once():
    """alpha = 1 has no memory worth the name: y + 1 * (x - y) from any finite state of the input's size -- the stall rows meet at once"""
    assert DM.meet_index(DC.constant(100), DC.ONE, F(0.0), F(0.0), start=DC.STEP_LEN) == DC.STEP_LEN
    assert DM.meet_index(DC.silent(400), DC.ONE, F(0.0), F(0.0), start=DC.NOISE_LEN) == DC.NOISE_LEN


def test_the_row_of_halves_stalls_from_both_sides():
    """the issue's own figures at alpha = 0.2425: 0x3F000002 from above, 0x3EFFFFFE from below; silence stalls at 2 * 2^-149"""
    x = np.full(3000, 0.5, F)
    assert DM.deemph(x, DC.A48, 2.0)[1].view(np.uint32) == 0x3F000002
    assert DM.deemph(x, DC.A48, 0.0)[1].view(np.uint32) == 0x3EFFFFFE
    z = np.zeros(3000, F)
    assert abs(int(DM.deemph(z, DC.A48, 0.3)[1].view(np.uint32))) == 2 and DM.deemph(z, DC.A48, 0.0)[1].view(np.uint32) == 0


@pytest.mark.parametrize("alpha", DC.ALPHAS, ids=DC.ALPHA_IDS)
def test_the_scheme_on_ordinary_rows_repairs_nothing(alpha):
    for r, x in enumerate(DC.ordinary_rows(4, 4096, 3)):
        out, fin, stats = DM.wg_scheme(x, alpha, 0.25)
        want, wfin = DM.deemph(x, alpha, 0.25)
        assert stats == (0, 0, 0, 256), f"row {r}: {stats}"
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and fin.view(np.uint32) == wfin.view(np.uint32)


@pytest.mark.parametrize("alpha", [DC.A48, DC.A256], ids=DC.ALPHA_IDS[:2])
@pytest.mark.parametrize("row", ["constant", "silent"])
def test_the_scheme_on_the_stall_rows_repairs_and_still_equals_the_model(alpha, row):
    x = DC.constant(4096) if row == "constant" else DC.silent(4096)
    out, fin, stats = DM.wg_scheme(x, alpha, 0.0)
    want, wfin = DM.deemph(x, alpha, 0.0)
    assert stats[0] > 0 and stats[2] > 0 and stats[1] == 0 and stats[3] == 256, stats
    assert stats[0] <= 256
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32)) and fin.view(np.uint32) == wfin.view(np.uint32)


def test_a_short_run_in_is_repaired():
    x = DC.ordinary("noise", 1024, 5)
    out, fin, stats = DM.wg_scheme(x, DC.A48, 0.25, run_in=4)
    assert stats[2] > 0 and stats[3] == 64
    assert np.array_equal(out.view(np.uint32), DM.deemph(x, DC.A48, 0.25)[0].view(np.uint32))


@pytest.mark.parametrize("alpha", DC.ALPHAS, ids=DC.ALPHA_IDS)
@pytest.mark.parametrize("variant", ["overflow", "inf", "nan"])
def test_the_directed_rows_first_nan_sits_where_the_cases_say(alpha, variant):
    x, at = DC.directed(4096, variant)
    assert at is not None
    assert np.signbit(x[1]) and x[1] == 0 and 0 < abs(x[2]) < 1.1754944e-38 and np.isinf(x[DC.INF_AT] if variant != "nan" else np.inf) and np.isnan(x[DC.NAN_AT])
    out, fin = DM.deemph(x, alpha, 0.0)
    assert DM.first_nan(out) == at, f"{variant}: first NaN at {DM.first_nan(out)}, the cases say {at}"
    assert np.isnan(out[at:]).all() and np.isnan(fin)
    # a prefix that ends before the NaN has none
    short, none = DC.directed(7, variant)
    assert none is None and not np.isnan(DM.deemph(short, alpha, 0.0)[0]).any()
