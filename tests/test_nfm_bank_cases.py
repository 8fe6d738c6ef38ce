"""The case table of the narrow-band FM bank's GPU tests (tests/nfm_bank_cases.py), shown FROM THE MODELS ALONE to reach what it is
for: launch ends around the overlapped tile's advance, the clauses of fmDemod the common case does not take (phase(0) from all-zero windows and
from a zero predecessor, exact +-pi, NaN and Inf predecessors), and Cross outputs at a tile's first output and as the predecessor of a One output.  No
device, no product code: it holds on any tree."""
import numpy as np

import am_bank_cases as AC
import nfm_bank_cases as NC
import tuner_bank_cases as BC

PI = np.float32(np.pi)


def test_launch_ends_sit_around_the_tile_advance():
    assert NC.ADV < NC.OUTS and NC.OUTS - NC.ADV == 2, "the overlap is one thread's pair"
    for want in (NC.ADV - 1, NC.ADV, NC.ADV + 1, NC.OUTS, 2 * NC.ADV + 1):
        assert want in NC.COUNTS
    # tile starts stay multiples of 16 bytes for all three input formats at factors 4, 8 and 16
    for factor in (4, 8, 16):
        for bytes_per_sample in (2, 4, 8):
            assert NC.ADV * factor * bytes_per_sample % 16 == 0
    assert all(c % 2 == 1 for c in NC.ODD_CUTS3) and NC.ODD_CUTS5[0] == 1


def test_silent_stretches_give_phase_of_zero_and_a_zero_predecessor(oracle):
    exp = {j: NC.expected(oracle, t, 0, "u8", stream="directed") for j, t in enumerate(NC.directed_tables())}
    iq = {j: NC.expected_iq(oracle, t, 0, "u8", stream="directed") for j, t in enumerate(NC.directed_tables())}
    start, edge = NC.inside(NC.SILENT[0]), NC.inside(NC.SILENT[1])
    assert start[0] == 0, "the launch's first output, from the zero state"
    assert edge[0] < NC.ADV < NC.OUTS < edge[-1], "the stretch crosses the first tile edge"
    for j in exp:
        for k in list(start) + list(edge):
            assert iq[j][2 * k] == 0 and iq[j][2 * k + 1] == 0
        for k in list(start) + list(edge[1:]):
            assert exp[j][k] == 0, "phase(0 * conj 0) is 0 (Demod.hs:27)"
        # a FIR sum that starts at +0 never becomes -0, so the zero OUTPUTS are +0; the zero signs fmDemod meets are those of the
        # PRODUCT y[k] * conj y[k - 1]: its imaginary part is 0 * (-0) + 0 * 0 = +0 and its real part 0 * 0 - 0 * (-0) = +0, while
        # the first output after the stretch multiplies a non-zero y[k] by conj (+0, +0) = (+0, -0): both zero signs, by y[k]'s
        assert not np.signbit(iq[j][2 * edge[0]:2 * edge[-1] + 2]).any()
        after = int(edge[-1]) + 1
        while iq[j][2 * after] == 0 and iq[j][2 * after + 1] == 0:
            after += 1
        assert exp[j][after] == 0 and iq[j][2 * after - 2] == 0, "a non-zero output on a zero predecessor: phase(+-0, +-0)"


def test_a_negative_zero_state_puts_both_zero_signs_under_phase_of_zero(oracle):
    """A FIR sum cannot yield -0, a STATE can: from (-0, -0) the silent start's first product is 0 * (-0) - 0 * 0 = -0 and
    0 * 0 + 0 * (-0) = +0 -- a zero of each sign under the `phase 0 = 0` clause -- where the (0, 0) state gives (+0, +0)."""
    iq = NC.expected_iq(oracle, BC.IDENTITY, 0, "u8", stream="directed")
    assert iq[0] == 0 and iq[1] == 0 and not np.signbit(iq[:2]).any()
    cur, prev = iq[:2], np.array([-0.0, -0.0], np.float32)
    nd = -prev[1]
    re, im = cur[0] * prev[0] - cur[1] * nd, cur[0] * nd + cur[1] * prev[0]
    assert re == 0 and im == 0 and np.signbit(re) and not np.signbit(im)
    for state in ((-0.0, -0.0), (0.0, -0.0), (-0.0, 0.0)):
        row = NC.demod(oracle, iq[:2 * 8], state)
        assert (row == 0).all() and not np.signbit(row).any(), "phase(+-0) is +0 whatever the zeros' signs (Demod.hs:27)"


def test_exact_plus_and_minus_pi(oracle):
    row = NC.expected(oracle, NC.PM1, 0, "u8", stream="directed")
    iq = NC.expected_iq(oracle, NC.PM1, 0, "u8", stream="directed")
    ks = NC.inside(NC.CONST)
    for k in ks[1:]:
        assert iq[2 * k] == -iq[2 * (k - 1)] and iq[2 * k] != 0, "y[k] = -y[k - 1] exactly"
        assert abs(row[k]) == PI
    got = {float(row[k]) for k in ks[1:]}
    assert got == {float(PI), float(-PI)}, "both +pi and -pi occur"
    # ... on a tile's first computed and first stored output, and on the first output of a launch (the GPU test cuts at ks[3])
    assert 2 * NC.ADV in ks[1:] and 2 * NC.ADV + 2 in ks[1:] and ks[3] > ks[0]


def test_nan_and_inf_predecessors(oracle):
    iq, row = NC.nonfinite_expected(oracle, BC.IDENTITY, BC.B)
    inf_w, nan_w = AC.window_outputs(AC.INF_AT), AC.window_outputs(AC.NAN_AT)
    assert np.isinf(iq[2 * inf_w[-1]]) or np.isnan(iq[2 * inf_w[-1]]), "a non-finite predecessor of the one output after the window"
    for w in (inf_w, nan_w):
        assert np.isnan(row[w[-1] + 1]), "the output after the window takes a non-finite predecessor"
        assert np.isfinite(row[w[-1] + 2])
    assert np.isnan(row[nan_w]).all()


def test_cross_outputs_at_a_tile_start_and_in_front_of_a_one_output():
    cross = BC.straddlers(BC.B, BC.K_ALL)
    tile_starts = set(range(0, BC.K_ALL, NC.ADV))
    assert tile_starts & set(cross.tolist()), "a Cross output is a tile's first output (seam 8192, factor 8)"
    last = int(cross[cross < 2 * BC.B // 8].max())
    assert last + 1 not in set(cross.tolist()), "a Cross output is the predecessor of a One output"
    # factor 16 with seam 8192: one tile spans more than a block, i.e. holds two seams
    assert NC.OUTS * 16 + NC.LP > BC.B and (NC.OUTS * 16) // BC.B >= 1
    # seam = Lp: every output but the one at a block's start is Cross
    every = BC.straddlers(NC.LP, 64)
    assert set(range(64)) - set(every.tolist()) == set(range(0, 64, NC.LP // 8))
