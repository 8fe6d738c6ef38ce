"""The case table of the narrow-channel bank's GPU tests (tests/narrow_bank_cases.py), shown FROM THE MODELS ALONE to reach what it is
for: Cross outputs in stage 2 for every seamed pair, several seams inside one tile, Cross outputs that move through the tile's threads,
and Cross outputs on both sides of a One output under fmDemod.  No device, no product code: it holds on any tree."""
import numpy as np

import narrow_bank_cases as NB
import tuner_bank_cases as BC
from oracle import pipes_model as PM


def test_shapes_are_the_three_of_the_issue(oracle):
    for name, (taps, d2, lp2) in NB.SHAPES.items():
        model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=d2)
        assert model.num_coeffs == lp2 and model.factor == d2, name
    taps, d2, lp2 = NB.SHAPES["61/5"]
    assert taps.size == 61 and lp2 == 64 and d2 % 2 == 1, "an odd factor and three padded zero taps"
    assert NB.SHAPES["128/16"][1:] == (16, 128), "the fused route's limit"
    assert NB.n_out("24/4") >= 2 * NB.TILE + 1, "the 24 / 4 stream holds launches of two tiles and one output"
    assert NB.n_out("128/16") >= NB.TILE + 1


def test_the_model_of_stage_two_is_the_pipe_cut_into_blocks(oracle):
    """decimate2 with a block equals decimate2 without one at every One output and differs in summation order only at the Cross ones."""
    iq1 = BC.expected(oracle, BC.IDENTITY, NB.B)
    for shape in NB.SHAPES:
        whole = NB.decimate2(oracle, shape, iq1, 0)
        assert whole.size == 2 * NB.n_out(shape)
        for s2 in (1024, 1000, "Lp"):
            cut = NB.decimate2(oracle, shape, iq1, NB.seam2_of(shape, s2))
            assert (cut is not None) == NB.model_defined(shape, s2), (shape, s2)
            if cut is None:
                assert (shape, s2) == ("61/5", "Lp"), "the one pair the reference's Pipe asserts on: blocks of 64 and a factor of 5"
                continue
            cross = NB.cross2(shape, s2, cut.size // 2)
            one = np.setdiff1d(np.arange(cut.size // 2), cross)
            assert cut.size // 2 >= NB.n_out(shape) - NB.SHAPES[shape][2], (shape, s2)
            a, b = cut.reshape(-1, 2), whole.reshape(-1, 2)[:cut.size // 2]
            assert np.array_equal(a[one].view(np.uint32), b[one].view(np.uint32)), (shape, s2)
            assert not np.array_equal(a[cross].view(np.uint32), b[cross].view(np.uint32)), f"{shape}, {s2}: the Cross order shows in the bits"
            assert np.allclose(a, b, rtol=0, atol=1e-4)


def test_every_seamed_pair_has_cross_outputs_in_stage_two():
    for shape in NB.SHAPES:
        for seam, seam2 in NB.SEAM_PAIRS:
            cross = NB.cross2(shape, seam2)
            if seam2 == 0:
                assert cross.size == 0
            else:
                assert 0 < cross.size < NB.n_out(shape), (shape, seam, seam2)


def test_a_block_of_the_filters_length_puts_several_seams_into_one_tile():
    for shape, (_, d2, lp2) in NB.SHAPES.items():
        span = (NB.TILE - 1) * d2 + lp2                      # stage-1 outputs under one tile
        assert span // lp2 >= 2, shape
        cross = NB.cross2(shape, "Lp")
        ones = np.setdiff1d(np.arange(NB.n_out(shape)), cross)
        in_tile0 = ones[ones < NB.TILE]
        # one One output per block (the window that starts the block), the rest Cross: more than one block starts in tile 0
        assert in_tile0.size >= 2 and (ones * d2 % lp2 == 0).all(), shape


def test_a_block_of_1000_moves_the_cross_outputs_through_the_tiles_threads():
    """1024 / 4 is the tile: with seam_block2 = 1024 and D2 = 4 the Cross outputs sit on the same threads in every tile.  With 1000 the
    windows that cross a seam start at other threads of the tile from seam to seam (D2 = 4 and 5), and with D2 = 16, which does not
    divide 1000, also at other offsets from the seam."""
    same = NB.cross2("24/4", 1024) % NB.TILE
    assert set(same) == set(same[:5]), "seam 1024 / 4: one set of threads"
    for shape in ("24/4", "61/5"):
        _, d2, lp2 = NB.SHAPES[shape]
        cross = NB.cross2(shape, 1000)
        per = (lp2 - 1 + d2 - 1) // d2
        first = cross[::per][:5] if cross.size % per == 0 else cross[np.r_[True, np.diff(cross) > 1]]
        assert len(set(first % NB.TILE)) > 1, shape
    cross = NB.cross2("128/16", 1000)
    assert len(set((cross * 16) % 1000 % 16)) > 1, "windows start at more than one phase against the seam"


def test_fm_cases_hold_cross_outputs_on_both_sides_of_a_one_output():
    for shape in NB.SHAPES:
        for seam2 in (1024, 1000, "Lp"):
            cross = set(NB.cross2(shape, seam2).tolist())
            n = NB.n_out(shape)
            ones = [k for k in range(1, n - 1) if k not in cross]
            assert any(k - 1 in cross for k in ones), f"{shape}, {seam2}: a Cross predecessor of a One output"
            assert any(k + 1 in cross for k in ones), f"{shape}, {seam2}: a Cross successor of a One output"


def test_expected_rows_and_states(oracle):
    t = BC.bank_tables(3)[0]
    for form, dc in ((NB.ENV, False), (NB.ENV, True), (NB.FM, False)):
        e = NB.expected(oracle, t, "24/4", NB.B, 1024, "u8", form, dc)
        assert e.size == NB.n_out("24/4") and np.isfinite(e).all() and not e.flags.writeable
    iq2 = NB.expected_iq2(oracle, t, "24/4", NB.B, 1024, "u8")
    k = 601
    assert np.array_equal(NB.fm_state_before(oracle, t, "24/4", NB.B, 1024, "u8", k), iq2[2 * k - 2:2 * k])
    # a run over [k, n) from the states in front of k is the slice of the run over the whole stream
    fm = NB.demodulate(oracle, iq2[2 * k:], NB.FM, False, fm_state=iq2[2 * k - 2:2 * k])
    assert np.array_equal(fm.view(np.uint32), NB.expected(oracle, t, "24/4", NB.B, 1024, "u8", NB.FM)[k:].view(np.uint32))
    dcs = NB.dc_state_before(oracle, t, "24/4", NB.B, 1024, "u8", k)
    au = NB.demodulate(oracle, iq2[2 * k:], NB.ENV, True, dc_state=dcs)
    assert np.array_equal(au.view(np.uint32), NB.expected(oracle, t, "24/4", NB.B, 1024, "u8", NB.ENV, True)[k:].view(np.uint32))


def test_stage1_range_and_the_far_position():
    assert NB.stage1_range("24/4", 0, 1) == (0, 24) and NB.stage1_range("61/5", 7, 9) == (35, 104) and NB.stage1_range("61/5", 7, 7) == (35, 35)
    k = BC.FAR_K0
    for shape, (_, d2, _) in NB.SHAPES.items():
        j0 = k * d2
        assert (j0 * NB.D1) % NB.B % NB.D1 == 0 and j0 % 1024 % d2 == 0, shape
        assert j0 * NB.D1 > 2 ** 34
