"""What tests/tuner_tile_family_cases.py reaches, shown on the CPU from the models alone (tests/tuner_model.py, oracle/pipes_model.py)
and from the text of the launchers.  No assertion here depends on the library under test.

  * all 89 shapes tuner_fused_fits admits are in the table, and every row of the dispatch table holds the lengths listed for it;
  * the restated branch() is the dispatch of launch_tuner_bank_c4_shape and launch_tuner_c4_shape, read from their source;
  * every model run of the table is defined: no PipeAssert, N finite outputs, for every tap set, channel, seam and conversion;
  * the tight seam leaves one One output a buffer and Cross outputs in all three tiles of both tile advances; the wide seam satisfies
    the launcher's in-tile condition (the tight one does not) and puts its two seams' Cross outputs into the second and third tiles
    (none can lie in the first: the condition itself puts the first boundary behind the first tile's windows);
  * the cut run's launches start on the first Cross output and at odd and even outputs, so every output is compared in both of a
    thread's two output slots;
  * which table rows a defect confined to one branch would hit: dropping the last live tap chunk changes bits in every row of every
    shape; a walk one sample block short drops that chunk from a thread's second output only, and changes bits there in every row of
    every shape whichever parity the launch starts on."""
import re

import numpy as np
import pytest

import tuner_bank_cases as BC
import tuner_model as TM
import tuner_tile_family_cases as TF
from oracle import pipes_model as PM


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _src(name):
    return open(f"{TF.CSRC}/{name}").read()


# ---- the table and the dispatch ---------------------------------------------------------------------------------------------------------
def test_all_89_shapes_and_every_row_of_the_dispatch_table():
    assert len(TF.SHAPES) == 89 == len(set(TF.SHAPES))
    assert set(TF.SHAPES) == {(d, p) for d in range(1, 33) for p in range(1, 200) if TF.admitted(d, p)}
    rows = {b: sorted(p for d, p in TF.SHAPES if TF.branch(d, p) == b) for b in TF.BRANCHES}
    assert rows["D4"] == list(range(8, 129, 4))
    assert rows["D16/8"] == list(range(24, 129, 8))
    assert rows["D16/4"] == list(range(20, 125, 8))
    assert rows["D8 exact"] == [128]
    assert rows["D8/8"] == list(range(16, 121, 8))
    assert rows["D8/4"] == list(range(12, 125, 8))
    assert [len(rows[b]) for b in TF.BRANCHES] == [31, 14, 14, 1, 14, 15] and sum(len(r) for r in rows.values()) == 89
    # the small end of the guarded walks
    assert {(4, 8), (8, 12), (16, 20)} <= set(TF.SHAPES)
    for b, p in TF.PADDED.items():
        d = TF.BRANCHES[b][0]
        assert TF.branch(d, p) == b and {(d, p, p), (d, p, p - 1), (d, p, p - 3)} <= set(TF.TAP_SETS)
    assert len(TF.TAP_SETS) == 89 + 12


def test_branch_is_the_dispatch_of_both_launchers_read_from_the_source():
    for name in ("tuner_bank", "tuner"):
        lines = TF.dispatch_lines(name)
        assert [inst for _, inst in lines] == [(4, 4, True), (16, 8, True), (16, 4, True), (8, 8, False), (8, 8, True), (8, 4, True)], name
        for d, p in TF.SHAPES:
            assert TF.dispatched(lines, d, p) == TF.BRANCHES[TF.branch(d, p)], (name, d, p)
        for b, (d, tc, guard) in TF.BRANCHES.items():
            for p in (q for e, q in TF.SHAPES if TF.branch(e, q) == b):
                assert p % tc == 0 and (guard or p == 128), (b, p)           # a guarded walk takes whole tap chunks
    fits = _src("kernels_tuner.hip")
    assert "if (!((g.D == 8 || g.D == 4 || g.D == 16) && P >= 8 && P <= 128 && P % 4 == 0 && g.Lp == P && P > g.D)) return false;" in fits, \
        "tuner_fused_fits' shape condition changed: update tuner_tile_family_cases.admitted()"
    # every branch is compiled for the three formats and three forms (the one-row tuner: cfloat and u8; int16 takes the bank's kernel)
    bank = _src("kernels_tuner_bank.hip")
    for fmt in ("IN_U8", "IN_I16", "IN_CF32"):
        assert f"launch_tuner_bank_c4_shape<{fmt}, OUT>" in bank
    assert "launch_tuner_c4_shape<IN_U8>" in fits and "launch_tuner_c4_shape<IN_CF32>" in fits and "launch_tuner_c4_shape<IN_I16>" not in fits
    assert re.search(r"if \(fmt == IN_I16\) \{\n[^\n]*\n[^\n]*\n\s+return launch_tuner_bank\(", fits), "the one-row int16 tuner no longer takes the bank's kernel"


def test_the_in_tile_condition_holds_at_the_wide_seam_and_not_at_the_tight_one():
    cond = "g.seamBI >= (int64_t)T::OUTS * D + g.Lp"
    assert cond in _src("kernels_tuner_bank.hip") and cond in _src("kernels_tuner.hip"), "the launchers' in-tile condition changed"
    assert TF.OUTS == 512 and TF.ADV == 510 and TF.N == 1101
    for d, p in TF.SHAPES:
        none, tight, wide = TF.seams(d, p)
        assert none == 0 and p <= tight < p + d and tight % d == 0
        assert wide % d == 0 and wide - d < TF.OUTS * d + p <= wide
        assert TF.in_tile_condition(d, p, wide) and not TF.in_tile_condition(d, p, tight) and not TF.in_tile_condition(d, p, wide - d)
        assert TF.n_samples(d, p) == (TF.N - 1) * d + p <= 17728
        for seam in (tight, wide):
            assert TF.n_samples(d, p, seam) % seam == 0 and TF.n_samples(d, p, seam) <= TF.stream("u8").size // 2


def test_the_seams_put_cross_outputs_where_the_tiles_are():
    for d, p in TF.SHAPES:
        _, tight, wide = TF.seams(d, p)
        cr = TF.cross_outputs(d, p, tight)
        one = np.setdiff1d(np.arange(TF.N), cr)
        assert cr[0] == 1 and (np.bincount(one * d // tight) <= 1).all(), f"{d}/{p}: more than one One output in a buffer of the tight seam"
        assert cr.size >= TF.N - TF.N // 2 - 1
        for form in ("iq", "fm"):
            for a, b in TF.tile_ranges(form):
                assert ((cr >= a) & (cr < b)).any(), (d, p, form, a)
        cw = TF.cross_outputs(d, p, wide)
        assert cw.size >= 2 and len(set((cw * d + p - 1) // wide)) == 2 and (TF.N - 1) * d + p < 3 * wide, f"{d}/{p}: two seams in the stream"
        for form in ("iq", "fm"):
            t = TF.tile_ranges(form)
            assert not ((cw >= t[0][0]) & (cw < t[0][1])).any()
            assert ((cw >= t[1][0]) & (cw < t[1][1])).any() and ((cw >= t[2][0]) & (cw < t[2][1])).any(), (d, p, form)
        # an output whose window STARTS on the wide seam's first boundary is One: the residue test `rr >= seam` of the in-tile path
        m = wide // d
        assert m * d == wide and m < TF.N and m not in cw and m - 1 in cw


def test_the_cut_runs_start_on_cross_outputs_and_on_both_parities():
    for d, p in TF.SHAPES:
        for seam in TF.seams(d, p):
            cr = TF.cross_outputs(d, p, seam)
            for form in TF.FORMS:
                for fmt in TF.FORMATS:
                    c1, c2 = TF.cuts(d, p, seam, fmt, form)
                    ranges = TF.launches(d, p, seam, fmt, form, True)
                    assert ranges[0][0] == 0 and ranges[-1][1] == TF.N and len(ranges) == 3
                    if (fmt, d) == ("u8", 4):
                        assert c1 % 2 == 0 and c2 % 2 == 0
                        continue
                    if seam:
                        assert c1 == cr[0], "the second launch starts ON the first Cross output"
                    assert c2 == c1 + TF.advance(form) + 1
                    # a thread computes outputs k_begin + 2 t and k_begin + 2 t + 1: launches from an even and from an odd output put
                    # every output into both slots, beside the one run from 0
                    assert {a % 2 for a, _ in ranges} == {0, 1}, (d, p, seam, fmt, form)
            # fix-up launches: none without a seam; at the tight seam one per launch; at the wide one only with the in-tile path off
            whole = TF.launches(d, p, seam, "cf32", "iq", False)
            cut = TF.launches(d, p, seam, "cf32", "iq", True)
            if seam == 0:
                assert TF.fixup_launches(d, p, seam, cut, True) == 0 == TF.fixup_launches(d, p, seam, cut, False)
            elif not TF.in_tile_condition(d, p, seam):
                # (the cut run's first launch is output 0 alone, the One output of the first buffer)
                assert cut[0] == (0, 1) and TF.fixup_launches(d, p, seam, cut, True) == 2 and TF.fixup_launches(d, p, seam, whole, True) == 1
            else:
                assert TF.fixup_launches(d, p, seam, cut, True) == 0 and TF.fixup_launches(d, p, seam, whole, False) == 1
                # the first launch of the cut run ends on the first Cross output: it reads across no boundary
                assert TF.fixup_launches(d, p, seam, cut, False) == 2


# ---- every model run ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", TF.FACTORS)
def test_every_model_run_of_a_factor_is_defined(oracle, d):
    """No PipeAssert (tuner_expected would raise it), N finite outputs a row, the seams show in bits, the channels differ."""
    runs = 0
    for e, p, n in TF.TAP_SETS:
        if e != d:
            continue
        t = TF.taps(d, p, n)
        model = PM.FilterModel(oracle, t, PM.ORDER_AVX, complex_=True, factor=d)
        assert t.size == n and np.count_nonzero(t) == n and model.num_coeffs == p
        assert not model.cross_taps[n:].any() and model.cross_taps[n - 1] != 0
        shown = dict.fromkeys(TF.seams(d, p), 0)
        for fmt in ("u8", "i16"):
            for j in range(len(TF.tables())):
                rows = [TF.expected_iq(oracle, d, p, n, j, seam, fmt) for seam in TF.seams(d, p)]
                runs += len(rows)
                for seam, r in zip(TF.seams(d, p), rows):
                    assert r.size == 2 * TF.N and np.isfinite(r).all() and np.abs(r).max() > 0, (d, p, n, fmt, j, seam)
                    assert not r.flags.writeable
                    differ = np.nonzero((_bits(r) != _bits(rows[0])).reshape(-1, 2).any(axis=1))[0]
                    assert np.isin(differ, TF.cross_outputs(d, p, seam)).all(), "an output outside the rule's Cross set differs"
                    shown[seam] += differ.size
            heads = {_bits(TF.expected_iq(oracle, d, p, n, j, 0, fmt)[:64]).tobytes() for j in range(len(TF.tables()))}
            assert len(heads) == len(TF.tables())
        # (a lone row may keep its bits: the wide seam has one or two Cross outputs at the short lengths, the period-7 table is mostly zeros)
        assert shown[0] == 0 and all(v >= 1 for seam, v in shown.items() if seam), f"factor {d}, P {p} ({n} taps): a seam shows in no row: {shown}"
    print(f"    factor {d}: {runs} model runs")
    assert runs == 24 * sum(1 for e, _, _ in TF.TAP_SETS if e == d)


def test_the_forms_and_the_fm_state(oracle):
    d, p = 16, 36
    _, tight, _ = TF.seams(d, p)
    iq = TF.expected(oracle, "iq", d, p, p, 0, tight, "u8")
    env, fm = TF.expected(oracle, "env", d, p, p, 0, tight, "u8"), TF.expected(oracle, "fm", d, p, p, 0, tight, "u8")
    assert env.size == fm.size == TF.N and not env.flags.writeable and not fm.flags.writeable
    assert (TF.fm_state_before(oracle, d, p, p, 0, tight, "u8", 0) == 0).all()
    k = TF.cuts(d, p, tight, "u8", "fm")[1]
    import nfm_bank_cases as NC
    again = NC.demod(oracle, iq[2 * k:], TF.fm_state_before(oracle, d, p, p, 0, tight, "u8", k))
    assert (_bits(again) == _bits(fm[k:])).all(), "a launch from output k with the pair k - 1 as state continues the row"
    assert TF.expected(oracle, "env", d, p, p, 0, tight, "cf32") is env


# ---- what a defect confined to one branch would hit ------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", TF.FACTORS)
def test_a_dropped_tap_chunk_and_a_walk_one_sample_block_short_show_in_every_row_of_every_shape(oracle, d):
    """A guarded walk of nch_eff - 1 tap chunks loses the last TC taps of every output.  A walk of nb_eff - 1 sample blocks loses the
    last sample block of the thread's window, which only the thread's SECOND output meets, with its last tap chunk: outputs k_begin + 1,
    k_begin + 3, ... lose their last TC taps.  Both change bits in every channel's row at every length of the branch (every tap
    carries weight), the second among the odd outputs of a launch from an even output and among the even ones of a launch from an odd
    output -- and leaves the other parity alone."""
    for e, p, n in TF.TAP_SETS:
        if e != d:
            continue
        tc = TF.BRANCHES[TF.branch(d, p)][1]
        t = TF.taps(d, p, n)
        short = np.concatenate([t, np.zeros(p - n, np.float32)])
        short[p - tc:] = 0
        assert short.size == p and np.count_nonzero(short) == p - tc and np.count_nonzero(t[p - tc:]) >= 1
        x = TF.converted(oracle, "u8", TF.n_samples(d, p))
        for j, table in enumerate(TF.tables()):
            good = _bits(TF.expected_iq(oracle, d, p, n, j, 0, "u8")).reshape(-1, 2)
            bad = _bits(TM.tuner_expected(oracle, short, PM.ORDER_AVX, d, x, table, 0, 0, block_out=1)).reshape(-1, 2)
            assert bad.shape == good.shape == (TF.N, 2)
            changed = (good != bad).any(axis=1)
            what = f"factor {d}, P {p} ({n} taps), {TF.branch(d, p)}, channel {j}"
            for k0 in (0, 1):                                           # the launch's first output: even, odd
                second = (np.arange(TF.N) - k0) % 2 == 1                # the outputs a thread computes second
                assert (changed & second).any(), what + f": a walk one sample block short shows in no output of a launch from output {k0}"


def test_the_padded_sets_put_zero_taps_under_every_guarded_walk(oracle):
    for b, p in TF.PADDED.items():
        d, tc, _ = TF.BRANCHES[b]
        for z in (1, 3):
            model = PM.FilterModel(oracle, TF.taps(d, p, p - z), PM.ORDER_AVX, complex_=True, factor=d)
            assert model.num_coeffs == p and np.count_nonzero(model.cross_taps[p - z:]) == 0 and model.cross_taps[p - z - 1] != 0
            assert 1 <= np.count_nonzero(model.cross_taps[p - tc:]) == tc - z, "the last tap chunk holds zeros and at least one live tap"
            a, c = TF.expected_iq(oracle, d, p, p - z, 0, 0, "u8"), TF.expected_iq(oracle, d, p, p, 0, 0, "u8")
            assert (_bits(a) != _bits(c)).any()


def test_the_channels_and_their_periods():
    periods = [t.size // 2 for t in TF.tables()]
    assert periods == [1000, 1, 7, 5]
    for d in TF.FACTORS:
        assert (TF.ADV * d) % 5 == 0 and (TF.OUTS * d) % 5 != 0
        for n in (7, 1000):
            assert (TF.ADV * d) % n != 0 and (TF.OUTS * d) % n != 0
        # the fmDemod form's second and third tiles start at 510 and 1020, the others' at 512 and 1024; the third is ragged for both
        assert [a for a, _ in TF.tile_ranges("fm")] == [0, 510, 1020] and [a for a, _ in TF.tile_ranges("iq")] == [0, 512, 1024]
    assert (BC.straddlers(24, 10, 20, 16) == np.array([1, 2, 4, 5, 7, 8])).all()
