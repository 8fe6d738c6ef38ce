"""What tests/tail_family_cases.py reaches, shown on the CPU from the models alone (oracle/pipes_model.py and the seam rule restated in
tests/stream_slice_cases.py).  No assertion here depends on the library under test, except the host-only predicates of the last two
tests (AudioTail.fused_fits, the chain's plan: host arithmetic, no device).

  * every count 169 .. 192 prepares to the shape fm_tail_shape_ok admits, with the zero lanes its count implies, and all three patterns
    of zero lanes occur; 168 and 193 prepare to another shape;
  * the Cross term counts take a triple of their own at every count;
  * a kernel that carried 191 taps as a constant is told from the truth at every other count -- and HOW is stated: at 192 taps it drops
    a nonzero tap; below 191 its longer walk reads behind the end of the plain tap buffer, and is harmless exactly if zeros are there:
    what those counts pin is the zero fill, not the term count;
  * every (count, block) case with a seam holds Cross outputs of both stages (for chains: of all three) inside the compared range, at
    least one of which differs in bits from its grouped value, and more than two tiles of 2046 outputs;
  * the anchor's expectations are those of tests/audio_tail_cases.py, bit for bit;
  * no PipeAssert anywhere in the table (every expected value is computed here)."""
import os

import numpy as np
import pytest

import audio_tail_cases as AC
import signals as S
import tail_family_cases as TF
from oracle import pipes_model as PM


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------
def test_every_count_prepares_to_the_admitted_shape_with_the_zero_lanes_it_implies(oracle):
    patterns = set()
    for n in TF.COUNTS + TF.EDGES:
        taps = TF.resamp_taps(n)
        assert taps.size == n and taps[-1] != 0 and np.count_nonzero(taps) == n, n
        prep = oracle.prepare_coeffs(8, TF.I, TF.D, taps)
        shape = (prep["num_groups"], list(prep["increments"]), prep["padded_len"], PM.ResamplerModel(oracle, TF.I, TF.D, taps).num_coeffs)
        assert shape[2] == TF.nloop_of(n) and shape[3] == TF.rlp_of(n), (n, shape)
        nonzero = tuple(int(np.count_nonzero(g)) for g in prep["groups"])
        assert nonzero == TF.group_nonzero(n) and sum(nonzero) == n, (n, nonzero)
        for g, k in zip(prep["groups"], nonzero):
            assert not g[k:].any() and g[:k].all(), f"{n} taps: the zero lanes of a group are its last ones"
        if n in TF.COUNTS:
            assert shape == (3, [4, 3, 3], 64, 192) and TF.in_family(n), (n, shape)
            k = nonzero[0]
            patterns.add(tuple(x - k for x in nonzero))
        else:
            assert shape[:2] == (3, [4, 3, 3]) and (shape[2], shape[3]) != (64, 192) and not TF.in_family(n), (n, shape)
    assert patterns == {(0, -1, -1), (0, -1, 0), (0, 0, 0)}
    assert TF.group_nonzero(169) == (57, 56, 56) and TF.group_nonzero(191) == (64, 63, 64) and TF.group_nonzero(192) == (64, 64, 64)
    assert [(e.nloop, e.rlp) for e in TF.EDGE_SHAPES] == [(56, 168), (72, 216)]
    assert TF.ntaps(TF.ANCHOR) == 191 and TF.in_family(191)


def test_the_cross_term_counts_take_many_triples():
    triples = {TF.cross_terms(n) for n in TF.COUNTS}
    assert len(triples) >= 6 and len(triples) == len(TF.COUNTS)                # they sum to the count: no two counts share one
    assert TF.cross_terms(191) == (64, 64, 63) and TF.cross_terms(169) == (57, 56, 56) and TF.cross_terms(192) == (64, 64, 64)
    assert {TF.cross_terms(n) for n in TF.CHAIN_COUNTS} >= {(57, 56, 56), (57, 57, 56), (57, 57, 57), (60, 60, 60), (64, 63, 63), (64, 64, 64)}
    for n in TF.COUNTS:
        assert sum(TF.cross_terms(n)) == n


def test_the_decimator_sets_prepare_to_128_taps_with_one_two_three_and_no_padding_zeros(oracle):
    for n, zeros in ((127, 1), (126, 2), (125, 3), (128, 0)):
        taps = TF.decim_taps(n)
        model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=TF.DECIM)
        assert taps.size == n and taps[-1] != 0 and model.num_coeffs == 128
        assert np.count_nonzero(model.cross_taps[128 - zeros:]) == 0 and model.cross_taps[127 - zeros] != 0
    assert set(TF.DECIM_COUNTS) | {127} == {125, 126, 127, 128}


def test_the_blocks_are_the_ones_the_seam_arithmetic_has_not_met():
    assert TF.BLOCKS == (0, 8192, 7315, 7316, 8191) and AC.MIN_BLOCK == 7314
    for b in (7315, 8191):
        assert b % 2 == 1 and b % 8 != 0 and b % 3 != 0 and b % 10 != 0
    assert 7315 % 3 == 1 and 7316 % 3 == 2
    for b in TF.BLOCKS:
        assert AC.fused_fits(b)
        assert AC.late_first_outputs(b, 0, 40 * b).size == 0, b           # audio_tail_cases: none for seam block = output block, 3/10


# ---- a 191-shaped kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [n for n in TF.COUNTS if n != 191])
def test_a_kernel_that_carried_191_as_a_constant_is_told_from_the_truth(oracle, n):
    """One seam of block 8192, row 0.  The sequential kernel restated here gives the model's Cross outputs bit for bit with the set's
    own term counts.  With 191's term counts (64, 64, 63):
      * 192 taps: the walk of filter offset 2 stops one tap early, and that tap is not zero: outputs differ in bits;
      * fewer than 191 taps: the walk runs past the set's last tap.  The plain tap buffer ends there (abi_device.cpp uploads exactly
        ntaps floats), so what the walk reads is whatever lies behind the buffer; with any nonzero value there, outputs differ in bits.
        With zeros there they do NOT: +0 products leave a sequential sum from +0 as it is on finite samples.  So below 191 the table
        pins the kernel's own zero fill of its tap copy behind ntaps (and its reading no further than ntaps), not the term count."""
    block = 8192
    taps, y = TF.resamp_taps(n), TF.y_row(0)
    z, _ = TF.rows_streams(oracle, n, 0, block)
    z_one, _ = TF.rows_streams(oracle, n, 0, 0)
    cross = TF.resampler_cross(block, 0, 3000)
    assert 15 <= cross.size <= 21 and cross.max() - cross.min() == cross.size - 1, "one seam's Cross outputs, consecutive"
    own = np.array([TF.sequential_z(taps, y, m) for m in cross], np.float32)
    assert (_bits(own) == _bits(z[cross])).all(), "the restated sequential kernel is the model's"
    assert (_bits(z[cross]) != _bits(z_one[cross])).any(), "the seam shows in bits"
    t191 = TF.cross_terms(191)
    wrong = np.array([TF.sequential_z(taps, y, m, terms=t191, behind=1.0) for m in cross], np.float32)
    differ = int((_bits(wrong) != _bits(own)).sum())
    fo = (-(TF.D * cross)) % TF.I
    changed = np.array([t191[f] != TF.cross_terms(n)[f] for f in fo])
    print(f"    {n} taps: {cross.size} Cross outputs at the first seam, {int(changed.sum())} walk another term count under 191's, {differ} differ in bits")
    assert changed.any() and differ >= 1
    assert (_bits(wrong[~changed]) == _bits(own[~changed])).all()
    if n < 191:
        filled = np.array([TF.sequential_z(taps, y, m, terms=t191, behind=0.0) for m in cross], np.float32)
        assert (_bits(filled) == _bits(own)).all(), "zeros behind the last tap make the longer walk harmless"
        assert differ == int(changed.sum()), "every output whose walk grew read behind the buffer"


# ---- the rows table --------------------------------------------------------------------------------------------------------------------
def test_the_anchor_is_the_audio_tail_tables_own(oracle):
    for block in TF.rows_blocks(TF.ANCHOR):
        for row in range(TF.ROWS):
            assert (_bits(TF.rows_expected(oracle, TF.ANCHOR, row, block)) == _bits(AC.expected(oracle, row, block)[:TF.Q_MAX])).all(), (block, row)
    assert (TF.y_row(1)[:AC.N_Y] == AC.y_row(1)).all() and TF.y_row(1).size == TF.N_Y_MAX > AC.N_Y


@pytest.mark.parametrize("key,block", TF.ROWS_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.ROWS_CASES])
def test_a_rows_case_holds_cross_outputs_of_both_stages_that_differ_in_bits(oracle, key, block):
    z, a = TF.rows_streams(oracle, key, 0, block)
    assert np.isfinite(a[:TF.Q_MAX]).all() and np.abs(a[:TF.Q_MAX]).max() > 0
    assert TF.Q_MAX > 2 * TF.TILE and all(0 < c < TF.Q_MAX for c in TF.ROWS_CUTS) and any(c % TF.TILE not in (0, 1) for c in TF.ROWS_CUTS)
    if block == 0:
        return                                                      # a contiguous stream: every output is One
    z_one, _ = TF.rows_streams(oracle, key, 0, 0)
    a_one = AC.filter_stream(oracle, z, 0)[:TF.Q_MAX]
    rc, fc = TF.resampler_cross(block, 0, TF.Q_MAX + TF.LF - 1), TF.filter_cross(block, 0, TF.Q_MAX)
    r_diff, f_diff = rc[_bits(z[rc]) != _bits(z_one[rc])], fc[_bits(a[fc]) != _bits(a_one[fc])]
    print(f"    {key} taps, block {block}: {rc.size} resampler Cross outputs ({r_diff.size} differ in bits), {fc.size} filter Cross ({f_diff.size} differ)")
    assert rc.size >= 15 and fc.size == TF.LF - 1 and r_diff.size >= 1 and f_diff.size >= 1
    n = min(z.size, z_one.size)
    other = np.nonzero(_bits(z[:n]) != _bits(z_one[:n]))[0]
    assert np.isin(other, TF.resampler_cross(block, 0, n)).all(), "an output outside the rule's Cross set differs"


@pytest.mark.parametrize("key,block", TF.ROWS_LONG_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.ROWS_LONG_CASES])
def test_a_long_rows_case_holds_a_second_filter_seam_in_tiles_that_start_past_the_first(oracle, key, block):
    """Below the first boundary a tile's position modulo the block is the position itself, whatever the block: [0, Q_MAX) cannot
    tell `qa % seam` from `qa % (seam - 1)`.  The long cases hold Cross outputs of both stages, different in bits from their grouped
    values, in tiles whose start lies past the first boundary and whose reduction modulo the block differs from the one modulo its
    neighbour block - 1 -- for the launch from 0 and for the one from Q_LONG_START."""
    z, a = TF.rows_streams(oracle, key, 0, block, long=True)
    z_one, _ = TF.rows_streams(oracle, key, 0, 0, long=True)
    a_one = AC.filter_stream(oracle, z, 0)[:TF.Q_LONG]
    assert np.isfinite(a[:TF.Q_LONG]).all() and block < TF.Q_LONG_START < 2 * block - TF.LF and 2 * block < TF.Q_LONG
    fc = TF.filter_cross(block, block, TF.Q_LONG)
    assert fc.size == TF.LF - 1 and fc.min() == 2 * block - TF.LF + 1 and (_bits(a[fc]) != _bits(a_one[fc])).any()
    rc = TF.resampler_cross(block, TF.Q_LONG_START, TF.Q_LONG + TF.LF - 1)
    assert rc.size >= 3 * 15 and (_bits(z[rc]) != _bits(z_one[rc])).sum() >= 3
    for q0 in (0, TF.Q_LONG_START):
        qa = q0 // 3 * 3 + (fc - q0 // 3 * 3) // TF.TILE * TF.TILE          # the tiles of the second seam's Cross outputs
        assert (qa > block).all() and (qa % block != qa % (block - 1)).all() and (qa % block != qa).all(), (key, block, q0)
        c0 = (q0 // 3 * 3 + (rc - q0 // 3 * 3) // TF.TILE * TF.TILE) // 3
        assert ((30 * c0) % (3 * block) != 30 * c0).all()


def test_the_rows_table_runs_what_the_issue_names():
    assert len(TF.COUNTS) == 24 and set(TF.COUNTS) == set(range(169, 193))
    for key in TF.TAP_SETS:
        blocks = TF.rows_blocks(key)
        assert {8192, 7315} <= set(blocks)
        assert set(blocks) == set(TF.BLOCKS) if key in (169, 170, 171, 190, 192) else len(blocks) == 2
    assert TF.ROWS == 3 and TF.ROWS_CUTS == (2047, 6001)


# ---- the chains and banks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,block", TF.CHAIN_CASES + [TF.DECIM_CASE], ids=[f"{k} taps, block {b}" for k, b in TF.CHAIN_CASES] + ["decimator sets"])
def test_a_chain_case_yields_audio_with_cross_outputs_of_every_stage(oracle, key, block):
    decims = (127,) + TF.DECIM_COUNTS if (key, block) == TF.DECIM_CASE else (127,)
    for dn in decims:
        e = TF.chain_expected(oracle, key, block, dn)
        assert e.size == block and np.isfinite(e).all() and np.abs(e).max() > 0, (key, block, dn, e.size)
    n = e.size
    assert n > 2 * TF.TILE
    r = TF.chain_stage_ranges(0, n, TF.ntaps(key))
    assert TF.filter_cross(block, 0, n).size == TF.LF - 1
    assert TF.resampler_cross(block, 0, r["m1"]).size >= 15
    assert TF.decimator_cross(block, r["kd0"], r["kd1"]).size >= 15
    assert TF.CHAIN_NBLK * block >= (r["kd1"] - 1) * TF.DECIM + 128, "the source blocks hold the receptive field"


@pytest.mark.parametrize("key,block", TF.CHAIN_LONG_CASES, ids=[f"{k} taps, block {b}" for k, b in TF.CHAIN_LONG_CASES])
def test_a_long_chain_case_yields_two_audio_blocks(oracle, key, block):
    e = TF.chain_expected(oracle, key, block, nblk=TF.CHAIN_LONG_NBLK)
    assert e.size == 2 * block and np.isfinite(e).all() and np.abs(e[block:]).max() > 0
    assert TF.filter_cross(block, block, 2 * block).size == TF.LF - 1
    assert (key, block) in TF.CHAIN_CASES


def test_a_chain_of_another_count_is_another_receiver(oracle):
    """The expected audio depends on the tap set: no two counts of a block share their first audio samples."""
    for block in TF.CHAIN_BLOCKS:
        heads = {_bits(TF.chain_expected(oracle, key, block)[:64]).tobytes() for key in TF.CHAIN_COUNTS}
        assert len(heads) == len(TF.CHAIN_COUNTS), block


@pytest.mark.parametrize("fmt,key,block", TF.BANK_CASES, ids=[f"{f}, {k} taps, block {b}" for f, k, b in TF.BANK_CASES])
def test_a_bank_case_yields_one_audio_block_per_station(oracle, fmt, key, block):
    es = [TF.bank_expected(oracle, fmt, name, key, block) for name in TF.STATIONS]
    for e in es:
        assert e.size == block and np.isfinite(e).all() and np.abs(e).max() > 0
    assert not np.array_equal(es[0], es[1])
    if fmt == "u8":
        assert not np.array_equal(es[0], TF.chain_expected(oracle, key, block)), "the oscillator stage shows"


def test_the_edge_shapes_have_expectations_of_their_own(oracle):
    for n in TF.EDGES:
        for block in (0, TF.EDGE_BLOCK):
            for row in range(TF.ROWS):
                e = TF.rows_expected(oracle, n, row, block)
                assert e.size == TF.Q_MAX and np.isfinite(e).all() and np.abs(e).max() > 0
        e = TF.chain_expected(oracle, n, TF.EDGE_BLOCK)
        assert e.size == TF.EDGE_BLOCK and np.isfinite(e).all() and np.abs(e).max() > 0
        assert TF.resampler_cross(TF.EDGE_BLOCK, 0, TF.Q_MAX, TF.rlp_of(n)).size >= 15


# ---- host-only predicates of the library --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def test_fused_fits_on_the_host(L):
    def fits(n, block):
        t = L.AudioTail(TF.I, TF.D, TF.resamp_taps(n), TF.audio_half(), gain=1.0, block=block)
        try:
            return t.fused_fits()
        finally:
            t.close()
    for n in (169, 192):
        for block in (0, 7314, 7315, 8191):
            assert fits(n, block), (n, block)
        assert not fits(n, 7313), n
    for n in TF.COUNTS:
        assert fits(n, 8192) == TF.in_family(n) and fits(n, 7316), n
    for n in TF.EDGES:
        for block in (0, 7314, 7315, 8191, 8192):
            assert not fits(n, block), (n, block)


def test_the_chains_plan_on_the_host(L):
    """The plan of every chain case covers the audio block the Pipes yield, from the stream's start and without a halo."""
    for key, block in TF.CHAIN_CASES + [(n, TF.EDGE_BLOCK) for n in TF.EDGES]:
        ch = L.FmChain(TF.DECIM, TF.decim_taps(), TF.I, TF.D, TF.resamp_taps(key), TF.audio_half(), TF.GAIN, block)
        total = TF.CHAIN_NBLK * block
        q0, q1, halo = ch.plan(0, total, total)
        n = TF.ntaps(key)
        decimated = (total - 128) // TF.DECIM + 1
        assert (q0, halo) == (0, 0) and q1 == (decimated * TF.I - TF.rlp_of(n)) // TF.D + 1 - (TF.LF - 1) >= block, (key, block, q1)
        ch.close()
