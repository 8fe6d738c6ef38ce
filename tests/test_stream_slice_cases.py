"""CPU: the table of tests/stream_slice_cases.py reaches what it is there for -- shown from the restated Pipes
(oracle/pipes_model.py) and a Python restatement of the seam rule (kernels.hpp) alone, no device."""
import numpy as np
import pytest

import stream_slice_cases as SC

CASE_IDS = [c.name for c in SC.CASES]


@pytest.fixture(params=SC.CASES, ids=CASE_IDS)
def near(request, oracle):
    case = request.param
    raw, exp, trace, Lp = SC.near(case, oracle)
    K = exp.size // case.width
    return case, K, trace, Lp


def _cross(case, Lp, lo, hi):
    return SC.is_cross(np.arange(lo, hi, dtype=np.int64), case.I, case.D, Lp, case.seam, case.out_block)


def test_the_restated_seam_rule_is_the_pipes_own_decision(near):
    """The rule every later check leans on: One / Cross by the restatement == the kinds of the Pipe's own kernel calls."""
    case, K, trace, Lp = near
    assert np.array_equal(_cross(case, Lp, 0, K), SC.cross_of_trace(trace, K))


def test_every_launched_range_has_one_and_cross_outputs(near):
    case, K, trace, Lp = near
    for pos in SC.positions(case, K):
        assert 0 <= pos.a < pos.b <= K
        c = _cross(case, Lp, pos.a, pos.b)
        assert c.any() and not c.all(), (case.name, pos)
        edges, route = SC.launch_edges(case, pos.a, pos.b, 0)
        assert edges[route + 1] - edges[route] >= case.min_launch
        assert _cross(case, Lp, edges[route], edges[route + 1]).any(), "the route launch has a seam inside"
        assert any((e - pos.a) % 2 for e in edges[1:-1]) or case.systolic, "launches cut at odd outputs"


def test_shifts_satisfy_the_translation_rule(near):
    case, K, trace, Lp = near
    I, D, Bk, outB = case.I, case.D, case.seam, case.shift_out_block
    assert np.gcd(I, D) == 1
    s0, s33, s40 = SC.shifts(case)
    assert s0 == 0 and (1 << 33) < s33 <= (1 << 33) + D * Bk * outB and (1 << 40) < s40 <= (1 << 40) + D * Bk * outB
    m = np.arange(0, K, dtype=np.int64)
    for s, bound in ((s33, 1 << 31), (s40, 1 << 40)):
        assert s % (D * Bk * outB) == 0 and s % Bk == 0
        T = SC.output_shift(case, s)
        assert T * D == s * I and T % I == 0 and T % outB == 0 and (T * D) % (Bk * I) == 0
        assert (T * D) // I > bound, "k_begin D leaves the range the family tests run in"
        assert np.array_equal(SC.in_offset(m + T, I, D), SC.in_offset(m, I, D) + s)
        assert np.array_equal(SC.is_cross(m + T, I, D, Lp, Bk, case.out_block), _cross(case, Lp, 0, K)), "the Cross set moved with S"


def test_half_a_block_moves_the_cross_set(near):
    """Position matters: where S + B / 2 is a legal shift (a whole number of output groups), the Cross set differs, so a kernel that
    ignored in_base in its seam arithmetic would be caught."""
    case, K, trace, Lp = near
    half = case.seam // 2
    if (half * case.I) % case.D or ((half * case.I) // case.D) % case.I:
        return                                                  # not a legal shift for this ratio
    T = half * case.I // case.D
    m = np.arange(0, K - T, dtype=np.int64)
    assert not np.array_equal(SC.is_cross(m + T, case.I, case.D, Lp, case.seam, 0), SC.is_cross(m, case.I, case.D, Lp, case.seam, 0))


def test_half_block_shift_is_legal_somewhere():
    legal = [c.name for c in SC.CASES if (c.seam // 2 * c.I) % c.D == 0 and (c.seam // 2 * c.I // c.D) % c.I == 0]
    assert len(legal) >= 10, legal


def test_slice_is_what_the_header_guarantees(near):
    """include/sdr_hip.h: a filter needs inputs [k_begin, k_end - 1 + numCoeffsF), a decimator [k_begin * factor,
    (k_end - 1) * factor + numCoeffsD), a resampler [in_offset(k_begin), in_offset(k_end - 1) + numCoeffsR / interpolation)."""
    case, K, trace, Lp = near
    for pos in SC.positions(case, K):
        lo, hi = SC.input_range(case.I, case.D, Lp, pos.a, pos.b)
        if case.family == "filter":
            assert (lo, hi) == (pos.a, pos.b - 1 + Lp)
        elif case.family == "decimator":
            assert (lo, hi) == (pos.a * case.D, (pos.b - 1) * case.D + Lp)
        else:
            first = lambda k: -((-k * case.D) // case.I)
            assert Lp % case.I == 0 and (lo, hi) == (first(pos.a), first(pos.b - 1) + Lp // case.I)
        assert hi <= case.nblk * case.seam, "the last window ends inside the near stream"
        assert lo >= {"delta 0": 0, "delta 40": 40}.get(pos.label, 41) and (lo == 0) == (pos.label == "delta 0")
        host = SC.guarded_slice(np.arange(case.nblk * case.seam, dtype=np.float32), 1, lo, hi, False)
        assert host.size == hi - lo + 2 * SC.GUARD and np.isnan(host[:SC.GUARD]).all() and np.isnan(host[-SC.GUARD:]).all()
        assert host[SC.GUARD] == lo and host[-SC.GUARD - 1] == hi - 1


def test_u8_guards_are_the_stream_with_the_top_bit_flipped():
    raw = np.arange(200, dtype=np.uint8)
    host = SC.guarded_slice(raw, 2, 10, 20, True)
    g = 2 * SC.GUARD
    assert np.array_equal(host[g:g + 20], raw[20:40])
    assert np.array_equal(host[g - 20:g], raw[0:20] ^ 0x80) and np.array_equal(host[g + 20:g + 40], raw[40:60] ^ 0x80)
    assert (host[:g - 20] == 0x7F).all()


def test_cuts_start_a_resampler_launch_at_every_group(near):
    case, K, trace, Lp = near
    if case.family != "resampler":
        return
    starts = set()
    for s, pos, q in SC.combos(case, K):
        edges, _ = SC.launch_edges(case, pos.a, pos.b, q)
        starts.update((SC.output_shift(case, s) + e) % case.I for e in edges[:-1])
    assert len(starts) == min(case.I, 9) or (case.I > 9 and len(starts) >= 9), (case.name, sorted(starts))


def test_the_irregular_seams_are_reached(oracle):
    """Somewhere in the table a launched range meets a boundary at which the Pipe does not cross over (seam_has_crossover false),
    and somewhere an output that late_output_is_one keeps out of the Cross set -- at an output block of 97 too, where T is no
    power of two."""
    no_crossover, late, late97 = [], [], []
    for case in SC.CASES:
        if case.family != "resampler" or case.I == 1:
            continue
        raw, exp, trace, Lp = SC.near(case, oracle)
        K = exp.size // case.width
        m = np.arange(0, K - 2, dtype=np.int64)
        seam_bi = case.seam * case.I
        edge = (m * case.D // seam_bi + 1) * seam_bi
        straddle = m * case.D + Lp > edge
        if (straddle & ~SC.seam_has_crossover(edge, case.I, case.D, Lp)).any():
            no_crossover.append(case.name)
        if (straddle & SC.late_output_is_one(m, edge, case.I, case.D, case.out_block)).any():
            (late97 if case.out_block == 97 else late).append(case.name)
    assert no_crossover and late97, (no_crossover, late, late97)
    print("no crossover:", no_crossover, "| late One:", late, "| late One at out_block 97:", late97)


def test_every_branch_of_the_stream_api_is_in_the_table():
    """One case per branch of fir_run and resamp_run_demod (sdr_amd/csrc/abi_device.cpp), each with a counter assertion or -- in
    the table's comments -- the reason no counter exists."""
    names = " | ".join(CASE_IDS)
    for branch in ("c4 /8 cfloat, Cross in the tile", "c4 /8 u8, Cross in the tile", "c4 /8 cfloat, fix-up", "c4 /8 u8, fix-up", "c4 /4", "c4 /16",
                   "systolic /8 u8", "systolic /8 cfloat", "c_orders", "filter_c4_tile", "filter_cplx4_fast", "fir_split complex",
                   "generic complex scalar /3 cfloat", "generic complex scalar /3 u8", "short seamed real filter", "real8_fast symmetric",
                   "real8_fast SSE", "real16 /2", "real16 /16 symmetric", "fir_split real", "generic real scalar",
                   "resample_3_10_fast real AVX", "resample_3_10_fast real SSE", "resample3c_fast", "thread-per-cycle 5/7 real",
                   "thread-per-cycle 5/7 complex", "resample_split", "generic 97/100", "real decimator's kernel 1/8",
                   "generic scalar 2/3 real", "generic scalar 2/3 complex", "short seamed real resampler"):
        assert branch in names, branch
    for case in SC.CASES:
        assert case.moves or case.still, case.name
        assert set(case.moves + case.still) <= set(SC.COUNTERS)
    assert sum(c.out_block == 97 for c in SC.CASES) == 2
