"""The case table of the record-seam Pipe tests (tests/record_pipe_cases.py) reaches what it is there to reach.  Conditions on the
INPUTS, checked on the model alone (no device): tests/test_gpu_record_pipes.py then runs the very same cases on the device, and a
table that drifts away from a transition or branch fails here, where it is cheap to see why."""
import collections

import pytest

from oracle import pipes_model as PM
import record_pipe_cases as RC


@pytest.fixture(scope="module")
def runs(oracle):
    """Every case at every output block size through the plain model: {(case, out_block): (calls, trace, blocks yielded)}.
    A PipeAssert of the reference fails the whole module here."""
    out = {}
    for c in RC.CASES:
        for ob in RC.OUT_BLOCKS:
            m = RC.make_model(c, oracle)
            calls = RC.instrument(m)
            try:
                yielded, trace = RC.run_pipe(c, m, ob)
            except PM.PipeAssert as e:
                pytest.fail(f"{RC.case_id(c)} at blockSizeOut {ob}: the reference's assert `{e}` fires")
            assert [(k[0], k[1]) for k in calls] == trace
            out[(c, ob)] = (calls, trace, len(yielded))
    return out


def test_the_table_is_the_one_described():
    ids = [RC.case_id(c) for c in RC.CASES]
    assert len(set(ids)) == len(ids)
    fir = [c for c in RC.FIR_CASES if c.kind == "fir"]
    sym = [c for c in RC.FIR_CASES if c.kind == "sym"]
    # 3 orders x 2 data types x 6 factors x 4 tap counts, less the combinations whose padded length does not exceed the factor
    dropped = [(o, x, f, t) for o in RC.ORDERS for x in (False, True) for f in RC.FIR_FACTORS for t in RC.FIR_TAPS
               if RC.num_coeffs(RC.Case("fir", o, x, f, t, 1, f)) <= f]
    assert len(fir) == 144 - len(dropped) and all(t == 5 and f in (5, 8, 16) for _, _, f, t in dropped)
    assert all(RC.num_coeffs(c) > c.factor for c in RC.FIR_CASES)
    assert len(sym) == 2 * 3 * 4 and all(not c.cplx and c.order != "scalar" for c in sym)
    assert len(RC.RESAMPLER_CASES) == 3 * 2 * 7 * 3 + 2
    many = [c for c in RC.RESAMPLER_CASES if (c.I, c.D) == RC.MANY_GROUPS]
    assert sorted(c.ntaps for c in many) == [291, 500] and all(c.order == "avx" and not c.cplx for c in many)
    assert {k for k, _, _ in RC.GROUPS} == {"fir", "sym", "resampler"} and len(RC.GROUPS) == 6 + 2 + 6
    for c in RC.CASES:
        lens = RC.block_lengths(c)
        L = RC.num_coeffs(c)
        lo = PM.quot_up(L, c.I) + c.D if c.kind == "resampler" else L + c.factor
        hi = 3 * lo + 200 if c.kind == "resampler" else 3 * L + c.factor + 200
        assert len(lens) == RC.NUM_BLOCKS == 12 and all(lo <= n <= hi for n in lens)
        assert [b.size for b in RC.blocks(c)] == [n * (2 if c.cplx else 1) for n in lens]
    assert RC.OUT_BLOCKS == (97, 1000)


def test_no_case_trips_an_assert_of_the_reference(runs):
    assert len(runs) == 2 * len(RC.CASES)
    for (c, ob), (calls, trace, yielded) in runs.items():
        assert len(calls) >= RC.NUM_BLOCKS, (RC.case_id(c), ob)
        if ob == min(RC.OUT_BLOCKS):
            assert yielded >= 1, f"{RC.case_id(c)} yields no block even at blockSizeOut {ob}"


def test_every_family_reaches_every_transition(runs):
    """one -> one and cross -> cross are the output block filling up inside a buffer and inside a crossover; cross -> cross is also
    the only way buf_last survives a cross call (Filter.hs:563-569, 605-611, 720-727): the next call then gets its shortened tail."""
    seen = collections.defaultdict(collections.Counter)
    survived = collections.defaultdict(set)
    for (c, ob), (calls, trace, _) in runs.items():
        for a, b in zip(calls, calls[1:]):
            seen[RC.family(c)][(a[0], b[0])] += 1
            if a[0] == "cross" and b[0] == "cross":
                # the same `next`, and a strictly shorter, non-empty `last`: drop (count * D [- offset] / I) last
                assert b[3] == a[3] and 0 < b[2] < a[2], (RC.case_id(c), a, b)
                survived[RC.family(c)].add(c)
    families = {RC.family(c) for c in RC.CASES}
    assert len(families) == 6 + 6 + 2 + 2 + 6
    for f in sorted(families):
        for t in (("one", "one"), ("cross", "cross"), ("cross", "one"), ("one", "cross")):
            assert seen[f][t] > 0, f"no {t[0]} -> {t[1]} in family {f}"
        assert survived[f], f"buf_last never survives a cross call in family {f}"
    total = collections.Counter()
    for f in seen:
        total.update(seen[f])
    assert total[("cross", "cross")] > 300 and total[("one", "one")] > 1000


def test_resampler_inputs_reach_the_branches_of_the_host_side_assembly(runs):
    """Three things about resampleOne calls, from the closed forms (output k of a call that starts at filter offset fo reads from
    element ceil((k D - fo) / I); the SIMD loop walks the padded group length from there):

    * the empty-remainder branch of firResampler (`length bufIn == 0`, Filter.hs:700-703): a call that uses up its whole vector;
    * a call whose vector is much longer than it needs (count limited by the space left in the output block): its walk ends more
      than 100 elements before the vector's end -- concat() clamps to `need`, the rest must not be looked at;
    * how far the walk of the LAST output reaches.  Inside the reference's Pipe it never ends past the caller's vector:
      count <= (len I - numCoeffsR + fo) / D + 1 gives (count - 1) D - fo <= (len - numCoeffsR / I) I, so the last output starts
      at or before len - numCoeffsR / I, and numCoeffsR / I = roundUp(ceil(ntaps / I), simd) IS the padded group length.  What the
      Pipe does reach is the boundary itself: walks that end exactly on the vector's last element (one element less would be past
      it).  That is asserted here; the zero-filled walk past a short vector is a call only a direct caller can make, and
      tests/test_gpu_record_pipes.py makes it on the ABI."""
    import os
    from sdr_amd import build as B
    if not os.path.exists(B.LIB):
        B.build()
    import sdr_amd.lib as L            # descriptors and their closed forms need no device
    empty = exact = early = 0
    worst = None
    for (c, ob), (calls, _, _) in runs.items():
        if c.kind != "resampler":
            continue
        r = L.Resampler(c.I, c.D, RC.taps(c), RC.ORDERS[c.order], complex_=c.cplx)
        walk = RC.num_coeffs(c) // c.I                      # the padded group length
        first_of_group = {}
        for m in range(4 * c.I + 4):
            first_of_group.setdefault(r.group(m), m)
        for i, call in enumerate(calls):
            if call[0] != "one":
                continue
            _, count, n, (group, fo) = call
            m0 = first_of_group[group]
            assert r.filter_offset(m0) == fo, (RC.case_id(c), call)
            end = r.in_offset(m0 + count - 1) - r.in_offset(m0) + walk
            assert end == PM.quot_up((count - 1) * c.D - fo, c.I) + walk
            used = r.in_offset(m0 + count) - r.in_offset(m0)
            worst = end - n if worst is None else max(worst, end - n)
            exact += end == n
            early += n - end > 100
            empty += used == n and i + 1 < len(calls)
    assert empty >= 1, "no resampleOne call uses up its whole vector: the empty-remainder branch is never taken"
    assert early >= 1, "no resampleOne call leaves more than 100 elements of its vector unread"
    assert worst == 0 and exact >= 1, f"the longest SIMD walk ends {worst} elements past its vector (expected: exactly at its end)"
