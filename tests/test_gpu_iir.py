"""dcBlocker and agc on the device over the table of tests/iir_cases.py: the cancellation stream, the value classes, the subnormal
fixed point, magnitudes over 2^60 .. 2^100 and the plan edges, against the oracle / tests/agc_model.py -- bit for bit where the
expected output is finite or infinite, NaN positions where it holds NaN -- with the statistics words checked against what the
scheme model (iir_cases.scheme) says each launch had to do: the route, the repair rounds, and the one-lane walk.

tests/test_iir_cases.py shows on the CPU that the table reaches what it is for; run_in values the block does not cover
(up to INT_MAX) are checked there through the plan hooks and never launched."""
import numpy as np
import pytest
import torch

import agc_model
import gpu_util
import iir_cases as IC
import value_classes as V
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

OFFSETS = [(0, 1), (1, 0), (2, 0), (0, 2)]          # floats by which input / output are shifted off their 256-byte aligned buffers


def _floats(x):
    return np.ascontiguousarray(x).view(np.float32)


def _launch(hip, case, x, state, use_ws=True, off_in=0, off_out=0):
    """One sdrhip_dc_blocker_run / sdrhip_agc_run over x (float32 or complex64) from `state`, run_in as the case says.
    Returns (output as float32, final state as float32, the four statistics words)."""
    dc = case.op == "dc"
    n, fl = x.size, _floats(x).copy()                # the table's streams are shared and read-only
    d_in = torch.zeros(fl.size + 8, dtype=torch.float32, device="cuda")[off_in: off_in + fl.size]
    d_in.copy_(torch.from_numpy(fl))
    whole = gpu_util.dev_empty_f32(fl.size + 8)
    d_out = whole[off_out: off_out + fl.size]
    fin = gpu_util.dev_empty_f32(2 if dc else 1)
    wsb = (hip.lib.sdrhip_dc_blocker_workspace_bytes if dc else hip.lib.sdrhip_agc_workspace_bytes)(n)
    ws = torch.full((wsb,), 0xA5, dtype=torch.uint8, device="cuda")          # the launch itself must write every word it reports
    p_in, p_out = (d_in.data_ptr(), d_out.data_ptr()) if n else (None, None)
    p_ws, b_ws = (ws.data_ptr(), wsb) if use_ws else (None, 0)
    if dc:
        hip.check(hip.lib.sdrhip_dc_blocker_run(None, p_in, p_out, n, state[0], state[1], fin.data_ptr(), p_ws, b_ws, case.run_in),
                  "sdrhip_dc_blocker_run")
    else:
        hip.check(hip.lib.sdrhip_agc_run(None, p_in, p_out, n, case.mu, case.reference, state[0], fin.data_ptr(), p_ws, b_ws, case.run_in),
                  "sdrhip_agc_run")
    torch.cuda.synchronize()
    w = gpu_util.to_host(whole).view(np.uint32)
    assert np.all(w[:off_out] == gpu_util.CANARY) and np.all(w[off_out + fl.size:] == gpu_util.CANARY), "wrote outside its output"
    return w[off_out: off_out + fl.size].view(np.float32).copy(), gpu_util.to_host(fin).copy(), hip.dc_stats(ws)


def _compare(case, got, exp, what):
    if case.bitwise:
        assert_bit_equal(got, _floats(exp), what)
    else:
        V.assert_same_classes(got, _floats(exp), what, max_nan_share=0.5)


def _same_state(got, exp, what):
    got, exp = np.asarray(got, np.float32).ravel(), np.asarray(exp, np.float32).ravel()
    assert got.shape == exp.shape and IC.same(got, exp).all(), f"{what}: final state {got!r}, expected {exp!r}"


@pytest.mark.parametrize("case", IC.CASES, ids=[c.name for c in IC.CASES])
def test_case(hip, oracle, case):
    plan = IC.plan_of(hip, case)
    s = IC.scheme(case, plan, oracle)
    x, n = IC.stream(case), case.n
    print(f"{case.name}: {case.reach}\n    model: {s.describe()}")
    got, fin, stats = _launch(hip, case, x, case.state)
    print(f"    device statistics {stats}")
    _compare(case, got, s.out, case.name)
    _same_state(fin, s.final, case.name)

    # the statistics: the route, then what the rounds and the walk had to do
    assert stats[3] == plan[0] == s.chunks, (stats, plan)
    if s.n_wrong == 0 and not s.nan_starts:
        assert stats[:3] == (0, 0, 0), stats
    if s.n_wrong > 0:
        assert stats[2] > 0, "a chunk starts wrong: the repair rounds had work"
    if s.never_merging_run(8):
        assert stats[0] > 0 and stats[1] > 0, f"no three rounds can spare the walk here, yet the statistics are {stats}"
    if case.op == "dc" and any(end == n for _, end in s.walks):
        first = min(a for a, end in s.walks if end == n)
        assert stats[1] >= n - first, f"the walk runs from sample {first} to the end, {n - first} samples; it reports {stats[1]}"
    if not s.nan_starts:
        # no NaN meets a NaN at a chunk start, so the model's bit comparisons are the device's: the counts are exact
        assert stats[:3] == (s.left, s.rewritten, s.repaired), (stats, (s.left, s.rewritten, s.repaired))

    # input and output aligned differently: the access width has to follow the worse of the two
    for off_in, off_out in OFFSETS:
        g, f, st = _launch(hip, case, x, case.state, off_in=off_in, off_out=off_out)
        _compare(case, g, s.out, f"{case.name}, input + {off_in}, output + {off_out} floats")
        _same_state(f, s.final, case.name)
        assert st[3] == s.chunks
    # a null workspace: the sequential walk
    g, f, _ = _launch(hip, case, x, case.state, use_ws=False)
    _compare(case, g, s.out, f"{case.name}, null workspace")
    _same_state(f, s.final, case.name)

    # two calls chained through d_final, with an n == 0 call between them that must hand the state on unchanged
    k = n // 2 + 1
    g1, f1, _ = _launch(hip, case, x[:k], case.state)
    g0, f0, st0 = _launch(hip, case, x[:0], tuple(float(v) for v in f1))
    assert g0.size == 0
    assert_bit_equal(f0, f1, f"{case.name}: an n == 0 call hands the state on")
    g2, f2, _ = _launch(hip, case, x[k:], tuple(float(v) for v in f0))
    _compare(case, np.concatenate([g1, g2]), s.out, f"{case.name}, cut at {k}")
    _same_state(f2, s.final, f"{case.name}, cut at {k}")


def test_n_zero_hands_on_every_kind_of_state(hip):
    """sdrhip_dc_blocker_run with n == 0 writes {last_sample, last_output} to d_final: null pointers, with and without a workspace."""
    case = IC.BY_NAME["dc/n=2W"]
    for state in ((0.25, -0.5), (-0.0, 0.0), (np.inf, -np.inf), (1e-45, -3.4e38)):
        for use_ws in (True, False):
            _, fin, stats = _launch(hip, case, np.zeros(0, np.float32), state, use_ws=use_ws)
            assert_bit_equal(fin, np.array(state, np.float32), f"dcBlocker n == 0 from {state}")


# ---- the Pipes ----------------------------------------------------------------------------------------------------------------------
def _cuts(n, W):
    """Blocks of 2 W - 1 and 2 W samples (either side of the route change), ragged ones around them, the rest."""
    cuts = [0, 2 * W - 1, 4 * W - 1, 4 * W + 6, 4 * W + 7]
    assert cuts[-1] < n
    return cuts + [n]


def _pipe_run(pipe, blocks):
    outs = []
    for b in blocks:
        outs += pipe.push(b)
    outs += pipe.flush()
    assert [o.size for o in outs] == [b.size for b in blocks]
    return np.concatenate(outs)


@pytest.mark.parametrize("name", ["cancellation", "fixed_point"])
def test_dc_blocking_filter_pipe(hip, oracle, name):
    x = IC._stream(IC.CANCEL if name == "cancellation" else IC.FIXED)
    W = hip.dc_plan(x.size)[2]
    cuts = _cuts(x.size, W)
    assert hip.dc_plan(2 * W - 1)[0] == 0 and hip.dc_plan(2 * W)[0] > 0
    exp, efs, efo = oracle.dc_blocker(x, 0.0, 0.0)                   # the Pipe starts from (0, 0), Filter.hs:730-739
    case = IC.Case("dc/pipe-" + name, "dc", (), x.size, 0, "", state=(0.0, 0.0))
    one, fin, stats = _launch(hip, case, x, case.state)
    assert stats[3] > 0
    assert_bit_equal(one, exp, f"{name}: one call")
    got = _pipe_run(hip.dcBlockingFilter(), [x[a:b] for a, b in zip(cuts[:-1], cuts[1:])])
    assert_bit_equal(got, one, f"dcBlockingFilter over the {name} stream, blocks {np.diff(cuts).tolist()}")


@pytest.mark.parametrize("name", ["noise", "range"])
def test_agc_pipe(hip, name):
    """agcPipe starts from state 1 (Util.hs:348).  At mu = 2^-101 the default run-in is the largest there is (2^22 samples): no block
    a test can afford reaches two of them, so the range stream goes through ragged blocks on the sequential walk only."""
    if name == "noise":
        mu, ref, x = 0.4, 1.0, IC._stream(IC.NOISE)
        W = hip.agc_plan(x.size, mu)[2]
        assert hip.agc_plan(2 * W - 1, mu)[0] == 0 and hip.agc_plan(2 * W, mu)[0] > 0
        cuts = _cuts(x.size, W)
    else:
        mu, ref, x = IC.RANGE_MU, IC.RANGE_REF, IC.stream(IC.BY_NAME["agc/range-w64"])
        assert hip.agc_plan(x.size, mu)[0] == 0
        cuts = [0, 1, 8, 263, 4096, 4099, x.size]
    exp, _ = agc_model.agc(x, mu, ref, 1.0)
    case = IC.Case("agc/pipe-" + name, "agc", (), x.size, 0, "", state=(1.0,), mu=mu, reference=ref)
    one, fin, stats = _launch(hip, case, x, case.state)
    assert_bit_equal(one, _floats(exp), f"{name}: one call")
    got = _pipe_run(hip.agcPipe(mu, ref), [agc_model.interleaved(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])
    assert_bit_equal(got, one, f"agcPipe over the {name} stream, blocks {np.diff(cuts).tolist()}")
