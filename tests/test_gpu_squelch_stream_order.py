"""The squelch's stream contract on a gated stream (tests/stream_order.py says what a gated run is; its helpers are used unchanged): the
one-row call and the rows call on each route are ordered by `stream` alone and make no host synchronisation.  The rows cases are two
consecutive pushes of 3 rows whose state passes through device memory with d_final == d_state, both queued behind one gate.  The
input buffer is the signal AND the detector (self-detection), so the poison streams the helpers put into it before and after the
call would change the gates as well as the samples.  The expected values are tests/squelch_model.py's, never a device run.

The states are int32 pairs; the helpers carry them as the float32 words of the same bits."""
import numpy as np
import pytest

import squelch_model as SM
import stream_order as SO

pytestmark = pytest.mark.gpu
LAUNCHES = "sdrhip_debug_squelch_launches"
WG, LS = 1, 2
ROUTE_NAMES = {WG: "WG", LS: "LS"}
BLOCK, HANG = 64, 1
# uniform(-1, 1) noise has a mean square of 1 / 3: blocks of 64 scatter around it, so levels fall on either side of both thresholds
POL = dict(open_level=0.36, close_level=0.31, open_above=1)


class One(SO.Case):
    """sdrhip_squelch_run, self-detecting, state by value"""
    fmt, STATE = "f32", (1, 1)

    def __init__(self, n_blocks, route, seed):
        super().__init__(f"squelch, one row of {n_blocks} blocks, {ROUTE_NAMES[route]}")
        self.nb, self.n, self.route, self.seed = n_blocks, n_blocks * BLOCK, route, seed
        self.counters = {LAUNCHES: ("==", 3 if route == LS else 1)}

    def expected(self, oracle, x):
        out, fin, lv, _ = SM.squelch(x[None], False, BLOCK, x[None], BLOCK, hang=HANG, states=np.array([self.STATE], np.int32), **POL)
        return {"out": out[0].copy(), "final": fin.reshape(-1).view(np.float32).copy(), "levels": lv[0].copy()}

    def scratch(self, hip, obj):
        return {"ws": hip.lib.sdrhip_squelch_rows_workspace_bytes(1, self.nb)}

    def call(self, hip, obj, stream, p_in, buf):
        hip.set_squelch_route(self.route)
        try:
            hip.check(hip.lib.sdrhip_squelch_run(stream, p_in, 0, BLOCK, p_in, buf["out"].data_ptr(), BLOCK, self.nb, POL["open_level"],
                                                 POL["close_level"], HANG, 1, self.STATE[0], self.STATE[1], buf["final"].data_ptr(),
                                                 buf["levels"].data_ptr(), None, buf["ws"].data_ptr(), buf["ws"].numel()), self.name)
        finally:
            hip.set_squelch_route(0)


class Rows(SO.Case):
    """sdrhip_squelch_run_rows, 3 rows, two pushes of HALF blocks, d_final == d_state"""
    fmt, ROWS, HALF = "f32", 3, 75

    def __init__(self, route, seed):
        super().__init__(f"squelch rows x3, two pushes, {ROUTE_NAMES[route]}, d_final == d_state")
        self.route, self.seed = route, seed
        self.n = self.ROWS * 2 * self.HALF * BLOCK
        self.counters = {LAUNCHES: ("==", 6 if route == LS else 2)}

    def states(self):
        return {"state": np.array([[0, 0], [1, 1], [0, 1]], np.int32).reshape(-1).view(np.float32)}

    def expected(self, oracle, x):
        rows = x.reshape(self.ROWS, -1)
        out, fin, _, _ = SM.squelch(rows, False, BLOCK, rows, BLOCK, hang=HANG, states=self.states()["state"].view(np.int32).reshape(-1, 2), **POL)
        return {"out": out.ravel().copy(), "state": fin.reshape(-1).view(np.float32).copy()}

    def scratch(self, hip, obj):
        return {"ws": hip.lib.sdrhip_squelch_rows_workspace_bytes(self.ROWS, self.HALF)}

    def call(self, hip, obj, stream, p_in, buf):
        stride, st = 2 * self.HALF * BLOCK, buf["state"].data_ptr()
        hip.set_squelch_route(self.route)
        try:
            for push in range(2):
                off = 4 * push * self.HALF * BLOCK
                hip.check(hip.lib.sdrhip_squelch_run_rows(stream, p_in + off, stride, 0, BLOCK, p_in + off, stride, buf["out"].data_ptr() + off, stride,
                                                          BLOCK, self.ROWS, self.HALF, POL["open_level"], POL["close_level"], HANG, 1, st, st, None,
                                                          None, buf["ws"].data_ptr(), buf["ws"].numel()), self.name)
        finally:
            hip.set_squelch_route(0)


CASES = [One(300, WG, 91), One(300, LS, 92), Rows(WG, 93), Rows(LS, 94)]


def _dev(a):
    import gpu_util as G
    return G.to_dev(a)


@pytest.fixture(scope="module")
def gate(hip, oracle):
    g = SO.Gate(hip)
    g.pick_streams()
    case = CASES[-1]                       # the most launches behind one gate
    SO.sync_run(g, hip, case, None, oracle, _dev(case.stream(0)))
    q = SO.gated_run(g, hip, case, None, oracle, prepared=SO.prepare(g, hip, case, None, oracle))
    q.finish()
    g.set_delay(q.queue_ms)
    print("\n" + "\n".join(g.log))
    return g


def test_the_cases_would_show_a_stray_launch(oracle):
    for case in CASES:
        real = case.expected_real(oracle)["out"]
        assert 0.2 < (real == 0).mean() < 0.8, f"{case.name}: the gate is {(real != 0).mean():.2f} open: it should open and shut"
        for which in (1, 2):
            other = case.expected(oracle, case.stream(which))["out"]
            assert (~SO.same_bits(real, other)).mean() > 0.5, case.name


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gated_run(hip, oracle, gate, case):
    exp = case.expected_real(oracle)
    ref = SO.sync_run(gate, hip, case, None, oracle, _dev(case.stream(0)))
    for k, e in exp.items():
        case.check(ref[k], e, f"{case.name}: synchronous run on the null stream: {k}")
    prepared = SO.prepare(gate, hip, case, None, oracle)
    before = SO.counter_values(hip, case)
    q = SO.gated_run(gate, hip, case, None, oracle, prepared=prepared)
    snaps = q.finish()
    SO.assert_counters(case, before, SO.counter_values(hip, case))
    print(f"{case.name}: queued in {q.queue_ms:.3f} ms behind a delay of {gate.delay_ms:.1f} ms; stream busy after the call: {q.busy}")
    assert q.busy, f"{case.name}: the stream was idle when the calls returned: a call synchronised the host with its stream " \
                   f"(or took longer than the delay: queued in {q.queue_ms:.3f} ms)"
    for k, e in exp.items():
        case.check(snaps[k], e, f"{case.name}: gated run: {k}")
        assert SO.same_bits(snaps[k], ref[k]).all()
