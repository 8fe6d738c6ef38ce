"""De-emphasis' stream contract on a gated stream (tests/stream_order.py says what a gated run is; its helpers are used unchanged): the
one-row call and the rows call on each route are ordered by `stream` alone and make no host synchronisation.  The rows cases are two
consecutive pushes of 3 rows whose state passes through device memory with d_final == d_state, both queued behind one gate.  The Pipe
runs on streams of its own: it is driven while the gate is still closed on the gated stream, finishes without waiting for that
stream, and gives the model's blocks.  The expected values are tests/deemph_model.py's, never a device run."""
import numpy as np
import pytest

import deemph_cases as DC
import deemph_model as DM
import stream_order as SO

pytestmark = pytest.mark.gpu
LAUNCHES = "sdrhip_debug_deemph_launches"
ALPHA = DC.A48
SEQ, WG, LS = 1, 2, 3
ROUTE_NAMES = {SEQ: "SEQ", WG: "WG", LS: "LS"}


class One(SO.Case):
    """sdrhip_deemph_run, state by value: n = 24581 samples take the WG route; with a workspace past the bound, LS."""
    fmt, STATE = "f32", 0.375

    def __init__(self, n, route, seed):
        super().__init__(f"de-emphasis, one row of {n}, {ROUTE_NAMES[route]}")
        self.n, self.route, self.seed = n, route, seed
        self.counters = {LAUNCHES: ("==", 5 if route == LS else 1)}

    def expected(self, oracle, x):
        out, fin = DM.deemph(x, ALPHA, self.STATE)
        return {"out": out, "final": np.array([fin], np.float32)}

    def scratch(self, hip, obj):
        return {"ws": hip.lib.sdrhip_deemph_workspace_bytes(self.n)}

    def call(self, hip, obj, stream, p_in, buf):
        assert hip.deemph_plan(1, self.n, float(ALPHA))[1] == self.route
        hip.check(hip.lib.sdrhip_deemph_run(stream, p_in, buf["out"].data_ptr(), self.n, float(ALPHA), self.STATE, buf["final"].data_ptr(),
                                            buf["ws"].data_ptr(), buf["ws"].numel(), 0), self.name)


class Rows(SO.Case):
    """sdrhip_deemph_run_rows, 3 rows, two pushes, d_final == d_state; the route forced (SEQ, LS) or the plan's own (WG)."""
    fmt, ROWS, HALF = "f32", 3, 8192 + 3

    def __init__(self, route, seed):
        super().__init__(f"de-emphasis rows x3, two pushes, {ROUTE_NAMES[route]}, d_final == d_state")
        self.route, self.seed = route, seed
        self.n = self.ROWS * 2 * self.HALF
        self.counters = {LAUNCHES: ("==", 10 if route == LS else 2)}

    def states(self):
        return {"state": np.array([0.25, -0.5, 1.5], np.float32)}

    def expected(self, oracle, x):
        out, fin = DM.deemph(x.reshape(self.ROWS, -1), ALPHA, self.states()["state"])
        return {"out": out.ravel().copy(), "state": np.asarray(fin, np.float32).copy()}

    def scratch(self, hip, obj):
        return {"ws": hip.lib.sdrhip_deemph_rows_workspace_bytes(self.ROWS, self.HALF)}

    def call(self, hip, obj, stream, p_in, buf):
        stride, st = 2 * self.HALF, buf["state"].data_ptr()
        hip.set_deemph_route(self.route)
        try:
            for push in range(2):
                off = 4 * push * self.HALF
                hip.check(hip.lib.sdrhip_deemph_run_rows(stream, p_in + off, stride, buf["out"].data_ptr() + off, stride, self.ROWS, self.HALF,
                                                         float(ALPHA), st, st, buf["ws"].data_ptr(), buf["ws"].numel(), 0), self.name)
        finally:
            hip.set_deemph_route(0)


CASES = [One(3 * 8192 + 5, WG, 81), One(DC.WG_MAX + 5, LS, 82), Rows(SEQ, 83), Rows(WG, 84), Rows(LS, 85)]


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
        for which in (1, 2):
            other = case.expected(oracle, case.stream(which))["out"]
            assert (~SO.same_bits(real, other)).mean() > 0.9, case.name


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


def test_the_pipe_runs_beside_a_closed_gate(hip, gate):
    """The Pipe's submissions are ordered by its own streams: pushed and flushed while the gated stream still spins in its delay, it
    neither waits for that stream nor needs it, and its blocks are the model's."""
    torch = gate.torch
    sizes = [70001, 8192, 100, 8192, 7]    # the largest first: no buffer of the pipe grows (and frees, which waits for the device) later
    x = SO.seeded("f32", sum(sizes), 8600)
    want, _ = DM.deemph(x, ALPHA, 0.0)
    cut = np.cumsum([0] + sizes)
    pipe = hip.Pipe.deemph(float(ALPHA))
    pipe.set_adaptive(0)                   # every push on its own: the same submissions on every run
    warm = hip.Pipe.deemph(float(ALPHA))
    warm.push(x[:70001])
    warm.flush()
    torch.cuda.synchronize()
    with torch.cuda.stream(gate.s1):
        gate.sleep(gate.delay_ms)
    got = []
    for a, b in zip(cut[:-1], cut[1:]):
        got += pipe.push(x[a:b])
    got += pipe.flush()
    busy = not gate.s1.query()
    gate.s1.synchronize()
    assert busy, "the Pipe waited for a stream that is not its own (or took longer than the delay)"
    assert [g.size for g in got] == sizes
    assert SO.same_bits(np.concatenate(got), want).all()
