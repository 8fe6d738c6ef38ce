"""The general fused audio tail's stream contract on a gated stream, the way tests/test_gpu_audio_tail_stream_order.py holds the
existing routes to it (tests/stream_order.py says what a gated run is; its helpers are used unchanged).  One case is three rows of
one seeded y stream each on the 4/5 x 63 tail with block 256, cut into two runs at an odd output: route 0 with mode 1 (one launch
of k_audio_tail_rows_any a run) and with mode 2 (the composition's launch set through its workspace) are each ordered by `stream`
alone.  The expected values are the CPU side's: the restated Pipes' composition of tests/audio_tail_any_cases.py."""
import numpy as np
import pytest

import audio_tail_any_cases as AC
import stream_order as SO

pytestmark = pytest.mark.gpu

SHAPE = AC.SHAPES["4/5 x 63"]
BLOCK = 256
ROWS = 3
N_Y = 3700                                # per row; 256-sample blocks: a dozen seams of both stages lie inside
GENERAL, FUSED, FIR_ROWS = "sdrhip_debug_audio_tail_general_launches", "sdrhip_debug_audio_tail_launches", "sdrhip_debug_fir_rows_launches"
GAIN = -0.5


class Tail(SO.Case):
    fmt = "f32"
    n = ROWS * N_Y

    def __init__(self, mode, seed):
        super().__init__("general audio tail x3, " + {1: "mode 1: one launch a run", 2: "mode 2: resampler rows, filter rows, scale"}[mode]
                         + ", two runs")
        self.mode, self.seed = mode, seed
        self.counters = {1: {GENERAL: ("==", 2), FUSED: ("==", 0), FIR_ROWS: ("==", 0)},
                         2: {GENERAL: ("==", 0), FUSED: ("==", 0), FIR_ROWS: (">=", 4)}}[mode]

    def expected(self, oracle, x):
        rows = [AC.expected_from(oracle, SHAPE, np.ascontiguousarray(r), BLOCK, GAIN) for r in x.reshape(ROWS, N_Y)]
        return {"out": np.concatenate(rows)}

    def make(self, hip):
        t = hip.AudioTail(SHAPE.I, SHAPE.D, SHAPE.resamp_taps(), SHAPE.audio_half(), gain=GAIN, block=BLOCK)
        t.set_route(0)
        t.set_general(self.mode)
        return t

    def scratch(self, hip, obj):
        return {"ws": obj.workspace_bytes(ROWS, N_Y)}

    def call(self, hip, obj, stream, p_in, buf):
        Q = buf["out"].numel() // ROWS
        cut = 1461
        ws, wsb = buf["ws"].data_ptr(), buf["ws"].numel()
        out = buf["out"].data_ptr()
        kw = dict(y_base=0, n_y=N_Y, workspace=ws, workspace_bytes=wsb, stream=stream, y_stride=N_Y, audio_stride=Q, rows=ROWS)
        obj.run_rows(p_in, out, 0, cut, **kw)
        obj.run_rows(p_in, out + 4 * cut, cut, Q, **kw)


CASES = [Tail(1, 91), Tail(2, 92)]


def _dev(a):
    import gpu_util as G
    return G.to_dev(a)


@pytest.fixture(scope="module")
def gate(hip, oracle):
    g = SO.Gate(hip)
    g.pick_streams()
    case = CASES[1]
    obj = case.make(hip)
    SO.sync_run(g, hip, case, obj, oracle, _dev(case.stream(0)))
    q = SO.gated_run(g, hip, case, obj, oracle, prepared=SO.prepare(g, hip, case, obj, oracle))
    q.finish()
    g.set_delay(q.queue_ms)
    print("\n" + "\n".join(g.log))
    return g


def test_the_case_would_show_a_stray_launch(oracle):
    case = CASES[0]
    real = case.expected_real(oracle)["out"]
    Q = real.size // ROWS
    assert Q > 2 * AC.TILE and SHAPE.end_input(Q - 1) <= N_Y < SHAPE.end_input(Q)
    for which in (1, 2):
        other = case.expected(oracle, case.stream(which))["out"]
        assert (~SO.same_bits(real, other)).mean() > 0.9
    assert AC.resampler_cross(SHAPE, BLOCK, 0, Q + SHAPE.lf - 1).size and AC.filter_cross(SHAPE, BLOCK, 0, Q).size


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gated_run(hip, oracle, gate, case):
    exp = case.expected_real(oracle)
    obj = case.make(hip)
    ref = SO.sync_run(gate, hip, case, obj, oracle, _dev(case.stream(0)))
    case.check(ref["out"], exp["out"], f"{case.name}: synchronous run on the null stream")
    prepared = SO.prepare(gate, hip, case, obj, oracle)
    before = SO.counter_values(hip, case)
    q = SO.gated_run(gate, hip, case, obj, oracle, prepared=prepared)
    snaps = q.finish()
    SO.assert_counters(case, before, SO.counter_values(hip, case))
    print(f"{case.name}: queued in {q.queue_ms:.3f} ms behind a delay of {gate.delay_ms:.1f} ms; stream busy after the call: {q.busy}")
    assert q.busy, f"{case.name}: the stream was idle when the calls returned: a call synchronised the host with its stream " \
                   f"(or took longer than the delay: queued in {q.queue_ms:.3f} ms)"
    case.check(snaps["out"], exp["out"], f"{case.name}: gated run")
    assert SO.same_bits(snaps["out"], ref["out"]).all()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_first_ever_run_is_the_gated_one(hip, oracle, gate, case):
    """The tap uploads of a fresh tail against its first kernel on a non-blocking stream."""
    exp = case.expected_real(oracle)
    obj = case.make(hip)
    q = SO.gated_run(gate, hip, case, obj, oracle, prepared=SO.prepare(gate, hip, case, obj, oracle))
    case.check(q.finish()["out"], exp["out"], f"{case.name}: first run, gated")
