"""sdrhip_nfm_bank_run's stream contract on a gated stream, the way tests/test_gpu_stream_order.py holds every other device operator
to it (tests/stream_order.py says what a gated run is).  One case is a CALL SEQUENCE on one stream: outputs [0, K1) from the state,
an EMPTY range (its copy of the state is work on the stream too), outputs [K1, K) from that copy -- so the fused launch, route 2's
two calls and the empty-range copy are each ordered by `stream` alone, and the state hand-over between them with it.  The expected
values are the CPU side's: the tuner model's rows through oracle.fm_demod."""
import numpy as np
import pytest

import signals as S
import stream_order as SO

pytestmark = pytest.mark.gpu

B = SO.B
NFM, NFM_CROSS, ROWS = "sdrhip_debug_nfm_bank_launches", "sdrhip_debug_nfm_bank_cross_launches", "sdrhip_debug_rows_launches"
K1 = 1009                                      # the cut: an odd output, the first Cross output of the stream
STATE = np.array([0.25, -0.75, -3.0, 0.0, 0.0, 7.5], np.float32)


class NfmBank(SO.Case):
    def __init__(self, fmt, route, seed):
        super().__init__(f"nfm bank x3 {fmt}, " + {1: "fused: one fmDemod-form launch a run", 2: "composed: tuner bank + fmDemod rows",
                                                   0: "auto"}[route] + ", two runs around an empty range")
        self.fmt, self.route, self.seed = fmt, route, seed
        if route == 1:
            self.counters = {NFM: ("==", 2), NFM_CROSS: ("==", 0), SO.BANK_LAUNCHES: ("==", 0), ROWS: ("==", 1)}     # rows: the empty range's copy
        elif route == 2:
            self.counters = {NFM: ("==", 0), SO.BANK_LAUNCHES: ("==", 2), ROWS: ("==", 3)}
        else:
            self.counters = {NFM_CROSS: ("==", 0)}

    def rows(self, oracle, x):
        return [SO.tuner_outputs(oracle, self, x, t, B) for t in SO.BANK_TABLES]

    def expected(self, oracle, x):
        iq = self.rows(oracle, x)
        out = [oracle.fm_demod(q, (float(STATE[2 * j]), float(STATE[2 * j + 1]))) for j, q in enumerate(iq)]
        return {"out": np.concatenate(out), "final": np.concatenate([q[-2:] for q in iq])}

    def make(self, hip):
        b = hip.NfmBank(hip.TunerBank(8, S.taps_decim127(), SO.BANK_TABLES))
        b.set_route(self.route)
        return b

    def states(self):
        return {"state": STATE}

    def scratch(self, hip, obj):
        K = (self.n - 128) // 8 + 1
        return {"ws": obj.workspace_bytes(K), "mid": 24, "mid2": 24}

    def call(self, hip, obj, stream, p_in, buf):
        K = buf["out"].numel() // len(SO.BANK_TABLES)
        run = {"cf32": obj.run, "u8": obj.run_u8, "i16": obj.run_i16}[self.fmt]
        out, ws, wsb = buf["out"].data_ptr(), buf["ws"].data_ptr(), buf["ws"].numel()
        run(p_in, 0, out, K, 0, K1, B, buf["state"].data_ptr(), buf["mid"].data_ptr(), ws, wsb, stream=stream)
        run(p_in, 0, out, K, K1, K1, B, buf["mid"].data_ptr(), buf["mid2"].data_ptr(), ws, wsb, stream=stream)
        run(p_in, 0, out + 4 * K1, K, K1, K, B, buf["mid2"].data_ptr(), buf["final"].data_ptr(), ws, wsb, stream=stream)


CASES = [NfmBank("u8", 1, 71), NfmBank("cf32", 1, 72), NfmBank("i16", 1, 73), NfmBank("u8", 2, 74), NfmBank("i16", 2, 75), NfmBank("cf32", 0, 76)]
BY_NAME = {c.name: c for c in CASES}


def _dev(a):
    import gpu_util as G
    return G.to_dev(a)


@pytest.fixture(scope="module")
def gate(hip, oracle):
    """As tests/test_gpu_stream_order.py: the sleep calibration, the control that picks the gated streams, and the delay sized by the
    host queueing time of the longest call sequence here (route 2: seven launches)."""
    g = SO.Gate(hip)
    g.pick_streams()
    case = CASES[3]
    obj = case.make(hip)
    SO.sync_run(g, hip, case, obj, oracle, _dev(case.stream(0)))
    q = SO.gated_run(g, hip, case, obj, oracle, prepared=SO.prepare(g, hip, case, obj, oracle))
    q.finish()
    g.set_delay(q.queue_ms)
    print("\n" + "\n".join(g.log))
    return g


def _compare(case, snaps, exp, what):
    for name, e in exp.items():
        case.check(snaps[name], e, f"{what}: {name}")


def _same_as(snaps, ref, what):
    for name, r in ref.items():
        assert SO.same_bits(snaps[name], r).all(), f"{what}: {name}: {int((~SO.same_bits(snaps[name], r)).sum())} of {r.size} floats differ"


def test_the_case_would_show_a_stray_launch(oracle):
    """On the CPU side: a run that read either poison stream, or started from another state, gives other outputs AND another final
    state, so a launch out of order cannot pass."""
    case = CASES[0]
    real = case.expected_real(oracle)
    for which in (1, 2):
        other = case.expected(oracle, case.stream(which))
        for name in ("out", "final"):
            assert (~SO.same_bits(real[name], other[name])).mean() > 0.9, f"poison {which} gives the real {name}"
    assert SO.straddlers((case.n - 128) // 8 + 1)[0] == K1


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_gated_run(hip, oracle, gate, case):
    exp = case.expected_real(oracle)
    obj = case.make(hip)
    ref = SO.sync_run(gate, hip, case, obj, oracle, _dev(case.stream(0)))              # the warm-up, and the route's counters
    _compare(case, ref, exp, f"{case.name}: synchronous run on the null stream")
    prepared = SO.prepare(gate, hip, case, obj, oracle)
    before = SO.counter_values(hip, case)
    q = SO.gated_run(gate, hip, case, obj, oracle, prepared=prepared)
    snaps = q.finish()
    SO.assert_counters(case, before, SO.counter_values(hip, case))
    print(f"{case.name}: queued in {q.queue_ms:.3f} ms behind a delay of {gate.delay_ms:.1f} ms; stream busy after the call: {q.busy}")
    assert q.busy, f"{case.name}: the stream was idle when the calls returned: a call synchronised the host with its stream " \
                   f"(or took longer than the delay: queued in {q.queue_ms:.3f} ms)"
    _compare(case, snaps, exp, f"{case.name}: gated run")
    _same_as(snaps, ref, f"{case.name}: gated run against the synchronous run")


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[CASES[0].name, CASES[3].name])
def test_first_ever_run_is_the_gated_one(hip, oracle, gate, case):
    """The tap and table uploads of a fresh bank against its first kernel on a non-blocking stream."""
    exp = case.expected_real(oracle)
    obj = case.make(hip)
    q = SO.gated_run(gate, hip, case, obj, oracle, prepared=SO.prepare(gate, hip, case, obj, oracle))
    _compare(case, q.finish(), exp, f"{case.name}: first run, gated")


@pytest.mark.parametrize("case", [CASES[0], CASES[3]], ids=[CASES[0].name, CASES[3].name])
def test_one_bank_on_two_gated_streams(hip, oracle, gate, case):
    """One bank, one host thread, two gated streams with their own inputs, outputs, states and workspaces: the run queued first has
    the longer delay, so the device executes them in the reverse of call order."""
    inputs = [case.stream(0), case.stream(11)]
    exps = [case.expected_real(oracle), case.expected(oracle, inputs[1])]
    obj = case.make(hip)
    SO.sync_run(gate, hip, case, obj, oracle, _dev(inputs[0]))
    prepared = [SO.prepare(gate, hip, case, obj, oracle, real=x) for x in inputs]
    gate.torch.cuda.synchronize()
    plan = [(gate.s1, gate.delay_ms), (gate.s2, gate.delay_ms / 4)]
    queued = [SO.gated_run(gate, hip, case, obj, oracle, stream=s, delay_ms=d, prepared=p) for (s, d), p in zip(plan, prepared)]
    snaps = [q.finish() for q in queued]
    gate.torch.cuda.synchronize()
    for i, (sn, e) in enumerate(zip(snaps, exps)):
        _compare(case, sn, e, f"{case.name}: run {i} on stream S{1 + i}")
