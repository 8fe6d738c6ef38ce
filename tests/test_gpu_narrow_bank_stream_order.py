"""sdrhip_narrow_bank_run's stream contract on a gated stream, the way tests/test_gpu_nfm_bank_stream_order.py holds the narrow-band FM
bank to it (tests/stream_order.py says what a gated run is).  One case is a CALL SEQUENCE on one stream: stage-2 outputs [0, K1) from
the state, an EMPTY range (the fmDemod form's copy of the state is work on the stream too), outputs [K1, N) from that copy or from the
dc state the first run left -- so the tuner bank's launches, the fused launch, route 2's calls, dcBlocker's launch set and the
empty-range copy are each ordered by `stream` alone, and the state hand-over between them with it.  The expected values are the CPU
side's: the tuner model's rows through tests/narrow_bank_cases.py."""
import numpy as np
import pytest

import narrow_bank_cases as NB
import signals as S
import stream_order as SO

pytestmark = pytest.mark.gpu

B = SO.B
SHAPE, SEAM2 = "24/4", 1024
NARROW, FIR_ROWS, AM_DEMOD = "sdrhip_debug_narrow_bank_launches", "sdrhip_debug_fir_rows_launches", "sdrhip_debug_am_demod_launches"
K1 = 251                                       # the cut: an odd output, the first Cross output of stage 2
FM_STATE = np.array([0.25, -0.75, -3.0, 0.0, 0.0, 7.5], np.float32)
DC_STATE = np.array([0.5, -0.25, 0.0, 1.0, -2.0, 0.125], np.float32)


class NarrowBank(SO.Case):
    def __init__(self, form, fmt, route, seed):
        dc = form == NB.ENV
        super().__init__(f"narrow bank x3 {'envelope + dcBlocker' if dc else 'fmDemod'} {fmt}, " +
                         {1: "fused: tuner bank + one narrow launch a run", 2: "composed", 0: "auto"}[route] + ", two runs around an empty range")
        self.form, self.dc, self.fmt, self.route, self.seed = form, dc, fmt, route, seed
        if route == 1:
            self.counters = {NARROW: ("==", 2), FIR_ROWS: ("==", 0), AM_DEMOD: ("==", 0), SO.BANK_LAUNCHES: ("==", 2)}
        elif route == 2:
            self.counters = {NARROW: ("==", 0), SO.BANK_LAUNCHES: ("==", 2), AM_DEMOD: ("==", 2 if dc else 0)}
        else:
            self.counters = {SO.BANK_LAUNCHES: ("==", 2)}

    def expected(self, oracle, x):
        out, fin = [], []
        for j, t in enumerate(SO.BANK_TABLES):
            iq2 = NB.decimate2(oracle, SHAPE, SO.tuner_outputs(oracle, self, x, t, B), SEAM2)
            if self.dc:
                env = NB.demodulate(oracle, iq2, NB.ENV, False)
                y = NB.demodulate(oracle, iq2, NB.ENV, True, dc_state=DC_STATE[2 * j:2 * j + 2])
                fin.append(np.array([env[-1], y[-1]], np.float32))
            else:
                y = NB.demodulate(oracle, iq2, NB.FM, False, fm_state=FM_STATE[2 * j:2 * j + 2])
                fin.append(iq2[-2:])
            out.append(y)
        return {"out": np.concatenate(out), "dc" if self.dc else "final": np.concatenate(fin)}

    def make(self, hip):
        taps, d2, _ = NB.SHAPES[SHAPE]
        b = hip.NarrowBank(hip.TunerBank(8, S.taps_decim127(), SO.BANK_TABLES), hip.Decimator(d2, taps, complex_=True), self.form, self.dc)
        b.set_route(self.route)
        return b

    def states(self):
        return {"dc": DC_STATE} if self.dc else {"state": FM_STATE}

    def scratch(self, hip, obj):
        N = NB.n_out(SHAPE, (self.n - 128) // 8 + 1)
        return {"ws": obj.workspace_bytes(N), "mid": 24, "mid2": 24}

    def call(self, hip, obj, stream, p_in, buf):
        N = buf["out"].numel() // len(SO.BANK_TABLES)
        run = {"cf32": obj.run, "u8": obj.run_u8, "i16": obj.run_i16}[self.fmt]
        out, ws, wsb = buf["out"].data_ptr(), buf["ws"].data_ptr(), buf["ws"].numel()
        if self.dc:
            dc = buf["dc"].data_ptr()
            run(p_in, 0, out, N, 0, K1, B, SEAM2, None, None, dc, ws, wsb, stream=stream)
            run(p_in, 0, out, N, K1, K1, B, SEAM2, None, None, dc, ws, wsb, stream=stream)
            run(p_in, 0, out + 4 * K1, N, K1, N, B, SEAM2, None, None, dc, ws, wsb, stream=stream)
        else:
            run(p_in, 0, out, N, 0, K1, B, SEAM2, buf["state"].data_ptr(), buf["mid"].data_ptr(), None, ws, wsb, stream=stream)
            run(p_in, 0, out, N, K1, K1, B, SEAM2, buf["mid"].data_ptr(), buf["mid2"].data_ptr(), None, ws, wsb, stream=stream)
            run(p_in, 0, out + 4 * K1, N, K1, N, B, SEAM2, buf["mid2"].data_ptr(), buf["final"].data_ptr(), None, ws, wsb, stream=stream)


CASES = [NarrowBank(NB.FM, "u8", 1, 81), NarrowBank(NB.ENV, "cf32", 1, 82), NarrowBank(NB.FM, "i16", 1, 83), NarrowBank(NB.FM, "u8", 2, 84),
         NarrowBank(NB.ENV, "i16", 2, 85), NarrowBank(NB.FM, "cf32", 0, 86)]


def _dev(a):
    import gpu_util as G
    return G.to_dev(a)


@pytest.fixture(scope="module")
def gate(hip, oracle):
    """As tests/test_gpu_stream_order.py: the sleep calibration, the control that picks the gated streams, and the delay sized by the
    host queueing time of the longest call sequence here (route 2 with dcBlocker)."""
    g = SO.Gate(hip)
    g.pick_streams()
    case = CASES[4]
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
    """On the CPU side: a run that read either poison stream gives other outputs AND another final state, so a launch out of order
    cannot pass; and the cut is a Cross output of stage 2."""
    for case in (CASES[0], CASES[1]):
        real = case.expected_real(oracle)
        for which in (1, 2):
            other = case.expected(oracle, case.stream(which))
            for name in real:
                assert (~SO.same_bits(real[name], other[name])).mean() > 0.9, f"poison {which} gives the real {name}"
    assert NB.cross2(SHAPE, SEAM2)[0] == K1


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


@pytest.mark.parametrize("case", [CASES[0], CASES[1], CASES[3]], ids=[CASES[0].name, CASES[1].name, CASES[3].name])
def test_first_ever_run_is_the_gated_one(hip, oracle, gate, case):
    """The tap and table uploads of a fresh bank and a fresh second decimator against their first kernels on a non-blocking stream."""
    exp = case.expected_real(oracle)
    obj = case.make(hip)
    q = SO.gated_run(gate, hip, case, obj, oracle, prepared=SO.prepare(gate, hip, case, obj, oracle))
    _compare(case, q.finish(), exp, f"{case.name}: first run, gated")
