"""GPU: the stage operators of the device stream API on stream SLICES -- in_base != 0, only the guaranteed inputs resident, and
positions beyond 2^33 and 2^40 -- against the restated Pipes (oracle/pipes_model.py) on the stream that starts at 0.

The translation rule that makes the near stream's answer the far launch's expected value is stated in
tests/stream_slice_cases.py and checked on the CPU by tests/test_stream_slice_cases.py.  Every comparison is assert_bit_equal
with the model; no expected value comes from the device."""
import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from oracle import pipes_model as PM
import signals as S
import stream_slice_cases as SC
from gpu_util import dev_empty_f32, ptr, to_host

pytestmark = pytest.mark.gpu

B = 8192


# ---- every branch of fir_run / resamp_run_demod, at every (S, delta) ------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_stage_on_slices(hip, oracle, case):
    """Nine runs per case: S in {0, > 2^33, > 2^40} x three first inputs (stream_slice_cases.positions), each cut into three
    launches.  The route launch's counters are asserted where the slice is 16-byte aligned (a misaligned first window is what the
    aligned-load kernels hand to their fallbacks, by design)."""
    raw, exp, trace, Lp = SC.near(case, oracle)
    w = case.width
    K = exp.size // w
    desc = case.make(hip)
    assert desc.num_coeffs == Lp
    with SC.route_knobs(hip, case):
        for s, pos, q in SC.combos(case, K):
            got, delta = SC.run_case(hip, case, desc, raw, Lp, s, pos, q)
            what = f"{case.name}: S = {s}, {pos.label}, outputs [{pos.a}, {pos.b})"
            if pos.mis == 0:
                for name in case.moves:
                    assert delta[name] > 0, f"{what}: the route launch did not move `{name}` ({delta})"
                for name in case.still:
                    assert delta[name] == 0, f"{what}: the route launch moved `{name}` ({delta})"
            assert_bit_equal(got, exp[w * pos.a:w * pos.b], what)


# ---- fmDemod on a slice ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def demod_stream(oracle):
    x = oracle.convert_u8(S.iq_u8_fm(3 * B))
    exp = np.concatenate(PM.fm_demod_pipe(oracle, [x[2 * i * B:2 * (i + 1) * B] for i in range(3)]))
    x.setflags(write=False)
    exp.setflags(write=False)
    return x, exp


@pytest.mark.parametrize("s", [0, (1 << 33) + 12345, (1 << 40) + 7])
@pytest.mark.parametrize("k0,k1", [(B, 3 * B), (1001, 2 * B + 77)])
def test_fm_demod_on_a_slice(hip, demod_stream, s, k0, k1):
    """k_begin == in_base: the sample before the slice is (last_re, last_im), and what lies in front of d_in is a NaN guard.
    k_begin > in_base: it is d_in[k_begin - 1 - in_base].  Both cut into two launches, near and far; fmDemod has no position of
    its own, so any S translates."""
    x, exp = demod_stream
    cut = k0 + 4097
    # the previous sample as an argument
    keep, d_in = SC.upload_slice(x, 2, k0, k1, False)
    out = dev_empty_f32(k1 - k0)
    last = x[2 * k0 - 2:2 * k0]
    hip.check(hip.lib.sdrhip_fm_demod_run(None, d_in, k0 + s, ptr(out), k0 + s, cut + s, float(last[0]), float(last[1])))
    hip.check(hip.lib.sdrhip_fm_demod_run(None, d_in, k0 + s, ptr(out) + 4 * (cut - k0), cut + s, k1 + s, float("nan"), float("nan")))
    assert_bit_equal(to_host(out), exp[k0:k1], f"fmDemod [{k0}, {k1}) at S = {s}, previous sample passed in")
    # the previous sample from the buffer, five samples into it
    keep, d_in = SC.upload_slice(x, 2, k0 - 5, k1, False, mis=1)
    out = dev_empty_f32(k1 - k0)
    hip.check(hip.lib.sdrhip_fm_demod_run(None, d_in, k0 - 5 + s, ptr(out), k0 + s, cut + s, float("nan"), float("nan")))
    hip.check(hip.lib.sdrhip_fm_demod_run(None, d_in, k0 - 5 + s, ptr(out) + 4 * (cut - k0), cut + s, k1 + s, float("nan"), float("nan")))
    assert_bit_equal(to_host(out), exp[k0:k1], f"fmDemod [{k0}, {k1}) at S = {s}, previous sample in the buffer")
    del keep


# ---- the untuned FM chain far into a stream ----------------------------------------------------------------------------------
CHAIN_S = 5 << 31            # S / 8 and 3 S / 80 are multiples of 8192: every stage of the chain keeps its seams, groups and blocks
CHAIN_MODEL_BLOCKS = 300     # the restated Pipes yield whole 8192-blocks only: ten audio blocks, enough for the systolic route's run


@pytest.fixture(scope="module")
def chain_stream(oracle):
    u8 = S.iq_u8(CHAIN_MODEL_BLOCKS * B)
    blocks = [u8[2 * i * B:2 * (i + 1) * B] for i in range(CHAIN_MODEL_BLOCKS)]
    exp = np.concatenate(PM.fm_receiver(oracle, blocks, S.taps_decim127(), 8, S.taps_resamp191(), 3, 10, S.taps_audio_half64(), 0.2, B))
    u8.setflags(write=False)
    exp.setflags(write=False)
    return u8, exp


def _timed_run(chain, *args):
    chain.enable_timing(True)
    try:
        chain.run(*args)
        torch.cuda.synchronize()
        stage_ms, runs = chain.read_timing()
    finally:
        chain.enable_timing(False)
    assert runs == 1
    return stage_ms


# route -> (source blocks resident, how the route is set, as tests/test_gpu_chain.py and tests/test_gpu_bench_size.py set it)
CHAIN_ROUTES = {
    "one-kernel chain": 6,
    "fused tail": 6,
    "stage kernels, tile decimator": 6,
    "stage kernels, systolic decimator": 240,      # test_gpu_systolic's seamed shape: past the 5 * 32768 outputs that stay on the tile kernel
}


@pytest.mark.parametrize("route", list(CHAIN_ROUTES))
def test_untuned_chain_far_into_a_stream(hip, chain_stream, route):
    """s0 = S + 8 * 12345 for S = 5 * 2^31 and 256 times that: the plan is the near plan shifted by 3 S / 80, and the audio is,
    bit for bit, the restated receiver Pipes' on the near stream over the same audio range."""
    u8, exp = chain_stream
    n_in = CHAIN_ROUTES[route] * B
    near_s0 = 8 * 12345
    chain = hip.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, B, hip.ORDER_AVX)
    q0n, q1n, halo_n = chain.plan(near_s0, near_s0 + n_in, near_s0 + n_in)
    assert halo_n == 0 and 0 < q0n < q1n <= exp.size
    keep, d_in = SC.upload_slice(u8, 2, near_s0, near_s0 + n_in, True)
    ws_bytes = chain.workspace_bytes(n_in)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    chain.set_small_chain(1 if route == "one-kernel chain" else 0)
    chain.set_fused_tail(1 if route == "fused tail" else 0)
    hip.lib.sdrhip_debug_set_systolic(1 if "systolic" in route else 0)
    try:
        for s in (0, CHAIN_S, CHAIN_S * 256):
            s0 = s + near_s0
            shift = 3 * s // 80
            assert shift * 80 == 3 * s
            q0, q1, halo = chain.plan(s0, s0 + n_in, s0 + n_in)
            assert (q0, q1, halo) == (q0n + shift, q1n + shift, 0), f"the plan at s0 = {s0} is not the near plan shifted by {shift}"
            out = dev_empty_f32(q1 - q0)
            small0, sys0 = hip.lib.sdrhip_debug_small_chain_launches(), hip.lib.sdrhip_debug_systolic_launches()
            stage_ms = _timed_run(chain, d_in, s0, n_in, ptr(out), q0, q1, ptr(ws), ws_bytes)
            small, systolic = hip.lib.sdrhip_debug_small_chain_launches() - small0, hip.lib.sdrhip_debug_systolic_launches() - sys0
            took = f"{route} at s0 = {s0}: one-kernel launches {small}, systolic launches {systolic}, stage ms {stage_ms}"
            if route == "one-kernel chain":
                assert small == 1 and systolic == 0, took
            elif route == "fused tail":
                assert small == 0 and systolic == 0 and stage_ms["fused_tail"] > 0.0 and stage_ms["filter"] == 0.0, took
            elif route == "stage kernels, tile decimator":
                assert small == 0 and systolic == 0 and stage_ms["fused_tail"] == 0.0 and stage_ms["filter"] > 0.0, took
            else:
                assert small == 0 and systolic == 1 and stage_ms["fused_tail"] == 0.0 and stage_ms["filter"] > 0.0, took
            assert_bit_equal(to_host(out), exp[q0n:q1n], f"{route}: audio [{q0}, {q1}) from s0 = {s0}")
    finally:
        hip.lib.sdrhip_debug_set_systolic(2)
    del keep
