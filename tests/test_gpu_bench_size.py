"""GPU parity at bench.py's own configuration and on both sides of every launch-size threshold the library routes by.

bench.py times the FM chain over 65 536 blocks of 8192 samples (2^29 u8 IQ samples per pass) with two runs in flight.  At that
size the library's own choice takes routes that smaller tests never reach: the systolic decimator with its seam fix-up as a
second launch (past kFixInsideMaxOutputs), the example's 52 taps on the 64-tap instantiation with that fix-up, fmDemod inside the
resampler's loader over the whole pass.  Here each of them is checked bit for bit against the forced alternative routes and, on
windows of the stream, against the restated reference Pipes; and every size constant of the routing is run at its threshold and
just past it, with a counter proving that the route flipped between the two sizes.

The threshold values are not exported: they are restated below with the source line they come from.  If one moves, the "route
flipped" assertions fail instead of testing one side twice."""
import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from oracle.oracle import duplicate
from oracle import pipes_model as PM
from sdr_amd import sharding
import signals as S
from gpu_util import dev_empty_f32, ptr, to_host

pytestmark = pytest.mark.gpu

B = 8192
BENCH_BLOCKS = 65536                 # bench.py --blocks default: one pass = 2^29 samples
# The seamed chain repeats itself every 80 input blocks: 80 * 8192 / 8 = 81 920 decimator outputs (a multiple of the resampler's 10
# and of the 1024-output seam grid), * 3 / 10 = 24 576 audio samples (three audio blocks).
PERIOD_BLOCKS, PERIOD_AUDIO = 80, 3 * B
WIN_BLOCKS = 120                     # the restated Pipes emit whole audio blocks: 116 blocks in are the fewest that give three out
SKIP = 256                           # a window not at 0 starts with fmDemod's carried sample 0: its first outputs may differ

# the routing constants (not exported)
FIX_INSIDE_MAX = 1 << 23             # kFixInsideMaxOutputs, sdr_amd/csrc/kernels_systolic.hip:342
PLAIN_MIN, PLAIN_MAX = 1000 * 1024, 4400 * 1024   # kPlainLoadMinOutputs / kPlainLoadMaxOutputs, kernels_systolic.hip:340-341
SYSTOLIC_MIN = 64 * 240 * 4          # the systolic launcher's minimum count, kernels_systolic.hip:353
SMALL_CHAIN_MAX = 159 * 1728         # kSmallChainAutoOutputs, sdr_amd/csrc/chain.cpp:41
FUSED_TAIL_MAX = 768                 # kFusedTailAutoOutputs, chain.cpp:35
FUSED_DEMOD_MIN = 1 << 18            # kFusedDemodMinOutputs, sdr_amd/csrc/abi_device.cpp:23 (resampler outputs of one launch)


def _taps(example):
    if example:
        return S.taps_example_rf_decim(), S.taps_example_audio_resampler(), S.taps_example_audio_filter_half()
    return S.taps_decim127(), S.taps_resamp191(), S.taps_audio_half64()


def _chain(hip, example=False):
    hd, hr, ha = _taps(example)
    return hip.FmChain(8, hd, 3, 10, hr, ha, 0.2, B)


def _counters(hip):
    """The process-wide route counters: systolic decimator launches, those with plain cfloat loads, stand-alone seam fix-up launches
    of the complex decimator, one-kernel chain launches, resampler launches with fmDemod in their loader."""
    L = hip.lib
    return {"systolic": int(L.sdrhip_debug_systolic_launches()), "plain": int(L.sdrhip_debug_systolic_plain_launches()),
            "crossfix": int(L.sdrhip_debug_decimator_crossfix_launches()), "small_chain": int(L.sdrhip_debug_small_chain_launches()),
            "fused_demod": int(L.sdrhip_debug_fused_demod_launches())}


@pytest.fixture
def routes(hip):
    """Snapshots of the route counters; the systolic mode goes back to the library's own choice afterwards."""
    try:
        yield lambda: _counters(hip)
    finally:
        hip.lib.sdrhip_debug_set_systolic(2)


def _delta(a, b):
    return {k: b[k] - a[k] for k in a}


def _timed_run(chain, *args, **kw):
    """One run with per-stage timing on -> stage_ms (what ran: a stage that did not run reads 0)."""
    chain.enable_timing(True)
    try:
        chain.run(*args, **kw)
        torch.cuda.synchronize()
        stage_ms, runs = chain.read_timing()
    finally:
        chain.enable_timing(False)
    assert runs == 1
    return stage_ms


def _patchy(u8, seed, nedges):
    """Stretches of silence (decimator output exactly 0: fmDemod's 0/0 clause) and of DC (the product's imaginary part exactly 0: atan2's
    axis clauses) between stretches of noise, cut at odd places (as tests/test_gpu_fullsize.py:test_chain_demod_fusion_is_invisible)."""
    n = u8.numel() // 2
    rng = np.random.default_rng(seed)
    edges = np.sort(rng.integers(0, n, nedges)) * 2
    for k in range(0, len(edges) - 1, 2):
        a, b = int(edges[k]), int(edges[k + 1])
        if k % 4 == 0:
            u8[a:b] = 128
        else:
            u8[a:b:2] = int(rng.integers(0, 256))
            u8[a + 1:b:2] = int(rng.integers(0, 256))


def _same(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _first_diff(a, b):
    bad = torch.nonzero(a.view(torch.int32) != b.view(torch.int32))
    return f"{bad.numel()} of {a.numel()} differ, first at {int(bad[0]) if bad.numel() else -1}"


# ---------------------------------------------------------------------------------------------------------------------------------
# 1 + 2: the chain at the bench's own configuration (bench.py:measure), bench taps and the reference example's own taps
# ---------------------------------------------------------------------------------------------------------------------------------
class BenchPass:
    pass


@pytest.fixture(scope="module", params=[("bench", "uniform"), ("bench", "patchy"), ("example", "uniform")], ids=lambda p: "-".join(p))
def bench_pass(request, hip):
    """One pass of bench.py's workload: FmChain as bench.py builds it, ShardPlan(chain, 0, 1, 65536 * 8192), S_len + halo_cap input
    samples, the workspace of workspace_bytes(S_len + halo_cap) -- run once on the library's own route (A) with route counters and
    per-stage timing."""
    taps, kind = request.param
    P = BenchPass()
    P.example = taps == "example"
    P.kind = kind
    P.chain = _chain(hip, P.example)
    S_len = BENCH_BLOCKS * B
    P.plan = sharding.ShardPlan(P.chain, 0, 1, S_len)
    assert P.plan.q0 == 0 and P.plan.s0 == 0
    n = S_len + P.plan.halo_cap
    gen = torch.Generator(device="cuda").manual_seed(S.SEED_IQ)          # bench.py's generator for rank 0
    P.u8 = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=gen)
    if kind == "patchy":
        _patchy(P.u8, 2029, 4000)
    P.ws = torch.empty(P.chain.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    P.nq = P.plan.q1 - P.plan.q0
    hip.lib.sdrhip_debug_set_systolic(2)
    before = _counters(hip)
    P.audio = torch.full((P.nq,), float("nan"), device="cuda")
    P.stage_ms = _timed_run(P.chain, ptr(P.u8), P.plan.s0, P.plan.n_in, ptr(P.audio), P.plan.q0, P.plan.q1, ptr(P.ws), P.ws.numel())
    P.delta = _delta(before, _counters(hip))
    yield P
    del P.u8, P.ws, P.audio, P.chain
    torch.cuda.empty_cache()


def test_bench_default_route_is_the_expected_one(bench_pass):
    """(a) One run of the default route: one systolic decimator launch with its seam fix-up as a launch of its own (past 2^23 outputs),
    not the one-kernel chain, fmDemod inside the resampler's loader."""
    P = bench_pass
    assert P.delta["systolic"] == 1, f"the systolic decimator did not take the bench's launch ({P.delta})"
    assert P.delta["crossfix"] == 1, f"the seam fix-up did not run as a second launch ({P.delta})"
    assert P.delta["small_chain"] == 0, P.delta
    assert P.delta["fused_demod"] == 1, f"fmDemod did not run inside the resampler's loader ({P.delta})"
    assert P.stage_ms["fm_demod"] == 0.0 and P.stage_ms["decimate"] > 0.0 and P.stage_ms["resample"] > 0.0, P.stage_ms
    assert not torch.isnan(P.audio).any(), "the run left outputs unwritten"


def test_bench_routes_agree(bench_pass, hip, routes):
    """(b) Whole-buffer bit equality of the default route with the LDS-tiled decimator (its own seam handling) and with a stand-alone
    fmDemod kernel."""
    P = bench_pass
    args = (ptr(P.u8), P.plan.s0, P.plan.n_in)
    other = dev_empty_f32(P.nq)
    hip.lib.sdrhip_debug_set_systolic(0)
    before = routes()
    P.ws.fill_(0x5A)                     # stale workspace contents must not matter
    P.chain.run(*args, ptr(other), P.plan.q0, P.plan.q1, ptr(P.ws), P.ws.numel())
    torch.cuda.synchronize()
    d = _delta(before, routes())
    hip.lib.sdrhip_debug_set_systolic(2)
    assert d["systolic"] == 0 and d["crossfix"] == 1, d
    assert _same(P.audio, other), f"set_systolic(0): {_first_diff(P.audio, other)}"
    P.chain.set_demod_fusion(False)
    try:
        before = routes()
        stage_ms = _timed_run(P.chain, *args, ptr(other), P.plan.q0, P.plan.q1, ptr(P.ws), P.ws.numel())
        d = _delta(before, routes())
    finally:
        P.chain.set_demod_fusion(True)
    assert stage_ms["fm_demod"] > 0.0 and d["fused_demod"] == 0 and d["systolic"] == 1, (stage_ms, d)
    assert _same(P.audio, other), f"set_demod_fusion(False): {_first_diff(P.audio, other)}"


def test_bench_two_runs_in_flight(bench_pass, hip):
    """(d) set_overlap(True) as bench.py uses it: runs alternating over two different inputs, audio and input double-buffered, each run
    on one half of the workspace -- every run's audio equals the one-at-a-time result for its input."""
    P = bench_pass
    gen = torch.Generator(device="cuda").manual_seed(S.SEED_IQ + 17)
    u8_b = torch.randint(0, 256, P.u8.shape, dtype=torch.uint8, device="cuda", generator=gen)
    ref_b = dev_empty_f32(P.nq)
    P.chain.run(ptr(u8_b), P.plan.s0, P.plan.n_in, ptr(ref_b), P.plan.q0, P.plan.q1, ptr(P.ws), P.ws.numel())
    inputs, refs = [P.u8, u8_b], [P.audio, ref_b]
    P.chain.set_overlap(True)
    try:
        wsb = P.chain.workspace_bytes(P.plan.n_in)
        assert wsb >= 2 * P.ws.numel() - 512
        ws2 = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        audio = [dev_empty_f32(P.nq) for _ in range(2)]
        st = torch.cuda.current_stream()
        order = [0, 1, 0, 1, 1, 0]
        checked = 0
        for k, which in enumerate(order):
            if k >= 2:      # run k - 2's audio is complete on this stream before run k reuses its buffer
                assert _same(audio[k % 2], refs[order[k - 2]]), f"run {k - 2}: {_first_diff(audio[k % 2], refs[order[k - 2]])}"
                checked += 1
            P.chain.run(ptr(inputs[which]), P.plan.s0, P.plan.n_in, ptr(audio[k % 2]), P.plan.q0, P.plan.q1, ptr(ws2), wsb,
                        stream=st.cuda_stream)
        P.chain.join(st.cuda_stream)
        n = len(order)
        for k in (n - 2, n - 1):
            assert _same(audio[k % 2], refs[order[k]]), f"run {k}: {_first_diff(audio[k % 2], refs[order[k]])}"
            checked += 1
        assert checked == n
    finally:
        P.chain.set_overlap(False)
    del ws2, u8_b
    torch.cuda.empty_cache()


def _oracle_windows(oracle, u8, audio, q1, js, example, what):
    """The restated Pipes on input blocks [80 j, 80 j + 120) reproduce the device's audio from 24576 j + 256 on (from 0 when j = 0).
    Blocks past the real input are filler: only outputs below q1 are compared, whose receptive fields lie inside the real input."""
    hd, hr, ha = _taps(example)
    n_real = u8.numel() // 2
    for j in js:
        a = PERIOD_BLOCKS * j * B
        hi = min(a + WIN_BLOCKS * B, n_real)
        assert hi > a
        raw = np.full(2 * WIN_BLOCKS * B, 128, np.uint8)
        raw[: 2 * (hi - a)] = u8[2 * a: 2 * hi].cpu().numpy()
        blocks = [raw[2 * i * B: 2 * (i + 1) * B] for i in range(WIN_BLOCKS)]
        exp = np.concatenate(PM.fm_receiver(oracle, blocks, hd, 8, hr, 3, 10, ha, 0.2, B))
        base = PERIOD_AUDIO * j
        lo, top = base + (0 if j == 0 else SKIP), min(q1, base + exp.size)
        assert exp.size >= PERIOD_AUDIO and top > lo, (j, exp.size)
        assert_bit_equal(to_host(audio[lo:top]), exp[lo - base: top - base], f"{what}: window j = {j}, audio [{lo}, {top})")
        yield top


def test_bench_audio_against_the_pipes_on_windows(bench_pass, oracle):
    """(c) Windows of the restated reference Pipes over the bench-size stream: the first (nothing skipped), windows around sample 2^28
    (the middle), seeded random ones and the last, which reaches the final output q1 - 1.  Each covers many 8192-sample seams of every
    stage."""
    P = bench_pass
    q1 = P.plan.q1
    jlast = (q1 - 1) // PERIOD_AUDIO
    mid = (1 << 28) // (PERIOD_BLOCKS * B)
    rng = np.random.default_rng(80 + P.example + 2 * (P.kind == "patchy"))
    if P.example:
        js = [0, mid, int(rng.integers(1, jlast)), jlast - 1, jlast]
    else:
        js = sorted({0, 1, mid - 1, mid, mid + 1, jlast - 1, jlast} | {int(j) for j in rng.integers(1, jlast, 20)})
    tops = list(_oracle_windows(oracle, P.u8, P.audio, q1, js, P.example, f"{'example' if P.example else 'bench'} taps, {P.kind}"))
    assert tops[-1] == q1, "the last window did not reach the final output"


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: BASELINE configs[1] -- the cfloat decimator (127 -> 128 taps, /8) over 2^27 samples
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seam", [B, 0])
def test_cfloat_decimator_at_2_to_the_27(hip, oracle, routes, seam):
    """configs[1]: 2^27 cfloat samples (1 GiB), 2^24 - 15 outputs: the systolic kernel with non-temporal loads, its seam fix-up as a
    launch of its own; whole-buffer equal to the LDS-tiled kernel, and spot outputs against the oracle on their 128-sample windows."""
    n = 1 << 27
    g = torch.Generator(device="cuda").manual_seed(27)
    x = torch.rand(2 * n, device="cuda", generator=g) * 2 - 1
    taps = S.taps_decim127()
    h = np.concatenate([taps, np.zeros(1, np.float32)])
    dec = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
    K = (n - 128) // 8 + 1
    assert K > FIX_INSIDE_MAX and K > PLAIN_MAX
    out = dev_empty_f32(2 * K)
    before = routes()
    dec.run(ptr(x), 0, ptr(out), 0, K, seam)
    torch.cuda.synchronize()
    d = _delta(before, routes())
    assert d["systolic"] == 1 and d["plain"] == 0 and d["crossfix"] == (1 if seam else 0), d
    tile = dev_empty_f32(2 * K)
    hip.lib.sdrhip_debug_set_systolic(0)
    dec.run(ptr(x), 0, ptr(tile), 0, K, seam)
    torch.cuda.synchronize()
    hip.lib.sdrhip_debug_set_systolic(2)
    assert _same(out, tile), f"systolic vs tile kernel: {_first_diff(out, tile)}"
    del tile
    rng = np.random.default_rng(127 + seam)
    ks = {0, K - 1} | set(range(0, K, 1 << 16)) | {int(k) for k in rng.integers(0, K, 800)}
    for s in rng.choice(np.arange(1, n // B), 64, replace=False):        # 64 distinct seams
        e = int(s) * B // 8              # the first output whose window starts at the seam
        ks |= set(range(e - 15, e + 1))  # the 15 Cross outputs (with seams on) and the first One output after them
    ks = np.array(sorted(k for k in ks if 0 <= k < K), np.int64)
    assert ks.size >= 2000
    idx = torch.from_numpy(16 * ks[:, None] + np.arange(256)[None, :]).cuda()
    wins = x[idx].cpu().numpy()
    got = out.view(-1, 2)[torch.from_numpy(ks).cuda()].cpu().numpy()
    ncross = 0
    for i, k in enumerate(ks):
        cross = seam and (8 * k) // seam != (8 * k + 127) // seam
        ncross += bool(cross)
        if cross:
            exp = oracle.decimate_cross_c(8, h, 1, wins[i], np.zeros(2, np.float32))
        else:
            exp = oracle.decimate_rc(4, 1, 8, duplicate(h), wins[i])
        assert_bit_equal(got[i], exp, f"output {k} ({'cross' if cross else 'one'}), seam {seam}")
    assert ncross >= (64 * 15 if seam else 0)
    del x, out
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: both sides of every size threshold
# ---------------------------------------------------------------------------------------------------------------------------------
def _decimate_both(hip, routes, dec, u8, d_in, K, seam):
    """The library's own route and the forced tile kernel over outputs [0, K) -> (route deltas of the first, both outputs)."""
    outs = []
    before = routes()
    for mode in (2, 0):
        hip.lib.sdrhip_debug_set_systolic(mode)
        out = dev_empty_f32(2 * K)
        (dec.run_u8 if u8 else dec.run)(ptr(d_in), 0, ptr(out), 0, K, seam)
        torch.cuda.synchronize()
        if mode == 2:
            d = _delta(before, routes())
        outs.append(out)
    hip.lib.sdrhip_debug_set_systolic(2)
    return d, outs


@pytest.mark.parametrize("kind", ["u8-128", "cfloat-128", "u8-52"])
def test_fix_inside_threshold(hip, routes, kind):
    """kFixInsideMaxOutputs: at 2^23 outputs the seam fix-up runs inside the systolic launch, at 2^23 + 2 as a launch of its own --
    both bit-equal with the tile kernel, 8192-sample seams."""
    u8 = kind.startswith("u8")
    taps = S.taps_example_rf_decim() if kind.endswith("52") else S.taps_decim127()
    dec = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
    Lp = 52 if kind.endswith("52") else 128
    Kmax = FIX_INSIDE_MAX + 2
    n = 8 * (Kmax - 1) + Lp
    g = torch.Generator(device="cuda").manual_seed(23)
    if u8:
        d_in = torch.randint(0, 256, (2 * n,), dtype=torch.uint8, device="cuda", generator=g)
    else:
        d_in = torch.rand(2 * n, device="cuda", generator=g) * 2 - 1
    inside = {}
    for K in (FIX_INSIDE_MAX, FIX_INSIDE_MAX + 2):
        d, (a, b) = _decimate_both(hip, routes, dec, u8, d_in, K, B)
        assert d["systolic"] == 1, (K, d)
        assert _same(a, b), f"{kind}, {K} outputs: {_first_diff(a, b)}"
        inside[K] = d["crossfix"] == 0
        del a, b
    assert inside == {FIX_INSIDE_MAX: True, FIX_INSIDE_MAX + 2: False}, f"the fix-up did not flip from inside to a launch of its own: {inside}"
    del d_in
    torch.cuda.empty_cache()


def test_plain_load_thresholds(hip, routes):
    """kPlainLoadMinOutputs / kPlainLoadMaxOutputs: cfloat launches take plain loads in [1000 * 1024, 4400 * 1024] outputs and
    non-temporal ones outside -- all bit-equal with the tile kernel."""
    counts = [PLAIN_MIN - 2, PLAIN_MIN, PLAIN_MAX, PLAIN_MAX + 2]
    n = 8 * (max(counts) - 1) + 128
    g = torch.Generator(device="cuda").manual_seed(44)
    x = torch.rand(2 * n, device="cuda", generator=g) * 2 - 1
    dec = hip.Decimator(8, S.taps_decim127(), hip.ORDER_AVX, complex_=True)
    plain = []
    for K in counts:
        d, (a, b) = _decimate_both(hip, routes, dec, False, x, K, B)
        assert d["systolic"] == 1, (K, d)
        assert _same(a, b), f"{K} outputs: {_first_diff(a, b)}"
        plain.append(d["plain"])
    assert plain == [0, 1, 1, 0], f"plain-load launches by count {counts}: {plain}"


def test_systolic_minimum(hip, oracle, routes):
    """The systolic launcher's minimum (64 * 240 * 4 outputs): one output fewer stays on the tile kernel, exactly that many takes the
    systolic kernel; both against the oracle's decimateAVXRC."""
    taps = S.taps_decim127()
    h = np.concatenate([taps, np.zeros(1, np.float32)])
    dec = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
    took = []
    for K in (SYSTOLIC_MIN - 1, SYSTOLIC_MIN):
        n = 8 * (K - 1) + 128
        raw = S.iq_u8(n)
        d, (a, b) = _decimate_both(hip, routes, dec, True, torch.from_numpy(raw).cuda(), K, 0)
        assert _same(a, b)
        assert_bit_equal(to_host(a), oracle.decimate_rc(4, K, 8, duplicate(h), oracle.convert_u8(raw)), f"{K} outputs vs the oracle")
        took.append(d["systolic"])
    assert took == [0, 1], f"systolic launches at {SYSTOLIC_MIN - 1} / {SYSTOLIC_MIN} outputs: {took}"


@pytest.fixture(scope="module")
def mid_stream(oracle):
    """1280 blocks of seeded u8 IQ and the restated Pipes' audio of the whole stream: enough for audio runs of 2^18 outputs from the
    stream start and from block 37."""
    nblk = 1280
    u8 = S.iq_u8(nblk * B)
    hd, hr, ha = _taps(False)
    blocks = [u8[2 * i * B:2 * (i + 1) * B] for i in range(nblk)]
    exp = np.concatenate(PM.fm_receiver(oracle, blocks, hd, 8, hr, 3, 10, ha, 0.2, B))
    return u8, exp


def _chain_run(chain, d_u8, s0, N, total):
    """Audio outputs [q0, q0 + N) of a run whose input starts at sample s0 (q0: the plan's first output owned from s0)."""
    q0, q1, _ = chain.plan(s0, total, total)
    assert q1 - q0 >= N + 1
    out = dev_empty_f32(N)
    args = (ptr(d_u8) + 2 * s0, s0, total - s0, ptr(out), q0, q0 + N)
    return q0, out, args


@pytest.mark.parametrize("s0_blocks", [0, 37])
def test_small_chain_threshold(hip, routes, mid_stream, s0_blocks):
    """kSmallChainAutoOutputs: a run of exactly 159 * 1728 audio outputs takes the one-kernel chain, one more takes the stage kernels --
    both equal to the stage kernels forced by set_small_chain(0) and to the restated Pipes."""
    u8, exp = mid_stream
    total = u8.size // 2
    d_u8 = torch.from_numpy(u8).cuda()
    s0 = s0_blocks * B
    chain = _chain(hip)
    ws = torch.empty(chain.workspace_bytes(total), dtype=torch.uint8, device="cuda")
    took = []
    for N in (SMALL_CHAIN_MAX, SMALL_CHAIN_MAX + 1):
        q0, out, args = _chain_run(chain, d_u8, s0, N, total)
        assert exp.size >= q0 + N
        before = routes()
        chain.run(*args, ptr(ws), ws.numel())
        torch.cuda.synchronize()
        took.append(_delta(before, routes())["small_chain"])
        forced = dev_empty_f32(N)
        chain.set_small_chain(0)
        chain.run(*args[:3], ptr(forced), *args[4:], ptr(ws), ws.numel())
        chain.set_small_chain(2)
        assert _same(out, forced), f"{N} outputs from block {s0_blocks}: {_first_diff(out, forced)}"
        assert_bit_equal(to_host(out), exp[q0:q0 + N], f"{N} outputs from block {s0_blocks} vs the Pipes")
    assert took == [1, 0], f"one-kernel chain launches at {SMALL_CHAIN_MAX} / {SMALL_CHAIN_MAX + 1} outputs: {took}"


@pytest.mark.parametrize("s0_blocks", [0, 37])
def test_fused_tail_threshold(hip, mid_stream, s0_blocks):
    """kFusedTailAutoOutputs (the one-kernel chain off): runs of 768 audio outputs take the fused tail kernel, 769 the stage kernels --
    both equal to set_fused_tail(0) and to the restated Pipes."""
    u8, exp = mid_stream
    total = u8.size // 2
    d_u8 = torch.from_numpy(u8).cuda()
    s0 = s0_blocks * B
    chain = _chain(hip)
    chain.set_small_chain(0)
    ws = torch.empty(chain.workspace_bytes(total), dtype=torch.uint8, device="cuda")
    took = []
    for N in (FUSED_TAIL_MAX, FUSED_TAIL_MAX + 1):
        q0, out, args = _chain_run(chain, d_u8, s0, N, total)
        stage_ms = _timed_run(chain, *args, ptr(ws), ws.numel())
        took.append(stage_ms["fused_tail"] > 0.0)
        forced = dev_empty_f32(N)
        chain.set_fused_tail(0)
        stage_f = _timed_run(chain, *args[:3], ptr(forced), *args[4:], ptr(ws), ws.numel())
        chain.set_fused_tail(2)
        assert stage_f["fused_tail"] == 0.0 and stage_f["filter"] > 0.0, stage_f
        assert _same(out, forced), f"{N} outputs from block {s0_blocks}: {_first_diff(out, forced)}"
        assert_bit_equal(to_host(out), exp[q0:q0 + N], f"{N} outputs from block {s0_blocks} vs the Pipes")
    assert took == [True, False], f"fused tail at {FUSED_TAIL_MAX} / {FUSED_TAIL_MAX + 1} outputs: {took}"


@pytest.mark.parametrize("s0_blocks", [0, 37])
def test_fused_demod_threshold(hip, routes, mid_stream, s0_blocks):
    """kFusedDemodMinOutputs (the one-kernel chain off): the resampler launch of a run covers its audio outputs plus the 127 the audio
    filter looks ahead, so runs of 2^18 - 128 and 2^18 - 127 audio outputs put 2^18 - 1 and 2^18 outputs into it -- the first with a
    stand-alone fmDemod, the second with fmDemod in its loader; both equal to set_demod_fusion(False) and to the restated Pipes."""
    u8, exp = mid_stream
    total = u8.size // 2
    d_u8 = torch.from_numpy(u8).cuda()
    s0 = s0_blocks * B
    chain = _chain(hip)
    chain.set_small_chain(0)
    ws = torch.empty(chain.workspace_bytes(total), dtype=torch.uint8, device="cuda")
    lookahead = 2 * S.taps_audio_half64().size - 1
    took = []
    for M in (FUSED_DEMOD_MIN - 1, FUSED_DEMOD_MIN):
        N = M - lookahead
        q0, out, args = _chain_run(chain, d_u8, s0, N, total)
        before = routes()
        stage_ms = _timed_run(chain, *args, ptr(ws), ws.numel())
        took.append(_delta(before, routes())["fused_demod"])
        assert stage_ms["fm_demod"] == 0.0, "with the fusion on, fmDemod is booked under `resample` either way"
        forced = dev_empty_f32(N)
        chain.set_demod_fusion(False)
        stage_f = _timed_run(chain, *args[:3], ptr(forced), *args[4:], ptr(ws), ws.numel())
        chain.set_demod_fusion(True)
        assert stage_f["fm_demod"] > 0.0, stage_f
        assert _same(out, forced), f"resampler launch of {M} outputs from block {s0_blocks}: {_first_diff(out, forced)}"
        assert_bit_equal(to_host(out), exp[q0:q0 + N], f"{N} audio outputs from block {s0_blocks} vs the Pipes")
    assert took == [0, 1], f"fused fmDemod launches at {FUSED_DEMOD_MIN - 1} / {FUSED_DEMOD_MIN} resampler outputs: {took}"
