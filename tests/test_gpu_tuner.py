"""GPU parity of the tuner (sdrhip_tuner_*, sdrhip_pipe_tuner): the oscillator mix in front of the complex decimator against the
restated Pipe on the mixed stream (tests/tuner_model.py) and against its defining identity -- sdrhip_decimator_run on a device
buffer that already holds the mixed samples -- on both routes, bit for bit."""
import threading

import numpy as np
import pytest

import signals as S
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B = 8192
NBLK = 5
CUTS = [1, 1000, 1009, 1024, 3000]
PERIODS = [1, 2, 4, 5, 1000, 8192, 65536]      # 5 and 1000 divide neither a tile (4096 samples) nor a block; 65536 > the input


def osc_table(n):
    """An oscillator of period n: the shift tables, and for n = 1 a lone user value."""
    if n == 1:
        return np.array([0.6, -0.8], np.float32)
    num = {2: 1, 4: 1, 5: 2, 1000: 7, 8192: 4095, 65536: 1}[n]
    return TM.shift_table(num, n)


_cache = {}


def stream_u8():
    """5 blocks of uniform u8 IQ with 127 / 128 / 129 forced into a few dozen positions, block edges included: converted, 128
    is +0, and the mix then meets zeros of both signs."""
    if "u8" not in _cache:
        u8 = S.iq_u8(NBLK * B).copy()
        rng = np.random.default_rng(77)
        pos = list(rng.integers(0, 2 * NBLK * B, 40))
        for e in (B, 2 * B, 3 * B):
            pos += [2 * e - 2, 2 * e - 1, 2 * e, 2 * e + 1, 2 * e + 3]
        pos += [0, 1, 2 * NBLK * B - 1]
        for i, p in enumerate(pos):
            u8[p] = (128, 127, 129, 128)[i % 4]
        _cache["u8"] = u8
    return _cache["u8"]


def expected(oracle, n, seam):
    """Every output of the 5-block stream for period n (computed once per (n, seam), shared, never written)."""
    key = ("exp", n, seam)
    if key not in _cache:
        x = oracle.convert_u8(stream_u8())
        e = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, x, osc_table(n), seam, 0, block_out=1)
        e.setflags(write=False)
        _cache[key] = e
    return _cache[key]


def run_ranges(op, d_in, K, seam, cuts, u8, k0=0, in_base=0):
    """Outputs [k0, k0 + K) as launches cut at k0 + cuts, all reading the same device buffer (whose sample 0 is in_base)."""
    out = dev_empty_f32(2 * K)
    edges = [0] + [c for c in cuts if c < K] + [K]
    for a, b in zip(edges[:-1], edges[1:]):
        (op.run_u8 if u8 else op.run)(ptr(d_in), in_base, ptr(out) + 8 * a, k0 + a, k0 + b, seam)
    return to_host(out)


@pytest.fixture(params=["Cross outputs in the tile kernel", "tile kernel + fix-up launch"])
def launch_route(hip, request):
    """Short seamed launches compute their Cross outputs inside the tile kernel by default; with the threshold at 0 every
    seamed launch takes the fix-up launch (sdrhip_set_small_launch_outputs)."""
    prev = hip.set_small_launch_outputs(-1 if request.param.startswith("Cross") else 0)
    yield request.param
    hip.set_small_launch_outputs(prev)


@pytest.mark.parametrize("seam", [0, B])
@pytest.mark.parametrize("n", PERIODS)
def test_fused_route_against_the_model(hip, oracle, n, seam, launch_route):
    exp = expected(oracle, n, seam)
    K = exp.size // 2
    assert K == (NBLK * B - 128) // 8 + 1 and K % 512 != 0         # the last tile of the whole stream is ragged
    u8 = stream_u8()
    x = oracle.convert_u8(u8)
    t = hip.Tuner(8, S.taps_decim127(), osc_table(n))
    assert (t.num_coeffs, t.period) == (128, n)
    t.set_route(hip.TUNER_ROUTE_FUSED)
    for is_u8, d_in in ((True, to_dev(u8)), (False, to_dev(x))):
        what = f"period {n}, seam {seam}, {'u8' if is_u8 else 'cfloat'}"
        c0 = hip.tuner_fused_launches()
        assert_bit_equal(run_ranges(t, d_in, K, seam, [], is_u8), exp, what + ": one launch")
        assert_bit_equal(run_ranges(t, d_in, K, seam, CUTS, is_u8), exp, what + ": cut into launches")
        assert_bit_equal(run_ranges(t, d_in, 4097, seam, [], is_u8), exp[:2 * 4097], what + ": one output into the ninth tile")
        assert_bit_equal(run_ranges(t, d_in, 4608, seam, [], is_u8), exp[:2 * 4608], what + ": whole tiles")
        assert hip.tuner_fused_launches() - c0 == 1 + (len(CUTS) + 1) + 1 + 1, "the fused route did not serve every launch"


@pytest.mark.parametrize("seam", [0, B])
@pytest.mark.parametrize("n", PERIODS)
def test_two_pass_route_and_the_defining_identity(hip, oracle, n, seam, launch_route):
    """Route 2 gives route 1's bits without a fused launch, and both give sdrhip_decimator_run's on a device buffer holding the
    mixed samples uploaded from the host."""
    u8 = stream_u8()
    x = oracle.convert_u8(u8)
    osc = osc_table(n)
    taps = S.taps_decim127()
    K = (NBLK * B - 128) // 8 + 1
    dec = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
    ident = run_ranges(dec, to_dev(TM.mix(x, osc, 0)), K, seam, CUTS, False)
    assert_bit_equal(ident, expected(oracle, n, seam), "decimator on the mixed stream against the model")
    t = hip.Tuner(8, taps, osc)
    for is_u8, d_in in ((True, to_dev(u8)), (False, to_dev(x))):
        what = f"period {n}, seam {seam}, {'u8' if is_u8 else 'cfloat'}"
        t.set_route(hip.TUNER_ROUTE_FUSED)
        fused = run_ranges(t, d_in, K, seam, CUTS, is_u8)
        t.set_route(hip.TUNER_ROUTE_TWO_PASS)
        c0 = hip.tuner_fused_launches()
        two = run_ranges(t, d_in, K, seam, CUTS, is_u8)
        two_whole = run_ranges(t, d_in, K, seam, [], is_u8)
        prev = hip.set_tuner_chunk(5000)                   # several scratch chunks per launch, cut at no tile or block edge
        try:
            two_chunked = run_ranges(t, d_in, K, seam, [3000], is_u8)
        finally:
            hip.set_tuner_chunk(prev)
        assert hip.tuner_fused_launches() == c0, "route 2 launched the fused kernel"
        assert_bit_equal(two, fused, what + ": two-pass against fused")
        assert_bit_equal(two_whole, fused, what + ": two-pass, one launch")
        assert_bit_equal(two_chunked, fused, what + ": two-pass in 5000-sample chunks")
        assert_bit_equal(fused, ident, what + ": fused against the decimator on the mixed stream")


def _short_case(hip, oracle, order, factor, ntaps, n, fused, u8_too=True):
    """3 blocks of 4096 samples, one launch and one cut; `fused`: which route `auto` must take."""
    nb, blk = 3, 4096
    u8 = stream_u8()[:2 * nb * blk]
    x = oracle.convert_u8(u8)
    taps = S.taps_decim127() if ntaps == 127 else S.gauss_taps(ntaps, 40 + ntaps)
    osc = osc_table(n)
    exp = TM.tuner_expected(oracle, taps, order, factor, x, osc, blk, 0, block_out=1)
    K = exp.size // 2
    t = hip.Tuner(factor, taps, osc, order)
    for is_u8, d_in in ((True, to_dev(u8)), (False, to_dev(x)))[0 if u8_too else 1:]:
        what = f"order {order}, factor {factor}, {ntaps} taps, period {n}, {'u8' if is_u8 else 'cfloat'}"
        c0 = hip.tuner_fused_launches()
        assert_bit_equal(run_ranges(t, d_in, K, blk, [], is_u8), exp, what)
        assert (hip.tuner_fused_launches() - c0 == 1) == fused, what + ": auto took the wrong route"
        assert_bit_equal(run_ranges(t, d_in, K, blk, [64, 500], is_u8), exp, what + ", cut")
        assert (hip.tuner_fused_launches() - c0 == 4) == fused
    return t, exp, K


@pytest.mark.parametrize("factor,ntaps", [(4, 127), (16, 127), (8, 31), (8, 52), (8, 64), (4, 52), (16, 31)])
def test_fused_route_other_factors_and_tap_counts(hip, oracle, factor, ntaps, launch_route):
    """Factor 16: a tile spans more than a 4096-sample block, so the Cross outputs come from the fix-up launch under either
    setting; 52 taps walk the taps four at a time."""
    _short_case(hip, oracle, PM.ORDER_AVX, factor, ntaps, 5, fused=True)


@pytest.mark.parametrize("order,factor", [(PM.ORDER_SSE, 8), (PM.ORDER_SCALAR, 8), (PM.ORDER_AVX, 5), (PM.ORDER_SSE, 5)])
def test_two_pass_serves_every_other_order_and_factor(hip, oracle, order, factor, launch_route):
    t, exp, K = _short_case(hip, oracle, order, factor, 127, 1000, fused=False)
    t.set_route(hip.TUNER_ROUTE_FUSED)                       # no kernel for this shape: an error, not another route
    d_in = to_dev(oracle.convert_u8(stream_u8()[:2 * 3 * 4096]))
    with pytest.raises(hip.SdrHipError):
        t.run(ptr(d_in), 0, ptr(dev_empty_f32(2 * K)), 0, K, 4096)


def test_auto_falls_back_where_a_launch_is_not_aligned(hip, oracle):
    """Factor 4 on u8: output 1's window starts 8 bytes into the buffer, which the tile kernel's 16-byte loads cannot take --
    `auto` runs that launch on the two-pass route, same bits."""
    u8 = stream_u8()[:2 * 3 * 4096]
    taps, osc = S.taps_decim127(), osc_table(1000)
    exp = TM.tuner_expected(oracle, taps, PM.ORDER_AVX, 4, oracle.convert_u8(u8), osc, 4096, 0, block_out=1)
    K = exp.size // 2
    t = hip.Tuner(4, taps, osc)
    c0 = hip.tuner_fused_launches()
    assert_bit_equal(run_ranges(t, to_dev(u8), K, 4096, [1, 2], True), exp, "factor 4, cut at outputs 1 and 2")
    assert hip.tuner_fused_launches() - c0 == 2            # [0, 1) and [2, K) are aligned, [1, 2) is not


def test_user_table_with_subnormals_and_negative_zeros(hip, oracle):
    """A table no shortcut survives: subnormal, tiny, -0 and ordinary entries (period 7), on both routes against the model."""
    osc = np.array([1e-42, -3e-39, -0.0, 1.0, 0.0, -0.0, 0.70710677, -0.70710677, -1.0, 1e-45, 2.5, -0.0, 1e-30, 3.0, -0.0, -0.0],
                   np.float32)[:14]
    u8 = stream_u8()[:2 * 2 * B]
    x = oracle.convert_u8(u8)
    exp = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, x, osc, B, 0, block_out=1)
    K = exp.size // 2
    t = hip.Tuner(8, S.taps_decim127(), osc)
    for route in (hip.TUNER_ROUTE_FUSED, hip.TUNER_ROUTE_TWO_PASS):
        t.set_route(route)
        assert_bit_equal(run_ranges(t, to_dev(u8), K, B, [700], True), exp, f"route {route}, u8")
        assert_bit_equal(run_ranges(t, to_dev(x), K, B, [700], False), exp, f"route {route}, cfloat")


@pytest.mark.parametrize("n", [1000, 5])
def test_far_stream_position(hip, oracle, n, launch_route):
    """in_base = 8 k_begin with k_begin = 3 * 2^30 + 5: the stream position is past 2^34 samples and the device buffer holds only
    the slice; the model mixes the slice with pos0 = in_base.  Pins the 64-bit phase arithmetic (in_base mod 1000 = 816,
    mod 5 = 1; the slice starts 40 samples into a block)."""
    k_begin = 3 * 2 ** 30 + 5
    in_base = 8 * k_begin
    assert in_base % B == 40 and in_base % 1000 == 816 and in_base % 5 == 1
    ns = 3 * B - 40
    u8 = stream_u8()[:2 * ns]
    x = oracle.convert_u8(u8)
    osc = osc_table(n)
    exp = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, x, osc, B, in_base, block_out=1)
    K = exp.size // 2
    assert K == (ns - 128) // 8 + 1
    t = hip.Tuner(8, S.taps_decim127(), osc)
    for route in (hip.TUNER_ROUTE_FUSED, hip.TUNER_ROUTE_TWO_PASS):
        t.set_route(route)
        for is_u8, d_in in ((True, to_dev(u8)), (False, to_dev(x))):
            what = f"period {n}, route {route}, {'u8' if is_u8 else 'cfloat'}"
            assert_bit_equal(run_ranges(t, d_in, K, B, [], is_u8, k_begin, in_base), exp, what)
            assert_bit_equal(run_ranges(t, d_in, K, B, [1000, 1019], is_u8, k_begin, in_base), exp, what + ", cut")


def _drive(pipe, blocks):
    outs = []
    for b in blocks:
        outs += pipe.push(b)
    return outs


def _cut(x, sizes):
    out, pos = [], 0
    for s in sizes:
        out.append(x[2 * pos:2 * (pos + s)])
        pos += s
    return out


def _cmp(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} blocks vs {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        assert_bit_equal(g, e, f"{what} block {i}")


def test_pipe_ragged_pushes(hip, oracle):
    """`P.map (zipWith (*) osc) >-> firDecimator` on ragged host blocks: the reference's Pipe on the mixed blocks.  A 1-sample
    block is shorter than the filter -- the reference asserts (Filter.hs:586), the Pipe refuses it with an error and carries
    on as if it had not been pushed, as sdrhip_pipe_fir_decimator does."""
    sizes = [8191, 8192, 20000, 8192, 8191, 300, 12000]
    x = S.cfloat_block(sum(sizes))
    osc = osc_table(1000)
    taps = S.taps_decim127()
    model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=8)
    exp, _ = PM.fir_decimator_pipe(model, _cut(TM.mix(x, osc, 0), sizes), 700)
    t = hip.Tuner(8, taps, osc)
    for route in (hip.TUNER_ROUTE_AUTO, hip.TUNER_ROUTE_TWO_PASS):
        t.set_route(route)
        pipe = hip.Pipe.tuner(t, 700)
        got = []
        for i, b in enumerate(_cut(x, sizes)):
            if i in (0, 2):
                with pytest.raises(hip.SdrHipError):
                    pipe.push(np.zeros(2, np.float32))
            got += pipe.push(b)
        _cmp(got + pipe.flush(), exp, f"ragged tuner pipe, route {route}")


@pytest.mark.parametrize("mode", ["coalesce", "adaptive"])
def test_pipe_uniform_blocks_coalesce_and_adaptive(hip, oracle, mode):
    nblk = 12
    x = oracle.convert_u8(stream_u8())
    x = np.concatenate([x, S.cfloat_block((nblk - NBLK) * B)])
    osc = osc_table(1000)                                   # 1000 does not divide the block: every block starts at another phase
    taps = S.taps_decim127()
    model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=8)
    exp, _ = PM.fir_decimator_pipe(model, _cut(TM.mix(x, osc, 0), [B] * nblk), 512)
    t = hip.Tuner(8, taps, osc)
    pipe = hip.Pipe.tuner(t, 512)
    if mode == "coalesce":
        pipe.set_coalesce(5)
    else:
        pipe.set_adaptive(4)
    c0 = hip.tuner_fused_launches()
    got = _drive(pipe, _cut(x, [B] * nblk)) + pipe.flush()
    _cmp(got, exp, f"uniform tuner pipe, {mode}")
    assert hip.tuner_fused_launches() > c0, "uniform blocks of the AVX shape take the fused route"


def test_pipe_save_and_restore_mid_stream(hip, oracle):
    """Saved after 4 of 9 ragged blocks at a position that is no multiple of the period, restored into a fresh Pipe: the saved
    stream position selects the oscillator phase of everything that follows."""
    sizes = [4096, 8192, 1000, 20000, 777, 8192, 300, 5000, 8192]       # every block holds a whole filter behind its crossover
    x = S.cfloat_block(sum(sizes))
    osc = osc_table(1000)
    taps = S.taps_decim127()
    model = PM.FilterModel(oracle, taps, PM.ORDER_AVX, complex_=True, factor=8)
    exp, _ = PM.fir_decimator_pipe(model, _cut(TM.mix(x, osc, 0), sizes), 700)
    t = hip.Tuner(8, taps, osc)
    blocks = _cut(x, sizes)
    cut = 4
    assert sum(sizes[:cut]) % 1000 != 0
    first = hip.Pipe.tuner(t, 700)
    got = _drive(first, blocks[:cut])
    state = first.save()
    second = hip.Pipe.tuner(t, 700)
    got += second.restore(state)
    got += _drive(second, blocks[cut:]) + second.flush()
    _cmp(got, exp, "tuner pipe saved and restored")
    with pytest.raises(hip.SdrHipError):
        dec = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
        hip.firDecimator(dec, 700).restore(state)           # a tuner state is not a decimator state


def test_device_argument_errors(hip, oracle):
    taps, osc = S.taps_decim127(), osc_table(4)
    t = hip.Tuner(8, taps, osc)
    d_in = to_dev(oracle.convert_u8(stream_u8()[:2 * B]))
    out = dev_empty_f32(2 * 64)
    with pytest.raises(hip.SdrHipError):
        t.run(ptr(d_in), 0, ptr(out), 0, 64, 127)           # seam block shorter than the 128 prepared taps
    with pytest.raises(hip.SdrHipError):
        t.run(ptr(d_in), 8, ptr(out), 0, 64, 0)             # the first window starts before d_in
    with pytest.raises(hip.SdrHipError):
        t.run(ptr(d_in), 0, ptr(out), 64, 0, 0)
    with pytest.raises(hip.SdrHipError):
        t.run(ptr(d_in), 0, 0, 0, 64, 0)                    # null output
    t.set_route(hip.TUNER_ROUTE_FUSED)
    with pytest.raises(hip.SdrHipError):
        t.run(ptr(d_in), 0, ptr(out), 0, 64, -1)            # every output Cross: not a fused launch
    t.set_route(hip.TUNER_ROUTE_AUTO)
    t.run(ptr(d_in), 0, ptr(out), 0, 64, -1)                # ... auto runs it on the two-pass route: sequential order
    m = TM.mix(oracle.convert_u8(stream_u8()[:2 * B]), osc, 0)
    dec = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
    ref = dev_empty_f32(2 * 64)
    dec.run(ptr(to_dev(m)), 0, ptr(ref), 0, 64, -1)
    assert_bit_equal(to_host(out), to_host(ref), "all-Cross launch against the decimator on the mixed stream")
    with pytest.raises(hip.SdrHipError):
        hip.Pipe.tuner(t, 0)                                # block_size_out must be positive


def test_one_descriptor_two_host_threads(hip, oracle):
    """One descriptor, two host threads, each on a stream of its own, both routes in turn: the same bits as one thread."""
    import torch
    exp = expected(oracle, 1000, B)
    K = exp.size // 2
    t = hip.Tuner(8, S.taps_decim127(), osc_table(1000))
    d_u8 = to_dev(stream_u8())
    for route in (hip.TUNER_ROUTE_FUSED, hip.TUNER_ROUTE_TWO_PASS):
        t.set_route(route)
        outs = [dev_empty_f32(2 * K) for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        errors = []
        torch.cuda.synchronize()

        def work(i):
            try:
                for rep in range(4):
                    edges = [0] + [c + i for c in CUTS] + [K]
                    for a, b in zip(edges[:-1], edges[1:]):
                        t.run_u8(ptr(d_u8), 0, ptr(outs[i]) + 8 * a, a, b, B, stream=streams[i].cuda_stream)
                streams[i].synchronize()
            except Exception as e:                           # noqa: BLE001 -- reported below, on the main thread
                errors.append(e)

        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for q in th:
            q.start()
        for q in th:
            q.join()
        assert not errors, errors
        for i in range(2):
            assert_bit_equal(to_host(outs[i]), exp, f"route {route}, thread {i}")
