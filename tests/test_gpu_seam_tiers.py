"""One case per seam fix-up tier: every stage launcher rewrites its seam straddlers ("Cross" outputs) with one of a few fix-up
kernels, chosen by the shape (straddlers per seam `per = ceil((Lp - 1) / D)`, the union of inputs they read).  Each case
below is chosen to land in one tier by the bounds in the launcher, so that a bound that moves by accident fails by name.

Every case: bit for bit against the restated Pipes (oracle/pipes_model.py, output block 512), seam block 4096, AVX order,
the one-launch short route off -- one launch of about 20 000 outputs (above every launcher's 4096- / 16 384-output minimum,
several seams), then the same range cut into two launches at an output that is not on a seam."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from oracle import pipes_model as PM
import signals as S
from gpu_util import to_dev, dev_empty_f32, ptr, to_host

pytestmark = pytest.mark.gpu

SEAM = 4096
OUTB = 512
AVX = PM.ORDER_AVX


@pytest.fixture(autouse=True)
def _tiled_route(hip):
    """Short seamed launches take a one-launch route by default (sdrhip_set_small_launch_outputs): off, these tests are about
    the tiled kernels' fix-ups."""
    prev = hip.set_small_launch_outputs(0)
    yield
    hip.set_small_launch_outputs(prev)


def _blocks(x, width, nblk):
    return [x[i * SEAM * width:(i + 1) * SEAM * width] for i in range(nblk)]


def _run(run, d_in, width, K, cuts, **kw):
    out = dev_empty_f32(K * width)
    edges = [0] + list(cuts) + [K]
    assert edges == sorted(set(edges))
    for a, b in zip(edges[:-1], edges[1:]):
        run(ptr(d_in), 0, ptr(out) + 4 * width * a, a, b, SEAM, **kw)
    return to_host(out)


def _both(run, d_in, width, exp, cut, what, **kw):
    """One launch, then two launches cut at `cut` (even, so that the complex tile kernels keep their 16-byte alignment)."""
    K = exp.size // width
    assert 0 < cut < K
    assert_bit_equal(_run(run, d_in, width, K, [], **kw), exp, what + ": one launch")
    assert_bit_equal(_run(run, d_in, width, K, [cut], **kw), exp, what + f": two launches, cut at {cut}")


# ---- real decimator (launch_decimate_real16_fast): per = ceil((Lp - 1) / D), uni(PER) = Lp + PER * D + 4 -------------------
#   /8, 120 taps: per 15 <= 16, uni(16) = 252 <= 416                      -> <16, 416, 32>
#   /4, 128 taps: per 32 (> 16), uni(32) = 260 <= 416                     -> <32, 416, 32>
#   /4, 200 taps: per 50 (> 32), uni(64) = 460 <= 1152                    -> <64, 1152, 64>
#   /2, 300 taps (-> 304): per 152 > 64                                   -> the generic real fix-up
@pytest.mark.parametrize("factor,ntaps,tier", [(8, 120, "lds16"), (4, 128, "lds32"), (4, 200, "lds64"), (2, 300, "generic")])
def test_real_decimator_tier(hip, oracle, factor, ntaps, tier):
    nblk = 5 * factor
    x = S.real_block(nblk * SEAM, seed=7 + factor)
    taps = S.gauss_taps(ntaps, 31 * factor + ntaps)
    model = PM.FilterModel(oracle, taps, AVX, factor=factor)
    blocks, _ = PM.fir_decimator_pipe(model, _blocks(x, 1, nblk), OUTB)
    exp = np.concatenate(blocks)
    d = hip.Decimator(factor, taps, AVX)
    per = -(-(d.num_coeffs - 1) // factor)
    assert {"lds16": per <= 16, "lds32": 16 < per <= 32, "lds64": 32 < per <= 64, "generic": per > 64}[tier]
    before = hip.lib.sdrhip_debug_decimate_real16_launches()
    _both(d.run, to_dev(x), 1, exp, 10001, f"real /{factor}, {ntaps} taps ({tier})")
    assert hip.lib.sdrhip_debug_decimate_real16_launches() == before + 3, "the real decimator's kernel did not take every launch"


def test_real_resampler_interpolation_1_unpadded_cross_taps(hip, oracle):
    """1/2 with 300 taps runs on the real decimator's kernel (Lp = 304); its Cross outputs walk the 300 UNPADDED taps: per = 152
    fits no LDS tier, so it takes the generic resampler fix-up with ncross = 300."""
    nblk = 10
    x = S.real_block(nblk * SEAM, seed=12)
    taps = S.gauss_taps(300, 1200)
    model = PM.ResamplerModel(oracle, 1, 2, taps, AVX, False)
    blocks, _ = PM.fir_resampler_pipe(model, _blocks(x, 1, nblk), OUTB)
    exp = np.concatenate(blocks)
    r = hip.Resampler(1, 2, taps, AVX, False)
    before = hip.lib.sdrhip_debug_decimate_real16_launches()
    _both(r.run, to_dev(x), 1, exp, 10001, "real 1/2, 300 taps", out_block=OUTB)
    assert hip.lib.sdrhip_debug_decimate_real16_launches() == before + 3, "the real decimator's kernel did not take every launch"


# ---- cycle resampler (launch_resample_cycle_fast): uni(PER) = nloop + ceil(PER * D / I) + 4 --------------------------------
#   2/3, 150 taps: Lp 160, per 53 (> 32), nloop 80, uni(64) = 180 <= 384  -> <64, 384, 64>
#   3/5,  37 taps: Lp 48, per 10, nloop 16, uni(32) = 74 <= 192           -> <32, 192, 32>
#   2/3, 700 taps: Lp 704, per 235 > 64                                   -> the generic real fix-up
#   complex 2/3, 150 taps                                                 -> the generic complex fix-up (complex data has no LDS tier)
@pytest.mark.parametrize("I,D,ntaps,complex_,tier", [(2, 3, 150, False, "lds64"), (3, 5, 37, False, "lds32"), (2, 3, 700, False, "generic"),
                                                     (2, 3, 150, True, "generic complex")])
def test_cycle_resampler_tier(hip, oracle, I, D, ntaps, complex_, tier):
    w = 2 if complex_ else 1
    nblk = -(-20000 * D // (I * SEAM)) + 1
    x = S.cfloat_block(nblk * SEAM, seed=40 + ntaps) if complex_ else S.real_block(nblk * SEAM, seed=40 + ntaps)
    taps = S.gauss_taps(ntaps, 100 * I + D + ntaps)
    model = PM.ResamplerModel(oracle, I, D, taps, AVX, complex_)
    blocks, _ = PM.fir_resampler_pipe(model, _blocks(x, w, nblk), OUTB)
    exp = np.concatenate(blocks)
    r = hip.Resampler(I, D, taps, AVX, complex_)
    before = hip.lib.sdrhip_debug_resample_cycle_launches()
    _both(r.run, to_dev(x), w, exp, 10001, f"{I}/{D}, {ntaps} taps ({tier})", out_block=OUTB)
    assert hip.lib.sdrhip_debug_resample_cycle_launches() == before + 3, "the thread-per-cycle kernel did not take every launch"


# ---- real filter (launch_fir_real8_fast): full == 128 / 64 -> k_filter_real_crossfix_lds, else the generic real fix-up -----
@pytest.mark.parametrize("sym,ntaps,tier", [(True, 64, "lds128"), (False, 64, "lds64"), (False, 40, "generic")])
def test_real_filter_tier(hip, oracle, sym, ntaps, tier):
    nblk = 5
    x = S.real_block(nblk * SEAM, seed=60 + ntaps)
    taps = S.gauss_taps(ntaps, 600 + ntaps + sym)
    model = PM.FilterModel(oracle, taps, AVX, sym=sym)
    blocks, _ = PM.fir_filter_pipe(model, _blocks(x, 1, nblk), OUTB)
    exp = np.concatenate(blocks)
    f = hip.Filter(taps, AVX, sym=sym)
    _both(f.run, to_dev(x), 1, exp, 10001, f"real filter, {ntaps} {'half-' if sym else ''}taps ({tier})")


# ---- complex filter: 128 taps at >= 16 384 outputs -> launch_filter_c4_tile (k_filter_cplx_crossfix_lds<128>);
#      40 taps -> launch_filter_cplx4_fast (the generic complex fix-up) ---------------------------------------------------------
@pytest.mark.parametrize("ntaps,nblk,cut", [(128, 10, 20418), (40, 5, 10002)])
def test_complex_filter_tier(hip, oracle, ntaps, nblk, cut):
    """(128 taps: ten blocks instead of five, so that BOTH launches of the cut run have the 16 384 outputs the tile kernel asks
    for -- 20 418 and 20 415 -- and take its fix-up, not the rolled kernel's.)"""
    x = S.cfloat_block(nblk * SEAM, seed=80 + ntaps)
    taps = S.gauss_taps(ntaps, 800 + ntaps)
    model = PM.FilterModel(oracle, taps, AVX, complex_=True)
    blocks, _ = PM.fir_filter_pipe(model, _blocks(x, 2, nblk), OUTB)
    exp = np.concatenate(blocks)
    K = exp.size // 2
    assert ntaps != 128 or (cut >= 16384 and K - cut >= 16384)
    f = hip.Filter(taps, AVX, complex_=True)
    _both(f.run, to_dev(x), 2, exp, cut, f"complex filter, {ntaps} taps")


# ---- complex decimator (launch_decimate_c4_fast), fix-up as a launch of its own (systolic kernel and short route off) --------
#   /8, 128 taps -> k_decimate_c_crossfix<.., 128>        /8, 52 taps -> k_decimate_c_crossfix<.., 52>
#   /8, 76 taps  -> the guarded 128-tap fix-up            /4, 128 taps and /8, 200 taps -> the generic complex fix-up
@pytest.mark.parametrize("u8", [False, True])
@pytest.mark.parametrize("factor,ntaps,tier", [(8, 128, "exact 128"), (8, 52, "exact 52"), (8, 76, "guarded"), (4, 128, "generic"),
                                               (8, 200, "generic")])
def test_complex_decimator_tier(hip, oracle, factor, ntaps, tier, u8):
    nblk = 5 * factor
    raw = S.iq_u8(nblk * SEAM, seed=90 + ntaps)
    x = oracle.convert_u8(raw) if u8 else S.cfloat_block(nblk * SEAM, seed=90 + ntaps)
    taps = S.gauss_taps(ntaps, 900 + factor + ntaps)
    model = PM.FilterModel(oracle, taps, AVX, complex_=True, factor=factor)
    blocks, _ = PM.fir_decimator_pipe(model, _blocks(x, 2, nblk), OUTB)
    exp = np.concatenate(blocks)
    d = hip.Decimator(factor, taps, AVX, complex_=True)
    assert d.num_coeffs == ntaps
    hip.lib.sdrhip_debug_set_systolic(0)
    try:
        before = hip.lib.sdrhip_debug_decimator_crossfix_launches()
        _both(d.run_u8 if u8 else d.run, to_dev(raw if u8 else x), 2, exp, 10002, f"complex /{factor}, {ntaps} taps ({tier}), u8 {u8}")
        assert hip.lib.sdrhip_debug_decimator_crossfix_launches() == before + 3, "one stand-alone fix-up launch per launch"
    finally:
        hip.lib.sdrhip_debug_set_systolic(2)


# ---- the two edges of "seams strictly inside the launch's window range": real 3/10, 191 taps (Lp 192, seam 3 * 4096 = 12288
#      upsampled positions; output m's window is [10 m, 10 m + 192)) ----------------------------------------------------------
#   4897: the window of output 4896 ends at 48960 + 192 = 49152 = 4 * 12288: the first launch's range ENDS on a seam multiple
#         (that seam has no straddler in it), the second launch owns every straddler of it
#   2439: 10 * 2438 + 192 = 24572 <= 24576 = 2 * 12288 < 24390 + 192: output 2439 is the FIRST straddler of seam 2, and the
#         first output of the second launch
@pytest.mark.parametrize("cut", [4897, 2439])
def test_launch_edges_of_the_seam_span(hip, oracle, cut):
    I, D = 3, 10
    nblk = 17
    x = S.real_block(nblk * SEAM, seed=33)
    taps = S.taps_resamp191()
    model = PM.ResamplerModel(oracle, I, D, taps, AVX, False)
    blocks, _ = PM.fir_resampler_pipe(model, _blocks(x, 1, nblk), OUTB)
    exp = np.concatenate(blocks)
    r = hip.Resampler(I, D, taps, AVX, False)
    Lp, seam_bi = 192, I * SEAM
    if cut == 4897:
        assert ((cut - 1) * D + Lp) % seam_bi == 0
    else:
        edge = 2 * seam_bi
        assert (cut - 1) * D + Lp <= edge < cut * D + Lp and cut * D < edge
    _both(r.run, to_dev(x), 1, exp, cut, "real 3/10, 191 taps", out_block=OUTB)
