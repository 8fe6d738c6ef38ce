"""GPU: the row forms of the FIR filter, decimator and resampler (sdrhip_filter_run_rows, sdrhip_decimator_run_rows,
sdrhip_resampler_run_rows).

For every case of tests/fir_rows_cases.py, on route 1 (banked), 2 (row by row) and 0 (auto), every row is held bit for bit to
  (a) the one-row device call on that row alone (existing code, pinned by the suites of the one-row operators), and
  (b) for the seamed three-row case of every family and the directed cases, the restated Pipe (oracle/pipes_model.py) on that
      row's stream, computed as tests/test_gpu_stream_slices.py computes its expected values: no device code in it.
The input rows hold exactly the inputs the header guarantees, NaN between and around them; the output buffer starts as NaN canaries
and every float outside the rows' outputs -- before, between and behind them -- is a canary afterwards.  Launch counters: a banked
call is one tile launch and one fix-up launch exactly when a seam lies inside the range, and none of the one-row lane-split
launches; the row-by-row route moves neither of the new counters.  tests/test_fir_rows_cases.py shows on the CPU what the table
reaches."""
import numpy as np
import pytest
import torch

import fir_rows_cases as RC
import gpu_util
import signals as S
import value_classes as VC
from conftest import assert_bit_equal
from test_gpu_rows import Rows

pytestmark = pytest.mark.gpu

ROUTES = (1, 2, 0)
_desc = {}


def desc_of(hip, f):
    if f.name not in _desc:
        _desc[f.name] = f.make(hip)
    return _desc[f.name]


def _kw(case):
    return {"out_block": case.out_block} if case.family.kind == "resampler" else {}


def counters(hip):
    return hip.fir_rows_launches(), hip.fir_rows_fixups(), int(hip.lib.sdrhip_debug_tiled_launches())


def row_inputs(case, g, xs):
    """Each row's guaranteed inputs, from its stream element in_base on."""
    w = case.family.width
    need = RC.need_inputs(case.family, g) * w
    return [x[g.in_base * w:g.in_base * w + need] for x in xs]


def run_rows(hip, case, g, xs, route, layout=None, cuts=None, what=""):
    """One rows call (or one per cut) over the near streams xs -> (output rows as float32 arrays, counter deltas)."""
    f = case.family
    w = f.width
    desc = desc_of(hip, f)
    ins = row_inputs(case, g, xs)
    gi, go, oi, oo = layout if layout is not None else case.layout_floats
    src = Rows(len(xs), ins[0].size, gi, oi, host=ins)
    dst = Rows(len(xs), g.n * w, go, oo)
    edges = [g.k_begin] + list(cuts or []) + [g.k_end]
    c0 = counters(hip)
    for a, b in zip(edges[:-1], edges[1:]):
        out = dst.view[:, (a - g.k_begin) * w:(b - g.k_begin) * w]
        desc.run_rows(src.view, out, g.T + a, g.T + b, in_base=g.in_base + g.S, seam_block=g.seam, route=route, **_kw(case))
    delta = tuple(y - x for x, y in zip(c0, counters(hip)))
    return dst.read(what), delta


def one_row_calls(hip, case, g, xs):
    """(a): the one-row device call on every row alone, from a buffer that holds that row's guaranteed inputs and NaN around them."""
    f = case.family
    w = f.width
    desc = desc_of(hip, f)
    ins = row_inputs(case, g, xs)
    src = Rows(len(xs), ins[0].size, 2, 0, host=ins)
    out = gpu_util.dev_empty_f32(len(xs) * g.n * w)
    for r in range(len(xs)):
        desc.run(src.view[r].data_ptr(), g.in_base + g.S, out.data_ptr() + 4 * r * g.n * w, g.T + g.k_begin, g.T + g.k_end, g.seam,
                 **_kw(case))
    return gpu_util.to_host(out).reshape(len(xs), g.n * w).copy()


PIPE_CASES = {c.name for c in RC.pipe_cases()}


@pytest.mark.parametrize("case", RC.CASES, ids=[c.name for c in RC.CASES])
def test_rows_against_the_one_row_call_and_the_restated_pipe(hip, oracle, case):
    f = case.family
    g = RC.resolve(hip, case, desc_of(hip, f))
    xs = [RC.row_stream(case, g, r) for r in range(case.rows)]
    exp = one_row_calls(hip, case, g, xs)
    if case.name in PIPE_CASES:
        for r in range(case.rows):
            assert_bit_equal(exp[r], RC.pipe_expected(case, g, oracle, xs[r]), f"{case.name}: the one-row call against the restated Pipe, row {r}")
    seamed = bool(RC.seams_inside(f, g.k_begin, g.k_end, g.seam))
    for route in ROUTES:
        what = f"{case.name}, route {route}"
        if route == 1 and not f.banked:
            ins = row_inputs(case, g, xs)
            src, f2 = Rows(case.rows, ins[0].size, 0, 0, host=ins), Rows(case.rows, g.n * f.width, 0, 0)
            with pytest.raises(hip.SdrHipError, match="route 1"):
                desc_of(hip, f).run_rows(src.view, f2.view, g.T + g.k_begin, g.T + g.k_end, in_base=g.in_base + g.S, seam_block=g.seam,
                                         route=1, **_kw(case))
            assert f2.untouched(), f"{what}: a refused call wrote"
            continue
        outs, (tiles, fixups, split) = run_rows(hip, case, g, xs, route, what=what)
        print(f"    {what}: plan {g.plan}, tile launches {tiles}, fix-up launches {fixups}, one-row lane-split launches {split}")
        if route == 1:
            assert (tiles, fixups) == (1, int(seamed)), f"{what}: {tiles} tile launches, {fixups} fix-up launches (a seam inside: {seamed})"
            assert split == 0, f"{what}: the banked route went through the one-row lane-split launcher"
        elif route == 2:
            assert (tiles, fixups) == (0, 0), f"{what}: the row-by-row route moved the banked counters"
        else:
            assert (tiles, fixups) in ((0, 0), (1, int(seamed))), what
            assert f.banked or tiles == 0, what
        for r in range(case.rows):
            assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the one-row call")


def _case(family, size, rows=None):
    for c in RC.CASES:
        if c.family.name == family and c.size == size and c.first < 0 and (rows is None or c.rows == rows):
            return c
    raise KeyError((family, size, rows))


NEIGHBOUR_CASES = [_case("cdec AVX /4, 64 taps", "3 tiles - 1"), _case("rres 3/10 AVX, the chain's taps", "3 tiles - 1"),
                   _case("rfilt AVX, 77 taps", "tile + 1")]


@pytest.mark.parametrize("case", NEIGHBOUR_CASES, ids=[c.name for c in NEIGHBOUR_CASES])
def test_a_neighbour_row_of_nan_and_inf_changes_nothing_in_the_others(hip, case):
    assert case.rows == 3 and case.seam_kind != "none"
    f = case.family
    g = RC.resolve(hip, case, desc_of(hip, f))
    xs = [RC.row_stream(case, g, r) for r in range(3)]
    clean, _ = run_rows(hip, case, g, xs, 1)
    bad = xs[1].copy()
    bad[0::3] = np.nan
    bad[1::7] = np.inf
    bad[2::11] = -np.inf
    salted = [xs[0], bad, xs[2]]
    exp_bad = one_row_calls(hip, case, g, salted)[1]
    assert np.isnan(exp_bad).any()
    for route in (1, 2):
        outs, _ = run_rows(hip, case, g, salted, route)
        for r in (0, 2):
            assert_bit_equal(outs[r], clean[r], f"{case.name}, route {route}: row {r} beside a row of NaN / Inf")
        VC.assert_same_classes(outs[1], exp_bad, f"{case.name}, route {route}: the NaN / Inf row against the one-row call", max_nan_share=1.0)


CUT_CASES = [_case(f.name, "tile + 1") for f in RC.FAMILIES if f.banked]


@pytest.mark.parametrize("case", CUT_CASES, ids=[c.name for c in CUT_CASES])
def test_a_range_cut_into_three_calls_at_odd_outputs_equals_the_single_call(hip, case):
    f = case.family
    g = RC.resolve(hip, case, desc_of(hip, f))
    xs = [RC.row_stream(case, g, r) for r in range(case.rows)]
    whole, _ = run_rows(hip, case, g, xs, 1)
    cuts = [g.k_begin + ((g.n // 3) | 1), g.k_begin + ((2 * g.n // 3) | 1)]
    assert g.k_begin < cuts[0] < cuts[1] < g.k_end and all((c - g.k_begin) % 2 == 1 for c in cuts)
    for route in (1, 2):
        parts, (tiles, fixups, _) = run_rows(hip, case, g, xs, route, cuts=cuts)
        if route == 1:
            assert tiles == 3 and fixups <= 3
        for r in range(case.rows):
            assert_bit_equal(parts[r], whole[r], f"{case.name}, route {route}: three calls cut at {cuts} against one, row {r}")


@pytest.mark.parametrize("side", ["input", "output"])
def test_rows_2_31_plus_6_floats_apart(hip, side):
    """Two rows whose bases are 2^31 + 6 floats apart on one side: the row offset is 64-bit arithmetic in the tile kernel and in
    the fix-up kernel (the range has seams inside)."""
    case = _case("rfilt AVX, 77 taps", "tile + 1")
    f = case.family
    g = RC.resolve(hip, case, desc_of(hip, f))
    xs = [RC.row_stream(case, g, r) for r in range(2)]
    ins = row_inputs(case, g, xs)
    exp = one_row_calls(hip, case, g, xs)
    far = (1 << 31) + 6
    need, n = ins[0].size, g.n
    in_stride, out_stride = (far, n) if side == "input" else (need, far)
    src = torch.empty(in_stride + need, dtype=torch.float32, device="cuda")
    dst = torch.empty(out_stride + n + 16, dtype=torch.float32, device="cuda")
    for r in range(2):
        src[r * in_stride:r * in_stride + need].copy_(torch.from_numpy(ins[r].copy()))
        dst[r * out_stride:r * out_stride + n + (16 if r else 0)].fill_(float("nan"))
    desc = desc_of(hip, f)
    for route in (1, 2):
        c0 = counters(hip)
        desc.run_rows(src.data_ptr(), dst.data_ptr(), g.T + g.k_begin, g.T + g.k_end, in_base=g.in_base + g.S, seam_block=g.seam,
                      route=route, in_stride=in_stride, out_stride=out_stride, rows=2, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        if route == 1:
            assert tuple(y - x for x, y in zip(c0, counters(hip))) == (1, 1, 0)
        for r in range(2):
            assert_bit_equal(dst[r * out_stride:r * out_stride + n].cpu().numpy(), exp[r], f"rows {far} floats apart on the {side} side, route {route}, row {r}")
        assert torch.isnan(dst[out_stride + n:]).all()
        dst[:n].fill_(float("nan"))
        dst[out_stride:out_stride + n].fill_(float("nan"))
    del src, dst
    torch.cuda.empty_cache()


def test_the_narrow_band_receiver_on_one_stream_without_synchronisation(hip, oracle):
    """TunerBank.run -> Decimator.run_rows -> fm_demod_rows -> Resampler.run_rows -> Filter.run_rows for 3 channels, every stage
    enqueued on one stream with nothing in between, against the same stages run row by row with the one-row calls."""
    K = 3
    n0 = 16384
    x = gpu_util.to_dev(S.cfloat_block(n0, seed=4242))
    tables = [hip.tuner_shift_table(num, 16) for num in (1, -3, 5)]
    bank = hip.TunerBank(8, S.taps_decim127(), tables)
    dec = hip.Decimator(4, S.gauss_taps(64, 604), hip.ORDER_AVX, complex_=True)
    res = hip.Resampler(3, 10, S.taps_example_audio_resampler(), hip.ORDER_AVX)
    fil = hip.Filter(S.taps_example_audio_filter_half(), hip.ORDER_AVX, sym=True)
    n1 = (n0 - bank.num_coeffs) // 8 + 1
    n2 = (n1 - dec.num_coeffs) // 4 + 1
    n3 = 0
    while res.in_offset(n3) + res.num_coeffs // 3 <= n2:
        n3 += 1
    n4 = n3 - fil.num_coeffs + 1
    assert n4 > 64

    def buffers():
        return (gpu_util.dev_empty_f32(K * (2 * n1 + 6)).view(K, 2 * n1 + 6)[:, :2 * n1], gpu_util.dev_empty_f32(K * 2 * n2).view(K, 2 * n2),
                gpu_util.dev_empty_f32(K * n2).view(K, n2), gpu_util.dev_empty_f32(K * (n3 + 1)).view(K, n3 + 1)[:, :n3],
                gpu_util.dev_empty_f32(K * n4).view(K, n4))

    results = {}
    for route in (1, 0, "one-row calls"):
        y1, y2, y3, y4, y5 = buffers()
        c0 = counters(hip)
        bank.run(x.data_ptr(), 0, y1.data_ptr(), y1.stride(0), 0, n1)
        if route == "one-row calls":
            for r in range(K):
                dec.run(y1[r].data_ptr(), 0, y2[r].data_ptr(), 0, n2)
                hip.check(hip.lib.sdrhip_fm_demod_run(None, y2[r].data_ptr(), 0, y3[r].data_ptr(), 0, n2, 0.0, 0.0))
                res.run(y3[r].data_ptr(), 0, y4[r].data_ptr(), 0, n3)
                fil.run(y4[r].data_ptr(), 0, y5[r].data_ptr(), 0, n4)
        else:
            dec.run_rows(y1, y2, 0, n2, route=route)
            hip.fm_demod_rows(y2, out=y3)
            res.run_rows(y3, y4, 0, n3, route=route)
            fil.run_rows(y4, y5, 0, n4, route=route)
        delta = tuple(b - a for a, b in zip(c0, counters(hip)))
        if route == 1:
            assert delta == (3, 0, 0), f"three banked stages, contiguous streams: {delta}"
        results[route] = gpu_util.to_host(y5).copy()
    audio = results["one-row calls"]
    assert np.isfinite(audio).all() and np.abs(audio).max() > 0
    for route in (1, 0):
        for r in range(K):
            assert_bit_equal(results[route][r], audio[r], f"narrow-band receiver, route {route}, channel {r}")


# (family, rows, outputs per row, a seam inside, banked by the rule of sdr_hip.h)
AUTO_POINTS = [
    ("cdec AVX /4, 64 taps", 2, 128, False, True), ("cdec AVX /4, 64 taps", 2, 16384, False, True), ("cdec AVX /4, 64 taps", 7, 1024, True, False),
    ("cdec AVX /4, 64 taps", 8, 1025, True, True), ("cdec AVX /4, 64 taps", 1, 128, False, False), ("cdec AVX /4, 64 taps", 33, 1024, False, False),
    ("cdec AVX /4, 64 taps", 8, 127, False, False),
    ("rres 3/10 AVX, the chain's taps", 3, 5000, False, True), ("rres 3/10 AVX, the chain's taps", 3, 5000, True, False),
    ("rfilt sym SSE, the chain's audio taps", 2, 1024, False, True), ("rfilt sym SSE, the chain's audio taps", 7, 1025, False, False),
    ("rfilt sym SSE, the chain's audio taps", 8, 16384, False, True),
    # families and data types the sweep did not hold: row by row
    ("rdec AVX /5, 61 taps", 8, 1024, False, False), ("cfilt AVX, 45 taps", 8, 1024, False, False), ("cres 7/9 SSE, 100 taps", 8, 1024, False, False),
]


@pytest.mark.parametrize("name,rows,n,seamed,banked", AUTO_POINTS, ids=[f"{p[0]}: {p[1]} x {p[2]}{', seam' if p[3] else ''}" for p in AUTO_POINTS])
def test_auto_banks_inside_the_measured_part_of_the_sweep_only(hip, name, rows, n, seamed, banked):
    f = RC.BY_NAME[name]
    desc = desc_of(hip, f)
    w = f.width
    need = -(-((n - 1) * f.D) // f.I) + f.Lp // f.I
    seam = -(-(n * f.D) // f.I) if seamed else 0
    assert bool(RC.seams_inside(f, 0, n, seam)) == seamed
    x = gpu_util.to_dev(S.real_block(rows * need * w, seed=n + rows)).view(rows, need * w)
    outs = [gpu_util.dev_empty_f32(rows * n * w).view(rows, n * w) for _ in range(2)]
    kw = {"out_block": 0} if f.kind == "resampler" else {}
    c0 = counters(hip)
    desc.run_rows(x, outs[0], 0, n, seam_block=seam, route=0, **kw)
    tiles, fixups, _ = (b - a for a, b in zip(c0, counters(hip)))
    assert (tiles, fixups) == ((1, int(seamed)) if banked else (0, 0)), f"auto on {name}, {rows} rows x {n} outputs: {tiles} banked launches"
    desc.run_rows(x, outs[1], 0, n, seam_block=seam, route=2, **kw)
    assert_bit_equal(gpu_util.to_host(outs[0]), gpu_util.to_host(outs[1]), f"auto against row by row: {name}, {rows} x {n}")
