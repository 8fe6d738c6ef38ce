"""GPU: the audio tail over rows (sdrhip_audio_tail_run_rows).

For every launch of tests/audio_tail_cases.py, route 1 (the fused kernel), route 2 (the composition of the row forms, the
definition) and route 0 (auto) are held bit for bit, NaN by position, to the restated Pipes' composition (oracle/pipes_model.py:
firResampler(block) >-> firFilter(block) >-> (* gain) on that row's y stream) -- no device code in the expected values.  The y
rows hold exactly what the launch may read, NaN between and around them; the audio buffer starts as NaN canaries and every float
outside the rows' outputs is a canary afterwards.  Launch counters: a route-1 run is exactly one fused launch and no launch of the
row forms, a route-2 run the reverse.  tests/test_audio_tail_cases.py shows on the CPU what the table reaches."""
import threading

import numpy as np
import pytest
import torch

import audio_tail_cases as AC
import gpu_util
import signals as S
from conftest import assert_bit_equal
from test_gpu_rows import Rows

pytestmark = pytest.mark.gpu

_tails = {}


def tail_of(hip, block, gain=1.0):
    key = (block, float(np.float32(gain)))
    if key not in _tails:
        _tails[key] = hip.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), gain=gain, block=block)
    return _tails[key]


def counters(hip):
    return hip.audio_tail_launches(), hip.fir_rows_launches() + hip.fir_rows_fixups()


def workspace(tail, rows, n_y):
    return torch.full((max(tail.workspace_bytes(rows, n_y), 1),), 0xA5, dtype=torch.uint8, device="cuda")


def run(hip, tail, ys, q0, q1, route, exact=True, layout=(0, 0, 0, 0), cuts=(), far=False, what="", ws="auto"):
    """The launch (or one per cut) over the near streams ys (each from stream element 0) -> (audio rows, counter deltas).  exact: each
    run's buffer holds exactly its receptive field."""
    gy, ga, oy, oa = layout
    rows = len(ys)
    T, Sh = (AC.FAR_T, AC.FAR_S) if far else (0, 0)
    dst = Rows(rows, q1 - q0, ga, oa)
    tail.set_route(route)
    c0 = counters(hip)
    edges = [q0] + list(cuts) + [q1]
    keep = []
    for a, b in zip(edges[:-1], edges[1:]):
        lo, hi = (AC.first_input(a), AC.end_input(b - 1)) if exact else (0, ys[0].size)
        src = Rows(rows, hi - lo, gy, oy, host=[y[lo:hi] for y in ys])
        w = workspace(tail, rows, hi - lo) if ws == "auto" else ws
        tail.run_rows(src.view, dst.view[:, a - q0:b - q0], T + a, T + b, y_base=Sh + lo, n_y=hi - lo, workspace=w)
        keep.append((src, w))
    delta = tuple(y - x for x, y in zip(c0, counters(hip)))
    out = dst.read(what)
    tail.set_route(0)
    return out, delta


@pytest.mark.parametrize("case", AC.LAUNCHES, ids=[c.name for c in AC.LAUNCHES])
def test_routes_against_the_restated_pipes(hip, oracle, case):
    tail = tail_of(hip, case.block, case.gain)
    ys = [AC.y_row(r) for r in range(case.rows)]
    exp = [AC.expected(oracle, r, case.block, case.gain)[case.q0:case.q1] for r in range(case.rows)]
    assert all(np.isfinite(e).all() and np.abs(e).max() > 0 for e in exp)
    fits = AC.fused_fits(case.block)
    assert tail.fused_fits() == fits
    runs = len(case.cuts) + 1
    for route in (1, 2, 0):
        what = f"{case.name}, route {route}"
        if route == 1 and not fits:
            tail.set_route(1)
            src, dst = Rows(case.rows, AC.N_Y, 0, 0, host=ys), Rows(case.rows, case.q1 - case.q0, 0, 0)
            with pytest.raises(hip.SdrHipError, match="route 1"):
                tail.run_rows(src.view, dst.view, case.q0, case.q1)
            tail.set_route(0)
            assert dst.untouched(), f"{what}: a refused call wrote"
            continue
        outs, (fused, rows_launches) = run(hip, tail, ys, case.q0, case.q1, route, case.exact, case.layout, case.cuts, case.far, what)
        print(f"    {what}: fused launches {fused}, row-form launches {rows_launches}")
        if route == 1:
            assert (fused, rows_launches) == (runs, 0), what
        elif route == 2:
            assert fused == 0 and rows_launches >= 2 * runs, what
        else:
            assert 0 <= fused <= runs and (rows_launches == 0) == (fused == runs), what      # every run is one or the other
            assert fits or fused == 0, what
        for r in range(case.rows):
            assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the restated Pipes")


def _salted(kind):
    y = AC.y_row(0, seed=5).copy()
    if kind == "nan":
        y[:] = np.nan
    elif kind == "inf and nan samples":
        y[100::997] = np.inf
        y[350::1499] = -np.inf
        y[7000::2003] = np.nan
    elif kind == "zeros":
        y[:] = 0.0
    elif kind == "negative zeros":
        y[:] = -0.0
    return y


def test_rows_between_nan_rows_value_classes_and_silent_rows(hip, oracle):
    tail = tail_of(hip, 8192, -0.5)
    kinds = ["nan", "plain", "nan", "inf and nan samples", "zeros", "negative zeros", "nan"]
    ys = [AC.y_row(1) if k == "plain" else _salted(k) for k in kinds]
    q0, q1 = 1900, 8300
    exp = [AC.expected_from(oracle, y, 8192, -0.5)[q0:q1] for y in ys]
    assert np.isnan(exp[3]).any() and not np.isnan(exp[3]).all() and np.isfinite(exp[1]).all()
    assert (exp[4].view(np.uint32) << 1 == 0).all() and (exp[5].view(np.uint32) << 1 == 0).all()
    for route in (1, 2):
        outs, _ = run(hip, tail, ys, q0, q1, route, what=f"value classes, route {route}")
        for r, k in enumerate(kinds):
            if k == "nan":
                assert np.isnan(outs[r]).all(), f"route {route}: row {r}"
            else:
                nan = np.isnan(exp[r])
                assert (np.isnan(outs[r]) == nan).all(), f"route {route}: NaN by position, row {r} ({k})"
                assert_bit_equal(np.where(nan, 0, outs[r]), np.where(nan, 0, exp[r]), f"route {route}: row {r} ({k}) beside NaN rows")


def test_another_shape_goes_through_the_composition_only(hip, oracle):
    """2/3 with 31 taps in the SSE order and 8 half-taps: routes 2 and 0 against the one-row operators, route 1 refused."""
    rt, ah = S.taps_resamp31(), S.taps_audio_half32()[:8]
    block = 500
    tail = hip.AudioTail(2, 3, rt, ah, gain=0.25, block=block, order=hip.ORDER_SSE)
    res, fil = hip.Resampler(2, 3, rt, hip.ORDER_SSE), hip.Filter(ah, hip.ORDER_SSE, sym=True)
    n_y = 4000
    q1 = tail.ready(n_y)
    assert q1 > 2 * block and not tail.fused_fits()
    ys = [S.real_block(n_y, seed=77 + r) for r in range(3)]
    exp = []
    for y in ys:
        d_y, d_z, d_a = gpu_util.to_dev(y), gpu_util.dev_empty_f32(q1 + 15), gpu_util.dev_empty_f32(q1)
        res.run(d_y.data_ptr(), 0, d_z.data_ptr(), 0, q1 + 15, block, out_block=block)
        fil.run(d_z.data_ptr(), 0, d_a.data_ptr(), 0, q1, block)
        hip.check(hip.lib.sdrhip_scale_run(None, 0.25, d_a.data_ptr(), d_a.data_ptr(), q1))
        exp.append(gpu_util.to_host(d_a).copy())
    src = Rows(3, n_y, 3, 1, host=ys)
    for route in (2, 0):
        dst = Rows(3, q1, 1, 2)
        tail.set_route(route)
        c0 = counters(hip)
        tail.run_rows(src.view, dst.view, 0, q1, workspace=workspace(tail, 3, n_y))
        assert counters(hip)[0] == c0[0]
        outs = dst.read()
        for r in range(3):
            assert_bit_equal(outs[r], exp[r], f"2/3 SSE tail, route {route}, row {r}")
    tail.set_route(1)
    dst = Rows(3, q1, 0, 0)
    with pytest.raises(hip.SdrHipError, match="route 1"):
        tail.run_rows(src.view, dst.view, 0, q1)
    assert dst.untouched()


def test_workspaces_null_on_route_1_and_a_byte_short_on_route_2(hip, oracle):
    tail = tail_of(hip, 8192)
    ys = [AC.y_row(r) for r in range(3)]
    exp = [AC.expected(oracle, r, 8192)[:2500] for r in range(3)]
    outs, delta = run(hip, tail, ys, 0, 2500, 1, ws=None, what="route 1, null workspace")
    assert delta == (1, 0)
    for r in range(3):
        assert_bit_equal(outs[r], exp[r], f"route 1 without a workspace, row {r}")
    n_y = AC.end_input(2499)
    short = torch.empty(tail.workspace_bytes(3, n_y) - 1, dtype=torch.uint8, device="cuda")
    src, dst = Rows(3, n_y, 0, 0, host=[y[:n_y] for y in ys]), Rows(3, 2500, 0, 0)
    for route in (2, 0):
        tail.set_route(route)
        c0 = counters(hip)
        with pytest.raises(hip.SdrHipError, match="workspace"):
            tail.run_rows(src.view, dst.view, 0, 2500, workspace=short)
        with pytest.raises(hip.SdrHipError, match="workspace"):
            tail.run_rows(src.view, dst.view, 0, 2500, workspace=None)
        assert counters(hip) == c0 and dst.untouched()
    tail.set_route(0)


def test_one_descriptor_on_two_host_threads(hip, oracle):
    tail = hip.AudioTail(3, 10, AC.resamp_taps(), AC.audio_half(), gain=1.0, block=8192)     # a first-ever run on both threads
    tail.set_route(1)
    ys = [AC.y_row(r) for r in range(2)]
    exp = [AC.expected(oracle, r, 8192)[:AC.Q_MAX] for r in range(2)]
    src = [Rows(1, AC.N_Y, 0, 0, host=[ys[r]]) for r in range(2)]
    dst = [Rows(1, AC.Q_MAX, 0, 0) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    errors = []
    torch.cuda.synchronize()

    def work(j):
        try:
            for _ in range(20):
                tail.run_rows(src[j].view, dst[j].view, 0, AC.Q_MAX, stream=streams[j].cuda_stream)
        except Exception as e:                                                                # noqa: BLE001
            errors.append(e)
    c0 = counters(hip)
    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    torch.cuda.synchronize()
    assert not errors, errors
    assert counters(hip)[0] - c0[0] == 40
    for r in range(2):
        assert_bit_equal(dst[r].read()[0], exp[r], f"thread {r}")


# (rows, outputs per row, block, row layout, route 1 by the rule of sdr_hip.h).  Layouts as tools/audio_tail_bench.py measured them:
# "rows" = both sides back to back; "y-strided" = the audio Pipes' padded y rows, 4 bytes past a 16-byte boundary; "a-strided" = the
# audio rows apart as well.
AUTO_POINTS = [
    (1, 153, 0, "rows", True), (1, 152, 0, "rows", False), (32, 153, 8192, "rows", True), (33, 153, 0, "rows", False),
    (2, 314574, 0, "rows", True), (2, 314575, 0, "rows", False), (5, 5000, AC.MIN_BLOCK, "rows", True), (8, 2458, 1024, "rows", False),
    (3, 153, 8192, "y-strided", True), (32, 2458, 0, "y-strided", True), (3, 152, 8192, "y-strided", False), (33, 2458, 0, "y-strided", False),
    (2, 153, 0, "a-strided", True), (8, 39322, 8192, "a-strided", True), (8, 39322, 1024, "a-strided", False),
]


@pytest.mark.parametrize("rows,n,block,layout,fused", AUTO_POINTS, ids=[f"{p[0]} x {p[1]}, block {p[2]}, {p[3]}" for p in AUTO_POINTS])
def test_auto_takes_the_fused_kernel_inside_the_measured_part_of_the_sweep_only(hip, rows, n, block, layout, fused):
    tail = tail_of(hip, block)
    n_y = AC.end_input(n - 1)
    ys = n_y if layout == "rows" else n_y + n_y // 4 + 513
    os_ = n + 5 if layout == "a-strided" else n
    off = 0 if layout == "rows" else 1
    y = gpu_util.to_dev(S.real_block(off + rows * ys, seed=n + rows))[off:].as_strided((rows, n_y), (ys, 1))
    outs = [gpu_util.dev_empty_f32(rows * os_).as_strided((rows, n), (os_, 1)) for _ in range(2)]
    ws = workspace(tail, rows, n_y)
    tail.set_route(0)
    c0 = counters(hip)
    tail.run_rows(y, outs[0], 0, n, workspace=ws)
    got = counters(hip)[0] - c0[0]
    assert got == int(fused), f"auto on {rows} rows x {n} outputs, block {block}, {layout}: {got} fused launches"
    tail.set_route(2)
    tail.run_rows(y, outs[1], 0, n, workspace=ws)
    assert counters(hip)[0] - c0[0] == got
    tail.set_route(0)
    torch.cuda.synchronize()
    assert_bit_equal(outs[0].cpu().numpy().ravel(), outs[1].cpu().numpy().ravel(), f"auto against the composition: {rows} x {n}, {layout}")
