"""GPU: the audio tail over rows on the general fused kernel (k_audio_tail_rows_any; sdrhip_audio_tail_set_general).

For every launch of tests/audio_tail_any_cases.py -- nine down-sampling shapes with 64, 32 and 8 half-taps, blocks 0, 200, 250, 256,
1000 and the lowest block the predicate admits -- route 0 with mode 1 is held bit for bit, NaN by position, to the restated Pipes'
composition (oracle/pipes_model.py: firResampler(block) >-> firFilter(block) >-> (* gain) on that row's y stream): no device code
in the expected values.  The one block of this table at which the reference's Pipe asserts (8/9 x 511 at block 64) is held route
against route; over the family the reference asserts on a zone of blocks above the lowest one, not on one block
(tests/tail_any_family_cases.py states the rule, tests/test_gpu_tail_any_family.py runs the family).
The y rows hold exactly what the launch may read, NaN between and around them; the audio buffer starts as canaries and every float
outside the rows' outputs is a canary afterwards.  Launch counters: a mode-1 run is exactly one launch of the general kernel, none
of k_audio_tail_rows and none of the row forms; mode 2 and route 2 the reverse.  tests/test_audio_tail_any_cases.py shows on the CPU
what the table reaches."""
import threading

import numpy as np
import pytest
import torch

import audio_tail_any_cases as AC
import audio_tail_cases as FM
import gpu_util
import signals as S
from conftest import assert_bit_equal
from test_audio_tail_any_cases import ASSERTING
from test_gpu_rows import Rows

pytestmark = pytest.mark.gpu

_tails = {}


def tail_of(hip, shape, block, gain=1.0):
    key = (shape.name, block, float(np.float32(gain)))
    if key not in _tails:
        _tails[key] = hip.AudioTail(shape.I, shape.D, shape.resamp_taps(), shape.audio_half(), gain=gain, block=block)
    return _tails[key]


def counters(hip):
    """(general kernel, k_audio_tail_rows, row forms)"""
    return hip.audio_tail_general_launches(), hip.audio_tail_launches(), hip.fir_rows_launches() + hip.fir_rows_fixups()


def workspace(tail, rows, n_y):
    return torch.full((max(tail.workspace_bytes(rows, n_y), 1),), 0xA5, dtype=torch.uint8, device="cuda")


def run(hip, tail, shape, ys, q0, q1, mode, route=0, exact=True, layout=(0, 0, 0, 0), cuts=(), shift=(0, 0), what=""):
    """The launch (or one per cut) over the near streams ys (each from stream element 0) -> (audio rows, counter deltas).  exact: each
    run's buffer holds exactly its receptive field."""
    gy, ga, oy, oa = layout
    rows = len(ys)
    T, Sh = shift
    dst = Rows(rows, q1 - q0, ga, oa)
    tail.set_route(route)
    tail.set_general(mode)
    c0 = counters(hip)
    edges = [q0] + list(cuts) + [q1]
    keep = []
    for a, b in zip(edges[:-1], edges[1:]):
        lo, hi = (shape.first_input(a), shape.end_input(b - 1)) if exact else (0, ys[0].size)
        src = Rows(rows, hi - lo, gy, oy, host=[y[lo:hi] for y in ys])
        w = workspace(tail, rows, hi - lo)
        tail.run_rows(src.view, dst.view[:, a - q0:b - q0], T + a, T + b, y_base=Sh + lo, n_y=hi - lo, workspace=w)
        keep.append((src, w))
    delta = tuple(y - x for x, y in zip(c0, counters(hip)))
    out = dst.read(what)
    tail.set_route(0)
    tail.set_general(0)
    return out, delta


@pytest.mark.parametrize("case", AC.LAUNCHES, ids=[c.name for c in AC.LAUNCHES])
def test_mode_1_against_the_restated_pipes(hip, oracle, case):
    s = case.shape
    tail = tail_of(hip, s, case.block, case.gain)
    assert tail.general_fits() and AC.general_fits(s, case.block)
    ys = [AC.y_row(s, r) for r in range(case.rows)]
    runs = len(case.cuts) + 1
    what = f"{case.name}, block {case.block}, mode 1"
    outs, delta = run(hip, tail, s, ys, case.q0, case.q1, 1, 0, case.exact, case.layout, case.cuts, case.far_shift, what)
    print(f"    {what}: launches (general, k_audio_tail_rows, row forms) {delta}")
    assert delta == (runs, 0, 0), what
    if (s.name, case.block) in ASSERTING or case.seamed and not case.cuts and not case.far:
        # mode 2 inside route 0 and route 2 itself: the composition, the general counter still
        for mode, route in ((2, 0), (1, 2)):
            comp, d2 = run(hip, tail, s, ys, case.q0, case.q1, mode, route, case.exact, case.layout, case.cuts, case.far_shift, what)
            assert d2[0] == 0 and d2[1] == 0 and d2[2] >= 2 * runs, f"{what}: mode {mode}, route {route}: {d2}"
            for r in range(case.rows):
                assert_bit_equal(outs[r], comp[r], f"{what}, row {r} against mode {mode} on route {route}")
    if (s.name, case.block) in ASSERTING:
        return                                               # the reference's Pipe is not defined here: route against route only
    exp = [AC.expected(oracle, s, r, case.block, case.gain)[case.q0:case.q1] for r in range(case.rows)]
    assert all(np.isfinite(e).all() for e in exp) and (case.q1 - case.q0 < 8 or all(np.abs(e).max() > 0 for e in exp))
    for r in range(case.rows):
        assert_bit_equal(outs[r], exp[r], f"{what}, row {r} against the restated Pipes")


def _salted(shape, kind):
    y = AC.y_row(shape, 0, seed=5).copy()
    if kind == "nan":
        y[:] = np.nan
    elif kind == "inf and nan samples":
        y[100::397] = np.inf
        y[350::499] = -np.inf
        y[1700::503] = np.nan
    elif kind == "zeros":
        y[:] = 0.0
    elif kind == "negative zeros":
        y[:] = -0.0
    return y


@pytest.mark.parametrize("name", ["4/5 x 63", "7/8 x 255"])
def test_rows_between_nan_rows_value_classes_and_silent_rows(hip, oracle, name):
    s = AC.SHAPES[name]
    tail = tail_of(hip, s, 200, -0.5)
    kinds = ["nan", "plain", "nan", "inf and nan samples", "zeros", "negative zeros", "nan"]
    ys = [AC.y_row(s, 1) if k == "plain" else _salted(s, k) for k in kinds]
    q0, q1 = 300, AC.Q_MAX
    exp = [AC.expected_from(oracle, s, y, 200, -0.5)[q0:q1] for y in ys]
    assert np.isnan(exp[3]).any() and not np.isnan(exp[3]).all() and np.isfinite(exp[1]).all()
    assert (exp[4].view(np.uint32) << 1 == 0).all() and (exp[5].view(np.uint32) << 1 == 0).all()
    outs, delta = run(hip, tail, s, ys, q0, q1, 1, what="value classes")
    assert delta == (1, 0, 0)
    for r, k in enumerate(kinds):
        if k == "nan":
            assert np.isnan(outs[r]).all(), f"row {r}"
        else:
            nan = np.isnan(exp[r])
            assert (np.isnan(outs[r]) == nan).all(), f"NaN by position, row {r} ({k})"
            assert_bit_equal(np.where(nan, 0, outs[r]), np.where(nan, 0, exp[r]), f"row {r} ({k}) beside NaN rows")


def test_the_fm_shape_on_both_kernels_at_block_8192(hip, oracle):
    """Route 1 is k_audio_tail_rows; route 0 with mode 1 reaches the general kernel where route 1's own rule does not take the run
    (33 rows lie outside its sweep): the same bits, and the restated Pipes'."""
    tail = hip.AudioTail(3, 10, FM.resamp_taps(), FM.audio_half(), gain=0.5, block=8192)
    assert tail.fused_fits() and tail.general_fits()
    rows = 33
    ys = [FM.y_row(r % 3) for r in range(rows)]
    exp = [FM.expected(oracle, r, 8192, 0.5)[:FM.Q_MAX] for r in range(3)]
    src = Rows(rows, FM.N_Y, 1, 1, host=ys)
    outs = {}
    for key, route, mode in (("k_audio_tail_rows", 1, 2), ("general", 0, 1), ("auto", 0, 0), ("composed", 0, 2)):
        dst = Rows(rows, FM.Q_MAX, 0, 0)
        tail.set_route(route)
        tail.set_general(mode)
        c0 = counters(hip)
        tail.run_rows(src.view, dst.view, 0, FM.Q_MAX, workspace=workspace(tail, rows, FM.N_Y))
        d = tuple(y - x for x, y in zip(c0, counters(hip)))
        assert (d[0], d[1]) == {"k_audio_tail_rows": (0, 1), "general": (1, 0), "auto": (0, 0), "composed": (0, 0)}[key], (key, d)
        outs[key] = dst.read(key)
    tail.set_route(0)
    tail.set_general(0)
    for key, o in outs.items():
        for r in range(rows):
            assert_bit_equal(o[r], exp[r % 3], f"FM shape, {key}, row {r}")


def test_mode_0_on_the_fm_shape_never_takes_the_general_kernel(hip):
    for block, rows, n in ((1024, 3, 2500), (1000, 1, 2500), (8192, 33, 300), (0, 2, 100), (256, 8, 204), (0, 1, 51)):
        tail = hip.AudioTail(3, 10, FM.resamp_taps(), FM.audio_half(), gain=1.0, block=block)
        assert tail.general_fits()
        n_y = FM.end_input(n - 1)
        y = gpu_util.to_dev(S.real_block(rows * n_y, seed=n)).view(rows, n_y)
        out = gpu_util.dev_empty_f32(rows * n).view(rows, n)
        c0 = counters(hip)
        tail.run_rows(y, out, 0, n, workspace=workspace(tail, rows, n_y))
        assert counters(hip)[0] == c0[0], f"block {block}, {rows} rows x {n}"
    torch.cuda.synchronize()


# (shape, rows, outputs per row, block, row layout, the general kernel by the shipped table).  The sweep (tools/audio_tail_any_bench.py,
# profiles/audio_tail_any_bench.txt) found the general kernel ahead at every point: inside it -- the two swept tails, 1 .. 32 rows of
# 51 .. 52428 outputs, any block -- mode 0 is the general kernel in every layout, outside it the composition.
AUTO_POINTS = [
    ("4/5 x 63", 1, 51, 0, "rows", True), ("4/5 x 63", 1, 50, 0, "rows", False), ("4/5 x 63", 32, 52428, 256, "rows", True),
    ("4/5 x 63", 33, 204, 0, "rows", False), ("2/5 x 127", 2, 52428, 0, "rows", True), ("2/5 x 127", 2, 52429, 0, "rows", False),
    ("2/5 x 127", 8, 3276, 256, "y-strided", True), ("2/5 x 127", 5, 1000, 200, "y-strided", True), ("2/5 x 127", 33, 1000, 200, "y-strided", False),
    ("4/5 x 63", 2, 204, 256, "a-strided", True), ("4/5 x 63", 32, 50, 256, "a-strided", False), ("3/5 x 71", 2, 204, 256, "rows", False),
]


@pytest.mark.parametrize("name,rows,n,block,layout,general", AUTO_POINTS, ids=[f"{p[0]}, {p[1]} x {p[2]}, block {p[3]}, {p[4]}" for p in AUTO_POINTS])
def test_mode_0_follows_the_shipped_table(hip, name, rows, n, block, layout, general):
    s = AC.SHAPES[name]
    tail = hip.AudioTail(s.I, s.D, s.resamp_taps(), S.taps_audio_half64(), gain=1.0, block=block)
    assert tail.general_fits()
    n_y = -(-(n + 127) * s.D // s.I) + s.nloop
    assert tail.ready(n_y) >= n
    ys = n_y if layout == "rows" else n_y + n_y // 4 + 513
    os_ = n + 5 if layout == "a-strided" else n
    off = 0 if layout == "rows" else 1
    y = gpu_util.to_dev(S.real_block(off + rows * ys, seed=n + rows))[off:].as_strided((rows, n_y), (ys, 1))
    outs = [gpu_util.dev_empty_f32(rows * os_).as_strided((rows, n), (os_, 1)) for _ in range(3)]
    ws = workspace(tail, rows, n_y)
    got = []
    for k, mode in enumerate((0, 1, 2)):
        tail.set_general(mode)
        c0 = counters(hip)
        tail.run_rows(y, outs[k], 0, n, workspace=ws)
        got.append(counters(hip)[0] - c0[0])
    tail.set_general(0)
    assert got == [int(general), 1, 0], f"{name}: {rows} rows x {n} outputs, block {block}, {layout}: general launches by mode {got}"
    torch.cuda.synchronize()
    for k in (1, 2):
        assert_bit_equal(outs[0].cpu().numpy().ravel(), outs[k].cpu().numpy().ravel(), f"mode 0 against mode {k}: {name}, {rows} x {n}, {layout}")


def test_refusals_leave_the_canaries(hip):
    s = AC.SHAPES["3/5 x 71"]
    tail = tail_of(hip, s, 250)
    ys = [AC.y_row(s, r) for r in range(3)]
    src, dst = Rows(3, s.n_y, 0, 0, host=ys), Rows(3, AC.Q_MAX, 0, 0)
    tail.set_general(1)
    c0 = counters(hip)
    tail.set_route(1)
    with pytest.raises(hip.SdrHipError, match="route 1"):
        tail.run_rows(src.view, dst.view, 0, AC.Q_MAX, workspace=workspace(tail, 3, s.n_y))
    tail.set_route(0)
    short = torch.empty(tail.workspace_bytes(3, s.n_y) - 1, dtype=torch.uint8, device="cuda")
    for ws in (short, None):
        with pytest.raises(hip.SdrHipError, match="sdrhip_audio_tail_run_rows"):
            tail.run_rows(src.view, dst.view, 0, AC.Q_MAX, workspace=ws)
    with pytest.raises(hip.SdrHipError, match="sdrhip_audio_tail_run_rows"):           # a receptive field one sample behind the rows
        tail.run_rows(src.view, dst.view, 0, AC.Q_MAX, n_y=s.n_y - 1, workspace=workspace(tail, 3, s.n_y))
    with pytest.raises(hip.SdrHipError, match="sdrhip_audio_tail_run_rows"):           # ... or one in front of them
        tail.run_rows(src.view, dst.view[:, 5:], 5, AC.Q_MAX, y_base=s.first_input(5) + 1, workspace=workspace(tail, 3, s.n_y))
    with pytest.raises(hip.SdrHipError, match="sdrhip_audio_tail_set_general"):
        tail.set_general(3)
    assert counters(hip) == c0 and dst.untouched()
    tail.set_general(0)


def test_one_descriptor_on_two_host_threads(hip, oracle):
    s = AC.SHAPES["2/5 x 127"]
    tail = hip.AudioTail(s.I, s.D, s.resamp_taps(), s.audio_half(), gain=1.0, block=256)      # a first-ever run on both threads
    tail.set_general(1)
    ys = [AC.y_row(s, r) for r in range(2)]
    exp = [AC.expected(oracle, s, r, 256)[:AC.Q_MAX] for r in range(2)]
    src = [Rows(1, s.n_y, 0, 0, host=[ys[r]]) for r in range(2)]
    dst = [Rows(1, AC.Q_MAX, 0, 0) for _ in range(2)]
    ws = [workspace(tail, 1, s.n_y) for _ in range(2)]
    streams = [torch.cuda.Stream() for _ in range(2)]
    errors = []
    torch.cuda.synchronize()

    def work(j):
        try:
            for _ in range(20):
                tail.run_rows(src[j].view, dst[j].view, 0, AC.Q_MAX, stream=streams[j].cuda_stream, workspace=ws[j])
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
    assert counters(hip)[0] - c0[0] == 40 and counters(hip)[1:] == c0[1:]
    for r in range(2):
        assert_bit_equal(dst[r].read()[0], exp[r], f"thread {r}")
