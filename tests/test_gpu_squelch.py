"""The squelch on the device (sdrhip_squelch_run, _run_rows) against tests/squelch_model.py: outputs bit for bit (NaN payloads
included), final states and gates exactly, levels bit for bit with NaN by position.  The expected values are the model's, never a
device run.  Every output sits between canaries (gpu_util.dev_empty_f32); the floats of an output buffer outside the rows'
[0, n_blocks * block_sig) are prefilled and checked; the detector and, out of place, the signal are checked to be unwritten.

The shapes are the smallest at which each path is taken: blocks around the 256-sample stretch of the level sum, block counts around
the 1024-block group of the gate, rows up to the 1024 the library admits, the three access widths on each of the three arrays."""
import threading

import numpy as np
import pytest

import gpu_util as G
import squelch_cases as SC
import squelch_model as SM

pytestmark = pytest.mark.gpu
F = np.float32
WG, LS = SC.WG, SC.LS
FILL = 0x7FC0BEEF                                  # what the gaps of an output buffer hold before a call
ERR_ARG = -1


@pytest.fixture(autouse=True)
def _auto_route(hip):
    hip.set_squelch_route(0)
    yield
    hip.set_squelch_route(0)


def _place(x, pad, off, fill=None):
    """rows x n floats -> (flat host buffer with the rows `n + pad` floats apart behind `off` floats, stride)"""
    rows, n = x.shape
    stride = n + pad
    h = np.zeros(off + rows * stride + 1, F)
    if fill is not None:
        h.view(np.uint32)[:] = fill
    for r in range(rows):
        h[off + r * stride: off + r * stride + n] = x[r]
    return h, stride


def _rows_of(h, rows, n, stride, off):
    return np.stack([h[off + r * stride: off + r * stride + n] for r in range(rows)]) if rows else np.zeros((0, n), F)


def _gaps_intact(h, rows, n, stride, off, what):
    gaps = np.ones(h.size, bool)
    for r in range(rows):
        gaps[off + r * stride: off + r * stride + n] = False
    assert (h.view(np.uint32)[gaps] == FILL).all(), f"{what}: floats outside the rows' range were written"


def run(hip, det, cplx, bd, sig, bs, pol, hang, states, nb, mode="out", det_pad=0, det_off=0, sig_pad=0, sig_off=0, out_pad=0, out_off=0,
        levels=True, gates=True, ws="auto", alias_final=True, stream=None):
    """One sdrhip_squelch_run_rows call -> dict(out, final, levels, gates), each a host array or None.
    mode: "out" (detector, signal and output apart), "inplace" (detector apart, d_out == d_in), "self" (d_det == d_in), "self_inplace"
    (all three the same), "detect" (no signal).  states: rows x 2 int32, or None for a null d_state."""
    import torch
    det = np.ascontiguousarray(det, F)
    rows = det.shape[0]
    c = 2 if cplx else 1
    n_det, n_sig = nb * bd * c, nb * bs
    self_det = mode in ("self", "self_inplace")
    if self_det:
        assert not cplx and sig is None
        sig = det
        width = max(n_det, n_sig)
        if det.shape[1] < width:
            det = sig = np.concatenate([det, np.zeros((rows, width - det.shape[1]), F)], 1)
    h_det, det_stride = _place(det, det_pad, det_off, FILL if mode == "self_inplace" else None)
    d_det = G.dev_empty_f32(h_det.size)
    d_det.copy_(torch.from_numpy(h_det))
    p_det = d_det.data_ptr() + 4 * det_off
    p_in = p_out = None
    in_stride = out_stride = 0
    d_in = d_out = None
    if mode == "self":
        d_in, p_in, in_stride = d_det, p_det, det_stride
    elif mode == "self_inplace":
        d_in = d_out = d_det
        p_in = p_out = p_det
        in_stride = out_stride = det_stride
        out_off = det_off
    elif mode != "detect":
        sig = np.ascontiguousarray(sig, F)[:, :n_sig]
        h_in, in_stride = _place(sig, sig_pad, sig_off, FILL if mode == "inplace" else None)
        d_in = G.dev_empty_f32(h_in.size)
        d_in.copy_(torch.from_numpy(h_in))
        p_in = d_in.data_ptr() + 4 * sig_off
        if mode == "inplace":
            d_out, p_out, out_stride, out_off = d_in, p_in, in_stride, sig_off
    if mode in ("out", "self"):
        out_stride = n_sig + out_pad
        d_out = G.dev_empty_f32(out_off + rows * out_stride + 1)
        d_out.view(torch.int32).fill_(FILL)
        p_out = d_out.data_ptr() + 4 * out_off
    d_state = G.dev_empty_f32(2 * rows).view(torch.int32)
    if states is not None:
        d_state.copy_(torch.from_numpy(np.ascontiguousarray(states, np.int32).reshape(-1)))
    d_final = d_state if (alias_final and states is not None) else G.dev_empty_f32(2 * rows).view(torch.int32)
    d_levels = G.dev_empty_f32(rows * nb) if levels else None
    d_gates = torch.full((rows * nb + 128,), 0xA5, dtype=torch.uint8, device="cuda") if gates else None
    need = hip.lib.sdrhip_squelch_rows_workspace_bytes(rows, nb)
    d_ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda") if ws == "auto" else None
    rc = hip.lib.sdrhip_squelch_run_rows(stream, p_det, det_stride, int(cplx), bd, p_in, in_stride, p_out, out_stride, bs, rows, nb,
                                         float(pol["open_level"]), float(pol["close_level"]), hang, pol["open_above"],
                                         d_state.data_ptr() if states is not None else None, d_final.data_ptr(),
                                         hip._dptr(d_levels) if levels else None,
                                         d_gates.data_ptr() if gates else None, d_ws.data_ptr() if d_ws is not None else None,
                                         need if d_ws is not None else 0)
    hip.check(rc, "sdrhip_squelch_run_rows")
    res = {"out": None, "final": G.to_host(d_final).copy().reshape(rows, 2), "levels": None, "gates": None}
    if mode != "detect":
        h_out = G.to_host(d_out)
        res["out"] = _rows_of(h_out, rows, n_sig, out_stride, out_off)
        _gaps_intact(h_out, rows, n_sig, out_stride, out_off, mode)
    if mode != "self_inplace":
        assert np.array_equal(G.to_host(d_det).view(np.uint32), h_det.view(np.uint32)), "the detector was written"
    if mode == "out":
        assert np.array_equal(G.to_host(d_in).view(np.uint32), h_in.view(np.uint32)), "the signal was written"
    if levels:
        res["levels"] = G.to_host(d_levels).copy().reshape(rows, nb)
    if gates:
        g = d_gates.cpu().numpy()
        assert (g[rows * nb:] == 0xA5).all(), "bytes behind the gates were written"
        res["gates"] = g[:rows * nb].reshape(rows, nb).copy()
    if d_ws is not None:
        assert (d_ws.cpu().numpy()[need:] == 0xA5).all(), "the 4096 bytes behind the reported workspace size were written"
    return res


def model(det, cplx, bd, sig, bs, pol, hang, states, nb):
    return SM.squelch(det, cplx, bd, sig, bs, hang=hang, states=states, n_blocks=nb, **pol)


def same(res, exp, what):
    out, final, lv, gates = exp
    if res["levels"] is not None:
        bad = np.argwhere(~SM.same_levels(res["levels"], lv))
        assert bad.size == 0, f"{what}: {len(bad)} levels differ; first at {tuple(bad[0])}: {res['levels'][tuple(bad[0])]!r} vs {lv[tuple(bad[0])]!r}"
    if res["gates"] is not None:
        bad = np.argwhere(res["gates"] != gates)
        assert bad.size == 0, f"{what}: {len(bad)} gates differ; first at {tuple(bad[0])}"
    assert np.array_equal(res["final"], final), f"{what}: final states {res['final'].tolist()} vs {final.tolist()}"
    if out is not None and res["out"] is not None:
        bad = np.argwhere(~SM.same_bits(res["out"], out))
        assert bad.size == 0, (f"{what}: {len(bad)} output floats differ; first at {tuple(bad[0])}: "
                               f"{res['out'].view(np.uint32)[tuple(bad[0])]:#x} vs {out.view(np.uint32)[tuple(bad[0])]:#x}")


def check(hip, rows, nb, bd, cplx, bs, pol=SC.ABOVE, hang=1, seed=1, states="seeded", route=0, what="", **kw):
    det = SC.detector(rows, nb, bd, cplx, seed)
    mode = kw.get("mode", "out")
    sig = None if mode in ("self", "self_inplace", "detect") else SC.signal(rows, nb * bs, seed + 1000)
    st = SC.states_array(rows, seed + 2000) if isinstance(states, str) else states
    msig = det[:, :nb * bs] if mode in ("self", "self_inplace") else sig
    if mode in ("self", "self_inplace") and det.shape[1] < nb * bs:
        msig = np.concatenate([det, np.zeros((rows, nb * bs - det.shape[1]), F)], 1)
    exp = model(det, cplx, bd, msig, bs, pol, hang, st, nb)
    hip.set_squelch_route(route)
    try:
        l0 = hip.squelch_launches()
        res = run(hip, det, cplx, bd, sig, bs, pol, hang, st, nb, **kw)
        launches = hip.squelch_launches() - l0
    finally:
        hip.set_squelch_route(0)
    same(res, exp, f"{what} rows {rows}, n_blocks {nb}, block_det {bd}{' complex' if cplx else ''}, block_sig {bs}, hang {hang}, "
                   f"route {route}, {kw}")
    return res, exp, launches


# ---- 1: the routes and their launches -----------------------------------------------------------------------------------------------
def test_each_route_and_the_launch_counter(hip):
    for mode, per_ls in (("out", 3), ("detect", 2), ("inplace", 3)):
        assert check(hip, 3, 65, 257, True, 5, route=WG, mode=mode)[2] == 1
        assert check(hip, 3, 65, 257, True, 5, route=LS, mode=mode)[2] == per_ls
        assert check(hip, 3, 65, 257, True, 5, route=0, mode=mode)[2] == 1
    # auto past either edge: LS with a workspace, the one WG launch without
    assert hip.squelch_plan(3, 1025, 4, False, 4) == (3, LS)
    assert check(hip, 3, 1025, 4, False, 4)[2] == 3 and check(hip, 3, 1025, 4, False, 4, ws=None)[2] == 1
    assert hip.squelch_plan(2, 64, 512, False, 513) == (3, LS)
    assert check(hip, 2, 64, 512, False, 513)[2] == 3 and check(hip, 2, 64, 512, False, 512)[2] == 1
    hip.set_squelch_route(LS)
    with pytest.raises(hip.SdrHipError, match="forced route"):
        run(hip, SC.detector(1, 4, 4, False, 1), False, 4, SC.signal(1, 16, 2), 4, SC.ABOVE, 1, None, 4, ws=None)


# ---- 2: block lengths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_every_block_det_around_the_stretch_of_256(hip, route, cplx):
    for bd in SC.BLOCK_DETS:
        check(hip, 2, 20, bd, cplx, 5 if bd != 5 else 7, route=route, seed=bd)
    # one block of a row: the width comes from the pointer alone
    check(hip, 1, 1, 4097, cplx, 3, route=route, det_off=1)


@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_every_block_sig(hip, route):
    for bs in SC.BLOCK_SIGS:
        check(hip, 3, 20, 3, True, bs, route=route, seed=bs, hang=3)
        check(hip, 3, 20, 12, False, bs, route=route, seed=bs, hang=0, pol=SC.BELOW)
    for bs in (2, 3, 4, 7, 8191, 8192, 8193):         # around the vector of four floats and the apply kernel's tile
        check(hip, 2, 5, 3, False, bs, route=route, seed=bs, states=np.array([[0, 0], [1, 0]], np.int32), out_off=1 if bs % 2 else 0)


# ---- 3: block counts, the last two across the group of 1024 ------------------------------------------------------------------------
@pytest.mark.parametrize("route,ws", [(WG, None), (LS, "auto"), (0, "auto"), (0, None)], ids=["WG", "LS", "auto", "auto-no-workspace"])
def test_every_block_count(hip, route, ws):
    for nb in SC.N_BLOCKS:
        res, exp, launches = check(hip, 3, nb, 4, False, 4, route=route, ws=ws, hang=3, seed=nb)
        if nb == 0:
            assert launches == 1 and np.array_equal(res["final"], [SM.clamp_state(s, 3) for s in SC.states_array(3, 2000)])
    for nb in (1025, 2049, 3000):
        check(hip, 2, nb, 3, True, 5, route=route, ws=ws, hang=1200, seed=nb, pol=SC.BELOW)
        check(hip, 2, nb, 6, False, 6, route=route, ws=ws, hang=2, seed=nb, mode="self_inplace")
        check(hip, 2, nb, 2, True, 3, route=route, ws=ws, hang=2, seed=nb, mode="inplace")


# ---- 4: rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_rows_up_to_the_most_the_library_admits(hip, route):
    for rows in (1, 3, 32):
        check(hip, rows, 40, 100, True, 25, route=route, seed=rows, hang=2)
    check(hip, 1024, 8, 4, False, 4, route=route, seed=5)
    check(hip, 1024, 8, 4, True, 4, route=route, seed=6, mode="inplace", pol=SC.BELOW)


# ---- 5: strides and bases: the three access widths on each array -------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_strides_and_bases_on_each_array(hip, route, cplx):
    nb, bd, bs = 20, 264, 12                          # rows that are multiples of four floats: the stride and the base decide the width
    pads = (0, 1, 2, 5) if not cplx else (0, 2, 4, 6)
    for which in ("det", "sig", "out"):
        for pad in pads if which == "det" else (0, 1, 2, 5):
            for off in (0, 1, 2):
                check(hip, 3, nb, bd, cplx, bs, route=route, seed=7, hang=1, **{which + "_pad": pad, which + "_off": off})
    check(hip, 3, nb, bd, cplx, bs, route=route, seed=8, det_pad=2, det_off=2, sig_pad=1, sig_off=3, out_pad=6, out_off=2)
    check(hip, 3, nb, bd, cplx, bs, route=route, seed=8, det_pad=4, det_off=0, sig_pad=5, sig_off=1, mode="inplace")
    if not cplx:
        for pad, off in ((0, 0), (1, 0), (2, 2), (5, 1)):
            check(hip, 3, nb, 12, False, 12, route=route, seed=9, det_pad=pad, det_off=off, mode="self_inplace")
            check(hip, 3, nb, 12, False, 12, route=route, seed=9, det_pad=pad, det_off=off, out_pad=1, out_off=off, mode="self")
        # blocks that are no multiple of four floats: the block length narrows the detector's width
        for bd2 in (6, 7):
            check(hip, 2, nb, bd2, False, 5, route=route, seed=10)


# ---- 6: polarities, hangs, every carried-in state ----------------------------------------------------------------------------------
@pytest.mark.parametrize("pol", list(SC.POLARITIES), ids=list(SC.POLARITIES))
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_polarities_hangs_and_every_carried_in_state(hip, route, pol):
    rows = len(SC.STATES_IN)
    states = np.array(SC.STATES_IN, np.int32)
    for hang in (0, 1, 3, SC.GATE_BLOCKS + 1, 1 << 30):
        check(hip, rows, SC.GATE_BLOCKS, 10, True, 4, pol=SC.POLARITIES[pol], hang=hang, states=states, route=route, seed=hang % 97)
        check(hip, rows, 2, 10, False, 4, pol=SC.POLARITIES[pol], hang=hang, states=states, route=route, seed=3)
    # a null d_state is {0, 0}
    res, exp, _ = check(hip, 3, SC.GATE_BLOCKS, 10, True, 4, pol=SC.POLARITIES[pol], hang=3, states=None, route=route)
    assert np.array_equal(exp[1], SM.squelch(SC.detector(3, SC.GATE_BLOCKS, 10, True, 1), True, 10, None, 4, hang=3,
                                             states=np.zeros((3, 2), np.int32), **SC.POLARITIES[pol])[1])


# ---- 7: [0, N) whole and cut into calls ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["out", "inplace", "self_inplace"])
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_consecutive_calls_with_the_state_handed_on_are_one_call(hip, route, mode):
    import torch
    rows, nb, bd, bs, hang = 3, SC.GATE_BLOCKS, 8, 8, 3
    cplx = mode != "self_inplace"
    c = 2 if cplx else 1
    det = SC.detector(rows, nb, bd, cplx, 21)
    sig = det if mode == "self_inplace" else SC.signal(rows, nb * bs, 22)
    st0 = SC.states_array(rows, 23)
    whole = SM.squelch(det, cplx, bd, sig, bs, hang=hang, states=st0, **SC.BELOW)
    hip.set_squelch_route(route)
    for cuts in ([0, nb], [0, 20, 50, nb], [0, 1, 2, 40, 41, nb]):
        d_det = G.to_dev(det)
        d_sig = d_det if mode == "self_inplace" else G.to_dev(sig)
        d_out = d_sig if mode != "out" else G.dev_empty_f32(rows * nb * bs)
        d_state = G.dev_empty_f32(2 * rows).view(torch.int32)
        d_state.copy_(torch.from_numpy(st0.reshape(-1)))
        d_lv, d_g = G.dev_empty_f32(rows * nb), torch.zeros(rows * nb, dtype=torch.uint8, device="cuda")
        need = hip.lib.sdrhip_squelch_rows_workspace_bytes(rows, nb)
        d_ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        lvs, gts = [], []
        for a, b in zip(cuts[:-1], cuts[1:]):
            hip.check(hip.lib.sdrhip_squelch_run_rows(None, d_det.data_ptr() + 4 * a * bd * c, nb * bd * c, int(cplx), bd,
                                                      d_sig.data_ptr() + 4 * a * bs, nb * bs, d_out.data_ptr() + 4 * a * bs, nb * bs, bs, rows, b - a,
                                                      SC.BELOW["open_level"], SC.BELOW["close_level"], hang, 0, d_state.data_ptr(), d_state.data_ptr(),
                                                      d_lv.data_ptr(), d_g.data_ptr(), d_ws.data_ptr(), need), "sdrhip_squelch_run_rows")
            lvs.append(G.to_host(d_lv)[:rows * (b - a)].copy().reshape(rows, b - a))
            gts.append(d_g.cpu().numpy()[:rows * (b - a)].reshape(rows, b - a))
        res = {"out": G.to_host(d_out).reshape(rows, nb * bs), "final": G.to_host(d_state).reshape(rows, 2), "levels": np.concatenate(lvs, 1),
               "gates": np.concatenate(gts, 1)}
        same(res, whole, f"{mode}, route {route}, cut at {cuts}")


# ---- 8: aliasing, detect-only, optional outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_self_detection_in_place_and_detect_only(hip, route):
    for pol in SC.POLARITIES.values():
        outs = {}
        for mode in ("self", "self_inplace"):
            outs[mode] = check(hip, 3, SC.GATE_BLOCKS, 16, False, 16, pol=pol, hang=2, route=route, seed=31, mode=mode)[0]
        assert SM.same_bits(outs["self"]["out"], outs["self_inplace"]["out"]).all()
        check(hip, 3, SC.GATE_BLOCKS, 16, False, 4, pol=pol, hang=2, route=route, seed=32, mode="self")     # a signal row shorter than its detector
        a = check(hip, 3, SC.GATE_BLOCKS, 16, True, 4, pol=pol, hang=2, route=route, seed=33, mode="inplace")[0]
        b = check(hip, 3, SC.GATE_BLOCKS, 16, True, 4, pol=pol, hang=2, route=route, seed=33, mode="out")[0]
        d = check(hip, 3, SC.GATE_BLOCKS, 16, True, 4, pol=pol, hang=2, route=route, seed=33, mode="detect")[0]
        assert SM.same_bits(a["out"], b["out"]).all() and np.array_equal(a["gates"], d["gates"]) and np.array_equal(b["final"], d["final"])
        assert d["out"] is None
        check(hip, 3, SC.GATE_BLOCKS, 16, True, -7, pol=pol, hang=2, route=route, seed=33, mode="detect")   # block_sig is ignored there


@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_levels_and_gates_are_optional_and_change_nothing(hip, route):
    outs = []
    for lv in (True, False):
        for g in (True, False):
            for mode in ("out", "detect"):
                outs.append((mode, check(hip, 3, 70, 300, True, 9, hang=1, route=route, seed=41, levels=lv, gates=g, mode=mode, alias_final=lv)[0]))
    ref = outs[0][1]
    for mode, o in outs:
        assert np.array_equal(o["final"], ref["final"])
        if mode == "out":
            assert SM.same_bits(o["out"], ref["out"]).all()


# ---- 9: the directed cases ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_threshold_equality_and_value_classes(hip, route):
    det, b, L = SC.equality_case()
    sig = SC.signal(1, 8 * 16, 51)
    up, down = np.nextafter(L, F(np.inf)), np.nextafter(L, F(-np.inf))
    hip.set_squelch_route(route)
    for open_level, close_level, above in ((L, 0.01, 1), (up, 0.01, 1), (down, 0.01, 1), (L, L, 0), (up, up, 0), (down, down, 0), (10.0, L, 1), (10.0, up, 1)):
        pol = dict(open_level=F(open_level), close_level=F(close_level), open_above=above)
        st = np.array([[1, 0]], np.int32) if open_level == 10.0 else np.zeros((1, 2), np.int32)
        res = run(hip, det, False, 256, sig, 16, pol, 0, st, 8)
        same(res, SM.squelch(det, False, 256, sig, 16, hang=0, states=st, **pol), f"equality case {pol}")
    det = SC.value_class_case()
    sig = SC.signal(1, 6 * 16, 52)
    for pol in SC.POLARITIES.values():
        res = run(hip, det, False, 256, sig, 16, pol, 0, None, 6)
        exp = SM.squelch(det, False, 256, sig, 16, hang=0, **pol)
        same(res, exp, f"value classes {pol}")
        lv = res["levels"][0]
        assert np.isnan(lv[1]) and np.isposinf(lv[2]) and lv[3].view(np.uint32) == 0 and 0 < lv[4] < np.finfo(F).tiny


# ---- 10: refusals leave everything as it was -----------------------------------------------------------------------------------------
def test_refusals_write_nothing(hip):
    import torch
    rows, nb, bd, bs = 2, 8, 16, 16
    d_det = G.to_dev(SC.detector(rows, nb, bd, False, 61))
    d_in = G.to_dev(SC.signal(rows, nb * bs, 62))
    d_out = G.dev_empty_f32(rows * nb * bs)
    d_out.view(torch.int32).fill_(FILL)
    d_state = G.dev_empty_f32(2 * rows).view(torch.int32)
    d_state.fill_(FILL)
    d_lv = G.dev_empty_f32(rows * nb)
    d_lv.view(torch.int32).fill_(FILL)
    d_g = torch.full((rows * nb,), 0xA5, dtype=torch.uint8, device="cuda")
    l0 = hip.squelch_launches()

    def call(**kw):
        a = dict(d_det=d_det.data_ptr(), det_stride=nb * bd, det_complex=0, block_det=bd, d_in=d_in.data_ptr(), in_stride=nb * bs,
                 d_out=d_out.data_ptr(), out_stride=nb * bs, block_sig=bs, rows=rows, n_blocks=nb, open_level=1.0, close_level=0.25, hang=1,
                 open_above=1, ws=None, ws_bytes=0)
        a.update(kw)
        return hip.lib.sdrhip_squelch_run_rows(None, a["d_det"], a["det_stride"], a["det_complex"], a["block_det"], a["d_in"], a["in_stride"], a["d_out"],
                                               a["out_stride"], a["block_sig"], a["rows"], a["n_blocks"], a["open_level"], a["close_level"], a["hang"],
                                               a["open_above"], d_state.data_ptr(), d_state.data_ptr(), d_lv.data_ptr(), d_g.data_ptr(), a["ws"],
                                               a["ws_bytes"])

    bad = [dict(rows=0), dict(rows=1025), dict(block_det=0), dict(block_sig=(1 << 20) + 1), dict(n_blocks=-1), dict(open_level=float("nan")),
           dict(close_level=-1.0), dict(open_level=0.1), dict(open_above=0), dict(hang=-1), dict(hang=(1 << 30) + 1), dict(open_above=2),
           dict(det_complex=2), dict(d_det=None), dict(d_in=None), dict(d_out=None), dict(det_stride=nb * bd - 1), dict(in_stride=nb * bs - 1),
           dict(out_stride=nb * bs - 1), dict(det_complex=1, det_stride=nb * bd + 1), dict(d_out=d_in.data_ptr(), out_stride=nb * bs + 4),
           dict(d_out=d_det.data_ptr()), dict(ws=d_g.data_ptr(), ws_bytes=8)]
    for kw in bad:
        assert call(**kw) == ERR_ARG and b"sdrhip_squelch_run_rows" in hip.lib.sdrhip_last_error(), kw
    hip.set_squelch_route(LS)
    assert call() == ERR_ARG
    hip.set_squelch_route(0)
    assert hip.squelch_launches() == l0
    assert (G.to_host(d_out).view(np.uint32) == FILL).all() and (G.to_host(d_state).view(np.uint32) == FILL).all()
    assert (G.to_host(d_lv).view(np.uint32) == FILL).all() and (d_g.cpu().numpy() == 0xA5).all()
    assert call() == 0 and hip.squelch_launches() == l0 + 1


# ---- 11: the one-row call and the binding ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", [WG, LS], ids=["WG", "LS"])
def test_the_one_row_call_and_the_binding(hip, route):
    import torch
    nb, bd, bs = SC.GATE_BLOCKS, 50, 10
    det = SC.detector(1, nb, bd, True, 71)
    sig = SC.signal(1, nb * bs, 72)
    hip.set_squelch_route(route)
    for state in SC.STATES_IN[:6]:
        exp = SM.squelch(det, True, bd, sig, bs, hang=2, states=np.array([state], np.int32), **SC.ABOVE)
        t_det = G.to_dev(det[0]).view(torch.complex64)
        out, fin, lv, g = hip.squelch_run(t_det, bd, G.to_dev(sig[0]), bs, 1.0, 0.25, 2, True, state=state, levels=True, gates=True)
        res = {"out": G.to_host(out)[None], "final": fin.cpu().numpy()[None], "levels": G.to_host(lv)[None], "gates": g.cpu().numpy()[None]}
        same(res, exp, f"sdrhip_squelch_run from {state}")
    # the rows binding on views: a complex detector bank, the signal a slice of a wider tensor, gated in place
    rows = 3
    det = SC.detector(rows, nb, bd, True, 73)
    sig = SC.signal(rows, nb * bs, 74)
    wide = torch.zeros((rows, nb * bs + 6), dtype=torch.float32, device="cuda")
    wide[:, 2:2 + nb * bs] = G.to_dev(sig)
    view = wide[:, 2:2 + nb * bs]
    exp = SM.squelch(det, True, bd, sig, bs, hang=2, **SC.ABOVE)
    out, fin, lv, g = hip.squelch_run_rows(G.to_dev(det).view(torch.complex64), bd, view, bs, 1.0, 0.25, 2, True, out=view, levels=True, gates=True)
    torch.cuda.synchronize()
    res = {"out": view.cpu().numpy(), "final": fin.cpu().numpy(), "levels": lv.cpu().numpy(), "gates": g.cpu().numpy()}
    same(res, exp, "squelch_run_rows in place on a view")
    assert (wide[:, :2] == 0).all() and (wide[:, 2 + nb * bs:] == 0).all()
    out, fin, lv, g = hip.squelch_run_rows(G.to_dev(det).view(torch.complex64), bd, None, 0, 1.0, 0.25, 2, True, gates=True)
    assert out is None and np.array_equal(g.cpu().numpy(), exp[3]) and np.array_equal(fin.cpu().numpy(), exp[1])


# ---- 12: two host threads ------------------------------------------------------------------------------------------------------------
def test_one_call_on_each_of_two_host_threads(hip):
    import torch
    jobs = []
    for k, (rows, nb, bd, cplx, bs) in enumerate(((3, 1500, 6, True, 4), (2, 700, 30, False, 30))):
        det = SC.detector(rows, nb, bd, cplx, 81 + k)
        sig = SC.signal(rows, nb * bs, 91 + k)
        st = SC.states_array(rows, 95 + k)
        jobs.append(dict(args=(det, cplx, bd, sig, bs, SC.ABOVE, 2, st, nb), exp=SM.squelch(det, cplx, bd, sig, bs, hang=2, states=st, **SC.ABOVE),
                         stream=torch.cuda.Stream(), res=None, err=None))

    def work(j):
        try:
            with torch.cuda.stream(j["stream"]):
                j["res"] = run(hip, *j["args"], stream=j["stream"].cuda_stream)
        except BaseException as e:      # noqa: B036 -- handed to the main thread
            j["err"] = e

    threads = [threading.Thread(target=work, args=(j,)) for j in jobs]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for k, j in enumerate(jobs):
        if j["err"] is not None:
            raise j["err"]
        same(j["res"], j["exp"], f"thread {k}")
