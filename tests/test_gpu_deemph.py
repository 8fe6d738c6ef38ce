"""De-emphasis on the device (sdrhip_deemph_run, _run_rows, sdrhip_pipe_deemph, examples/fm_replay --deemph) against
tests/deemph_model.py: bit for bit, final states included, NaN by position on the directed rows.  Every output sits between canaries
(gpu_util.dev_empty_f32), and the floats of an output buffer outside the rows' [0, n) are prefilled and checked.

The expected values are computed once per alpha at the longest length (a prefix of a de-emphasis output is the output of the prefix) and
shared read-only.  The stall rows (constant, silent) and the rows that turn NaN are ordinary finite-time work: every chunk behind the
event is repaired in turn, at most a sequential walk of the row."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import deemph_cases as DC
import deemph_model as DM
import gpu_util as G
import signals as S

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEQ, WG, LS = 1, 2, 3
NMAX = DC.WG_MAX + 1
FILL = 0x7FC0BEEF                                  # what the gaps of an output buffer hold before a call
ROW_NAMES = ["noise", "sine", "offset", "wide", "overflow", "inf", "nan", "constant", "silent"]
STATES = np.array([0.25, -1.5, 0.0, 3.0, 0.0, -0.125, 0.5, 0.0, 0.0], F)
NAN_ROWS = (4, 5, 6)


@pytest.fixture(autouse=True)
def _auto_route(hip):
    hip.set_deemph_route(0)
    yield
    hip.set_deemph_route(0)


def _inputs():
    rows = [DC.ordinary(k, NMAX, 40 + i) for i, k in enumerate(DC.ORDINARY_KINDS)]
    rows += [DC.directed(NMAX, v)[0] for v in ("overflow", "inf", "nan")]
    rows += [DC.constant(NMAX), DC.silent(NMAX)]
    return np.stack(rows)


@pytest.fixture(scope="module")
def shared():
    """the nine rows at the longest length and, per alpha, the model's output on them: computed once, read-only"""
    x = _inputs()
    x.setflags(write=False)
    exp = {}
    for a in DC.ALPHAS:
        out, _ = DM.deemph(x, a, STATES)
        out.setflags(write=False)
        exp[float(a)] = out
    return x, exp


def _final(exp_rows, states, n):
    return exp_rows[:, n - 1].copy() if n > 0 else np.asarray(states, F).copy()


def _same(got, exp, what, nan_rows=()):
    got, exp = np.ascontiguousarray(got, F), np.ascontiguousarray(exp, F)
    assert got.shape == exp.shape, f"{what}: shape {got.shape} vs {exp.shape}"
    ok = got.view(np.uint32) == exp.view(np.uint32)
    if len(nan_rows):
        loose = np.zeros(got.shape, bool)
        loose[list(nan_rows)] = True
        ok |= loose & np.isnan(got) & np.isnan(exp)
    bad = np.argwhere(~ok)
    assert bad.size == 0, (f"{what}: {len(bad)} floats differ; first at {tuple(bad[0])}: {got[tuple(bad[0])]!r} "
                           f"({got.view(np.uint32)[tuple(bad[0])]:#x}) vs {exp[tuple(bad[0])]!r} ({exp.view(np.uint32)[tuple(bad[0])]:#x})")


def run_rows(hip, x, alpha, states, in_pad=0, out_pad=0, in_off=0, out_off=0, ws="auto", run_in=0, alias_final=False, stream=None):
    """x: rows x n host floats -> (out rows x n, final, stats or None).  Rows in_pad / out_pad floats apart beyond n, bases in_off /
    out_off floats behind a 256-byte aligned address.  The output buffer is prefilled; its gaps are checked."""
    import torch
    x = np.ascontiguousarray(x, F)
    rows, n = x.shape
    si, so = n + in_pad, n + out_pad
    h_in = np.zeros(in_off + rows * si + 1, F)
    for r in range(rows):
        h_in[in_off + r * si: in_off + r * si + n] = x[r]
    d_in = G.to_dev(h_in)
    d_out = G.dev_empty_f32(out_off + rows * so + 1)
    d_out.view(torch.int32).fill_(FILL)
    d_state = G.to_dev(np.asarray(states, F))
    d_final = d_state if alias_final else G.dev_empty_f32(rows)
    need = hip.lib.sdrhip_deemph_rows_workspace_bytes(rows, n)
    d_ws = None
    if ws == "auto":
        d_ws = torch.full((need + 4096,), 0xA5, dtype=torch.uint8, device="cuda")
    rc = hip.lib.sdrhip_deemph_run_rows(stream, d_in.data_ptr() + 4 * in_off, si, d_out.data_ptr() + 4 * out_off, so, rows, n, float(alpha),
                                        d_state.data_ptr(), d_final.data_ptr(), d_ws.data_ptr() if d_ws is not None else None,
                                        need if d_ws is not None else 0, run_in)
    hip.check(rc, "sdrhip_deemph_run_rows")
    h_out = G.to_host(d_out)
    out = np.stack([h_out[out_off + r * so: out_off + r * so + n] for r in range(rows)])
    gaps = np.ones(h_out.size, bool)
    for r in range(rows):
        gaps[out_off + r * so: out_off + r * so + n] = False
    assert (h_out.view(np.uint32)[gaps] == FILL).all(), "floats outside the rows' [0, n) were written"
    stats = None
    if d_ws is not None:
        w = d_ws.cpu().numpy()
        assert (w[need:] == 0xA5).all(), "the 4096 bytes behind the reported workspace size were written"
        stats = [tuple(int(v) for v in r) for r in w[:16 * rows].view(np.uint32).reshape(rows, 4)] if n > 0 else None
    assert np.array_equal(G.to_host(d_in).view(np.uint32), h_in.view(np.uint32)), "the input was written"
    return out, G.to_host(d_final).copy(), stats


# ---- 1: against the model ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", DC.ALPHAS, ids=DC.ALPHA_IDS)
def test_against_the_model_at_every_plan_edge(hip, shared, alpha):
    x, exp = shared
    e = exp[float(alpha)]
    W = DM.default_run_in(alpha)
    for n in DC.lengths(alpha):
        for ws in (["auto", None] if n >= DC.WG_AUTO else ["auto"]):
            chunks, route, chunk, w = hip.deemph_plan(9, n, float(alpha), has_workspace=ws is not None)
            assert w == W and route == (SEQ if n < 2 * W else LS if ws and n >= DC.WG_AUTO else WG if n <= DC.WG_MAX else SEQ), (n, route)
            l0 = hip.deemph_launches()
            out, fin, stats = run_rows(hip, x[:, :n], alpha, STATES, ws=ws)
            assert hip.deemph_launches() - l0 == (5 if route == LS else 1)
            what = f"alpha {float(alpha):.4f}, n = {n}, route {route}"
            _same(out, e[:, :n], what, NAN_ROWS)
            _same(fin[None], _final(e, STATES, n)[None], what + ": final states", [0])
            if stats is not None:
                assert all(s[3] == chunks for s in stats), (what, stats)
                if route == SEQ:
                    assert all(s == (0, 0, 0, 0) for s in stats)
                if route == WG and float(alpha) < 1:
                    assert all(s == (0, 0, 0, chunks) for s in stats[:4]), f"{what}: ordinary rows were repaired: {stats[:4]}"
    # the one-row call with its state by value: row 1 at three lengths
    import torch
    for n in (7, 4097, NMAX):
        d_in, d_out, d_fin = G.to_dev(x[1, :n]), G.dev_empty_f32(n), G.dev_empty_f32(1)
        wsb = hip.lib.sdrhip_deemph_workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        hip.check(hip.lib.sdrhip_deemph_run(None, d_in.data_ptr(), d_out.data_ptr(), n, float(alpha), float(STATES[1]), d_fin.data_ptr(),
                                            ws.data_ptr(), wsb, 0), "sdrhip_deemph_run")
        _same(G.to_host(d_out)[None], e[1:2, :n], f"one-row call, n = {n}")
        _same(G.to_host(d_fin)[None], e[1:2, n - 1][None], f"one-row call, n = {n}: final")
    o, f = hip.deemph(G.to_dev(x[0, :4096]), float(alpha), state=float(STATES[0]))
    _same(G.to_host(o)[None], e[0:1, :4096], "lib.deemph")
    _same(G.to_host(f)[None], e[0:1, 4095][None], "lib.deemph: final")


# ---- 2: each route forced, launch counts, statistics -----------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha", DC.ALPHAS, ids=DC.ALPHA_IDS)
def test_each_route_forced_where_it_fits(hip, shared, alpha):
    x, exp = shared
    e = exp[float(alpha)]
    n, outs = 4096, {}
    for route, launches in ((SEQ, 1), (WG, 1), (LS, 5)):
        hip.set_deemph_route(route)
        assert hip.deemph_plan(9, n, float(alpha))[1] == route
        l0 = hip.deemph_launches()
        out, fin, stats = run_rows(hip, x[:, :n], alpha, STATES)
        assert hip.deemph_launches() - l0 == launches, f"route {route}"
        _same(out, e[:, :n], f"forced route {route}", NAN_ROWS)
        _same(fin[None], e[:, n - 1][None], f"forced route {route}: final states", [0])
        outs[route] = (out, fin)
        if route == LS:
            assert all(s[3] == 16 for s in stats) and all(s[:3] == (0, 0, 0) for s in stats[:4]), stats
    for route in (WG, LS):
        _same(outs[route][0], outs[SEQ][0], f"route {route} against SEQ", NAN_ROWS)
    hip.set_deemph_route(LS)
    n = 70001
    rng = np.random.default_rng(3)
    big = np.stack([DC.ordinary("noise", n, 60), DC.directed(n, "inf")[0], DC.ordinary("wide", n, 61)])
    st = rng.normal(0, 1, 3).astype(F)
    want, wfin = DM.deemph(big, alpha, st)
    out, fin, stats = run_rows(hip, big, alpha, st)
    _same(out, want, "LS at n = 70001 on 3 rows", [1])
    _same(fin[None], wfin[None], "LS at n = 70001: final states", [0])
    assert all(s[3] == hip.deemph_plan(3, n, float(alpha))[0] for s in stats)


def test_forced_routes_that_do_not_fit_are_refused_and_write_nothing(hip, shared):
    x, _ = shared
    a, W = DC.A48, DM.default_run_in(DC.A48)
    for route, n, ws in ((WG, 2 * W - 1, "auto"), (WG, DC.WG_MAX + 1, "auto"), (LS, 4096, None), (LS, 2 * W - 1, "auto")):
        hip.set_deemph_route(route)
        l0 = hip.deemph_launches()
        with pytest.raises(hip.SdrHipError, match="forced route"):
            run_rows(hip, x[:2, :n], a, STATES[:2], ws=ws)
        assert hip.deemph_launches() == l0
    # (run_rows' buffers, prefilled and between canaries, are checked by the guard fixture; the explicit check follows)
    hip.set_deemph_route(0)


@pytest.mark.parametrize("alpha", [DC.A48, DC.A256], ids=DC.ALPHA_IDS[:2])
def test_statistics_on_wg(hip, shared, alpha):
    x, exp = shared
    n = 4096
    out, fin, stats = run_rows(hip, x[:, :n], alpha, STATES)
    assert stats[:4] == [(0, 0, 0, 256)] * 4
    for r in (7, 8):                                   # the two stall rows: the scheme model's words
        _, _, want = DM.wg_scheme(x[r, :n], alpha, STATES[r])
        assert want[0] > 0 and want[2] > 0
        assert stats[r] == want, f"{ROW_NAMES[r]}: device {stats[r]}, scheme model {want}"
    # a run-in of 4 on an ordinary row: repaired, and still the model
    out4, fin4, stats4 = run_rows(hip, x[:1, :n], alpha, STATES[:1], run_in=4)
    assert stats4[0][2] > 0 and stats4[0][0] > 0 and stats4[0][3] == 256, stats4
    assert stats4[0] == DM.wg_scheme(x[0, :n], alpha, STATES[0], run_in=4)[2]
    _same(out4, exp[float(alpha)][:1, :n], "run-in of 4")


# ---- 3: rows ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 3, 65])
@pytest.mark.parametrize("route", [SEQ, WG, LS])
def test_rows_on_every_route(hip, route, rows):
    n = 2000
    x = DC.ordinary_rows(rows, n, 7)
    st = np.random.default_rng(rows).normal(0, 1, rows).astype(F)
    want, wfin = DM.deemph(x, DC.A48, st)
    hip.set_deemph_route(route)
    out, fin, _ = run_rows(hip, x, DC.A48, st, in_pad=5, out_pad=3)
    _same(out, want, f"{rows} rows on route {route}")
    _same(fin[None], wfin[None], f"{rows} rows on route {route}: final")


def test_1024_rows(hip):
    for n, route in ((100, SEQ), (1024, WG)):
        x = DC.ordinary_rows(1024, n, 9)
        st = np.random.default_rng(n).normal(0, 1, 1024).astype(F)
        want, wfin = DM.deemph(x, DC.A48, st)
        assert hip.deemph_plan(1024, n, float(DC.A48))[1] == route
        l0 = hip.deemph_launches()
        out, fin, stats = run_rows(hip, x, DC.A48, st)
        assert hip.deemph_launches() - l0 == 1
        _same(out, want, f"1024 rows x {n}")
        _same(fin[None], wfin[None], f"1024 rows x {n}: final")
        if route == WG:
            assert all(s[3] == 64 for s in stats)


@pytest.mark.parametrize("route", [SEQ, WG, LS])
@pytest.mark.parametrize("pad,off", [(0, 0), (1, 0), (3, 0), (0, 1), (0, 2), (1, 1), (2, 2), (3, 2)])
def test_strides_and_bases(hip, route, pad, off):
    """rows tight and +1 / +3 floats apart, bases 4 and 8 bytes off 16-byte alignment: 16 / 8 / 4-byte accesses, the same bits; row r
    equals the one-row call on row r"""
    n, rows = 1999, 3
    x = DC.ordinary_rows(rows, n, 11)
    st = np.array([0.5, -0.25, 2.0], F)
    want, wfin = DM.deemph(x, DC.A48, st)
    hip.set_deemph_route(route)
    out, fin, _ = run_rows(hip, x, DC.A48, st, in_pad=pad, out_pad=pad, in_off=off, out_off=off)
    _same(out, want, f"pad {pad}, base off {off}, route {route}")
    _same(fin[None], wfin[None], "final")
    for r in range(rows):
        o1, f1, _ = run_rows(hip, x[r:r + 1], DC.A48, st[r:r + 1], in_off=off, out_off=(off + 1) % 4)
        _same(o1, out[r:r + 1], f"row {r} against the one-row call")
        _same(f1[None], fin[None, r:r + 1], "final")


@pytest.mark.parametrize("route", [SEQ, WG, LS])
def test_a_neighbour_row_of_nan_or_inf_changes_nothing(hip, route):
    n = 2000
    x = DC.ordinary_rows(3, n, 13)
    st = np.array([0.5, -0.25, 2.0], F)
    hip.set_deemph_route(route)
    base, bfin, _ = run_rows(hip, x, DC.A48, st)
    for poison in (np.nan, np.inf):
        y = x.copy()
        y[1] = poison
        out, fin, _ = run_rows(hip, y, DC.A48, np.array([0.5, poison, 2.0], F))
        _same(out[[0, 2]], base[[0, 2]], f"rows next to a row of {poison}")
        _same(fin[None, [0, 2]], bfin[None, [0, 2]], "final")
        assert np.isnan(out[1][1:]).all()


@pytest.mark.parametrize("route", [0, SEQ, WG, LS])
def test_three_calls_cut_at_odd_samples_equal_one(hip, route):
    import torch
    n, rows, cuts = 6001, 3, [0, 1777, 3999, 6001]
    x = DC.ordinary_rows(rows, n, 17)
    st = np.array([0.5, -0.25, 2.0], F)
    want, wfin = DM.deemph(x, DC.A48, st)
    hip.set_deemph_route(route)
    d_in, d_out, d_state = G.to_dev(x), G.dev_empty_f32(rows * n), G.to_dev(st)
    wsb = hip.lib.sdrhip_deemph_rows_workspace_bytes(rows, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for a, b in zip(cuts[:-1], cuts[1:]):                  # d_final == d_state, no synchronisation between the calls
        hip.check(hip.lib.sdrhip_deemph_run_rows(None, d_in.data_ptr() + 4 * a, n, d_out.data_ptr() + 4 * a, n, rows, b - a, float(DC.A48),
                                                 d_state.data_ptr(), d_state.data_ptr(), ws.data_ptr(), wsb, 0), "sdrhip_deemph_run_rows")
    _same(G.to_host(d_out).reshape(rows, n), want, f"three calls, route {route}")
    _same(G.to_host(d_state)[None], wfin[None], "final")
    # n == 0 copies the states and touches nothing else
    d_fin = G.dev_empty_f32(rows)
    l0 = hip.deemph_launches()
    hip.check(hip.lib.sdrhip_deemph_run_rows(None, d_in.data_ptr(), n, d_out.data_ptr(), n, rows, 0, float(DC.A48), d_state.data_ptr(),
                                             d_fin.data_ptr(), ws.data_ptr(), wsb, 0), "n == 0")
    _same(G.to_host(d_fin)[None], wfin[None], "n == 0: the states are copied")
    _same(G.to_host(d_out).reshape(rows, n), want, "n == 0: the output is untouched")
    assert hip.deemph_launches() - l0 == 1


def test_rows_two_to_the_31_floats_apart(hip):
    """two rows 2^31 + 6 floats apart, short n: the row offset is 64-bit arithmetic on every route"""
    import torch
    stride, n = (1 << 31) + 6, 1000
    x = DC.ordinary_rows(2, n, 19)
    st = np.array([0.5, -0.25], F)
    want, wfin = DM.deemph(x, DC.A48, st)
    d_in = torch.empty(stride + n, dtype=torch.float32, device="cuda")
    d_out = torch.empty(stride + n + 64, dtype=torch.float32, device="cuda")
    for r in range(2):
        d_in[r * stride: r * stride + n] = torch.from_numpy(x[r]).cuda()
    d_state = G.to_dev(st)
    wsb = hip.lib.sdrhip_deemph_rows_workspace_bytes(2, n)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    for route in (SEQ, WG, LS):
        hip.set_deemph_route(route)
        for r in range(2):
            d_out[r * stride: r * stride + n + 64].view(torch.int32).fill_(FILL)
        d_fin = G.dev_empty_f32(2)
        hip.check(hip.lib.sdrhip_deemph_run_rows(None, d_in.data_ptr(), stride, d_out.data_ptr(), stride, 2, n, float(DC.A48),
                                                 d_state.data_ptr(), d_fin.data_ptr(), ws.data_ptr(), wsb, 0), "far rows")
        torch.cuda.synchronize()
        got = np.stack([d_out[r * stride: r * stride + n + 64].cpu().numpy() for r in range(2)])
        _same(got[:, :n], want, f"rows 2^31 + 6 apart, route {route}")
        assert (got[:, n:].view(np.uint32) == FILL).all()
        _same(G.to_host(d_fin)[None], wfin[None], "final")
    del d_in, d_out
    torch.cuda.empty_cache()


# ---- 4: workspace and refusals ----------------------------------------------------------------------------------------------------------
def test_workspace_short_null_and_refusals_write_nothing(hip):
    import torch
    n, rows = 70001, 2
    xin = np.stack([DC.ordinary("noise", n, 70), DC.ordinary("sine", n, 71)])
    want, wfin = DM.deemph(xin, DC.A48, STATES[:rows])
    # with a workspace (LS; run_rows checks the 4096 bytes behind it) and with none (SEQ): the same bits
    for ws, launches in (("auto", 5), (None, 1)):
        l0 = hip.deemph_launches()
        out, fin, _ = run_rows(hip, xin, DC.A48, STATES[:rows], ws=ws)
        assert hip.deemph_launches() - l0 == launches
        _same(out, want, f"n = {n}, workspace {ws}")
        _same(fin[None], wfin[None], "final")
    # refusals on the device: nothing written, nothing launched
    d_in, d_out, d_state, d_fin = G.to_dev(xin), G.dev_empty_f32(rows * n), G.to_dev(STATES[:rows]), G.dev_empty_f32(rows)
    d_out.view(torch.int32).fill_(FILL)
    d_fin.view(torch.int32).fill_(FILL)
    need = hip.lib.sdrhip_deemph_rows_workspace_bytes(rows, n)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    run = hip.lib.sdrhip_deemph_run_rows
    p_in, p_out, p_st, p_fin, p_ws = d_in.data_ptr(), d_out.data_ptr(), d_state.data_ptr(), d_fin.data_ptr(), ws.data_ptr()
    l0 = hip.deemph_launches()
    bad = [run(None, p_in, n, p_out, n, rows, n, float(DC.A48), p_st, p_fin, p_ws, need - 1, 0),          # one byte short
           run(None, p_in, n, p_out, n, rows, n, 0.0, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, rows, n, float("nan"), p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, rows, n, 1.5, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, 0, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, 1025, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n - 1, p_out, n, rows, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n - 1, rows, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_in, n, rows, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, rows, -1, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, rows, n, 0.25, p_st, p_fin, p_ws, need, -1),
           run(None, None, n, p_out, n, rows, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, None, n, rows, n, 0.25, p_st, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, rows, n, 0.25, None, p_fin, p_ws, need, 0),
           run(None, p_in, n, p_out, n, rows, n, 0.25, p_st, None, p_ws, need, 0)]
    assert bad == [-1] * len(bad), bad
    torch.cuda.synchronize()
    assert hip.deemph_launches() == l0
    assert (G.to_host(d_out).view(np.uint32) == FILL).all() and (G.to_host(d_fin).view(np.uint32) == FILL).all()
    assert (ws.cpu().numpy() == 0xA5).all() and np.array_equal(G.to_host(d_state), STATES[:rows])


# ---- 5: behind a bank -------------------------------------------------------------------------------------------------------------------
def test_behind_an_fm_bank_on_one_stream(hip):
    """FmBank.run, then deemph_rows on a strided view of its audio, queued on one stream with no synchronisation between: equals
    the model on that audio"""
    import torch
    import tuner_model as TM
    B, nblk = 8192, 20
    n_in = nblk * B
    u8 = S.iq_u8_fm(n_in, seed=4501)
    tables = [TM.shift_table(-3, 1000), TM.shift_table(1, 4), np.array([1.0, 0.0], F)]
    bank = hip.FmBank(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), tables, 0.2, B)
    q0, q1, _ = bank.plan(0, n_in, n_in)
    K, stride = len(tables), q1 - q0 + 5
    d_in = G.to_dev(u8)
    audio = G.dev_empty_f32(K * stride)
    wsb = max(bank.workspace_bytes(n_in), 16)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    alpha = hip.deemph_alpha(75e-6, 48000.0)
    states = G.to_dev(np.zeros(K, F))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        bank.run(d_in.data_ptr(), 0, n_in, audio.data_ptr(), stride, q0, q1, ws.data_ptr(), wsb, stream=s.cuda_stream)
        view = audio.view(K, stride)[:, 1:q1 - q0]               # a strided view, 4 bytes off the rows' alignment
        out, fin = hip.deemph_rows(view, alpha, states, final=states)
    s.synchronize()
    a = G.to_host(audio).reshape(K, stride)[:, 1:q1 - q0]
    assert np.isfinite(a).all() and np.abs(a).max() > 0
    want, wfin = DM.deemph(a, alpha, np.zeros(K, F))
    _same(out.cpu().numpy(), want, "deemph_rows behind FmBank.run")
    _same(states.cpu().numpy()[None], wfin[None], "final")


# ---- 6: the Pipe ------------------------------------------------------------------------------------------------------------------------
UNIFORM = [8192] * 12
RAGGED = [4096, 8192, 1, 1000, 20000, 777, 7, 8192, 129, 5000, 3, 8192]


def _blocks(sizes, alpha, seed=11):
    x = DC.ordinary("sine", sum(sizes), seed)
    e, _ = DM.deemph(x, alpha, 0.0)
    cut = np.cumsum([0] + list(sizes))
    return [x[a:b] for a, b in zip(cut[:-1], cut[1:])], [e[a:b] for a, b in zip(cut[:-1], cut[1:])]


def _cmp(got, exp, what):
    assert [g.size for g in got] == [e.size for e in exp], f"{what}: block lengths {[g.size for g in got]} vs {[e.size for e in exp]}"
    for i, (g, e) in enumerate(zip(got, exp)):
        _same(g[None], e[None], f"{what}, block {i}")


@pytest.mark.parametrize("adaptive", [32, 2, 0], ids=["adaptive 32", "adaptive 2", "every push on its own"])
@pytest.mark.parametrize("sizes", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
def test_pipe_uniform_and_ragged_pushes(hip, sizes, adaptive):
    blocks, exp = _blocks(sizes, DC.A48)
    pipe = hip.Pipe.deemph(float(DC.A48))
    assert pipe.rows == 1 and not pipe.complex_in and not pipe.complex_out
    pipe.set_adaptive(adaptive)
    got = []
    for i, b in enumerate(blocks):
        got += pipe.push(b)
        if i % 5 == 4:
            got += pipe.poll()
    got += pipe.flush()
    _cmp(got, exp, f"de-emphasis Pipe, adaptive {adaptive}")
    assert pipe.flush() == [] and pipe.poll() == []


def test_pipe_both_sides_of_the_staging_bound(hip):
    """The staging engine reads runs of up to 512 KiB of input in place over PCIe for the map stages that allow it; de-emphasis never
    does (its lanes re-read their run-in), so blocks of 131071 / 131072 / 131073 floats, each alone in its run, and two that pile up past
    the bound all go through the copy engines and give the same blocks.  Runs of 32768 samples and more take the launch set."""
    sizes = [131071, 131072, 131073, 80000, 80000]
    blocks, exp = _blocks(sizes, DC.A48, seed=13)
    pipe = hip.Pipe.deemph(float(DC.A48))
    pipe.set_adaptive(0)
    l0 = hip.deemph_launches()
    got = []
    for b in blocks:
        got += pipe.push(b)
    got += pipe.flush()
    assert hip.deemph_launches() - l0 == 5 * len(sizes)          # adaptive off: every push is one run, from 32768 samples on one launch set
    _cmp(got, exp, "de-emphasis Pipe across the staging bound")
    pipe = hip.Pipe.deemph(float(DC.A48))
    got = []
    for b in blocks:
        got += pipe.push(b)
    _cmp(got + pipe.flush(), exp, "de-emphasis Pipe across the staging bound, adaptive")


def test_pipe_save_after_5_of_40_pushes_and_restore_with_the_three_refusals(hip):
    sizes = [int(s) for s in np.random.default_rng(5).choice([1, 7, 100, 1024, 4096, 8192], 40)]
    a = float(DC.A48)
    blocks, exp = _blocks(sizes, DC.A48, seed=17)
    first = hip.Pipe.deemph(a)
    got = []
    for b in blocks[:5]:
        got += first.push(b)
    state = first.save()
    fields = struct.unpack_from("<II10i5q6f", state)
    assert fields[:3] == (0x50504453, 1, 4), "a de-emphasis state holds the one-pole map kind's number"
    dc = struct.unpack_from("<4I", state, struct.calcsize("<II10i5q2f"))
    want_y = DM.deemph(np.concatenate(blocks[:5]), DC.A48, 0.0)[1]
    assert dc == (int(want_y.view(np.uint32)), 0, int(DC.A48.view(np.uint32)), 0), dc
    del first
    second = hip.Pipe.deemph(a)
    got += second.restore(state, max_block=max(sizes))
    for b in blocks[5:]:
        got += second.push(b)
    got += second.flush()
    _cmp(got, exp, "de-emphasis Pipe saved after 5 of 40 pushes")
    # the three refusals, each leaving the pipe fresh
    dcp = hip.dcBlockingFilter()
    dcp.push(blocks[0])
    dc_state = dcp.save()
    assert struct.unpack_from("<II10i", dc_state)[2] == 4
    assert struct.unpack_from("<4I", dc_state, struct.calcsize("<II10i5q2f"))[2:] == (0, 0), "a dcBlocker's state keeps the zeros it had"
    fresh = hip.Pipe.deemph(a)
    with pytest.raises(hip.SdrHipError, match="dcBlocker"):
        fresh.restore(dc_state)
    with pytest.raises(hip.SdrHipError, match="de-emphasis"):
        hip.dcBlockingFilter().restore(state)
    other = hip.Pipe.deemph(float(DC.A256))
    with pytest.raises(hip.SdrHipError, match="another alpha"):
        other.restore(state)
    with pytest.raises(hip.SdrHipError):
        fresh.restore(state[:-4])
    for p, al in ((fresh, DC.A48), (other, DC.A256)):          # both still fresh: they start from 0
        assert p.flush() == []
        b, e = _blocks([3000], al, seed=23)
        _cmp(p.push(b[0]) + p.flush(), e, "a pipe that refused a state goes on from 0")
    again = hip.Pipe.deemph(a)
    n_blocks = fields[11]
    _cmp(again.restore(state, max_block=max(sizes)), exp[5 - n_blocks: 5], "restore after the refusals")
    _cmp(again.push(blocks[5]) + again.flush(), exp[5:6], "the restored pipe goes on")


# ---- 7: the example ---------------------------------------------------------------------------------------------------------------------
def test_fm_replay_with_and_without_de_emphasis(hip, tmp_path):
    """--deemph 75 --audio-rate 48000 against the model on fm_replay's own audio; without the flags the audio is what it was (the
    bytes themselves are pinned against the restated reference pipeline by tests/test_gpu_examples.py): the same as a stream driven
    from the binding"""
    exe = os.path.join(ROOT, "examples", "bin", "fm_replay")
    if not os.path.exists(exe):
        from sdr_amd import build as Bd
        Bd.build_examples()
    B, nblk = 8192, 70
    u8 = S.iq_u8_fm(nblk * B)
    cap = tmp_path / "capture.u8"
    u8.tofile(cap)
    S.taps_decim127().tofile(str(cap) + ".decim.f32")
    S.taps_resamp191().tofile(str(cap) + ".resamp.f32")
    S.taps_audio_half64().tofile(str(cap) + ".audio_half.f32")
    plain, de = tmp_path / "plain.f32", tmp_path / "de.f32"
    for out, flags in ((plain, []), (de, ["--deemph", "75", "--audio-rate", "48000"])):
        r = subprocess.run([exe, str(cap), str(out), "7"] + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    a, d = np.fromfile(plain, F), np.fromfile(de, F)
    assert a.size >= 2 * B and a.size % B == 0 and np.isfinite(a).all()
    chain = hip.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, B)
    st = hip.FmStream(chain, 7 * B, B)
    outs = []
    for i in range(0, nblk, 7):
        outs += st.push(u8[2 * i * B: 2 * (i + 7) * B])
    outs += st.flush()
    _same(a[None], np.concatenate(outs)[None], "fm_replay without the flags against the stream driven from the binding")
    want, _ = DM.deemph(a, DM.alpha_of(75e-6, 48000.0), 0.0)
    _same(d[None], want[None], "fm_replay --deemph 75 --audio-rate 48000 against the model on fm_replay's own audio")
    assert not np.array_equal(a, d)
