"""De-emphasis (sdrhip_deemph_*, sdrhip_pipe_deemph) on a host without a GPU: the names are declared, exported and bound;
sdrhip_deemph_alpha's bits; the plan function's route edges; and every refusal comes back as SDRHIP_ERR_ARG under the function's own
name before any pointer is looked at (the pointers handed in here point nowhere) and moves no launch counter.  What the operator
COMPUTES is held to tests/deemph_model.py on the device (tests/test_gpu_deemph.py)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import deemph_cases as DC
import deemph_model as DM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_deemph_alpha", "sdrhip_deemph_workspace_bytes", "sdrhip_deemph_run", "sdrhip_deemph_rows_workspace_bytes",
               "sdrhip_deemph_run_rows", "sdrhip_debug_deemph_plan", "sdrhip_debug_set_deemph_route", "sdrhip_debug_deemph_launches",
               "sdrhip_pipe_deemph"]
P = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]      # never dereferenced: every call below is refused first
SEQ, WG, LS = 1, 2, 3


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


@pytest.fixture(autouse=True)
def _auto_route(L):
    L.set_deemph_route(0)
    yield
    L.set_deemph_route(0)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    for f in ("deemph_alpha", "deemph", "deemph_rows", "deemph_plan", "set_deemph_route", "deemph_launches"):
        assert callable(getattr(L, f))
    assert callable(L.Pipe.deemph) and L.deemph_launches() >= 0


def test_alpha_is_the_double_expression_rounded_once(L):
    for tau, rate in DC.ALPHA_ARGS:
        want = np.float32(1 - math.exp(-1 / (tau * rate)))
        got = np.float32(L.deemph_alpha(tau, rate))
        assert got.view(np.uint32) == want.view(np.uint32), f"({tau}, {rate}): {got!r} vs {want!r}"
        assert 0 < got <= 1
    assert abs(L.deemph_alpha(75e-6, 48000.0) - 0.2425) < 1e-4
    for tau, rate in ((0.0, 48000.0), (-75e-6, 48000.0), (75e-6, 0.0), (75e-6, -1.0), (math.nan, 48000.0), (75e-6, math.nan),
                      (math.inf, 48000.0), (75e-6, math.inf), (-math.inf, 48000.0)):
        assert L.deemph_alpha(tau, rate) == 0.0, f"({tau}, {rate}) is not refused with 0"


def test_the_plan_flips_at_two_run_ins_and_at_the_wg_bound(L):
    a = float(DC.A48)
    W = DM.default_run_in(a)
    assert W == 168 and L.deemph_plan(1, 10 * W, a)[3] == W
    assert L.deemph_plan(1, 2 * W - 1, a)[:2] == (0, SEQ)
    chunks, route, chunk, w = L.deemph_plan(1, 2 * W, a)
    assert route == WG and chunk == 16 and chunks == (2 * W + 15) // 16 and w == W
    # the bound of the WG route, 65536 / 65537: without a workspace auto flips there, WG -> SEQ; with one it has flipped to LS at the
    # measured edge 32767 / 32768 already; past the bound the route is LS with a workspace and SEQ without one
    assert L.deemph_plan(1, DC.WG_MAX, a, has_workspace=False) == (1024, WG, 64, W)
    assert L.deemph_plan(1, DC.WG_AUTO - 1, a)[:3] == (1024, WG, 32) and L.deemph_plan(1, DC.WG_AUTO, a)[1] == LS
    assert L.deemph_plan(1, DC.WG_AUTO, a, has_workspace=False)[1] == WG and L.deemph_plan(1, DC.WG_MAX, a)[1] == LS
    assert L.deemph_plan(1, DC.WG_MAX + 1, a, has_workspace=True)[1] == LS
    assert L.deemph_plan(1, DC.WG_MAX + 1, a, has_workspace=False)[:2] == (0, SEQ)
    L.set_deemph_route(WG)
    assert L.deemph_plan(1, DC.WG_MAX, a) == (1024, WG, 64, W)
    L.set_deemph_route(0)
    # the edges do not depend on the rows, and the chunk count never passes 1024 on WG
    for rows in (1, 3, 1024):
        assert L.deemph_plan(rows, 2 * W - 1, a)[1] == SEQ and L.deemph_plan(rows, 2 * W, a)[1] == WG
        assert L.deemph_plan(rows, DC.WG_MAX, a, has_workspace=False)[:2] == (1024, WG) and L.deemph_plan(rows, DC.WG_MAX + 1, a)[1] == LS
        assert L.deemph_plan(rows, DC.WG_AUTO - 1, a)[1] == WG and L.deemph_plan(rows, DC.WG_AUTO, a)[1] == LS
    for n in range(2 * W, DC.WG_MAX + 1, 997):
        chunks, route, chunk, _ = L.deemph_plan(1, n, a, has_workspace=False)
        assert route == WG and chunks <= 1024 and chunk % 4 == 0 and chunk >= 16 and chunks == (n + chunk - 1) // chunk
        assert (chunks, chunk) == ((n + DM.wg_chunk(n) - 1) // DM.wg_chunk(n), DM.wg_chunk(n))
    # LS: lane = (row, chunk) under the cap of 32768, chunks of at least 256
    for rows, n in ((1, 70001), (3, 70001), (1024, 70001), (1, 1 << 24)):
        chunks, route, chunk, _ = L.deemph_plan(rows, n, a)
        assert route == LS and chunk >= 256 and chunk % 4 == 0 and rows * chunks <= 32768 and chunks == (n + chunk - 1) // chunk
    # an explicit run-in is rounded up to a multiple of 4 and moves the lower edge with it
    assert L.deemph_plan(1, 1024, a, run_in=5)[3] == 8 and L.deemph_plan(1, 15, a, run_in=5)[1] == SEQ and L.deemph_plan(1, 16, a, run_in=5)[1] == WG
    for al in DC.ALPHAS:
        assert L.deemph_plan(1, 1 << 20, float(al))[3] == DM.default_run_in(al)


def test_a_tiny_alpha_plans_the_sequential_walk(L):
    a = 2.0 ** -20
    assert DM.default_run_in(a) == 40 << 20
    for n in (0, 1, 4096, DC.WG_MAX, DC.WG_MAX + 1, 1 << 24, (80 << 20) - 1):
        assert L.deemph_plan(1, n, a)[:2] == (0, SEQ) and L.deemph_plan(1024, n, a, has_workspace=False)[:2] == (0, SEQ)


def test_forced_routes_that_do_not_fit_are_refused_by_the_plan(L):
    a, W = float(DC.A48), 168
    L.set_deemph_route(WG)
    assert L.deemph_plan(1, 4096, a)[1] == WG
    for n in (2 * W - 1, DC.WG_MAX + 1):
        with pytest.raises(L.SdrHipError, match="sdrhip_debug_deemph_plan"):
            L.deemph_plan(1, n, a)
    L.set_deemph_route(LS)
    assert L.deemph_plan(1, 4096, a)[:3] == (16, LS, 256)
    with pytest.raises(L.SdrHipError):
        L.deemph_plan(1, 4096, a, has_workspace=False)
    with pytest.raises(L.SdrHipError):
        L.deemph_plan(1, 2 * W - 1, a)
    L.set_deemph_route(SEQ)
    assert L.deemph_plan(1, 4096, a)[:2] == (0, SEQ)
    L.set_deemph_route(0)
    assert L.deemph_plan(1, 4096, a)[1] == WG


def test_workspace_bytes(L):
    lib = L.lib
    assert lib.sdrhip_deemph_workspace_bytes(4096) == lib.sdrhip_deemph_rows_workspace_bytes(1, 4096) > 16
    assert lib.sdrhip_deemph_rows_workspace_bytes(0, 100) == 0 and lib.sdrhip_deemph_rows_workspace_bytes(1025, 100) == 0
    for rows, n in ((1, 0), (3, 4096), (3, 70001), (1024, 70001)):
        assert lib.sdrhip_deemph_rows_workspace_bytes(rows, n) >= 16 * rows, (rows, n)
    L.set_deemph_route(LS)
    for rows, n in ((1, 4096), (3, 70001), (1024, 70001)):
        chunks = L.deemph_plan(rows, n, 1.0)[0]
        assert lib.sdrhip_deemph_rows_workspace_bytes(rows, n) >= rows * 16 + rows * chunks * 13


def _rows(L, d_in=P[0], in_stride=100, d_out=P[1], out_stride=100, rows=3, n=100, alpha=0.25, d_state=P[2], d_final=P[3], ws=None, ws_bytes=0,
          run_in=0):
    return L.lib.sdrhip_deemph_run_rows(None, d_in, in_stride, d_out, out_stride, rows, n, alpha, d_state, d_final, ws, ws_bytes, run_in)


def _one(L, d_in=P[0], d_out=P[1], n=100, alpha=0.25, state=0.0, d_final=P[3], ws=None, ws_bytes=0, run_in=0):
    return L.lib.sdrhip_deemph_run(None, d_in, d_out, n, alpha, state, d_final, ws, ws_bytes, run_in)


def _refused(L, fn, what, rc, launches):
    assert rc == ERR_ARG, f"{fn}: {what} is not refused"
    assert fn.encode() in L.lib.sdrhip_last_error(), f"{fn}: {what}: {L.lib.sdrhip_last_error()!r}"
    assert L.deemph_launches() == launches, f"{fn}: {what}: a refused call launched"


BAD_ALPHAS = (0.0, -0.25, 1.0000001, 2.0, math.nan, math.inf, -math.inf, -0.0)


def test_rows_refusals_move_no_launch_counter(L):
    fn, c = "sdrhip_deemph_run_rows", L.deemph_launches()
    for alpha in BAD_ALPHAS:
        _refused(L, fn, f"alpha = {alpha}", _rows(L, alpha=alpha), c)
    for rows in (0, -1, 1025):
        _refused(L, fn, f"rows = {rows}", _rows(L, rows=rows), c)
    for name in ("d_in", "d_out", "d_state", "d_final"):
        _refused(L, fn, f"null {name}", _rows(L, **{name: None}), c)
        _refused(L, fn, f"null {name} with n = 0", _rows(L, n=0, **{name: None}), c)
        _refused(L, fn, f"null {name} with one row", _rows(L, rows=1, **{name: None}), c)
    _refused(L, fn, "n < 0", _rows(L, n=-1), c)
    _refused(L, fn, "run_in < 0", _rows(L, run_in=-1), c)
    _refused(L, fn, "in place", _rows(L, d_out=P[0]), c)
    _refused(L, fn, "in place with one row", _rows(L, rows=1, d_out=P[0]), c)
    _refused(L, fn, "in_stride shorter than a row", _rows(L, in_stride=99), c)
    _refused(L, fn, "out_stride shorter than a row", _rows(L, out_stride=99), c)
    _refused(L, fn, "a negative stride", _rows(L, in_stride=-100), c)
    need = L.lib.sdrhip_deemph_rows_workspace_bytes(3, 100)
    _refused(L, fn, "a workspace one byte short", _rows(L, ws=P[4], ws_bytes=need - 1), c)
    _refused(L, fn, "a workspace of no bytes", _rows(L, ws=P[4], ws_bytes=0), c)
    # forced routes that do not fit (alpha 0.25: the default run-in is 160)
    L.set_deemph_route(WG)
    _refused(L, fn, "forced WG below two run-ins", _rows(L, n=319, in_stride=400, out_stride=400), c)
    _refused(L, fn, "forced WG past its bound", _rows(L, n=65537, in_stride=65537, out_stride=65537), c)
    L.set_deemph_route(LS)
    _refused(L, fn, "forced LS without a workspace", _rows(L, n=4096, in_stride=4096, out_stride=4096), c)
    need = L.lib.sdrhip_deemph_rows_workspace_bytes(3, 319)
    _refused(L, fn, "forced LS below two run-ins", _rows(L, n=319, in_stride=400, out_stride=400, ws=P[4], ws_bytes=need), c)


def test_one_row_refusals_move_no_launch_counter(L):
    fn, c = "sdrhip_deemph_run", L.deemph_launches()
    for alpha in BAD_ALPHAS:
        _refused(L, fn, f"alpha = {alpha}", _one(L, alpha=alpha), c)
    for name in ("d_in", "d_out", "d_final"):
        _refused(L, fn, f"null {name}", _one(L, **{name: None}), c)
        _refused(L, fn, f"null {name} with n = 0", _one(L, n=0, **{name: None}), c)
    _refused(L, fn, "n < 0", _one(L, n=-1), c)
    _refused(L, fn, "run_in < 0", _one(L, run_in=-1), c)
    _refused(L, fn, "in place", _one(L, d_out=P[0]), c)
    _refused(L, fn, "a workspace one byte short", _one(L, ws=P[4], ws_bytes=L.lib.sdrhip_deemph_workspace_bytes(100) - 1), c)
    L.set_deemph_route(WG)
    _refused(L, fn, "forced WG below two run-ins", _one(L, n=319), c)
    L.set_deemph_route(LS)
    _refused(L, fn, "forced LS without a workspace", _one(L, n=4096), c)


def test_plan_refusals(L):
    plan = L.lib.sdrhip_debug_deemph_plan
    for args in ((0, 100, 0.25, 0, 1), (1025, 100, 0.25, 0, 1), (1, -1, 0.25, 0, 1), (1, 100, 0.25, -1, 1), (1, 100, 0.0, 0, 1),
                 (1, 100, math.nan, 0, 1), (1, 100, 1.5, 0, 1)):
        assert plan(*args, None, None, None) == ERR_ARG and b"sdrhip_debug_deemph_plan" in L.lib.sdrhip_last_error(), args
    assert plan(1, 4096, 0.25, 0, 1, None, None, None) == 256


def test_pipe_create_refusals(L):
    h = C.c_void_p(0x1234)
    assert L.lib.sdrhip_pipe_deemph(None, 0.25) == ERR_ARG and b"sdrhip_pipe_deemph" in L.lib.sdrhip_last_error()
    for alpha in BAD_ALPHAS:
        h.value = 0x1234
        assert L.lib.sdrhip_pipe_deemph(C.byref(h), alpha) == ERR_ARG, alpha
        assert b"sdrhip_pipe_deemph" in L.lib.sdrhip_last_error() and not h.value


def test_the_example_takes_the_flags_together_or_not_at_all(L):
    import subprocess
    from sdr_amd import build as Bld
    Bld.build_examples()
    exe = os.path.join(Bld.EXAMPLES, "bin", "fm_replay")
    assert os.access(exe, os.X_OK)
    for args in (["--deemph", "75"], ["--audio-rate", "48000"], ["--deemph", "0", "--audio-rate", "48000"], ["--deemph", "75", "--audio-rate", "-1"]):
        r = subprocess.run([exe, "in.u8", "out.f32"] + args, capture_output=True, text=True)
        assert r.returncode == 2 and "--deemph" in r.stderr, (args, r.returncode, r.stderr)
