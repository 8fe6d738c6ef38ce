"""The row forms (sdrhip_agc_run_rows, sdrhip_dc_blocker_run_rows, sdrhip_fm_demod_run_rows) on a host without a GPU: the names are
declared, exported and bound; every refusal comes back as SDRHIP_ERR_ARG under the function's own name before any pointer is looked
at (the pointers handed in here point nowhere); the rows plan of one row is the one-row plan, and 1024 rows stay within the lane
cap.  What the row forms COMPUTE is held to the models on the device (tests/test_gpu_rows.py)."""
import ctypes as C
import os

import pytest

import iir_cases as IC

ERR_ARG = -1
LANE_CAP = 32768                                        # kAgcMaxLanes, kDcMaxLanes
NEW_SYMBOLS = ["sdrhip_agc_rows_workspace_bytes", "sdrhip_agc_run_rows", "sdrhip_debug_agc_rows_plan",
               "sdrhip_dc_blocker_rows_workspace_bytes", "sdrhip_dc_blocker_run_rows", "sdrhip_debug_dc_rows_plan",
               "sdrhip_fm_demod_run_rows", "sdrhip_debug_rows_launches"]
P = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000]       # never dereferenced: every call below is refused first


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    assert L.lib.sdrhip_debug_rows_launches.restype is C.c_longlong
    assert L.lib.sdrhip_agc_rows_workspace_bytes.restype is C.c_size_t and L.lib.sdrhip_dc_blocker_rows_workspace_bytes.restype is C.c_size_t
    assert L.rows_launches() >= 0
    header = open(os.path.join(os.path.dirname(L.HERE), "include", "sdr_hip.h")).read()
    assert "#define SDRHIP_ROWS_MAX 1024" in header and L.ROWS_MAX == 1024
    for f in ("agc_rows", "dc_blocker_rows", "fm_demod_rows", "agc_rows_plan", "dc_rows_plan", "rows_stats", "rows_launches"):
        assert callable(getattr(L, f))


def _refused(L, fn, what, rc):
    assert rc == ERR_ARG, f"{fn}: {what} is not refused"
    assert fn.encode() in L.lib.sdrhip_last_error(), f"{fn}: {what}: {L.lib.sdrhip_last_error()!r}"


def _agc(L, d_in=P[0], in_stride=200, d_out=P[1], out_stride=200, rows=3, n=100, mu=0.4, ref=1.0, d_state=P[2], d_final=P[3], ws=None,
         ws_bytes=0, run_in=0):
    return L.lib.sdrhip_agc_run_rows(None, d_in, in_stride, d_out, out_stride, rows, n, mu, ref, d_state, d_final, ws, ws_bytes, run_in)


def _dc(L, d_in=P[0], in_stride=100, d_out=P[1], out_stride=100, rows=3, n=100, d_state=P[2], d_final=P[3], ws=None, ws_bytes=0, run_in=0):
    return L.lib.sdrhip_dc_blocker_run_rows(None, d_in, in_stride, d_out, out_stride, rows, n, d_state, d_final, ws, ws_bytes, run_in)


def _fm(L, d_in=P[0], in_stride=200, in_base=0, d_out=P[1], out_stride=100, rows=3, k_begin=0, k_end=100, last=None, last_out=None):
    return L.lib.sdrhip_fm_demod_run_rows(None, d_in, in_stride, in_base, d_out, out_stride, rows, k_begin, k_end, last, last_out)


def test_agc_rows_refusals(L):
    fn = "sdrhip_agc_run_rows"
    for rows in (0, -1, 1025):
        _refused(L, fn, f"rows = {rows}", _agc(L, rows=rows))
    for name in ("d_in", "d_out", "d_state", "d_final"):
        _refused(L, fn, f"null {name}", _agc(L, **{name: None}))
    _refused(L, fn, "n < 0", _agc(L, n=-1))
    _refused(L, fn, "run_in < 0 (the one-row call refuses it)", _agc(L, run_in=-1))
    _refused(L, fn, "in place (the one-row call refuses it)", _agc(L, d_out=P[0]))
    _refused(L, fn, "in_stride shorter than a row", _agc(L, in_stride=198))
    _refused(L, fn, "out_stride shorter than a row", _agc(L, out_stride=198))
    _refused(L, fn, "a negative stride", _agc(L, in_stride=-200))
    _refused(L, fn, "odd in_stride", _agc(L, in_stride=201))
    _refused(L, fn, "odd out_stride", _agc(L, out_stride=203))
    need = L.lib.sdrhip_agc_rows_workspace_bytes(3, 100)
    assert need >= 3 * 16
    _refused(L, fn, "a workspace one byte too small", _agc(L, ws=P[4], ws_bytes=need - 1))
    _refused(L, fn, "a workspace of no bytes", _agc(L, ws=P[4], ws_bytes=0))
    assert b"workspace" in L.lib.sdrhip_last_error()


def test_dc_blocker_rows_refusals(L):
    fn = "sdrhip_dc_blocker_run_rows"
    for rows in (0, -1, 1025):
        _refused(L, fn, f"rows = {rows}", _dc(L, rows=rows))
    for name in ("d_in", "d_out", "d_state", "d_final"):
        _refused(L, fn, f"null {name}", _dc(L, **{name: None}))
    _refused(L, fn, "n < 0", _dc(L, n=-1))
    _refused(L, fn, "run_in < 0", _dc(L, run_in=-1))
    _refused(L, fn, "in place", _dc(L, d_out=P[0]))
    _refused(L, fn, "in_stride shorter than a row", _dc(L, in_stride=99))
    _refused(L, fn, "out_stride shorter than a row", _dc(L, out_stride=99))
    need = L.lib.sdrhip_dc_blocker_rows_workspace_bytes(3, 100)
    assert need >= 3 * 16
    _refused(L, fn, "a workspace one byte too small", _dc(L, ws=P[4], ws_bytes=need - 1))
    assert b"workspace" in L.lib.sdrhip_last_error()


def test_fm_demod_rows_refusals(L):
    fn = "sdrhip_fm_demod_run_rows"
    for rows in (0, -1, 1025):
        _refused(L, fn, f"rows = {rows}", _fm(L, rows=rows))
    for name in ("d_in", "d_out"):
        _refused(L, fn, f"null {name}", _fm(L, **{name: None}))
    _refused(L, fn, "k_end < k_begin (the one-row call refuses it)", _fm(L, k_begin=10, k_end=9))
    _refused(L, fn, "k_begin < in_base (the one-row call refuses it)", _fm(L, in_base=1))
    _refused(L, fn, "in_stride shorter than the row's samples in_base .. k_end", _fm(L, in_stride=198))
    _refused(L, fn, "... which counts from in_base, not k_begin", _fm(L, in_base=0, k_begin=50, k_end=101, in_stride=200))
    _refused(L, fn, "out_stride shorter than a row", _fm(L, out_stride=99))
    _refused(L, fn, "odd in_stride", _fm(L, in_stride=201))
    # the sdrhip_fm_demod_run refusals are the same two
    assert L.lib.sdrhip_fm_demod_run(None, P[0], 0, P[1], 10, 9, 0.0, 0.0) == ERR_ARG
    assert L.lib.sdrhip_fm_demod_run(None, P[0], 1, P[1], 0, 100, 0.0, 0.0) == ERR_ARG


def test_plan_hooks_refuse_and_workspace_bytes_of_no_rows_is_zero(L):
    for rows in (0, 1025):
        assert L.lib.sdrhip_debug_agc_rows_plan(rows, 100, 0.4, 0, None, None) == ERR_ARG
        assert L.lib.sdrhip_debug_dc_rows_plan(rows, 100, 0, None, None) == ERR_ARG
        assert L.lib.sdrhip_agc_rows_workspace_bytes(rows, 100) == 0 and L.lib.sdrhip_dc_blocker_rows_workspace_bytes(rows, 100) == 0
    assert L.lib.sdrhip_debug_agc_rows_plan(1, -1, 0.4, 0, None, None) == ERR_ARG
    assert L.lib.sdrhip_debug_dc_rows_plan(1, 100, -1, None, None) == ERR_ARG


def test_one_row_plans_are_the_one_row_hooks(L):
    """Over every size of iir_cases.CASES (its plan edges among them), one below and one above each, default and given run-ins."""
    seen = 0
    for case in IC.CASES:
        for n in {max(case.n - 1, 0), case.n, case.n + 1}:
            for run_in in {case.run_in, 0}:
                if case.op == "dc":
                    assert L.dc_rows_plan(1, n, run_in) == L.dc_plan(n, run_in), (case.name, n, run_in)
                else:
                    assert L.agc_rows_plan(1, n, case.mu, run_in) == L.agc_plan(n, case.mu, run_in), (case.name, n, run_in)
                seen += 1
    assert seen > 100
    for n in (1 << 20, (1 << 26) + 5):                              # where the one-row chunk itself has grown past the floor
        assert L.dc_rows_plan(1, n) == L.dc_plan(n) and L.agc_rows_plan(1, n, 0.4) == L.agc_plan(n, 0.4)


def test_rows_share_the_lane_cap_and_keep_the_route_edge(L):
    n = 1 << 16
    for plan, one in ((L.agc_rows_plan(1024, n, 0.4, 64), L.agc_plan(n, 0.4, 64)), (L.dc_rows_plan(1024, n, 64), L.dc_plan(n, 64))):
        chunks, C_, W = plan
        assert one[0] * 1024 > LANE_CAP, "the one-row plan would pass the cap: this is a case"
        assert chunks > 0 and chunks * 1024 <= LANE_CAP and chunks == -(-n // C_)
        assert C_ % 8 == 0 and C_ > one[1] and W == one[2]
        assert -(-n // (C_ - 8)) * 1024 > LANE_CAP, "a chunk 8 samples shorter would pass the cap: it grew no further than it had to"
    # below the cap nothing changes, whatever the rows
    for rows in (2, 32, 127):
        assert L.agc_rows_plan(rows, n, 0.4, 64) == L.agc_plan(n, 0.4, 64) and L.dc_rows_plan(rows, n, 64) == L.dc_plan(n, 64)
    # the route edge n == 2 W does not move with the rows
    for rows in (1, 3, 65, 1024):
        for W in (64, 1024):
            assert L.dc_rows_plan(rows, 2 * W - 1, W)[0] == 0 and L.dc_rows_plan(rows, 2 * W, W)[0] > 0
            assert L.agc_rows_plan(rows, 2 * W - 1, 0.4, W)[0] == 0 and L.agc_rows_plan(rows, 2 * W, 0.4, W)[0] > 0
    # the workspace covers the plan of any run-in: four words of statistics and thirteen bytes a chunk, per row
    for rows in (1, 3, 1024):
        for m in (1, 255, 4100, n, 1 << 20):
            for run_in in (8, 64, 0):
                a, d = L.agc_rows_plan(rows, m, 0.4, run_in), L.dc_rows_plan(rows, m, run_in)
                assert L.lib.sdrhip_agc_rows_workspace_bytes(rows, m) >= rows * (16 + 13 * a[0])
                assert L.lib.sdrhip_dc_blocker_rows_workspace_bytes(rows, m) >= rows * (16 + 13 * d[0])
