"""The squelch (sdrhip_squelch_*) on a host without a GPU: the names are declared, exported and bound; the plan function follows the
stated auto rule on both sides of each edge; and every refusal comes back as SDRHIP_ERR_ARG under the function's own name before any
pointer is looked at (the pointers handed in here point nowhere) and moves no launch counter.  What the operator COMPUTES is held to
tests/squelch_model.py on the device (tests/test_gpu_squelch.py)."""
import ctypes as C
import math
import os

import pytest

import squelch_model as SM

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_squelch_rows_workspace_bytes", "sdrhip_squelch_run_rows", "sdrhip_squelch_run", "sdrhip_debug_squelch_plan",
               "sdrhip_debug_set_squelch_route", "sdrhip_debug_squelch_launches"]
P = [0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000, 0x70000]      # never dereferenced: every call below is refused first
WG, LS = 1, 2
ROWS_MAX = 1024


@pytest.fixture(scope="module")
def L():
    from sdr_amd import build as Bld
    if not os.path.exists(Bld.LIB):
        Bld.build()
    import sdr_amd.lib as L
    return L


@pytest.fixture(autouse=True)
def _auto_route(L):
    L.set_squelch_route(0)
    yield
    L.set_squelch_route(0)


def test_new_symbols_are_declared_exported_and_bound(L):
    from test_abi import declared_functions
    declared = declared_functions()
    product = C.CDLL(L.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert n in declared, f"{n} is not declared in sdr_hip.h"
        assert hasattr(product, n), f"{n} is not exported"
        assert getattr(L.lib, n).argtypes is not None, f"{n} is not bound in sdr_amd/lib.py"
    for f in ("squelch_run", "squelch_run_rows", "squelch_plan", "set_squelch_route", "squelch_launches"):
        assert callable(getattr(L, f))
    assert L.squelch_launches() >= 0


def test_the_plan_follows_the_auto_rule_on_both_sides_of_each_edge(L):
    # the edge in blocks: 1024 / 1025 blocks of 4 + 4 floats (32 KiB a row, far below the byte edge)
    assert L.squelch_plan(1, 1024, 4, False, 4) == (1, WG)
    assert L.squelch_plan(1, 1025, 4, False, 4) == (3, LS)
    assert L.squelch_plan(1, 1025, 4, False, 4, has_workspace=False) == (1, WG)
    assert L.squelch_plan(1, 1025, 4, False, 0) == (2, LS)                         # detect-only: no apply launch
    # the edge in bytes: detector plus signal of a row, 262144 bytes and 4 more
    assert L.squelch_plan(1, 64, 512, False, 512) == (1, WG)                       # 64 * (512 + 512) * 4 = 262144
    assert L.squelch_plan(1, 64, 512, False, 513) == (3, LS)
    assert L.squelch_plan(1, 64, 512, False, 513, has_workspace=False) == (1, WG)
    assert L.squelch_plan(1, 64, 256, True, 512) == (1, WG)                        # a complex detector sample is two floats
    assert L.squelch_plan(1, 64, 257, True, 512) == (3, LS)
    assert L.squelch_plan(1, 64, 1024, False, 0) == (1, WG) and L.squelch_plan(1, 64, 1025, False, 0) == (2, LS)
    assert L.squelch_plan(1, 0, 256, False, 256) == (1, WG)
    # the rule does not depend on the rows, and is the model's restatement of it
    for rows in (1, 3, ROWS_MAX):
        for nb, bd, cplx, bs in ((1, 1, 0, 1), (1024, 32, 0, 32), (1024, 32, 0, 33), (1025, 1, 0, 1), (1, 1 << 20, 1, 0), (16, 4096, 0, 1), (16, 4096, 0, 0)):
            for ws in (True, False):
                assert L.squelch_plan(rows, nb, bd, bool(cplx), bs, ws)[1] == SM.route(nb, bd, cplx, bs, ws), (rows, nb, bd, cplx, bs, ws)
    # forced routes
    L.set_squelch_route(WG)
    assert L.squelch_plan(1, 1 << 20, 256, False, 256) == (1, WG)
    L.set_squelch_route(LS)
    assert L.squelch_plan(1, 4, 256, False, 256) == (3, LS) and L.squelch_plan(1, 0, 256, False, 256) == (1, WG)
    with pytest.raises(L.SdrHipError, match="sdrhip_debug_squelch_plan"):
        L.squelch_plan(1, 4, 256, False, 256, has_workspace=False)
    L.set_squelch_route(7)                                                         # anything else is auto
    assert L.squelch_plan(1, 4, 256, False, 256) == (1, WG)


def test_plan_refusals(L):
    plan = L.lib.sdrhip_debug_squelch_plan
    for args in ((0, 4, 256, 0, 256, 1), (ROWS_MAX + 1, 4, 256, 0, 256, 1), (1, -1, 256, 0, 256, 1), (1, 4, 0, 0, 256, 1),
                 (1, 4, (1 << 20) + 1, 0, 256, 1), (1, 4, 256, 2, 256, 1), (1, 4, 256, 0, -1, 1), (1, 4, 256, 0, (1 << 20) + 1, 1),
                 (1, (1 << 40) + 1, 1, 0, 0, 1), (1, 1 << 40, 1, 1, 0, 1), (1, 1 << 40, 1, 0, 2, 1), (1, 1 << 62, 1 << 20, 0, 1, 1)):
        assert plan(*args, None) == ERR_ARG and b"sdrhip_debug_squelch_plan" in L.lib.sdrhip_last_error(), args
    assert plan(1, 1 << 40, 1, 0, 1, 1, None) == 3


def test_workspace_bytes(L):
    ws = L.lib.sdrhip_squelch_rows_workspace_bytes
    assert ws(0, 100) == 0 and ws(ROWS_MAX + 1, 100) == 0 and ws(1, -1) == 0
    for rows, nb in ((1, 0), (1, 1), (3, 1025), (ROWS_MAX, 4096)):
        assert rows * nb * 5 <= ws(rows, nb) <= rows * nb * 5 + 64, (rows, nb)


def _rows(L, d_det=P[0], det_stride=1000, det_complex=0, block_det=10, d_in=P[1], in_stride=1000, d_out=P[2], out_stride=1000, block_sig=10,
          rows=3, n_blocks=100, open_level=1.0, close_level=0.25, hang=2, open_above=1, d_state=P[3], d_final=P[4], d_levels=None, d_gates=None,
          ws=None, ws_bytes=0):
    return L.lib.sdrhip_squelch_run_rows(None, d_det, det_stride, det_complex, block_det, d_in, in_stride, d_out, out_stride, block_sig, rows,
                                         n_blocks, open_level, close_level, hang, open_above, d_state, d_final, d_levels, d_gates, ws, ws_bytes)


def _one(L, d_det=P[0], det_complex=0, block_det=10, d_in=P[1], d_out=P[2], block_sig=10, n_blocks=100, open_level=1.0, close_level=0.25, hang=2,
         open_above=1, det=0, hang_left=0, d_final=P[4], d_levels=None, d_gates=None, ws=None, ws_bytes=0):
    return L.lib.sdrhip_squelch_run(None, d_det, det_complex, block_det, d_in, d_out, block_sig, n_blocks, open_level, close_level, hang,
                                    open_above, det, hang_left, d_final, d_levels, d_gates, ws, ws_bytes)


def _refused(L, fn, what, rc, launches):
    assert rc == ERR_ARG, f"{fn}: {what} is not refused"
    assert fn.encode() in L.lib.sdrhip_last_error(), f"{fn}: {what}: {L.lib.sdrhip_last_error()!r}"
    assert L.squelch_launches() == launches, f"{fn}: {what}: a refused call launched"


BAD_LEVELS = (-0.25, math.nan, math.inf, -math.inf)


def _common_refusals(L, fn, call, c, rows):
    for bd in (0, -1, (1 << 20) + 1):
        _refused(L, fn, f"block_det = {bd}", call(L, block_det=bd), c)
        _refused(L, fn, f"block_sig = {bd}", call(L, block_sig=bd), c)
    _refused(L, fn, "n_blocks < 0", call(L, n_blocks=-1), c)
    _refused(L, fn, "a detector row longer than 2^40 floats", call(L, n_blocks=(1 << 21), block_det=1 << 20), c)
    _refused(L, fn, "a signal row longer than 2^40 floats", call(L, n_blocks=(1 << 21), block_det=1, block_sig=1 << 20), c)
    _refused(L, fn, "n_blocks that overflows the products", call(L, n_blocks=1 << 62, block_det=4, block_sig=4), c)
    for v in BAD_LEVELS:
        _refused(L, fn, f"open_level = {v}", call(L, open_level=v), c)
        _refused(L, fn, f"close_level = {v}", call(L, close_level=v), c)
    _refused(L, fn, "close above open with open_above = 1", call(L, open_level=0.25, close_level=1.0), c)
    _refused(L, fn, "close below open with open_above = 0", call(L, open_level=1.0, close_level=0.25, open_above=0), c)
    for h in (-1, (1 << 30) + 1):
        _refused(L, fn, f"hang = {h}", call(L, hang=h), c)
    for v in (-1, 2):
        _refused(L, fn, f"open_above = {v}", call(L, open_above=v), c)
        _refused(L, fn, f"det_complex = {v}", call(L, det_complex=v), c)
    _refused(L, fn, "null d_det", call(L, d_det=None), c)
    _refused(L, fn, "null d_det, detect-only", call(L, d_det=None, d_in=None, d_out=None), c)
    _refused(L, fn, "null d_det with n_blocks = 0", call(L, d_det=None, n_blocks=0), c)
    _refused(L, fn, "null d_in alone", call(L, d_in=None), c)
    _refused(L, fn, "null d_out alone", call(L, d_out=None), c)
    _refused(L, fn, "d_out == d_det without d_in == d_det", call(L, d_out=P[0]), c)
    _refused(L, fn, "in place on the detector with other block lengths", call(L, d_in=P[0], d_out=P[0], block_sig=5), c)
    _refused(L, fn, "in place on a complex detector", call(L, d_in=P[0], d_out=P[0], det_complex=1, block_det=5), c)
    need = L.lib.sdrhip_squelch_rows_workspace_bytes(rows, 100)
    _refused(L, fn, "a workspace one byte short", call(L, ws=P[5], ws_bytes=need - 1), c)
    _refused(L, fn, "a workspace of no bytes", call(L, ws=P[5], ws_bytes=0), c)
    L.set_squelch_route(LS)
    _refused(L, fn, "forced LS without a workspace", call(L), c)
    _refused(L, fn, "forced LS without a workspace, detect-only", call(L, d_in=None, d_out=None), c)
    L.set_squelch_route(0)


def test_rows_refusals_move_no_launch_counter(L):
    fn, c = "sdrhip_squelch_run_rows", L.squelch_launches()
    for rows in (0, -1, ROWS_MAX + 1):
        _refused(L, fn, f"rows = {rows}", _rows(L, rows=rows), c)
    _common_refusals(L, fn, _rows, c, 3)
    _refused(L, fn, "det_stride shorter than a row", _rows(L, det_stride=999), c)
    _refused(L, fn, "det_stride shorter than a complex row", _rows(L, det_complex=1, det_stride=1998), c)
    _refused(L, fn, "in_stride shorter than a row", _rows(L, in_stride=999), c)
    _refused(L, fn, "out_stride shorter than a row", _rows(L, out_stride=999), c)
    _refused(L, fn, "a negative stride", _rows(L, in_stride=-1000), c)
    _refused(L, fn, "an odd det_stride with a complex detector", _rows(L, det_complex=1, det_stride=2001), c)
    _refused(L, fn, "an odd det_stride with a complex detector and one row", _rows(L, rows=1, det_complex=1, det_stride=2001), c)
    _refused(L, fn, "in place with out_stride != in_stride", _rows(L, d_out=P[1], out_stride=1004), c)
    _refused(L, fn, "in place on the detector with det_stride != in_stride", _rows(L, d_in=P[0], d_out=P[0], det_stride=1004), c)


def test_one_row_refusals_move_no_launch_counter(L):
    fn, c = "sdrhip_squelch_run", L.squelch_launches()
    _common_refusals(L, fn, _one, c, 1)
