"""amDemod (sdrhip_am_demod_run, sdrhip_am_demod_run_rows, sdrhip_pipe_am_demod) on a host without a GPU: the names are declared,
exported and bound; every refusal comes back as SDRHIP_ERR_ARG under the function's own name before any pointer is looked at (the
pointers handed in here point nowhere) and moves no launch counter.  What the operator COMPUTES is held to agc_model.magnitude on
the device (tests/test_gpu_am_demod.py)."""
import ctypes as C
import os

import pytest

ERR_ARG = -1
NEW_SYMBOLS = ["sdrhip_am_demod_run", "sdrhip_am_demod_run_rows", "sdrhip_debug_am_demod_launches", "sdrhip_pipe_am_demod"]
P = [0x10000, 0x20000]                                  # never dereferenced: every call below is refused first


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
    assert L.lib.sdrhip_debug_am_demod_launches.restype is C.c_longlong
    assert L.am_demod_launches() >= 0
    for f in ("am_demod", "am_demod_rows", "am_demod_launches", "amDemod"):
        assert callable(getattr(L, f))
    assert callable(L.Pipe.am_demod)


def test_the_example_is_built_from_the_directory(L):
    from sdr_amd import build as Bld
    assert os.path.exists(os.path.join(Bld.EXAMPLES, "am_replay.c"))
    Bld.build_examples()
    assert os.access(os.path.join(Bld.EXAMPLES, "bin", "am_replay"), os.X_OK)


def _rows(L, d_in=P[0], in_stride=200, d_out=P[1], out_stride=100, rows=3, n=100):
    return L.lib.sdrhip_am_demod_run_rows(None, d_in, in_stride, d_out, out_stride, rows, n)


def _refused(L, fn, what, rc, counters):
    assert rc == ERR_ARG, f"{fn}: {what} is not refused"
    assert fn.encode() in L.lib.sdrhip_last_error(), f"{fn}: {what}: {L.lib.sdrhip_last_error()!r}"
    assert (L.am_demod_launches(), L.rows_launches()) == counters, f"{fn}: {what}: a refused call launched"


def test_rows_refusals_move_no_launch_counter(L):
    fn = "sdrhip_am_demod_run_rows"
    c = (L.am_demod_launches(), L.rows_launches())
    for rows in (0, -1, 1025):
        _refused(L, fn, f"rows = {rows}", _rows(L, rows=rows), c)
    for name in ("d_in", "d_out"):
        _refused(L, fn, f"null {name}", _rows(L, **{name: None}), c)
        _refused(L, fn, f"null {name} with n = 0", _rows(L, n=0, **{name: None}), c)
        _refused(L, fn, f"null {name} with one row", _rows(L, rows=1, **{name: None}), c)
    _refused(L, fn, "n < 0", _rows(L, n=-1), c)
    _refused(L, fn, "n < 0 with one row", _rows(L, rows=1, n=-1), c)
    _refused(L, fn, "in_stride shorter than a row", _rows(L, in_stride=198), c)
    _refused(L, fn, "a negative in_stride", _rows(L, in_stride=-200), c)
    _refused(L, fn, "odd in_stride", _rows(L, in_stride=201), c)
    _refused(L, fn, "out_stride shorter than a row", _rows(L, out_stride=99), c)
    _refused(L, fn, "a negative out_stride", _rows(L, out_stride=-100), c)
    _refused(L, fn, "2n past int64", _rows(L, n=2 ** 62, in_stride=2 ** 62, out_stride=2 ** 62), c)
    _refused(L, fn, "in place", _rows(L, d_out=P[0]), c)
    _refused(L, fn, "in place with one row", _rows(L, rows=1, d_out=P[0]), c)


def test_one_row_refusals_move_no_launch_counter(L):
    fn = "sdrhip_am_demod_run"
    c = (L.am_demod_launches(), L.rows_launches())
    run = L.lib.sdrhip_am_demod_run
    _refused(L, fn, "null d_in", run(None, None, P[1], 100), c)
    _refused(L, fn, "null d_out", run(None, P[0], None, 100), c)
    _refused(L, fn, "null d_in with n = 0", run(None, None, P[1], 0), c)
    _refused(L, fn, "n < 0", run(None, P[0], P[1], -1), c)
    _refused(L, fn, "in place", run(None, P[0], P[0], 100), c)
    with pytest.raises(L.SdrHipError, match="sdrhip_am_demod_run"):
        L.am_demod(P[0], -1, P[1])


def test_no_samples_is_ok_without_a_launch(L):
    """n == 0 returns before any device work: it needs no GPU."""
    c = L.am_demod_launches()
    assert L.lib.sdrhip_am_demod_run(None, P[0], P[1], 0) == 0
    assert _rows(L, n=0) == 0 and _rows(L, n=0, rows=1024, in_stride=0, out_stride=0) == 0
    assert L.am_demod_launches() == c


def test_pipe_create_refuses_a_null_handle(L):
    assert L.lib.sdrhip_pipe_am_demod(None) == ERR_ARG and b"sdrhip_pipe_am_demod" in L.lib.sdrhip_last_error()
