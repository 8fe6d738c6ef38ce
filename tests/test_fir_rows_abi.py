"""The FIR row forms (sdrhip_filter_run_rows, sdrhip_decimator_run_rows, sdrhip_resampler_run_rows) on a host without a GPU: the
names are declared, exported and bound; every refusal comes back as SDRHIP_ERR_ARG under the function's own name before any pointer
is looked at or any device work is done (the pointers handed in here point nowhere, and there is no device); route 1 on a shape the
banked kernel does not serve is refused, an empty range is SDRHIP_OK; and the rows plan of a long row is the tile plan_tile gives
k_split.  What the row forms COMPUTE is held to the one-row calls and the restated Pipes on the device (tests/test_gpu_fir_rows.py)."""
import ctypes as C
import os

import pytest

import fir_rows_cases as RC
import signals as S

OK, ERR_ARG = 0, -1
NEW_SYMBOLS = ["sdrhip_filter_run_rows", "sdrhip_decimator_run_rows", "sdrhip_resampler_run_rows", "sdrhip_debug_fir_rows_plan",
               "sdrhip_debug_fir_rows_launches", "sdrhip_debug_fir_rows_fixups"]
P = [0x10000, 0x20000]                                  # never dereferenced: every call below is refused (or empty) first


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
    assert L.lib.sdrhip_debug_fir_rows_launches.restype is C.c_longlong and L.lib.sdrhip_debug_fir_rows_fixups.restype is C.c_longlong
    assert L.fir_rows_launches() >= 0 and L.fir_rows_fixups() >= 0
    for cls in (L.Filter, L.Decimator, L.Resampler):
        assert callable(cls.run_rows)
    assert callable(L.fir_rows_plan)
    assert (L.FIR_ROWS_AUTO, L.FIR_ROWS_BANKED, L.FIR_ROWS_ROW_BY_ROW) == (0, 1, 2)


# ---- the three operators, with arguments that are fine: 3 rows of outputs [10, 110), in_base 5 ------------------------------------
class Op:
    def __init__(self, L, name, desc, fn, I, D, Lp, width, resampler=False):
        self.L, self.name, self.desc, self.fn, self.I, self.D, self.Lp, self.w, self.resampler = L, name, desc, fn, I, D, Lp, width, resampler
        last = -(-(109 * D) // I)
        self.need_in = (last + Lp // I - 5) * width     # floats a row holds from in_base on
        self.need_out = 100 * width
        self.seam_ok = 4096

    def call(self, **kw):
        a = dict(d_in=P[0], in_stride=self.need_in, in_base=5, d_out=P[1], out_stride=self.need_out, rows=3, k_begin=10, k_end=110,
                 seam_block=0, out_block=0, route=1)
        a.update(kw)
        args = [self.desc.h, None, a["d_in"], a["in_stride"], a["in_base"], a["d_out"], a["out_stride"], a["rows"], a["k_begin"],
                a["k_end"], a["seam_block"]] + ([a["out_block"]] if self.resampler else []) + [a["route"]]
        return self.fn(*args)

    def refused(self, what, **kw):
        rc = self.call(**kw)
        assert rc == ERR_ARG, f"{self.name}: {what} is not refused (rc {rc})"
        assert self.name.encode() in self.L.lib.sdrhip_last_error(), f"{self.name}: {what}: {self.L.lib.sdrhip_last_error()!r}"


@pytest.fixture(scope="module")
def ops(L):
    out = []
    f = L.Filter(S.gauss_taps(45, 1), L.ORDER_AVX, complex_=True)
    out.append(Op(L, "sdrhip_filter_run_rows", f, L.lib.sdrhip_filter_run_rows, 1, 1, f.num_coeffs, 2))
    d = L.Decimator(5, S.gauss_taps(61, 2), L.ORDER_AVX)
    out.append(Op(L, "sdrhip_decimator_run_rows", d, L.lib.sdrhip_decimator_run_rows, 1, 5, d.num_coeffs, 1))
    r = L.Resampler(3, 10, S.taps_example_audio_resampler(), L.ORDER_AVX)
    out.append(Op(L, "sdrhip_resampler_run_rows", r, L.lib.sdrhip_resampler_run_rows, 3, 10, r.num_coeffs, 1, resampler=True))
    return out


def test_refusals_come_before_any_pointer_is_looked_at(L, ops):
    for op in ops:
        for rows in (0, -1, 1025):
            op.refused(f"rows = {rows}", rows=rows)
        for route in (-1, 3):
            op.refused(f"route = {route}", route=route)
        op.refused("null d_in", d_in=None)
        op.refused("null d_out", d_out=None)
        op.refused("in place", d_out=P[0])
        op.refused("out_stride one float short of a row's outputs", out_stride=op.need_out - op.w)
        op.refused("in_stride one element short of the guaranteed inputs, counted from in_base", in_stride=op.need_in - op.w)
        op.refused("a negative stride", in_stride=-op.need_in)
        if op.w == 2:
            op.refused("odd in_stride on a complex side", in_stride=op.need_in + 1)
            op.refused("odd out_stride on a complex side", out_stride=op.need_out + 1)
            op.refused("odd stride with one row", rows=1, out_stride=op.need_out + 1)
        # what the one-row call refuses
        op.refused("k_end < k_begin", k_begin=10, k_end=9)
        op.refused("2^31 outputs", k_end=10 + (1 << 31))
        op.refused("the first window starts before d_in", in_base=int(-(-(10 * op.D) // op.I)) + 1)
        op.refused("a seam block shorter than the filter", seam_block=-(-op.Lp // op.I) - 1)
        if op.resampler:
            op.refused("k_begin < 0", k_begin=-1, in_base=-10)
        # with one row the strides' lengths are not looked at
        assert op.call(rows=1, in_stride=0, out_stride=0, k_begin=10, k_end=10) == OK
    # the one-row calls refuse the same
    f, d, r = (op.desc for op in ops)
    assert L.lib.sdrhip_filter_run(f.h, None, P[0], 5, P[1], 10, 9, 0) == ERR_ARG
    assert L.lib.sdrhip_decimator_run(d.h, None, P[0], 51, P[1], 10, 110, 0) == ERR_ARG
    assert L.lib.sdrhip_resampler_run(r.h, None, P[0], 5, P[1], 10, 110, 15, 0) == ERR_ARG
    for op in ops:
        assert op.fn(*([None, None, P[0], op.need_in, 5, P[1], op.need_out, 3, 10, 110, 0] + ([0] if op.resampler else []) + [1])) == ERR_ARG
        assert op.name.encode() in L.lib.sdrhip_last_error()


def test_an_empty_range_is_ok_and_touches_nothing(L, ops):
    for op in ops:
        for route in (0, 1, 2):
            assert op.call(k_begin=10, k_end=10, route=route) == OK
            assert op.call(k_begin=10, k_end=10, route=route, d_in=None, d_out=None, in_stride=0, out_stride=0) == OK
        op.refused("an empty range with rows = 0", k_begin=10, k_end=10, rows=0)
        op.refused("an empty range with route 3", k_begin=10, k_end=10, route=3)


def test_route_1_on_a_fallback_shape_is_refused(L):
    for fam in RC.FAMILIES:
        if fam.banked:
            continue
        desc = fam.make(L)
        assert L.fir_rows_plan(desc, 0, 100) is None
        lo = 0
        need_in = (-(-(99 * fam.D) // fam.I) + fam.Lp // fam.I) * fam.width
        if fam.kind == "resampler":
            fn, name = L.lib.sdrhip_resampler_run_rows, b"sdrhip_resampler_run_rows"
            rc = fn(desc.h, None, P[0], need_in, lo, P[1], 100 * fam.width, 3, 0, 100, 0, 0, 1)
        else:
            fn, name = L.lib.sdrhip_decimator_run_rows, b"sdrhip_decimator_run_rows"
            rc = fn(desc.h, None, P[0], need_in, lo, P[1], 100 * fam.width, 3, 0, 100, 0, 1)
        assert rc == ERR_ARG and name in L.lib.sdrhip_last_error() and b"route 1" in L.lib.sdrhip_last_error(), fam.name
    # seam_block < 0 (every output Cross) is a one-row shape only
    d = L.Decimator(5, S.gauss_taps(61, 2), L.ORDER_AVX)
    assert L.lib.sdrhip_decimator_run_rows(d.h, None, P[0], 1000, 0, P[1], 100, 3, 0, 100, -1, 1) == ERR_ARG
    assert b"route 1" in L.lib.sdrhip_last_error()
    assert L.fir_rows_plan(d, 0, 100, seam_block=-1) is None and L.fir_rows_plan(d, 0, 100) is not None
    # more than 64 chunks of lane-count taps
    long_ = L.Filter(S.gauss_taps(8 * 65, 3), L.ORDER_AVX)
    assert L.fir_rows_plan(long_, 0, 100) is None and L.fir_rows_plan(L.Filter(S.gauss_taps(8 * 64, 3), L.ORDER_AVX), 0, 100) is not None


def test_plan_hook_refuses_and_counts(L):
    d = L.Decimator(5, S.gauss_taps(61, 2), L.ORDER_AVX)
    p = (C.c_int * 6)()
    for args in ((None, 1, 1, 0, 100, 0), (d.h, 3, 1, 0, 100, 0), (d.h, 1, 0, 0, 100, 0), (d.h, 1, 1025, 0, 100, 0), (d.h, 1, 1, 100, 100, 0),
                 (d.h, 1, 1, -1, 100, 0)):
        assert L.lib.sdrhip_debug_fir_rows_plan(*args, p) == ERR_ARG, args
    assert L.lib.sdrhip_debug_fir_rows_plan(d.h, 1, 1, 0, 100, 0, None) == 1


def test_the_plan_of_a_long_row_is_plan_tile_s(L):
    """plan[4], plan[5] are what plan_tile gives k_split for one such row; a row of at least one such tile keeps it, whatever the
    rows, and a short row only ever shrinks it to its own cycles rounded up to a whole run of lanes."""
    for fam in RC.FAMILIES:
        if not fam.banked:
            continue
        desc = fam.make(L)
        G = 64 // fam.M
        for k0 in (0, 1, 2, 7):
            long_ = L.fir_rows_plan(desc, k0, k0 + (1 << 20))
            NN, U, NC = long_["split_cycles_per_tile"], long_["split_per_lane"], long_["per_cycle"]
            assert (long_["cycles_per_tile"], long_["per_lane"]) == (NN, U), (fam.name, long_)
            assert NN * NC <= 1024 and NN % (U * G) == 0
            for rows in (1, 3, 1024):
                for n in (NN * NC, NN * NC + 1, 5 * NN * NC - 1, 1 << 20):
                    p = L.fir_rows_plan(desc, k0, k0 + n, rows)
                    assert (p["cycles_per_tile"], p["per_lane"]) == (NN, U) == (p["split_cycles_per_tile"], p["split_per_lane"]), (fam.name, n, p)
                    assert p["tiles_per_row"] == -(-(-(-n // NC)) // NN)
            for n in (1, G * NC - 1, G * NC, G * NC + 1, 4 * 2 * G * NC - 1, 4 * 2 * G * NC, NN * NC - 1):
                p = L.fir_rows_plan(desc, k0, k0 + n, 33)
                cycles = -(-n // NC)
                u = 1 if cycles < 8 * G else 2
                assert p["per_lane"] == min(u, 2) and p["cycles_per_tile"] == min(NN, -(-cycles // (u * G)) * (u * G)), (fam.name, n, p)
                assert p["tiles_per_row"] == 1 and (p["split_cycles_per_tile"], p["split_per_lane"]) == (NN, U)
