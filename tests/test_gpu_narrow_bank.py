"""GPU parity of the narrow-channel bank (sdrhip_narrow_bank_*): tuner -> firDecimator D1 -> firDecimator D2 -> magnitude [-> dcBlocker]
or fmDemod for every channel of one capture.  Rows are held to the models (tests/narrow_bank_cases.py: the restated Pipes alone,
independent of the product), to the composition driven by hand through the C ABI, and the three routes to each other.  Every
comparison is bit for bit, NaN by position; every output buffer starts as NaN canaries and every float between and around the rows
is a canary still afterwards."""
import threading

import numpy as np
import pytest

import am_bank_cases as AC
import narrow_bank_cases as NB
import nfm_bank_cases as NC
import signals as S
import test_gpu_tuner as T
import tuner_bank_cases as BC
import tuner_i16_cases as IC
import tuner_model as TM
from conftest import assert_bit_equal
from gpu_util import CANARY, dev_empty_f32, ptr, to_dev, to_host
from oracle import pipes_model as PM

pytestmark = pytest.mark.gpu

B, ENV, FM, TILE = NB.B, NB.ENV, NB.FM, NB.TILE
ROUTES = (1, 2, 0)
FORMS = [(ENV, False), (ENV, True), (FM, False)]
FORM_IDS = ["env", "env-dc", "fm"]


def r4(n):
    return (n + 3) // 4 * 4


def device_inputs(oracle):
    u8 = T.stream_u8()
    return {"u8": to_dev(u8), "cf32": to_dev(oracle.convert_u8(u8)), "i16": to_dev(IC.stream_i16())}


def counters(hip):
    """[narrow kernel, FIR rows tile, FIR rows fix-up, amDemod, rows (dcBlocker and fmDemod rows), AM bank tile, NFM bank tile]"""
    return np.array([hip.narrow_bank_launches(), hip.fir_rows_launches(), hip.fir_rows_fixups(), hip.am_demod_launches(), hip.rows_launches(),
                     hip.am_bank_launches(), hip.nfm_bank_launches()], np.int64)


def make(hip, shape, form, dc, tables, order=None):
    taps, d2, _ = NB.SHAPES[shape]
    tb = hip.TunerBank(NB.D1, S.taps_decim127(), tables)
    dec = hip.Decimator(d2, taps, hip.ORDER_AVX if order is None else order, complex_=True)
    return hip.NarrowBank(tb, dec, form, dc)


def _edges(count, cuts):
    return [0] + [c for c in cuts if 0 < c < count] + [count]


def _rows_of(out, nch, count, stride, base):
    whole = to_host(out).view(np.uint32)                       # (checks the guard bands around the buffer)
    mask = np.zeros(whole.size, bool)
    for j in range(nch):
        mask[base + j * stride:base + j * stride + count] = True
    assert (whole[~mask] == CANARY).all(), f"{int((whole[~mask] != CANARY).sum())} floats between or around the rows were written"
    return np.stack([whole[base + j * stride:base + j * stride + count] for j in range(nch)]).view(np.float32)


def run_nb(hip, nb, fmt, d_in, count, seam, seam2, cuts=(), k0=0, in_base=0, stride=None, base=0, fm_state=None, dc_state=None, stream=None,
           d_in_ptr=None):
    """Outputs [k0, k0 + count) of every channel as runs cut at k0 + cuts: the fm state arrays swapped between the runs (fm_state None
    = a null d_state for the first run), the dc state array reused -> (rows [channels, count], final fm pairs or None, final dc
    state or None)."""
    import torch
    nch, fm, dc = nb.channels, nb.form == FM, nb.dc_block
    stride = count if stride is None else stride
    out = dev_empty_f32(base + nch * stride + 5)
    st = [to_dev(np.ascontiguousarray(np.zeros((nch, 2)) if fm_state is None else fm_state, np.float32).reshape(-1)), dev_empty_f32(2 * nch)]
    dcs = to_dev(np.ascontiguousarray(np.zeros((nch, 2)) if dc_state is None else dc_state, np.float32).reshape(-1)) if dc else None
    run = {"cf32": nb.run, "u8": nb.run_u8, "i16": nb.run_i16}[fmt]
    edges = _edges(count, cuts)
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        wsb = nb.workspace_bytes(b - a)
        ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
        first = (None if (i == 0 and fm_state is None) else ptr(st[i & 1])) if fm else None
        run(ptr(d_in) if d_in_ptr is None else d_in_ptr, in_base, ptr(out) + 4 * (base + a), stride, k0 + a, k0 + b, seam, seam2, first,
            ptr(st[(i + 1) & 1]) if fm else None, ptr(dcs) if dc else None, ptr(ws), wsb, stream)
        torch.cuda.synchronize()                               # (the workspace of this run is dropped at the next iteration)
    rows = _rows_of(out, nch, count, stride, base)
    return rows, to_host(st[(len(edges) - 1) & 1]).reshape(nch, 2) if fm else None, to_host(dcs).reshape(nch, 2) if dc else None


def compose(hip, nb, fmt, d_in, count, seam, seam2, k0=0, in_base=0, fm_state=None, dc_state=None):
    """The same outputs by the calls a caller makes without the object: TunerBank.run*, sdrhip_decimator_run_rows (route 0),
    sdrhip_am_demod_run_rows | sdrhip_fm_demod_run_rows, sdrhip_dc_blocker_run_rows."""
    import torch
    nch, fm, dc = nb.channels, nb.form == FM, nb.dc_block
    tb, dec = nb.tuner_bank, nb.decimator
    j0, j1 = nb.stage1_range(k0, k0 + count)
    np1, npo = r4(j1 - j0), r4(count)
    iq1 = torch.zeros(nch * 2 * np1, dtype=torch.float32, device="cuda")
    iq2 = torch.zeros(nch * 2 * npo, dtype=torch.float32, device="cuda")
    {"cf32": tb.run, "u8": tb.run_u8, "i16": tb.run_i16}[fmt](ptr(d_in), in_base, ptr(iq1), 2 * np1, j0, j1, seam)
    hip.check(hip.lib.sdrhip_decimator_run_rows(dec.h, None, ptr(iq1), 2 * np1, j0, ptr(iq2), 2 * npo, nch, k0, k0 + count, seam2, 0),
              "sdrhip_decimator_run_rows")
    out = dev_empty_f32(nch * count)
    fin = None
    if fm:
        st = None if fm_state is None else to_dev(np.ascontiguousarray(fm_state, np.float32).reshape(-1))
        fin = dev_empty_f32(2 * nch)
        hip.check(hip.lib.sdrhip_fm_demod_run_rows(None, ptr(iq2), 2 * npo, k0, ptr(out), count, nch, k0, k0 + count,
                                                   None if st is None else ptr(st), ptr(fin)), "sdrhip_fm_demod_run_rows")
        return to_host(out).reshape(nch, count), to_host(fin).reshape(nch, 2), None
    if not dc:
        hip.check(hip.lib.sdrhip_am_demod_run_rows(None, ptr(iq2), 2 * npo, ptr(out), count, nch, count), "sdrhip_am_demod_run_rows")
        return to_host(out).reshape(nch, count), None, None
    env = torch.zeros(nch * npo, dtype=torch.float32, device="cuda")
    hip.check(hip.lib.sdrhip_am_demod_run_rows(None, ptr(iq2), 2 * npo, ptr(env), npo, nch, count), "sdrhip_am_demod_run_rows")
    dcs = to_dev(np.ascontiguousarray(np.zeros((nch, 2)) if dc_state is None else dc_state, np.float32).reshape(-1))
    wsb = hip.lib.sdrhip_dc_blocker_rows_workspace_bytes(nch, count)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    hip.check(hip.lib.sdrhip_dc_blocker_run_rows(None, ptr(env), npo, ptr(out), count, nch, count, ptr(dcs), ptr(dcs), ptr(ws), wsb, 0),
              "sdrhip_dc_blocker_run_rows")
    return to_host(out).reshape(nch, count), None, to_host(dcs).reshape(nch, 2)


def states_before(oracle, tables, shape, seam, seam2, fmt, form, dc, k):
    fm = [NB.fm_state_before(oracle, t, shape, seam, seam2, fmt, k) for t in tables] if form == FM else None
    dcs = [NB.dc_state_before(oracle, t, shape, seam, seam2, fmt, k) for t in tables] if dc else None
    return fm, dcs


def counts_for(n_all, k0):
    """n_all: the outputs the model holds (a last block shorter than the filter yields none: fewer than NB.n_out with short blocks)"""
    n = n_all - k0
    return [c for c in (1, 2, TILE - 2, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE + 1) if c <= n] + [n]


# ---- 1: shapes, forms, routes, counts, seams, formats, channels, counters -------------------------------------------------------
@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("shape", list(NB.SHAPES))
def test_forms_routes_counts_and_seams(hip, oracle, shape, form, dc):
    """Counts around the tile (256 outputs; the fmDemod form advances by 255) on every seam pair, from a run that STARTS on a Cross
    output of stage 2 where there is one; the launch counters of routes 1 and 2."""
    ins = device_inputs(oracle)
    for nch in (1, 3):
        tables = BC.bank_tables(nch)
        nb = make(hip, shape, form, dc, tables)
        for fmt in NB.FORMATS:
            for seam, seam2 in NB.SEAM_PAIRS:
                s2 = NB.seam2_of(shape, seam2)
                cross = NB.cross2(shape, seam2)
                k0 = int(cross[0]) if cross.size else 0
                model = NB.model_defined(shape, seam2)
                exp = [NB.expected(oracle, t, shape, seam, seam2, fmt, form, dc) for t in tables]
                fm0, dc0 = states_before(oracle, tables, shape, seam, seam2, fmt, form, dc, k0) if model else (None, None)
                full = (seam, seam2) in ((B, 1024), (0, "Lp")) and (nch == 3 or fmt == "u8")
                n_all = exp[0].size if model else NB.n_out(shape)
                for count in counts_for(n_all, k0) if full else [min(TILE + 1, n_all - k0)]:
                    what = f"{shape}, form {form}, dc {dc}, {nch} channels, seams ({seam}, {s2}), {fmt}, {count} outputs from {k0}"
                    got = {}
                    for route in ROUTES:
                        nb.set_route(route)
                        c0 = counters(hip)
                        rows, fin, dcf = run_nb(hip, nb, fmt, ins[fmt], count, seam, s2, k0=k0, fm_state=fm0, dc_state=dc0)
                        d = counters(hip) - c0
                        if route == 1:
                            assert d[0] == 1 and not d[1:4].any() and not d[5:].any() and (d[4] > 0) == dc, what + f": route 1 {d}"
                        if route == 2:
                            assert d[0] == 0 and not d[5:].any() and d[4 if form == FM or dc else 3] >= 1, what + f": route 2 {d}"
                        got[route] = (rows, fin, dcf)
                        if model:
                            for j, t in enumerate(tables):
                                assert_bit_equal(rows[j], exp[j][k0:k0 + count], what + f", route {route}: channel {j}")
                                if form == FM:
                                    assert_bit_equal(fin[j], NB.fm_state_before(oracle, t, shape, seam, seam2, fmt, k0 + count),
                                                     what + f", route {route}: d_final {j}")
                                if dc:
                                    assert_bit_equal(dcf[j], NB.dc_state_before(oracle, t, shape, seam, seam2, fmt, k0 + count),
                                                     what + f", route {route}: dc state {j}")
                    hand = compose(hip, nb, fmt, ins[fmt], count, seam, s2, k0=k0, fm_state=fm0, dc_state=dc0)
                    for route in ROUTES:
                        for a, b, name in zip(got[route], hand, ("rows", "d_final", "dc state")):
                            if b is not None:
                                assert_bit_equal(a, b, what + f": route {route} against the calls by hand: {name}")


@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_32_channels(hip, oracle, form, dc):
    tables = BC.bank_tables(32)
    nb = make(hip, "24/4", form, dc, tables)
    ins = device_inputs(oracle)
    count = 2 * TILE + 1
    for fmt in NB.FORMATS:
        for route in ROUTES:
            nb.set_route(route)
            rows, _, _ = run_nb(hip, nb, fmt, ins[fmt], count, B, 1024)
            for j, t in enumerate(tables):
                assert_bit_equal(rows[j], NB.expected(oracle, t, "24/4", B, 1024, fmt, form, dc)[:count], f"{fmt}, route {route}: channel {j} of 32")


# ---- 2: state and stream position -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("seam,seam2", [(0, 0), (B, 1024), (B, 1000)])
def test_cut_streams_equal_one_run(hip, oracle, seam, seam2, form, dc):
    """[0, N) whole and as three and five consecutive runs (one of ONE output) that swap the fm state arrays or reuse the dc state."""
    tables = BC.bank_tables(3)
    ins = device_inputs(oracle)
    for shape in ("24/4", "61/5"):
        nb = make(hip, shape, form, dc, tables)
        n = NB.n_out(shape)
        for fmt in ("u8", "i16"):
            for route in (1, 2):
                nb.set_route(route)
                for cuts in ([], [255, 601], [1, 255, 256, 601]):
                    rows, fin, dcf = run_nb(hip, nb, fmt, ins[fmt], n, seam, seam2, cuts)
                    for j, t in enumerate(tables):
                        what = f"{shape}, {fmt}, seams ({seam}, {seam2}), route {route}, cuts {cuts}: channel {j}"
                        assert_bit_equal(rows[j], NB.expected(oracle, t, shape, seam, seam2, fmt, form, dc), what)
                        if form == FM:
                            assert_bit_equal(fin[j], NB.fm_state_before(oracle, t, shape, seam, seam2, fmt, n), what + " d_final")
                        if dc:
                            assert_bit_equal(dcf[j], NB.dc_state_before(oracle, t, shape, seam, seam2, fmt, n), what + " dc state")


@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("k0", [0, 1, 601])
def test_k_begin_from_exactly_the_receptive_field(hip, oracle, k0, form, dc):
    """The device buffer holds exactly the samples the run may read, with the bit-flipped stream in front of and behind them."""
    shape, seam, seam2, count = "24/4", B, 1024, TILE + 1
    tables = BC.bank_tables(3)
    nb = make(hip, shape, form, dc, tables)
    j0, j1 = nb.stage1_range(k0, k0 + count)
    s0, s1 = j0 * NB.D1, (j1 - 1) * NB.D1 + NB.LP1
    u8 = T.stream_u8()
    pad = 64                                                   # samples: the slice stays 16-byte aligned for every format
    for fmt, full in (("u8", u8), ("cf32", oracle.convert_u8(u8)), ("i16", IC.stream_i16())):
        a = np.asarray(full).reshape(-1, 2)
        flipped = (a.view(np.uint8) ^ 0xFF).view(a.dtype).reshape(a.shape)
        buf = np.concatenate([flipped[max(s0 - pad, 0):s0][-pad:] if s0 else flipped[:0], a[s0:s1], flipped[s1:s1 + pad]])
        lead = min(pad, s0)
        d = to_dev(np.ascontiguousarray(buf).reshape(-1))
        itemsize = a.dtype.itemsize * 2
        fm0, dc0 = states_before(oracle, tables, shape, seam, seam2, fmt, form, dc, k0)
        for route in ROUTES:
            nb.set_route(route)
            rows, _, _ = run_nb(hip, nb, fmt, d, count, seam, seam2, k0=k0, in_base=s0, fm_state=fm0, dc_state=dc0,
                                d_in_ptr=ptr(d) + lead * itemsize)
            for j, t in enumerate(tables):
                assert_bit_equal(rows[j], NB.expected(oracle, t, shape, seam, seam2, fmt, form, dc)[k0:k0 + count],
                                 f"{fmt}, route {route}, k_begin {k0}: channel {j}")


@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_far_stream_position(hip, oracle, form, dc):
    """k_begin = 3 * 2^30 + 5 of STAGE 2: stage-1 outputs beyond 2^33, samples beyond 2^36; the device holds only the slice."""
    shape, seam, seam2 = "24/4", B, 1024
    k_begin = BC.FAR_K0
    ns = 2 * B + 1000
    u8 = T.stream_u8()[:2 * ns]
    tables = [T.osc_table(1000), T.osc_table(5)]
    in_base, iq2 = NB.far_case(oracle, shape, seam, seam2, tables, k_begin, u8)
    assert in_base == k_begin * 4 * 8
    n = iq2[0].size // 2
    assert n > TILE + 1
    fm_state = np.array([[0.25, -0.5], [1.5, 2.0]], np.float32)
    dc_state = np.array([[0.5, -0.25], [0.0, 1.0]], np.float32)
    exp = [NB.demodulate(oracle, q, form, dc, fm_state[j], dc_state[j]) for j, q in enumerate(iq2)]
    nb = make(hip, shape, form, dc, tables)
    for fmt, d_in in (("u8", to_dev(u8)), ("cf32", to_dev(oracle.convert_u8(u8)))):
        for route in ROUTES:
            nb.set_route(route)
            for cuts in ([], [100, 257]):
                rows, fin, _ = run_nb(hip, nb, fmt, d_in, n, seam, seam2, cuts, k0=k_begin, in_base=in_base, fm_state=fm_state, dc_state=dc_state)
                for j in range(2):
                    assert_bit_equal(rows[j], exp[j], f"{fmt}, route {route}, cuts {cuts}: channel {j}")
                    if form == FM:
                        assert_bit_equal(fin[j], iq2[j][-2:], f"{fmt}, route {route}, cuts {cuts}: d_final {j}")


# ---- 3: rows and addresses ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
@pytest.mark.parametrize("extra", [0, 1, 5])
def test_out_strides_and_bases(hip, oracle, extra, form, dc):
    tables = BC.bank_tables(3)
    nb = make(hip, "61/5", form, dc, tables)
    d_in = device_inputs(oracle)["u8"]
    n = NB.n_out("61/5")
    for base in (0, 1, 3):
        for route in (1, 2):
            nb.set_route(route)
            rows, _, _ = run_nb(hip, nb, "u8", d_in, n, B, 1000, [255, 601], stride=n + extra, base=base)
            for j, t in enumerate(tables):
                assert_bit_equal(rows[j], NB.expected(oracle, t, "61/5", B, 1000, "u8", form, dc),
                                 f"route {route}, stride n + {extra}, base {4 * base} bytes: channel {j}")


# ---- 4: what route 1 does not serve -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_an_sse_order_second_decimator(hip, oracle, form, dc):
    """A 4-tap-chunk SSE-order decimator2: route 1 refuses it and writes nothing, auto composes it, and the bits are the composition's."""
    import torch
    tables = BC.bank_tables(3)
    nb = make(hip, "24/4", form, dc, tables, order=hip.ORDER_SSE)
    d_in = device_inputs(oracle)["u8"]
    n = TILE + 1
    nb.set_route(1)
    out = dev_empty_f32(3 * n)
    ws = torch.empty(nb.workspace_bytes(n) + nb.workspace_bytes(n), dtype=torch.uint8, device="cuda")
    dcs = to_dev(np.full(6, 0.5, np.float32))
    c0 = counters(hip)
    with pytest.raises(hip.SdrHipError):
        nb.run_u8(ptr(d_in), 0, ptr(out), n, 0, n, B, 1024, None, None, ptr(dcs) if dc else None, ptr(ws), ws.numel())
    assert (to_host(out).view(np.uint32) == CANARY).all() and (to_host(dcs) == 0.5).all(), "a refused run wrote"
    assert (counters(hip) == c0).all()
    got = {}
    for route in (0, 2):
        nb.set_route(route)
        c0 = counters(hip)
        got[route] = run_nb(hip, nb, "u8", d_in, n, B, 1024)
        assert (counters(hip) - c0)[0] == 0
    hand = compose(hip, nb, "u8", d_in, n, B, 1024)
    for route in (0, 2):
        for a, b in zip(got[route], hand):
            if b is not None:
                assert_bit_equal(a, b, f"SSE order, route {route} against the calls by hand")
    # the SSE order shows in the bits: the same taps in the AVX order give another row
    avx = make(hip, "24/4", form, dc, tables)
    avx.set_route(2)
    assert not np.array_equal(run_nb(hip, avx, "u8", d_in, n, B, 1024)[0].view(np.uint32), got[2][0].view(np.uint32))


# ---- 5: value classes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_subnormal_products_and_signed_zeros(hip, oracle, form, dc):
    """The sparse cfloat stream under the subnormal / -0 oscillator table: every product under the first FIR sum is subnormal or a
    signed zero, and the second decimator sums those."""
    shape, seam, seam2 = "24/4", B, 1024
    tables = [BC.SUBNORMALS, BC.IDENTITY]
    d_in = to_dev(AC.sparse_stream())
    nb = make(hip, shape, form, dc, tables)
    exp = []
    for t in tables:
        iq2 = NB.decimate2(oracle, shape, AC.sparse_expected_iq(oracle, t, seam), seam2)
        exp.append(NB.demodulate(oracle, iq2, form, dc))
    n = exp[0].size
    assert n == NB.n_out(shape, AC.SPARSE_OUT)
    for route in ROUTES:
        nb.set_route(route)
        rows, _, _ = run_nb(hip, nb, "cf32", d_in, n, seam, seam2, [TILE])
        for j in range(2):
            assert_bit_equal(rows[j], exp[j], f"route {route}: channel {j}")


@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_inf_and_nan_samples(hip, oracle, form, dc):
    shape, seam, seam2 = "61/5", B, 1000
    tables = [T.osc_table(1000), BC.IDENTITY, T.osc_table(5)]
    d_in = to_dev(AC.nonfinite_stream(oracle))
    nb = make(hip, shape, form, dc, tables)
    for route in ROUTES:
        nb.set_route(route)
        rows, _, _ = run_nb(hip, nb, "cf32", d_in, NB.n_out(shape), seam, seam2, [601])
        for j, t in enumerate(tables):
            iq1 = TM.tuner_expected(oracle, S.taps_decim127(), PM.ORDER_AVX, 8, AC.nonfinite_stream(oracle), t, seam, 0, block_out=1)
            e = NB.demodulate(oracle, NB.decimate2(oracle, shape, iq1, seam2), form, dc)
            nan = np.isnan(e)
            assert nan.any() and not nan.all()
            assert np.array_equal(np.isnan(rows[j]), nan), f"route {route}: channel {j}: NaN positions"
            assert_bit_equal(rows[j][~nan], e[~nan], f"route {route}: channel {j}")


@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_silent_u8_stretches(hip, oracle, form, dc):
    """The directed u8 stream: all-zero stage-1 windows at the start and across a stage-1 tile edge, hence all-zero stage-2 windows:
    magnitude 0 and phase(0) of both zero signs."""
    shape, seam, seam2 = "24/4", B, 1024
    tables = NC.directed_tables()
    nb = make(hip, shape, form, dc, tables)
    d_in = to_dev(NC.directed_u8())
    iq2 = NB.expected_iq2(oracle, tables[1], shape, seam, seam2, "u8", stream="directed")
    zero = (iq2[0::2] == 0) & (iq2[1::2] == 0)
    assert zero[0] and zero[1:].any(), "all-zero stage-2 windows at the start and later"
    for route in ROUTES:
        nb.set_route(route)
        rows, _, _ = run_nb(hip, nb, "u8", d_in, NB.n_out(shape), seam, seam2, [255])
        for j, t in enumerate(tables):
            assert_bit_equal(rows[j], NB.expected(oracle, t, shape, seam, seam2, "u8", form, dc, stream="directed"), f"route {route}: channel {j}")


# ---- 6: refusals and edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc", FORMS, ids=FORM_IDS)
def test_run_time_refusals_write_nothing(hip, oracle, form, dc):
    import torch
    nb = make(hip, "24/4", form, dc, BC.bank_tables(3))
    d_in = device_inputs(oracle)["u8"]
    n = 64
    st = to_dev(np.full(12, 0.5, np.float32))
    dcs = to_dev(np.full(6, 0.5, np.float32))
    s0, s1 = (ptr(st), ptr(st) + 24) if form == FM else (None, None)
    pdc = ptr(dcs) if dc else None
    c0 = counters(hip)
    for route in ROUTES:
        nb.set_route(route)
        wsb = nb.workspace_bytes(n)
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        out = dev_empty_f32(3 * n)

        def refused(what, *args):
            assert hip.lib.sdrhip_narrow_bank_run_u8(nb.h, None, *args) == -1, f"route {route}: {what}"
            assert b"sdrhip_narrow_bank_run" in hip.lib.sdrhip_last_error(), what
            clean = (to_host(out).view(np.uint32) == CANARY).all() and (to_host(st) == 0.5).all() and (to_host(dcs) == 0.5).all()
            assert clean, f"route {route}: {what}: a refused run wrote"

        refused("a null workspace", ptr(d_in), 0, ptr(out), n, 0, n, B, 1024, s0, s1, pdc, None, wsb)
        refused("a workspace one byte short", ptr(d_in), 0, ptr(out), n, 0, n, B, 1024, s0, s1, pdc, ptr(ws), wsb - 1)
        refused("a workspace off 16 bytes", ptr(d_in), 0, ptr(out), n, 0, n, B, 1024, s0, s1, pdc, ptr(ws) + 4, wsb)
        refused("rows would overlap", ptr(d_in), 0, ptr(out), n - 1, 0, n, B, 1024, s0, s1, pdc, ptr(ws), wsb)
        refused("seam_block2 shorter than the second filter", ptr(d_in), 0, ptr(out), n, 0, n, B, 23, s0, s1, pdc, ptr(ws), wsb)
        refused("seam_block shorter than the first filter", ptr(d_in), 0, ptr(out), n, 0, n, 127, 1024, s0, s1, pdc, ptr(ws), wsb)
        refused("the first window before d_in", ptr(d_in), 8, ptr(out), n, 0, n, B, 1024, s0, s1, pdc, ptr(ws), wsb)
        if form == FM:
            refused("the same state array twice", ptr(d_in), 0, ptr(out), n, 0, n, B, 1024, s0, s0, pdc, ptr(ws), wsb)
        else:
            refused("a state array with the envelope form", ptr(d_in), 0, ptr(out), n, 0, n, B, 1024, ptr(st), None, pdc, ptr(ws), wsb)
    assert (counters(hip) == c0).all()


def test_an_empty_range(hip, oracle):
    d_in = device_inputs(oracle)["u8"]
    st = to_dev(np.arange(6, dtype=np.float32) + 0.5)
    for form, dc in FORMS:
        nb = make(hip, "24/4", form, dc, BC.bank_tables(3))
        dcs = to_dev(np.full(6, 0.5, np.float32))
        for route in ROUTES:
            nb.set_route(route)
            c0 = counters(hip)
            out, fin = dev_empty_f32(8), dev_empty_f32(6)
            if form == FM:
                nb.run_u8(ptr(d_in), 0, ptr(out), 1, 7, 7, B, 1024, ptr(st), ptr(fin))
                assert_bit_equal(to_host(fin), to_host(st), f"route {route}: d_final of an empty range")
                nb.run_u8(ptr(d_in), 0, ptr(out), 1, 7, 7, B, 1024, None, ptr(fin))
                assert_bit_equal(to_host(fin), np.zeros(6, np.float32), f"route {route}: d_final of an empty range from a null state")
            else:
                nb.run_u8(ptr(d_in), 0, ptr(out), 1, 7, 7, B, 1024, None, None, ptr(dcs) if dc else None)
                assert (to_host(dcs) == 0.5).all(), "the dc state of an empty range is left as it is"
            assert (to_host(out).view(np.uint32) == CANARY).all()
            assert (counters(hip) - c0)[0] == 0


# ---- 7: concurrency -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,dc", [(ENV, True), (FM, False)], ids=["env-dc", "fm"])
def test_one_bank_two_host_threads(hip, oracle, form, dc):
    """One bank, two host threads, each with a stream, state arrays and workspaces of its own."""
    import torch
    shape, seam, seam2 = "24/4", B, 1024
    tables = BC.bank_tables(3)
    nb = make(hip, shape, form, dc, tables)
    d_u8 = device_inputs(oracle)["u8"]
    n = NB.n_out(shape)
    for route in (1, 2):
        nb.set_route(route)
        outs = [dev_empty_f32(3 * n) for _ in range(2)]
        states = [[torch.zeros(6, dtype=torch.float32, device="cuda") for _ in range(2)] for _ in range(2)]
        dcst = [torch.zeros(6, dtype=torch.float32, device="cuda") for _ in range(2)]
        wss = [torch.empty(nb.workspace_bytes(n), dtype=torch.uint8, device="cuda") for _ in range(2)]
        streams = [torch.cuda.Stream() for _ in range(2)]
        errors = []
        torch.cuda.synchronize()

        def work(i):
            try:
                for rep in range(3):
                    edges = [0, 255 + i, 601, n]
                    with torch.cuda.stream(streams[i]):
                        dcst[i].zero_()
                    for q, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                        fm = form == FM
                        nb.run_u8(ptr(d_u8), 0, ptr(outs[i]) + 4 * a, n, a, b, seam, seam2,
                                  (None if q == 0 else ptr(states[i][q & 1])) if fm else None, ptr(states[i][(q + 1) & 1]) if fm else None,
                                  ptr(dcst[i]) if dc else None, ptr(wss[i]), wss[i].numel(), stream=streams[i].cuda_stream)
                streams[i].synchronize()
            except Exception as e:                           # noqa: BLE001 -- reported below, on the main thread
                errors.append(e)

        th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
        for q in th:
            q.start()
        for q in th:
            q.join()
        assert not errors, errors
        for i in range(2):
            rows = to_host(outs[i]).reshape(3, n)
            for j, t in enumerate(tables):
                assert_bit_equal(rows[j], NB.expected(oracle, t, shape, seam, seam2, "u8", form, dc), f"route {route}, thread {i}, channel {j}")


# ---- 8: the auto rule -----------------------------------------------------------------------------------------------------------
def test_the_edges_of_the_auto_rule(hip, oracle):
    """Auto takes the fused launch exactly at the cells read from profiles/narrow_bank_bench.txt (sdr_hip.h states the rule), over
    the stage-2 outputs a channel; the same bits on both sides of each edge."""
    import torch
    big = torch.randint(0, 256, (2 * (8 * 16500 + 128),), dtype=torch.uint8, device="cuda")
    t32 = BC.bank_tables(32)
    # (shape, form, dc, channels, seam_block2, count, fused): 247 / 4087 and 190 are the measured launches of 8192 and 2^17 samples
    points = [("24/4", FM, False, 1, 0, 247, 1), ("24/4", FM, False, 1, 0, 246, 0), ("24/4", ENV, True, 1, 0, 247, 1),
              ("24/4", ENV, True, 1, 0, 4087, 0), ("24/4", ENV, True, 1, 0, 4088, 0), ("24/4", ENV, False, 1, 0, 247, 1),
              ("24/4", FM, False, 1, 1000, 247, 0), ("24/4", FM, False, 1, 1024, 247, 1), ("61/5", FM, False, 3, 0, 190, 1),
              ("61/5", ENV, True, 3, 0, 3262, 0), ("61/5", ENV, True, 8, 0, 3262, 1), ("24/4", ENV, False, 2, 1024, 247, 1),
              ("24/4", FM, False, 32, 0, 4087, 1), ("24/4", FM, False, 32, 0, 4088, 1), ("128/16", FM, False, 1, 0, 64, 0)]
    for shape, form, dc, nch, seam2, n_out, fused in points:
        nb = make(hip, shape, form, dc, t32[:nch])
        what = f"{shape}, form {form}, dc {dc}, {nch} channels, seam_block2 {seam2}, {n_out} outputs"
        got = {}
        for route in (0, 2 if fused else 1):
            nb.set_route(route)
            ws = torch.empty(nb.workspace_bytes(n_out), dtype=torch.uint8, device="cuda")
            out = torch.zeros(nch * n_out, dtype=torch.float32, device="cuda")
            fin = torch.zeros(2 * nch, dtype=torch.float32, device="cuda")
            dcs = torch.zeros(2 * nch, dtype=torch.float32, device="cuda")
            c0 = counters(hip)
            nb.run_u8(ptr(big), 0, ptr(out), n_out, 0, n_out, B if seam2 else 0, seam2, None, ptr(fin) if form == FM else None,
                      ptr(dcs) if dc else None, ptr(ws), ws.numel())
            torch.cuda.synchronize()
            if route == 0:
                assert (counters(hip) - c0)[0] == fused, what + ": auto took the other route"
            got[route] = torch.cat([out, fin, dcs]).view(torch.int32).clone()
        a, b = got.values()
        assert torch.equal(a, b), what + ": the two routes differ"
