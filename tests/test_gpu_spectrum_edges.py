"""The spectrum family on the device at its edges (tests/spectrum_edge_cases.py states the cases, tests/test_spectrum_edge_cases.py
shows on the CPU what they reach): the host loops of fft.cpp on their second turn -- chunks of rows, batches of a reduction with state
carried between them, slices of output rows and of layers, grids smaller than the work -- with the counters asserting that the slicing
happened; every size and format of the one-kernel route; directed inputs with a closed form; offset bases (the narrow loads of u8 and
cf32) between guard bands; the refusal of a float32 base that is not 4-byte aligned; non-finite cf32 input, which poisons the rows
and output rows that hold it and no other; and the float32 value classes.

Tolerances are the operator's own: assert_close is tests/test_gpu_spectrum.py's contract, with "one float32 unit in the last place"
taken as the subnormal spacing 2^-149 where the value is a float32 subnormal (spectrum_edge_cases.close_bound: unchanged at normal
magnitudes), and R.check for the reducing form.  Outputs come from gpu_util.dev_empty_f32: a stray write trips the NaN guard bands."""
import itertools

import numpy as np
import pytest

import gpu_util as G
import spectrum_edge_cases as E
import spectrum_model as M
import spectrum_reduce_model as R

pytestmark = pytest.mark.gpu

REDUCES = (R.MEAN_POWER, R.MEAN_MAGNITUDE, R.MAX_MAGNITUDE)
UNITS = (R.LINEAR, R.DB)
ALL_PAIRS = tuple(itertools.product(REDUCES, UNITS))
TWO_PAIRS = ((R.MEAN_POWER, R.DB), (R.MAX_MAGNITUDE, R.LINEAR))
FLOOR = -150.0
ERR_ARG = -1
FUSED, SPLIT, BATCHES, LAYERS = range(4)


def counters(hip):
    return np.array([hip.spectrum_fused_launches(), hip.spectrum_reduce_split_launches(), hip.spectrum_hipfft_batches(),
                     hip.spectrum_reduce_layer_launches()])


def assert_close(got, ref64, what="", where=None):
    got = np.asarray(got, dtype=np.float64).reshape(ref64.shape)
    where = np.ones(ref64.shape, bool) if where is None else where
    assert np.all(np.isfinite(got[where])), f"{what}: non-finite bins (a row not written?)"
    bound = E.close_bound(ref64)
    with np.errstate(invalid="ignore"):
        err = np.where(where, np.abs(got - ref64), 0.0)
    worst = np.unravel_index(np.argmax(err - bound), err.shape)
    print(f"{what}: max |got - ref| = {err.max():.3e}, worst bin {worst}: err {err[worst]:.3e} vs bound {bound[worst]:.3e}")
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} bins outside the tolerance, worst {worst}: {err[worst]:.3e} > {bound[worst]:.3e}"


def run(spec, base, ns, hop, rows):
    """base: a device address -> rows x n float32 through run_device on guarded device memory."""
    d_out = G.dev_empty_f32(rows * spec.n)
    assert spec.run_device(base, ns, G.ptr(d_out), hop=hop, rows=rows) == rows
    return G.to_host(d_out).reshape(rows, spec.n)


def reduce(spec, base, ns, hop, rows_out, group, red, unit):
    d_out = G.dev_empty_f32(rows_out * spec.n)
    assert spec.reduce_device(base, ns, G.ptr(d_out), group, red, unit, FLOOR, hop=hop, rows_out=rows_out) == rows_out
    return G.to_host(d_out).reshape(rows_out, spec.n)


def same_bits_but_for_nan_payloads(a, b):
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


# ---- 1. run_device on the hipFFT route: chunks of rows ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.RUN_HIPFFT, ids=lambda c: f"{c.n}x{c.rows}")
def test_run_device_in_chunks_of_rows(hip, case):
    n, hop, scale = case.n, case.hop, 1.0 / case.n
    ns = E.samples_for(n, hop, case.rows)
    iq = E.u8_iq(n, ns)
    d_in = G.to_dev(iq)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, scale)
    ref64, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, scale, hop, case.rows)
    before = counters(hip)
    got = run(spec, G.ptr(d_in), ns, hop, case.rows)
    moved = counters(hip) - before
    assert moved[BATCHES] == case.batches, case.what
    assert moved[FUSED] == 0 and moved[LAYERS] == 0, "the one-kernel route ran"
    assert_close(got, ref64, f"n={n} rows={case.rows}")
    if case.then_rows:                               # the same object again: the last chunk has a size no plan was made for
        before = counters(hip)
        again = run(spec, G.ptr(d_in), E.samples_for(n, hop, case.then_rows), hop, case.then_rows)
        assert (counters(hip) - before)[BATCHES] == case.then_batches
        assert_close(again, ref64[:case.then_rows], f"n={n} rows={case.then_rows} on the same object")


# ---- 2. the reducing form on the hipFFT route: batches with carried state --------------------------------------------------------------
@pytest.mark.parametrize("case", E.REDUCE_HIPFFT, ids=lambda c: c.edge)
def test_reduce_in_batches_with_carried_state(hip, case):
    n, hop, scale = case.n, case.hop, 1.0 / case.n
    rows = case.rows_out * case.group
    ns = E.samples_for(n, hop, rows)
    iq = E.u8_iq(case.group, ns)
    d_in = G.to_dev(iq)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, scale)
    if case.force:
        spec.set_route(hip.SPECTRUM_ROUTE_HIPFFT)
    mag, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, scale, hop, rows)
    for red, unit in (ALL_PAIRS if case is E.ALL_PAIRS_CASE else TWO_PAIRS):
        if case.dirty_group:                         # state left behind in the rows this case's batches start with
            reduce(spec, G.ptr(d_in), ns, hop, case.rows_out, case.dirty_group, red, unit)
        before = counters(hip)
        got = reduce(spec, G.ptr(d_in), ns, hop, case.rows_out, case.group, red, unit)
        moved = counters(hip) - before
        assert moved[BATCHES] == case.batches, case.what
        assert moved[FUSED] == 0 and moved[SPLIT] == 0 and moved[LAYERS] == 0, "the one-kernel route ran"
        v, delta = R.reduce_rows(mag, case.group, red)
        R.check(got, v, delta, red, unit, FLOOR, f"{case.edge} reduce={red} unit={unit}")


# ---- 3. run_device on the one-kernel route: more tiles than the grid -------------------------------------------------------------------
@pytest.mark.parametrize("case", E.RUN_FUSED, ids=lambda c: f"{c.n}x{c.rows}")
def test_more_tiles_than_the_grid_of_the_plain_kernel(hip, case):
    n, hop, scale = case.n, case.hop, 1.0 / case.n
    ns = E.samples_for(n, hop, case.rows)
    iq = E.u8_iq(n + 1, ns)
    d_in = G.to_dev(iq)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, scale)
    before = counters(hip)
    got = run(spec, G.ptr(d_in), ns, hop, case.rows)
    moved = counters(hip) - before
    assert moved[FUSED] == 1 and moved[BATCHES] == 0
    ref64, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, scale, hop, case.rows)
    assert_close(got, ref64, case.what)
    for row in (case.second_turn_row, case.rows - 1):        # the first row of a workgroup's second turn; the partial last tile
        d_row = G.to_dev(iq[2 * row * hop:2 * (row * hop + n)].copy())
        alone = run(spec, G.ptr(d_row), n, n, 1)
        assert alone[0].tobytes() == got[row].tobytes(), f"row {row}"


# ---- 4. the layers of the reducing kernel in slices of output rows and of chunks -------------------------------------------------------
def test_layers_in_slices_of_rows_and_of_chunks(hip):
    case = E.REDUCE_LAYERS
    n, hop, group, scale = case.n, case.hop, case.group, 1.0 / case.n
    ns = E.samples_for(n, hop, case.rows_out * group)
    iq = E.u8_iq(9, ns)
    d_in = G.to_dev(iq)
    spec = hip.Spectrum(n, hip.IQ_U8, hip.WINDOW_HANNING, True, scale)
    for red, unit in TWO_PAIRS:
        got = {}
        for mode in (hip.REDUCE_SPLIT_NEVER, hip.REDUCE_SPLIT_ALWAYS):
            spec.set_reduce_split(mode)
            before = counters(hip)
            got[mode] = reduce(spec, G.ptr(d_in), ns, hop, case.rows_out, group, red, unit)
            moved = counters(hip) - before
            assert moved[LAYERS] == case.launches, case.what
            assert moved[FUSED] == 1 and moved[BATCHES] == 0 and moved[SPLIT] == (1 if mode == hip.REDUCE_SPLIT_ALWAYS else 0)
        assert got[hip.REDUCE_SPLIT_NEVER].tobytes() == got[hip.REDUCE_SPLIT_ALWAYS].tobytes()
        for row in case.model_rows:
            first = row * group * hop
            part = iq[2 * first:2 * (first + E.samples_for(n, hop, group))]
            v, delta = R.spectrum_reduce(part, n, M.IQ_U8, M.WINDOW_HANNING, None, True, scale, hop, 1, group, red)
            R.check(got[hip.REDUCE_SPLIT_NEVER][row:row + 1], v, delta, red, unit, FLOOR, f"row {row} reduce={red} unit={unit}")


# ---- 5. every size and format of the one-kernel route ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [M.IQ_U8, M.IQ_CF32, E.IQ_I16], ids=["u8", "cf32", "i16"])
@pytest.mark.parametrize("n", E.FUSED_SIZES)
def test_every_size_and_format_on_the_one_kernel_route(hip, n, fmt):
    assert (hip.IQ_U8, hip.IQ_CF32, hip.IQ_I16) == (M.IQ_U8, M.IQ_CF32, E.IQ_I16)
    (rows, hop), group, scale = E.size_case(n), 3, 1.0 / n
    ns = E.samples_for(n, hop, rows * group)
    iq, floats = E.format_input(fmt, n + fmt, ns)
    d_in = G.to_dev(iq)
    spec = hip.Spectrum(n, fmt, hip.WINDOW_BLACKMAN, True, scale)
    mag, _ = M.spectrum(floats, n, M.IQ_CF32, M.WINDOW_BLACKMAN, None, True, scale, hop, rows * group)
    before = counters(hip)
    got = run(spec, G.ptr(d_in), E.samples_for(n, hop, rows), hop, rows)
    got_reduced = reduce(spec, G.ptr(d_in), ns, hop, rows, group, R.MEAN_MAGNITUDE, R.LINEAR)
    moved = counters(hip) - before
    assert moved[FUSED] == 2 and moved[BATCHES] == 0 and moved[LAYERS] == 0
    assert_close(got, mag[:rows], f"n={n} fmt={fmt} run_device")
    v, delta = R.reduce_rows(mag, group, R.MEAN_MAGNITUDE)
    R.check(got_reduced, v, delta, R.MEAN_MAGNITUDE, R.LINEAR, FLOOR, f"n={n} fmt={fmt} reduce")


# ---- 6. directed inputs with a closed form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.DIRECTED_SIZES)
def test_impulses_and_tones_have_their_closed_forms(hip, n):
    before = counters(hip)
    scale = 0.75
    spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_HAMMING, True, scale)
    w = M.window(M.WINDOW_HAMMING, n)
    for j in E.impulse_positions(n):
        d_in = G.to_dev(E.impulse(n, j))
        got = run(spec, G.ptr(d_in), n, n, 1)
        assert_close(got, np.full((1, n), scale * w[j]), f"n={n} impulse at {j}")          # |X[k]| = w[j] in every bin
    for shift in (False, True):
        spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_NONE, shift, scale)
        for k in E.tone_bins(n):
            iq, peak = E.tone(n, k)
            d_in = G.to_dev(iq)
            got = run(spec, G.ptr(d_in), n, n, 1)[0].astype(np.float64)
            at = (k + n // 2) % n if shift else k
            assert int(np.argmax(got)) == at, f"n={n} tone at {k} shift {shift}"
            assert abs(got[at] - scale * peak) <= 1e-11 * scale * peak + 2.0 ** -23 * scale * peak, f"n={n} tone at {k}: the peak"
            assert abs(scale * peak - scale * n) <= 1e-7 * scale * n
            assert np.max(np.delete(got, at)) <= 1e-6 * scale * n, "what float32 samples of a tone leak into the other bins"
    moved = counters(hip) - before
    assert (moved[FUSED] > 0 and moved[BATCHES] == 0) if n in E.FUSED_SIZES else (moved[FUSED] == 0 and moved[BATCHES] > 0)


# ---- 7. offset bases: the narrow loads of u8 and cf32 ----------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", [M.IQ_U8, M.IQ_CF32], ids=["u8", "cf32"])
@pytest.mark.parametrize("n,hop,route", [(64, 48, 1), (8192, 4096, 1), (1000, 501, 0)])
def test_offset_bases_give_the_same_bits_and_reads_stay_inside_the_input(hip, n, hop, route, fmt):
    """The same samples at a base that allows one load per sample (u8: even, cf32: 8-byte aligned) and one element on (two loads) give
    the bits of a plain aligned copy, between guard bands far from the samples -- at the buffer's start and ending exactly at the last
    row's last sample.  Every run covers 210 input rows, so all of them end on the last sample: the plain kernel, the reducing kernel
    with a group of 3, and with a group of 70 (on the one-kernel route: through the layers)."""
    rows = 210
    ns = E.samples_for(n, hop, rows)
    iq, _ = E.format_input(fmt, n, ns)
    guard = 64                                   # elements: a multiple of 2, so the payload keeps the base's alignment
    if fmt == M.IQ_U8:
        band, size, aligned = iq[:guard] ^ np.uint8(0x80), 1, 2
    else:
        band, size, aligned = iq[:guard] + np.float32(1e6), 4, 8
    spec = hip.Spectrum(n, fmt, hip.WINDOW_BLACKMAN, False, 1.0 / n)
    spec.set_route(route)

    def all_paths(base):
        before = counters(hip)
        out = (run(spec, base, ns, hop, rows), reduce(spec, base, ns, hop, rows // 3, 3, R.MEAN_POWER, R.DB),
               reduce(spec, base, ns, hop, rows // 70, 70, R.MEAN_POWER, R.DB))
        moved = counters(hip) - before
        assert (moved[FUSED] == 3 and moved[LAYERS] == 1 and moved[BATCHES] == 0) if route == 1 else (moved[FUSED] == 0 and moved[BATCHES] >= 3)
        return out

    got = {}
    for off in (0, 1):
        buf = np.concatenate([np.zeros(off, iq.dtype), band, iq, band])
        d = G.to_dev(buf)
        base = G.ptr(d) + size * (off + guard)
        assert base % aligned == size * off
        got[off] = all_paths(base)
    plain = G.to_dev(iq)
    want = all_paths(G.ptr(plain))
    for off in (0, 1):
        for a, b, what in zip(got[off], want, ("run_device", "reduce, group 3", "reduce, group 70")):
            assert a.tobytes() == b.tobytes(), f"{what} at base offset {size * off} bytes"


# ---- 8. a float32 base that is not 4-byte aligned is refused ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", [1, 2])
def test_a_misaligned_float32_base_is_refused_with_nothing_written(hip, route):
    n, hop, rows = 256, 128, 4
    ns = E.samples_for(n, hop, rows)
    d = G.to_dev(np.random.default_rng(4).standard_normal(2 * ns + 2).astype(np.float32))
    spec = hip.Spectrum(n, hip.IQ_CF32)
    spec.set_route(route)
    d_out = G.dev_empty_f32(rows * n)
    before = counters(hip)
    for off in (1, 2, 3):
        assert hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d) + off, ns, hop, rows, G.ptr(d_out)) == ERR_ARG, off
        assert hip.lib.sdrhip_spectrum_reduce_run_device(spec.h, None, G.ptr(d) + off, ns, hop, rows, 1, 1, 0, FLOOR, G.ptr(d_out)) == ERR_ARG, off
    assert np.array_equal(counters(hip), before), "a refused call counts nowhere"
    assert np.all(np.isnan(G.to_host(d_out))), "nothing may be written"
    assert hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d) + 4, ns, hop, rows, G.ptr(d_out)) == 0
    assert np.all(np.isfinite(G.to_host(d_out)))


# ---- 9. non-finite cf32 input ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,route", E.NONFINITE_SIZES, ids=["one kernel", "hipFFT"])
def test_a_non_finite_sample_poisons_its_rows_and_no_other(hip, n, route):
    """One NaN or Inf in the input: every bin of the two input rows that hold it is non-finite (NaN for a NaN, also where the window is
    0), so is every bin of the output rows they belong to in every reduce and unit -- a max hold does not drop the row, the dB floor
    does not hide it -- and every other row has the bits of the run on the clean input."""
    hop, scale = n // 2, 1.0 / n
    spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_HANNING, True, scale)
    spec.set_route(route)
    for group, rows_out in E.NONFINITE_GROUPS:
        rows = group * rows_out
        ns = E.samples_for(n, hop, rows)
        iq = np.random.default_rng(n + group).standard_normal(2 * ns).astype(np.float32)
        splits = (hip.REDUCE_SPLIT_NEVER, hip.REDUCE_SPLIT_ALWAYS) if route == 1 and group > E.CHUNK else (hip.REDUCE_SPLIT_AUTO,)

        def everything(samples):
            d_in = G.to_dev(samples)
            out = {"rows": run(spec, G.ptr(d_in), ns, hop, rows)}
            for split in splits:
                spec.set_reduce_split(split)
                for red, unit in ALL_PAIRS:
                    out[split, red, unit] = reduce(spec, G.ptr(d_in), ns, hop, rows_out, group, red, unit)
            return out

        clean = everything(iq)
        assert all(np.all(np.isfinite(a)) for a in clean.values())
        for name, value, imaginary, at_j0 in E.POISONS:
            p, held = E.poison_place(n, group, at_j0)
            bad = E.poisoned(iq, p, value, imaginary)
            got = everything(bad)
            spoiled = (lambda a: np.all(np.isnan(a))) if np.isnan(value) else (lambda a: not np.any(np.isfinite(a)))
            what = f"n={n} group={group} {name}"
            for r in range(rows):
                if r in held:
                    assert spoiled(got["rows"][r]), f"{what}: input row {r} holds the sample"
                else:
                    assert got["rows"][r].tobytes() == clean["rows"][r].tobytes(), f"{what}: input row {r} does not hold the sample"
            mag = E.reference(bad, n, scale, hop, rows, M.WINDOW_HANNING, True)
            for split in splits:
                for red, unit in ALL_PAIRS:
                    a, where = got[split, red, unit], f"{what} split={split} reduce={red} unit={unit}"
                    for row in range(rows_out):
                        if row in {r // group for r in held}:
                            assert spoiled(a[row]), f"{where}: output row {row} has a poisoned input row"
                        else:
                            assert a[row].tobytes() == clean[split, red, unit][row].tobytes(), f"{where}: output row {row} is clean"
                    if np.isnan(value):              # the definition in numpy propagates the NaN too: the whole result against it
                        v, delta = R.reduce_rows(mag, group, red)
                        assert np.all(np.isnan(v[:2])) and np.all(np.isfinite(v[2:]))
                        R.check(a, v, delta, red, unit, FLOOR, where)
                    assert same_bits_but_for_nan_payloads(a, got[splits[0], red, unit]), f"{where}: the split modes differ"


# ---- 10. float32 value classes of cf32 input -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", E.VALUE_CLASS_SIZES)
def test_float32_value_classes(hip, n):
    for vc in E.value_classes(n):
        spec = hip.Spectrum(n, hip.IQ_CF32, hip.WINDOW_NONE, False, vc.scale)
        iq = vc.iq()
        d_in = G.to_dev(iq)
        got = run(spec, G.ptr(d_in), vc.rows * n, n, vc.rows)
        ref64 = E.reference(iq, n, vc.scale, n, vc.rows)
        if not vc.overflows:
            assert_close(got, ref64, f"n={n} {vc.name}")
            continue
        must_inf, must_close, left_out = E.overflow_split(ref64)
        assert left_out.sum() <= ref64.size // 100
        assert np.all(got[must_inf] == np.inf), f"n={n} {vc.name}: a bin past FLT_MAX is +Inf"
        assert_close(got, ref64, f"n={n} {vc.name}, the bins below FLT_MAX", where=must_close)
