"""int16 IQ into the spectrum operator (SDRHIP_IQ_I16: load_sample<2>, kernels_spectrum.hip).  The definition is the cfloat operator on
the buffer sdrhip_convert_i16_run makes of the same int16 buffer: on the one-kernel route the two agree BIT FOR BIT (the conversion is
exact), for run_device and for every reduce x unit, groups on both sides of the chunk length, split or not; on both routes the rows
hold the operator's tolerance contract against the numpy model on oracle.convert_i16's floats.  The input is the first blocks of
tuner_i16_cases.stream_i16 (the whole int16 range, forced edge values either side of sample 8192; tests/test_spectrum_pipe_model.py
shows that they lie inside rows).  Every output buffer starts as NaN canaries."""
import itertools

import numpy as np
import pytest
import torch

import gpu_util as G
import spectrum_model as M
import spectrum_pipe_model as SP
import spectrum_reduce_model as R
import tuner_i16_cases as IC

pytestmark = pytest.mark.gpu

REDUCES = (R.MEAN_POWER, R.MEAN_MAGNITUDE, R.MAX_MAGNITUDE)
UNITS = (R.LINEAR, R.DB)
FLOOR = -150.0
ERR_ARG = -1
# n: (hop and output rows of the group-3 runs, hop and output rows of the group-70 runs); every run reaches past sample 8195
SHAPES = {64: ((64, 43), (64, 2)), 2048: ((1024, 3), (100, 2)), 8192: ((4096, 1), (128, 1))}


def stream():
    return SP.stream("i16", 3 * IC.B)


def pair(hip, n, route=None):
    """An int16 object and the cfloat object of the same arguments."""
    out = []
    for fmt in (hip.IQ_I16, hip.IQ_CF32):
        s = hip.Spectrum(n, fmt, hip.WINDOW_HANNING, True, 1.0 / n)
        if route is not None:
            s.set_route(route)
        out.append(s)
    return out


def converted(hip, d_i16):
    out = torch.empty(d_i16.numel(), dtype=torch.float32, device="cuda")
    hip.check(hip.lib.sdrhip_convert_i16_run(None, G.ptr(d_i16), G.ptr(out), d_i16.numel()), "sdrhip_convert_i16_run")
    torch.cuda.synchronize()
    return out


def run(spec, d_in, ns, hop, rows):
    d_out = G.dev_empty_f32(rows * spec.n)
    assert spec.run_device(d_in, ns, G.ptr(d_out), hop=hop, rows=rows) == rows
    return G.to_host(d_out).reshape(rows, spec.n)


def reduce(spec, d_in, ns, hop, rows_out, group, red, unit):
    d_out = G.dev_empty_f32(rows_out * spec.n)
    assert spec.reduce_device(d_in, ns, G.ptr(d_out), group, red, unit, FLOOR, hop=hop, rows_out=rows_out) == rows_out
    return G.to_host(d_out).reshape(rows_out, spec.n)


# ---- (a), (e): the one-kernel route against the cfloat operator on the converted buffer, bit for bit ---------------------------------
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_one_kernel_route_equals_the_cfloat_operator_on_the_converted_buffer(hip, n):
    i16, cf = pair(hip, n, hip.SPECTRUM_ROUTE_FUSED)
    iq = stream()
    d_i16 = G.to_dev(iq)
    d_cf = converted(hip, d_i16)
    assert G.to_host(d_cf).tobytes() == SP.i16_to_float(iq).tobytes()
    (hop3, rows3), (hop70, rows70) = SHAPES[n]
    ns = SP.samples_for(n, hop3, rows3, 3)
    rows = (ns - n) // hop3 + 1
    before = hip.spectrum_fused_launches()
    got = run(i16, G.ptr(d_i16), ns, hop3, rows)
    assert hip.spectrum_fused_launches() == before + 1, "run_device on int16 counts as on u8"
    assert got.tobytes() == run(cf, G.ptr(d_cf), ns, hop3, rows).tobytes(), "run_device"
    for group, hop, rows_out in ((3, hop3, rows3), (70, hop70, rows70)):
        ns = SP.samples_for(n, hop, rows_out, group)
        assert IC.B + 3 <= ns <= iq.size // 2
        for split in (hip.REDUCE_SPLIT_NEVER, hip.REDUCE_SPLIT_ALWAYS):
            i16.set_reduce_split(split)
            cf.set_reduce_split(split)
            for red, unit in itertools.product(REDUCES, UNITS):
                before, before_split = hip.spectrum_fused_launches(), hip.spectrum_reduce_split_launches()
                a = reduce(i16, G.ptr(d_i16), ns, hop, rows_out, group, red, unit)
                assert hip.spectrum_fused_launches() == before + 1, "one count per reduce call, as on u8"
                assert hip.spectrum_reduce_split_launches() == before_split + (1 if group > 32 and split == hip.REDUCE_SPLIT_ALWAYS else 0)
                b = reduce(cf, G.ptr(d_cf), ns, hop, rows_out, group, red, unit)
                assert a.tobytes() == b.tobytes(), f"group {group} split {split} reduce {red} unit {unit}"


# ---- (b): both routes against the model on oracle.convert_i16's floats --------------------------------------------------------------
@pytest.mark.parametrize("n,hop,rows_out,route", [(64, 64, 43, 1), (2048, 1024, 3, 1), (8192, 4096, 1, 1), (1000, 501, 6, 0), (1024, 512, 6, 2)])
def test_both_routes_hold_the_tolerance_contract(hip, oracle, n, hop, rows_out, route):
    group = 3
    spec = hip.Spectrum(n, hip.IQ_I16, hip.WINDOW_HANNING, True, 1.0 / n)
    spec.set_route(route)
    iq = stream()
    ns = SP.samples_for(n, hop, rows_out, group)
    assert IC.B + 3 <= ns <= iq.size // 2
    floats = np.asarray(oracle.convert_i16(iq), np.float32)
    mag, _ = M.spectrum(floats, n, M.IQ_CF32, M.WINDOW_HANNING, None, True, 1.0 / n, hop, rows_out * group)
    d_in = G.to_dev(iq)
    before = hip.spectrum_fused_launches()
    got = run(spec, G.ptr(d_in), ns, hop, rows_out * group)
    v, delta = R.reduce_rows(mag, 1, R.MEAN_MAGNITUDE)
    R.check(got, v, delta, R.MEAN_MAGNITUDE, R.LINEAR, FLOOR, f"run_device n={n}")
    for red, unit in itertools.product(REDUCES, UNITS):
        v, delta = R.reduce_rows(mag, group, red)
        R.check(reduce(spec, G.ptr(d_in), ns, hop, rows_out, group, red, unit), v, delta, red, unit, FLOOR, f"n={n} reduce={red} unit={unit}")
    assert hip.spectrum_fused_launches() == before + (7 if route == 1 else 0), "the route that was asked for"


# ---- (c): base pointers and reads ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,rows_out,route", [(64, 48, 60, 1), (8192, 4096, 1, 1), (1000, 501, 6, 0)])
def test_wide_and_narrow_loads_and_reads_stay_inside_the_input(hip, n, hop, rows_out, route):
    """The same samples at a 4-byte aligned base (one load per sample) and 2 bytes on (two loads) give the same bits, also where the
    samples stand between guard bands that hold the stream with the top bit flipped -- at the buffer's start and ending exactly at the
    last row's last sample: a load that reached outside [0, 4 * n_samples) would read a value far from its neighbour's."""
    group = 3
    spec = hip.Spectrum(n, hip.IQ_I16, hip.WINDOW_BLACKMAN, False, 1.0 / n)
    spec.set_route(route)
    ns = SP.samples_for(n, hop, rows_out, group)
    iq = stream()[:2 * ns]
    flipped = (iq.view(np.uint16) ^ np.uint16(0x8000)).view(np.int16)
    guard = 64                                   # int16 elements: a multiple of 2, so the payload keeps the base's alignment
    got = {}
    for off in (0, 1):                           # int16 elements in front: base 4-byte aligned, base 2 bytes on
        buf = np.concatenate([np.zeros(off, np.int16), flipped[:guard], iq, flipped[:guard]])
        d = G.to_dev(buf)
        base = G.ptr(d) + 2 * (off + guard)
        assert base % 4 == 2 * off
        got[off] = (run(spec, base, ns, hop, rows_out * group), reduce(spec, base, ns, hop, rows_out, group, R.MEAN_POWER, R.DB))
    plain = G.to_dev(iq)
    want = (run(spec, G.ptr(plain), ns, hop, rows_out * group), reduce(spec, G.ptr(plain), ns, hop, rows_out, group, R.MEAN_POWER, R.DB))
    for off in (0, 1):
        for a, b, what in zip(got[off], want, ("run_device", "reduce_device")):
            assert a.tobytes() == b.tobytes(), f"{what} at base offset {2 * off} bytes"


def test_an_odd_address_is_refused_with_nothing_written(hip):
    n, hop, rows = 256, 128, 4
    ns = SP.samples_for(n, hop, rows, 1)
    d = G.to_dev(stream()[:2 * ns + 2])
    for route in (1, 2):
        spec = hip.Spectrum(n, hip.IQ_I16)
        spec.set_route(route)
        d_out = G.dev_empty_f32(rows * n)
        before = hip.spectrum_fused_launches()
        assert hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d) + 1, ns, hop, rows, G.ptr(d_out)) == ERR_ARG
        assert hip.lib.sdrhip_spectrum_reduce_run_device(spec.h, None, G.ptr(d) + 3, ns, hop, rows, 1, 1, 0, FLOOR, G.ptr(d_out)) == ERR_ARG
        assert hip.spectrum_fused_launches() == before
        assert np.all(np.isnan(G.to_host(d_out))), "nothing may be written"
        assert hip.lib.sdrhip_spectrum_run_device(spec.h, None, G.ptr(d) + 2, ns, hop, rows, G.ptr(d_out)) == 0
        assert np.all(np.isfinite(G.to_host(d_out)))


# ---- (d): the host entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,hop,rows_out", [(256, 253, 9), (1000, 997, 3)])
def test_host_entry_points_equal_the_device_ones(hip, n, hop, rows_out):
    group = 4
    ns = SP.samples_for(n, hop, rows_out, group)
    iq = stream()[:2 * ns]
    assert ns >= IC.B + 3
    spec = hip.Spectrum(n, hip.IQ_I16, hip.WINDOW_HAMMING, True, 2.0)
    d_in = G.to_dev(iq)
    assert spec.run(iq, hop=hop).tobytes() == run(spec, G.ptr(d_in), ns, hop, rows_out * group).tobytes()
    for red, unit in ((R.MEAN_POWER, R.DB), (R.MAX_MAGNITUDE, R.LINEAR)):
        host = spec.reduce(iq, group, red, unit, FLOOR, hop=hop)
        assert host.shape == (rows_out, n)
        assert host.tobytes() == reduce(spec, G.ptr(d_in), ns, hop, rows_out, group, red, unit).tobytes()
