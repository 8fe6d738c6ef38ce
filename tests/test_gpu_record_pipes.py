"""The record seam (sdrhip_{filter,decimator,resampler}_{one,cross}, abi_records.cpp) driven the way its first user drives it: the
reference's own Pipes (restated in oracle/pipes_model.py) with both closures of each record bound to the device
(tests/record_models.py, the Python twin of haskell/SDR/GPU.hs).  The same Pipe with the oracle's closures is the expected answer,
bit for bit.  The cases are tests/record_pipe_cases.py's; tests/test_record_pipe_cases.py proves on the CPU which transitions and
branches they reach."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest
import torch

from conftest import assert_bit_equal
from gpu_util import dev_empty_f32, ptr, to_host
from oracle import pipes_model as PM
from oracle.oracle import duplicate
from record_models import DeviceFilterModel, DeviceResamplerModel, GuardedOut
import record_pipe_cases as RC
import signals as S

pytestmark = pytest.mark.gpu

ERR_ARG = -1
DIRECT_BYTES = 512 << 10            # abi_records.cpp: buffers up to this size are read and written in place


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _pad(taps, m):
    t = np.asarray(taps, np.float32)
    return np.concatenate([t, np.zeros((-t.size) % m, np.float32)])


def _copied(hip):
    return int(hip.lib.sdrhip_debug_record_copied_calls())


def _last_error(hip):
    return hip.lib.sdrhip_last_error().decode()


def _run(c, model, out_block):
    """-> (yielded blocks, trace, what every closure call returned)"""
    results = []
    RC.instrument(model, results)
    yielded, trace = RC.run_pipe(c, model, out_block)
    return yielded, trace, results


def _device_model(c, oracle, desc=None):
    return RC.make_model(c, oracle, functools.partial(DeviceFilterModel, desc=desc), functools.partial(DeviceResamplerModel, desc=desc))


def _assert_same_run(c, out_block, got, exp, what="device"):
    """Every closure call's result, the trace and the yielded blocks of two runs of one case."""
    tag = f"{RC.case_id(c)}, blockSizeOut {out_block}, {what}"
    (g_blocks, g_trace, g_results), (e_blocks, e_trace, e_results) = got, exp
    for i, (g, e) in enumerate(zip(g_results, e_results)):
        call = f"{tag}: call {i} {e_trace[i]}"
        if c.kind == "resampler":
            assert_bit_equal(g[0], e[0], call)
            assert tuple(g[1]) == tuple(e[1]) and g[2] == e[2], f"{call}: state {g[1:]} vs {e[1:]}"
        else:
            assert_bit_equal(g, e, call)
    assert g_trace == e_trace, f"{tag}: the traces differ"
    assert len(g_blocks) == len(e_blocks), tag
    for i, (g, e) in enumerate(zip(g_blocks, e_blocks)):
        assert_bit_equal(g, e, f"{tag}: yielded block {i}")


@pytest.mark.parametrize("key", RC.GROUPS, ids=lambda k: f"{k[0]}-{k[1]}-{'c' if k[2] else 'r'}")
def test_every_family_through_its_pipe(hip, oracle, key):
    """Every case of the table, at both output block sizes, once with the device-backed record and once with the plain model."""
    cases = RC.cases_of(key)
    assert len(cases) >= 12
    calls = 0
    for c in cases:
        for ob in RC.OUT_BLOCKS:
            exp = _run(c, RC.make_model(c, oracle), ob)
            got = _run(c, _device_model(c, oracle), ob)
            _assert_same_run(c, ob, got, exp)
            calls += len(exp[1])
    assert calls > 500


def test_fm_receiver_as_the_haskell_binding_composes_it(hip, oracle):
    """examples/fm/fm.hs with the records of GPU.hs: convert, fmDemod and scale through the drop-in symbols, the decimator, the
    resampler and the symmetric filter as device-backed records inside the reference's three Pipes.  64 source blocks of 1024 u8 IQ
    samples, the bench taps, every block size 1024, gain 0.2."""
    B, nblk, gain = 1024, 64, 0.2
    hd, hr, ha = S.taps_decim127(), S.taps_resamp191(), S.taps_audio_half64()
    u8 = S.iq_u8_fm(nblk * B)
    blocks = [u8[2 * i * B:2 * (i + 1) * B] for i in range(nblk)]

    iq = [hip.DropIn.convert("convertCAVX", b) for b in blocks]
    d_blocks, d_trace = PM.fir_decimator_pipe(DeviceFilterModel(oracle, hd, PM.ORDER_AVX, complex_=True, factor=8), iq, B)
    y_blocks, last = [], (0.0, 0.0)
    for b in d_blocks:
        y_blocks.append(hip.DropIn.fm_demod(b, last))
        last = (float(b[-2]), float(b[-1]))
    z_blocks, z_trace = PM.fir_resampler_pipe(DeviceResamplerModel(oracle, 3, 10, hr, PM.ORDER_AVX), y_blocks, B)
    a_blocks, a_trace = PM.fir_filter_pipe(DeviceFilterModel(oracle, ha, PM.ORDER_AVX, sym=True), z_blocks, B)
    a_blocks = [hip.DropIn.scale("scaleAVX", gain, a) for a in a_blocks]
    assert ("cross", 15) in d_trace and any(k == "cross" for k, _ in z_trace) and any(k == "cross" for k, _ in a_trace)

    exp = PM.fm_receiver(oracle, blocks, hd, 8, hr, 3, 10, ha, gain, block=B)
    assert len(exp) >= 1 and len(a_blocks) == len(exp)
    got = np.concatenate(a_blocks)
    assert_bit_equal(got, np.concatenate(exp), "records in the reference's Pipes vs the restated receiver")

    total = nblk * B
    chain = hip.FmChain(8, hd, 3, 10, hr, ha, gain, B)
    q0, q1, _ = chain.plan(0, total, total)
    assert q0 == 0
    wsb = chain.workspace_bytes(total)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    out = dev_empty_f32(q1)
    chain.run(ptr(torch.from_numpy(u8).cuda()), 0, total, ptr(out), 0, q1, ptr(ws), wsb)
    audio = to_host(out)
    n = min(audio.size, got.size)
    assert n >= B
    assert_bit_equal(got[:n], audio[:n], "records in the reference's Pipes vs FmChain over the same 65536 samples")


# ---- both sides of the staging threshold -----------------------------------------------------------------------------------------
def _fir_one(hip, name, desc, num, x, width=1):
    g = GuardedOut(num * width)
    rc = getattr(hip.lib, name)(desc.h, num, _fp(x), _fp(g.out))
    assert rc == 0, _last_error(hip)
    g.check(name)
    return g.out


def test_filter_one_on_both_sides_of_the_staging_threshold(hip, oracle):
    """A real AVX 32-tap filter: num = 131072 - 32 + 1 outputs read exactly 524288 bytes, in place; one output more is copied."""
    taps = S.gauss_taps(32, 41)
    f = hip.Filter(taps, hip.ORDER_AVX)
    assert f.num_coeffs == 32
    num = 131072 - 32 + 1
    x = S.real_block(131072 + 1, seed=42)
    assert 4 * (num - 1 + 32) == DIRECT_BYTES
    c0 = _copied(hip)
    assert_bit_equal(_fir_one(hip, "sdrhip_filter_one", f, num, x), oracle.filter_rr(8, num, taps, x), "filterOne in place")
    assert _copied(hip) == c0, "a 524288-byte input took the copying branch"
    assert_bit_equal(_fir_one(hip, "sdrhip_filter_one", f, num + 1, x), oracle.filter_rr(8, num + 1, taps, x), "filterOne copied")
    assert _copied(hip) == c0 + 1, "a 524292-byte input did not take the copying branch"


def test_decimator_one_on_both_sides_of_the_staging_threshold(hip, oracle):
    """The complex AVX /8 128-tap decimator: 8177 outputs read 65536 complex elements = 524288 bytes."""
    taps = S.gauss_taps(128, 43)
    d = hip.Decimator(8, taps, hip.ORDER_AVX, complex_=True)
    assert d.num_coeffs == 128
    num = (65536 - 128) // 8 + 1
    assert 8 * ((num - 1) * 8 + 128) == DIRECT_BYTES
    x = S.cfloat_block(65536 + 8, seed=44)
    c0 = _copied(hip)
    assert_bit_equal(_fir_one(hip, "sdrhip_decimator_one", d, num, x, 2), oracle.decimate_rc(4, num, 8, duplicate(taps), x), "decimateOne in place")
    assert _copied(hip) == c0
    assert_bit_equal(_fir_one(hip, "sdrhip_decimator_one", d, num + 1, x, 2), oracle.decimate_rc(4, num + 1, 8, duplicate(taps), x),
                     "decimateOne copied")
    assert _copied(hip) == c0 + 1


def test_cross_and_resampler_one_through_the_copying_branch(hip, oracle):
    """A filterCross call whose assembled input (last ++ next, clamped to what the outputs read) is over the threshold, and one
    resampleOne call of 3/10 with 191 taps on a 200000-float vector."""
    taps = S.gauss_taps(32, 45)
    f = hip.Filter(taps, hip.ORDER_AVX)
    num = 131072
    last, nxt = S.real_block(20, seed=46), S.real_block(131200, seed=47)
    assert 4 * (num - 1 + 32) > DIRECT_BYTES
    c0 = _copied(hip)
    g = GuardedOut(num)
    assert hip.lib.sdrhip_filter_cross(f.h, num, _fp(last), last.size, _fp(nxt), nxt.size, _fp(g.out)) == 0, _last_error(hip)
    g.check("sdrhip_filter_cross")
    assert_bit_equal(g.out, oracle.decimate_cross_r(1, taps, num, last, nxt), "filterCross copied")
    assert _copied(hip) == c0 + 1

    I, D, rt = 3, 10, S.taps_resamp191()
    r = hip.Resampler(I, D, rt, hip.ORDER_AVX)
    x = S.real_block(200000, seed=48)
    count = (x.size * I - r.num_coeffs) // D + 1
    g = GuardedOut(count)
    g2 = hip.lib.sdrhip_resampler_one(r.h, 0, count, _fp(x), x.size, _fp(g.out))
    assert g2 >= 0, _last_error(hip)
    g.check("sdrhip_resampler_one")
    exp, eg = oracle.resample_rr(8, count, oracle.prepare_coeffs(8, I, D, rt), 0, x)
    assert_bit_equal(g.out, exp, "resampleOne copied")
    assert g2 == eg
    assert _copied(hip) == c0 + 2


# ---- call edges, straight on the ABI ---------------------------------------------------------------------------------------------
def _refused(hip, name, *args):
    """The call returns SDRHIP_ERR_ARG, sdrhip_last_error names the function and the guarded output (the last argument) is untouched."""
    g = args[-1]
    rc = getattr(hip.lib, name)(*args[:-1], _fp(g.out))
    assert rc == ERR_ARG, (name, rc)
    assert name in _last_error(hip), _last_error(hip)
    assert g.untouched(), f"{name} refused the call but wrote to its output"


def _resampler_cross_need(I, D, ntaps, fo, num):
    """Elements of last ++ next that resampleCrossHighLevel reads for `num` outputs from filter offset fo (FilterInternal.hs:410-423):
    output k starts at element p = ceil((k D - fo) / I) with offset p I - (k D - fo) and strides the unpadded taps from there."""
    need = 0
    for k in range(num):
        p = PM.quot_up(k * D - fo, I)
        need = max(need, p + PM.quot_up(ntaps - (p * I - (k * D - fo)), I))
    return need


def test_fir_call_edges(hip, oracle):
    lib = hip.lib
    taps = S.gauss_taps(31, 51)
    filt = hip.Filter(taps, hip.ORDER_AVX)
    dtaps = S.gauss_taps(62, 52)
    deci = hip.Decimator(5, dtaps, hip.ORDER_AVX, complex_=True)
    assert filt.num_coeffs == 32 and deci.num_coeffs == 64
    x = S.real_block(12000, seed=53)
    xc = S.cfloat_block(12000, seed=54)
    for name, d, w, src, Lp, factor in (("sdrhip_filter", filt, 1, x, 32, 1), ("sdrhip_decimator", deci, 2, xc, 64, 5)):
        one, cross = name + "_one", name + "_cross"
        num = 20
        need = (num - 1) * factor + Lp
        last, nxt = src[:10 * w], src[10 * w:]
        if w == 1:
            def ref(n, a, b):
                return oracle.decimate_cross_r(factor, _pad(taps, 8), n, a, b)
        else:
            def ref(n, a, b):
                return oracle.decimate_cross_c(factor, _pad(dtaps, 4), n, a, b)
        # num = 0: OK, nothing read (null vectors), nothing written
        g = GuardedOut(8)
        assert getattr(lib, one)(d.h, 0, None, _fp(g.out)) == 0 and g.untouched()
        assert getattr(lib, cross)(d.h, 0, None, 0, None, 0, _fp(g.out)) == 0 and g.untouched()
        # refused
        g = GuardedOut(num * w)
        _refused(hip, one, None, num, _fp(src), g)
        _refused(hip, one, d.h, -1, _fp(src), g)
        _refused(hip, cross, None, num, _fp(last), 10, _fp(nxt), need - 10, g)
        _refused(hip, cross, d.h, -1, _fp(last), 10, _fp(nxt), need - 10, g)
        _refused(hip, cross, d.h, num, _fp(last), -1, _fp(nxt), need, g)
        _refused(hip, cross, d.h, num, _fp(last), 10, _fp(nxt), -1, g)
        _refused(hip, cross, d.h, num, _fp(last), 10, _fp(nxt), need - 11, g)            # one element too few
        # exactly enough
        assert getattr(lib, cross)(d.h, num, _fp(last), 10, _fp(nxt), need - 10, _fp(g.out)) == 0, _last_error(hip)
        g.check(cross)
        assert_bit_equal(g.out, ref(num, last, nxt[:(need - 10) * w]), f"{cross} with exactly enough elements")
        # everything in `last` (and more of it than the outputs read), nothing in `next`
        g = GuardedOut(num * w)
        long_last = src[:(need + 100) * w]
        assert getattr(lib, cross)(d.h, num, _fp(long_last), need + 100, _fp(nxt), 0, _fp(g.out)) == 0, _last_error(hip)
        g.check(cross)
        assert_bit_equal(g.out, ref(num, long_last, nxt), f"{cross} with every element in last")
        # `next` far longer than needed
        g = GuardedOut(num * w)
        short_last = src[:3 * w]
        far = src[3 * w:]
        assert far.size // w > 50 * need
        assert getattr(lib, cross)(d.h, num, _fp(short_last), 3, _fp(far), far.size // w, _fp(g.out)) == 0, _last_error(hip)
        g.check(cross)
        assert_bit_equal(g.out, ref(num, short_last, far), f"{cross} with a long next")
        # _one on an array that holds NaN from element `need` onwards: the C kernel reads `need` elements and not one more
        num1 = 333
        need1 = (num1 - 1) * factor + Lp
        poisoned = src[:(need1 + 300) * w].copy()
        poisoned[need1 * w:] = np.nan
        out = _fir_one(hip, one, d, num1, poisoned, w)
        assert not np.isnan(out).any(), f"{one} read past the {need1} elements its outputs need"
        exp = oracle.filter_rr(8, num1, _pad(taps, 8), poisoned) if w == 1 else oracle.decimate_rc(4, num1, factor, duplicate(_pad(dtaps, 4)), poisoned)
        assert_bit_equal(out, exp, one)


@pytest.mark.parametrize("cplx", [False, True], ids=["r", "c"])
def test_resampler_call_edges(hip, oracle, cplx):
    lib = hip.lib
    I, D, w = 3, 10, 2 if cplx else 1
    rt = S.gauss_taps(31, 55)
    r = hip.Resampler(I, D, rt, hip.ORDER_AVX, complex_=cplx)
    prep = oracle.prepare_coeffs(8, I, D, rt)
    assert r.num_coeffs == 48 and r.num_groups == 3 and prep["padded_len"] == 16 and list(prep["offsets"]) == [0, 2, 1]
    src = S.cfloat_block(6000, seed=56) if cplx else S.real_block(6000, seed=56)
    one_ref = (lambda n, g, a: oracle.resample_rc(4, n, prep, g, a)) if cplx else (lambda n, g, a: oracle.resample_rr(8, n, prep, g, a))
    cross_ref = oracle.resample_cross_c if cplx else oracle.resample_cross_r
    # num = 0: the given group / the given offset, nothing read, nothing written
    g = GuardedOut(8)
    for group in range(3):
        assert lib.sdrhip_resampler_one(r.h, group, 0, None, 0, _fp(g.out)) == group and g.untouched()
    for fo in range(I):
        assert lib.sdrhip_resampler_cross(r.h, fo, 0, None, 0, None, 0, _fp(g.out)) == fo and g.untouched()
    # refused
    num, fo = 20, 2
    need = _resampler_cross_need(I, D, rt.size, fo, num)
    last, nxt = src[:10 * w], src[10 * w:]
    g = GuardedOut(num * w)
    _refused(hip, "sdrhip_resampler_one", None, 0, num, _fp(src), 6000, g)
    _refused(hip, "sdrhip_resampler_one", r.h, 3, num, _fp(src), 6000, g)                 # group >= num_groups
    _refused(hip, "sdrhip_resampler_one", r.h, -1, num, _fp(src), 6000, g)
    _refused(hip, "sdrhip_resampler_one", r.h, 0, -1, _fp(src), 6000, g)
    _refused(hip, "sdrhip_resampler_one", r.h, 0, num, _fp(src), -1, g)
    _refused(hip, "sdrhip_resampler_cross", None, fo, num, _fp(last), 10, _fp(nxt), need - 10, g)
    _refused(hip, "sdrhip_resampler_cross", r.h, I, num, _fp(last), 10, _fp(nxt), need - 10, g)      # filter_offset >= I
    _refused(hip, "sdrhip_resampler_cross", r.h, -1, num, _fp(last), 10, _fp(nxt), need - 10, g)
    _refused(hip, "sdrhip_resampler_cross", r.h, fo, -1, _fp(last), 10, _fp(nxt), need - 10, g)
    _refused(hip, "sdrhip_resampler_cross", r.h, fo, num, _fp(last), -1, _fp(nxt), need, g)
    _refused(hip, "sdrhip_resampler_cross", r.h, fo, num, _fp(last), 10, _fp(nxt), -1, g)
    _refused(hip, "sdrhip_resampler_cross", r.h, fo, num, _fp(last), 10, _fp(nxt), need - 11, g)     # one element too few
    # exactly enough
    o2 = lib.sdrhip_resampler_cross(r.h, fo, num, _fp(last), 10, _fp(nxt), need - 10, _fp(g.out))
    assert o2 >= 0, _last_error(hip)
    g.check("sdrhip_resampler_cross")
    exp, eo = cross_ref(I, D, rt, fo, num, last, nxt[:(need - 10) * w])
    assert_bit_equal(g.out, exp, "resampleCross with exactly enough elements")
    assert o2 == eo
    # everything in `last` (more than the outputs read), nothing in `next`; and a `next` far longer than needed
    long_last, short_last, far = src[:(need + 100) * w], src[:3 * w], src[3 * w:]
    assert far.size // w > 50 * need
    for a, b, nb, what in ((long_last, nxt, 0, "every element in last"), (short_last, far, far.size // w, "a long next")):
        g = GuardedOut(num * w)
        o2 = lib.sdrhip_resampler_cross(r.h, fo, num, _fp(a), a.size // w, _fp(b), nb, _fp(g.out))
        assert o2 >= 0, _last_error(hip)
        g.check("sdrhip_resampler_cross")
        exp, eo = cross_ref(I, D, rt, fo, num, a, b)
        assert_bit_equal(g.out, exp, f"resampleCross with {what}")
        assert o2 == eo
    # resampleOne on an array that holds NaN from element `need` onwards (the whole array is declared): no NaN
    for group in range(3):
        num1 = 333
        m0 = next(m for m in range(4 * I + 4) if r.group(m) == group)
        need1 = r.in_offset(m0 + num1 - 1) - r.in_offset(m0) + prep["padded_len"]
        poisoned = src[:(need1 + 300) * w].copy()
        poisoned[need1 * w:] = np.nan
        g = GuardedOut(num1 * w)
        g2 = lib.sdrhip_resampler_one(r.h, group, num1, _fp(poisoned), poisoned.size // w, _fp(g.out))
        assert g2 >= 0, _last_error(hip)
        g.check("sdrhip_resampler_one")
        assert not np.isnan(g.out).any(), f"sdrhip_resampler_one read past the {need1} elements its walk covers"
        exp, eg = one_ref(num1, group, poisoned)
        assert_bit_equal(g.out, exp, f"resampleOne from group {group}")
        assert g2 == eg
    # n_in short of the SIMD walk: the last output's group has 11 (group 0) or 10 taps, the loop walks 16; the vector ends where
    # the taps end and NaN follows it in memory.  Past the caller's vector the taps are zero: the answer is the oracle's on the
    # zero-extended vector.
    for num1 in (331, 332, 333):
        last_group = (num1 - 1) % 3
        start = r.in_offset(num1 - 1)
        n_in = start + (11 if last_group == 0 else 10)
        assert n_in < start + prep["padded_len"]
        arr = np.full((n_in + 64) * w, np.nan, np.float32)
        arr[:n_in * w] = src[:n_in * w]
        g = GuardedOut(num1 * w)
        g2 = lib.sdrhip_resampler_one(r.h, 0, num1, _fp(arr), n_in, _fp(g.out))
        assert g2 >= 0, _last_error(hip)
        g.check("sdrhip_resampler_one")
        extended = np.concatenate([src[:n_in * w], np.zeros(64 * w, np.float32)])
        exp, eg = one_ref(num1, 0, extended)
        assert not np.isnan(exp).any()
        assert_bit_equal(g.out, exp, f"resampleOne of {num1} outputs on a vector {start + 16 - n_in} short of the walk")
        assert g2 == eg


# ---- threads ---------------------------------------------------------------------------------------------------------------------
def test_record_pipes_from_four_threads(hip, oracle):
    """scratch_pool.hpp: the closures of several pipelines do not queue behind one another -- and do not share state.  Four threads,
    each running its own device-backed Pipe five times: a complex decimator, a symmetric real filter and two resampler Pipes (another
    output block size each) on ONE shared descriptor.  Every run equals the single-threaded run of the same Pipe, bit for bit."""
    dec = RC.Case("fir", "avx", True, 8, 127, 1, 8)
    sym = RC.Case("sym", "sse", False, 1, 32, 1, 1)
    res = RC.Case("resampler", "avx", False, 1, 191, 3, 10)
    assert {dec, sym, res} <= set(RC.CASES)
    shared = hip.Resampler(res.I, res.D, RC.taps(res), hip.ORDER_AVX)
    jobs = [(dec, 97, None), (sym, 1000, None), (res, 97, shared), (res, 1000, shared)]
    single = []
    for c, ob, desc in jobs:
        run = _run(c, _device_model(c, oracle, desc), ob)
        _assert_same_run(c, ob, run, _run(c, RC.make_model(c, oracle), ob), "single-threaded")
        single.append(run)
    errors = []
    start = threading.Barrier(len(jobs))

    def work(job, exp):
        c, ob, desc = job
        try:
            start.wait(timeout=60)
            for i in range(5):
                _assert_same_run(c, ob, _run(c, _device_model(c, oracle, desc), ob), exp, f"threaded run {i}")
        except Exception as e:          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(j, e)) for j, e in zip(jobs, single)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors[0]
