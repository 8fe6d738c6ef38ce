"""The waterfall Pipe (sdrhip_pipe_spectrum) on the device.  Its definition is ONE sdrhip_spectrum_reduce_run_device over the
concatenation of every push: on the one-kernel route every row the Pipe hands out is compared BIT FOR BIT with that call's row, for
u8, cfloat and int16 blocks, push sizes uniform, ragged (1-sample pushes included) and one huge one, plain, coalesced and adaptive;
on the hipFFT route the operator's tolerance contract against the numpy model holds.  The bookkeeping (which push completes how many
rows; pushes that complete none launch nothing; one launch per submission) is held to tests/spectrum_pipe_model.py.  Every pop goes
between canaries."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

import gpu_util as G
import spectrum_model as M
import spectrum_pipe_model as SP
import spectrum_reduce_model as R
from gpu_util import CANARY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMATS = ("u8", "cf32", "i16")
FLOOR = -150.0
ERR_ARG = -1
PAD = 16
_f32p = C.POINTER(C.c_float)
_cache = {}


def fmt_id(hip, fmt):
    return {"u8": hip.IQ_U8, "cf32": hip.IQ_CF32, "i16": hip.IQ_I16}[fmt]


def spectrum(hip, fmt, n, route=None):
    s = hip.Spectrum(n, fmt_id(hip, fmt), hip.WINDOW_HANNING, True, 1.0 / n)
    if route is not None:
        s.set_route(route)
    return s


def stream(fmt, nsamples):
    key = (fmt, nsamples)
    if key not in _cache:
        s = SP.stream(fmt, nsamples)
        s.setflags(write=False)
        _cache[key] = s
    return _cache[key]


def reference(hip, fmt, n, hop, group, reduce, unit, nsamples):
    """Every row of the stream's first nsamples samples from ONE reduce_device call; computed once, shared, never written."""
    key = ("ref", fmt, n, hop, group, reduce, unit, nsamples)
    if key not in _cache:
        iq = stream(fmt, nsamples)
        rows = SP.brute_force(n, hop, group, nsamples)[0]
        d_out = G.dev_empty_f32(rows * n)
        spec = spectrum(hip, fmt, n)
        assert spec.reduce_device(G.ptr(G.to_dev(iq)), nsamples, G.ptr(d_out), group, reduce, unit, FLOOR, hop=hop, rows_out=rows) == rows
        ref = G.to_host(d_out).reshape(rows, n).copy()
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def canary_pop(hip, p, ready):
    """`ready` rows through sdrhip_pipe_pop, each into n floats between two bands of canaries."""
    n, rows = p.block_size_out, []
    for _ in range(ready):
        o = np.full(n + 2 * PAD, CANARY, np.uint32)
        got = hip.lib.sdrhip_pipe_pop(p.h, o[PAD:].view(np.float32).ctypes.data_as(_f32p), n)
        assert got == n, hip.lib.sdrhip_last_error()
        assert (o[:PAD] == CANARY).all() and (o[PAD + n:] == CANARY).all(), "a pop wrote outside its row"
        rows.append(o[PAD:PAD + n].view(np.float32).copy())
    return rows


def pipe(hip, spec, hop, group, reduce=1, unit=0, mode="plain"):
    p = hip.Pipe.spectrum(spec, hop, group, reduce, unit, FLOOR)
    p._pop = lambda ready: canary_pop(hip, p, ready)
    if mode == "plain":
        p.set_adaptive(0)
    elif mode == "coalesce":
        p.set_coalesce(4)
    else:
        p.set_adaptive(16)
    return p


def same_rows(got, ref, what):
    assert len(got) == ref.shape[0], f"{what}: {len(got)} rows, the one call gives {ref.shape[0]}"
    g = np.stack(got) if got else np.zeros((0, ref.shape[1]), np.float32)
    bad = np.nonzero((g.view(np.uint32) != ref.view(np.uint32)).any(axis=1))[0]
    assert bad.size == 0, f"{what}: rows {bad[:8].tolist()} differ from the one call's"


def geometries(n):
    return [(n, 1), (n // 2, 3), (n + 37, 2), (n, 33)]


# ---- the matrix ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [64, 2048])
@pytest.mark.parametrize("fmt", FORMATS)
def test_every_push_pattern_gives_the_one_calls_rows(hip, fmt, n):
    """u8 / cfloat / int16 x n x (hop, group) x {pushes of n, pushes of 8192, ragged, one push}.  Plain submission, so the launch counts
    are the model's: a push that completes no row launches nothing, one that completes rows is exactly one fused launch."""
    for hop, group in geometries(n):
        few = SP.samples_for(n, hop, 5, group) + 11                # five rows and a rest
        many = max(SP.samples_for(n, hop, 24, group) + 5, 8192 * 3 + 100)
        patterns = {"pushes of n": (few, [n] * (few // n) + ([few % n] if few % n else [])),
                    "pushes of 8192": (many, [8192] * (many // 8192) + [many % 8192]),
                    "ragged": (few, SP.ragged_sizes(n + hop + group, few)),
                    "one push": (many, [many])}
        spec = spectrum(hip, fmt, n)
        for name, (total, sizes) in patterns.items():
            assert sum(sizes) == total
            ref = reference(hip, fmt, n, hop, group, 1, 0, total)
            assert name != "one push" or ref.shape[0] >= 24
            p, model, got = pipe(hip, spec, hop, group), SP.PipeModel(n, hop, group), []
            for blk in SP.cut(stream(fmt, total), sizes):
                before = hip.spectrum_fused_launches()
                got += p.push(blk)
                r = model.push(blk.size // 2)
                assert hip.spectrum_fused_launches() - before == (1 if r else 0), f"{fmt} n={n} hop={hop} group={group} {name}"
            before = hip.spectrum_fused_launches()
            got += p.flush()
            assert hip.spectrum_fused_launches() == before, "flush launched although no row was complete"
            assert p.rows == 1
            same_rows(got, ref, f"{fmt} n={n} hop={hop} group={group} {name}")


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_reduce_and_unit(hip, fmt):
    n, hop, group = 64, 48, 3
    total = SP.samples_for(n, hop, 9, group) + 7
    sizes = SP.ragged_sizes(7, total)
    spec = spectrum(hip, fmt, n)
    for reduce in (0, 1, 2):
        for unit in (0, 1):
            p, got = pipe(hip, spec, hop, group, reduce, unit), []
            for blk in SP.cut(stream(fmt, total), sizes):
                got += p.push(blk)
            got += p.flush()
            same_rows(got, reference(hip, fmt, n, hop, group, reduce, unit, total), f"{fmt} reduce={reduce} unit={unit}")


# ---- throughput knobs --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_plain_coalesced_and_adaptive_give_the_same_rows(hip, fmt):
    """... with every third push written into the staging memory input_buffer* lends."""
    for n, hop, group in ((64, 32, 3), (2048, 2048 + 37, 2), (64, 64, 33)):
        total = SP.samples_for(n, hop, 20, group) + 3
        sizes = SP.ragged_sizes(n + group, total, most=max(total // 24, 2))
        ref = reference(hip, fmt, n, hop, group, 0, 1, total)
        spec = spectrum(hip, fmt, n)
        for mode in ("plain", "coalesce", "adaptive"):
            p, got = pipe(hip, spec, hop, group, 0, 1, mode), []
            for i, blk in enumerate(SP.cut(stream(fmt, total), sizes)):
                if i % 3 == 2:
                    view = p.input_buffer(blk.size // 2)
                    assert view.dtype == blk.dtype and view.size == blk.size
                    view[:] = blk
                    blk = view
                got += p.push(blk)
            got += p.flush()
            same_rows(got, ref, f"{fmt} n={n} hop={hop} group={group} {mode}")


# ---- ordering ----------------------------------------------------------------------------------------------------------------------
def test_two_hundred_one_row_pushes_through_the_scratch_layers(hip):
    """Groups of 70 rows go through the object's one scratch buffer: 200 one-row pushes made as fast as the host can, four submissions
    in flight, all ordered by one stream.  A race between slots would mix the layers of two rows."""
    n, hop, group, nb = 64, 64, 70, 200
    total = nb * group * hop
    spec = spectrum(hip, "u8", n, hip.SPECTRUM_ROUTE_FUSED)
    ref = reference(hip, "u8", n, hop, group, 0, 0, total)
    p, got = pipe(hip, spec, hop, group, 0, 0), []
    before = hip.spectrum_fused_launches()
    for blk in SP.cut(stream("u8", total), [group * hop] * nb):
        got += p.push(blk)
    got += p.flush()
    assert hip.spectrum_fused_launches() == before + nb, "every push completes exactly one row: one submission each"
    same_rows(got, ref, "200 pushes, group 70")


def test_two_hundred_one_row_pushes_on_the_hipfft_route(hip):
    n, nb = 1000, 200
    total = nb * n
    iq = stream("u8", total)
    spec = spectrum(hip, "u8", n)
    p, got = pipe(hip, spec, n, 1, R.MEAN_MAGNITUDE, R.LINEAR), []
    before = hip.spectrum_fused_launches()
    for blk in SP.cut(iq, [n] * nb):
        got += p.push(blk)
    got += p.flush()
    assert hip.spectrum_fused_launches() == before, "n = 1000 takes the hipFFT route"
    assert len(got) == nb
    mag, _ = M.spectrum(iq, n, M.IQ_U8, M.WINDOW_HANNING, None, True, 1.0 / n, n, nb)
    v, delta = R.reduce_rows(mag, 1, R.MEAN_MAGNITUDE)
    R.check(np.stack(got), v, delta, R.MEAN_MAGNITUDE, R.LINEAR, FLOOR, "200 pushes, hipFFT route")


# ---- calls -------------------------------------------------------------------------------------------------------------------------
def test_pop_capacity_and_pop_rows(hip):
    n, hop, group = 64, 32, 3
    total = SP.samples_for(n, hop, 4, group)
    ref = reference(hip, "u8", n, hop, group, 1, 0, total)
    spec = spectrum(hip, "u8", n)
    p = hip.Pipe.spectrum(spec, hop, group, 1, 0, FLOOR)
    iq = np.ascontiguousarray(stream("u8", total))
    assert hip.check(hip.lib.sdrhip_pipe_push_u8(p.h, iq.ctypes.data_as(C.POINTER(C.c_uint8)), total), "push") >= 0
    assert hip.check(hip.lib.sdrhip_pipe_flush(p.h), "flush") == 4
    o = np.full(n + 2 * PAD, CANARY, np.uint32)
    assert hip.lib.sdrhip_pipe_pop(p.h, o[PAD:].view(np.float32).ctypes.data_as(_f32p), n - 1) == ERR_ARG
    assert b"sdrhip_pipe_pop" in hip.lib.sdrhip_last_error() and (o == CANARY).all(), "a refused pop wrote"
    assert hip.check(hip.lib.sdrhip_pipe_poll(p.h), "poll") == 4, "a refused pop took a row"
    rows = canary_pop(hip, p, 1)
    o = np.full(3 * n + 2 * PAD, CANARY, np.uint32)
    assert hip.lib.sdrhip_pipe_pop_rows(p.h, o[PAD:].view(np.float32).ctypes.data_as(_f32p), 2 * n - 1, 2) == ERR_ARG and (o == CANARY).all()
    assert hip.lib.sdrhip_pipe_pop_rows(p.h, o[PAD:].view(np.float32).ctypes.data_as(_f32p), 3 * n, 3) == 3
    assert (o[:PAD] == CANARY).all() and (o[PAD + 3 * n:] == CANARY).all()
    rows += list(o[PAD:PAD + 3 * n].view(np.float32).reshape(3, n))
    same_rows(rows, ref, "pop and pop_rows")
    assert hip.lib.sdrhip_pipe_pop(p.h, o[PAD:].view(np.float32).ctypes.data_as(_f32p), n) == 0, "no row left"


def test_the_wrong_call_for_the_pipes_type_is_refused(hip):
    push = {"cf32": ("sdrhip_pipe_push", _f32p), "u8": ("sdrhip_pipe_push_u8", C.POINTER(C.c_uint8)), "i16": ("sdrhip_pipe_push_i16", C.POINTER(C.c_int16))}
    lend = {"cf32": "sdrhip_pipe_input_buffer", "u8": "sdrhip_pipe_input_buffer_u8", "i16": "sdrhip_pipe_input_buffer_i16"}
    n = 64
    data = {f: np.ascontiguousarray(stream(f, 4 * n)) for f in FORMATS}
    before = hip.spectrum_fused_launches()
    for fmt in FORMATS:
        p = hip.Pipe.spectrum(spectrum(hip, fmt, n))
        for other in FORMATS:
            if other == fmt:
                continue
            name, ptr_t = push[other]
            assert getattr(hip.lib, name)(p.h, data[other].ctypes.data_as(ptr_t), 4 * n) == ERR_ARG, f"{other} blocks into a {fmt} pipe"
            assert name.encode() + b":" in hip.lib.sdrhip_last_error()
            assert not getattr(hip.lib, lend[other])(p.h, n), f"{lend[other]} on a {fmt} pipe"
            with pytest.raises(hip.SdrHipError):
                p.push(data[other])
        assert p.flush() == [], "a refused push staged something"
    assert hip.spectrum_fused_launches() == before


# ---- save / restore ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("hop,group,what", [(32, 3, "mid-group"), (64 + 37, 2, "skip pending")])
def test_save_and_restore(hip, fmt, hop, group, what):
    n = 64
    first = [50, 1, 99, 7, 23]                                   # 180 samples: row 0 done; 84 samples into row 1's group / 22 still to skip
    total = SP.samples_for(n, hop, 12, group) + 9
    sizes = first + SP.ragged_sizes(11, total - sum(first), most=(total - sum(first)) // 20)[:34]
    sizes.append(total - sum(sizes))
    assert len(sizes) == 40 and sizes[-1] >= 1
    blocks = SP.cut(stream(fmt, total), sizes)
    ref = reference(hip, fmt, n, hop, group, 0, 1, total)
    spec = spectrum(hip, fmt, n)
    args = (hop, group, 0, 1, FLOOR)
    a, got_a = pipe(hip, spec, *args), []
    for blk in blocks[:5]:
        got_a += a.push(blk)
    state = a.save()
    got_a += a.poll()
    h = SP.StateHeader.from_buffer_copy(state[:C.sizeof(SP.StateHeader)])
    assert (h.version, h.kind, h.n, h.group, h.hop, h.pos, h.rows_done) == (3, 10, n, group, hop, 180, 1)
    assert h.input_type == {"cf32": 0, "u8": 1, "i16": 2}[fmt]
    assert (h.tail_n > 0 and h.skip == 0) if what == "mid-group" else (h.tail_n == 0 and h.skip == 22)
    assert len(state) == C.sizeof(SP.StateHeader) + h.tail_n * SP.SAMPLE_BYTES[fmt] + 4 * h.pending

    def refused(p, st, why):
        assert hip.lib.sdrhip_pipe_restore(p.h, st, C.c_size_t(len(st))) == ERR_ARG, why
        assert b"sdrhip_pipe_restore" in hip.lib.sdrhip_last_error(), why

    b = pipe(hip, spec, *args)
    for cutoff in (len(state) - 1, C.sizeof(SP.StateHeader) - 1, 40, 12):
        refused(b, state[:cutoff], f"a state truncated to {cutoff} bytes")
    am = hip.Pipe.am_demod()
    am.push(np.zeros(16, np.float32))
    refused(b, am.save(), "an amDemod pipe's state")
    refused(hip.Pipe.am_demod(), state, "a waterfall state into an amDemod pipe")
    other_fmt = "u8" if fmt != "u8" else "i16"
    different = {"n": hip.Pipe.spectrum(spectrum(hip, fmt, 128), *args),
                 "input type": hip.Pipe.spectrum(spectrum(hip, other_fmt, n), *args),
                 "hop": hip.Pipe.spectrum(spec, hop + 1, group, 0, 1, FLOOR),
                 "group": hip.Pipe.spectrum(spec, hop, group + 1, 0, 1, FLOOR),
                 "reduce": hip.Pipe.spectrum(spec, hop, group, 1, 1, FLOOR),
                 "unit": hip.Pipe.spectrum(spec, hop, group, 0, 0, FLOOR),
                 "floor_db": hip.Pipe.spectrum(spec, hop, group, 0, 1, FLOOR + 1.0)}
    for name, q in different.items():
        refused(q, state, f"another {name}")
        assert hip.lib.sdrhip_pipe_poll(q.h) == 0 and q.flush() == [], f"another {name}: the refused restore left rows behind"
    refused(b, SP.patch_state(state, tail_n=h.tail_n + 1), "a tail that does not start where the next row does")
    assert hip.lib.sdrhip_pipe_poll(b.h) == 0
    got_b = b.restore(state)                                     # ... and after all those refusals the pipe is as fresh as it was
    # the same state moved beyond 2^33 samples by a whole number of groups
    k = (1 << 33) // (group * hop) + 1
    far = SP.patch_state(state, pos=h.pos + k * group * hop, rows_done=h.rows_done + k)
    c = pipe(hip, spec, *args)
    got_c = c.restore(far)
    for blk in blocks[5:]:
        got_a += a.push(blk)
        got_b += b.push(blk)
        got_c += c.push(blk)
    got_a += a.flush()
    got_b += b.flush()
    got_c += c.flush()
    same_rows(got_a, ref, f"the saved pipe, {fmt}, {what}")
    done_before = h.rows_done - h.pending // n                   # rows the first pipe had popped before the save
    same_rows(got_b, ref[done_before:], f"the restored pipe, {fmt}, {what}")
    same_rows(got_c, ref[done_before:], f"the pipe restored beyond 2^33 samples, {fmt}, {what}")
    far_state = c.save()
    hf = SP.StateHeader.from_buffer_copy(far_state[:C.sizeof(SP.StateHeader)])
    assert hf.pos == total + k * group * hop and hf.pos > 1 << 33 and hf.rows_done == ref.shape[0] + k


def test_saved_states_of_every_existing_kind_keep_their_bytes(hip):
    import pipe_am_bank_cases as PC
    states = SP.existing_kind_states(hip)
    want = dict(PC.PARENT_STATE_SHA256, am_bank=SP.PARENT_AM_BANK_STATE_SHA256)
    assert set(states) == set(want) and len(states) == 10
    for kind, st in states.items():
        assert hashlib.sha256(st).hexdigest() == want[kind], f"the saved state of a {kind} pipe changed"


# ---- the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args", [[], ["--s16"], ["--hop", "512", "--group", "3", "--db", "--reduce", "power"],
                                  ["--s16", "--n", "2048", "--hop", "1000", "--group", "3", "--db", "--reduce", "max", "--window", "blackman", "--shift"]])
def test_waterfall_replay_example(hip, args, tmp_path):
    """examples/waterfall_replay.c against the same Pipe driven from the binding with the same pushes of 8192 samples."""
    exe = os.path.join(ROOT, "examples", "bin", "waterfall_replay")
    assert os.path.exists(exe), "build() makes the examples"
    fmt = "i16" if "--s16" in args else "u8"
    opt = {args[i]: args[i + 1] for i in range(len(args) - 1) if args[i] in ("--n", "--hop", "--group", "--reduce", "--window")}
    n = int(opt.get("--n", 1024))
    hop, group = int(opt.get("--hop", n)), int(opt.get("--group", 1))
    reduce = {"power": 0, "mag": 1, "max": 2}[opt.get("--reduce", "mag")]
    window = {"hanning": hip.WINDOW_HANNING, "blackman": hip.WINDOW_BLACKMAN}[opt.get("--window", "hanning")]
    total = 5 * 8192 + 1234
    s = stream(fmt, total)
    cap, out = tmp_path / "capture.bin", tmp_path / "rows.f32"
    s.tofile(cap)
    r = subprocess.run([exe, str(cap), str(out)] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    spec = hip.Spectrum(n, fmt_id(hip, fmt), window, "--shift" in args, 1.0)
    p = hip.Pipe.spectrum(spec, hop, group, reduce, hip.UNIT_DB if "--db" in args else hip.UNIT_LINEAR, -200.0)
    rows = []
    for blk in SP.cut(s, [8192] * 5 + [1234]):
        rows += p.push(blk)
    rows += p.flush()
    assert len(rows) == SP.brute_force(n, hop, group, total)[0] >= 4
    got = np.fromfile(str(out), np.float32)
    assert got.tobytes() == np.concatenate(rows).tobytes(), f"waterfall_replay {' '.join(args)}"
