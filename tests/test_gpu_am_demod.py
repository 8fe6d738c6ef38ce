"""GPU: amDemod, the AM receiver's envelope detector (sdrhip_am_demod_run, sdrhip_am_demod_run_rows, sdrhip_pipe_am_demod,
examples/am_replay.c).

Every comparison is bit for bit against agc_model.magnitude, NaN by position (am_demod_cases.same).  Output buffers start as NaN
canaries, and every float outside the outputs -- before, between and behind the rows -- is a canary afterwards; the gaps between
input rows hold NaN, so a kernel that reads past a row computes on NaN.  sdrhip_debug_am_demod_launches counts the kernel's
launches: one per call, none for n == 0.

The inputs are those of tests/am_demod_cases.py (directed pairs, a normal stream, a wide-exponent stream);
tests/test_am_demod_cases.py shows on the CPU what they reach.  One workgroup's span is 256 threads x 4 samples = 1024 samples."""
import os
import subprocess

import numpy as np
import pytest
import torch

import am_demod_cases as AC
import gpu_util
import signals as S
from conftest import assert_bit_equal
from gpu_util import CANARY
from test_gpu_rows import Rows, _floats

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPAN = 1024
LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, SPAN - 1, SPAN, SPAN + 1, 3 * SPAN + 3)
NMAX = 3 * SPAN + 3
MAX_ROWS = 65

_rows_cache = {}


def row_input(r):
    """(input, truth) of row r at the longest length; AC.mixed is prefix-stable, so row r of length n is their first n samples."""
    if r not in _rows_cache:
        z = AC.mixed(NMAX, seed=r)
        e = AC.expected(z)
        z.setflags(write=False)
        e.setflags(write=False)
        _rows_cache[r] = (z, e)
    return _rows_cache[r]


def test_prefixes_of_a_row_are_rows():
    for n in (5, 27, 100):
        assert np.array_equal(AC.mixed(n, seed=3).view(np.uint32), row_input(3)[0][:n].view(np.uint32))


def run_one(hip, z, in_off=0, out_off=0, what=""):
    """sdrhip_am_demod_run on z, the input in_off floats and the output out_off floats behind a 256-byte boundary -> (output, launches)."""
    n = z.size
    src = Rows(1, 2 * n, 0, in_off, host=[z])
    dst = Rows(1, n, 0, out_off)
    l0, r0 = hip.am_demod_launches(), hip.rows_launches()
    hip.am_demod(src.view, n, dst.view)
    launches = hip.am_demod_launches() - l0
    assert hip.rows_launches() == r0
    return dst.read(what)[0], launches


def run_rows(hip, zs, in_extra=0, out_extra=0, in_off=0, out_off=0, what=""):
    rows, n = len(zs), zs[0].size
    src = Rows(rows, 2 * n, in_extra, in_off, host=zs)
    dst = Rows(rows, n, out_extra, out_off)
    l0 = hip.am_demod_launches()
    hip.am_demod_rows(src.view, out=dst.view)
    return dst.read(what), hip.am_demod_launches() - l0


# ---- 1: one row ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["directed", "normal", "wide"])
def test_the_three_inputs(hip, name):
    z = AC.inputs()[name]
    got, launches = run_one(hip, z, what=name)
    assert launches == 1
    AC.assert_same(got, AC.expected(z), f"amDemod on the {name} input")
    if name == "directed":
        for (re, im, want), g in zip(AC.DIRECTED, got):
            print(f"    magnitude({re!r}, {im!r}) = {g!r} ({int(g.view(np.uint32)):#010x})")
            assert np.isnan(g) if want is None else int(g.view(np.uint32)) == want, (re, im, g)


def test_one_row_lengths(hip):
    z, e = row_input(0)
    for n in LENGTHS:
        got, launches = run_one(hip, z[:n], what=f"n = {n}")
        assert launches == (1 if n else 0), f"n = {n}: {launches} launches"
        AC.assert_same(got, e[:n], f"amDemod, one row of {n}")


@pytest.mark.parametrize("in_off", [0, 1, 2, 3])
@pytest.mark.parametrize("out_off", [0, 1, 2])
def test_one_row_base_alignment(hip, in_off, out_off):
    """The input 0 / 4 / 8 / 12 bytes and the output 0 / 4 / 8 bytes past a 16-byte boundary: 16- / 4- / 8- / 4-byte loads against
    16- / 4- / 8-byte stores, every pair of them."""
    z, e = row_input(1)
    for n in (3, 9, SPAN + 1, NMAX):
        got, launches = run_one(hip, z[:n], in_off, out_off, what=f"n = {n}, input +{4 * in_off} B, output +{4 * out_off} B")
        assert launches == 1
        AC.assert_same(got, e[:n], f"amDemod, one row of {n}, input +{4 * in_off} B, output +{4 * out_off} B")


# ---- 2: rows --------------------------------------------------------------------------------------------------------------------------
# (input gap, output gap, input offset, output offset) in floats: tight, +2 / +1, +6 / +3, and bases off 16-byte alignment
LAYOUTS = [(0, 0, 0, 0), (2, 1, 0, 0), (6, 3, 0, 0), (2, 3, 2, 1), (6, 1, 0, 2)]


@pytest.mark.parametrize("rows", [1, 3, MAX_ROWS])
def test_rows_lengths_and_layouts(hip, rows):
    zs, es = zip(*[row_input(r) for r in range(rows)])
    for n in LENGTHS:
        for lay in (LAYOUTS if n in (5, 9, SPAN + 1, NMAX) else LAYOUTS[:2]):
            what = f"{rows} rows of {n}, layout {lay}"
            outs, launches = run_rows(hip, [z[:n] for z in zs], *lay, what=what)
            assert launches == (1 if n else 0), f"{what}: {launches} launches"
            for r in range(rows):
                AC.assert_same(outs[r], es[r][:n], f"{what}, row {r}")
        if n in (5, SPAN + 1, NMAX):
            for r in sorted({0, rows // 2, rows - 1}):
                one, _ = run_one(hip, zs[r][:n])
                assert_bit_equal(outs[r], one, f"{rows} rows of {n}, row {r} vs the one-row call")


@pytest.mark.parametrize("poison", [np.nan, np.inf])
def test_a_neighbour_of_nan_or_inf_changes_nothing(hip, poison):
    for n in (7, SPAN + 1):
        zs = [row_input(r)[0][:n].copy() for r in range(3)]
        zs[1][:] = complex(poison, poison)
        outs, _ = run_rows(hip, zs, 2, 1, what=f"a row of {poison}")
        for r in (0, 2):
            AC.assert_same(outs[r], row_input(r)[1][:n], f"row {r} beside a row of {poison}, n = {n}")
        assert np.isnan(outs[1]).all() if np.isnan(poison) else (outs[1].view(np.uint32) == AC.PINF).all()


def _sliding(rows, n):
    """rows x n samples, row r = base[r : r + n] of one mixed stream, and their truth: one reference for 1024 rows."""
    base = AC.mixed(n + rows, seed=7)
    e = AC.expected(base)
    win = np.lib.stride_tricks.sliding_window_view
    return np.ascontiguousarray(win(base, n)[:rows]), win(e, n)[:rows]


@pytest.mark.parametrize("n,lay", [(100, (2, 1, 0, 0)), (8193, (0, 0, 0, 0)), (20481, (0, 0, 0, 0))], ids=["1024 x 100", "1024 x 8193", "1024 x 20481"])
def test_1024_rows(hip, n, lay):
    """SDRHIP_ROWS_MAX rows in one launch.  An odd count a row: tight output rows start at every 4-byte alignment (4-byte stores), the
    input rows 8 bytes apart in alignment (8-byte loads).  At 1024 rows a row's share of the grid is 16 workgroups = 16384 samples:
    20481 samples a row is the size at which the workgroups loop over a row."""
    zs, es = _sliding(1024, n)
    outs, launches = run_rows(hip, list(zs), *lay, what=f"1024 rows of {n}")
    assert launches == 1
    got = np.stack(outs)
    bad = ~AC.same(got, es)
    assert not bad.any(), f"1024 rows of {n}: {int(bad.sum())} floats differ, first in row {int(np.nonzero(bad.any(axis=1))[0][0])}"
    with pytest.raises(hip.SdrHipError):
        hip.am_demod_rows(torch.zeros((1025, 8), device="cuda"), out=torch.zeros((1025, 4), device="cuda"))


def test_row_offsets_are_64_bit(hip):
    """Two rows 2^31 + 6 floats apart on the input side with tight output rows, then the other way round, n = 129: one buffer of about
    8.6 GB, allocated uninitialised and touched only at the rows.  A 32-bit row offset would put row 1 somewhere else."""
    stride, n = 2 ** 31 + 6, 129
    zs = [row_input(r)[0][:n] for r in (4, 5)]
    es = [row_input(r)[1][:n] for r in (4, 5)]
    big = torch.empty(stride + 2 * n + 64, dtype=torch.float32, device="cuda")
    try:
        far = big.as_strided((2, 2 * n), (stride, 1))
        for r in range(2):
            far[r].copy_(torch.from_numpy(_floats(zs[r]).copy()))
        dst = Rows(2, n)
        l0 = hip.am_demod_launches()
        hip.am_demod_rows(far, out=dst.view)
        assert hip.am_demod_launches() - l0 == 1
        outs = dst.read("far input rows")
        for r in range(2):
            AC.assert_same(outs[r], es[r], f"input rows 2^31 + 6 floats apart, row {r}")
        src = Rows(2, 2 * n, host=zs)
        far_out = big.as_strided((2, n), (stride, 1))
        big[:n + 32].view(torch.int32).fill_(CANARY)
        big[stride - 32: stride + n + 32].view(torch.int32).fill_(CANARY)
        hip.am_demod_rows(src.view, out=far_out)
        torch.cuda.synchronize()
        for r in range(2):
            AC.assert_same(far_out[r].cpu().numpy(), es[r], f"output rows 2^31 + 6 floats apart, row {r}")
        near = torch.cat([big[n: n + 32], big[stride - 32: stride], big[stride + n: stride + n + 32]])
        assert (near.view(torch.int32) == CANARY).all().item(), "floats around the far output rows were written"
    finally:
        del big
        torch.cuda.empty_cache()


def test_refusals_on_the_device_write_nothing(hip):
    n = 100
    src, dst = Rows(3, 2 * n, host=[row_input(r)[0][:n] for r in range(3)]), Rows(3, n)
    run = hip.lib.sdrhip_am_demod_run_rows
    l0 = hip.am_demod_launches()
    pi, po = src.view.data_ptr(), dst.view.data_ptr()
    for what, args in (("rows = 0", (pi, 2 * n, po, n, 0, n)), ("rows = 1025", (pi, 2 * n, po, n, 1025, n)), ("n < 0", (pi, 2 * n, po, n, 3, -1)),
                       ("in_stride < 2n", (pi, 2 * n - 2, po, n, 3, n)), ("odd in_stride", (pi, 2 * n + 1, po, n, 3, n)),
                       ("out_stride < n", (pi, 2 * n, po, n - 1, 3, n)), ("in place", (pi, 2 * n, pi, n, 3, n)), ("null input", (None, 2 * n, po, n, 3, n)),
                       ("null output", (pi, 2 * n, None, n, 3, n))):
        assert run(None, *args) == -1, what
        assert b"sdrhip_am_demod_run_rows" in hip.lib.sdrhip_last_error(), what
    assert hip.lib.sdrhip_am_demod_run(None, pi, pi, n) == -1 and hip.lib.sdrhip_am_demod_run(None, pi, po, -1) == -1
    torch.cuda.synchronize()
    assert hip.am_demod_launches() == l0 and dst.untouched()


# ---- 3: behind a bank -----------------------------------------------------------------------------------------------------------------
def test_am_receiver_behind_a_tuner_bank_on_one_stream(hip, oracle):
    """TunerBank.run -> am_demod_rows -> dc_blocker_rows -> Resampler.run_rows -> Filter.run_rows for three channels, every stage
    enqueued on one stream with nothing in between, am_demod_rows reading the bank's rows where they lie (stride 2 n + 6).  Expected,
    row by row: the restated tuner Pipe (tests/tuner_model.py), agc_model.magnitude, the oracle's dc_blocker, and the restated
    firResampler and firFilter Pipes on one block."""
    from oracle import pipes_model as PM
    from test_gpu_rows import _tuner_bank_rows
    bank, d_in, exp, n, B = _tuner_bank_rows(hip, oracle)
    rtaps, half = S.taps_example_audio_resampler(), S.taps_example_audio_filter_half()
    res = hip.Resampler(3, 10, rtaps, hip.ORDER_AVX)
    fil = hip.Filter(half, hip.ORDER_AVX, sym=True)
    rm, fm = PM.ResamplerModel(oracle, 3, 10, rtaps, PM.ORDER_AVX), PM.FilterModel(oracle, half, PM.ORDER_AVX, sym=True)
    n3 = (n * 3 - rm.num_coeffs) // 10 + 1                    # what firResampler computes from one block of n
    n4 = n3 - fm.num_coeffs + 1
    assert rm.num_coeffs == res.num_coeffs and fm.num_coeffs == fil.num_coeffs and n4 > 64
    assert res.in_offset(n3 - 1) + res.num_coeffs // 3 <= n
    mid = Rows(3, 2 * n, 6)
    env, audio, rs, out = Rows(3, n, 1), Rows(3, n, 3), Rows(3, n3, 1), Rows(3, n4)
    st = torch.zeros((3, 2), dtype=torch.float32, device="cuda")                # the Pipe's start, Filter.hs:730-739
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())                            # the buffers were filled on the default stream
    l0 = hip.am_demod_launches()
    with torch.cuda.stream(stream):
        bank.run(d_in.data_ptr(), 0, mid.view.data_ptr(), mid.stride, 0, n, B, stream.cuda_stream)
        hip.am_demod_rows(mid.view, out=env.view)
        hip.dc_blocker_rows(env.view, st, out=audio.view, final=st)
        res.run_rows(audio.view, rs.view, 0, n3)
        fil.run_rows(rs.view, out.view, 0, n4)
    stream.synchronize()
    assert hip.am_demod_launches() - l0 == 1
    g_mid, g_env, g_audio, g_rs, g_out = mid.read("the bank's rows"), env.read("am_demod_rows"), audio.read("dc_blocker_rows"), \
        rs.read("Resampler.run_rows"), out.read("Filter.run_rows")
    for j in range(3):
        assert_bit_equal(g_mid[j], exp[j], f"channel {j}: the bank's row")
        e_env = AC.expected(exp[j].view(np.complex64))
        assert np.isfinite(e_env).all() and e_env.max() > 0
        AC.assert_same(g_env[j], e_env, f"channel {j}: am_demod_rows behind the bank")
        e_audio, _, _ = oracle.dc_blocker(e_env, 0.0, 0.0)
        assert_bit_equal(g_audio[j], e_audio, f"channel {j}: dc_blocker_rows behind am_demod_rows")
        (e_rs,), _ = PM.fir_resampler_pipe(rm, [e_audio], n3)
        assert_bit_equal(g_rs[j], e_rs, f"channel {j}: Resampler.run_rows")
        (e_out,), _ = PM.fir_filter_pipe(fm, [e_rs], n4)
        assert_bit_equal(g_out[j], e_out, f"channel {j}: Filter.run_rows")
    assert not np.array_equal(g_out[0], g_out[1])


# ---- 4: the Pipe ----------------------------------------------------------------------------------------------------------------------
def _blocks(sizes, seed=11):
    z = AC.mixed(sum(sizes), seed=seed)
    e = AC.expected(z)
    cut = np.cumsum([0] + list(sizes))
    return [_floats(z[a:b]) for a, b in zip(cut[:-1], cut[1:])], [e[a:b] for a, b in zip(cut[:-1], cut[1:])]


def _cmp(got, exp, what):
    assert len(got) == len(exp), f"{what}: {len(got)} blocks vs {len(exp)}"
    for i, (g, e) in enumerate(zip(got, exp)):
        AC.assert_same(g, e, f"{what}, block {i}")


UNIFORM = [8192] * 12
RAGGED = [4096, 8192, 1, 1000, 20000, 777, 7, 8192, 129, 5000, 3, 8192]


@pytest.mark.parametrize("adaptive", [32, 2, 0], ids=["adaptive 32", "adaptive 2", "every push on its own"])
@pytest.mark.parametrize("sizes", [UNIFORM, RAGGED], ids=["uniform", "ragged"])
def test_pipe_uniform_and_ragged_pushes(hip, sizes, adaptive):
    """One output block per input block at the length it came in, whatever piles up into one run (adaptive) or goes out alone, with
    polls in between; nothing is carried, so any grouping gives the same blocks."""
    blocks, exp = _blocks(sizes)
    pipe = hip.Pipe.am_demod()
    assert pipe.rows == 1 and pipe.complex_in and not pipe.complex_out
    pipe.set_adaptive(adaptive)
    got = []
    for i, b in enumerate(blocks):
        got += pipe.push(b)
        if i % 5 == 4:
            got += pipe.poll()
    got += pipe.flush()
    _cmp(got, exp, f"amDemod Pipe, adaptive {adaptive}")
    assert pipe.flush() == [] and pipe.poll() == []


def test_pipe_answers_the_filter_pipes_calls_as_the_other_map_pipes_do(hip):
    """set_coalesce, input_buffer and pop_rows belong to the filter-like pipes: an amDemod pipe refuses them exactly as an fmDemod
    pipe does, stages nothing and goes on working; pop on an empty pipe is 0."""
    import ctypes as C
    blocks, exp = _blocks([100, 8192, 5])
    am, fm = hip.Pipe.am_demod(), hip.fmDemod()
    o = np.empty(64, np.float32)
    for p in (am, fm):
        with pytest.raises(hip.SdrHipError):
            p.set_coalesce(4)
        with pytest.raises(hip.SdrHipError):
            p.input_buffer(100)
        assert hip.lib.sdrhip_pipe_pop_rows(p.h, o.ctypes.data_as(C.POINTER(C.c_float)), 64, 1) == -1
        assert hip.lib.sdrhip_pipe_pop(p.h, o.ctypes.data_as(C.POINTER(C.c_float)), 64) == 0
        with pytest.raises(hip.SdrHipError):
            p.set_adaptive(1)
    got = []
    for b in blocks:
        got += am.push(b)
    _cmp(got + am.flush(), exp, "amDemod Pipe after the refused calls")


def test_pipe_both_sides_of_the_direct_bound(hip):
    """512 KiB of staged input (65536 complex samples) is read and written in place over PCIe, one sample more goes through the copy
    engines: the same blocks.  Blocks of 65535 / 65536 / 65537 samples, each alone in its run, then two that pile up past the bound."""
    sizes = [65535, 65536, 65537, 40000, 40000]
    blocks, exp = _blocks(sizes, seed=13)
    pipe = hip.Pipe.am_demod()
    pipe.set_adaptive(0)
    l0 = hip.am_demod_launches()
    got = []
    for b in blocks:
        got += pipe.push(b)
    got += pipe.flush()
    assert hip.am_demod_launches() - l0 == len(sizes)        # adaptive off: every push is one run, one launch
    _cmp(got, exp, "amDemod Pipe across the direct bound")
    pipe = hip.Pipe.am_demod()
    got = []
    for b in blocks:
        got += pipe.push(b)
    _cmp(got + pipe.flush(), exp, "amDemod Pipe across the direct bound, adaptive")


def test_pipe_save_after_5_of_40_pushes_and_restore(hip):
    sizes = [int(s) for s in np.random.default_rng(5).choice([1, 7, 100, 1024, 4096, 8192], 40)]
    blocks, exp = _blocks(sizes, seed=17)
    first = hip.Pipe.am_demod()
    got = []
    for b in blocks[:5]:
        got += first.push(b)
    state = first.save()
    import struct
    magic, version, kind, _, _, _, _, cplx_in, cplx_out, _, _, n_blocks, _, _, head_cap, hist_n, pending = struct.unpack_from("<II10i5q", state)
    assert (magic, version, kind, cplx_in, cplx_out) == (0x50504453, 1, 8, 1, 0)           # the ninth PipeKind: older numbers keep their meaning
    assert hist_n == 0 and head_cap == 0, "nothing is carried from block to block"
    assert n_blocks == 5 - len(got) and pending == sum(sizes[len(got):5])
    assert len(state) == struct.calcsize("<II10i5q6f") + 4 * pending + 4 * n_blocks       # only the output not yet popped
    del first
    second = hip.Pipe.am_demod()
    got += second.restore(state, max_block=max(sizes))
    for b in blocks[5:]:
        got += second.push(b)
    got += second.flush()
    _cmp(got, exp, "amDemod Pipe saved after 5 of 40 pushes")

    # refused, the pipe unchanged: an fmDemod pipe's state and truncated states
    fm = hip.fmDemod()
    fm.push(blocks[0])
    fm_state = fm.save()
    assert struct.unpack_from("<II10i", fm_state)[2] == 3
    fresh = hip.Pipe.am_demod()
    for bad, what in ((fm_state, "an fmDemod pipe's state"), (state[:-4], "a state four bytes short"), (state[:60], "half a header")):
        with pytest.raises(hip.SdrHipError):
            fresh.restore(bad)
    with pytest.raises(hip.SdrHipError):
        hip.fmDemod().restore(state)                          # and the other way round
    assert fresh.flush() == []
    _cmp(fresh.restore(state, max_block=max(sizes)), exp[5 - n_blocks: 5], "restore after the refusals")
    _cmp(fresh.push(blocks[5]) + fresh.flush(), exp[5:6], "the restored pipe goes on")


def test_pipe_pop_and_the_block_lengths(hip):
    """sdrhip_pipe_pop hands the blocks back one by one at the lengths they came in; a capacity below the block's length is refused
    and the block stays."""
    import ctypes as C
    blocks, exp = _blocks([300, 5, 1024], seed=19)
    pipe = hip.Pipe.am_demod()
    for b in blocks:
        hip.check(hip.lib.sdrhip_pipe_push(pipe.h, b.ctypes.data_as(C.POINTER(C.c_float)), b.size // 2))
    assert hip.check(hip.lib.sdrhip_pipe_flush(pipe.h)) == 3
    o = np.full(2048, np.nan, np.float32)
    fp = o.ctypes.data_as(C.POINTER(C.c_float))
    assert hip.lib.sdrhip_pipe_pop(pipe.h, fp, 299) == -1 and np.isnan(o).all()
    for e in exp:
        assert hip.lib.sdrhip_pipe_pop(pipe.h, fp, 2048) == e.size
        AC.assert_same(o[:e.size], e, "sdrhip_pipe_pop")
    assert hip.lib.sdrhip_pipe_pop(pipe.h, fp, 2048) == 0


# ---- 5: the example -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("no_dc", [False, True], ids=["with dcBlockingFilter", "--no-dc"])
def test_am_replay_example(hip, tmp_path, no_dc):
    """examples/am_replay on a seeded u8 capture equals the same three Pipes driven from the binding."""
    exe = os.path.join(ROOT, "examples", "bin", "am_replay")
    if not os.path.exists(exe):
        from sdr_amd import build as Bd
        Bd.build_examples()
    assert os.path.exists(exe)
    B = 8192
    n = 6 * B + 1234                                     # six whole pushes and a ragged rest
    u = S.iq_u8(n, seed=77)
    cap, tp, outp = tmp_path / "capture.u8", tmp_path / "taps.f32", tmp_path / "out.f32"
    u.tofile(cap)
    S.taps_decim127().tofile(tp)
    r = subprocess.run([exe, str(cap), str(tp), str(outp), "--channel", "-3/1000", "--block-out", "500"] + (["--no-dc"] if no_dc else []),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    tuner = hip.Pipe.tuner_bank(hip.TunerBank(8, S.taps_decim127(), [hip.tuner_shift_table(-3, 1000)]), 500, input_u8=True)
    am, dc = hip.Pipe.am_demod(), hip.dcBlockingFilter()
    audio = []

    def through_am(iq_blocks):
        for blk in iq_blocks:
            through_dc(am.push(blk[0]))

    def through_dc(env_blocks):
        for e in env_blocks:
            if no_dc:
                audio.append(e)
            else:
                audio.extend(dc.push(e))

    u = u.reshape(-1)
    for a in list(range(0, 2 * 6 * B, 2 * B)) + [2 * 6 * B]:
        through_am(tuner.push(u[a: a + 2 * B]))
    through_am(tuner.flush())
    through_dc(am.flush())
    if not no_dc:
        audio.extend(dc.flush())
    want = np.concatenate(audio)
    assert want.size == ((n - 128) // 8 + 1) // 500 * 500 and np.isfinite(want).all()
    got = np.fromfile(outp, np.float32)
    assert_bit_equal(got, want, "am_replay against the three Pipes driven from the binding")
    if no_dc:
        assert got.min() >= 0 and got.max() > 0              # an envelope
