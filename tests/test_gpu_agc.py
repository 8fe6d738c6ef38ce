"""agc / agcPipe on the device (kernels_agc.hip: speculative chunks, repair rounds, settling walk) against the numpy model
(tests/agc_model.py), bit for bit: every route, the settling path, a non-contracting mu, unaligned buffers, the argument
checks, the Pipe with save / restore, and the save bytes of an existing Pipe kind."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

import agc_model
import gpu_util
from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

N_MAX = 1 << 17
SIZES = [1, 2, 7, 8192, 24_576, 100_001, 131_072]
NAMES = ["noise", "fm", "tone", "u8fm", "zeros", "wide-down"]
ERR_ARG = -1


def _fm_phase(n):
    t = np.arange(n, dtype=np.float64)
    return np.cumsum(2 * np.pi * (0.02 + 0.05 * np.sin(2 * np.pi * t / 480.0)))


def _u8fm(n):
    ph = _fm_phase(n)
    q = np.clip(np.rint(128.0 + 100.0 * np.stack([np.cos(ph), np.sin(ph)], axis=1)), 0, 255)
    v = ((q - 128.0) / 128.0).astype(np.float32)
    return (v[:, 0] + 1j * v[:, 1]).astype(np.complex64)


def _fm(n, rng):
    return (0.5 * np.exp(1j * _fm_phase(n)) + 0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def _signals(n, seed=4711):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    noise = 0.3 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    fm = _fm(n, rng)
    tone = 0.5 * np.exp(2j * np.pi * 0.01234 * t)
    wide = np.clip(rng.standard_normal((2, n)) * np.exp(rng.uniform(-60, 0, (2, n))), -1.0, 1.0)
    sig = {"noise": noise, "fm": fm, "tone": tone, "u8fm": _u8fm(n), "zeros": np.zeros(n), "wide-down": wide[0] + 1j * wide[1]}
    return {k: np.ascontiguousarray(v, dtype=np.complex64) for k, v in sig.items()}


@pytest.fixture(scope="module")
def signals():
    return _signals(N_MAX)


@pytest.fixture(scope="module")
def model(signals):
    """(mu, reference, state) -> (outputs (6, N_MAX) complex64, {n: states after n samples}); one model run per parameter set,
    every shorter length is a prefix of it."""
    cache = {}
    batch = np.stack([signals[k] for k in NAMES])

    def get(mu, reference, state):
        key = (mu, reference, state)
        if key not in cache:
            out, _, snaps = agc_model.agc(batch, mu, reference, state, states_at=SIZES)
            out.setflags(write=False)
            cache[key] = (out, snaps)
        return cache[key]
    return get


def _run(hip, x, mu, reference, state, run_in=0, use_ws=True, offset=0):
    """x complex64 (n,).  offset: floats by which input and output are shifted off their 256-byte aligned buffers.
    Returns (out complex64, final state float32 (1,), the four statistics words)."""
    n = x.size
    d_in_whole = torch.zeros(2 * n + 8, dtype=torch.float32, device="cuda")
    d_in = d_in_whole[offset: offset + 2 * n]
    d_in.copy_(torch.from_numpy(x.view(np.float32)))
    whole = gpu_util.dev_empty_f32(2 * n + 8)
    d_out = whole[offset: offset + 2 * n]
    fin = gpu_util.dev_empty_f32(1)
    wsb = hip.lib.sdrhip_agc_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    hip.check(hip.lib.sdrhip_agc_run(None, d_in.data_ptr(), d_out.data_ptr(), n, mu, reference, state, fin.data_ptr(),
                                     ws.data_ptr() if use_ws else None, wsb if use_ws else 0, run_in), "sdrhip_agc_run")
    torch.cuda.synchronize()
    w = gpu_util.to_host(whole).view(np.uint32)
    assert np.all(w[:offset] == gpu_util.CANARY) and np.all(w[offset + 2 * n:] == gpu_util.CANARY), "wrote outside its output"
    stats = tuple(int(v) for v in ws[:16].cpu().numpy().view(np.uint32))
    return w[offset: offset + 2 * n].view(np.complex64).copy(), gpu_util.to_host(fin), stats


def _same(got, exp, what):
    assert_bit_equal(np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(exp).view(np.float32), what)


@pytest.mark.parametrize("params", [(0.1, 1.0, 1.0), (0.01, 0.5, 3.0)])
@pytest.mark.parametrize("n", SIZES)
def test_device_matches_model(hip, signals, model, n, params):
    mu, reference, state = params
    exp, snaps = model(*params)
    for k, name in enumerate(NAMES):
        got, fin, stats = _run(hip, signals[name][:n], mu, reference, state)
        _same(got, exp[k, :n], f"agc {name} n={n} mu={mu}")
        assert_bit_equal(fin, snaps[n][k: k + 1], f"agc final state {name} n={n} mu={mu}")
        if mu == 0.1 and n >= 24_576:
            assert stats[3] >= 8, f"{name} n={n}: the default plan should speculate on at least 8 chunks, took {stats[3]}"
            assert stats[3] == hip.agc_plan(n, mu)[0]


def test_settling_does_not_change_the_result(hip, signals, model):
    """A run-in far too short leaves most chunks to the repair rounds and the walk; an ample one leaves nothing."""
    n = N_MAX
    exp, snaps = model(0.1, 1.0, 1.0)
    for k, name in enumerate(NAMES):
        got, fin, stats = _run(hip, signals[name], 0.1, 1.0, 1.0, run_in=16)
        print(f"run_in=16 {name}: stats {stats}")
        _same(got, exp[k], f"agc settle {name}")
        assert_bit_equal(fin, snaps[n][k: k + 1], f"agc settle final state {name}")
        if name in ("noise", "fm"):
            assert stats[2] > 0, "the short run-in should have left work for the repair rounds"
    for name in ("noise", "fm", "tone", "u8fm"):
        _, _, stats = _run(hip, signals[name], 0.1, 1.0, 1.0, run_in=2048)
        print(f"run_in=2048 {name}: stats {stats}")
        assert stats[:3] == (0, 0, 0) and stats[3] > 0, (name, stats)


def _bounded_for_mu3(x, mu, reference, state):
    """Samples of x shrunk (halved until it fits) wherever the model's next state would fall below -0.2.  A negative state
    grows by (1 + mu |x|) per sample and runs off to -inf unless mu * reference brings it back, which it does from -0.2 for any
    |x| < 4.6; with x = 0 the next state is state + mu * reference, so halving always ends."""
    mu, reference, s = np.float32(mu), np.float32(reference), np.float32(state)
    y = x.copy()
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for i in range(y.size):
            v = y[i]
            while True:
                re, im = np.float32(v.real) * s, np.float32(v.imag) * s
                nxt = s + mu * (reference - agc_model.magnitude(re, im))
                if nxt >= -0.2:
                    break
                v = np.complex64(v * np.float32(0.5))
            y[i], s = v, np.float32(nxt)
    return y


def test_non_contracting_mu(hip, signals):
    """mu * |x| is often > 2: speculative starts need not merge at all, the result is the model's all the same."""
    x = _bounded_for_mu3((signals["noise"][:40_000] / np.float32(0.3)).astype(np.complex64), 3.0, 1.0, 0.1)
    frac = np.mean(3.0 * np.abs(x) > 2.0)
    print(f"mu * |x| > 2 on {frac:.3f} of the samples")
    assert frac > 0.25, frac
    exp, fin_m, snaps = agc_model.agc(x, 3.0, 1.0, 0.1, states_at=[4096, 40_000])
    assert np.all(np.isfinite(exp.view(np.float32))) and np.isfinite(fin_m), "the model's trajectory must stay finite"
    for n in (4096, 40_000):
        got, fin, stats = _run(hip, x[:n], 3.0, 1.0, 0.1, run_in=256)
        print(f"mu=3 n={n}: stats {stats}")
        assert stats[3] > 0
        _same(got, exp[:n], f"agc mu=3 n={n}")
        assert_bit_equal(fin, np.array([snaps[n]], np.float32), f"agc mu=3 final state n={n}")


def test_alignment_and_sequential_route(hip, signals, model):
    n = 100_001
    exp, snaps = model(0.1, 1.0, 1.0)
    k = NAMES.index("fm")
    x = signals["fm"][:n]
    aligned, fin, stats = _run(hip, x, 0.1, 1.0, 1.0)
    assert stats[3] > 0
    _same(aligned, exp[k, :n], "aligned")
    for offset, what in ((2, "8-byte aligned only"), (1, "4-byte aligned only")):
        got, f, st = _run(hip, x, 0.1, 1.0, 1.0, offset=offset)
        assert st[3] > 0
        _same(got, aligned, what)
        assert_bit_equal(f, fin, what + ": final state")
        got, f, _ = _run(hip, x[:8191], 0.1, 1.0, 1.0, use_ws=False, offset=offset)     # the same widths on the one-lane route
        _same(got, aligned[:8191], what + ", sequential")
    got, f, _ = _run(hip, x, 0.1, 1.0, 1.0, use_ws=False)
    _same(got, aligned, "null workspace: the sequential route")
    assert_bit_equal(f, fin, "sequential final state")


def test_full_size_default_route(hip):
    """2^22 samples in one call: default route == sequential route == the model on the first 65 536 samples; the default
    run-in at mu = 0.01 covers this signal's merge distance (CPU-measured worst: 2 433 samples)."""
    n = 1 << 22
    x = _u8fm(n)
    got, fin, stats = _run(hip, x, 0.01, 1.0, 1.0)
    print(f"2^22 u8fm mu=0.01: stats {stats}, plan {hip.agc_plan(n, 0.01)}")
    seq, fin_s, _ = _run(hip, x, 0.01, 1.0, 1.0, use_ws=False)
    _same(got, seq, "2^22: default route vs sequential")
    assert_bit_equal(fin, fin_s, "2^22 final state")
    exp, _ = agc_model.agc(x[:65_536], 0.01, 1.0, 1.0)
    _same(got[:65_536], exp, "2^22: first 65 536 samples vs the model")
    assert stats[3] >= 8 and stats[0] == 0, stats


def test_argument_errors(hip):
    n = 4096
    d_in = torch.zeros(2 * n, dtype=torch.float32, device="cuda")
    d_out = gpu_util.dev_empty_f32(2 * n)
    fin = gpu_util.dev_empty_f32(1)
    wsb = hip.lib.sdrhip_agc_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")
    run = hip.lib.sdrhip_agc_run
    bad = {
        "in-place": (None, d_in.data_ptr(), d_in.data_ptr(), n, 0.1, 1.0, 1.0, fin.data_ptr(), ws.data_ptr(), wsb, 0),
        "null output": (None, d_in.data_ptr(), None, n, 0.1, 1.0, 1.0, fin.data_ptr(), ws.data_ptr(), wsb, 0),
        "null input": (None, None, d_out.data_ptr(), n, 0.1, 1.0, 1.0, fin.data_ptr(), ws.data_ptr(), wsb, 0),
        "null final": (None, d_in.data_ptr(), d_out.data_ptr(), n, 0.1, 1.0, 1.0, None, ws.data_ptr(), wsb, 0),
        "short workspace": (None, d_in.data_ptr(), d_out.data_ptr(), n, 0.1, 1.0, 1.0, fin.data_ptr(), ws.data_ptr(), wsb - 1, 0),
        "negative run_in": (None, d_in.data_ptr(), d_out.data_ptr(), n, 0.1, 1.0, 1.0, fin.data_ptr(), ws.data_ptr(), wsb, -1),
    }
    for what, args in bad.items():
        assert run(*args) == ERR_ARG, what
        assert b"sdrhip_agc_run" in hip.lib.sdrhip_last_error(), what
    hip.check(run(None, None, None, 0, 0.1, 1.0, 2.5, fin.data_ptr(), None, 0, 0), "n = 0")
    assert_bit_equal(gpu_util.to_host(fin), np.array([2.5], np.float32), "n = 0 hands the state on")
    torch.cuda.synchronize()
    assert np.all(gpu_util.to_host(d_out).view(np.uint32) == gpu_util.CANARY), "a refused call must not write"


def test_binding_on_tensors_and_arrays(hip, signals, model):
    exp, snaps = model(0.1, 1.0, 1.0)
    k, n = NAMES.index("noise"), 8192
    x = signals["noise"][:n]
    out, fin = hip.agc(x, 0.1, 1.0)
    _same(out, exp[k, :n], "agc on a host array")
    assert np.float32(fin).tobytes() == snaps[n][k].tobytes()
    out_t, fin_t = hip.agc(torch.from_numpy(x).cuda(), 0.1, 1.0, state=1.0)
    _same(out_t.cpu().numpy(), exp[k, :n], "agc on a device tensor")
    assert np.float32(fin_t).tobytes() == snaps[n][k].tobytes()


def test_pipe_agc_with_save_and_restore(hip):
    n = 200_000
    x = _fm(n, np.random.default_rng(9))
    exp, _ = agc_model.agc(x, 0.01, 1.0, 1.0)
    cuts = [0, 8192, 16384, 16391, 50_000, 120_000, 200_000]        # short, ragged and long blocks (the long ones speculate)
    blocks = [agc_model.interleaved(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    pipe = hip.agcPipe(0.01, 1.0)
    outs = []
    for b in blocks:
        outs += pipe.push(b)
    outs += pipe.flush()
    assert [o.size for o in outs] == [b.size for b in blocks]
    _same(np.concatenate(outs), exp, "agcPipe")

    first = hip.Pipe("agc", mu=0.01, reference=1.0)
    got = []
    for b in blocks[:3]:
        got += first.push(b)
    state = first.save()
    magic, version, kind = struct.unpack_from("<IIi", state)
    assert (magic, version, kind) == (0x50504453, 1, 5)
    del first
    second = hip.agcPipe(0.01, 1.0)
    got += second.restore(state, max_block=max(b.size // 2 for b in blocks))
    for b in blocks[3:]:
        got += second.push(b)
    got += second.flush()
    assert [o.size for o in got] == [b.size for b in blocks]
    _same(np.concatenate(got), exp, "agcPipe, saved after three blocks")


def test_save_bytes_of_a_dc_blocker_pipe_unchanged(hip):
    """The header of a Pipe state keeps its layout and version: 112 bytes, then the history, the output not yet popped and the
    block lengths (sdrhip_pipe_state_bytes in pipes_state.cpp)."""
    rng = np.random.default_rng(1)
    x = rng.uniform(-1, 1, 1777).astype(np.float32)
    pipe = hip.dcBlockingFilter()
    popped = sum(o.size for o in pipe.push(x[:1000])) + sum(o.size for o in pipe.push(x[1000:]))
    hip.lib.sdrhip_pipe_state_bytes.restype = C.c_size_t
    hip.lib.sdrhip_pipe_state_bytes.argtypes = [C.c_void_p]
    need = hip.lib.sdrhip_pipe_state_bytes(pipe.h)
    state = pipe.save()
    header = "<II10i5q6f"
    assert struct.calcsize(header) == 112
    f = struct.unpack_from(header, state)
    magic, version, kind, n_blocks = f[0], f[1], f[2], f[11]
    e_prev, m_done, head_cap, hist_n, pending = f[12:17]
    assert (magic, version, kind) == (0x50504453, 1, 4)
    assert head_cap == 0 and hist_n == 0 and pending == 1777 - popped
    assert len(state) == need == 112 + 4 * hist_n + 4 * pending + 4 * n_blocks
    assert f[19] == x[-1], "dc[0] is the last input sample"
    assert f[21] == 0.0 and f[22] == 0.0
