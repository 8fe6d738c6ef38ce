"""examples/squelch_scan.c against the same two calls driven from the binding (NarrowBank.run_u8, then squelch_run_rows in place, each
row its own detector): file bytes against arrays, and the gates against tests/squelch_model.py on the binding's ungated rows.

The capture is seeded noise with a carrier at one channel's frequency that is keyed on and off, so that the channel tuned to it opens
and shuts in either form; the thresholds are read off the ungated rows' own block levels (the model's), between the quiet and the loud
blocks, and handed to the program with nine significant digits, which a float32 survives."""
import os
import subprocess

import numpy as np
import pytest

import narrow_bank_cases as NB
import signals as S
import squelch_model as SM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FM, ENV = 1, 0
N, BLOCK, HANG = 40 * 1024, 32, 1
CHANNELS = [(1, 64), (-1, 64)]


def capture():
    rng = np.random.default_rng(4242)
    n = np.arange(N)
    keyed = ((n // 6000) % 2 == 1).astype(np.float64)                 # the carrier is on in every second stretch of 6000 samples
    ph = 2 * np.pi * n / 64.0
    i = 127.5 + 50 * keyed * np.cos(ph) + rng.normal(0, 6, N)
    q = 127.5 + 50 * keyed * np.sin(ph) + rng.normal(0, 6, N)
    return np.clip(np.round(np.stack([i, q], 1)), 0, 255).astype(np.uint8).reshape(-1)


@pytest.mark.parametrize("form", [FM, ENV], ids=["fm", "env"])
def test_squelch_scan_against_the_binding(hip, form, tmp_path):
    import torch
    from sdr_amd import build as Bld
    Bld.build_examples()                                              # (a no-op where build() has made it already)
    exe = os.path.join(ROOT, "examples", "bin", "squelch_scan")
    assert os.path.exists(exe)
    cap = capture()
    taps2, d2, lp2 = NB.SHAPES["61/5"]
    tables = [hip.tuner_shift_table(a, b) for a, b in CHANNELS]
    bank = hip.NarrowBank(hip.TunerBank(8, S.taps_decim127(), tables), hip.Decimator(d2, taps2, complex_=True), form, False)
    j_all = (N - bank.tuner_bank.num_coeffs) // 8 + 1
    k_all = (j_all - lp2) // d2 + 1
    nb = k_all // BLOCK
    count = nb * BLOCK
    assert nb >= 20
    rows = torch.empty((len(CHANNELS), count), dtype=torch.float32, device="cuda")
    wsb = bank.workspace_bytes(count)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    bank.run_u8(torch.from_numpy(cap).cuda().data_ptr(), 0, rows.data_ptr(), count, 0, count, workspace=ws.data_ptr(), workspace_bytes=wsb)
    torch.cuda.synchronize()
    ungated = rows.cpu().numpy().copy()
    lv = SM.levels(ungated, False, BLOCK)
    lo, hi = np.percentile(lv, 10), np.percentile(lv, 90)
    assert hi > 4 * lo > 0, f"the keyed carrier does not show in the block levels: 10th and 90th percentile {lo}, {hi}"
    mid = np.float32(np.sqrt(lo * hi))
    open_level, close_level = (np.float32(mid * 0.8), np.float32(mid * 1.25)) if form == FM else (np.float32(mid * 1.25), np.float32(mid * 0.8))
    want_out, _, _, want_gates = SM.squelch(ungated, False, BLOCK, ungated, BLOCK, open_level, close_level, HANG, 0 if form == FM else 1)
    assert 0.1 < want_gates.mean() < 0.9 and any(0 < g.mean() < 1 for g in want_gates), "the gate should open and shut"

    out, _, _, gates = hip.squelch_run_rows(rows, BLOCK, rows, BLOCK, float(open_level), float(close_level), HANG, form != FM, out=rows, gates=True)
    torch.cuda.synchronize()
    assert SM.same_bits(out.cpu().numpy(), want_out).all() and np.array_equal(gates.cpu().numpy(), want_gates)

    capf, tp, tp2 = tmp_path / "capture.u8", tmp_path / "taps.f32", tmp_path / "taps2.f32"
    cap.tofile(capf)
    S.taps_decim127().tofile(tp)
    taps2.tofile(tp2)
    args = [exe, str(capf), str(tp), str(tmp_path / "out"), "--channels", ",".join(f"{a}/{b}" for a, b in CHANNELS), "--narrow", str(tp2), str(d2),
            "--form", "fm" if form == FM else "env", "--squelch", f"{open_level:.9g},{close_level:.9g},{HANG}", "--block", str(BLOCK)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    for j in range(len(CHANNELS)):
        got = np.fromfile(str(tmp_path / f"out.{j}.f32"), np.float32)
        g = np.fromfile(str(tmp_path / f"out.{j}.gate"), np.uint8)
        assert got.size == count and g.size == nb
        assert np.array_equal(got.view(np.uint32), out[j].cpu().numpy().view(np.uint32)), f"channel {j}: samples"
        assert np.array_equal(g, gates[j].cpu().numpy()), f"channel {j}: gates"
    # the options come together or not at all
    for bad in (args[:-2], args[:4], args[:-2] + ["--block", "0"], [a if a not in ("fm", "env") else "ssb" for a in args]):
        r = subprocess.run(bad, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "usage" in r.stderr, (bad, r.returncode, r.stderr)
