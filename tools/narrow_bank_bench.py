"""The narrow-channel bank's fused route against its composed route of the same build, alternating the two in one process.

    python tools/narrow_bank_bench.py [--rounds R] [--window S] [--out profiles/narrow_bank_bench.txt]

Sweep: K = 1, 2, 8, 32 channels x resident launches of 8192, 2^17, 2^20 and 2^24 input samples (stage 1: the 128-tap / 8 shape), u8,
cfloat and int16 input, the envelope form without and with dcBlocker and the fmDemod form, second decimators 24 taps / 4 and 61 taps
/ 5 (tests/narrow_bank_cases.py), (seam_block, seam_block2) = (0, 0) and (8192, 1024).
  fused     one sdrhip_narrow_bank_run* on route 1: the tuner bank, then ONE launch of k_narrow_rows for all K channels [and dcBlocker's
            rows launch set]
  composed  the same call on route 2: sdrhip_tuner_bank_run*, sdrhip_decimator_run_rows (its auto route), sdrhip_am_demod_run_rows or
            sdrhip_fm_demod_run_rows [, sdrhip_dc_blocker_run_rows] -- what a caller does without the bank, so it is the baseline
Every figure is a host clock around `reps` back-to-back runs that end in ONE device synchronise, after warm-up runs of the same
shape; reps are chosen so that a window lasts about `--window` seconds.  The legs alternate within each round, the two fm state arrays
are swapped from run to run, the dc state is reused; the table gives the median and the spread over the rounds.  Before it is timed,
a point's two legs are compared bit for bit, the final states included.
No number is fixed in advance.  The last lines give, per form, second decimator and seam pair, the points where the fused route is
ahead by the project's criterion -- its SLOWEST round below the composed route's FASTEST -- for ALL THREE input types, as the table
narrow_bank.cpp's auto rule is read from.  A missing GPU is an error."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
import sdr_amd.lib as L
import narrow_bank_cases as NB
import signals as S

CHANNELS = (1, 2, 8, 32)
SIZES = (("8192", 8192), ("2^17", 1 << 17), ("2^20", 1 << 20), ("2^24", 1 << 24))
KINDS = ("u8", "cf32", "i16")
FORMS = (("env", L.NARROW_ENV, False), ("env+dc", L.NARROW_ENV, True), ("fm", L.NARROW_FM, False))
SHAPES = ("24/4", "61/5")
SEAMS = ((0, 0), (8192, 1024))


def tables(K):
    """K channels on a raster of 1/64 of the sampling frequency around the centre (the centre itself: the table {1, 0})"""
    return [L.tuner_shift_table((j - K // 2) % 64, 64) if j != K // 2 else [1.0, 0.0] for j in range(K)]


def counts(n_samples, shape):
    _, d2, lp2 = NB.SHAPES[shape]
    return ((n_samples - 128) // 8 + 1 - lp2) // d2 + 1


def legs(K, n_samples, kind, form, dc, shape, seams):
    taps2, d2, _ = NB.SHAPES[shape]
    tb = L.TunerBank(8, S.taps_decim127(), tables(K))
    dec = L.Decimator(d2, taps2, complex_=True)
    banks = {"fused": L.NarrowBank(tb, dec, form, dc), "composed": L.NarrowBank(tb, dec, form, dc)}
    banks["fused"].set_route(L.NarrowBank.ROUTE_FUSED)
    banks["composed"].set_route(L.NarrowBank.ROUTE_COMPOSED)
    n = counts(n_samples, shape)
    if kind == "u8":
        d_in = torch.randint(0, 256, (2 * n_samples,), dtype=torch.uint8, device="cuda")
    elif kind == "i16":
        d_in = torch.randint(-2048, 2048, (2 * n_samples,), dtype=torch.int16, device="cuda")
    else:
        d_in = torch.rand(2 * n_samples, dtype=torch.float32, device="cuda") * 2.0 - 1.0
    out = torch.empty(K * n, dtype=torch.float32, device="cuda")
    states = [torch.zeros(2 * K, dtype=torch.float32, device="cuda") for _ in range(2)]
    dcs = torch.zeros(2 * K, dtype=torch.float32, device="cuda")
    wsb = banks["composed"].workspace_bytes(n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    pi, po, pw = d_in.data_ptr(), out.data_ptr(), ws.data_ptr()
    ps = [s.data_ptr() for s in states]
    pdc = dcs.data_ptr() if dc else None
    fm = form == L.NARROW_FM

    def leg(bank):
        run = {"u8": bank.run_u8, "i16": bank.run_i16, "cf32": bank.run}[kind]

        def fn(reps):
            for r in range(reps):
                run(pi, 0, po, n, 0, n, seams[0], seams[1], ps[r & 1] if fm else None, ps[(r + 1) & 1] if fm else None, pdc, pw, wsb)
            torch.cuda.synchronize()
        return fn

    fns = {name: leg(b) for name, b in banks.items()}
    got = {}
    for name, fn in fns.items():
        out.zero_()
        dcs.zero_()
        for s in states:
            s.zero_()
        fn(1)
        got[name] = (out.clone(), states[1].clone(), dcs.clone())
    for a, b in zip(got["fused"], got["composed"]):
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            sys.exit(f"narrow_bank_bench: the two routes differ at K = {K}, {n_samples} samples, {kind}, form {form}, dc {dc}, {shape}, seams {seams}")
    del got
    return fns, n, (tb, dec, banks, d_in, out, states, dcs, ws)


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("narrow_bank_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("narrow_bank_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, windows of about {a.window} s, fused route (1) and composed route (2) alternating; "
             "us per run of ALL K channels: median (min .. max)"]
    print(lines[0], flush=True)
    points = {}
    for fname, form, dc in FORMS:
        for shape in SHAPES:
            for seams in SEAMS:
                for kind in KINDS:
                    for si, (size_name, n_samples) in enumerate(SIZES):
                        for ki, K in enumerate(CHANNELS):
                            fns, n, keep = legs(K, n_samples, kind, form, dc, shape, seams)
                            reps = {}
                            for name, fn in fns.items():
                                fn(5)                                # warm-up of this shape: code objects, table uploads
                                per = timed(fn, 10) * 1e-6
                                reps[name] = max(5, min(20000, int(a.window / per)))
                            f0 = L.narrow_bank_launches()
                            times = {k: [] for k in fns}
                            for _ in range(a.rounds):
                                for name, fn in fns.items():
                                    times[name].append(timed(fn, reps[name]))
                            assert L.narrow_bank_launches() - f0 == a.rounds * reps["fused"], "a leg took another route than the one it is named for"
                            med = {k: statistics.median(v) for k, v in times.items()}
                            fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                            clear = max(times["fused"]) < min(times["composed"])
                            line = (f"{fname:6s} {shape:5s} seams {seams[0]:4d},{seams[1]:4d} {kind:4s} {size_name:5s} K {K:2d}  outputs {n:7d} x {K:2d}   "
                                    f"fused {fmt(times['fused'])}   composed {fmt(times['composed'])}   fused / composed {med['fused'] / med['composed']:.3f}"
                                    f"{'' if clear else '   (not ahead by the criterion)'}")
                            print(line, flush=True)
                            lines.append(line)
                            points[(fname, shape, seams, kind, si, ki)] = (clear, med["fused"] / med["composed"])
                            del fns, keep
                            torch.cuda.empty_cache()
    tail = ["# fused ahead (slowest fused round below the composed route's fastest) for ALL THREE input types; rows K = 1 / 2 / 8 / 32, columns "
            "8192 / 2^17 / 2^20 / 2^24 input samples; 1 = ahead; (min .. max of the three types' median ratios)"]
    for fname, form, dc in FORMS:
        for shape in SHAPES:
            for seams in SEAMS:
                tail.append(f"# {fname} {shape} seams {seams[0]},{seams[1]}:")
                for ki, K in enumerate(CHANNELS):
                    cells = []
                    for si in range(len(SIZES)):
                        ps = [points[(fname, shape, seams, kind, si, ki)] for kind in KINDS]
                        cells.append(f"{int(all(p[0] for p in ps))} ({min(p[1] for p in ps):.2f} .. {max(p[1] for p in ps):.2f})")
                    tail.append(f"#   K {K:2d}:  " + "   ".join(cells))
    print("\n".join(tail), flush=True)
    lines += tail
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
