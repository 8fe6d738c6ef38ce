"""The narrow-band FM bank's fused route against its composed route of the same build, alternating the two in one process.

    python tools/nfm_bank_bench.py [--rounds R] [--out profiles/nfm_bank_bench.txt]

Sweep: K = 1, 2, 8, 32 channels x resident launches of 8192, 2^17, 2^20 and 2^24 input samples of the 128-tap shape (contiguous
stream), u8, cfloat and int16 input, factors 8 and 16, seam_block 0 and 8192.
  fused     one sdrhip_nfm_bank_run* on route 1: ONE fmDemod-form launch of the tuner bank's tile kernel for all K channels
  composed  the same call on route 2: sdrhip_tuner_bank_run* (the tuner bank on its default route) and sdrhip_fm_demod_run_rows -- what
            a caller does without the bank, so it is the baseline
  env       a reference point, no leg of the comparison: sdrhip_am_bank_run* without dc_block on ITS route 1 -- the envelope form of the
            same tile launch, whose tiles do not overlap and which takes a fix-up launch where the fmDemod form computes Cross outputs
            in the tile -- at the same shape, in the same rounds
Every figure is a host clock around `reps` back-to-back runs that end in ONE device synchronise, after warm-up runs of the same
shape; reps are chosen so that a window lasts about 0.05 s.  The legs alternate within each round, the two state arrays are swapped
from run to run; the table gives the median and the spread over the rounds.  Before it is timed, a point's two legs are compared
bit for bit, d_final included.
No number is fixed in advance.  The last lines list, per input type, factor and seam, the points where the fused route is ahead by the
project's criterion -- its SLOWEST round below the composed route's FASTEST -- and those where it is not: the auto rule of
sdrhip_nfm_bank_run is read from them.  A missing GPU is an error."""
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
import signals as S

CHANNELS = (1, 2, 8, 32)
SIZES = (("8192", 8192), ("2^17", 1 << 17), ("2^20", 1 << 20), ("2^24", 1 << 24))
KINDS = ("u8", "cf32", "i16")
FACTORS = (8, 16)
SEAMS = (0, 8192)
WINDOW_S = 0.05


def tables(K):
    """K channels on a raster of 1/64 of the sampling frequency around the centre (the centre itself: the table {1, 0})"""
    return [L.tuner_shift_table((j - K // 2) % 64, 64) if j != K // 2 else [1.0, 0.0] for j in range(K)]


def legs(K, n_samples, kind, factor, seam):
    taps = S.taps_decim127()
    tb = L.TunerBank(factor, taps, tables(K))
    banks = {"fused": L.NfmBank(tb), "composed": L.NfmBank(tb)}
    banks["fused"].set_route(L.NfmBank.ROUTE_FUSED)
    banks["composed"].set_route(L.NfmBank.ROUTE_COMPOSED)
    env = L.AmBank(tb, dc_block=False)
    env.set_route(L.AmBank.ROUTE_FUSED)
    n = (n_samples - 128) // factor + 1
    if kind == "u8":
        d_in = torch.randint(0, 256, (2 * n_samples,), dtype=torch.uint8, device="cuda")
    elif kind == "i16":
        d_in = torch.randint(-2048, 2048, (2 * n_samples,), dtype=torch.int16, device="cuda")
    else:
        d_in = torch.rand(2 * n_samples, dtype=torch.float32, device="cuda") * 2.0 - 1.0
    out = torch.empty(K * n, dtype=torch.float32, device="cuda")
    states = [torch.zeros(2 * K, dtype=torch.float32, device="cuda") for _ in range(2)]
    wsb = banks["composed"].workspace_bytes(n)
    ws = torch.empty(max(wsb, 16), dtype=torch.uint8, device="cuda")
    pi, po, pw = d_in.data_ptr(), out.data_ptr(), ws.data_ptr()
    ps = [s.data_ptr() for s in states]

    def leg(bank):
        run = {"u8": bank.run_u8, "i16": bank.run_i16, "cf32": bank.run}[kind]

        def fn(reps):
            for r in range(reps):
                run(pi, 0, po, n, 0, n, seam, ps[r & 1], ps[(r + 1) & 1], pw, wsb)
            torch.cuda.synchronize()
        return fn

    def env_leg(reps):
        run = {"u8": env.run_u8, "i16": env.run_i16, "cf32": env.run}[kind]
        for _ in range(reps):
            run(pi, 0, po, n, 0, n, seam, None, None, 0)
        torch.cuda.synchronize()

    fns = {name: leg(b) for name, b in banks.items()}
    got = {}
    for name, fn in fns.items():
        out.zero_()
        for s in states:
            s.zero_()
        fn(1)
        got[name] = (out.clone(), states[1].clone())
    for a, b in zip(got["fused"], got["composed"]):
        if not torch.equal(a.view(torch.int32), b.view(torch.int32)):
            sys.exit(f"nfm_bank_bench: the two routes differ at K = {K}, {n_samples} samples, {kind}, factor {factor}, seam {seam}")
    del got
    fns["env"] = env_leg
    return fns, n, (tb, banks, env, d_in, out, states, ws)


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("nfm_bank_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("nfm_bank_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, fused route (1), composed route (2) and the AM bank's envelope launch (reference) "
             "alternating; us per run of ALL K channels: median (min .. max)"]
    print(lines[0], flush=True)
    points = []
    for kind in KINDS:
        for factor in FACTORS:
            for seam in SEAMS:
                for size_name, n_samples in SIZES:
                    for K in CHANNELS:
                        fns, n, keep = legs(K, n_samples, kind, factor, seam)
                        reps = {}
                        for name, fn in fns.items():
                            fn(5)                                    # warm-up of this shape: code objects, table uploads, kernel attributes
                            per = timed(fn, 10) * 1e-6
                            reps[name] = max(5, min(20000, int(WINDOW_S / per)))
                        f0, r0 = L.nfm_bank_launches(), int(L.lib.sdrhip_debug_rows_launches())
                        times = {k: [] for k in fns}
                        for _ in range(a.rounds):
                            for name, fn in fns.items():
                                times[name].append(timed(fn, reps[name]))
                        nf, nr = L.nfm_bank_launches() - f0, int(L.lib.sdrhip_debug_rows_launches()) - r0
                        assert nf == a.rounds * reps["fused"] and nr == a.rounds * reps["composed"], "a leg took another route than the one it is named for"
                        med = {k: statistics.median(v) for k, v in times.items()}
                        fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                        clear = max(times["fused"]) < min(times["composed"])
                        line = (f"{kind:4s} /{factor:<2d} seam {seam:4d} {size_name:5s} K {K:2d}  outputs {n:7d} x {K:2d}   fused {fmt(times['fused'])}   "
                                f"composed {fmt(times['composed'])}   fused / composed {med['fused'] / med['composed']:.3f}"
                                f"{'' if clear else '   (not clear of the spread)'}   env {fmt(times['env'])}   fused / env {med['fused'] / med['env']:.3f}")
                        print(line, flush=True)
                        lines.append(line)
                        points.append((kind, factor, seam, size_name, K, med["fused"] / med["composed"], clear, med["fused"] / med["env"]))
                        del fns, keep
                        torch.cuda.empty_cache()
    nsum = 0
    for kind in KINDS:
        for factor in FACTORS:
            for seam in SEAMS:
                mine = [p for p in points if p[:3] == (kind, factor, seam)]
                ahead = [p for p in mine if p[6]]
                lost = [p for p in mine if not p[6]]
                r, e = [p[5] for p in ahead], [p[7] for p in mine]
                lines.append(f"# {kind} /{factor} seam {seam}: fused ahead (slowest fused round below the composed route's fastest) at {len(ahead)} of "
                             f"{len(mine)} points" + (f", ratio {min(r):.3f} .. {max(r):.3f}" if r else "")
                             + ("; NOT ahead at: " + ", ".join(f"{p[3]} K {p[4]} (ratio {p[5]:.3f})" for p in lost) if lost else "")
                             + f"; fused / env {min(e):.3f} .. {max(e):.3f}")
                nsum += 1
    print("\n".join(lines[-nsum:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
