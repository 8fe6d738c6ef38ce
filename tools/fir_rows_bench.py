"""The row forms of the FIR filter, decimator and resampler on route 1 (one banked launch set) against K one-row calls of the same
build, alternating the two in one process.

    python tools/fir_rows_bench.py [--rounds R] [--out profiles/fir_rows_bench.txt]

Sweep: K = 1, 2, 8, 32 rows x 128, 1024, 16384 and 2^20 outputs per row, for three shapes -- the stages of a narrow-band receiver
behind a tuner bank --
  cdec   complex AVX decimator, 64 taps, by 4
  rres   real AVX resampler 3/10, the example chain's taps (tests/golden/example_taps.npz)
  rfilt  real symmetric AVX filter, the example chain's audio taps
each with seam_block 0 (a contiguous stream) and with the row's own block as the seam: seam_block = the inputs the row's outputs
consume, so the last outputs of the row straddle a seam and the launch has Cross outputs (a fix-up launch on the banked route).
  rows    one sdrhip_*_run_rows call, route 1: one tile launch for all K rows, and one fix-up launch where there is a seam
  calls   K one-row calls (sdrhip_decimator_run / sdrhip_resampler_run / sdrhip_filter_run) on the same stream, one row after the
          other -- whatever kernel the one-row operator picks for that length: the generic kernel for short rows, the specialised
          ones (the tiled c4 decimator, the 3/10 kernel, the real8 filter) for long ones
Every figure is a host clock around `reps` back-to-back call sets that end in ONE device synchronise, after warm-up runs of the
same shape; reps are chosen so that a window lasts about 0.05 s.  The two legs alternate within each round; the table gives the
median and the spread over the rounds.  Both legs are driven through ctypes on resident tensors.  Before it is timed, a point's two
legs are compared bit for bit.
No number is fixed in advance: the yardstick is the K-call loop.  A point is "ahead" by the project's criterion: the rows form's
SLOWEST round is below the loop's FASTEST.  The last lines say, per shape and seam, where that holds.  A missing GPU is an error."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import sdr_amd.lib as L

ROWS = (1, 2, 8, 32)
SIZES = (("128", 128), ("1024", 1024), ("16384", 16384), ("2^20", 1 << 20))
WINDOW_S = 0.05


def shapes():
    """name -> (descriptor, one-row function, rows function, interpolation, decimation, floats per element)"""
    taps = np.load(os.path.join(ROOT, "tests", "golden", "example_taps.npz"))
    rng = np.random.default_rng(64)
    dec = L.Decimator(4, (rng.standard_normal(64) * 0.05).astype(np.float32), L.ORDER_AVX, complex_=True)
    res = L.Resampler(3, 10, taps["audio_resampler"], L.ORDER_AVX)
    fil = L.Filter(taps["audio_filter_half"], L.ORDER_AVX, sym=True)
    return {"cdec": (dec, L.lib.sdrhip_decimator_run, L.lib.sdrhip_decimator_run_rows, 1, 4, 2),
            "rres": (res, L.lib.sdrhip_resampler_run, L.lib.sdrhip_resampler_run_rows, 3, 10, 1),
            "rfilt": (fil, L.lib.sdrhip_filter_run, L.lib.sdrhip_filter_run_rows, 1, 1, 1)}


def legs(name, shape, K, n, seamed):
    """-> ({leg: function(reps) that runs reps call sets over all K rows and synchronises}, what to keep alive, seam block)"""
    desc, one, rows_fn, I, D, w = shape
    need = -(-((n - 1) * D) // I) + desc.num_coeffs // I            # inputs a row holds: the header's guaranteed range
    seam = -(-(n * D) // I) if seamed else 0
    g = torch.Generator(device="cuda").manual_seed(4321 + K)
    x = torch.rand((K, need * w), generator=g, dtype=torch.float32, device="cuda") * 2 - 1
    y = [torch.empty((K, n * w), dtype=torch.float32, device="cuda") for _ in range(2)]
    px, py, h = x.data_ptr(), [t.data_ptr() for t in y], desc.h
    tail = (seam, 0) if name == "rres" else (seam,)

    def rows(reps, o=0):
        for _ in range(reps):
            rows_fn(h, None, px, need * w, 0, py[o], n * w, K, 0, n, *tail, 1)
        torch.cuda.synchronize()

    def calls(reps, o=1):
        for _ in range(reps):
            for r in range(K):
                one(h, None, px + 4 * r * need * w, 0, py[o] + 4 * r * n * w, 0, n, *tail)
        torch.cuda.synchronize()

    rows(1)
    calls(1)
    if not torch.equal(y[0].view(torch.int32), y[1].view(torch.int32)):
        sys.exit(f"fir_rows_bench: the rows call and the one-row calls differ: {name}, K = {K}, n = {n}, seam {seam}")
    return {"rows": rows, "calls": calls}, (x, y), seam


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
        sys.exit("fir_rows_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("fir_rows_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the rows call (route 1) and K one-row calls alternating; us per call set over ALL K rows: median (min .. max)",
             "# cdec: complex AVX decimator 64 taps / 4; rres: real AVX resampler 3/10, 31 taps; rfilt: real symmetric AVX filter, 2 x 32 taps; n = outputs per row"]
    print("\n".join(lines), flush=True)
    points = []
    all_shapes = shapes()
    for name, shape in all_shapes.items():
        for seamed in (False, True):
            for size_name, n in SIZES:
                for K in ROWS:
                    fns, keep, seam = legs(name, shape, K, n, seamed)
                    reps = {}
                    for leg, fn in fns.items():
                        fn(3)                                            # warm-up of this shape
                        per = timed(fn, 5) * 1e-6
                        reps[leg] = max(3, min(20000, int(WINDOW_S / per)))
                    l0, f0 = L.fir_rows_launches(), L.fir_rows_fixups()
                    times = {k: [] for k in fns}
                    for _ in range(a.rounds):
                        for leg, fn in fns.items():
                            times[leg].append(timed(fn, reps[leg]))
                    sets = a.rounds * reps["rows"]
                    assert L.fir_rows_launches() - l0 == sets and L.fir_rows_fixups() - f0 == (sets if seamed else 0), \
                        "the rows leg took another route than one tile launch (and one fix-up launch with a seam) per call"
                    plan = L.fir_rows_plan(shape[0], 0, n, K, seam)
                    med = {k: statistics.median(v) for k, v in times.items()}
                    fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                    clear = max(times["rows"]) < min(times["calls"])
                    line = (f"{name:5s} seam {'block' if seamed else '0    '} n {size_name:6s} K {K:2d}  tiles {plan['tiles_per_row']:5d} x {plan['tile_outputs']:4d}  "
                            f"rows {fmt(times['rows'])}   calls {fmt(times['calls'])}   rows / calls {med['rows'] / med['calls']:.3f}"
                            f"{'' if clear else '   (not ahead: slowest rows round against fastest loop round)'}")
                    print(line, flush=True)
                    lines.append(line)
                    points.append((name, seamed, size_name, K, med["rows"] / med["calls"], clear))
                    del fns, keep
                    torch.cuda.empty_cache()
    for name in all_shapes:
        for seamed in (False, True):
            mine = [p for p in points if p[0] == name and p[1] == seamed]
            ahead = {s: [K for _, _, s2, K, _, c in mine if s2 == s and c] for s, _ in SIZES}
            lines.append(f"# {name} seam {'block' if seamed else '0'}: ahead at " + "; ".join(f"n {s}: K {ahead[s] if ahead[s] else 'none'}" for s, _ in SIZES))
    print("\n".join(lines[-2 * len(all_shapes):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
