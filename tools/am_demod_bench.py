"""The rows form of amDemod against K one-row calls of the same build, alternating the two in one process.

    python tools/am_demod_bench.py [--rounds R] [--out profiles/am_demod_bench.txt]

Sweep: K = 1, 2, 8, 32 rows x n = 1024, 16384 and 2^20 samples per row.
  rows    one sdrhip_am_demod_run_rows call: one launch for all K rows
  calls   K sdrhip_am_demod_run calls on the same stream, one row after the other -- the only way to get K rows without the rows form
Every figure is a host clock around `reps` back-to-back call sets that end in ONE device synchronise, after warm-up runs of the
same shape; reps are chosen so that a window lasts about 0.1 s.  The two legs alternate within each round; the table gives the
median and the spread over the rounds.  Both legs are driven through ctypes on resident tensors.  Before it is timed, a point's two
legs are compared bit for bit.
No number is fixed in advance: the yardstick is the K-call loop.  A point is "ahead" by the project's criterion: the rows form's
SLOWEST round is below the loop's FASTEST.  The last lines say where that holds, whether K = 1 is level, and the bytes moved per
second (8 read + 4 written per sample) at the largest point.  No routing rule depends on this table.  A missing GPU is an error."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import sdr_amd.lib as L

ROWS = (1, 2, 8, 32)
SIZES = (("1024", 1024), ("16384", 16384), ("2^20", 1 << 20))
WINDOW_S = 0.1
BYTES_PER_SAMPLE = 12


def legs(K, n):
    """-> ({name: function(reps) that runs reps call sets over all K rows and synchronises}, what to keep alive)"""
    g = torch.Generator(device="cuda").manual_seed(1234 + K)
    x = torch.randn((K, 2 * n), generator=g, dtype=torch.float32, device="cuda") * 0.3
    y = [torch.empty((K, n), dtype=torch.float32, device="cuda") for _ in range(2)]
    px, py = x.data_ptr(), [t.data_ptr() for t in y]
    lib = L.lib

    def rows(reps, o=0):
        for _ in range(reps):
            lib.sdrhip_am_demod_run_rows(None, px, 2 * n, py[o], n, K, n)
        torch.cuda.synchronize()

    def calls(reps, o=1):
        for _ in range(reps):
            for r in range(K):
                lib.sdrhip_am_demod_run(None, px + 8 * r * n, py[o] + 4 * r * n, n)
        torch.cuda.synchronize()
    # the two legs compute the same rows (tests/test_gpu_am_demod.py holds them to the model; here: that the legs time the same work)
    rows(1)
    calls(1)
    if not torch.equal(y[0].view(torch.int32), y[1].view(torch.int32)):
        sys.exit(f"am_demod_bench: the rows call and the one-row calls differ: K = {K}, n = {n}")
    return {"rows": rows, "calls": calls}, (x, y)


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
        sys.exit("am_demod_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("am_demod_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the rows call and K one-row calls alternating; us per call set over ALL K rows: median (min .. max)",
             "# amDemod: noise at level 0.3, rows tight and 16-byte aligned"]
    print("\n".join(lines), flush=True)
    points = []
    for size_name, n in SIZES:
        for K in ROWS:
            fns, keep = legs(K, n)
            reps = {}
            for name, fn in fns.items():
                fn(3)                                            # warm-up of this shape
                per = timed(fn, 5) * 1e-6
                reps[name] = max(3, min(20000, int(WINDOW_S / per)))
            l0 = L.am_demod_launches()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for name, fn in fns.items():
                    times[name].append(timed(fn, reps[name]))
            assert L.am_demod_launches() - l0 == a.rounds * (reps["rows"] + K * reps["calls"]), "a call was not exactly one launch"
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
            clear = max(times["rows"]) < min(times["calls"])
            line = (f"am  n {size_name:6s} K {K:2d}  rows {fmt(times['rows'])}   calls {fmt(times['calls'])}   "
                    f"rows / calls {med['rows'] / med['calls']:.3f}{'' if clear else '   (not ahead: slowest rows round against fastest loop round)'}")
            print(line, flush=True)
            lines.append(line)
            points.append((n, size_name, K, med["rows"] / med["calls"], clear, med["rows"], med["calls"]))
            del fns, keep
            torch.cuda.empty_cache()
    lost = [(s, K, r) for _, s, K, r, c, _, _ in points if K > 1 and not c]
    one = [(s, r, c) for _, s, K, r, c, _, _ in points if K == 1]
    tail = ["# K >= 2 points not ahead: " + (", ".join(f"n {s} K {K} (ratio {r:.3f})" for s, K, r in lost) if lost else "none"),
            "# K = 1 rows / calls " + ", ".join(f"n {s} {r:.3f}{' ahead' if c else ''}" for s, r, c in one)]
    n, s, K, _, _, t_rows, t_calls = points[-1]
    moved = BYTES_PER_SAMPLE * n * K
    tail.append(f"# n {s} K {K}: {moved / 1e6:.1f} MB moved per call set (8 bytes read, 4 written per sample): rows {moved / t_rows / 1e3:.1f} GB/s, "
                f"calls {moved / t_calls / 1e3:.1f} GB/s")
    lines += tail
    print("\n".join(tail), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
