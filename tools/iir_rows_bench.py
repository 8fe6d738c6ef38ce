"""The row forms of agc, dcBlocker and fmDemod against K one-row calls of the same build, alternating the two in one process.

    python tools/iir_rows_bench.py [--rounds R] [--out profiles/iir_rows_bench.txt]

Sweep: K = 1, 2, 8, 32 rows x n = 1024, 16384 and 2^20 samples per row, for the three operators, with a workspace and the default
run-in (agc at mu = 0.01: 12808 samples; dcBlocker: 12288), so n = 1024 and 16384 take the sequential walk -- what a live receiver's
blocks do -- and 2^20 the chunks.
  rows    one sdrhip_*_run_rows call: one launch set for all K rows
  calls   K one-row calls (sdrhip_agc_run / sdrhip_dc_blocker_run / sdrhip_fm_demod_run) on the same stream, one row after the
          other -- the only way to get K rows without the row forms
Every figure is a host clock around `reps` back-to-back call sets that end in ONE device synchronise, after warm-up runs of the
same shape; reps are chosen so that a window lasts about 0.1 s.  The two legs alternate within each round; the table gives the
median and the spread over the rounds.  Both legs are driven through ctypes on resident tensors.  Before it is timed, a point's two
legs are compared bit for bit, final states included.
No number is fixed in advance: the yardstick is the K-call loop.  A point is "ahead" by the project's criterion: the rows form's
SLOWEST round is below the loop's FASTEST.  The last lines say, per operator, where that holds.  A missing GPU is an error."""
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
OPS = ("agc", "dc", "fm")
MU, REF = 0.01, 1.0
WINDOW_S = 0.1


def legs(op, K, n):
    """-> ({name: function(reps) that runs reps call sets over all K rows and synchronises}, what to keep alive)"""
    g = torch.Generator(device="cuda").manual_seed(1234 + K)
    width = n if op == "dc" else 2 * n
    x = torch.randn((K, width), generator=g, dtype=torch.float32, device="cuda") * 0.3
    y = [torch.empty((K, n if op == "fm" else width), dtype=torch.float32, device="cuda") for _ in range(2)]
    px, py = x.data_ptr(), [t.data_ptr() for t in y]
    ow = y[0].shape[1]
    lib = L.lib
    if op == "fm":
        def rows(reps, o=0):
            for _ in range(reps):
                lib.sdrhip_fm_demod_run_rows(None, px, width, 0, py[o], ow, K, 0, n, None, None)
            torch.cuda.synchronize()

        def calls(reps, o=1):
            for _ in range(reps):
                for r in range(K):
                    lib.sdrhip_fm_demod_run(None, px + 4 * r * width, 0, py[o] + 4 * r * ow, 0, n, 0.0, 0.0)
            torch.cuda.synchronize()
        keep = (x, y)
        fins = None
    else:
        per = 2 if op == "dc" else 1
        st = torch.tensor([[0.0, 0.0]] * K if op == "dc" else [[1.0]] * K, dtype=torch.float32, device="cuda")
        fins = [torch.empty((K, per), dtype=torch.float32, device="cuda") for _ in range(2)]
        pf = [t.data_ptr() for t in fins]
        if op == "dc":
            wsb, wsb1 = lib.sdrhip_dc_blocker_rows_workspace_bytes(K, n), lib.sdrhip_dc_blocker_workspace_bytes(n)
        else:
            wsb, wsb1 = lib.sdrhip_agc_rows_workspace_bytes(K, n), lib.sdrhip_agc_workspace_bytes(n)
        ws, ws1 = torch.empty(wsb, dtype=torch.uint8, device="cuda"), torch.empty(wsb1, dtype=torch.uint8, device="cuda")
        pw, pw1, ps = ws.data_ptr(), ws1.data_ptr(), st.data_ptr()

        if op == "dc":
            def rows(reps, o=0):
                for _ in range(reps):
                    lib.sdrhip_dc_blocker_run_rows(None, px, width, py[o], ow, K, n, ps, pf[o], pw, wsb, 0)
                torch.cuda.synchronize()

            def calls(reps, o=1):
                for _ in range(reps):
                    for r in range(K):
                        lib.sdrhip_dc_blocker_run(None, px + 4 * r * width, py[o] + 4 * r * ow, n, 0.0, 0.0, pf[o] + 8 * r, pw1, wsb1, 0)
                torch.cuda.synchronize()
        else:
            def rows(reps, o=0):
                for _ in range(reps):
                    lib.sdrhip_agc_run_rows(None, px, width, py[o], ow, K, n, MU, REF, ps, pf[o], pw, wsb, 0)
                torch.cuda.synchronize()

            def calls(reps, o=1):
                for _ in range(reps):
                    for r in range(K):
                        lib.sdrhip_agc_run(None, px + 4 * r * width, py[o] + 4 * r * ow, n, MU, REF, 1.0, pf[o] + 4 * r, pw1, wsb1, 0)
                torch.cuda.synchronize()
        keep = (x, y, st, fins, ws, ws1)
    # the two legs compute the same rows (tests/test_gpu_rows.py holds the row forms to the models; here: that the legs time the same work)
    rows(1)
    calls(1)
    if not torch.equal(y[0].view(torch.int32), y[1].view(torch.int32)) or (fins and not torch.equal(fins[0].view(torch.int32), fins[1].view(torch.int32))):
        sys.exit(f"iir_rows_bench: the rows call and the one-row calls differ: {op}, K = {K}, n = {n}")
    return {"rows": rows, "calls": calls}, keep


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def route(op, K, n):
    if op == "fm":
        return "one kernel"
    chunks = (L.dc_rows_plan(K, n) if op == "dc" else L.agc_rows_plan(K, n, MU))[0]
    return f"{chunks} chunks a row" if chunks else "sequential walk"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("iir_rows_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("iir_rows_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the rows call and K one-row calls alternating; us per call set over ALL K rows: median (min .. max)",
             f"# agc: mu {MU}, reference {REF}, noise at level 0.3; workspace given, default run-in"]
    print("\n".join(lines), flush=True)
    points = []
    for op in OPS:
        for size_name, n in SIZES:
            for K in ROWS:
                fns, keep = legs(op, K, n)
                reps = {}
                for name, fn in fns.items():
                    fn(3)                                            # warm-up of this shape
                    per = timed(fn, 5) * 1e-6
                    reps[name] = max(3, min(20000, int(WINDOW_S / per)))
                l0 = L.rows_launches()
                times = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for name, fn in fns.items():
                        times[name].append(timed(fn, reps[name]))
                per_call = (L.rows_launches() - l0) / (a.rounds * reps["rows"])
                assert per_call in (1, 5), "the rows leg took another route than one launch set per call"
                med = {k: statistics.median(v) for k, v in times.items()}
                fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                clear = max(times["rows"]) < min(times["calls"])
                line = (f"{op:3s} n {size_name:6s} K {K:2d}  {route(op, K, n):16s} rows {fmt(times['rows'])}   calls {fmt(times['calls'])}   "
                        f"rows / calls {med['rows'] / med['calls']:.3f}{'' if clear else '   (not ahead: slowest rows round against fastest loop round)'}")
                print(line, flush=True)
                lines.append(line)
                points.append((op, n, size_name, K, med["rows"] / med["calls"], clear))
                del fns, keep
                torch.cuda.empty_cache()
    for op in OPS:
        mine = [p for p in points if p[0] == op]
        lost = [(s, K, r) for _, _, s, K, r, c in mine if K > 1 and not c]
        one = [(s, r, c) for _, _, s, K, r, c in mine if K == 1]
        short = [c for _, n, _, K, _, c in mine if K >= 8 and n == 1024]
        lines.append(f"# {op}: K >= 8 at n = 1024 {'ahead at every point' if all(short) else 'NOT ahead at every point'}; K >= 2 points not ahead: "
                     + (", ".join(f"n {s} K {K} (ratio {r:.3f})" for s, K, r in lost) if lost else "none"))
        lines.append(f"# {op}: K = 1 rows / calls " + ", ".join(f"n {s} {r:.3f}{' ahead' if c else ''}" for s, r, c in one))
    print("\n".join(lines[-2 * len(OPS):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
