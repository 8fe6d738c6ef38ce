"""The tuner's routes against each other and against the plain decimator at the same shape.

    python tools/tuner_bench.py [--sizes 16777216 134217728] [--seams 0 8192] [--rounds 7] [--iters 10] [--json FILE]

Decimation 8, 127 taps (128 prepared), AVX order, oscillator period 1000; u8 and cfloat input; per size and seam_block

  fused      Tuner.run / run_u8 on the fused route     (kernels_tuner.hip: the mix in the tile kernel's loader)
  two_pass   the same on the two-pass route            (mix kernel -> scratch -> the stock decimator, in 2^22-sample chunks)
  decim_tile Decimator.run / run_u8 with the systolic kernel switched off: the tile kernel the fused route is built on, WITHOUT
             a mix -- what the fused loader costs on top of it
  decim      Decimator.run / run_u8 as the library routes it (the systolic kernel at these sizes): the floor, also without a mix

All four are timed alternately in one process, `rounds` windows of `iters` calls each, every window ended by a device synchronise;
the table shows the median window and the spread (min .. max).  GB/s are the bytes the operator needs (2 or 8 B in per sample, 1 B
out) over that time: an achieved rate of the call, not a kernel's share of peak.  Before timing, fused and two_pass outputs are
compared bit for bit on the timed input.  No GPU: the tool fails (there is no fall-back)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="*", default=[1 << 24, 1 << 27])
    ap.add_argument("--seams", type=int, nargs="*", default=[0, 8192])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    import sdr_amd.lib as L
    import signals as S
    if L.device_count() < 1:
        sys.exit("tuner_bench: no HIP device")
    taps = S.taps_decim127()
    osc = L.tuner_shift_table(7, 1000)
    print(f"# {L.device_name()}  decimation 8, 128 prepared taps, period 1000, rounds {args.rounds} x {args.iters} calls")
    print("| samples | input | seam | route | ms per call (median, min .. max) | Gsamples/s | GB/s needed bytes |")
    print("|---|---|---|---|---|---|---|")
    results = []
    rng = np.random.default_rng(1)
    for n in args.sizes:
        K = (n - 128) // 8 + 1
        for is_u8, name in ((True, "u8"), (False, "cfloat")):
            if is_u8:
                d_in = torch.from_numpy(rng.integers(0, 256, 2 * n, dtype=np.uint8)).cuda()
            else:
                d_in = (torch.rand(2 * n, dtype=torch.float32, device="cuda") * 2 - 1)
            outs = {r: torch.empty(2 * K, dtype=torch.float32, device="cuda") for r in ("fused", "two_pass", "decim_tile", "decim")}
            tuner = {"fused": L.Tuner(8, taps, osc), "two_pass": L.Tuner(8, taps, osc)}
            tuner["fused"].set_route(L.TUNER_ROUTE_FUSED)
            tuner["two_pass"].set_route(L.TUNER_ROUTE_TWO_PASS)
            dec = L.Decimator(8, taps, L.ORDER_AVX, complex_=True)
            for seam in args.seams:
                def call(r):
                    if r in tuner:
                        (tuner[r].run_u8 if is_u8 else tuner[r].run)(d_in.data_ptr(), 0, outs[r].data_ptr(), 0, K, seam)
                        return
                    L.lib.sdrhip_debug_set_systolic(0 if r == "decim_tile" else 2)
                    (dec.run_u8 if is_u8 else dec.run)(d_in.data_ptr(), 0, outs[r].data_ptr(), 0, K, seam)

                for r in outs:                      # warm-up: code objects, tap uploads, the scratch
                    for _ in range(2):
                        call(r)
                torch.cuda.synchronize()
                same = bool(torch.equal(outs["fused"].view(torch.int32), outs["two_pass"].view(torch.int32)))
                if not same:
                    sys.exit(f"tuner_bench: fused and two-pass outputs differ ({n} samples, {name}, seam {seam})")
                ms = {r: [] for r in outs}
                for _ in range(args.rounds):
                    for r in outs:                  # alternate the routes inside every round
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        for _ in range(args.iters):
                            call(r)
                        torch.cuda.synchronize()
                        ms[r].append((time.perf_counter() - t0) * 1e3 / args.iters)
                L.lib.sdrhip_debug_set_systolic(2)
                need = n * (2 if is_u8 else 8) + K * 8
                for r in outs:
                    med = statistics.median(ms[r])
                    results.append({"samples": n, "input": name, "seam": seam, "route": r, "ms_median": med, "ms_min": min(ms[r]),
                                    "ms_max": max(ms[r]), "gsamples_per_s": n / med / 1e6, "needed_GB_per_s": need / med / 1e6})
                    print(f"| {n} | {name} | {seam} | {r} | {med:.3f} ({min(ms[r]):.3f} .. {max(ms[r]):.3f}) | {n / med / 1e6:.2f} | {need / med / 1e6:.1f} |",
                          flush=True)
            del d_in, outs, tuner, dec
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
