"""Spectrum rows per second: the one-kernel route, the hipFFT route, and the host way (what the library offered before the operator).

    python tools/spectrum_bench.py [--samples 16777216] [--rounds 7] [--iters 20] [--json FILE]

For n in {1024, 8192} x {u8, cf32}: a batch of `samples / n` rows with hop = n (16 Mi samples by default: 16384 rows of 1024, far more
workgroups than the chip has CUs) through

  fused    Spectrum.run_device on the one-kernel route             (kernels_spectrum.hip)
  hipfft   Spectrum.run_device on the hipFFT route                 (pre-kernel, hipFFT Z2Z in place, post-kernel)
  host     numpy convert / sign / window on the host + Fft(n, batch).run + numpy magnitude: the only way to the same rows without
           the operator; host arrays in, host arrays out, on an eighth of the rows (it is slow)

The two device routes are timed alternately, `rounds` windows of `iters` calls each, every window ended by a device synchronise; the
table shows the median window and the spread (min .. max).  Bytes/s are the bytes the operator needs (2 or 8 B in, 4 B out per sample)
over that time: an achieved rate of the call, not a kernel's share of peak.  Before timing, the two routes' outputs are compared on
the timed input.  No GPU: the tool fails (there is no fall-back)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=1 << 24)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 8192])
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    import torch
    import sdr_amd.lib as L
    if L.device_count() < 1:
        sys.exit("spectrum_bench: no HIP device")
    print(f"# {L.device_name()}  samples per call {args.samples}  rounds {args.rounds} x {args.iters} calls")
    print("| n | input | rows | route | ms per call (median, min .. max) | rows/s | GB/s needed bytes | max rel. diff vs fused |")
    print("|---|---|---|---|---|---|---|---|")
    results = []
    rng = np.random.default_rng(1)
    for n in args.sizes:
        rows = args.samples // n
        for fmt, name in ((L.IQ_U8, "u8"), (L.IQ_CF32, "cf32")):
            if fmt == L.IQ_U8:
                iq = rng.integers(0, 256, 2 * rows * n, dtype=np.uint8)
            else:
                iq = rng.standard_normal(2 * rows * n).astype(np.float32)
            d_in = torch.from_numpy(iq).cuda()
            d_out = {r: torch.empty(rows * n, dtype=torch.float32, device="cuda") for r in ("fused", "hipfft")}
            spec = {}
            for r, route in (("fused", L.SPECTRUM_ROUTE_FUSED), ("hipfft", L.SPECTRUM_ROUTE_HIPFFT)):
                spec[r] = L.Spectrum(n, fmt, L.WINDOW_HANNING, True, 1.0 / n)
                spec[r].set_route(route)

            def call(r):
                spec[r].run_device(d_in.data_ptr(), rows * n, d_out[r].data_ptr(), hop=n, rows=rows)

            for r in spec:                      # warm-up: code objects, the hipFFT plan, the scratch
                for _ in range(3):
                    call(r)
            torch.cuda.synchronize()
            a, b = d_out["fused"].cpu().numpy().astype(np.float64), d_out["hipfft"].cpu().numpy().astype(np.float64)
            diff = float(np.max(np.abs(a - b)) / np.max(np.abs(a)))
            ms = {r: [] for r in spec}
            for _ in range(args.rounds):
                for r in spec:                  # alternate the routes inside every round
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        call(r)
                    torch.cuda.synchronize()
                    ms[r].append((time.perf_counter() - t0) * 1e3 / args.iters)
            need = rows * n * ((2 if fmt == L.IQ_U8 else 8) + 4)
            for r in spec:
                med = statistics.median(ms[r])
                results.append({"n": n, "input": name, "rows": rows, "route": r, "ms_median": med, "ms_min": min(ms[r]), "ms_max": max(ms[r]),
                                "rows_per_s": rows / med * 1e3, "needed_GB_per_s": need / med / 1e6, "max_rel_diff_vs_fused": diff if r == "hipfft" else 0.0})
                print(f"| {n} | {name} | {rows} | {r} | {med:.3f} ({min(ms[r]):.3f} .. {max(ms[r]):.3f}) | {rows / med * 1e3:.3e} | {need / med / 1e6:.1f} | "
                      f"{diff:.1e} |" if r == "hipfft" else
                      f"| {n} | {name} | {rows} | {r} | {med:.3f} ({min(ms[r]):.3f} .. {max(ms[r]):.3f}) | {rows / med * 1e3:.3e} | {need / med / 1e6:.1f} | |")

            # the host way, on an eighth of the rows
            hrows = max(rows // 8, 1)
            fft = L.Fft(n, batch=hrows)
            w = spec["fused"].window() * np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
            part = iq[:2 * hrows * n]

            def host():
                v = (part.astype(np.float64) - 128.0) / 128.0 if fmt == L.IQ_U8 else part.astype(np.float64)
                x = (v[0::2] + 1j * v[1::2]).reshape(hrows, n) * w[None, :]
                return ((1.0 / n) * np.abs(fft.run(x))).astype(np.float32)

            ref = host()                        # warm-up, and a third opinion on the outputs
            hdiff = float(np.max(np.abs(ref.astype(np.float64).reshape(-1) - a[:hrows * n])) / np.max(np.abs(a)))
            hms = []
            for _ in range(3):
                t0 = time.perf_counter()
                host()
                hms.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(hms)
            results.append({"n": n, "input": name, "rows": hrows, "route": "host", "ms_median": med, "ms_min": min(hms), "ms_max": max(hms),
                            "rows_per_s": hrows / med * 1e3, "needed_GB_per_s": need / rows * hrows / med / 1e6, "max_rel_diff_vs_fused": hdiff})
            print(f"| {n} | {name} | {hrows} | host | {med:.1f} ({min(hms):.1f} .. {max(hms):.1f}) | {hrows / med * 1e3:.3e} | {need / rows * hrows / med / 1e6:.2f} | {hdiff:.1e} |")
            del fft, spec, d_in, d_out
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
