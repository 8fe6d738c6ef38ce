"""Reduced spectrum rows: the reducing call against what the library offered before it.

    python tools/spectrum_reduce_bench.py [--samples 16777216] [--rounds 7] [--iters 10] [--reduce 0|1|2] [--out FILE]

For n in {1024, 8192}, hop = n, u8 input, and group in {16, 1024, all rows} (a batch of `samples / n` input rows), mean power (or with
--reduce 1 / 2 the mean magnitude / the max hold), linear:

  reduce    Spectrum.reduce_device: one call, rows_out x n float32 out                        (the new code)
  rows+torch  Spectrum.run_device into a full rows x n float32 buffer, then torch on the same stream: square, mean over the group axis
            (the parent commit's way; run_device's kernels are the parent's)

The two are timed alternately, `rounds` windows of `iters` calls each, every window ended by a device synchronise; the table shows the
median window and the spread (min .. max).  Before timing the two results are compared (linear mean power, relative to the largest
bin).  Where rows_out = 1 (group = all rows) the reducing call is also timed with the split forced off and on, which is the
measurement the `auto` rule of sdrhip_spectrum_set_reduce_split is to be set from.  No GPU: the tool fails (there is no fall-back)."""
import argparse
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
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--sizes", type=int, nargs="*", default=[1024, 8192])
    ap.add_argument("--reduce", type=int, default=0, choices=[0, 1, 2], help="0 mean power, 1 mean magnitude, 2 max hold")
    ap.add_argument("--out", default=None, help="also write the table to this file")
    args = ap.parse_args()

    import torch
    import sdr_amd.lib as L
    if L.device_count() < 1:
        sys.exit("spectrum_reduce_bench: no HIP device")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"# {L.device_name()}  u8 samples per call {args.samples}  hop = n  {('mean power', 'mean magnitude', 'max hold')[args.reduce]}  rounds {args.rounds} x {args.iters} calls")
    emit("| n | group | rows_out | way | ms per call (median, min .. max) | input rows/s | max rel. diff vs rows+torch |")
    emit("|---|---|---|---|---|---|---|")
    rng = np.random.default_rng(1)
    stream = torch.cuda.current_stream().cuda_stream
    for n in args.sizes:
        rows = args.samples // n
        iq = rng.integers(0, 256, 2 * rows * n, dtype=np.uint8)
        d_in = torch.from_numpy(iq).cuda()
        d_rows = torch.empty(rows * n, dtype=torch.float32, device="cuda")
        for group in (16, 1024, rows):
            if group > rows or rows % group:
                continue
            rows_out = rows // group
            spec = {}
            for way, mode in (("reduce", L.REDUCE_SPLIT_AUTO), ("reduce never-split", L.REDUCE_SPLIT_NEVER), ("reduce always-split", L.REDUCE_SPLIT_ALWAYS)):
                spec[way] = L.Spectrum(n, L.IQ_U8, L.WINDOW_HANNING, True, 1.0 / n)
                spec[way].set_route(L.SPECTRUM_ROUTE_FUSED)
                spec[way].set_reduce_split(mode)
            d_red = torch.empty(rows_out * n, dtype=torch.float32, device="cuda")
            result = {}

            def reduce_call(way):
                spec[way].reduce_device(d_in.data_ptr(), rows * n, d_red.data_ptr(), group, args.reduce, L.UNIT_LINEAR, hop=n, rows_out=rows_out,
                                        stream=stream)
                result[way] = d_red

            def parent_call(way):
                spec["reduce"].run_device(d_in.data_ptr(), rows * n, d_rows.data_ptr(), hop=n, rows=rows, stream=stream)
                r = d_rows.view(rows_out, group, n)
                result[way] = torch.square(r).mean(dim=1) if args.reduce == 0 else r.mean(dim=1) if args.reduce == 1 else r.amax(dim=1)

            ways = [("reduce", reduce_call), ("rows+torch", parent_call)]
            if rows_out == 1:
                ways += [("reduce never-split", reduce_call), ("reduce always-split", reduce_call)]
            diff = {}
            for way, call in ways:                      # warm-up (code objects, scratch, torch's allocator) and the comparison
                for _ in range(2):
                    call(way)
                torch.cuda.synchronize()
                diff[way] = result[way].reshape(rows_out, n).double().cpu().numpy()
            ref = diff["rows+torch"]
            ms = {way: [] for way, _ in ways}
            for _ in range(args.rounds):
                for way, call in ways:                  # alternate the ways inside every round
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        call(way)
                    torch.cuda.synchronize()
                    ms[way].append((time.perf_counter() - t0) * 1e3 / args.iters)
            for way, _ in ways:
                med = statistics.median(ms[way])
                rel = "" if way == "rows+torch" else f"{float(np.max(np.abs(diff[way] - ref)) / np.max(np.abs(ref))):.1e}"
                emit(f"| {n} | {group} | {rows_out} | {way} | {med:.3f} ({min(ms[way]):.3f} .. {max(ms[way]):.3f}) | {rows / med * 1e3:.3e} | {rel} |")
            del spec, d_red, result
        del d_in, d_rows
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
