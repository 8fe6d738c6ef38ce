"""The waterfall Pipe against what a caller did without it, and int16 input against convert + cfloat: both legs of every comparison
are code of the SAME build, alternating in one process.

    python tools/spectrum_pipe_bench.py [--rounds R] [--out profiles/spectrum_pipe_bench.txt]

(A) u8, n = 1024, hop = n, group 1 and 64 (mean power, dB), a stream of 512 blocks of 8192 samples handed over 1 / 16 / 128 blocks at
    a time.
      pipe    sdrhip_pipe_push_u8 per hand-over, rows popped as they become ready, one sdrhip_pipe_flush at the end
      caller  the bookkeeping a caller does alone: append the hand-over to a host buffer of its own, work out the complete rows, ONE
              synchronous sdrhip_spectrum_reduce_run over them, keep the rest for the next hand-over
    A host clock around the whole stream, first hand-over to last row in host memory.  Before a point is timed its two legs' rows are
    compared bit for bit.
(B) int16, n = 1024, hop = n, group 1 and 64, 2^20 and 2^24 samples resident in device memory.
      i16      one sdrhip_spectrum_reduce_run_device of an SDRHIP_IQ_I16 object
      convert  sdrhip_convert_i16_run into a float buffer, then the same call of an SDRHIP_IQ_CF32 object
    A host clock around `reps` back-to-back call sets that end in ONE device synchronise; rows compared bit for bit first.
Every figure is the median (min .. max) over the rounds.  "ahead" is the project's criterion: the leg's SLOWEST round is below the
other leg's FASTEST.  No number is fixed in advance and no route or auto rule is read from this sweep.  A missing GPU is an error."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import sdr_amd.lib as L

N, BLOCK, NBLOCKS = 1024, 8192, 512
FLOOR = -200.0
_u8p, _f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_float)


def pipe_leg(spec, group, blocks_per_push, iq, out):
    p = L.Pipe.spectrum(spec, N, group, L.REDUCE_MEAN_POWER, L.UNIT_DB, FLOOR)
    step = blocks_per_push * BLOCK
    base = iq.ctypes.data

    def fn():
        rows = 0
        for s0 in range(0, NBLOCKS * BLOCK, step):
            ready = L.lib.sdrhip_pipe_push_u8(p.h, C.cast(base + 2 * s0, _u8p), step)
            if ready > 0:
                rows += L.lib.sdrhip_pipe_pop_rows(p.h, C.cast(out.ctypes.data + 4 * N * rows, _f32p), ready * N, ready)
        ready = L.lib.sdrhip_pipe_flush(p.h)
        if ready > 0:
            rows += L.lib.sdrhip_pipe_pop_rows(p.h, C.cast(out.ctypes.data + 4 * N * rows, _f32p), ready * N, ready)
        return rows
    return fn, p


def caller_leg(spec, group, blocks_per_push, iq, out):
    step = blocks_per_push * BLOCK
    per_row = group * N
    held = np.empty(2 * (per_row + step), np.uint8)

    def fn():
        rows, have = 0, 0
        for s0 in range(0, NBLOCKS * BLOCK, step):
            held[2 * have:2 * (have + step)] = iq[2 * s0:2 * (s0 + step)]
            have += step
            r = have // per_row
            if r:
                L.check(L.lib.sdrhip_spectrum_reduce_run(spec.h, held.ctypes.data, r * per_row, N, r, group, L.REDUCE_MEAN_POWER, L.UNIT_DB, FLOOR,
                                                         out.ctypes.data + 4 * N * rows), "sdrhip_spectrum_reduce_run")
                rows += r
                rest = have - r * per_row
                held[:2 * rest] = held[2 * r * per_row:2 * have]
                have = rest
        return rows
    return fn, held


def timed(fn, reps=1):
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def fmt(v):
    return f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"


def verdict(a, b, name_a, name_b):
    if max(a) < min(b):
        return f"{name_a} ahead"
    if max(b) < min(a):
        return f"{name_b} ahead"
    return "neither clear of the spread"


def part_a(rounds, lines):
    iq = np.random.default_rng(5).integers(0, 256, 2 * NBLOCKS * BLOCK, dtype=np.uint8)
    for group in (1, 64):
        rows = NBLOCKS * BLOCK // (group * N)
        for bpp in (1, 16, 128):
            outs = {k: np.zeros(rows * N, np.float32) for k in ("pipe", "caller")}
            specs = {k: L.Spectrum(N, L.IQ_U8, L.WINDOW_HANNING, True, 1.0 / N) for k in outs}
            fns, keep = {}, []
            for k, make in (("pipe", pipe_leg), ("caller", caller_leg)):
                fns[k], held = make(specs[k], group, bpp, iq, outs[k])
                keep.append(held)
            for k, fn in fns.items():
                assert fn() == rows, f"{k}: wrong row count"
                fn()                                                 # warm-up: pinned buffers, plans, code objects
            if outs["pipe"].tobytes() != outs["caller"].tobytes():
                sys.exit(f"spectrum_pipe_bench: the two legs differ at group {group}, {bpp} blocks per hand-over")
            times = {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():
                    times[k].append(timed(fn))
            ms = NBLOCKS * BLOCK / 1e6
            line = (f"(A) u8 n {N} group {group:2d}  {bpp:3d} blocks per hand-over  {rows:5d} rows   pipe {fmt(times['pipe'])} us   caller {fmt(times['caller'])} us   "
                    f"pipe / caller {statistics.median(times['pipe']) / statistics.median(times['caller']):.3f}   "
                    f"pipe {ms / (statistics.median(times['pipe']) * 1e-6):.0f} Msamples/s   {verdict(times['pipe'], times['caller'], 'pipe', 'caller')}")
            print(line, flush=True)
            lines.append(line)
            del fns, keep, specs


def part_b(rounds, lines):
    for log2 in (20, 24):
        ns = 1 << log2
        d_i16 = torch.randint(-32768, 32768, (2 * ns,), dtype=torch.int16, device="cuda")
        d_cf = torch.empty(2 * ns, dtype=torch.float32, device="cuda")
        for group in (1, 64):
            rows = ns // (group * N)
            out = {k: torch.zeros(rows * N, dtype=torch.float32, device="cuda") for k in ("i16", "convert")}
            si = L.Spectrum(N, L.IQ_I16, L.WINDOW_HANNING, True, 1.0 / N)
            sc = L.Spectrum(N, L.IQ_CF32, L.WINDOW_HANNING, True, 1.0 / N)

            def leg_i16():
                si.reduce_device(d_i16.data_ptr(), ns, out["i16"].data_ptr(), group, L.REDUCE_MEAN_POWER, L.UNIT_DB, FLOOR, hop=N, rows_out=rows)

            def leg_convert():
                L.check(L.lib.sdrhip_convert_i16_run(None, d_i16.data_ptr(), d_cf.data_ptr(), 2 * ns), "sdrhip_convert_i16_run")
                sc.reduce_device(d_cf.data_ptr(), ns, out["convert"].data_ptr(), group, L.REDUCE_MEAN_POWER, L.UNIT_DB, FLOOR, hop=N, rows_out=rows)

            fns = {"i16": leg_i16, "convert": leg_convert}

            def run(fn, reps):
                for _ in range(reps):
                    fn()
                torch.cuda.synchronize()

            reps = {}
            for k, fn in fns.items():
                run(fn, 5)
                t0 = time.perf_counter()
                run(fn, 10)
                reps[k] = max(5, min(5000, int(0.05 / ((time.perf_counter() - t0) / 10))))
            if not torch.equal(out["i16"].view(torch.int32), out["convert"].view(torch.int32)):
                sys.exit(f"spectrum_pipe_bench: int16 and convert + cfloat differ at 2^{log2} samples, group {group}")
            times = {k: [] for k in fns}
            for _ in range(rounds):
                for k, fn in fns.items():
                    t0 = time.perf_counter()
                    run(fn, reps[k])
                    times[k].append((time.perf_counter() - t0) / reps[k] * 1e6)
            line = (f"(B) i16 n {N} group {group:2d}  2^{log2} samples  {rows:5d} rows   i16 {fmt(times['i16'])} us   convert + cf32 {fmt(times['convert'])} us   "
                    f"i16 / convert {statistics.median(times['i16']) / statistics.median(times['convert']):.3f}   "
                    f"{verdict(times['i16'], times['convert'], 'i16', 'convert + cf32')}")
            print(line, flush=True)
            lines.append(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("spectrum_pipe_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("spectrum_pipe_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the two legs of a point alternating; us per stream (A) / per call set (B): median (min .. max)"]
    print(lines[0], flush=True)
    part_a(a.rounds, lines)
    part_b(a.rounds, lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
