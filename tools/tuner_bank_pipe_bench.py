"""The tuner bank's Pipe against what a caller of K channels had before it: K one-row Pipe.tuner objects fed the same pushes.  Both
in one process, alternating.

    python tools/tuner_bank_pipe_bench.py [--rounds R] [--out profiles/tuner_bank_pipe_bench.txt]
    python tools/tuner_bank_pipe_bench.py --i16 [--rounds R] [--out profiles/tuner_i16_pipe_bench.txt]

Sweep: K = 1, 2, 8, 12, 32 channels x pushes of 1, 16 and 128 source blocks (8192 samples each, one push = one block of that many
samples) x two ways of pushing, 128 prepared taps / 8, block_size_out 1024:
  memcpy   push(block): the library copies the caller's block into its pinned staging buffer -- K copies for K pipes
  buffer   input_buffer / push of that pointer: the source writes the staging buffer itself (here: one numpy copy of the block into
           it, inside the clock on both sides).  A source can write ONE buffer: with K pipes the caller copies the block from pipe
           0's staging buffer into the other K - 1
Legs:
  cfloat   ONE cfloat bank Pipe against K cfloat Pipes
  u8       ONE u8 bank Pipe (2 bytes per sample over the link) against the same K cfloat Pipes fed floats converted BEFORE the clock
           starts -- the conversion a u8 source owes the old way is left out, which favours the old way
  ragged   memcpy pushes of seeded sizes in [256, 3 * 8192], odd ones included, cfloat and u8: every push of the bank Pipe is one
           all-Cross launch and one banked launch, every push of a one-row Pipe its tuner's Cross and One runs
Every figure is a host clock around `reps` pushes and the flush that ends them (the work ends in a synchronise and every block is
popped into numpy arrays on both sides, with pop_rows on both), after a warm-up of the same shape; reps are chosen for windows of
about 0.05 s.  Both sides run with the defaults a caller gets (slots, adaptive submission).  The table gives median (min .. max) in
us PER PUSH of all K channels over the rounds.  The comparison is against the K one-row Pipes of the same build, never against the
bank Pipe itself.  Reading rule (the project's): for K >= 2 the bank Pipe is ahead when its SLOWEST round is below the K Pipes'
FASTEST; at K = 1 the two are level when their medians differ by no more than the larger spread.  Points that miss the rule are
marked and listed at the end; no threshold is fixed and nothing in the library is switched on the outcome.  The last column is the
output volume of a push: K = 32 at factor 8 returns 32 bytes per 2 bytes of u8 input, and the return crossing is what large pushes
are expected to cost.  A missing GPU is an error.

--i16: ONE int16 bank Pipe (sdrhip_pipe_tuner_bank_i16, 4 bytes per sample over the link) against ONE cfloat bank Pipe and against K
one-row cfloat Pipes, both fed floats converted BEFORE the clock starts (the u8 leg's convention); K = 2, 8, 32 x pushes of 1, 16 and
128 blocks, memcpy and buffer pushes, the three legs alternating.  This leg is reported; no rule depends on it."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import sdr_amd.lib as L
import signals as S

B = 8192
BLOCK_OUT = 1024
CHANNELS = (1, 2, 8, 12, 32)
PUSH_BLOCKS = (1, 16, 128)
RAGGED_CHANNELS = (2, 8, 32)
WINDOW_S = 0.05
TAPS = S.taps_decim127()
_f32p, _u8p, _i16p = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int16)
I16_CHANNELS = (2, 8, 32)


def tables(K):
    """K channels on a raster of 1/64 of the sampling frequency around the centre (the centre itself: the table {1, 0})"""
    return [L.tuner_shift_table((j - K // 2) % 64, 64) if j != K // 2 else np.array([1.0, 0.0], np.float32) for j in range(K)]


def bank_pipe(K, u8, i16=False):
    return [L.Pipe.tuner_bank(L.TunerBank(8, TAPS, tables(K)), BLOCK_OUT, input_u8=u8, input_i16=i16)]


def tuner_pipes(K):
    return [L.Pipe.tuner(L.Tuner(8, TAPS, t), BLOCK_OUT) for t in tables(K)]


def push_ptr(p, arr):
    """one push of a contiguous array of the pipe's input type; every ready block of every row popped at once"""
    if p.input_i16:
        ready = L.check(L.lib.sdrhip_pipe_push_i16(p.h, arr.ctypes.data_as(_i16p), arr.size // 2), "sdrhip_pipe_push_i16")
    elif p.input_u8:
        ready = L.check(L.lib.sdrhip_pipe_push_u8(p.h, arr.ctypes.data_as(_u8p), arr.size // 2), "sdrhip_pipe_push_u8")
    else:
        ready = L.check(L.lib.sdrhip_pipe_push(p.h, arr.ctypes.data_as(_f32p), arr.size // 2), "sdrhip_pipe_push")
    return [p.pop_rows(ready)] if ready > 0 else []


def flush(p):
    ready = L.check(L.lib.sdrhip_pipe_flush(p.h), "sdrhip_pipe_flush")
    return [p.pop_rows(ready)] if ready > 0 else []


def leg(pipes, chunks, how):
    """-> function(reps): reps pushes (cycling through `chunks`) into every pipe, then the flush; returns what each pipe popped"""
    def run(reps):
        got = [[] for _ in pipes]
        for r in range(reps):
            chunk = chunks[r % len(chunks)]
            if how == "memcpy":
                for g, p in zip(got, pipes):
                    g += push_ptr(p, chunk)
            else:
                first = None
                for g, p in zip(got, pipes):
                    view = p.input_buffer(chunk.size // 2)
                    if first is None:
                        first = view
                        view[:] = chunk                 # the source writes this one
                    else:
                        view[:] = first                 # ... and the caller copies it into every other pipe's buffer
                    g += push_ptr(p, view)
        for g, p in zip(got, pipes):
            g += flush(p)
        return got
    return run


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def measure(fns, rounds, multiple=1):
    """fns: {name: function(reps)} -> {name: [us per push, one per round]}, the legs alternating within each round"""
    reps = {}
    for name, fn in fns.items():
        fn(8 if multiple == 1 else multiple)                # warm-up of this shape: code objects, tables, staging buffers
        per = timed(fn, 16 if multiple == 1 else 2 * multiple) * 1e-6
        reps[name] = max(8, min(4000, int(WINDOW_S / per))) // multiple * multiple or multiple
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, reps[name]))
    return times


def fmt(v):
    return f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"


def rows_of(got, K):
    """what leg() returned as [K, floats]: one bank pipe's rows, or K one-row pipes' blocks"""
    if len(got) == 1 and K > 1:
        return np.concatenate([g.reshape(K, -1) for g in got[0]], axis=1) if got[0] else np.zeros((K, 0), np.float32)
    return np.stack([np.concatenate([g.reshape(-1) for g in one]) if one else np.zeros(0, np.float32) for one in got])


def same_rows(K, u8, chunks_bank, chunks_f32, what):
    """the two sides compute the same rows (tests/test_gpu_pipe_tuner_bank.py holds the Pipe to it; here: that they time the same work)"""
    reps = max(4, len(chunks_bank))
    a = rows_of(leg(bank_pipe(K, u8), chunks_bank, "memcpy")(reps), K)
    b = rows_of(leg(tuner_pipes(K), chunks_f32, "memcpy")(reps), K)
    if a.shape != b.shape or not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        sys.exit(f"tuner_bank_pipe_bench: the bank Pipe and the K Pipes differ ({what}, K {K})")


def verdict(K, t, name="bank", other="pipes"):
    mb, ms = statistics.median(t[name]), statistics.median(t[other])
    if K == 1:
        ok = abs(mb - ms) <= max(max(v) - min(v) for v in t.values())
        return ok, "level within the spread" if ok else "NOT level within the spread"
    ok = max(t[name]) < min(t[other])
    return ok, "ahead by more than the spread" if ok else "NOT ahead by more than the spread"


def main_i16(a):
    rng = np.random.default_rng(16)
    i16_all = rng.integers(-32768, 32768, 2 * 128 * B, dtype=np.int64).astype(np.int16)
    f32_all = i16_all.astype(np.float32) * np.float32(2.0 ** -11)                         # converted before any clock starts
    lines = [f"# {L.device_name()}; {a.rounds} rounds; ONE int16 bank Pipe, ONE cfloat bank Pipe and K one-row cfloat Pipes alternating (the "
             "cfloat sides fed floats converted outside the clock); host clock around push ... flush, us PER PUSH (all K channels): "
             "median (min .. max); 128 taps / 8, block_size_out 1024"]
    print(lines[0], flush=True)
    for nblk in PUSH_BLOCKS:
        cf = [np.ascontiguousarray(f32_all[:2 * nblk * B])]
        ci = [np.ascontiguousarray(i16_all[:2 * nblk * B])]
        for K in I16_CHANNELS:
            reps = 4
            ra = rows_of(leg(bank_pipe(K, False, True), ci, "memcpy")(reps), K)
            rb = rows_of(leg(tuner_pipes(K), cf, "memcpy")(reps), K)
            if ra.shape != rb.shape or not np.array_equal(ra.view(np.uint32), rb.view(np.uint32)):
                sys.exit(f"tuner_bank_pipe_bench: the int16 bank Pipe and the K Pipes differ ({nblk} blocks per push, K {K})")
            for how in ("memcpy", "buffer"):
                b16, bcf, pipes = bank_pipe(K, False, True), bank_pipe(K, False), tuner_pipes(K)
                i0, b0 = L.tuner_i16_launches(), L.tuner_bank_launches()
                t = measure({"i16 bank": leg(b16, ci, how), "cf32 bank": leg(bcf, cf, how), "pipes": leg(pipes, cf, how)}, a.rounds)
                ni, nb = L.tuner_i16_launches() - i0, L.tuner_bank_launches() - b0
                m = {k: statistics.median(v) for k, v in t.items()}
                vs_cf = "ahead" if max(t["i16 bank"]) < min(t["cf32 bank"]) else "BEHIND" if min(t["i16 bank"]) > max(t["cf32 bank"]) else "within the spread"
                vs_p = "ahead" if max(t["i16 bank"]) < min(t["pipes"]) else "BEHIND" if min(t["i16 bank"]) > max(t["pipes"]) else "within the spread"
                line = (f"i16 {nblk:3d} blocks per push  {how:6s}  K {K:2d}   i16 bank {fmt(t['i16 bank'])}   cf32 bank {fmt(t['cf32 bank'])}   "
                        f"pipes {fmt(t['pipes'])}   i16 / cf32 bank {m['i16 bank'] / m['cf32 bank']:.3f} {vs_cf}   i16 bank / pipes "
                        f"{m['i16 bank'] / m['pipes']:.3f} {vs_p}   [launches: int16 tile kernel {ni}, banked (both banks) {nb}; "
                        f"{K * nblk * B // 8 * 8 / 1024:.0f} KiB out per push]")
                print(line, flush=True)
                lines.append(line)
                del b16, bcf, pipes
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--i16", action="store_true", help="the int16 bank Pipe's leg instead of the cfloat / u8 sweep")
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("tuner_bank_pipe_bench: no HIP device")
    if a.i16:
        return main_i16(a)
    u8_all = S.iq_u8(128 * B)
    f32_all = ((u8_all.astype(np.float32) - np.float32(128.0)) * np.float32(1.0 / 128.0))        # converted before any clock starts
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the bank Pipe and K one-row tuner Pipes alternating; host clock around push ... flush, "
             "us PER PUSH (all K channels): median (min .. max); 128 taps / 8, block_size_out 1024"]
    print(lines[0], flush=True)
    missed = []

    def point(label, K, bank, pipes, chunks_bank, chunks_f32, how, out_bytes, multiple=1):
        b0, x0, f0 = L.tuner_bank_launches(), L.tuner_bank_cross_launches(), L.tuner_fused_launches()
        t = measure({"bank": leg(bank, chunks_bank, how), "pipes": leg(pipes, chunks_f32, how)}, a.rounds, multiple)
        nb, nx, nf = L.tuner_bank_launches() - b0, L.tuner_bank_cross_launches() - x0, L.tuner_fused_launches() - f0
        ok, v = verdict(K, t)
        line = (f"{label}  {how:6s}  K {K:2d}   bank {fmt(t['bank'])}   pipes {fmt(t['pipes'])}   bank / pipes "
                f"{statistics.median(t['bank']) / statistics.median(t['pipes']):.3f}   {v}   "
                f"[launches: banked {nb}, cross {nx}, tuners' own {nf}; {out_bytes / 1024:.0f} KiB out per push]")
        print(line, flush=True)
        lines.append(line)
        if not ok:
            missed.append(line)

    for u8 in (False, True):
        kind = "u8    " if u8 else "cfloat"
        for nblk in PUSH_BLOCKS:
            cf = [np.ascontiguousarray(f32_all[:2 * nblk * B])]
            cb = [np.ascontiguousarray(u8_all[:2 * nblk * B])] if u8 else cf
            for K in CHANNELS:
                same_rows(K, u8, cb, cf, f"{kind.strip()}, {nblk} blocks per push")
                for how in ("memcpy", "buffer"):
                    bank, pipes = bank_pipe(K, u8), tuner_pipes(K)
                    point(f"{kind} {nblk:3d} blocks per push", K, bank, pipes, cb, cf, how, K * nblk * B // 8 * 8)
                    del bank, pipes

    lines.append("# ragged pushes: seeded sizes in [256, 24576] samples, odd ones included (mean about 1.5 blocks), memcpy; per push the bank "
                 "Pipe makes one all-Cross launch and one banked launch, a one-row Pipe its tuner's Cross and One runs")
    print(lines[-1], flush=True)
    rng = np.random.default_rng(11)
    sizes = [int(v) for v in rng.integers(256, 3 * B + 1, 24)]
    edges = np.concatenate([[0], np.cumsum(sizes)])
    assert edges[-1] <= 128 * B
    for u8 in (False, True):
        kind = "u8    " if u8 else "cfloat"
        cf = [np.ascontiguousarray(f32_all[2 * a_:2 * b_]) for a_, b_ in zip(edges[:-1], edges[1:])]
        cb = [np.ascontiguousarray(u8_all[2 * a_:2 * b_]) for a_, b_ in zip(edges[:-1], edges[1:])] if u8 else cf
        for K in RAGGED_CHANNELS:
            same_rows(K, u8, cb, cf, f"{kind.strip()}, ragged")
            bank, pipes = bank_pipe(K, u8), tuner_pipes(K)
            point(f"{kind} ragged, {len(sizes)} sizes   ", K, bank, pipes, cb, cf, "memcpy", K * int(np.mean(sizes)) // 8 * 8, multiple=len(sizes))
            del bank, pipes
    lines.append(f"# points that miss the reading rule: {len(missed)}")
    lines += ["#   " + m for m in missed]
    print("\n".join(lines[-1 - len(missed):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
