"""The audio tail over rows (sdrhip_audio_tail_run_rows) on the general fused kernel (route 0 with sdrhip_audio_tail_set_general(1):
k_audio_tail_rows_any, one launch) against route 2 (the composition: resampler rows, filter rows, scale -- the row forms' banked
launch sets, unchanged code) of the same build, alternating the two in one process.

    python tools/audio_tail_any_bench.py [--rounds R] [--out profiles/audio_tail_any_bench.txt]

Sweep: K = 1, 2, 8, 32 rows x 51 (a 2048-sample push decimated by 32 at 4/5), 204 (one 8192-sample block), 3276 (16 blocks) and
52428 (256 blocks) audio outputs per row, with block 0 (a contiguous stream) and block 256 (the narrow Pipe's block: seams of both
stages inside every range beyond the first), on two tails: 4/5 with 63 taps and 2/5 with 127 taps, each with 2 x 64 symmetric audio
taps and gain 0.5.  Every run computes outputs [0, n) of each row from rows that hold exactly their receptive field, in the three
row layouts of tools/audio_tail_bench.py:
  rows      y rows and audio rows back to back (y_stride = n_y, audio_stride = n), the buffers 256-byte aligned
  y-strided the audio Pipes' layout: the y rows in a padded rows buffer (y_stride = n_y + n_y / 4 + 513, odd, the first row 4 bytes
            past a 16-byte boundary), the audio rows back to back
  a-strided the same y rows, and the audio rows n + 5 floats apart (route 2 then scales row by row)
Every figure is a host clock around `reps` back-to-back runs that end in ONE device synchronise, after warm-up runs of the same
shape; reps are chosen so that a window lasts about 0.05 s.  The two legs alternate within each round; the table gives the median
and the spread over the rounds.  Both legs are driven through ctypes on resident tensors.  Before it is timed, a point's two legs
are compared bit for bit.
No number is fixed in advance: the yardstick is route 2.  A point is "ahead" by the project's criterion: the general kernel's
SLOWEST round is below route 2's FASTEST.  The last lines say where that holds: that table is the mode-0 rule of sdr_hip.h.  A
missing GPU is an error."""
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

ROWS = (1, 2, 8, 32)
LAYOUTS = ("rows", "y-strided", "a-strided")
SIZES = (51, 204, 3276, 52428)
BLOCKS = (0, 256)
SHAPES = ((4, 5, 63), (2, 5, 127))
WINDOW_S = 0.05
GENERAL, COMPOSED = "general", "composed"


def legs(tail, K, n, layout, D, I):
    """-> ({leg: function(reps) that makes reps runs over all K rows and synchronises}, what to keep alive, y per row)"""
    n_y = 0
    while tail.ready(n_y) < n:
        n_y += max(1, (n - tail.ready(n_y)) * D // I)
    while tail.ready(n_y - 1) >= n:
        n_y -= 1
    g = torch.Generator(device="cuda").manual_seed(4321 + K)
    ys = n_y if layout == "rows" else n_y + n_y // 4 + 513
    os_ = n + 5 if layout == "a-strided" else n
    off = 0 if layout == "rows" else 1
    ybuf = torch.rand(off + K * ys, generator=g, dtype=torch.float32, device="cuda") * 2 - 1
    y = ybuf[off:].as_strided((K, n_y), (ys, 1))
    obuf = {r: torch.zeros(K * os_, dtype=torch.float32, device="cuda") for r in (GENERAL, COMPOSED)}
    out = {r: obuf[r].as_strided((K, n), (os_, 1)) for r in (GENERAL, COMPOSED)}
    ws = torch.empty(tail.workspace_bytes(K, n_y), dtype=torch.uint8, device="cuda")
    run, h = L.lib.sdrhip_audio_tail_run_rows, tail.h

    def leg(which):
        po = out[which].data_ptr()

        def fn(reps):
            tail.set_route(0 if which == GENERAL else 2)
            tail.set_general(1 if which == GENERAL else 2)
            for _ in range(reps):
                rc = run(h, None, y.data_ptr(), ys, 0, n_y, po, os_, K, 0, n, ws.data_ptr(), ws.numel())
                if rc != 0:
                    sys.exit(f"audio_tail_any_bench: the {which} leg failed: {L.lib.sdrhip_last_error().decode()}")
            torch.cuda.synchronize()
        return fn
    fns = {GENERAL: leg(GENERAL), COMPOSED: leg(COMPOSED)}
    fns[GENERAL](1)
    fns[COMPOSED](1)
    if not torch.equal(out[GENERAL].contiguous().view(torch.int32), out[COMPOSED].contiguous().view(torch.int32)):
        sys.exit(f"audio_tail_any_bench: the two legs differ: K = {K}, n = {n}, block {tail.block}, layout {layout}")
    return fns, (ybuf, obuf, ws), n_y


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
        sys.exit("audio_tail_any_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("audio_tail_any_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the general kernel (route 0, mode 1; tile of 840 outputs) and route 2 (composed) alternating; "
             "us per run over ALL K rows: median (min .. max)",
             "# tails: real AVX resampler 4/5 x 63 taps and 2/5 x 127 taps; real symmetric AVX filter, 2 x 64 taps; gain 0.5; n = audio outputs per row"]
    print("\n".join(lines), flush=True)
    points = []
    for I, D, ntaps in SHAPES:
        taps = (I * S.windowed_sinc(ntaps, 1.0 / D)).astype("float32")
        for layout in LAYOUTS:
            for block in BLOCKS:
                tail = L.AudioTail(I, D, taps, S.taps_audio_half64(), gain=0.5, block=block)
                assert tail.general_fits() and not tail.fused_fits()
                for n in SIZES:
                    for K in ROWS:
                        fns, keep, n_y = legs(tail, K, n, layout, D, I)
                        reps = {}
                        for which, fn in fns.items():
                            fn(3)                                            # warm-up of this shape
                            per = timed(fn, 5) * 1e-6
                            reps[which] = max(3, min(20000, int(WINDOW_S / per)))
                        c0 = (L.audio_tail_general_launches(), L.audio_tail_launches())
                        times = {k: [] for k in fns}
                        for _ in range(a.rounds):
                            for which, fn in fns.items():
                                times[which].append(timed(fn, reps[which]))
                        general, fused = L.audio_tail_general_launches() - c0[0], L.audio_tail_launches() - c0[1]
                        assert general == a.rounds * reps[GENERAL] and fused == 0, "a leg took another route than it was set to"
                        fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                        clear = max(times[GENERAL]) < min(times[COMPOSED])
                        ratio = statistics.median(times[GENERAL]) / statistics.median(times[COMPOSED])
                        line = (f"{I}/{D} x {ntaps:3d} {layout:9s} block {block:4d} n {n:6d} K {K:2d}  y per row {n_y:7d}  general {fmt(times[GENERAL])}   "
                                f"composed {fmt(times[COMPOSED])}   general / composed {ratio:.3f}"
                                f"{'' if clear else '   (not ahead: slowest general round against fastest composed round)'}")
                        print(line, flush=True)
                        lines.append(line)
                        points.append((f"{I}/{D} x {ntaps}", layout, block, n, K, clear))
                        del fns, keep
                        torch.cuda.empty_cache()
    tail_lines = 1
    for I, D, ntaps in SHAPES:
        for layout in LAYOUTS:
            for block in BLOCKS:
                mine = [p for p in points if p[0] == f"{I}/{D} x {ntaps}" and p[1] == layout and p[2] == block]
                lines.append(f"# {I}/{D} x {ntaps}, {layout}, block {block}: general ahead at "
                             + "; ".join(f"n {n}: K {[K for _, _, _, n2, K, c in mine if n2 == n and c] or 'none'}" for n in SIZES))
                tail_lines += 1
    lines.append("# not measured: other tails, other blocks, other strides and offsets than the three layouts', more than 32 rows, fewer than 51 or more "
                 "than 52428 outputs per row, a tile of another size, the Pipes' rate")
    print("\n".join(lines[-tail_lines:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
