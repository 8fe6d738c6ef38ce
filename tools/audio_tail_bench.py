"""The audio tail over rows (sdrhip_audio_tail_run_rows) on route 1 (the fused kernel, one launch) against route 2 (the composition:
resampler rows, filter rows, scale -- the row forms' banked launch sets) of the same build, alternating the two in one process.

    python tools/audio_tail_bench.py [--rounds R] [--out profiles/audio_tail_bench.txt]

Sweep: K = 1, 2, 8, 32 rows x 153 (one 8192-sample push decimated by 16), 2458, 39322 and 314574 audio outputs per row, with
block 0 (a contiguous stream) and block 8192 (every Pipe's block: seams of both stages inside every range beyond the first), on the
FM tail: 3/10 resampler of 191 taps, 2 x 64 symmetric audio taps, gain 0.5.  Every run computes outputs [0, n) of each row from
rows that hold exactly their receptive field, in three row layouts:
  rows      y rows and audio rows back to back (y_stride = n_y, audio_stride = n), the buffers 256-byte aligned
  y-strided the audio Pipes' layout: the y rows in a padded rows buffer (y_stride = n_y + n_y / 4 + 513, odd, the first row 4 bytes
            past a 16-byte boundary, so that the rows meet the 4-, 8- and 16-byte loaders), the audio rows back to back
  a-strided the same y rows, and the audio rows n + 5 floats apart (route 2 then scales row by row)
Every figure is a host clock around `reps` back-to-back runs that end in ONE device synchronise, after warm-up runs of the same
shape; reps are chosen so that a window lasts about 0.05 s.  The two routes alternate within each round; the table gives the median
and the spread over the rounds.  Both routes are driven through ctypes on resident tensors.  Before it is timed, a point's two routes
are compared bit for bit.
No number is fixed in advance: the yardstick is route 2.  A point is "ahead" by the project's criterion: route 1's SLOWEST round is
below route 2's FASTEST.  The last lines say where that holds: that table is the auto rule of sdr_hip.h.  A missing GPU is an
error."""
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
SIZES = (153, 2458, 39322, 314574)
BLOCKS = (0, 8192)
WINDOW_S = 0.05


def legs(tail, K, n, layout):
    """-> ({route: function(reps) that makes reps runs over all K rows and synchronises}, what to keep alive)"""
    n_y = 0
    while tail.ready(n_y) < n:
        n_y += max(1, (n - tail.ready(n_y)) * 10 // 3)
    while tail.ready(n_y - 1) >= n:
        n_y -= 1
    g = torch.Generator(device="cuda").manual_seed(4321 + K)
    ys = n_y if layout == "rows" else n_y + n_y // 4 + 513
    os_ = n + 5 if layout == "a-strided" else n
    off = 0 if layout == "rows" else 1
    ybuf = torch.rand(off + K * ys, generator=g, dtype=torch.float32, device="cuda") * 2 - 1
    y = ybuf[off:].as_strided((K, n_y), (ys, 1))
    obuf = {r: torch.zeros(K * os_, dtype=torch.float32, device="cuda") for r in (1, 2)}
    out = {r: obuf[r].as_strided((K, n), (os_, 1)) for r in (1, 2)}
    ws = torch.empty(tail.workspace_bytes(K, n_y), dtype=torch.uint8, device="cuda")
    run, h = L.lib.sdrhip_audio_tail_run_rows, tail.h

    def leg(route):
        po = out[route].data_ptr()

        def fn(reps):
            tail.set_route(route)
            for _ in range(reps):
                rc = run(h, None, y.data_ptr(), ys, 0, n_y, po, os_, K, 0, n, ws.data_ptr(), ws.numel())
                if rc != 0:
                    sys.exit(f"audio_tail_bench: route {route} failed: {L.lib.sdrhip_last_error().decode()}")
            torch.cuda.synchronize()
        return fn
    fns = {1: leg(1), 2: leg(2)}
    fns[1](1)
    fns[2](1)
    if not torch.equal(out[1].contiguous().view(torch.int32), out[2].contiguous().view(torch.int32)):
        sys.exit(f"audio_tail_bench: the two routes differ: K = {K}, n = {n}, block {tail.block}, layout {layout}")
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
        sys.exit("audio_tail_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("audio_tail_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, route 1 (fused, tile of 2046 outputs) and route 2 (composed) alternating; us per run over ALL K rows: median (min .. max)",
             "# FM tail: real AVX resampler 3/10, 191 taps; real symmetric AVX filter, 2 x 64 taps; gain 0.5; n = audio outputs per row"]
    print("\n".join(lines), flush=True)
    points = []
    for layout in LAYOUTS:
        for block in BLOCKS:
            tail = L.AudioTail(3, 10, S.taps_resamp191(), S.taps_audio_half64(), gain=0.5, block=block)
            assert tail.fused_fits()
            for n in SIZES:
                for K in ROWS:
                    fns, keep, n_y = legs(tail, K, n, layout)
                    reps = {}
                    for route, fn in fns.items():
                        fn(3)                                            # warm-up of this shape
                        per = timed(fn, 5) * 1e-6
                        reps[route] = max(3, min(20000, int(WINDOW_S / per)))
                    c0 = (L.audio_tail_launches(), L.fir_rows_launches())
                    times = {k: [] for k in fns}
                    for _ in range(a.rounds):
                        for route, fn in fns.items():
                            times[route].append(timed(fn, reps[route]))
                    fused, banked = L.audio_tail_launches() - c0[0], L.fir_rows_launches() - c0[1]
                    assert fused == a.rounds * reps[1] and banked == 2 * a.rounds * reps[2], "a leg took another route than it was set to"
                    fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                    clear = max(times[1]) < min(times[2])
                    ratio = statistics.median(times[1]) / statistics.median(times[2])
                    line = (f"{layout:9s} block {block:4d} n {n:6d} K {K:2d}  y per row {n_y:7d}  fused {fmt(times[1])}   composed {fmt(times[2])}   "
                            f"fused / composed {ratio:.3f}{'' if clear else '   (not ahead: slowest fused round against fastest composed round)'}")
                    print(line, flush=True)
                    lines.append(line)
                    points.append((layout, block, n, K, clear))
                    del fns, keep
                    torch.cuda.empty_cache()
    for layout in LAYOUTS:
        for block in BLOCKS:
            mine = [p for p in points if p[0] == layout and p[1] == block]
            lines.append(f"# {layout}, block {block}: fused ahead at " + "; ".join(f"n {n}: K {[K for _, _, n2, K, c in mine if n2 == n and c] or 'none'}" for n in SIZES))
    lines.append("# not measured: other blocks, other strides and offsets than the three layouts', more than 32 rows, fewer than 153 or more than 314574 "
                 "outputs per row, a tile of another size, the Pipes' rate")
    print("\n".join(lines[-7:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
