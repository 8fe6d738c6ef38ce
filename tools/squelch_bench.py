"""Squelch: its two routes against each other, the rows call against K one-row calls, and a device-to-device copy of the same signal
bytes as a yardstick, alternating in one process.

    python tools/squelch_bench.py [--rounds R] [--out profiles/squelch_bench.txt]

Sweep: K = 1 / 2 / 8 / 32 rows x 1024 / 16384 / 2^17 / 2^20 signal samples a row x blocks of 256 and 1024 signal samples, for
  self  the signal row is its own (real) detector, block_det = block_sig, out of place
  cplx  a complex detector row of its own with block_det = 4 * block_sig (a carrier squelch in front of a decimator by 4)
Noise at level 1 with thresholds around its mean power and a hang of 2, so that the gate opens and shuts; workspace given; levels and
gates not asked for.  Legs of a point:
  WG, LS  the rows call with the route forced
  calls   K one-row calls (sdrhip_squelch_run, auto route), one row after the other on the same stream
  copy    sdrhip_memcpy_d2d of the K rows' signal bytes: what moving the bytes once costs; a ratio, not a pass mark
Every figure is a host clock around `reps` back-to-back calls that end in ONE device synchronise, after warm-up runs of the same shape;
reps are chosen so that a window lasts about 0.05 s.  The legs of a point alternate within each round; the table gives the median and
the spread over the rounds.  Before it is timed, a point's squelch legs are compared bit for bit, final states included.
A leg is "ahead" of another by the project's criterion: its SLOWEST round is below the other's FASTEST.  A missing GPU is an error."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import sdr_amd.lib as L

WINDOW_S = 0.05
WG, LS = 1, 2
NAMES = {0: "auto", WG: "WG", LS: "LS"}
HANG = 2
lib = L.lib


class Shape:
    def __init__(self, K, n, block, cplx):
        g = torch.Generator(device="cuda").manual_seed(8765 + K)
        self.K, self.n, self.bs, self.cplx = K, n, block, cplx
        self.nb = n // block
        self.bd = 4 * block if cplx else block
        self.sig = torch.randn((K, n), generator=g, dtype=torch.float32, device="cuda")
        self.det = torch.randn((K, 2 * 4 * n), generator=g, dtype=torch.float32, device="cuda") if cplx else self.sig
        self.det_stride = self.det.shape[1]
        # mean power 1 (real) or 2 (complex); blocks scatter around it
        self.open, self.close = (2.05, 1.95) if cplx else (1.03, 0.97)
        self.wsb, self.wsb1 = lib.sdrhip_squelch_rows_workspace_bytes(K, self.nb), lib.sdrhip_squelch_rows_workspace_bytes(1, self.nb)
        self.ws = torch.empty(max(self.wsb, self.wsb1), dtype=torch.uint8, device="cuda")
        self.st = torch.zeros((K, 2), dtype=torch.int32, device="cuda")
        self.outs = {}

    def buf(self, leg):
        if leg not in self.outs:
            self.outs[leg] = (torch.zeros((self.K, self.n), dtype=torch.float32, device="cuda"), torch.zeros((self.K, 2), dtype=torch.int32, device="cuda"))
        return self.outs[leg]

    def rows(self, leg, route):
        y, f = self.buf(leg)
        a = (None, self.det.data_ptr(), self.det_stride, int(self.cplx), self.bd, self.sig.data_ptr(), self.n, y.data_ptr(), self.n, self.bs, self.K,
             self.nb, self.open, self.close, HANG, 1, self.st.data_ptr(), f.data_ptr(), None, None, self.ws.data_ptr(), self.wsb)

        def run(reps):
            L.set_squelch_route(route)
            for _ in range(reps):
                rc = lib.sdrhip_squelch_run_rows(*a)
            L.set_squelch_route(0)
            torch.cuda.synchronize()
            assert rc == 0, lib.sdrhip_last_error()
        return run

    def calls(self, leg):
        y, f = self.buf(leg)
        pd, ps, py, pf, pw = self.det.data_ptr(), self.sig.data_ptr(), y.data_ptr(), f.data_ptr(), self.ws.data_ptr()

        def run(reps):
            for _ in range(reps):
                for r in range(self.K):
                    rc = lib.sdrhip_squelch_run(None, pd + 4 * r * self.det_stride, int(self.cplx), self.bd, ps + 4 * r * self.n, py + 4 * r * self.n,
                                                self.bs, self.nb, self.open, self.close, HANG, 1, 0, 0, pf + 8 * r, None, None, pw, self.wsb1)
            torch.cuda.synchronize()
            assert rc == 0, lib.sdrhip_last_error()
        return run

    def copy(self, leg):
        y, _ = self.buf(leg)
        a = (y.data_ptr(), self.sig.data_ptr(), 4 * self.K * self.n, None)

        def run(reps):
            for _ in range(reps):
                lib.sdrhip_memcpy_d2d(*a)
            torch.cuda.synchronize()
        return run

    def same(self, a, b):
        (ya, fa), (yb, fb) = self.outs[a], self.outs[b]
        return torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and torch.equal(fa, fb)

    def open_share(self, leg):
        return float((self.outs[leg][0] != 0).float().mean())


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def measure(legs, rounds):
    reps = {}
    for name, fn in legs.items():
        fn(3)
        reps[name] = max(3, min(20000, int(WINDOW_S / (timed(fn, 5) * 1e-6))))
    times = {k: [] for k in legs}
    for _ in range(rounds):
        for name, fn in legs.items():
            times[name].append(timed(fn, reps[name]))
    return times


def fmt(v):
    return f"{statistics.median(v):8.1f} ({min(v):.1f} .. {max(v):.1f})"


def ahead(a, b):
    return max(a) < min(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("squelch_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("squelch_bench: no HIP device")
    torch.cuda.set_device(0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {L.device_name()}; {a.rounds} rounds, the legs of a point alternating; us per call (calls: per call set over ALL K rows): median (min .. max)")
    say(f"# noise at level 1, thresholds around its mean power, hang {HANG}, workspace given, levels and gates not asked for")
    say("# auto = the route the auto rule takes with a workspace; verdict = WG against LS by the criterion; rows = auto's route against K one-row calls")
    points = []
    for kind in ("self", "cplx"):
        for size_name, n in (("1024", 1024), ("16384", 16384), ("2^17", 1 << 17), ("2^20", 1 << 20)):
            for block in (256, 1024):
                for K in (1, 2, 8, 32):
                    s = Shape(K, n, block, kind == "cplx")
                    legs = {"WG": s.rows("WG", WG), "LS": s.rows("LS", LS), "calls": s.calls("calls"), "copy": s.copy("copy")}
                    for k in ("WG", "LS", "calls"):
                        legs[k](1)
                    if not (s.same("WG", "LS") and s.same("WG", "calls")):
                        sys.exit(f"squelch_bench: the legs differ: {kind}, K = {K}, n = {n}, block = {block}")
                    share = s.open_share("WG")
                    t = measure(legs, a.rounds)
                    auto = L.squelch_plan(K, s.nb, s.bd, s.cplx, s.bs, True)[1]
                    verdict = "WG ahead" if ahead(t["WG"], t["LS"]) else "LS ahead" if ahead(t["LS"], t["WG"]) else "neither ahead"
                    rows_t = t[NAMES[auto]]
                    say(f"{kind} n {size_name:6s} block {block:4d} ({s.nb:4d} blocks) K {K:2d}  open {share:.2f}  WG {fmt(t['WG'])}   LS {fmt(t['LS'])}   WG / LS "
                        f"{statistics.median(t['WG']) / statistics.median(t['LS']):6.3f}  {verdict:13s}  auto {NAMES[auto]}   calls {fmt(t['calls'])}   rows / calls "
                        f"{statistics.median(rows_t) / statistics.median(t['calls']):.3f}{'' if ahead(rows_t, t['calls']) or K == 1 else ' (rows not ahead)'}"
                        f"   copy {fmt(t['copy'])}   rows / copy {statistics.median(rows_t) / statistics.median(t['copy']):.2f}")
                    points.append((kind, n, block, K, auto, verdict))
                    del s, legs
                    torch.cuda.empty_cache()
    against = [p for p in points if (p[4] == WG and p[5] == "LS ahead") or (p[4] == LS and p[5] == "WG ahead")]
    say("# points where the other route is ahead of the one the auto rule takes: " +
        ("none" if not against else "; ".join(f"{k} n {n} block {b} K {K} (auto {NAMES[r]}, {v})" for k, n, b, K, r, v in against)))
    for r in (WG, LS):
        mine = [p for p in points if p[4] == r]
        say(f"# auto takes {NAMES[r]} at {len(mine)} points: {sum(p[5] == NAMES[r] + ' ahead' for p in mine)} with it ahead, "
            f"{sum(p[5] == 'neither ahead' for p in mine)} with neither ahead")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
