"""De-emphasis: its three routes against each other, the rows call against K one-row calls, and the dcBlocker rows form at the same
shapes as a reference point, alternating in one process.

    python tools/deemph_bench.py [--rounds R] [--out profiles/deemph_bench.txt]

alpha = sdrhip_deemph_alpha(75e-6, 48000) = 0.2425 (default run-in 168), noise at level 0.3, workspace given, default run-in.
  A  the rows call against K one-row calls (sdrhip_deemph_run, one row after the other on the same stream), K = 1 / 2 / 8 / 32,
     n = 1024 / 16384 / 2^20, with sdrhip_dc_blocker_run_rows at the same shape beside them
  B  SEQ against WG (both forced) for n from two run-ins (336) up to 65536, at 1 and 32 rows: the lower edge of WG
  C  WG against LS (both forced) for n = 2^14 .. 2^16, and LS against SEQ for 2^17, 2^18 where WG cannot be forced, at 1 and 32 rows
  D  the slow case: one constant row (2.0, then 0.5 for ever) and one silent-after-noise row of 16384 samples, SEQ against WG
Every figure is a host clock around `reps` back-to-back calls that end in ONE device synchronise, after warm-up runs of the same shape;
reps are chosen so that a window lasts about 0.05 s.  The legs of a point alternate within each round; the table gives the median and
the spread over the rounds.  Before it is timed, a point's de-emphasis legs are compared bit for bit, final states included.
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
SEQ, WG, LS = 1, 2, 3
NAMES = {0: "auto", SEQ: "SEQ", WG: "WG", LS: "LS"}
lib = L.lib


class Shape:
    def __init__(self, K, n, x=None):
        g = torch.Generator(device="cuda").manual_seed(4321 + K)
        self.K, self.n = K, n
        self.x = x if x is not None else torch.randn((K, n), generator=g, dtype=torch.float32, device="cuda") * 0.3
        self.st = torch.zeros(K, dtype=torch.float32, device="cuda")
        self.st2 = torch.zeros((K, 2), dtype=torch.float32, device="cuda")
        self.wsb, self.wsb1 = lib.sdrhip_deemph_rows_workspace_bytes(K, n), lib.sdrhip_deemph_workspace_bytes(n)
        self.dwsb = lib.sdrhip_dc_blocker_rows_workspace_bytes(K, n)
        self.ws = torch.empty(max(self.wsb, self.wsb1, self.dwsb), dtype=torch.uint8, device="cuda")
        self.outs = {}

    def buf(self, leg):
        if leg not in self.outs:
            self.outs[leg] = (torch.empty((self.K, self.n), dtype=torch.float32, device="cuda"), torch.empty((self.K, 2), dtype=torch.float32, device="cuda"))
        return self.outs[leg]

    def rows(self, leg, alpha, route):
        y, f = self.buf(leg)
        a = (None, self.x.data_ptr(), self.n, y.data_ptr(), self.n, self.K, self.n, alpha, self.st.data_ptr(), f.data_ptr(), self.ws.data_ptr(), self.wsb, 0)

        def run(reps):
            L.set_deemph_route(route)
            for _ in range(reps):
                rc = lib.sdrhip_deemph_run_rows(*a)
            L.set_deemph_route(0)
            torch.cuda.synchronize()
            assert rc == 0, lib.sdrhip_last_error()
        return run

    def calls(self, leg, alpha):
        y, f = self.buf(leg)
        px, py, pf, pw, n = self.x.data_ptr(), y.data_ptr(), f.data_ptr(), self.ws.data_ptr(), self.n

        def run(reps):
            for _ in range(reps):
                for r in range(self.K):
                    lib.sdrhip_deemph_run(None, px + 4 * r * n, py + 4 * r * n, n, alpha, 0.0, pf + 4 * r, pw, self.wsb1, 0)
            torch.cuda.synchronize()
        return run

    def dc_rows(self, leg):
        y, f = self.buf(leg)
        a = (None, self.x.data_ptr(), self.n, y.data_ptr(), self.n, self.K, self.n, self.st2.data_ptr(), f.data_ptr(), self.ws.data_ptr(), self.dwsb, 0)

        def run(reps):
            for _ in range(reps):
                lib.sdrhip_dc_blocker_run_rows(*a)
            torch.cuda.synchronize()
        return run

    def same(self, a, b):
        (ya, fa), (yb, fb) = self.outs[a], self.outs[b]
        K = self.K
        return torch.equal(ya.view(torch.int32), yb.view(torch.int32)) and torch.equal(fa.view(torch.int32).flatten()[:K], fb.view(torch.int32).flatten()[:K])


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
    return f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"


def ahead(a, b):
    return max(a) < min(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("deemph_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("deemph_bench: no HIP device")
    torch.cuda.set_device(0)
    alpha = L.deemph_alpha(75e-6, 48000.0)
    W = L.deemph_plan(1, 1 << 20, alpha)[3]
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# {L.device_name()}; {a.rounds} rounds, the legs of a point alternating; us per call (A: per call set over ALL K rows): median (min .. max)")
    say(f"# alpha {alpha:.6f} (75 us at 48 kHz), default run-in {W}, noise at level 0.3, workspace given")
    say("# A: the rows call (auto route) against K one-row calls, and the dcBlocker rows form at the same shape")
    for size_name, n in (("1024", 1024), ("16384", 16384), ("2^20", 1 << 20)):
        for K in (1, 2, 8, 32):
            s = Shape(K, n)
            legs = {"rows": s.rows("rows", alpha, 0), "calls": s.calls("calls", alpha), "dc rows": s.dc_rows("dc")}
            legs["rows"](1), legs["calls"](1)
            if not s.same("rows", "calls"):
                sys.exit(f"deemph_bench: the rows call and the one-row calls differ: K = {K}, n = {n}")
            t = measure(legs, a.rounds)
            chunks, route, _, _ = L.deemph_plan(K, n, alpha)
            dchunks = L.dc_rows_plan(K, n)[0]
            say(f"A n {size_name:6s} K {K:2d}  {NAMES[route]:3s} {chunks:5d} chunks  rows {fmt(t['rows'])}   calls {fmt(t['calls'])}   rows / calls "
                f"{statistics.median(t['rows']) / statistics.median(t['calls']):.3f}{'' if ahead(t['rows'], t['calls']) else '   (rows not ahead)'}"
                f"   | dcBlocker rows ({dchunks if dchunks else 'sequential'}{' chunks' if dchunks else ''}) {fmt(t['dc rows'])}")
            del s, legs
            torch.cuda.empty_cache()

    def versus(tag, K, n, routes, x=None, label=""):
        s = Shape(K, n, x)
        legs = {NAMES[r]: s.rows(NAMES[r], alpha, r) for r in routes}
        for fn in legs.values():
            fn(1)
        names = list(legs)
        for other in names[1:]:
            if not s.same(names[0], other):
                sys.exit(f"deemph_bench: {names[0]} and {other} differ: K = {K}, n = {n} {label}")
        t = measure(legs, a.rounds)
        first, second = names
        verdict = f"{first} ahead" if ahead(t[first], t[second]) else f"{second} ahead" if ahead(t[second], t[first]) else "neither ahead"
        stats = ""
        if WG in routes:
            L.set_deemph_route(WG)
            legs["WG"](1)
            stats = f"   WG statistics {L.rows_stats(s.ws, K)[0]}"
        say(f"{tag} n {n:7d} K {K:2d} {label} " + "   ".join(f"{k} {fmt(v)}" for k, v in t.items()) + f"   {first} / {second} "
            f"{statistics.median(t[first]) / statistics.median(t[second]):.3f}   {verdict}{stats}")
        res = ahead(t[first], t[second])
        del s, legs
        torch.cuda.empty_cache()
        return res

    say(f"# B: WG against SEQ, both forced, from two run-ins ({2 * W}) up to 65536")
    wg_wins = []
    for K in (1, 32):
        for n in (2 * W, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536):
            wg_wins.append((K, n, versus("B", K, n, (WG, SEQ))))
    say("# C: WG against LS, both forced, up to the WG bound; past it (WG cannot be forced there) LS against SEQ")
    ls_pts = []
    for K in (1, 32):
        for n in (1 << 14, 1 << 15, 1 << 16):
            ls_pts.append((K, n, versus("C", K, n, (WG, LS))))
        for n in (1 << 17, 1 << 18):
            versus("C", K, n, (LS, SEQ))
    say("# D: the slow case, 16384 samples, one row: trajectories do not meet on an exactly constant input, every chunk is repaired in turn")
    n = 16384
    const = torch.full((1, n), 0.5, dtype=torch.float32, device="cuda")
    const[0, :37] = 2.0
    silent = torch.zeros((1, n), dtype=torch.float32, device="cuda")
    silent[0, :300] = torch.randn(300, generator=torch.Generator(device="cuda").manual_seed(5), dtype=torch.float32, device="cuda") * 0.3
    versus("D", 1, n, (WG, SEQ), const, "constant          ")
    versus("D", 1, n, (WG, SEQ), silent, "silent-after-noise")
    versus("D", 1, n, (WG, SEQ), None, "noise (for scale) ")
    lost = [(K, n) for K, n, w in wg_wins if not w]
    say("# B: WG ahead of SEQ at " + ("every point from two run-ins up" if not lost else "all points but " + ", ".join(f"K {K} n {n}" for K, n in lost)))
    lost = [(K, n) for K, n, w in ls_pts if not w]
    say("# C: WG ahead of LS at " + ("every point up to its bound" if not lost else "all points but " + ", ".join(f"K {K} n {n}" for K, n in lost)))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
