"""The receiver bank against K tuned chain objects of the same build, alternating the two in one process.

    python tools/fm_bank_bench.py [--rounds R] [--out profiles/fm_bank_bench.txt]

Sweep: K = 1, 2, 4, 8, 16, 32 stations x resident runs of 1 source block, 16 source blocks and 2^20 samples (plus the chain's halo).
  banked   one sdrhip_fm_bank_run on the banked route (route 1): ONE launch for all K stations
  chains   K sdrhip_fm_chain_run calls of K tuned chain objects on the same stream, each in its default mode -- the code path a
           receiver of K stations takes without the bank (at these sizes: K launches of the tuned one-kernel chain)
Every figure is a host clock around `reps` back-to-back pushes that end in ONE device synchronise, after warm-up pushes of the
same shape; reps are chosen so that a window lasts about 0.15 s.  The two legs alternate within each round; the table gives the
median and the spread over the rounds, so a ratio can be read against the run-to-run noise.  Both legs are driven through ctypes
and the binding's argument marshalling: the host cost of one such call is measured on FmChain.run / FmBank.run themselves with an
EMPTY output range (q1 = q0: the same ten or eleven arguments, and the library returns before any device work) and printed,
because the K-chain leg pays it K times per push and the banked leg once -- that is part of what K calls cost a Python caller,
and a C caller pays less of it.
No number is fixed in advance: the yardstick is the K-chain loop.  The last lines derive the auto rule, which has two dimensions
because the sweep is a rectangle (stations x outputs per station): the largest total, stations * outputs, below which EVERY
measured point has the banked launch ahead of the loop by more than the spread, and the longest run per station the sweep holds --
sdrhip_fm_bank_run takes the banked launch on its own inside both, and nothing outside the rectangle is measured.  A missing GPU
is an error.

    python tools/fm_bank_bench.py --i16 [--rounds R] [--out profiles/fm_bank_i16_bench.txt]

The same sweep on 16-bit signed IQ (sdrhip_fm_bank_run_i16), three legs alternating in one process:
  banked   one FmBank.run_i16 on the banked route (route 1): ONE launch for all K stations
  route 2  the same bank station by station (route 2): per station the tuner's int16 first stage, then the stage kernels
  rows     what a caller could do without the int16 bank: TunerBank.run_i16 -> fm_demod_rows -> Resampler.run_rows ->
           Filter.run_rows -> sdrhip_scale_run, every stage one launch set for all K rows
Leg A (banked against route 2) decides the bank's auto rule for int16 input by the project's criterion: at a point with K >= 2 the
banked launch's slowest round is below route 2's fastest.  K = 1 and leg B (banked against rows) are reported; no rule depends
on them."""
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

B = 8192
STATIONS = (1, 2, 4, 8, 16, 32)
SIZES = (("1 block", B), ("16 blocks", 16 * B), ("2^20 samples", 1 << 20))
WINDOW_S = 0.15


def tables(K):
    """K stations on a raster of 1/64 of the sampling frequency around the centre (the centre itself: the table {1, 0})"""
    return [L.tuner_shift_table((j - K // 2) % 64, 64) if j != K // 2 else [1.0, 0.0] for j in range(K)]


def legs(K, n_samples):
    """-> ({name: function(reps) that runs reps pushes and synchronises}, outputs per station)"""
    args = (8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64())
    tabs = tables(K)
    bank = L.FmBank(*args, tabs, 0.2, B)
    bank.set_route(L.FmBank.ROUTE_BANKED)
    chains = []
    for t in tabs:
        ch = L.FmChain(*args, 0.2, B)
        ch.set_tuner(t)
        chains.append(ch)
    n_in = n_samples + chains[0].halo_samples()
    q0, q1, _ = bank.plan(0, n_samples, -1)
    n = q1 - q0
    d_in = torch.randint(0, 256, (2 * n_in,), dtype=torch.uint8, device="cuda")
    out = torch.empty(K * n, dtype=torch.float32, device="cuda")
    wsb = bank.workspace_bytes(n_in)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    pi, po, pw = d_in.data_ptr(), out.data_ptr(), ws.data_ptr()

    def banked(reps):
        for _ in range(reps):
            bank.run(pi, 0, n_in, po, n, q0, q1, pw, wsb)
        torch.cuda.synchronize()

    def loop(reps):
        for _ in range(reps):
            for j, ch in enumerate(chains):
                ch.run(pi, 0, n_in, po + 4 * j * n, q0, q1, pw, wsb)
        torch.cuda.synchronize()

    # the two legs compute the same audio (tests/test_gpu_fm_bank.py holds every route to it; here: that the legs time the same work)
    loop(1)
    ref = out.clone()
    out.zero_()
    banked(1)
    if not torch.equal(out.view(torch.int32), ref.view(torch.int32)):
        sys.exit(f"fm_bank_bench: banked launch and chain loop differ at K = {K}, {n_samples} samples")
    return {"banked": banked, "chains": loop}, n, (bank, chains, d_in, out, ws)


def legs_i16(K, n_samples):
    """-> ({name: function(reps)}, outputs per station, what must stay alive)"""
    args = (8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64())
    tabs = tables(K)
    banks = {}
    for name, route in (("banked", L.FmBank.ROUTE_BANKED), ("route 2", L.FmBank.ROUTE_STATIONS)):
        banks[name] = L.FmBank(*args, tabs, 0.2, B)
        banks[name].set_route(route)
    bank = banks["banked"]
    n_in = n_samples + L.FmChain(*args, 0.2, B).halo_samples()
    q0, q1, _ = bank.plan(0, n_samples, -1)
    n = q1 - q0
    d_in = torch.randint(-32768, 32768, (2 * n_in,), dtype=torch.int16, device="cuda")
    out = torch.empty(K * n, dtype=torch.float32, device="cuda")
    wsb = bank.workspace_bytes(n_in)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
    pi, po, pw = d_in.data_ptr(), out.data_ptr(), ws.data_ptr()
    # the row forms over the chain's ranges (chain.cpp's plan_run)
    tb = L.TunerBank(8, S.taps_decim127(), tabs)
    res = L.Resampler(3, 10, S.taps_resamp191())
    filt = L.Filter(S.taps_audio_half64(), sym=True)
    m1 = q1 + filt.num_coeffs - 1
    ky0, ky1 = res.in_offset(q0), res.in_offset(m1 - 1) + 64
    kd0, kd1 = max(ky0 - 1, 0), ky1
    d = torch.empty((K, 2 * (kd1 - kd0)), dtype=torch.float32, device="cuda")
    y = torch.empty((K, ky1 - ky0), dtype=torch.float32, device="cuda")
    z = torch.empty((K, m1 - q0), dtype=torch.float32, device="cuda")
    au = torch.empty((K, n), dtype=torch.float32, device="cuda")
    out_rows = torch.empty(K * n, dtype=torch.float32, device="cuda")

    def run_bank(which):
        def fn(reps):
            for _ in range(reps):
                banks[which].run_i16(pi, 0, n_in, po, n, q0, q1, pw, wsb)
            torch.cuda.synchronize()
        return fn

    def rows(reps):
        cs = torch.cuda.current_stream().cuda_stream
        for _ in range(reps):
            tb.run_i16(pi, 0, d.data_ptr(), d.shape[1], kd0, kd1, B, stream=cs)
            L.fm_demod_rows(d, out=y, in_base=kd0, k_begin=ky0, k_end=ky1)
            res.run_rows(y, z, q0, m1, in_base=ky0, seam_block=B, out_block=B)
            filt.run_rows(z, au, q0, q1, in_base=q0, seam_block=B)
            L.check(L.lib.sdrhip_scale_run(cs, 0.2, au.data_ptr(), out_rows.data_ptr(), K * n), "sdrhip_scale_run")
        torch.cuda.synchronize()

    fns = {"banked": run_bank("banked"), "route 2": run_bank("route 2"), "rows": rows}
    # the three legs compute the same audio (tests/test_gpu_fm_bank_i16.py holds the bank's routes to the hand-driven composition)
    rows(1)
    fns["route 2"](1)
    ref = out.clone()
    if not torch.equal(out_rows.view(torch.int32), ref.view(torch.int32)):
        sys.exit(f"fm_bank_bench: route 2 and the row forms differ at K = {K}, {n_samples} samples")
    out.zero_()
    fns["banked"](1)
    if not torch.equal(out.view(torch.int32), ref.view(torch.int32)):
        sys.exit(f"fm_bank_bench: banked launch and route 2 differ at K = {K}, {n_samples} samples")
    return fns, n, (banks, tb, res, filt, d_in, out, ws, d, y, z, au, out_rows)


def main_i16(a):
    lines = [f"# {L.device_name()}; int16 IQ; {a.rounds} rounds, the three legs alternating; us per run of ALL K stations: median (min .. max)",
             "# leg A: banked (route 1) against route 2 of the same bank; leg B: banked against the row forms a caller could drive by hand"]
    print("\n".join(lines), flush=True)
    fails = []
    for size_name, n_samples in SIZES:
        for K in STATIONS:
            fns, n, keep = legs_i16(K, n_samples)
            reps = {}
            for name, fn in fns.items():
                fn(20)
                per = timed(fn, 50) * 1e-6
                reps[name] = max(50, min(20000, int(WINDOW_S / per)))
            b0, i0 = L.fm_bank_launches(), L.fm_bank_i16_launches()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for name, fn in fns.items():
                    times[name].append(timed(fn, reps[name]))
            nb, ni = L.fm_bank_launches() - b0, L.fm_bank_i16_launches() - i0
            assert nb == ni == a.rounds * reps["banked"], "a leg took another route than the one it is named for"
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda v: f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"
            clear = max(times["banked"]) < min(times["route 2"])
            line = (f"{size_name:13s} K {K:2d}  outputs {n:6d} x {K:2d} = {K * n:8d}   banked {fmt(times['banked'])}   route 2 {fmt(times['route 2'])}   "
                    f"rows {fmt(times['rows'])}   A: banked / route 2 {med['banked'] / med['route 2']:.3f}{'' if clear else ' (not clear of the spread)'}   "
                    f"B: banked / rows {med['banked'] / med['rows']:.3f}")
            print(line, flush=True)
            lines.append(line)
            if K >= 2 and not clear:
                fails.append((size_name, K))
            del fns, keep
            torch.cuda.empty_cache()
    if fails:
        lines.append(f"# leg A: the criterion (K >= 2: the banked launch's slowest round below route 2's fastest) FAILS at {fails}: auto "
                     "must shrink to the part of the rectangle where it holds")
    else:
        lines.append("# leg A: the criterion (K >= 2: the banked launch's slowest round below route 2's fastest) holds on the WHOLE rectangle: "
                     "auto for int16 input is the u8 rule (outputs per station <= 39322, stations * outputs <= 32 * 39322)")
    print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def host_call_us(calls=100000):
    """What the host pays for one run call BEFORE the library does any work: the binding's marshalling of the run's own arguments,
    the foreign call and the library's argument checks.  An empty output range returns there; no GPU work is queued."""
    fns, n, keep = legs(1, B)
    bank, chains, d_in, out, ws = keep
    pi, po, pw = d_in.data_ptr(), out.data_ptr(), ws.data_ptr()
    b0, c0 = L.fm_bank_launches(), L.small_chain_tuned_launches()
    us = {}
    t0 = time.perf_counter()
    for _ in range(calls):
        chains[0].run(pi, 0, d_in.numel() // 2, po, 0, 0, pw, ws.numel())
    us["chain"] = (time.perf_counter() - t0) / calls * 1e6
    t0 = time.perf_counter()
    for _ in range(calls):
        bank.run(pi, 0, d_in.numel() // 2, po, n, 0, 0, pw, ws.numel())
    us["bank"] = (time.perf_counter() - t0) / calls * 1e6
    assert (L.fm_bank_launches(), L.small_chain_tuned_launches()) == (b0, c0), "an empty run launched a kernel"
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--i16", action="store_true", help="the sweep on 16-bit signed IQ: banked against route 2 and against the row forms")
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("fm_bank_bench: no HIP device")
    torch.cuda.set_device(0)
    if a.i16:
        return main_i16(a)
    call_us = host_call_us()
    lines = [f"# {L.device_name()}; {a.rounds} rounds, banked launch and K-chain loop alternating; us per push of ALL K stations: median (min .. max)",
             f"# host time of one call that launches nothing (q1 = q0, the run's own arguments): FmChain.run {call_us['chain']:.2f} us, "
             f"FmBank.run {call_us['bank']:.2f} us (the loop makes K such calls per push, the bank one)"]
    print("\n".join(lines), flush=True)
    points, station_runs = [], []
    for size_name, n_samples in SIZES:
        for K in STATIONS:
            fns, n, keep = legs(K, n_samples)
            reps = {}
            for name, fn in fns.items():
                fn(20)                                           # warm-up of this shape: code objects, table uploads, kernel attributes
                per = timed(fn, 50) * 1e-6
                reps[name] = max(50, min(20000, int(WINDOW_S / per)))
            b0, c0 = L.fm_bank_launches(), L.small_chain_tuned_launches()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for name, fn in fns.items():
                    times[name].append(timed(fn, reps[name]))
            nb, nc = L.fm_bank_launches() - b0, L.small_chain_tuned_launches() - c0
            assert nb == a.rounds * reps["banked"] and nc == a.rounds * reps["chains"] * K, "a leg took another route than the one it is named for"
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda v: f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"
            # ahead by more than the spread: the banked leg's slowest round against the loop's fastest
            clear = max(times["banked"]) < min(times["chains"])
            line = (f"{size_name:13s} K {K:2d}  outputs {n:6d} x {K:2d} = {K * n:8d}   banked {fmt(times['banked'])}   chains {fmt(times['chains'])}   "
                    f"banked / chains {med['banked'] / med['chains']:.3f}{'' if clear else '   (not clear of the spread)'}")
            print(line, flush=True)
            lines.append(line)
            points.append((K * n, K, size_name, med["banked"] / med["chains"], clear))
            station_runs.append((size_name, n))
            del fns, keep
            torch.cuda.empty_cache()
    points.sort()
    wins = 0
    for total, K, size_name, ratio, clear in points:
        if K == 1:
            continue
        if not (ratio < 1.0 and clear):
            break
        wins = total
    losing = [(t, K, s, r) for t, K, s, r, c in points if K > 1 and not (r < 1.0 and c)]
    per_station = max(n for _, n in station_runs)
    lines.append("# K = 1 is one launch either way (the banked kernel against the tuned one-kernel chain): it sets no bound")
    if losing:
        t, K, s, r = losing[0]
        lines.append(f"# bound: the banked launch is ahead at every measured point (K > 1) up to stations * outputs = {wins}; "
                     f"the first point where it is not: {t} (K {K}, {s}, ratio {r:.3f})")
    else:
        margin = [r for t, K, s, r, c in points if t == wins and K > 1][-1]
        lines.append(f"# bound: the banked launch is ahead at EVERY measured point (K > 1), up to stations * outputs = {wins} "
                     f"(banked / chains {margin:.3f} there): the sweep does not reach the crossover, the bound is its end")
    lines.append(f"# the sweep is a rectangle: the longest run per station it holds is {per_station} outputs.  Auto banks a run only inside "
                 f"BOTH bounds (outputs per station <= {per_station}, stations * outputs <= the total above); a longer run per station is "
                 "not measured at any K and goes station by station")
    print("\n".join(lines[-3:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
