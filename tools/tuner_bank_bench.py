"""The tuner bank against K tuner objects of the same build, alternating the two in one process.

    python tools/tuner_bank_bench.py [--rounds R] [--out profiles/tuner_bank_bench.txt]
    python tools/tuner_bank_bench.py --i16 [--rounds R] [--out profiles/tuner_i16_bench.txt]

Sweep: K = 1, 2, 4, 8, 12, 32 channels x resident launches of 1 block (8192 samples), 16 blocks, 2^20 and 2^24 samples of the 128-tap
/ 8 shape (contiguous stream), u8 and cfloat input.
  banked   one sdrhip_tuner_bank_run on the banked route (route 1): ONE launch for all K channels
  tuners   K sdrhip_tuner_run calls of K tuner objects on the same stream, each on its default route (the fused tile kernel: K
           launches) -- the only way to get K channels without the bank
Every figure is a host clock around `reps` back-to-back runs that end in ONE device synchronise, after warm-up runs of the same
shape; reps are chosen so that a window lasts about 0.1 s.  The two legs alternate within each round; the table gives the median and
the spread over the rounds, so a ratio can be read against the run-to-run noise.  Both legs are driven through ctypes; the host cost
of one call that launches nothing (an empty output range) is printed, because the K-tuner leg pays it K times per run and the banked
leg once.  Before it is timed, a point's two legs are compared bit for bit.
No number is fixed in advance: the yardstick is the K-tuner loop.  The last lines derive the auto rule per input type with the FM
bank's criterion -- a point is banked where the banked launch's SLOWEST round is below the loop's FASTEST -- as the largest launch
size up to which every measured K >= 2 is banked, and say what K = 1 did.  A missing GPU is an error.

--i16: the same sweep and protocol on 16-bit signed IQ (sdrhip_tuner_bank_run_i16), three legs alternating in each round:
  banked    one sdrhip_tuner_bank_run_i16 on the banked route
  tuners    K sdrhip_tuner_run_i16 calls of K tuner objects (each the int16 tile kernel with one channel)
  convert   what a caller had before the int16 entry points: sdrhip_convert_i16_run into a cfloat buffer, then the cfloat
            sdrhip_tuner_bank_run on its default route
The auto rule for int16 input is read from banked against tuners; banked against convert is reported point by point and no rule
depends on it."""
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
CHANNELS = (1, 2, 4, 8, 12, 32)
SIZES = (("1 block", B), ("16 blocks", 16 * B), ("2^20 samples", 1 << 20), ("2^24 samples", 1 << 24))
WINDOW_S = 0.1


def tables(K):
    """K channels on a raster of 1/64 of the sampling frequency around the centre (the centre itself: the table {1, 0})"""
    return [L.tuner_shift_table((j - K // 2) % 64, 64) if j != K // 2 else [1.0, 0.0] for j in range(K)]


def legs(K, n_samples, u8):
    """-> ({name: function(reps) that runs reps runs of all K channels and synchronises}, outputs per channel, what to keep alive)"""
    taps = S.taps_decim127()
    tabs = tables(K)
    bank = L.TunerBank(8, taps, tabs)
    bank.set_route(L.TunerBank.ROUTE_BANKED)
    tuners = [L.Tuner(8, taps, t) for t in tabs]
    n = (n_samples - 128) // 8 + 1
    if u8:
        d_in = torch.randint(0, 256, (2 * n_samples,), dtype=torch.uint8, device="cuda")
    else:
        d_in = torch.rand(2 * n_samples, dtype=torch.float32, device="cuda") * 2.0 - 1.0
    out = torch.empty(K * 2 * n, dtype=torch.float32, device="cuda")
    pi, po = d_in.data_ptr(), out.data_ptr()
    bank_run = bank.run_u8 if u8 else bank.run
    tuner_runs = [t.run_u8 if u8 else t.run for t in tuners]

    def banked(reps):
        for _ in range(reps):
            bank_run(pi, 0, po, 2 * n, 0, n)
        torch.cuda.synchronize()

    def loop(reps):
        for _ in range(reps):
            for j, run in enumerate(tuner_runs):
                run(pi, 0, po + 8 * j * n, 0, n)
        torch.cuda.synchronize()

    # the two legs compute the same rows (tests/test_gpu_tuner_bank.py holds every route to it; here: that the legs time the same work)
    loop(1)
    ref = out.clone()
    out.zero_()
    banked(1)
    if not torch.equal(out.view(torch.int32), ref.view(torch.int32)):
        sys.exit(f"tuner_bank_bench: banked launch and tuner loop differ at K = {K}, {n_samples} samples, {'u8' if u8 else 'cfloat'}")
    del ref
    return {"banked": banked, "tuners": loop}, n, (bank, tuners, d_in, out)


def legs_i16(K, n_samples):
    taps = S.taps_decim127()
    tabs = tables(K)
    bank = L.TunerBank(8, taps, tabs)
    bank.set_route(L.TunerBank.ROUTE_BANKED)
    bank_cf = L.TunerBank(8, taps, tabs)                     # the cfloat bank as a caller gets it: route auto
    tuners = [L.Tuner(8, taps, t) for t in tabs]
    n = (n_samples - 128) // 8 + 1
    d_in = torch.randint(-32768, 32768, (2 * n_samples,), dtype=torch.int16, device="cuda")
    d_cf = torch.empty(2 * n_samples, dtype=torch.float32, device="cuda")
    out = torch.empty(K * 2 * n, dtype=torch.float32, device="cuda")
    pi, pc, po = d_in.data_ptr(), d_cf.data_ptr(), out.data_ptr()

    def banked(reps):
        for _ in range(reps):
            bank.run_i16(pi, 0, po, 2 * n, 0, n)
        torch.cuda.synchronize()

    def loop(reps):
        for _ in range(reps):
            for j, t in enumerate(tuners):
                t.run_i16(pi, 0, po + 8 * j * n, 0, n)
        torch.cuda.synchronize()

    def convert(reps):
        for _ in range(reps):
            L.check(L.lib.sdrhip_convert_i16_run(None, pi, pc, 2 * n_samples), "sdrhip_convert_i16_run")
            bank_cf.run(pc, 0, po, 2 * n, 0, n)
        torch.cuda.synchronize()

    loop(1)
    ref = out.clone()
    for name, fn in (("banked", banked), ("convert", convert)):
        out.zero_()
        fn(1)
        if not torch.equal(out.view(torch.int32), ref.view(torch.int32)):
            sys.exit(f"tuner_bank_bench: the {name} leg and the tuner loop differ at K = {K}, {n_samples} samples, i16")
    del ref
    return {"banked": banked, "tuners": loop, "convert": convert}, n, (bank, bank_cf, tuners, d_in, d_cf, out)


def main_i16(a):
    lines = [f"# {L.device_name()}; {a.rounds} rounds, int16 IQ input; banked int16 launch, K-tuner loop (run_i16) and convert + cfloat bank "
             "alternating; us per run of ALL K channels: median (min .. max)"]
    print(lines[0], flush=True)
    points = []
    for size_name, n_samples in SIZES:
        for K in CHANNELS:
            fns, n, keep = legs_i16(K, n_samples)
            reps = {}
            for name, fn in fns.items():
                fn(5)
                per = timed(fn, 10) * 1e-6
                reps[name] = max(5, min(20000, int(WINDOW_S / per)))
            i0, f0 = L.tuner_i16_launches(), L.tuner_fused_launches()
            times = {k: [] for k in fns}
            for _ in range(a.rounds):
                for name, fn in fns.items():
                    times[name].append(timed(fn, reps[name]))
            ni = L.tuner_i16_launches() - i0
            assert ni == a.rounds * (reps["banked"] + reps["tuners"] * K), "an int16 leg took another route than the one it is named for"
            med = {k: statistics.median(v) for k, v in times.items()}
            fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
            clear = max(times["banked"]) < min(times["tuners"])
            clear_c = max(times["banked"]) < min(times["convert"])
            behind_c = min(times["banked"]) > max(times["convert"])
            line = (f"i16  {size_name:13s} K {K:2d}  outputs {n:7d} x {K:2d}   banked {fmt(times['banked'])}   tuners {fmt(times['tuners'])}   "
                    f"convert+cf32 {fmt(times['convert'])}   banked / tuners {med['banked'] / med['tuners']:.3f}"
                    f"{'' if clear else ' (not clear of the spread)'}   banked / convert+cf32 {med['banked'] / med['convert']:.3f}"
                    f"{' ahead' if clear_c else ' BEHIND' if behind_c else ' (within the spread)'}")
            print(line, flush=True)
            lines.append(line)
            points.append((n_samples, size_name, K, med["banked"] / med["tuners"], clear, med["banked"] / med["convert"], clear_c))
            del fns, keep
            torch.cuda.empty_cache()
    bound, bound_name = 0, "none"
    for size_name, n_samples in SIZES:
        if not all(c for ns, _, K, _, c, _, _ in points if ns == n_samples and K > 1):
            break
        bound, bound_name = n_samples, size_name
    lost = [(s, K, r) for ns, s, K, r, c, _, _ in points if K > 1 and not c]
    lines.append(f"# i16: every measured K >= 2 is banked (slowest banked round below the loop's fastest) at every launch size up to "
                 f"{bound_name} ({bound} samples)" + ("; points that are not: " + ", ".join(f"{s} K {K} (ratio {r:.3f})" for s, K, r in lost)
                                                      if lost else ": the whole sweep, the bound is its end, not a crossover"))
    lines.append("# i16: K = 1 (the same kernel with one channel either way) banked / tuners "
                 + ", ".join(f"{s} {r:.3f}{' clear' if c else ''}" for ns, s, K, r, c, _, _ in points if K == 1))
    notc = [(s, K, r) for ns, s, K, _, _, r, c in points if not c]
    lines.append("# i16 against convert + cfloat bank (no rule depends on it): the fused int16 launch is ahead by more than the spread at "
                 f"{sum(1 for p in points if p[6])} of {len(points)} points" + ("; not ahead at: " + ", ".join(f"{s} K {K} (ratio {r:.3f})" for s, K, r in notc)
                                                                                if notc else ""))
    print("\n".join(lines[-3:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def host_call_us(calls=100000):
    """What the host pays for one run call BEFORE the library does any work: the binding's marshalling, the foreign call and the
    library's argument checks.  An empty output range returns there; no GPU work is queued."""
    fns, n, keep = legs(2, B, True)
    bank, tuners, d_in, out = keep
    pi, po = d_in.data_ptr(), out.data_ptr()
    b0, c0 = L.tuner_bank_launches(), L.tuner_fused_launches()
    us = {}
    t0 = time.perf_counter()
    for _ in range(calls):
        tuners[0].run_u8(pi, 0, po, 0, 0)
    us["tuner"] = (time.perf_counter() - t0) / calls * 1e6
    t0 = time.perf_counter()
    for _ in range(calls):
        bank.run_u8(pi, 0, po, 2 * n, 0, 0)
    us["bank"] = (time.perf_counter() - t0) / calls * 1e6
    assert (L.tuner_bank_launches(), L.tuner_fused_launches()) == (b0, c0), "an empty run launched a kernel"
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--i16", action="store_true", help="the int16 legs instead of the u8 / cfloat sweep")
    a = ap.parse_args()
    if a.rounds < 7:
        sys.exit("tuner_bank_bench: at least 7 rounds")
    if L.device_count() < 1:
        sys.exit("tuner_bank_bench: no HIP device")
    torch.cuda.set_device(0)
    if a.i16:
        return main_i16(a)
    call_us = host_call_us()
    lines = [f"# {L.device_name()}; {a.rounds} rounds, banked launch and K-tuner loop alternating; us per run of ALL K channels: median (min .. max)",
             f"# host time of one call that launches nothing (k_end = k_begin): Tuner.run_u8 {call_us['tuner']:.2f} us, "
             f"TunerBank.run_u8 {call_us['bank']:.2f} us (the loop makes K such calls per run, the bank one)"]
    print("\n".join(lines), flush=True)
    points = []
    for u8 in (True, False):
        kind = "u8" if u8 else "cf32"
        for size_name, n_samples in SIZES:
            for K in CHANNELS:
                fns, n, keep = legs(K, n_samples, u8)
                reps = {}
                for name, fn in fns.items():
                    fn(5)                                            # warm-up of this shape: code objects, table uploads, kernel attributes
                    per = timed(fn, 10) * 1e-6
                    reps[name] = max(5, min(20000, int(WINDOW_S / per)))
                b0, c0 = L.tuner_bank_launches(), L.tuner_fused_launches()
                times = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for name, fn in fns.items():
                        times[name].append(timed(fn, reps[name]))
                nb, nc = L.tuner_bank_launches() - b0, L.tuner_fused_launches() - c0
                assert nb == a.rounds * reps["banked"] and nc == a.rounds * reps["tuners"] * K, "a leg took another route than the one it is named for"
                med = {k: statistics.median(v) for k, v in times.items()}
                fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
                # ahead by more than the spread: the banked leg's slowest round against the loop's fastest
                clear = max(times["banked"]) < min(times["tuners"])
                line = (f"{kind:4s} {size_name:13s} K {K:2d}  outputs {n:7d} x {K:2d}   banked {fmt(times['banked'])}   tuners {fmt(times['tuners'])}   "
                        f"banked / tuners {med['banked'] / med['tuners']:.3f}{'' if clear else '   (not clear of the spread)'}")
                print(line, flush=True)
                lines.append(line)
                points.append((kind, n_samples, size_name, K, med["banked"] / med["tuners"], clear))
                del fns, keep
                torch.cuda.empty_cache()
    for kind in ("u8", "cf32"):
        mine = [p for p in points if p[0] == kind]
        bound, bound_name = 0, "none"
        for size_name, n_samples in SIZES:
            if not all(c for _, ns, _, K, _, c in mine if ns == n_samples and K > 1):
                break
            bound, bound_name = n_samples, size_name
        lost = [(s, K, r) for _, ns, s, K, r, c in mine if K > 1 and not c]
        one = [(s, r, c) for _, ns, s, K, r, c in mine if K == 1]
        lines.append(f"# {kind}: every measured K >= 2 is banked (slowest banked round below the loop's fastest) at every launch size up to "
                     f"{bound_name} ({bound} samples)" + ("; points that are not: " + ", ".join(f"{s} K {K} (ratio {r:.3f})" for s, K, r in lost)
                                                          if lost else ": the whole sweep, the bound is its end, not a crossover"))
        lines.append(f"# {kind}: K = 1 (one launch either way) banked / tuners " + ", ".join(f"{s} {r:.3f}{' clear' if c else ''}" for s, r, c in one)
                     + ": auto sends one channel to its tuner")
    print("\n".join(lines[-4:]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
