"""A/B of the two "work the bits do not need" changes to the FM pass (LABNOTES "First multiply-add as one fma; newest-first tiles"):

  first_mac   the first multiply and add of every lane partial as one fma onto +0 (sdr_amd/csrc/first_mac.hpp)
  newest      the fused fmDemod + resampler launch takes its tiles last to first (sdrhip_debug_set_resample_order; measured, not
              kept: tools/lab_variants/resample_newest_first.patch adds it back -- a library without the switch is measured
              oldest-first only)

in ONE process, on the bench's own pass (bench.py: 65536 blocks of 8192 samples, two runs in flight inside the library, and one run
at a time), with up to three builds of the library loaded side by side:

    --parent PATH    libsdr_hip.so of the parent commit (neither change; it has no order switch)
    --unfused PATH   this tree built with -DSDRHIP_FIRST_MAC_UNFUSED (the order switch, multiply and add as two instructions)
    (the product library of this tree is always loaded: first_mac on, order switch)

    python -m sdr_amd.build && python tools/pass_energy_ab.py --parent P/libsdr_hip.so --unfused U/libsdr_hip.so > profiles/pass_energy_ab.txt

--base new: the same alternation with this tree's library as the base and the parent as the only variant -- the other load order
(a library makes its two internal streams at its first two-runs-in-flight run, so which build runs first decides which hardware
queues its streams get; a gain that is real shows in both orders).

Rows alternate  base X1 base X2 base X3 ...  (base = the parent, or the unfused build oldest-first when no parent is given), every
row at least --row-seconds of back-to-back passes, --rounds alternations.  Per row: ms per pass (wall clock over the row), per-stage ms
(HIP events; one-run-at-a-time rows only, as in bench.py), mean socket power and shader clock over the row (tools/power_probe.py: the
hwmon files, read only).  The summary gives the base's own SPREAD -- the standard deviation of its rows, which are rows of one binary
in the same alternation -- and each variant's mean gain against the base's mean; a change "clears the bar" when its gain exceeds
twice that spread in the two-runs-in-flight mode (bench.py's default).  The range (max - min) of the base's rows is printed too.

--order-sweep 2048,8192: afterwards, oldest-first against newest-first on this tree's library at those pass sizes (for the library's
own choice of order).  Run on a GPU box, as one job."""
import argparse
import ctypes as C
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np          # noqa: E402
import torch                # noqa: E402
import sdr_amd.lib as L     # noqa: E402  (maps torch's HIP runtime first: every library below shares it)
import signals as S         # noqa: E402
import power_probe as PP    # noqa: E402

B = 8192
_vp, _i64 = C.c_void_p, C.c_int64
_f32p = C.POINTER(C.c_float)
STAGES = ("decimate", "fm_demod", "resample", "filter", "fused_tail", "fused_chain")


class Build:
    """One libsdr_hip.so and one FM chain made by it (the few entry points a pass needs, bound by hand: sdr_amd.lib binds one library)."""

    def __init__(self, name, path):
        self.name, self.path = name, path
        self.lib = lib = L.lib if os.path.realpath(path) == os.path.realpath(L.LIB_PATH) else C.CDLL(path)
        lib.sdrhip_fm_chain_create.argtypes = [C.POINTER(_vp), C.c_int, C.c_int, _f32p, C.c_int, C.c_int, C.c_int, _f32p, C.c_int, _f32p, C.c_int, C.c_float, _i64]
        lib.sdrhip_fm_chain_destroy.argtypes = [_vp]
        lib.sdrhip_fm_chain_destroy.restype = None
        lib.sdrhip_fm_chain_plan.argtypes = [_vp, _i64, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)]
        lib.sdrhip_fm_chain_workspace_bytes.argtypes = [_vp, _i64]
        lib.sdrhip_fm_chain_workspace_bytes.restype = C.c_size_t
        lib.sdrhip_fm_chain_run.argtypes = [_vp, _vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp, C.c_size_t]
        lib.sdrhip_fm_chain_set_overlap.argtypes = [_vp, C.c_int]
        lib.sdrhip_fm_chain_join.argtypes = [_vp, _vp]
        lib.sdrhip_fm_chain_enable_timing.argtypes = [_vp, C.c_int]
        lib.sdrhip_fm_chain_read_timing.argtypes = [_vp, C.POINTER(C.c_double), C.POINTER(C.c_int)]
        lib.sdrhip_last_error.restype = C.c_char_p
        self.has_order = hasattr(lib, "sdrhip_debug_set_resample_order")
        if self.has_order:
            lib.sdrhip_debug_set_resample_order.argtypes = [C.c_int]
            lib.sdrhip_debug_set_resample_order.restype = None
        self.h = _vp()
        a, b, c = (np.ascontiguousarray(t, np.float32) for t in (S.taps_decim127(), S.taps_resamp191(), S.taps_audio_half64()))
        self.ok(lib.sdrhip_fm_chain_create(C.byref(self.h), L.ORDER_AVX, 8, a.ctypes.data_as(_f32p), a.size, 3, 10, b.ctypes.data_as(_f32p), b.size,
                                           c.ctypes.data_as(_f32p), c.size, C.c_float(0.2), B), "create")

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{self.name}: {what}: {self.lib.sdrhip_last_error().decode()}")

    def plan(self, total):
        q0, q1, halo = _i64(), _i64(), _i64()
        self.ok(self.lib.sdrhip_fm_chain_plan(self.h, 0, total, -1, C.byref(q0), C.byref(q1), C.byref(halo)), "plan")
        return q0.value, q1.value, halo.value

    def set_order(self, order):
        if self.has_order:
            self.lib.sdrhip_debug_set_resample_order(2 if order is None else order)

    def close(self):
        self.lib.sdrhip_fm_chain_destroy(self.h)


class Pass:
    """The buffers of one pass size, shared by every build (the chains differ, the data does not)."""

    def __init__(self, builds, blocks):
        self.n = blocks * B
        q0, q1, halo = builds[0].plan(self.n)
        assert all(b.plan(self.n) == (q0, q1, halo) for b in builds), "the builds plan the pass differently"
        self.q0, self.q1, self.halo = q0, q1, halo
        gen = torch.Generator(device="cuda").manual_seed(S.SEED_IQ)
        self.u8 = [torch.randint(0, 256, (2 * (self.n + B),), dtype=torch.uint8, device="cuda", generator=gen)]
        self.u8.append(self.u8[0].clone())          # two runs in flight: input and audio double-buffered (sdr_hip.h)
        self.audio = [torch.empty(q1 - q0, dtype=torch.float32, device="cuda") for _ in range(2)]
        self.ws = None
        self.stream = torch.cuda.current_stream().cuda_stream

    def workspace(self, builds):
        wsb = max(int(b.lib.sdrhip_fm_chain_workspace_bytes(b.h, self.n + B)) for b in builds)
        if self.ws is None or self.ws.numel() < wsb:
            self.ws = None
            self.ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")
        return wsb

    def run(self, b, k, flip):
        for _ in range(k):
            flip[0] ^= 1
            b.ok(b.lib.sdrhip_fm_chain_run(b.h, self.stream, self.u8[flip[0]].data_ptr(), 0, self.n + self.halo, self.audio[flip[0]].data_ptr(),
                                           self.q0, self.q1, self.ws.data_ptr(), self.ws.numel()), "run")


def measure_row(p, b, order, overlap, row_s, sampler):
    b.set_order(order)
    flip = [0]
    p.run(b, 8, flip)
    if overlap:
        b.ok(b.lib.sdrhip_fm_chain_join(b.h, p.stream), "join")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    p.run(b, 8, flip)
    if overlap:
        b.ok(b.lib.sdrhip_fm_chain_join(b.h, p.stream), "join")
    torch.cuda.synchronize()
    per = (time.perf_counter() - t0) / 8
    k = max(16, int(math.ceil(row_s / per)))
    if not overlap:
        b.ok(b.lib.sdrhip_fm_chain_enable_timing(b.h, 1), "enable_timing")
    t_lo = time.perf_counter() - sampler.t0 if sampler.available else None
    t0 = time.perf_counter()
    p.run(b, k, flip)
    if overlap:
        b.ok(b.lib.sdrhip_fm_chain_join(b.h, p.stream), "join")
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    t_hi = time.perf_counter() - sampler.t0 if sampler.available else None
    stages = None
    if not overlap:
        ms, runs = (C.c_double * 6)(), C.c_int()
        b.ok(b.lib.sdrhip_fm_chain_read_timing(b.h, ms, C.byref(runs)), "read_timing")
        b.ok(b.lib.sdrhip_fm_chain_enable_timing(b.h, 0), "enable_timing")
        stages = {s: ms[i] / max(runs.value, 1) for i, s in enumerate(STAGES)}
    b.set_order(None)
    power = PP.HwmonSampler.summarize(sampler.samples, t_lo, t_hi) if sampler.available else None
    return {"ms": dt / k * 1e3, "passes": k, "seconds": dt, "stages": stages, "power": power}


def fmt_row(label, r):
    s = f"{label:34s} {r['ms']:8.4f} ms/pass  ({r['passes']} passes, {r['seconds']:.2f} s)"
    if r["stages"]:
        st = r["stages"]
        s += f"  stages dec {st['decimate']:.4f} demod {st['fm_demod']:.4f} resamp {st['resample']:.4f} filt {st['filter']:.4f}"
    if r["power"]:
        pw = r["power"]
        s += f"  {pw['mean_w']:.0f} W  {pw['mean_sclk_mhz']:.0f} MHz ({pw['samples']} samples)"
    return s


def alternate(p, base, variants, overlap, rounds, row_s, sampler):
    """base X1 base X2 ... for `rounds` rounds -> {label: [row, ...]}"""
    rows = {}
    for b in {base[1]} | {v[1] for v in variants}:
        b.ok(b.lib.sdrhip_fm_chain_set_overlap(b.h, 1 if overlap else 0), "set_overlap")
    p.workspace(          # (two runs in flight take a workspace half each: sized after the switch)
        [base[1]] + [v[1] for v in variants])
    for rnd in range(rounds):
        for label, b, order in variants:
            for lab, bb, oo in (base, (label, b, order)):
                r = measure_row(p, bb, oo, overlap, row_s, sampler)
                rows.setdefault(lab, []).append(r)
                print(f"  round {rnd}  " + fmt_row(lab, r), flush=True)
    for b in {base[1]} | {v[1] for v in variants}:
        b.ok(b.lib.sdrhip_fm_chain_set_overlap(b.h, 0), "set_overlap")
    return rows


def summary(rows, base_label, what):
    base = np.array([r["ms"] for r in rows[base_label]])
    mean, sd, rng = base.mean(), base.std(ddof=1), base.max() - base.min()
    print(f"  SUMMARY {what}")
    print(f"    base {base_label}: {len(base)} rows, mean {mean:.4f} ms, spread (std of rows) {sd:.4f} ms = {100 * sd / mean:.3f} %, "
          f"range {rng:.4f} ms = {100 * rng / mean:.3f} %, bar 2 x spread = {200 * sd / mean:.3f} %")
    out = {}
    for label, rs in rows.items():
        if label == base_label:
            continue
        v = np.array([r["ms"] for r in rs])
        gain = 100 * (mean - v.mean()) / mean
        out[label] = gain
        line = f"    {label:34s} {len(v)} rows, mean {v.mean():.4f} ms (std {v.std(ddof=1):.4f}), gain {gain:+.3f} %  -> {'CLEARS' if gain > 200 * sd / mean else 'does not clear'} the bar"
        pw = [r["power"] for r in rs if r["power"]]
        bw = [r["power"] for r in rows[base_label] if r["power"]]
        if pw and bw:
            line += (f"; {np.mean([q['mean_w'] for q in pw]):.0f} W / {np.mean([q['mean_sclk_mhz'] for q in pw]):.0f} MHz against "
                     f"{np.mean([q['mean_w'] for q in bw]):.0f} W / {np.mean([q['mean_sclk_mhz'] for q in bw]):.0f} MHz")
        print(line)
        if rs[0]["stages"]:
            for s in ("decimate", "resample", "filter"):
                a = np.mean([r["stages"][s] for r in rows[base_label]])
                c = np.mean([r["stages"][s] for r in rs])
                print(f"        {s:9s} {a:.4f} -> {c:.4f} ms ({100 * (a - c) / a:+.2f} %)")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--unfused")
    ap.add_argument("--blocks", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--row-seconds", type=float, default=2.0)
    ap.add_argument("--base", choices=("parent", "new"), default="parent",
                    help="new: this tree's library is the base and runs first, the parent is the variant (the other load order: "
                         "the two-runs-in-flight streams of a library are made at its first such run)")
    ap.add_argument("--order-sweep", default="", help="comma-separated pass sizes in blocks")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    print(f"device {L.device_name()}; product library {L.version()}")
    new = Build("new", L.LIB_PATH)
    parent = Build("parent", args.parent) if args.parent else None
    unfused = Build("unfused", args.unfused) if args.unfused else None
    for b in (parent, unfused, new):
        if b:
            print(f"  build {b.name}: {b.path}  order switch: {b.has_order}")
    variants = []
    if unfused:
        if parent:
            variants.append(("unfused, oldest-first (= parent)", unfused, 0))
        if unfused.has_order:
            variants.append(("newest-first alone", unfused, 1))
    variants.append(("first_mac alone", new, 0))
    if new.has_order:
        variants.append(("first_mac + newest-first", new, 1))
    if args.base == "new" and parent:
        base, variants = ("first_mac (this tree), runs first", new, 0), [("parent", parent, None)]
    else:
        base = ("parent", parent, None) if parent else (("unfused, oldest-first", unfused, 0) if unfused else variants.pop(0))
    print(f"base: {base[0]}; variants: {', '.join(v[0] for v in variants)}")
    builds = [b for b in (parent, unfused, new) if b]
    sampler = PP.HwmonSampler(0.05, PP.device_bdf()).start()
    print(f"hwmon sampler available: {sampler.available}; cap {sampler.cap_watts() if sampler.available else None} W")
    p = Pass(builds, args.blocks)
    # the same audio from every build and order before anything is timed
    p.workspace(builds)
    ref = None
    for label, b, order in [base] + variants:
        b.set_order(order)
        flip = [1]
        p.run(b, 1, flip)
        torch.cuda.synchronize()
        b.set_order(None)
        a = p.audio[0].view(torch.int32).clone()
        if ref is None:
            ref = a
        assert torch.equal(ref, a), f"{label}: the audio differs from the base's"
    print(f"audio of {1 + len(variants)} configurations bit-equal ({ref.numel()} samples)")
    del ref, a
    for overlap in (True, False):
        what = f"{args.blocks} blocks, " + ("two runs in flight (bench.py's default mode)" if overlap else "one run at a time")
        print(f"== {what}")
        rows = alternate(p, base, variants, overlap, args.rounds, args.row_seconds, sampler)
        summary(rows, base[0], what)
    del p
    torch.cuda.empty_cache()
    for blocks in [int(x) for x in args.order_sweep.split(",") if x and new.has_order]:
        p = Pass([new], blocks)
        for overlap in (True, False):
            what = f"{blocks} blocks, " + ("two runs in flight" if overlap else "one run at a time") + ": tile order, this tree's library"
            print(f"== {what}")
            rows = alternate(p, ("oldest-first", new, 0), [("newest-first", new, 1)], overlap, args.rounds, min(args.row_seconds, 1.0), sampler)
            summary(rows, "oldest-first", what)
        del p
        torch.cuda.empty_cache()
    sampler.stop()
    for b in builds:
        b.close()


if __name__ == "__main__":
    main()
