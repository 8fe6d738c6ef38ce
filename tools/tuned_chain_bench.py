"""The FM chain with a tuner against the untuned chain of the same build, alternating the two in one process.

    python tools/tuned_chain_bench.py [--rounds R] [--out FILE]

Three sizes, `shift_table(1, 4)`:
  * 16-block pushes through sdrhip_fm_stream (the one-kernel chain, input staged to the device on the slot's stream);
  * a resident run of 2^20 samples (the one-kernel chain);
  * a resident run of 2^27 samples (untuned: the systolic decimator; tuned: the tuner's tile kernel -- there is no tuned systolic
    kernel, and this ratio is what that costs).
Every figure is a host clock around work that ends in a device synchronise (pushes: a flush), after warm-up launches of the same
shape; tuned and untuned alternate within each round and the table gives the median and the spread over the rounds, so a ratio can
be read against the run-to-run noise of the untuned chain itself.  A missing GPU is an error.  The parent commit's untuned chain
is measured by running this same file's untuned legs on a build of the parent (--untuned-only)."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import sdr_amd.lib as L
import signals as S

B = 8192


def chain(tuned):
    ch = L.FmChain(8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64(), 0.2, B)
    if tuned:
        ch.set_tuner(L.tuner_shift_table(1, 4))
    return ch


def stream_case(tuned, pushes=1500, bpp=16):
    """-> a function that times `pushes` zero-copy pushes of bpp source blocks (microseconds per push)"""
    st = L.FmStream(chain(tuned), bpp * B, B)
    x = np.random.default_rng(2).integers(0, 256, 2 * bpp * B, dtype=np.uint8)

    def go(n):
        for _ in range(n):
            v = st.input_buffer(bpp * B)
            v[:] = x
            st.push_inplace(v)
        st.flush()

    go(64)

    def timed():
        t0 = time.perf_counter()
        go(pushes)
        return (time.perf_counter() - t0) / pushes * 1e6

    return timed


def resident_case(tuned, n_samples, reps):
    """-> a function that times `reps` back-to-back runs over n_samples resident samples (microseconds per run)"""
    ch = chain(tuned)
    halo = ch.halo_samples()
    n_in = n_samples + halo
    q0, q1, _ = ch.plan(0, n_samples, -1)
    d_in = torch.randint(0, 256, (2 * n_in,), dtype=torch.uint8, device="cuda")
    out = torch.empty(q1 - q0, dtype=torch.float32, device="cuda")
    wsb = ch.workspace_bytes(n_in)
    ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

    def go(n):
        for _ in range(n):
            ch.run(d_in.data_ptr(), 0, n_in, out.data_ptr(), q0, q1, ws.data_ptr(), wsb)
        torch.cuda.synchronize()

    go(3)

    def timed():
        t0 = time.perf_counter()
        go(reps)
        return (time.perf_counter() - t0) / reps * 1e6

    return timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--untuned-only", action="store_true", help="only the untuned legs (for a build of the parent commit)")
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("tuned_chain_bench: no HIP device")
    lines = [f"# {L.device_name()}; {a.rounds} rounds, tuned and untuned alternating; us per push / run: median (min .. max)"]
    cases = [("fm_stream, 16-block pushes", lambda t: stream_case(t)),
             ("resident run, 2^20 samples", lambda t: resident_case(t, 1 << 20, 400)),
             ("resident run, 2^27 samples", lambda t: resident_case(t, 1 << 27, 12))]
    for name, make in cases:
        legs = {False: make(False)}
        if not a.untuned_only:
            legs[True] = make(True)
        c0 = (L.small_chain_tuned_launches(), int(L.lib.sdrhip_debug_small_chain_launches()), L.tuner_fused_launches(),
              int(L.lib.sdrhip_debug_systolic_launches()))
        times = {k: [] for k in legs}
        for _ in range(a.rounds):
            for k in legs:
                times[k].append(legs[k]())
        c1 = (L.small_chain_tuned_launches(), int(L.lib.sdrhip_debug_small_chain_launches()), L.tuner_fused_launches(),
              int(L.lib.sdrhip_debug_systolic_launches()))
        fmt = lambda v: f"{statistics.median(v):10.1f} ({min(v):.1f} .. {max(v):.1f})"
        line = f"{name:30s} untuned {fmt(times[False])}"
        if True in times:
            line += f"   tuned {fmt(times[True])}   ratio {statistics.median(times[True]) / statistics.median(times[False]):.3f}"
        line += (f"   [launches: one-kernel chain {c1[1] - c0[1]} (tuned {c1[0] - c0[0]}), tuner tile kernel {c1[2] - c0[2]}, "
                 f"systolic {c1[3] - c0[3]}]")
        print(line, flush=True)
        lines.append(line)
        del legs
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
