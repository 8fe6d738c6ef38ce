"""A bank's host-block stream against what a receiver of K stations had before it: K FmStreams over K tuned chains, fed the same
pushes.  Both in one process, alternating.

    python tools/fm_bank_stream_bench.py [--rounds R] [--out profiles/fm_bank_stream_bench.txt]

Sweep: K = 1, 2, 8, 12, 32 stations x pushes of 1, 16 and 128 source blocks (8192 samples each) x two ways of pushing:
  memcpy   push(block): the library copies the caller's block into its pinned staging buffer -- K copies for K streams
  buffer   input_buffer / push of that pointer: the source writes the staging buffer itself.  A source can write ONE buffer: with K
           streams, stream 0 is pushed without a copy and the caller copies its block into the other K - 1 staging buffers
  bank     ONE FmStream over an FmBank of the K tables: one staging buffer, one crossing of the link, one launch per submission
  streams  K FmStreams over K tuned FmChains, every push made K times
Every figure is a host clock around `reps` pushes and the flush that ends them (so the work ends in a synchronise and all the
audio is popped into numpy arrays on both sides), after a warm-up of the same shape; reps are chosen for windows of about 0.05 s.
Both sides run with the defaults a caller gets (slots, adaptive submission).  The table gives median (min .. max) in us PER PUSH
over the rounds.  The reading rule: for K >= 2 the bank's stream is ahead when its slowest round is below the streams' fastest
(ahead by more than the spread of either side); at K = 1 the two are level when their medians differ by no more than the larger
spread (max - min).  Points that miss the rule are marked and listed at the end; nothing is tuned here.

Second table, the lone source block at K = 2, 4, 8, 12: the same bank stream with the lone block read IN PLACE over the link by
the banked launch (largest tile) against the slot-stream COPY (one pass over the link, then the launch on device memory),
selected for this comparison by SDRHIP_STAGE_SAMPLES at stream creation.  It decides whether streams of several stations keep an
in-place route.  A missing GPU is an error.

    python tools/fm_bank_stream_bench.py --i16 [--rounds R] [--out profiles/fm_bank_stream_i16_bench.txt]

One int16 bank stream (FmStream(bank, ..., input_i16=True), push_i16) against a u8 bank stream of the same pushes, the two
alternating: K = 2, 8, 32 stations x pushes of 1, 16 and 128 source blocks, memcpy pushes.  An int16 push carries twice the bytes
and never runs in place.  Reported; no rule depends on it."""
import argparse
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
STATIONS = (1, 2, 8, 12, 32)
PUSH_BLOCKS = (1, 16, 128)
ROUTE_STATIONS = (2, 4, 8, 12)
WINDOW_S = 0.05
ARGS = (8, S.taps_decim127(), 3, 10, S.taps_resamp191(), S.taps_audio_half64())


def tables(K):
    """K stations on a raster of 1/64 of the sampling frequency around the centre (the centre itself: the table {1, 0})"""
    return [L.tuner_shift_table((j - K // 2) % 64, 64) if j != K // 2 else np.array([1.0, 0.0], np.float32) for j in range(K)]


def bank_stream(K, nblk):
    return L.FmStream(L.FmBank(*ARGS, tables(K), 0.2, B), nblk * B, B)


def chain_streams(K, nblk):
    out = []
    for t in tables(K):
        ch = L.FmChain(*ARGS, 0.2, B)
        ch.set_tuner(t)
        out.append(L.FmStream(ch, nblk * B, B))
    return out


def leg(streams, chunk, how):
    """-> function(reps): reps pushes of `chunk` into every stream, then the flush; returns the audio blocks of the last call"""
    n = chunk.size // 2

    def run(reps):
        got = [[] for _ in streams]
        for _ in range(reps):
            if how == "memcpy":
                for g, st in zip(got, streams):
                    g += st.push(chunk)
            else:
                first = None
                for g, st in zip(got, streams):
                    view = st.input_buffer(n)
                    if first is None:
                        first = view                    # the source wrote this one
                    else:
                        view[:] = first                 # ... and the caller copies it into every other stream's buffer
                    g += st.push_inplace(view)
        for g, st in zip(got, streams):
            g += st.flush()
        return got
    return run


def leg_i16(st, chunk):
    def run(reps):
        got = []
        for _ in range(reps):
            got += st.push_i16(chunk)
        got += st.flush()
        return [got]
    return run


def main_i16(a):
    rng = np.random.default_rng(1601)
    i16 = rng.integers(-32768, 32768, 2 * 128 * B, dtype=np.int64).astype(np.int16)
    u8 = S.iq_u8_fm(128 * B)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, an int16 bank stream and a u8 bank stream of the same pushes alternating; memcpy pushes; "
             "host clock around push ... flush, us PER PUSH (all K stations): median (min .. max)"]
    print(lines[0], flush=True)
    for nblk in PUSH_BLOCKS:
        c16, c8 = np.ascontiguousarray(i16[:2 * nblk * B]), np.ascontiguousarray(u8[:2 * nblk * B])
        for K in (2, 8, 32):
            s16 = L.FmStream(L.FmBank(*ARGS, tables(K), 0.2, B), nblk * B, B, input_i16=True)
            s8 = bank_stream(K, nblk)
            b0, i0 = L.fm_bank_launches(), L.fm_bank_i16_launches()
            t = measure({"int16": leg_i16(s16, c16), "u8": leg([s8], c8, "memcpy")}, a.rounds)
            nb, ni = L.fm_bank_launches() - b0, L.fm_bank_i16_launches() - i0
            assert ni > 0 and nb > ni, "a leg took another route than the one it is named for"
            line = (f"{nblk:3d} blocks per push  K {K:2d}   int16 {fmt(t['int16'])}   u8 {fmt(t['u8'])}   "
                    f"int16 / u8 {statistics.median(t['int16']) / statistics.median(t['u8']):.3f}")
            print(line, flush=True)
            lines.append(line)
            del s16, s8
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def timed(fn, reps):
    t0 = time.perf_counter()
    fn(reps)
    return (time.perf_counter() - t0) / reps * 1e6


def measure(fns, rounds):
    """fns: {name: function(reps)} -> {name: [us per push, one per round]}, the legs alternating within each round"""
    reps = {}
    for name, fn in fns.items():
        fn(8)                                               # warm-up of this shape: code objects, tables, staging buffers
        per = timed(fn, 16) * 1e-6
        reps[name] = max(8, min(4000, int(WINDOW_S / per)))
    times = {k: [] for k in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            times[name].append(timed(fn, reps[name]))
    return times


def fmt(v):
    return f"{statistics.median(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"


def same_audio(K, nblk, chunk):
    """the two sides compute the same audio (tests/test_gpu_fm_bank_stream.py holds the stream to it; here: that they time the same work)"""
    bank = leg([bank_stream(K, nblk)], chunk, "memcpy")(max(4, 64 // nblk))[0]
    each = leg(chain_streams(K, nblk), chunk, "memcpy")(max(4, 64 // nblk))
    rows = np.concatenate(bank, axis=1) if bank else np.zeros((K, 0), np.float32)
    for j in range(K):
        ref = np.concatenate(each[j]) if each[j] else np.zeros(0, np.float32)
        if not np.array_equal(rows[j].view(np.uint32), ref.view(np.uint32)):
            sys.exit(f"fm_bank_stream_bench: station {j} of {K} differs between the bank's stream and its chain's ({nblk} blocks per push)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--i16", action="store_true", help="an int16 bank stream against a u8 bank stream of the same pushes")
    a = ap.parse_args()
    if L.device_count() < 1:
        sys.exit("fm_bank_stream_bench: no HIP device")
    if a.i16:
        return main_i16(a)
    u8 = S.iq_u8_fm(128 * B)
    lines = [f"# {L.device_name()}; {a.rounds} rounds, the bank's stream and K chain streams alternating; host clock around push ... flush, "
             "us PER PUSH (all K stations): median (min .. max)"]
    print(lines[0], flush=True)
    missed = []
    for nblk in PUSH_BLOCKS:
        chunk = np.ascontiguousarray(u8[:2 * nblk * B])
        for K in STATIONS:
            same_audio(K, nblk, chunk)
            for how in ("memcpy", "buffer"):
                bank, streams = bank_stream(K, nblk), chain_streams(K, nblk)
                b0, c0 = L.fm_bank_launches(), L.small_chain_tuned_launches()
                t = measure({"bank": leg([bank], chunk, how), "streams": leg(streams, chunk, how)}, a.rounds)
                nb, nc = L.fm_bank_launches() - b0, L.small_chain_tuned_launches() - c0
                assert nb > 0 and nc > 0, "a leg took another route than the one it is named for"
                mb, ms = statistics.median(t["bank"]), statistics.median(t["streams"])
                spread = max(max(v) - min(v) for v in t.values())
                if K == 1:
                    ok = abs(mb - ms) <= spread
                    verdict = "level within the spread" if ok else "NOT level within the spread"
                else:
                    ok = max(t["bank"]) < min(t["streams"])
                    verdict = "ahead by more than the spread" if ok else "NOT ahead by more than the spread"
                line = (f"{nblk:3d} blocks per push  {how:6s}  K {K:2d}   bank {fmt(t['bank'])}   streams {fmt(t['streams'])}   "
                        f"bank / streams {mb / ms:.3f}   {verdict}")
                print(line, flush=True)
                lines.append(line)
                if not ok:
                    missed.append(line)
                del bank, streams
    lines.append("# the lone source block: the banked launch reading the pinned staging buffer IN PLACE over the link (largest tile) against "
                 "the slot-stream COPY and a launch on device memory; the same bank stream, memcpy pushes")
    print(lines[-1], flush=True)
    chunk = np.ascontiguousarray(u8[:2 * B])
    inplace_wins = []
    for K in ROUTE_STATIONS:
        made = {}
        for name, bound in (("in place", 1 << 40), ("copy", 0)):
            os.environ["SDRHIP_STAGE_SAMPLES"] = str(bound)         # read when a stream is created
            made[name] = bank_stream(K, 1)
        del os.environ["SDRHIP_STAGE_SAMPLES"]
        t = measure({name: leg([st], chunk, "memcpy") for name, st in made.items()}, a.rounds)
        mi, mc = statistics.median(t["in place"]), statistics.median(t["copy"])
        wins = max(t["in place"]) < min(t["copy"])
        line = (f"  1 block  per push  K {K:2d}   in place {fmt(t['in place'])}   copy {fmt(t['copy'])}   in place / copy {mi / mc:.3f}   "
                f"{'in place ahead by more than the spread' if wins else 'in place NOT ahead by more than the spread'}")
        print(line, flush=True)
        lines.append(line)
        if wins:
            inplace_wins.append(K)
        del made
    lines.append(f"# in place is ahead of the copy by more than the spread at K = {inplace_wins if inplace_wins else 'no measured K'}")
    lines.append(f"# points that miss the reading rule: {len(missed)}")
    lines += ["#   " + m for m in missed]
    print("\n".join(lines[-2 - len(missed):]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
