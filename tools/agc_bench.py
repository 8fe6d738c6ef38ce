"""agc throughput on device-resident data: the speculative route (default run-in, a function of mu) and the one-lane
sequential walk, with the statistics words, for mu in {0.1, 0.01, 0.001} at 2^20, 2^24 and 2^26 complex samples -- next to a
single-thread plain-C restatement of the same arithmetic compiled and timed on the same box.

    python tools/agc_bench.py

The driver itself never opens the GPU: every measurement is a child process under its own time limit, and the first one that
fails ends the run."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUS = (0.1, 0.01, 0.001)
LOGS = (20, 24, 26)

C_RESTATEMENT = r"""
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>
static float magnitude(float re, float im)
{
    int er, ei;
    (void)frexpf(re, &er);
    (void)frexpf(im, &ei);
    const int k = er > ei ? er : ei;
    const float a = ldexpf(re, -k), b = ldexpf(im, -k);
    return ldexpf(sqrtf(a * a + b * b), k);
}
int main(int argc, char **argv)
{
    const long n = 1L << 24;
    const float mu = (float)atof(argv[1]), ref = 1.0f;
    float *x = malloc(sizeof(float) * 2 * n), *y = malloc(sizeof(float) * 2 * n);
    double ph = 0.0;
    unsigned s = 12345u;
    for (long i = 0; i < n; i++) {
        ph += 6.283185307179586 * (0.02 + 0.05 * sin(6.283185307179586 * (double)i / 480.0));
        s = s * 1664525u + 1013904223u;
        x[2 * i] = (float)(0.5 * cos(ph) + 0.01 * ((double)(s >> 8) / 8388608.0 - 1.0));
        s = s * 1664525u + 1013904223u;
        x[2 * i + 1] = (float)(0.5 * sin(ph) + 0.01 * ((double)(s >> 8) / 8388608.0 - 1.0));
    }
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    float state = 1.0f;
    for (long i = 0; i < n; i++) {
        const float cr = x[2 * i] * state, ci = x[2 * i + 1] * state;
        y[2 * i] = cr;
        y[2 * i + 1] = ci;
        state = state + mu * (ref - magnitude(cr, ci));
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    const double dt = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    printf("plain C, one thread, mu=%g n=2^24: %9.3f ms (%8.1f Ms/s)  final state %.9g, y[n-1] = %.9g\n", mu, dt * 1e3,
           (double)n / dt / 1e6, state, y[2 * n - 2]);
    return 0;
}
"""


def step(mu, lg):
    """One measurement in this process: both routes at one (mu, size)."""
    import time
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import sdr_amd.lib as L
    n = 1 << lg
    rng = np.random.default_rng(3)
    t = np.arange(n, dtype=np.float64)
    ph = np.cumsum(2 * np.pi * (0.02 + 0.05 * np.sin(2 * np.pi * t / 480.0)))
    z = (0.5 * np.exp(1j * ph)).astype(np.complex64)
    z += (0.01 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)
    x = torch.from_numpy(z.view(np.float32)).cuda()
    del t, ph, z
    out = torch.empty_like(x)
    fin = torch.zeros(1, dtype=torch.float32, device="cuda")
    wsb = L.lib.sdrhip_agc_workspace_bytes(n)
    ws = torch.zeros(wsb, dtype=torch.uint8, device="cuda")

    def timed(use_ws, reps):
        def go():
            L.check(L.lib.sdrhip_agc_run(None, x.data_ptr(), out.data_ptr(), n, mu, 1.0, 1.0, fin.data_ptr(),
                                         ws.data_ptr() if use_ws else None, wsb if use_ws else 0, 0), "sdrhip_agc_run")
        if use_ws:
            go()                                      # warm-up (the one-lane walk is seconds long: timed cold, once)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            go()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps, float(fin.cpu()[0]), out[-2:].cpu().numpy().copy()

    chunks, C, W = L.agc_plan(n, mu)
    dt, f_spec, tail_spec = timed(True, 5)
    st = ws[:16].cpu().numpy().view(np.uint32)
    line = (f"mu={mu:<6g} n=2^{lg}: speculative {dt * 1e3:9.3f} ms ({n / dt / 1e6:9.1f} Ms/s; {chunks} chunks of {C}, run-in {W}; "
            f"stats left/rewritten/repaired = {int(st[0])}/{int(st[1])}/{int(st[2])})")
    dt, f_seq, tail_seq = timed(False, 1)
    line += f" | one lane {dt * 1e3:10.3f} ms ({n / dt / 1e6:6.1f} Ms/s)"
    same = np.float32(f_spec).tobytes() == np.float32(f_seq).tobytes() and tail_spec.tobytes() == tail_seq.tobytes()
    print(line + (" | routes agree" if same else " | ROUTES DIFFER"), flush=True)
    return 0 if same else 1


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--step":
        return step(float(sys.argv[2]), int(sys.argv[3]))
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "agc_plain.c"), os.path.join(tmp, "agc_plain")
        with open(src, "w") as f:
            f.write(C_RESTATEMENT)
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", src, "-o", exe, "-lm"], check=True)
        for mu in MUS:
            subprocess.run(["timeout", "-k", "10", "120", exe, str(mu)], check=True)
    name = subprocess.run(["timeout", "-k", "10", "60", sys.executable, "-c",
                           f"import sys; sys.path.insert(0, {ROOT!r}); import sdr_amd.lib as L; print(L.device_name())"],
                          capture_output=True, text=True)
    if name.returncode != 0:
        sys.stderr.write(name.stdout + name.stderr)
        return name.returncode
    print(name.stdout.strip(), flush=True)
    for lg in LOGS:
        for mu in MUS:
            rc = subprocess.run(["timeout", "-k", "10", "180", sys.executable, os.path.abspath(__file__), "--step", str(mu), str(lg)]).returncode
            if rc != 0:
                print(f"step mu={mu} n=2^{lg} ended with status {rc}: stopping", flush=True)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
