// tuner.cpp -- the tuner of include/sdr_hip.h: descriptor, routes and the oscillator tables (kernels: kernels_tuner.hip).
//
// Routes.  Fused: one tile kernel, the mixed samples never reach memory (AVX order, decimation 4 / 8 / 16, up to 128 prepared
// taps, aligned tile starts).  Two-pass: k_tuner_mix writes the mixed samples of a bounded chunk of the launch into a leased
// scratch buffer and the stock decimator (fir_run, every order and factor) runs on it; chunks overlap by numCoeffs - factor
// samples, which are mixed twice.  Both give sdrhip_decimator_run's bits on the mixed stream.
// Input formats (InFmt): every kernel-side entry point takes the format.  int16 IQ (sdrhip_tuner_run_i16) has no one-row tile kernel:
// launch_tuner_fused hands it to the tuner bank's tile kernel with one channel; its two-pass route is k_tuner_mix on int16.
#include <math.h>

#include <atomic>
#include <mutex>

#include "descriptors.hpp"
#include "scratch_pool.hpp"

namespace sdrhip {

// Samples of scratch one two-pass chunk mixes (8 bytes each): 32 MiB by default (sdrhip_debug_set_tuner_chunk).
constexpr int64_t kTunerChunkSamples = (int64_t)1 << 22;
static std::atomic<int64_t> g_tuner_chunk{kTunerChunkSamples};

// The scratch of the two-pass route.  A run borrows a lane (a leased ScratchCtx's `work` buffer and an event) for the time it
// ENQUEUES; the lane goes back while its kernels may still be running, and the next borrower makes its own stream wait for the
// event before it writes the buffer.  So concurrent host threads get a lane each and nothing waits on the host.
struct TunerScratch {
    struct Lane { ScratchCtx* ctx; hipEvent_t done; };
    std::mutex mu;
    std::vector<Lane> idle;
    std::mutex upload_mu;
};

TunerDesc::TunerDesc() : scratch(new TunerScratch()) {}
TunerDesc::~TunerDesc()
{
    for (TunerScratch::Lane& l : scratch->idle) {
        (void)hipEventSynchronize(l.done);
        (void)hipEventDestroy(l.done);
        scratch_release(l.ctx);
    }
    delete scratch;
    if (d_osc) (void)hipFree(d_osc);
}

int TunerDesc::ensure_device() const
{
    int rc = fir.ensure_device();          // also refuses a device other than the one of the first use
    if (rc != SDRHIP_OK) return rc;
    std::lock_guard<std::mutex> lk(scratch->upload_mu);
    if (d_osc) return SDRHIP_OK;
    return upload_floats(&d_osc, h_osc);
}

static int tuner_two_pass(const TunerDesc* t, hipStream_t s, const void* d_in, InFmt fmt, const Geom& g, float* d_out, int64_t seam_block)
{
    TunerScratch* sc = t->scratch;
    TunerScratch::Lane lane = {nullptr, nullptr};
    {
        std::lock_guard<std::mutex> lk(sc->mu);
        if (!sc->idle.empty()) { lane = sc->idle.back(); sc->idle.pop_back(); }
    }
    if (!lane.ctx) {
        lane.ctx = scratch_acquire();
        if (!lane.ctx) return SDRHIP_ERR_HIP;
        hipError_t e = hipEventCreateWithFlags(&lane.done, hipEventDisableTiming);
        if (e != hipSuccess) {
            set_error("sdrhip_tuner_run: %s", hipGetErrorString(e));
            scratch_release(lane.ctx);
            return SDRHIP_ERR_HIP;
        }
    }
    auto give_back = [&] {
        std::lock_guard<std::mutex> lk(sc->mu);
        sc->idle.push_back(lane);
    };
    const int D = g.D, Lp = g.Lp;
    int64_t chunk = g_tuner_chunk.load(std::memory_order_relaxed);
    if (chunk < (int64_t)Lp + D) chunk = (int64_t)Lp + D;
    const int64_t cnt_max = (chunk - Lp) / D + 1;                  // outputs whose windows fit `chunk` samples
    const int64_t cnt0 = g.count < cnt_max ? g.count : cnt_max;
    const size_t bytes = (size_t)((cnt0 - 1) * D + Lp) * 8;
    int rc = SDRHIP_OK;
    hipError_t e = hipSuccess;
    // the lane's last borrower may have been another stream: order this run's writes behind its reads (growing frees the buffer)
    if (bytes > lane.ctx->work.cap) e = hipEventSynchronize(lane.done);
    else e = hipStreamWaitEvent(s, lane.done, 0);
    if (e == hipSuccess) rc = lane.ctx->work.ensure(bytes);
    if (e == hipSuccess && rc == SDRHIP_OK) {
        float* work = static_cast<float*>(lane.ctx->work.p);
        const int esz = in_fmt_bytes(fmt);
        const int64_t k_end = g.k_begin + g.count;
        for (int64_t kb = g.k_begin; kb < k_end && rc == SDRHIP_OK; kb += cnt_max) {
            const int64_t ke = kb + cnt_max < k_end ? kb + cnt_max : k_end;
            const int64_t a0 = kb * D, nin = (ke - kb - 1) * D + Lp;
            const char* src = static_cast<const char*>(d_in) + esz * (a0 - g.in_base);
            launch_tuner_mix(s, src, fmt, work, nin, t->d_osc, t->period, (int)(a0 % t->period));
            rc = fir_run(&t->fir, s, work, false, a0, d_out + 2 * (kb - g.k_begin), kb, ke, seam_block);
        }
        if (rc == SDRHIP_OK) e = hipGetLastError();
        const hipError_t e2 = hipEventRecord(lane.done, s);
        if (e == hipSuccess) e = e2;
    }
    give_back();
    if (e != hipSuccess) {
        set_error("sdrhip_tuner_run (two-pass): %s", hipGetErrorString(e));
        return SDRHIP_ERR_HIP;
    }
    return rc;
}

int tuner_run(const TunerDesc* t, hipStream_t s, const void* d_in, InFmt fmt, int64_t in_base, float* d_out, int64_t k_begin,
              int64_t k_end, int64_t seam_block)
{
    SDRHIP_REQUIRE(t != nullptr, "tuner_run");
    const FirDesc* d = &t->fir;
    SDRHIP_REQUIRE(k_begin >= 0 && k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, "tuner_run");
    SDRHIP_REQUIRE(k_begin * d->factor >= in_base, "tuner_run: first window starts before d_in");
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block >= d->Lp, "tuner_run: seam block shorter than the filter (Filter.hs:586)");
    if (k_end == k_begin) return SDRHIP_OK;
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr, "tuner_run");
    SDRHIP_REQUIRE(fmt != IN_I16 || (reinterpret_cast<uintptr_t>(d_in) & 3) == 0, "tuner_run: int16 IQ at an address that is no multiple of 4");
    int rc = t->ensure_device();
    if (rc != SDRHIP_OK) return rc;
    const Geom g = bank_geom(d, in_base, k_begin, k_end, seam_block);      // (a tuner is one channel of a bank)
    const int route = t->route;
    if (route != 2) {
        const bool fused = d->corder == CO_L4 && launch_tuner_fused(s, g, d->d_plain, d->Lp, d->d_cross, d_in, fmt, d_out, t->d_osc, t->period);
        if (fused) {
            SDRHIP_CHECK_HIP(hipGetLastError());
            return SDRHIP_OK;
        }
        if (route == 1) {
            set_error("sdrhip_tuner_run: the fused route serves the AVX order, factors 4 / 8 / 16, up to 128 prepared taps, seam_block >= 0 "
                      "and a 16-byte aligned first window; this launch is none of that (route 0 or 2 runs it)");
            return SDRHIP_ERR_ARG;
        }
    }
    return tuner_two_pass(t, s, d_in, fmt, g, d_out, seam_block);
}

// exp(2 pi i r / den) as float32, r in [0, den): the reduction documented in include/sdr_hip.h
static void shift_entry(int64_t r, int64_t den, float* re, float* im)
{
    const int64_t q = (4 * r) / den, f = 4 * r - q * den;      // quarter turn q, f / (4 den) of a turn into it
    float c, s;
    if (f == 0) { c = 1.0f; s = 0.0f; }
    else if (2 * f == den) { c = s = (float)cos(3.141592653589793 * 0.25); }
    else if (2 * f < den) {
        const double phi = 3.141592653589793 * ((double)f / (double)(2 * den));
        c = (float)cos(phi);
        s = (float)sin(phi);
    } else {
        const double phi = 3.141592653589793 * ((double)(den - f) / (double)(2 * den));
        c = (float)sin(phi);
        s = (float)cos(phi);
    }
    // 0.0f - x: the negative of x, and +0 for x = 0
    switch (q) {
    case 0: *re = c; *im = s; break;
    case 1: *re = 0.0f - s; *im = c; break;
    case 2: *re = 0.0f - c; *im = 0.0f - s; break;
    default: *re = s; *im = 0.0f - c; break;
    }
}

}  // namespace sdrhip

using namespace sdrhip;

extern "C" {

int sdrhip_tuner_create(sdrhip_tuner** t, int order, int factor, const float* coeffs, int ncoeffs, const float* osc_iq, int period)
{
    SDRHIP_REQUIRE(t != nullptr, "sdrhip_tuner_create");
    *t = nullptr;
    SDRHIP_REQUIRE(period >= 1 && period <= 65536, "sdrhip_tuner_create: period 1 .. 65536");
    SDRHIP_REQUIRE(osc_iq != nullptr, "sdrhip_tuner_create: null oscillator table");
    sdrhip_tuner* p = new sdrhip_tuner();
    int rc = fir_create(&p->fir, order, true, factor, coeffs, ncoeffs);
    if (rc != SDRHIP_OK) { delete p; return rc; }
    p->period = period;
    p->h_osc.assign(osc_iq, osc_iq + 2 * (size_t)period);
    *t = p;
    return SDRHIP_OK;
}
int sdrhip_tuner_num_coeffs(const sdrhip_tuner* t) { return t ? t->fir.Lp : SDRHIP_ERR_ARG; }
int sdrhip_tuner_factor(const sdrhip_tuner* t) { return t ? t->fir.factor : SDRHIP_ERR_ARG; }
int sdrhip_tuner_period(const sdrhip_tuner* t) { return t ? t->period : SDRHIP_ERR_ARG; }
void sdrhip_tuner_destroy(sdrhip_tuner* t) { delete t; }

int sdrhip_tuner_set_route(sdrhip_tuner* t, int route)
{
    SDRHIP_REQUIRE(t != nullptr && route >= 0 && route <= 2, "sdrhip_tuner_set_route");
    t->route = route;
    return SDRHIP_OK;
}

int sdrhip_tuner_run(const sdrhip_tuner* t, void* stream, const float* d_in, int64_t in_base, float* d_out, int64_t k_begin,
                     int64_t k_end, int64_t seam_block)
{
    return tuner_run(t, (hipStream_t)stream, d_in, IN_CF32, in_base, d_out, k_begin, k_end, seam_block);
}
int sdrhip_tuner_run_i16(const sdrhip_tuner* t, void* stream, const int16_t* d_in_iq, int64_t in_base, float* d_out, int64_t k_begin,
                         int64_t k_end, int64_t seam_block)
{
    return tuner_run(t, (hipStream_t)stream, d_in_iq, IN_I16, in_base, d_out, k_begin, k_end, seam_block);
}
int sdrhip_tuner_run_u8(const sdrhip_tuner* t, void* stream, const uint8_t* d_in_iq, int64_t in_base, float* d_out, int64_t k_begin,
                        int64_t k_end, int64_t seam_block)
{
    return tuner_run(t, (hipStream_t)stream, d_in_iq, IN_U8, in_base, d_out, k_begin, k_end, seam_block);
}

int sdrhip_tuner_shift_table(int64_t num, int64_t den, float* osc_iq)
{
    SDRHIP_REQUIRE(den >= 1 && den < ((int64_t)1 << 31) && osc_iq != nullptr, "sdrhip_tuner_shift_table");
    int64_t step = num % den;
    if (step < 0) step += den;
    int64_t r = 0;
    for (int64_t n = 0; n < den; n++) {
        shift_entry(r, den, &osc_iq[2 * n], &osc_iq[2 * n + 1]);
        r += step;                    // (num n) mod den without the product
        if (r >= den) r -= den;
    }
    return SDRHIP_OK;
}

long long sdrhip_debug_tuner_fused_launches(void) { return tuner_fused_launch_count(); }
long long sdrhip_debug_tuner_i16_launches(void) { return tuner_i16_launch_count(); }

int64_t sdrhip_debug_set_tuner_chunk(int64_t samples)
{
    if (samples > ((int64_t)1 << 30)) samples = (int64_t)1 << 30;
    return g_tuner_chunk.exchange(samples <= 0 ? kTunerChunkSamples : samples);
}

}  // extern "C"
