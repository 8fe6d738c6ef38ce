// fft.cpp -- the spectrum path next to the hot path: the reference's SDR.FFT (hs_sources/SDR/FFT.hs:44-168)
//     fftw' / fftw            complex-to-complex forward DFT of n Complex Double   (planDFT1d .. Forward)
//     fftwReal' / fftwReal    real-to-complex DFT of n Double -> n/2 + 1 bins        (planDFTR2C1d)
//     fftwParallel            the same c2c DFT, several buffers in flight            (a thread pool there; a BATCHED plan here)
// on hipFFT: double precision (the reference computes in Double), unnormalised, forward sign exp(-2 pi i jk/n) -- FFTW's
// conventions, so a waterfall / spectrum plot (SDR.Plot) sees the same bins.  This is floating-point work with a different
// summation tree from FFTW's: the contract is a tolerance (tests/test_gpu_fft.py: 1e-11 of the largest bin), not bit parity.
// libhipfft.so is bound at run time like RCCL, so libsdr_hip.so keeps loading where it is absent.
//
// The spectrum operator (sdrhip_spectrum_*, second half of this file) is the reference's whole waterfall pipe on device memory: raw IQ
// (u8 as Util.hs:92-98 converts it, or float32) x halfBandUp (Util.hs:264-271) x a window (FilterDesign.hs:39-60) -> DFT -> scale * |X|
// as float32 rows.  Two routes with one contract (tests/test_gpu_spectrum.py): power-of-two n from 64 to 8192 run as ONE kernel of
// ours with the transform resident in LDS (kernels_spectrum.hip); every other n, or any n on request, runs as a pre-kernel, the
// batched hipFFT Z2Z plan in place on a scratch_pool buffer, and a post-kernel, in chunks of rows that keep the scratch bounded.
#include <dlfcn.h>
#if __has_include(<hipfft/hipfft.h>)
#include <hipfft/hipfft.h>
#else
// hipFFT's development headers are absent: the library is bound at run time anyway, and these are the only declarations of
// hipfft.h this file uses
typedef struct hipfftHandle_t* hipfftHandle;
typedef enum { HIPFFT_SUCCESS = 0 } hipfftResult;
typedef enum { HIPFFT_Z2Z = 0x69, HIPFFT_D2Z = 0x6a } hipfftType;
typedef double2 hipfftDoubleComplex;
typedef double hipfftDoubleReal;
#define HIPFFT_FORWARD -1
#endif
#include <string.h>

#include <atomic>
#include <cmath>
#include <mutex>

#include "common.hpp"
#include "scratch_pool.hpp"
#include "spectrum.hpp"

using namespace sdrhip;

namespace {

struct HipFft {
    void* handle = nullptr;
    hipfftResult (*PlanMany)(hipfftHandle*, int, int*, int*, int, int, int*, int, int, hipfftType, int) = nullptr;
    hipfftResult (*SetStream)(hipfftHandle, hipStream_t) = nullptr;
    hipfftResult (*ExecZ2Z)(hipfftHandle, hipfftDoubleComplex*, hipfftDoubleComplex*, int) = nullptr;
    hipfftResult (*ExecD2Z)(hipfftHandle, hipfftDoubleReal*, hipfftDoubleComplex*) = nullptr;
    hipfftResult (*Destroy)(hipfftHandle) = nullptr;
    std::string why;
};

HipFft* hipfft()
{
    static HipFft f;
    static std::once_flag once;
    std::call_once(once, [] {
        for (const char* n : {"libhipfft.so.0", "libhipfft.so", "/opt/rocm/lib/libhipfft.so.0"}) {
            f.handle = dlopen(n, RTLD_NOW | RTLD_LOCAL);
            if (f.handle) break;
        }
        if (!f.handle) {
            const char* e = dlerror();        // one call: it clears the message it returns
            f.why = e ? e : "libhipfft.so.0 not found";
            return;
        }
        bool ok = true;
#define SYM(field, name) do { *reinterpret_cast<void**>(&f.field) = dlsym(f.handle, name); if (!f.field) { ok = false; f.why = std::string("missing symbol ") + name; } } while (0)
        SYM(PlanMany, "hipfftPlanMany");
        SYM(SetStream, "hipfftSetStream");
        SYM(ExecZ2Z, "hipfftExecZ2Z");
        SYM(ExecD2Z, "hipfftExecD2Z");
        SYM(Destroy, "hipfftDestroy");
#undef SYM
        if (!ok) { dlclose(f.handle); f.handle = nullptr; }
    });
    return &f;
}

#define SDRHIP_CHECK_FFT(expr)                                                              \
    do {                                                                                    \
        hipfftResult _r = (expr);                                                           \
        if (_r != HIPFFT_SUCCESS) {                                                         \
            set_error("%s failed: hipfftResult %d (%s:%d)", #expr, (int)_r, __FILE__, __LINE__); \
            return SDRHIP_ERR_HIP;                                                          \
        }                                                                                   \
    } while (0)

}  // namespace

struct sdrhip_fft {
    int n = 0, batch = 1;
    bool real_in = false;
    hipfftHandle plan = 0;
    bool have_plan = false;
    hipStream_t stream = nullptr;      // for the host-vector entry point
    DevBuf din, dout;
    PinBuf hin, hout;
    size_t in_bytes() const { return (size_t)batch * n * (real_in ? 8 : 16); }
    size_t out_bytes() const { return (size_t)batch * (real_in ? n / 2 + 1 : n) * 16; }
    ~sdrhip_fft()
    {
        if (stream) (void)hipStreamSynchronize(stream);
        if (have_plan && hipfft()->handle) (void)hipfft()->Destroy(plan);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

extern "C" {

int sdrhip_fft_create(sdrhip_fft** out, int n, int real_input, int batch)
{
    SDRHIP_REQUIRE(out != nullptr && n >= 2 && n <= (1 << 27) && batch >= 1 && batch <= (1 << 20), "sdrhip_fft_create");
    *out = nullptr;
    HipFft* h = hipfft();
    if (!h->handle) {
        set_error("sdrhip_fft_create: hipFFT is not available (%s)", h->why.c_str());
        return SDRHIP_ERR_STATE;
    }
    sdrhip_fft* f = new sdrhip_fft();
    f->n = n;
    f->batch = batch;
    f->real_in = real_input != 0;
    int len[1] = {n};
    hipfftResult r = h->PlanMany(&f->plan, 1, len, nullptr, 1, n, nullptr, 1, f->real_in ? n / 2 + 1 : n,
                                 f->real_in ? HIPFFT_D2Z : HIPFFT_Z2Z, batch);
    if (r != HIPFFT_SUCCESS) {
        set_error("hipfftPlanMany(n = %d, batch = %d) failed: hipfftResult %d", n, batch, (int)r);
        delete f;
        return SDRHIP_ERR_HIP;
    }
    f->have_plan = true;
    *out = f;
    return SDRHIP_OK;
}

void sdrhip_fft_destroy(sdrhip_fft* f) { delete f; }
int sdrhip_fft_size(const sdrhip_fft* f) { return f ? f->n : -1; }
int sdrhip_fft_bins(const sdrhip_fft* f) { return f ? (f->real_in ? f->n / 2 + 1 : f->n) : -1; }

// device vectors, asynchronous on `stream`: d_in = batch x n complex doubles (or n doubles), d_out = batch x bins complex doubles
int sdrhip_fft_run_device(sdrhip_fft* f, void* stream, const double* d_in, double* d_out)
{
    SDRHIP_REQUIRE(f != nullptr && d_in != nullptr && d_out != nullptr, "sdrhip_fft_run_device");
    HipFft* h = hipfft();
    SDRHIP_CHECK_FFT(h->SetStream(f->plan, (hipStream_t)stream));
    if (f->real_in) SDRHIP_CHECK_FFT(h->ExecD2Z(f->plan, const_cast<double*>(d_in), reinterpret_cast<hipfftDoubleComplex*>(d_out)));
    else SDRHIP_CHECK_FFT(h->ExecZ2Z(f->plan, reinterpret_cast<hipfftDoubleComplex*>(const_cast<double*>(d_in)),
                                     reinterpret_cast<hipfftDoubleComplex*>(d_out), HIPFFT_FORWARD));
    return SDRHIP_OK;
}

// host vectors, synchronous: what fftw' / fftwReal' return (FFT.hs:44-108), `batch` transforms per call
int sdrhip_fft_run(sdrhip_fft* f, const double* in, double* out)
{
    SDRHIP_REQUIRE(f != nullptr && in != nullptr && out != nullptr, "sdrhip_fft_run");
    if (!f->stream) SDRHIP_CHECK_HIP(hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking));
    int rc;
    if ((rc = f->din.ensure(f->in_bytes())) != SDRHIP_OK) return rc;
    if ((rc = f->dout.ensure(f->out_bytes())) != SDRHIP_OK) return rc;
    if ((rc = f->hin.ensure(f->in_bytes())) != SDRHIP_OK) return rc;
    if ((rc = f->hout.ensure(f->out_bytes())) != SDRHIP_OK) return rc;
    memcpy(f->hin.p, in, f->in_bytes());
    SDRHIP_CHECK_HIP(hipMemcpyAsync(f->din.p, f->hin.p, f->in_bytes(), hipMemcpyHostToDevice, f->stream));
    if ((rc = sdrhip_fft_run_device(f, f->stream, (const double*)f->din.p, (double*)f->dout.p)) != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(f->hout.p, f->dout.p, f->out_bytes(), hipMemcpyDeviceToHost, f->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(f->stream));
    memcpy(out, f->hout.p, f->out_bytes());
    return SDRHIP_OK;
}

}  // extern "C"

// ---- the spectrum operator ---------------------------------------------------------------------------------------------------------
namespace {

std::atomic<long long> g_spectrum_fused_launches{0};

constexpr size_t SPECTRUM_SCRATCH_BYTES = (size_t)64 << 20;      // the hipFFT route's intermediate: at most this, or one row

struct SpectrumPlan {
    int batch = 0;
    hipfftHandle plan = 0;
};

}  // namespace

struct sdrhip_spectrum {
    int n = 0, format = 0, shift = 0, route = 0;
    double scale = 1.0;
    std::vector<double> window;
    DevBuf d_window, d_twiddle;
    bool uploaded = false;
    ScratchCtx* ctx = nullptr;             // leased on first need (host entry point, hipFFT route), held until destroy
    hipStream_t last_stream = nullptr;     // the stream of the last hipFFT-route run: drained before the scratch goes back
    bool ran_hipfft = false;
    std::vector<SpectrumPlan> plans;       // one per batch size in use: the chunk, and the last chunk of a run
    bool fused_size() const { return spectrum_fused_size(n); }
    bool takes_fused() const { return route == 1 || (route == 0 && fused_size()); }
    size_t sample_bytes() const { return format == SDRHIP_IQ_U8 ? 2 : 8; }
    ~sdrhip_spectrum()
    {
        if (ran_hipfft) (void)hipStreamSynchronize(last_stream);
        if (ctx) (void)hipStreamSynchronize(ctx->stream);
        for (SpectrumPlan& p : plans) (void)hipfft()->Destroy(p.plan);
        if (ctx) scratch_release(ctx);
    }
};

namespace {

int spectrum_upload(sdrhip_spectrum* s)
{
    if (s->uploaded) return SDRHIP_OK;
    int rc;
    if ((rc = s->d_window.ensure(s->window.size() * sizeof(double))) != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(hipMemcpy(s->d_window.p, s->window.data(), s->window.size() * sizeof(double), hipMemcpyHostToDevice));
    if (s->fused_size()) {
        // exp(-2 pi i m / n): computed in long double, rounded once
        std::vector<double> tw(2 * (size_t)s->n);
        const long double step = -2.0L * 3.14159265358979323846264338327950288L / (long double)s->n;
        for (int m = 0; m < s->n; m++) {
            tw[2 * m] = (double)cosl(step * m);
            tw[2 * m + 1] = (double)sinl(step * m);
        }
        if ((rc = s->d_twiddle.ensure(tw.size() * sizeof(double))) != SDRHIP_OK) return rc;
        SDRHIP_CHECK_HIP(hipMemcpy(s->d_twiddle.p, tw.data(), tw.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    s->uploaded = true;
    return SDRHIP_OK;
}

int spectrum_lease(sdrhip_spectrum* s)
{
    if (!s->ctx) s->ctx = scratch_acquire();
    return s->ctx ? SDRHIP_OK : SDRHIP_ERR_HIP;
}

int spectrum_plan(sdrhip_spectrum* s, int batch, hipfftHandle* out)
{
    HipFft* h = hipfft();
    for (SpectrumPlan& p : s->plans)
        if (p.batch == batch) {
            *out = p.plan;
            return SDRHIP_OK;
        }
    if (s->plans.size() >= 2) {            // keep the first (the full chunk); replace the other (a run's last chunk)
        (void)hipStreamSynchronize(s->last_stream);
        (void)h->Destroy(s->plans.back().plan);
        s->plans.pop_back();
    }
    SpectrumPlan p;
    p.batch = batch;
    int len[1] = {s->n};
    hipfftResult r = h->PlanMany(&p.plan, 1, len, nullptr, 1, s->n, nullptr, 1, s->n, HIPFFT_Z2Z, batch);
    if (r != HIPFFT_SUCCESS) {
        set_error("hipfftPlanMany(n = %d, batch = %d) failed: hipfftResult %d", s->n, batch, (int)r);
        return SDRHIP_ERR_HIP;
    }
    s->plans.push_back(p);
    *out = p.plan;
    return SDRHIP_OK;
}

int spectrum_run_hipfft(sdrhip_spectrum* s, hipStream_t stream, const SpectrumArgs& a, float* d_out)
{
    HipFft* h = hipfft();
    if (!h->handle) {
        set_error("sdrhip_spectrum_run_device: hipFFT is not available (%s)", h->why.c_str());
        return SDRHIP_ERR_STATE;
    }
    int rc;
    if ((rc = spectrum_lease(s)) != SDRHIP_OK) return rc;
    const size_t row_bytes = (size_t)s->n * sizeof(double2);
    int64_t chunk = (int64_t)(SPECTRUM_SCRATCH_BYTES / row_bytes);
    if (chunk < 1) chunk = 1;
    if (chunk > a.rows) chunk = a.rows;
    if (s->ran_hipfft && s->last_stream != stream) SDRHIP_CHECK_HIP(hipStreamSynchronize(s->last_stream));   // one scratch: runs take turns
    if ((rc = s->ctx->work.ensure((size_t)chunk * row_bytes)) != SDRHIP_OK) return rc;
    double2* work = static_cast<double2*>(s->ctx->work.p);
    s->last_stream = stream;
    s->ran_hipfft = true;
    for (int64_t row0 = 0; row0 < a.rows; row0 += chunk) {
        const int64_t nrows = a.rows - row0 < chunk ? a.rows - row0 : chunk;
        hipfftHandle plan;
        if ((rc = spectrum_plan(s, (int)nrows, &plan)) != SDRHIP_OK) return rc;
        SDRHIP_CHECK_HIP(launch_spectrum_prepare(stream, a, row0, nrows, work));
        SDRHIP_CHECK_FFT(h->SetStream(plan, stream));
        SDRHIP_CHECK_FFT(h->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex*>(work), reinterpret_cast<hipfftDoubleComplex*>(work), HIPFFT_FORWARD));
        SDRHIP_CHECK_HIP(launch_spectrum_magnitude(stream, work, nrows * s->n, s->scale, d_out + row0 * s->n));
    }
    return SDRHIP_OK;
}

}  // namespace

extern "C" {

int sdrhip_spectrum_create(sdrhip_spectrum** out, int n, int input_format, int window, const double* custom_window, int half_band_shift,
                           double scale)
{
    SDRHIP_REQUIRE(out != nullptr, "sdrhip_spectrum_create");
    *out = nullptr;
    SDRHIP_REQUIRE(n >= 2 && n <= (1 << 27), "sdrhip_spectrum_create");
    SDRHIP_REQUIRE(input_format == SDRHIP_IQ_U8 || input_format == SDRHIP_IQ_CF32, "sdrhip_spectrum_create");
    SDRHIP_REQUIRE(window >= SDRHIP_WINDOW_NONE && window <= SDRHIP_WINDOW_CUSTOM, "sdrhip_spectrum_create");
    SDRHIP_REQUIRE(window != SDRHIP_WINDOW_CUSTOM || custom_window != nullptr, "sdrhip_spectrum_create");
    sdrhip_spectrum* s = new sdrhip_spectrum();
    s->n = n;
    s->format = input_format;
    s->shift = half_band_shift != 0;
    s->scale = scale;
    s->window.resize(n);
    const double pi = 3.14159265358979323846, size = (double)n;
    for (int j = 0; j < n; j++) {
        const double idx = (double)j;
        double w = 1.0;
        switch (window) {                  // FilterDesign.hs:39-60, as written there
        case SDRHIP_WINDOW_HANNING: w = 0.5 * (1 - cos((2 * pi * idx) / (size - 1))); break;
        case SDRHIP_WINDOW_HAMMING: w = 0.54 - 0.46 * cos((2 * pi * idx) / (size - 1)); break;
        case SDRHIP_WINDOW_BLACKMAN: w = 0.42 - 0.5 * cos((2 * pi * idx) / (size - 1)) + 0.08 * cos((4 * pi * idx) / (size - 1)); break;
        case SDRHIP_WINDOW_CUSTOM: w = custom_window[j]; break;
        default: break;
        }
        s->window[j] = w;
    }
    *out = s;
    return SDRHIP_OK;
}

void sdrhip_spectrum_destroy(sdrhip_spectrum* s) { delete s; }
int sdrhip_spectrum_size(const sdrhip_spectrum* s) { return s ? s->n : -1; }

int sdrhip_spectrum_window(const sdrhip_spectrum* s, double* out)
{
    SDRHIP_REQUIRE(s != nullptr && out != nullptr, "sdrhip_spectrum_window");
    memcpy(out, s->window.data(), s->window.size() * sizeof(double));
    return SDRHIP_OK;
}

int sdrhip_spectrum_set_route(sdrhip_spectrum* s, int route)
{
    SDRHIP_REQUIRE(s != nullptr && route >= 0 && route <= 2, "sdrhip_spectrum_set_route");
    SDRHIP_REQUIRE(route != 1 || s->fused_size(), "sdrhip_spectrum_set_route (the one-kernel route serves powers of two from 64 to 8192)");
    s->route = route;
    return SDRHIP_OK;
}

long long sdrhip_debug_spectrum_fused_launches(void) { return g_spectrum_fused_launches.load(); }

int sdrhip_spectrum_run_device(sdrhip_spectrum* s, void* stream, const void* d_in, int64_t n_samples, int64_t hop, int rows, float* d_out)
{
    SDRHIP_REQUIRE(s != nullptr && d_in != nullptr && d_out != nullptr, "sdrhip_spectrum_run_device");
    SDRHIP_REQUIRE(rows >= 1 && hop >= 1 && n_samples >= s->n, "sdrhip_spectrum_run_device");
    SDRHIP_REQUIRE(rows == 1 || hop <= (n_samples - s->n) / (rows - 1), "sdrhip_spectrum_run_device: the last row must end inside the input");
    int rc;
    if ((rc = spectrum_upload(s)) != SDRHIP_OK) return rc;
    SpectrumArgs a;
    a.in = d_in;
    a.format = s->format;
    a.hop = hop;
    a.rows = rows;
    a.n = s->n;
    a.shift = s->shift;
    a.scale = s->scale;
    a.window = static_cast<const double*>(s->d_window.p);
    a.twiddle = static_cast<const double2*>(s->d_twiddle.p);
    if (!s->takes_fused()) return spectrum_run_hipfft(s, (hipStream_t)stream, a, d_out);
    SDRHIP_CHECK_HIP(launch_spectrum_fused((hipStream_t)stream, a, d_out));
    g_spectrum_fused_launches.fetch_add(1);
    return SDRHIP_OK;
}

int sdrhip_spectrum_run(sdrhip_spectrum* s, const void* in, int64_t n_samples, int64_t hop, int rows, float* out)
{
    SDRHIP_REQUIRE(s != nullptr && in != nullptr && out != nullptr, "sdrhip_spectrum_run");
    SDRHIP_REQUIRE(rows >= 1 && hop >= 1 && n_samples >= s->n, "sdrhip_spectrum_run");
    SDRHIP_REQUIRE(rows == 1 || hop <= (n_samples - s->n) / (rows - 1), "sdrhip_spectrum_run: the last row must end inside the input");
    int rc;
    if ((rc = spectrum_lease(s)) != SDRHIP_OK) return rc;
    ScratchCtx* c = s->ctx;
    const size_t in_bytes = (size_t)n_samples * s->sample_bytes(), out_bytes = (size_t)rows * s->n * sizeof(float);
    if ((rc = c->in.ensure(in_bytes)) != SDRHIP_OK) return rc;
    if ((rc = c->out.ensure(out_bytes)) != SDRHIP_OK) return rc;
    if ((rc = c->hin.ensure(in_bytes)) != SDRHIP_OK) return rc;
    if ((rc = c->hout.ensure(out_bytes)) != SDRHIP_OK) return rc;
    memcpy(c->hin.p, in, in_bytes);
    SDRHIP_CHECK_HIP(hipMemcpyAsync(c->in.p, c->hin.p, in_bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = sdrhip_spectrum_run_device(s, c->stream, c->in.p, n_samples, hop, rows, static_cast<float*>(c->out.p))) != SDRHIP_OK) return rc;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(c->hout.p, c->out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(c->stream));
    memcpy(out, c->hout.p, out_bytes);
    return SDRHIP_OK;
}

}  // extern "C"
