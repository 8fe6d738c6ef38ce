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
// (u8 as Util.hs:92-98 converts it, int16 as convert.c:52-85 does, or float32) x halfBandUp (Util.hs:264-271) x a window (FilterDesign.hs:39-60) -> DFT -> scale * |X|
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
std::atomic<long long> g_spectrum_reduce_split_launches{0};
std::atomic<long long> g_spectrum_hipfft_batches{0};               // ExecZ2Z calls of the operator: one per chunk / batch of rows
std::atomic<long long> g_spectrum_reduce_layer_launches{0};        // layered spectrum_fused_reduce launches: one per (row slice, chunk slice)

constexpr size_t SPECTRUM_SCRATCH_BYTES = (size_t)64 << 20;      // the hipFFT route's intermediate: at most this, or one row

struct SpectrumPlan {
    int batch = 0;
    hipfftHandle plan = 0;
};

}  // namespace

struct sdrhip_spectrum {
    int n = 0, format = 0, shift = 0, route = 0;
    int reduce_split = 0;                  // 0 = auto, 1 = never, 2 = always
    double scale = 1.0;
    std::vector<double> window;
    DevBuf d_window, d_twiddle;
    bool uploaded = false;
    ScratchCtx* ctx = nullptr;             // leased on first need (host entry point, hipFFT route), held until destroy
    hipStream_t last_stream = nullptr;     // the stream of the last run that used ctx->work: drained before the scratch goes back
    bool ran_hipfft = false;               // ... and whether there was one (the hipFFT route, or a reduction through layers)
    std::vector<SpectrumPlan> plans;       // one per batch size in use: the chunk, and the last chunk of a run
    bool fused_size() const { return spectrum_fused_size(n); }
    bool takes_fused() const { return route == 1 || (route == 0 && fused_size()); }
    size_t sample_bytes() const { return format == SDRHIP_IQ_U8 ? 2 : format == SDRHIP_IQ_I16 ? 4 : 8; }
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

// ctx->work for a run on `stream`, at least `bytes` large.  There is one such buffer: a run on another stream waits for the last one.
int spectrum_take_work(sdrhip_spectrum* s, hipStream_t stream, size_t bytes)
{
    int rc;
    if ((rc = spectrum_lease(s)) != SDRHIP_OK) return rc;
    if (s->ran_hipfft && s->last_stream != stream) SDRHIP_CHECK_HIP(hipStreamSynchronize(s->last_stream));
    if ((rc = s->ctx->work.ensure(bytes)) != SDRHIP_OK) return rc;
    s->last_stream = stream;
    s->ran_hipfft = true;
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
    if ((rc = spectrum_take_work(s, stream, (size_t)chunk * row_bytes)) != SDRHIP_OK) return rc;
    double2* work = static_cast<double2*>(s->ctx->work.p);
    for (int64_t row0 = 0; row0 < a.rows; row0 += chunk) {
        const int64_t nrows = a.rows - row0 < chunk ? a.rows - row0 : chunk;
        hipfftHandle plan;
        if ((rc = spectrum_plan(s, (int)nrows, &plan)) != SDRHIP_OK) return rc;
        SDRHIP_CHECK_HIP(launch_spectrum_prepare(stream, a, row0, nrows, work));
        SDRHIP_CHECK_FFT(h->SetStream(plan, stream));
        SDRHIP_CHECK_FFT(h->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex*>(work), reinterpret_cast<hipfftDoubleComplex*>(work), HIPFFT_FORWARD));
        g_spectrum_hipfft_batches.fetch_add(1);
        SDRHIP_CHECK_HIP(launch_spectrum_magnitude(stream, work, nrows * s->n, s->scale, d_out + row0 * s->n));
    }
    return SDRHIP_OK;
}

// ---- the reducing form -----------------------------------------------------------------------------------------------------------
// Work items a layered launch is spread over when it splits: 4 per CU of a 256-CU chip.  A guess, like the rule that `auto` splits
// when the output tiles alone are fewer than the CUs: tools/spectrum_reduce_bench.py is there to set both.
constexpr int64_t SPECTRUM_SPLIT_ITEMS = 1024;
constexpr int64_t SPECTRUM_CHIP_CUS = 256;

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the input `rows` output rows further on (a.rows is set by the caller)
SpectrumArgs spectrum_args_from(const sdrhip_spectrum* s, const SpectrumArgs& a, int64_t rows, int group)
{
    SpectrumArgs b = a;
    b.in = static_cast<const unsigned char*>(a.in) + (size_t)(rows * group * a.hop) * s->sample_bytes();
    return b;
}

// One-kernel route.  A group of one chunk leaves the kernel as floats.  A longer one goes through layers of chunk sums in ctx->work
// and the finalise kernel, in slices of output rows and of chunks that keep the scratch inside SPECTRUM_SCRATCH_BYTES: rows are
// independent of each other and the total is carried from slice to slice in the defined order, so the slicing changes no bit.
int spectrum_reduce_fused(sdrhip_spectrum* s, hipStream_t stream, const SpectrumArgs& a, int rows_out, const SpectrumReduce& f, float* d_out)
{
    const int n = s->n;
    if (f.group <= SPECTRUM_REDUCE_CHUNK) {
        SDRHIP_CHECK_HIP(launch_spectrum_fused_reduce(stream, a, f, 0, 1, 1, nullptr, d_out));
        g_spectrum_fused_launches.fetch_add(1);
        return SDRHIP_OK;
    }
    const int rows_per_tile = n >= 2048 ? 1 : 2048 / n;
    const int nchunks = (int)ceil_div(f.group, SPECTRUM_REDUCE_CHUNK);
    const size_t row_bytes = (size_t)n * sizeof(double);
    // a sixteenth of the scratch for the carried totals of a row slice (whole tiles, at least one row), the rest for its layers
    int64_t rows_slice = (int64_t)(SPECTRUM_SCRATCH_BYTES / 16 / row_bytes);
    if (rows_slice > rows_per_tile) rows_slice -= rows_slice % rows_per_tile;
    if (rows_slice < 1) rows_slice = 1;
    if (rows_slice > rows_out) rows_slice = rows_out;
    int64_t layers_slice = (int64_t)(SPECTRUM_SCRATCH_BYTES / (rows_slice * row_bytes)) - 1;
    if (layers_slice < 1) layers_slice = 1;
    if (layers_slice > nchunks) layers_slice = nchunks;
    const int64_t tiles_all = ceil_div(rows_out, rows_per_tile);
    const bool split = s->reduce_split == 2 || (s->reduce_split == 0 && tiles_all < SPECTRUM_CHIP_CUS);
    int rc;
    if ((rc = spectrum_take_work(s, stream, (size_t)rows_slice * row_bytes * (size_t)(1 + layers_slice))) != SDRHIP_OK) return rc;
    double* total = static_cast<double*>(s->ctx->work.p);
    double* partial = total + rows_slice * n;
    for (int64_t r0 = 0; r0 < rows_out; r0 += rows_slice) {
        SpectrumArgs b = spectrum_args_from(s, a, r0, f.group);
        b.rows = rows_out - r0 < rows_slice ? rows_out - r0 : rows_slice;
        const int64_t tiles = ceil_div(b.rows, rows_per_tile);
        for (int c0 = 0; c0 < nchunks; c0 += (int)layers_slice) {
            const int c1 = c0 + layers_slice < nchunks ? c0 + (int)layers_slice : nchunks;
            int per_item = c1 - c0;                     // not split: a tile's chunks stay with one workgroup
            if (split) per_item = (int)ceil_div(c1 - c0, ceil_div(SPECTRUM_SPLIT_ITEMS, tiles));
            SDRHIP_CHECK_HIP(launch_spectrum_fused_reduce(stream, b, f, c0, c1, per_item, partial, nullptr));
            g_spectrum_reduce_layer_launches.fetch_add(1);
            SDRHIP_CHECK_HIP(launch_spectrum_reduce_finalise(stream, partial, c1 - c0, b.rows * n, total, c0 == 0, c1 == nchunks, f, d_out + r0 * n));
        }
    }
    g_spectrum_fused_launches.fetch_add(1);
    if (split) g_spectrum_reduce_split_launches.fetch_add(1);
    return SDRHIP_OK;
}

// hipFFT route: half the scratch for the state of a slice of output rows (two doubles per bin), half for the batches of its input rows
int spectrum_reduce_hipfft(sdrhip_spectrum* s, hipStream_t stream, const SpectrumArgs& a, int rows_out, const SpectrumReduce& f, float* d_out)
{
    HipFft* h = hipfft();
    if (!h->handle) {
        set_error("sdrhip_spectrum_reduce_run_device: hipFFT is not available (%s)", h->why.c_str());
        return SDRHIP_ERR_STATE;
    }
    const int n = s->n;
    const size_t state_row = 2 * (size_t)n * sizeof(double), work_row = (size_t)n * sizeof(double2);
    int64_t rows_slice = (int64_t)(SPECTRUM_SCRATCH_BYTES / 2 / state_row);
    if (rows_slice < 1) rows_slice = 1;
    if (rows_slice > rows_out) rows_slice = rows_out;
    int64_t batch = (int64_t)(SPECTRUM_SCRATCH_BYTES / 2 / work_row);
    if (batch < 1) batch = 1;
    if (batch > rows_slice * f.group) batch = rows_slice * f.group;
    int rc;
    if ((rc = spectrum_take_work(s, stream, (size_t)rows_slice * state_row + (size_t)batch * work_row)) != SDRHIP_OK) return rc;
    double* chunk = static_cast<double*>(s->ctx->work.p);
    double* total = chunk + rows_slice * n;
    double2* work = reinterpret_cast<double2*>(total + rows_slice * n);
    for (int64_t r0 = 0; r0 < rows_out; r0 += rows_slice) {
        const int64_t nr = rows_out - r0 < rows_slice ? rows_out - r0 : rows_slice;
        const int64_t in_rows = nr * f.group;
        for (int64_t b0 = 0; b0 < in_rows; b0 += batch) {
            const int64_t nrows = in_rows - b0 < batch ? in_rows - b0 : batch;
            hipfftHandle plan;
            if ((rc = spectrum_plan(s, (int)nrows, &plan)) != SDRHIP_OK) return rc;
            SDRHIP_CHECK_HIP(launch_spectrum_prepare(stream, a, r0 * f.group + b0, nrows, work));
            SDRHIP_CHECK_FFT(h->SetStream(plan, stream));
            SDRHIP_CHECK_FFT(h->ExecZ2Z(plan, reinterpret_cast<hipfftDoubleComplex*>(work), reinterpret_cast<hipfftDoubleComplex*>(work), HIPFFT_FORWARD));
        g_spectrum_hipfft_batches.fetch_add(1);
            SDRHIP_CHECK_HIP(launch_spectrum_accumulate(stream, work, b0, nrows, n, s->scale, f, chunk, total, d_out + r0 * n));
        }
    }
    return SDRHIP_OK;
}

// what both reduce entry points require of their arguments
bool spectrum_reduce_args_ok(const sdrhip_spectrum* s, int64_t n_samples, int64_t hop, int rows_out, int group, int reduce, int unit, double floor_db)
{
    if (rows_out < 1 || group < 1 || hop < 1 || n_samples < s->n) return false;
    if ((int64_t)rows_out * group > 2147483647LL) return false;
    const int64_t rows = (int64_t)rows_out * group;
    if (rows > 1 && hop > (n_samples - s->n) / (rows - 1)) return false;      // (rows - 1) hop + n <= n_samples, without overflow
    if (reduce < SDRHIP_REDUCE_MEAN_POWER || reduce > SDRHIP_REDUCE_MAX_MAGNITUDE) return false;
    if (unit != SDRHIP_UNIT_LINEAR && unit != SDRHIP_UNIT_DB) return false;
    return std::isfinite(floor_db);
}

}  // namespace

extern "C" {

int sdrhip_spectrum_create(sdrhip_spectrum** out, int n, int input_format, int window, const double* custom_window, int half_band_shift,
                           double scale)
{
    SDRHIP_REQUIRE(out != nullptr, "sdrhip_spectrum_create");
    *out = nullptr;
    SDRHIP_REQUIRE(n >= 2 && n <= (1 << 27), "sdrhip_spectrum_create");
    SDRHIP_REQUIRE(input_format == SDRHIP_IQ_U8 || input_format == SDRHIP_IQ_CF32 || input_format == SDRHIP_IQ_I16, "sdrhip_spectrum_create");
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
long long sdrhip_debug_spectrum_hipfft_batches(void) { return g_spectrum_hipfft_batches.load(); }
long long sdrhip_debug_spectrum_reduce_layer_launches(void) { return g_spectrum_reduce_layer_launches.load(); }

int sdrhip_spectrum_run_device(sdrhip_spectrum* s, void* stream, const void* d_in, int64_t n_samples, int64_t hop, int rows, float* d_out)
{
    SDRHIP_REQUIRE(s != nullptr && d_in != nullptr && d_out != nullptr, "sdrhip_spectrum_run_device");
    SDRHIP_REQUIRE(rows >= 1 && hop >= 1 && n_samples >= s->n, "sdrhip_spectrum_run_device");
    SDRHIP_REQUIRE(rows == 1 || hop <= (n_samples - s->n) / (rows - 1), "sdrhip_spectrum_run_device: the last row must end inside the input");
    SDRHIP_REQUIRE(s->format != SDRHIP_IQ_I16 || ((uintptr_t)d_in & 1u) == 0, "sdrhip_spectrum_run_device: int16 input at an odd address");
    SDRHIP_REQUIRE(s->format != SDRHIP_IQ_CF32 || ((uintptr_t)d_in & 3u) == 0, "sdrhip_spectrum_run_device: float32 input at an address that is not a multiple of 4");
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

// ---- the reducing form: mean power / mean magnitude / max hold over `group` consecutive rows, on the device ---------------------------
extern "C" {

int sdrhip_spectrum_set_reduce_split(sdrhip_spectrum* s, int mode)
{
    SDRHIP_REQUIRE(s != nullptr && mode >= 0 && mode <= 2, "sdrhip_spectrum_set_reduce_split");
    s->reduce_split = mode;
    return SDRHIP_OK;
}

long long sdrhip_debug_spectrum_reduce_split_launches(void) { return g_spectrum_reduce_split_launches.load(); }

}  // extern "C"

// what the waterfall Pipe (pipes_spectrum.cpp) asks of the object it borrows
namespace sdrhip {
int spectrum_size_of(const sdrhip_spectrum* s) { return s->n; }
int spectrum_format_of(const sdrhip_spectrum* s) { return s->format; }
bool spectrum_reduce_uses_scratch(const sdrhip_spectrum* s, int group) { return !s->takes_fused() || group > SPECTRUM_REDUCE_CHUNK; }
// `stream` is about to be destroyed: if the scratch was last used on it, drain it now, so that neither the next run nor the object's
// destructor waits on a stream that no longer exists
void spectrum_forget_stream(sdrhip_spectrum* s, hipStream_t stream)
{
    if (!s->ran_hipfft || s->last_stream != stream) return;
    (void)hipStreamSynchronize(stream);
    s->ran_hipfft = false;
    s->last_stream = nullptr;
}
}  // namespace sdrhip

extern "C" {

int sdrhip_spectrum_reduce_run_device(sdrhip_spectrum* s, void* stream, const void* d_in, int64_t n_samples, int64_t hop, int rows_out, int group,
                                      int reduce, int unit, double floor_db, float* d_out)
{
    SDRHIP_REQUIRE(s != nullptr && d_in != nullptr && d_out != nullptr, "sdrhip_spectrum_reduce_run_device");
    SDRHIP_REQUIRE(spectrum_reduce_args_ok(s, n_samples, hop, rows_out, group, reduce, unit, floor_db), "sdrhip_spectrum_reduce_run_device");
    SDRHIP_REQUIRE(s->format != SDRHIP_IQ_I16 || ((uintptr_t)d_in & 1u) == 0, "sdrhip_spectrum_reduce_run_device: int16 input at an odd address");
    SDRHIP_REQUIRE(s->format != SDRHIP_IQ_CF32 || ((uintptr_t)d_in & 3u) == 0,
                   "sdrhip_spectrum_reduce_run_device: float32 input at an address that is not a multiple of 4");
    int rc;
    if ((rc = spectrum_upload(s)) != SDRHIP_OK) return rc;
    SpectrumArgs a;
    a.in = d_in;
    a.format = s->format;
    a.hop = hop;
    a.rows = rows_out;
    a.n = s->n;
    a.shift = s->shift;
    a.scale = s->scale;
    a.window = static_cast<const double*>(s->d_window.p);
    a.twiddle = static_cast<const double2*>(s->d_twiddle.p);
    SpectrumReduce f;
    f.group = group;
    f.reduce = reduce;
    f.unit = unit;
    f.floor_db = floor_db;
    if (!s->takes_fused()) return spectrum_reduce_hipfft(s, (hipStream_t)stream, a, rows_out, f, d_out);
    return spectrum_reduce_fused(s, (hipStream_t)stream, a, rows_out, f, d_out);
}

int sdrhip_spectrum_reduce_run(sdrhip_spectrum* s, const void* in, int64_t n_samples, int64_t hop, int rows_out, int group, int reduce, int unit,
                               double floor_db, float* out)
{
    SDRHIP_REQUIRE(s != nullptr && in != nullptr && out != nullptr, "sdrhip_spectrum_reduce_run");
    SDRHIP_REQUIRE(spectrum_reduce_args_ok(s, n_samples, hop, rows_out, group, reduce, unit, floor_db), "sdrhip_spectrum_reduce_run");
    int rc;
    if ((rc = spectrum_lease(s)) != SDRHIP_OK) return rc;
    ScratchCtx* c = s->ctx;
    const size_t in_bytes = (size_t)n_samples * s->sample_bytes(), out_bytes = (size_t)rows_out * s->n * sizeof(float);
    if ((rc = c->in.ensure(in_bytes)) != SDRHIP_OK) return rc;
    if ((rc = c->out.ensure(out_bytes)) != SDRHIP_OK) return rc;
    if ((rc = c->hin.ensure(in_bytes)) != SDRHIP_OK) return rc;
    if ((rc = c->hout.ensure(out_bytes)) != SDRHIP_OK) return rc;
    memcpy(c->hin.p, in, in_bytes);
    SDRHIP_CHECK_HIP(hipMemcpyAsync(c->in.p, c->hin.p, in_bytes, hipMemcpyHostToDevice, c->stream));
    if ((rc = sdrhip_spectrum_reduce_run_device(s, c->stream, c->in.p, n_samples, hop, rows_out, group, reduce, unit, floor_db,
                                                static_cast<float*>(c->out.p))) != SDRHIP_OK)
        return rc;
    SDRHIP_CHECK_HIP(hipMemcpyAsync(c->hout.p, c->out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    SDRHIP_CHECK_HIP(hipStreamSynchronize(c->stream));
    memcpy(out, c->hout.p, out_bytes);
    return SDRHIP_OK;
}

}  // extern "C"
