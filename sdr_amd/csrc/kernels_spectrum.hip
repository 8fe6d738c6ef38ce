// kernels_spectrum.hip -- the spectrum operator (include/sdr_hip.h, sdrhip_spectrum_*): raw IQ -> windowed FFT magnitudes.
//
// The reference's waterfall pipe is interleavedIQUnsigned256ToFloat (Util.hs:92-98) -> halfBandUp (Util.hs:264-271) x a window
// (FilterDesign.hs:39-60) -> fftw (FFT.hs:44-76) -> magnitude, a scale -> SDR.Plot.  Row r of the output is
//     out[r][k] = (float)(scale * |sum_j x[r hop + j] s(j) w[j] exp(-2 pi i jk/n)|),   s(j) = (-1)^j with the shift, else 1
// in double throughout, like the reference.  Contract: a tolerance (tests/test_gpu_spectrum.py), not bit parity.
//
// ONE-KERNEL ROUTE (spectrum_fused): power-of-two n from 64 to 8192.  A workgroup of T threads holds a tile of E = 8 T complex
// doubles in LDS: one row of n = E points, or E / n rows when n is smaller (T = 256: 2048 points, so 32 rows of 64 share a workgroup),
// and loops over the tiles of the launch.  n = 8192 takes T = 1024 and 128 KiB of the CU's 160 KiB: this toolchain grants a single
// workgroup that much as a static allocation, so the route serves 8192 too.  HBM sees the raw samples once (2 B or 8 B each) and the
// float32 magnitudes once (4 B each); the window (8 n B) and the twiddle table (16 n B) are shared by every row and come from L2.
//
// The transform is a Stockham autosort FFT, decimation in time: radix-4 passes with p = 1, 4, 16, ... and, when log2 n is odd, one
// radix-2 pass at the end.  In the pass with sub-transform length p, butterfly i (k = i mod p) reads points i + r n/4, multiplies by
// exp(-2 pi i k r / (4 p)) and writes its outputs to 4 (i - k) + k + r p.  There is one LDS array, not two: every thread reads the
// inputs of its butterflies into registers, the workgroup meets at a barrier, and only then are the outputs written.  The first pass
// reads global memory (convert, sign, window) and the last one writes it (magnitude, scale, float32), so a tile crosses LDS
// log4(n) - 1 times.  Twiddles come from a table the host computed in double (no device sincos).
//
// Bank conflicts (16-byte elements): consecutive lanes own consecutive butterflies, so every LDS READ of a pass is a run of
// consecutive 16-byte elements -- conflict-free under ds_read_b128's lane groups, which is why the array is NOT padded: a pad would put
// conflicts into the reads of every pass.  WRITES go out at stride p elements within a butterfly and 4 elements from lane to lane
// while lanes share k: for p >= 8 the eight lanes of a store's lane group write eight consecutive elements (conflict-free); the pass
// p = 1 writes at a 64-byte lane stride (4 lanes of 8 on one bank group) and p = 4 at a 2-way conflict.  Those are two of the six LDS
// write passes at n = 8192, one of which would also exist with padding (a pad of one element per 8 leaves p = 4 at 2-way).
//
// No atomics, no state across workgroups: a row's bits depend on its samples alone, whatever its place in a batch (the same
// butterflies in the same order, whichever thread of whichever tile slot runs them; -ffp-contract=off as everywhere).
//
// HIPFFT ROUTE (every other n, or on request): spectrum_prepare writes the converted, signed, windowed rows as complex doubles,
// hipFFT transforms them in place, spectrum_magnitude takes scale * |X| to float32.
#include "spectrum.hpp"

namespace sdrhip {

namespace {

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// sample `idx` of the input as a complex double.  A row starts wherever hop puts it, so `wide` (the base pointer allows one load per
// sample: 2-byte aligned u8, 8-byte aligned float32) is decided per launch and the narrow loads serve every other base.
template <int FMT>
__device__ __forceinline__ double2 load_sample(const void* in, int64_t idx, bool wide)
{
    if (FMT == 0) {
        const unsigned char* p = static_cast<const unsigned char*>(in) + 2 * idx;
        unsigned re, im;
        if (wide) {
            const unsigned v = *reinterpret_cast<const unsigned short*>(p);
            re = v & 0xffu;
            im = v >> 8;
        } else {
            re = p[0];
            im = p[1];
        }
        return make_double2(((double)re - 128.0) / 128.0, ((double)im - 128.0) / 128.0);
    } else {
        const float* p = static_cast<const float*>(in) + 2 * idx;
        if (wide) {
            const float2 v = *reinterpret_cast<const float2*>(p);
            return make_double2((double)v.x, (double)v.y);
        }
        return make_double2((double)p[0], (double)p[1]);
    }
}

// forward radix-4 butterfly (exp(-2 pi i / 4) = -i), in place
__device__ __forceinline__ void radix4(double2 (&u)[4])
{
    const double2 a = cadd(u[0], u[2]), b = csub(u[0], u[2]), c = cadd(u[1], u[3]), d = csub(u[1], u[3]);
    const double2 dr = make_double2(d.y, -d.x);      // -i d
    u[0] = cadd(a, c);
    u[1] = cadd(b, dr);
    u[2] = csub(a, c);
    u[3] = csub(b, dr);
}

__device__ __forceinline__ float magnitude(double2 v, double scale) { return (float)(scale * sqrt(v.x * v.x + v.y * v.y)); }

template <int T, int FMT>
__global__ __launch_bounds__(T) void spectrum_fused(const void* __restrict__ in, int64_t hop, int64_t rows, int lg, int shift, double scale,
                                                    const double* __restrict__ window, const double2* __restrict__ twiddle, bool wide,
                                                    float* __restrict__ out)
{
    constexpr int E = 8 * T;                 // complex doubles per tile
    __shared__ double2 s[E];
    const int n = 1 << lg, q = n >> 2, lgq = lg - 2;
    const int rows_per_tile = E >> lg;
    const int64_t ntiles = (rows + rows_per_tile - 1) / rows_per_tile;
    const int passes4 = lg >> 1;
    const bool odd = (lg & 1) != 0;
    const int tid = threadIdx.x;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * rows_per_tile;

        // pass p = 1: global memory -> LDS.  Butterfly g = tid + b T of the tile is butterfly i of the tile's row rl.
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int g = tid + b * T, rl = g >> lgq, i = g & (q - 1);
            const int64_t row = row0 + rl;
            double2 u[4];
            if (row < rows) {
                const double sign = (shift && (i & 1)) ? -1.0 : 1.0;      // q is even: the parity of i + r q is that of i
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int j = i + r * q;
                    const double2 x = load_sample<FMT>(in, row * hop + j, wide);
                    const double w = sign * window[j];
                    u[r] = make_double2(x.x * w, x.y * w);
                }
            } else {
#pragma unroll
                for (int r = 0; r < 4; r++) u[r] = make_double2(0.0, 0.0);
            }
            radix4(u);
            double2* dst = s + (rl << lg) + 4 * i;
#pragma unroll
            for (int r = 0; r < 4; r++) dst[r] = u[r];
        }
        __syncthreads();

        // radix-4 passes p = 4, 16, ... that stay in LDS: LDS -> registers, barrier, registers -> LDS
        const int mid_end = odd ? passes4 : passes4 - 1;
#pragma unroll 1
        for (int ps = 1; ps < mid_end; ps++) {
            const int lgp = 2 * ps, p = 1 << lgp;
            double2 u[2][4];
            int rl[2], i[2];
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int g = tid + b * T;
                rl[b] = g >> lgq;
                i[b] = g & (q - 1);
                const double2* src = s + (rl[b] << lg) + i[b];
#pragma unroll
                for (int r = 0; r < 4; r++) u[b][r] = src[r * q];
            }
            __syncthreads();
#pragma unroll
            for (int b = 0; b < 2; b++) {
                const int k = i[b] & (p - 1);
                const int tw = k << (lgq - lgp);             // k n / (4 p)
                u[b][1] = cmul(u[b][1], twiddle[tw]);
                u[b][2] = cmul(u[b][2], twiddle[2 * tw]);
                u[b][3] = cmul(u[b][3], twiddle[3 * tw]);
                radix4(u[b]);
                double2* dst = s + (rl[b] << lg) + ((i[b] - k) << 2) + k;
#pragma unroll
                for (int r = 0; r < 4; r++) dst[r << lgp] = u[b][r];
            }
            __syncthreads();
        }

        // log2 n even: the last radix-4 pass p = n / 4, LDS -> global memory.  k = i: butterfly i holds bins i + r n/4.
        if (!odd) {
#pragma unroll 1
            for (int b = 0; b < 2; b++) {
                const int g = tid + b * T, rl = g >> lgq, i = g & (q - 1);
                if (row0 + rl >= rows) continue;
                const double2* src = s + (rl << lg) + i;
                double2 u[4];
                u[0] = src[0];
                u[1] = cmul(src[q], twiddle[i]);
                u[2] = cmul(src[2 * q], twiddle[2 * i]);
                u[3] = cmul(src[3 * q], twiddle[3 * i]);
                radix4(u);
                float* o = out + (row0 + rl) * n + i;
#pragma unroll
                for (int r = 0; r < 4; r++) o[r * q] = magnitude(u[r], scale);
            }
        }

        // log2 n odd: the radix-2 pass p = n / 2, LDS -> global memory.  Butterfly i holds bins i and i + n/2.
        if (odd) {
            const int h = n >> 1;
#pragma unroll 1
            for (int b = 0; b < 4; b++) {
                const int g = tid + b * T, rl = g >> (lg - 1), i = g & (h - 1);
                const double2* src = s + (rl << lg) + i;
                const double2 u0 = src[0], u1 = cmul(src[h], twiddle[i]);
                if (row0 + rl < rows) {
                    float* o = out + (row0 + rl) * n + i;
                    o[0] = magnitude(cadd(u0, u1), scale);
                    o[h] = magnitude(csub(u0, u1), scale);
                }
            }
        }
        __syncthreads();        // the next tile's first pass overwrites what this tile's last pass reads
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void spectrum_prepare(const void* __restrict__ in, int64_t hop, int64_t row0, int64_t nrows, int n, int shift,
                                                        const double* __restrict__ window, bool wide, double2* __restrict__ work)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double w = ((shift && (j & 1)) ? -1.0 : 1.0) * window[j];
    for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const double2 x = load_sample<FMT>(in, (row0 + r) * hop + j, wide);
        work[r * n + j] = make_double2(x.x * w, x.y * w);
    }
}

__global__ __launch_bounds__(256) void spectrum_magnitude(const double2* __restrict__ work, int64_t count, double scale, float* __restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < count; k += (int64_t)gridDim.x * 256) out[k] = magnitude(work[k], scale);
}

bool wide_loads(const SpectrumArgs& a) { return ((uintptr_t)a.in & (a.format == 0 ? 1u : 7u)) == 0; }

template <int T>
hipError_t launch_fused(hipStream_t stream, const SpectrumArgs& a, int lg, float* out)
{
    const int rows_per_tile = (8 * T) >> lg;
    const int64_t ntiles = (a.rows + rows_per_tile - 1) / rows_per_tile;
    const int64_t resident = 2048;           // 8 workgroups on each of 256 CUs: more tiles than that loop inside the launch
    const unsigned grid = (unsigned)(ntiles < resident ? ntiles : resident);
    if (a.format == 0)
        spectrum_fused<T, 0><<<grid, T, 0, stream>>>(a.in, a.hop, a.rows, lg, a.shift, a.scale, a.window, a.twiddle, wide_loads(a), out);
    else
        spectrum_fused<T, 1><<<grid, T, 0, stream>>>(a.in, a.hop, a.rows, lg, a.shift, a.scale, a.window, a.twiddle, wide_loads(a), out);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_spectrum_fused(hipStream_t stream, const SpectrumArgs& a, float* out)
{
    if (!spectrum_fused_size(a.n) || a.rows < 1) return hipErrorInvalidValue;
    int lg = 0;
    while ((1 << lg) < a.n) lg++;
    if (a.n == 8192) return launch_fused<1024>(stream, a, lg, out);
    if (a.n == 4096) return launch_fused<512>(stream, a, lg, out);
    return launch_fused<256>(stream, a, lg, out);
}

hipError_t launch_spectrum_prepare(hipStream_t stream, const SpectrumArgs& a, int64_t row0, int64_t nrows, double2* work)
{
    const dim3 grid((unsigned)((a.n + 255) / 256), (unsigned)(nrows < 4096 ? nrows : 4096));
    if (a.format == 0)
        spectrum_prepare<0><<<grid, 256, 0, stream>>>(a.in, a.hop, row0, nrows, a.n, a.shift, a.window, wide_loads(a), work);
    else
        spectrum_prepare<1><<<grid, 256, 0, stream>>>(a.in, a.hop, row0, nrows, a.n, a.shift, a.window, wide_loads(a), work);
    return hipGetLastError();
}

hipError_t launch_spectrum_magnitude(hipStream_t stream, const double2* work, int64_t count, double scale, float* out)
{
    const int64_t blocks = (count + 255) / 256;
    spectrum_magnitude<<<(unsigned)(blocks < 16384 ? blocks : 16384), 256, 0, stream>>>(work, count, scale, out);
    return hipGetLastError();
}

}  // namespace sdrhip
