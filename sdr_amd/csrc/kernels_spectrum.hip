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
//
// REDUCING FORM (sdrhip_spectrum_reduce_*: mean power, mean magnitude or max hold over `group` consecutive rows, linear or dB):
// spectrum_fused_reduce runs the passes above once per input row and keeps the last pass's magnitudes in registers, so the full-rate
// rows never reach memory; with few output rows and a long group the split form spreads a group's 32-row chunks over workgroups and
// spectrum_reduce_finalise adds them up.  The hipFFT route adds each batch into two doubles of state per output bin
// (spectrum_accumulate).  All three follow the summation order the header defines; the first two give the same bits.
#include "spectrum.hpp"

namespace sdrhip {

namespace {

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }

// sample `idx` of the input as a complex double.  A row starts wherever hop puts it, so `wide` (the base pointer allows one load per
// sample: 2-byte aligned u8, 8-byte aligned float32, 4-byte aligned int16) is decided per launch and the narrow loads serve every
// other base.  int16 is c(s) = s * 2^-11 over the whole range (the BladeRF conversion, convert.c:52-85): exact in double.
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
    } else if (FMT == 2) {
        const unsigned char* p = static_cast<const unsigned char*>(in) + 4 * idx;
        int re, im;
        if (wide) {
            const uint32_t w = *reinterpret_cast<const uint32_t*>(p);
            re = (int)(int16_t)(w & 0xffff);
            im = (int32_t)w >> 16;
        } else {
            re = (int)(int16_t)*reinterpret_cast<const unsigned short*>(p);
            im = (int)(int16_t)*reinterpret_cast<const unsigned short*>(p + 2);
        }
        return make_double2((double)re * 0.00048828125, (double)im * 0.00048828125);
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

// m = scale * |v|: the double every output of the operator is made from
__device__ __forceinline__ double magnitude_d(double2 v, double scale) { return scale * sqrt(v.x * v.x + v.y * v.y); }
__device__ __forceinline__ float magnitude(double2 v, double scale) { return (float)magnitude_d(v, scale); }

// ---- the passes of one tile, shared by spectrum_fused and spectrum_fused_reduce ---------------------------------------------------
// pass p = 1: global memory -> LDS.  Butterfly g = tid + b T of the tile is butterfly i of the tile's slot rl; slot rl of the tile
// that starts at slot0 transforms input row (slot0 + rl) * row_mul + row_add, and loads zeros when slot0 + rl >= slots.
template <int T, int FMT>
__device__ __forceinline__ void pass_first(double2* s, const void* __restrict__ in, int64_t hop, int64_t slot0, int64_t slots, int64_t row_mul,
                                           int64_t row_add, int lg, int shift, const double* __restrict__ window, bool wide)
{
    const int q = 1 << (lg - 2), lgq = lg - 2, tid = threadIdx.x;
#pragma unroll
    for (int b = 0; b < 2; b++) {
        const int g = tid + b * T, rl = g >> lgq, i = g & (q - 1);
        const int64_t slot = slot0 + rl;
        double2 u[4];
        if (slot < slots) {
            const int64_t row = slot * row_mul + row_add;
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
}

// radix-4 passes p = 4, 16, ... that stay in LDS: LDS -> registers, barrier, registers -> LDS
template <int T>
__device__ __forceinline__ void passes_mid(double2* s, const double2* __restrict__ twiddle, int lg)
{
    const int q = 1 << (lg - 2), lgq = lg - 2, tid = threadIdx.x;
    const int passes4 = lg >> 1;
    const int mid_end = (lg & 1) ? passes4 : passes4 - 1;
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
}

// log2 n even: butterfly i of slot rl in the last radix-4 pass p = n / 4.  k = i: u[r] is bin i + r n/4.
__device__ __forceinline__ void last_radix4(const double2* s, const double2* __restrict__ twiddle, int lg, int rl, int i, double2 (&u)[4])
{
    const int q = 1 << (lg - 2);
    const double2* src = s + (rl << lg) + i;
    u[0] = src[0];
    u[1] = cmul(src[q], twiddle[i]);
    u[2] = cmul(src[2 * q], twiddle[2 * i]);
    u[3] = cmul(src[3 * q], twiddle[3 * i]);
    radix4(u);
}

// log2 n odd: butterfly i of slot rl in the radix-2 pass p = n / 2: bins i (lo) and i + n/2 (hi).
__device__ __forceinline__ void last_radix2(const double2* s, const double2* __restrict__ twiddle, int lg, int rl, int i, double2& lo, double2& hi)
{
    const int h = 1 << (lg - 1);
    const double2* src = s + (rl << lg) + i;
    const double2 u0 = src[0], u1 = cmul(src[h], twiddle[i]);
    lo = cadd(u0, u1);
    hi = csub(u0, u1);
}

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
    const bool odd = (lg & 1) != 0;
    const int tid = threadIdx.x;

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * rows_per_tile;
        pass_first<T, FMT>(s, in, hop, row0, rows, 1, 0, lg, shift, window, wide);
        passes_mid<T>(s, twiddle, lg);

        // log2 n even: the last radix-4 pass, LDS -> global memory
        if (!odd) {
#pragma unroll 1
            for (int b = 0; b < 2; b++) {
                const int g = tid + b * T, rl = g >> lgq, i = g & (q - 1);
                if (row0 + rl >= rows) continue;
                double2 u[4];
                last_radix4(s, twiddle, lg, rl, i, u);
                float* o = out + (row0 + rl) * n + i;
#pragma unroll
                for (int r = 0; r < 4; r++) o[r * q] = magnitude(u[r], scale);
            }
        }

        // log2 n odd: the radix-2 pass, LDS -> global memory
        if (odd) {
            const int h = n >> 1;
#pragma unroll 1
            for (int b = 0; b < 4; b++) {
                const int g = tid + b * T, rl = g >> (lg - 1), i = g & (h - 1);
                double2 lo, hi;
                last_radix2(s, twiddle, lg, rl, i, lo, hi);
                if (row0 + rl < rows) {
                    float* o = out + (row0 + rl) * n + i;
                    o[0] = magnitude(lo, scale);
                    o[h] = magnitude(hi, scale);
                }
            }
        }
        __syncthreads();        // the next tile's first pass overwrites what this tile's last pass reads
    }
}

// ---- the reducing form (sdrhip_spectrum_reduce_*) -------------------------------------------------------------------------------
// one value into an accumulator / a chunk's accumulator into the total / the total into the output float.  A non-finite magnitude
// (cf32 input that holds a NaN or an Inf) poisons its bin in every reduce and unit, as numpy's max and maximum do in the model: the max
// hold takes a NaN and keeps one (a plain `m > acc ? m : acc` would drop the row), and the floor clamp lets a NaN through.
__device__ __forceinline__ double reduce_add(double acc, double m, int reduce)
{
    if (reduce == 2) return (m > acc || m != m) ? m : acc;
    return acc + (reduce == 0 ? m * m : m);
}
__device__ __forceinline__ double reduce_fold(double total, double acc, int reduce)
{
    if (reduce == 2) return (acc > total || acc != acc) ? acc : total;
    return total + acc;
}
__device__ __forceinline__ float reduce_finish(double v, const SpectrumReduce& f)
{
    if (f.reduce != 2) v = v / (double)f.group;
    if (f.unit == 1) {
        const double d = (f.reduce == 0 ? 10.0 : 20.0) * log10(v);
        v = d < f.floor_db ? f.floor_db : d;         // log10(0) = -inf: the floor; a NaN stays a NaN
    }
    return (float)v;
}

// element e (0 .. 7) of a thread's accumulators: which slot of the tile and which bin the last pass hands this thread
template <int T>
__device__ __forceinline__ void owned_bin(int tid, int lg, int e, int& rl, int& bin)
{
    if (lg & 1) {
        const int h = 1 << (lg - 1), g = tid + (e >> 1) * T;
        rl = g >> (lg - 1);
        bin = (g & (h - 1)) + (e & 1) * h;
    } else {
        const int q = 1 << (lg - 2), g = tid + (e >> 2) * T;
        rl = g >> (lg - 2);
        bin = (g & (q - 1)) + (e & 3) * q;
    }
}

// Tile slot rl belongs to OUTPUT row tile * rows_per_tile + rl; the workgroup runs that slot's input rows one after the other through
// the same passes as spectrum_fused and keeps what the last pass produces in registers: 8 doubles per thread (2 butterflies x 4 bins,
// or 4 x 2 when log2 n is odd).  The group is cut into chunks of SPECTRUM_REDUCE_CHUNK rows, each summed from 0.0 in ascending order.
// LAYERS = false (a group of one chunk): one work item per tile; the chunk's sums are the totals (0.0 + x = x) and leave as n floats.
// LAYERS = true: a work item is (tile, `per_item` consecutive chunks of [chunk0, chunk1)); every chunk's sums go out as doubles, layer
// (chunk - chunk0) of `partial`, and spectrum_reduce_finalise adds the layers in ascending order from 0.0.  How the chunks are dealt
// out to work items (all of a tile's to one, or spread over the chip: the split) therefore cannot change a bit.  A second set of 8
// doubles for the running total does not fit beside the transform at T = 1024 (128 VGPRs: 8 spilled), which is why groups of more
// than one chunk always go through the layers.
template <int T, int FMT, bool LAYERS>
__global__ __launch_bounds__(T) void spectrum_fused_reduce(const void* __restrict__ in, int64_t hop, int64_t rows_out, int lg, int shift, double scale,
                                                           const double* __restrict__ window, const double2* __restrict__ twiddle, bool wide,
                                                           SpectrumReduce f, int chunk0, int chunk1, int per_item, double* __restrict__ partial,
                                                           float* __restrict__ out)
{
    constexpr int E = 8 * T;
    __shared__ double2 s[E];
    const int n = 1 << lg;
    const int rows_per_tile = E >> lg;
    const int64_t ntiles = (rows_out + rows_per_tile - 1) / rows_per_tile;
    const bool odd = (lg & 1) != 0;
    const int tid = threadIdx.x;
    const int per_tile = LAYERS ? (chunk1 - chunk0 + per_item - 1) / per_item : 1;      // work items of one tile
    const int64_t items = ntiles * per_tile;

    for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const int64_t tile = item / per_tile, row0 = tile * rows_per_tile;
        const int c0 = LAYERS ? chunk0 + (int)(item - tile * per_tile) * per_item : chunk0;
        const int c1 = LAYERS ? (c0 + per_item < chunk1 ? c0 + per_item : chunk1) : chunk1;
        double acc[8];
#pragma unroll
        for (int e = 0; e < 8; e++) acc[e] = 0.0;
        const int j0 = c0 * SPECTRUM_REDUCE_CHUNK;
        const int j1 = (int64_t)c1 * SPECTRUM_REDUCE_CHUNK < f.group ? c1 * SPECTRUM_REDUCE_CHUNK : f.group;
#pragma unroll 1
        for (int j = j0; j < j1; j++) {
            {
                const double* w = window;
                const double2* tw = twiddle;
                asm volatile("" : "+s"(w), "+s"(tw));
                pass_first<T, FMT>(s, in, hop, row0, rows_out, f.group, j, lg, shift, w, wide);
                passes_mid<T>(s, tw, lg);
                // One butterfly at a time, like spectrum_fused (two in flight cost 30 VGPRs more, and T = 1024 has 128).  The loops are
                // real loops, so the accumulators rotate instead of being indexed: every turn works on the first elements and moves
                // them to the back, and after the last turn each one is in its own place again.
                if (!odd) {
#pragma unroll 1
                    for (int b = 0; b < 2; b++) {
                        const int g = tid + b * T;
                        double2 u[4];
                        last_radix4(s, tw, lg, g >> (lg - 2), g & ((n >> 2) - 1), u);
                        double v[4];
#pragma unroll
                        for (int r = 0; r < 4; r++) v[r] = reduce_add(acc[r], magnitude_d(u[r], scale), f.reduce);
#pragma unroll
                        for (int r = 0; r < 4; r++) {
                            acc[r] = acc[r + 4];
                            acc[r + 4] = v[r];
                        }
                    }
                } else {
#pragma unroll 1
                    for (int b = 0; b < 4; b++) {
                        const int g = tid + b * T;
                        double2 lo, hi;
                        last_radix2(s, tw, lg, g >> (lg - 1), g & ((n >> 1) - 1), lo, hi);
                        const double v0 = reduce_add(acc[0], magnitude_d(lo, scale), f.reduce);
                        const double v1 = reduce_add(acc[1], magnitude_d(hi, scale), f.reduce);
#pragma unroll
                        for (int e = 0; e < 6; e++) acc[e] = acc[e + 2];
                        acc[6] = v0;
                        acc[7] = v1;
                    }
                }
                __syncthreads();        // the next row's first pass overwrites what this row's last pass reads
            }
            // a chunk that ends with this row goes out
            // (the thread index behind an empty asm: what is computed from it for these rare steps stays here, instead of being
            // hoisted out of every loop into registers the transform needs)
            if (LAYERS && (((j + 1) & (SPECTRUM_REDUCE_CHUNK - 1)) == 0 || j + 1 == j1)) {
                int t = tid;
                asm volatile("" : "+v"(t));
                double* layer = partial + (int64_t)(j / SPECTRUM_REDUCE_CHUNK - chunk0) * rows_out * n;
#pragma unroll 1
                for (int e = 0; e < 8; e++) {       // a real loop: the sums rotate past element 0
                    int rl, bin;
                    owned_bin<T>(t, lg, e, rl, bin);
                    if (row0 + rl < rows_out) layer[(row0 + rl) * n + bin] = acc[0];
#pragma unroll
                    for (int x = 0; x < 7; x++) acc[x] = acc[x + 1];
                }
#pragma unroll
                for (int e = 0; e < 8; e++) acc[e] = 0.0;
            }
        }
        if (!LAYERS) {
            // the sums go through LDS (free since the last row's barrier) in output order: the finishing loop, with its division and
            // log10, then holds one value at a time and writes whole runs of consecutive floats
            double* sd = reinterpret_cast<double*>(s);
            int t = tid;
            asm volatile("" : "+v"(t));
#pragma unroll
            for (int e = 0; e < 8; e++) {
                int rl, bin;
                owned_bin<T>(t, lg, e, rl, bin);
                sd[(rl << lg) + bin] = acc[e];
            }
            __syncthreads();
            const int64_t left = (rows_out - row0) * n;        // floats of `out` from this tile's first row on
#pragma unroll 1
            for (int x = t; x < E && x < left; x += T) out[row0 * n + x] = reduce_finish(sd[x], f);
            __syncthreads();        // the next item's first pass overwrites what this loop reads
        }
    }
}

// the layers' second kernel: per output bin, the layers of `partial` in ascending order onto the carried total (0.0 before the
// first slice of a group); the last slice applies mean / dB and writes the float
__global__ __launch_bounds__(256) void spectrum_reduce_finalise(const double* __restrict__ partial, int layers, int64_t count, double* __restrict__ total,
                                                                 int first, int last, SpectrumReduce f, float* __restrict__ out)
{
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < count; k += (int64_t)gridDim.x * 256) {
        double t = first ? 0.0 : total[k];
        for (int l = 0; l < layers; l++) t = reduce_fold(t, partial[(int64_t)l * count + k], f.reduce);
        if (last) out[k] = reduce_finish(t, f);
        else total[k] = t;
    }
}

// hipFFT route: input rows [b0, b0 + nrows) of a slice (transformed, in `work`) into the two doubles of state every output bin has,
// the running chunk sum and the total, in the defined order; the row that completes a group writes the output float
__global__ __launch_bounds__(256) void spectrum_accumulate(const double2* __restrict__ work, int64_t b0, int64_t nrows, int n, double scale,
                                                            SpectrumReduce f, double* __restrict__ chunk, double* __restrict__ total,
                                                            float* __restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t r_first = b0 / f.group, r_last = (b0 + nrows - 1) / f.group;
    for (int64_t R = r_first + blockIdx.y; R <= r_last; R += gridDim.y) {
        const int64_t lo = R * f.group > b0 ? R * f.group : b0;
        const int64_t hi = (R + 1) * f.group < b0 + nrows ? (R + 1) * f.group : b0 + nrows;
        int64_t j = lo - R * f.group;
        double c = 0.0, t = 0.0;
        if (j != 0) {
            c = chunk[R * n + k];
            t = total[R * n + k];
        }
        for (int64_t r = lo; r < hi; r++, j++) {
            if (j != 0 && j % SPECTRUM_REDUCE_CHUNK == 0) {
                t = reduce_fold(t, c, f.reduce);
                c = 0.0;
            }
            c = reduce_add(c, magnitude_d(work[(r - b0) * n + k], scale), f.reduce);
        }
        if (j == f.group) {
            out[R * n + k] = reduce_finish(reduce_fold(t, c, f.reduce), f);
        } else {
            chunk[R * n + k] = c;
            total[R * n + k] = t;
        }
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

bool wide_loads(const SpectrumArgs& a) { return ((uintptr_t)a.in & (a.format == 0 ? 1u : a.format == 2 ? 3u : 7u)) == 0; }

template <int T>
hipError_t launch_fused(hipStream_t stream, const SpectrumArgs& a, int lg, float* out)
{
    const int rows_per_tile = (8 * T) >> lg;
    const int64_t ntiles = (a.rows + rows_per_tile - 1) / rows_per_tile;
    const int64_t resident = 2048;           // 8 workgroups on each of 256 CUs: more tiles than that loop inside the launch
    const unsigned grid = (unsigned)(ntiles < resident ? ntiles : resident);
    if (a.format == 0)
        spectrum_fused<T, 0><<<grid, T, 0, stream>>>(a.in, a.hop, a.rows, lg, a.shift, a.scale, a.window, a.twiddle, wide_loads(a), out);
    else if (a.format == 2)
        spectrum_fused<T, 2><<<grid, T, 0, stream>>>(a.in, a.hop, a.rows, lg, a.shift, a.scale, a.window, a.twiddle, wide_loads(a), out);
    else
        spectrum_fused<T, 1><<<grid, T, 0, stream>>>(a.in, a.hop, a.rows, lg, a.shift, a.scale, a.window, a.twiddle, wide_loads(a), out);
    return hipGetLastError();
}

template <int T>
hipError_t launch_fused_reduce(hipStream_t stream, const SpectrumArgs& a, const SpectrumReduce& f, int lg, int chunk0, int chunk1, int per_item,
                               double* partial, float* out)
{
    const int rows_per_tile = (8 * T) >> lg;
    const int64_t ntiles = (a.rows + rows_per_tile - 1) / rows_per_tile;
    const int64_t items = partial ? ntiles * ((chunk1 - chunk0 + per_item - 1) / per_item) : ntiles;
    const int64_t resident = 2048;
    const unsigned grid = (unsigned)(items < resident ? items : resident);
    const bool wide = wide_loads(a);
#define SDRHIP_REDUCE_LAUNCH(FMT, LAYERS)                                                                                                     \
    spectrum_fused_reduce<T, FMT, LAYERS><<<grid, T, 0, stream>>>(a.in, a.hop, a.rows, lg, a.shift, a.scale, a.window, a.twiddle, wide, f, chunk0, \
                                                                 chunk1, per_item, partial, out)
    if (a.format == 0) {
        if (partial) SDRHIP_REDUCE_LAUNCH(0, true);
        else SDRHIP_REDUCE_LAUNCH(0, false);
    } else if (a.format == 2) {
        if (partial) SDRHIP_REDUCE_LAUNCH(2, true);
        else SDRHIP_REDUCE_LAUNCH(2, false);
    } else {
        if (partial) SDRHIP_REDUCE_LAUNCH(1, true);
        else SDRHIP_REDUCE_LAUNCH(1, false);
    }
#undef SDRHIP_REDUCE_LAUNCH
    return hipGetLastError();
}

}  // namespace

hipError_t launch_spectrum_fused_reduce(hipStream_t stream, const SpectrumArgs& a, const SpectrumReduce& f, int chunk0, int chunk1, int per_item,
                                        double* partial, float* out)
{
    if (!spectrum_fused_size(a.n) || a.rows < 1 || f.group < 1 || chunk0 < 0 || chunk1 <= chunk0 || per_item < 1) return hipErrorInvalidValue;
    if ((int64_t)(chunk1 - 1) * SPECTRUM_REDUCE_CHUNK >= f.group) return hipErrorInvalidValue;      // the last chunk holds a row
    if (!partial && (chunk0 != 0 || f.group > SPECTRUM_REDUCE_CHUNK)) return hipErrorInvalidValue;   // straight to `out`: one chunk
    int lg = 0;
    while ((1 << lg) < a.n) lg++;
    if (a.n == 8192) return launch_fused_reduce<1024>(stream, a, f, lg, chunk0, chunk1, per_item, partial, out);
    if (a.n == 4096) return launch_fused_reduce<512>(stream, a, f, lg, chunk0, chunk1, per_item, partial, out);
    return launch_fused_reduce<256>(stream, a, f, lg, chunk0, chunk1, per_item, partial, out);
}

hipError_t launch_spectrum_reduce_finalise(hipStream_t stream, const double* partial, int layers, int64_t count, double* total, bool first, bool last,
                                           const SpectrumReduce& f, float* out)
{
    const int64_t blocks = (count + 255) / 256;
    spectrum_reduce_finalise<<<(unsigned)(blocks < 16384 ? blocks : 16384), 256, 0, stream>>>(partial, layers, count, total, first, last, f, out);
    return hipGetLastError();
}

hipError_t launch_spectrum_accumulate(hipStream_t stream, const double2* work, int64_t b0, int64_t nrows, int n, double scale, const SpectrumReduce& f,
                                      double* chunk, double* total, float* out)
{
    const int64_t touched = (b0 + nrows - 1) / f.group - b0 / f.group + 1;
    const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(touched < 4096 ? touched : 4096));
    spectrum_accumulate<<<grid, 256, 0, stream>>>(work, b0, nrows, n, scale, f, chunk, total, out);
    return hipGetLastError();
}

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
    else if (a.format == 2)
        spectrum_prepare<2><<<grid, 256, 0, stream>>>(a.in, a.hop, row0, nrows, a.n, a.shift, a.window, wide_loads(a), work);
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
