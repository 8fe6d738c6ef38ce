// kernels_tuner.hip -- the tuner: multiplication by a periodic complex oscillator in front of the complex FIR decimator
// (`P.map (VG.zipWith (*) osc) >-> firDecimator deci n`; oscillators: quarterBandUp / halfBandUp, Util.hs:263-285).
//
//     x[n] = input sample n (u8 IQ: (u - 128) * (1/128), exact; int16 IQ: s * 2^-11, exact; cfloat: as given)
//     o[n] = osc[n mod N]                       n = ABSOLUTE stream index, N = period
//     m[n] = (x.re*o.re - x.im*o.im, x.re*o.im + x.im*o.re)        Data.Complex's (*) at Float: every product and sum rounded
//     y[k] = the complex decimator on m (One outputs in the AVX "RC" order, Cross outputs sequential)
//
// Fused route (k_tuner_c4): the LDS-tiled decimator of decimate_tile.hpp -- its tile geometry, raw loads, MAC walk, fold and
// in-tile Cross outputs -- with a loader of its own between the raw 16-byte loads and the LDS stores: convert, fetch the
// oscillator entry, four multiplies and two adds, store to the padded layout.  m never reaches memory.  The mix is always
// computed in full: (-0)*1 - (+0)*0 and (+0)*1 - (+0)*0 differ in the sign of zero, so there is no shortcut for entries that
// are 0 or +-1.  Two shortcuts of the decimator's own u8 loader are NOT taken: LDS holds the SCALED mixed samples and the
// kernel gets the plain taps (the mix rounds on the scaled value; h/128 * m is no longer the same real number as h * m
// rounded once), and no tap's MACs are skipped (a mixed sample is finite, but the walk is the guarded one anyway).
//
// The oscillator table (8 N bytes, N <= 65536: at most 512 KiB, L2-resident) is read with one 8-byte load per sample; a
// thread's entries are consecutive modulo N.  The phase of a thread's first sample is
//     (k_begin D + tile TS + tid SPV) mod N,  TS = samples between tiles, SPV = samples per 16-byte vector,
// evaluated in 32 bits from (k_begin D) mod N -- the one 64-bit modulo, done by the host -- and (tile mod N)(TS mod N) mod N
// (both factors below 2^16); from there it advances with a compare-and-wrap.
//
// Cross outputs of launches too long to compute them in the tile kernel: k_tuner_crossfix, one thread per candidate slot of a
// seam (seam_span, kernels.hpp), mixing the same way, sequential over the plain taps.
// Two-pass route (every other order / factor, and the A/B partner): k_tuner_mix writes m to a scratch buffer, the stock
// decimator runs on it (tuner.cpp).
// FMT is the input format (InFmt).  k_tuner_c4 exists for cfloat and u8: the int16 tuner's fused route is the bank's tile kernel
// with one channel (launch_tuner_bank, kernels_tuner_bank.hip).
#include "decimate_tile.hpp"
#include "tuner_mix.hpp"

namespace sdrhip {

static std::atomic<long long> g_tuner_fused_launches{0};
long long tuner_fused_launch_count() { return g_tuner_fused_launches.load(); }

namespace {

// One tile: decimate_c4_tile's general body (ragged-end loader, in-tile Cross outputs) around the mixing loader.
template <int D, int P, int R, int NT, int FMT, int TC, bool GUARD>
__global__ void __launch_bounds__(NT) k_tuner_c4(const void* __restrict__ in, int64_t x0 /* sample index of output 0's window in `in` */,
                                                 int count, const float* __restrict__ taps /* plain */, float* __restrict__ out,
                                                 int p_eff /* GUARD: taps of the filter (multiple of TC, <= P) */,
                                                 int inl_seam /* > 0: compute the Cross outputs of buffers this long HERE */,
                                                 int inl_r0 /* window start of output 0 inside its buffer */,
                                                 const float2* __restrict__ osc, int period, int ph_launch /* (k_begin D) mod period */)
{
    using T = Tile<D, P, R, NT>;
    using St = Stage<T, FMT, NT>;
    constexpr int NP = 4, ORD = 0;                           // the AVX "RC" order
    extern __shared__ __attribute__((aligned(16))) unsigned char tuner_smem[];
    float2* lds = reinterpret_cast<float2*>(tuner_smem);

    // XCD-aware tile order, as k_decimate_c4
    const int ntiles = (count + T::OUTS - 1) / T::OUTS;
    const int b = blockIdx.x;
    const int tile = (b & ~63) + ((b & 7) << 3) + ((b >> 3) & 7);
    if (tile >= ntiles) return;

    const int out0 = tile * T::OUTS;
    const int64_t s0 = (int64_t)out0 * D;                     // first sample of the tile, relative to x0
    {
        St st;
        const int64_t total_avail = (int64_t)(count - 1) * D + (GUARD ? p_eff : P);      // samples that exist from x0 on
        const int64_t av = total_avail - s0;
        st.load(in, x0 + s0, av > T::SPAN ? T::SPAN : (int)av);
        const uint32_t n = (uint32_t)period;
        constexpr uint32_t TS = (uint32_t)T::OUTS * D;
        const uint32_t ph = ((uint32_t)ph_launch + (((uint32_t)tile % n) * (TS % n)) % n + (uint32_t)(threadIdx.x * St::SPV)) % n;
        tuner_store<T, FMT, NT>(st.r, lds, osc, n, ph);
    }
    __syncthreads();

    const float2* win = lds + T::lds_idx(threadIdx.x * T::CHUNK);
    float2 acc[R][NP];
#pragma unroll
    for (int r = 0; r < R; r++)
#pragma unroll
        for (int k = 0; k < NP; k++) acc[r][k] = make_float2(0.0f, 0.0f);
    mac_window<D, P, R, T, TC, GUARD, NP, 0>(win, taps, acc, GUARD ? p_eff / TC : 0);

    const int o = out0 + threadIdx.x * R;
    float2 res[R];
#pragma unroll
    for (int r = 0; r < R; r++) res[r] = fold_partials<NP, ORD>(acc[r]);
    if (inl_seam > 0) {
        // as decimate_c4_tile: outputs whose window straddles a multiple of inl_seam, sequential order from the same LDS tile
        const int plen = GUARD ? p_eff : P;
        const int rt = (int)(((int64_t)inl_r0 + s0) % inl_seam);
        bool cross[R];
        bool any = false;
#pragma unroll
        for (int r = 0; r < R; r++) {
            int rr = rt + (threadIdx.x * R + r) * D;
            if (rr >= inl_seam) rr -= inl_seam;
            cross[r] = rr + plen > inl_seam;
            any |= cross[r];
        }
        if (any) inline_cross_outputs<D, R, T, TC, GUARD>(win, taps, plen, cross, res);
    }
    // (an output pointer that is only 8-byte aligned -- a launch cut at an odd output -- takes the float2 stores)
    if (R % 2 == 0 && o + R <= count && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        float4* dst = reinterpret_cast<float4*>(out + 2 * (int64_t)o);
#pragma unroll
        for (int r = 0; r + 1 < R; r += 2) dst[r / 2] = make_float4(res[r].x, res[r].y, res[r + 1].x, res[r + 1].y);
    } else {
#pragma unroll
        for (int r = 0; r < R; r++)
            if (o + r < count) *reinterpret_cast<float2*>(out + 2 * (int64_t)(o + r)) = res[r];
    }
}

// Cross outputs, one thread per candidate slot of a seam (k_fir_cplx_crossfix with the mix in front of every product)
template <int FMT>
__global__ void __launch_bounds__(256) k_tuner_crossfix(Geom g, const float* __restrict__ xtaps, const void* __restrict__ in,
                                                         float* __restrict__ out, int64_t first_seam, int nseams, int per_seam,
                                                         const float2* __restrict__ osc, int period)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseams * per_seam) return;
    const int si = t / per_seam, ci = t - si * per_seam;
    const int64_t edge = (first_seam + si) * g.seamBI;
    const int64_t m = (edge + g.D - 1) / g.D - 1 - ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    const uint32_t n = (uint32_t)period;
    uint32_t ph = (uint32_t)((uint64_t)v % n);
    float re = 0.0f, im = 0.0f;
    for (int j = 0; j < g.Lp; j++) {
        const float2 mx = tuner_mul(tuner_sample<FMT>(in, v - g.in_base + j), osc[ph]);
        ph = wrap_inc(ph, n);
        re = re + mx.x * xtaps[j];
        im = im + mx.y * xtaps[j];
    }
    *reinterpret_cast<float2*>(out + 2 * (m - g.k_begin)) = make_float2(re, im);
}

// Two-pass route, first pass: out[i] = m of sample i, i < n; ph0 = phase of sample 0.  Grid-stride, 8 bytes out per lane.
template <int FMT>
__global__ void __launch_bounds__(256) k_tuner_mix(const void* __restrict__ in, float2* __restrict__ out, uint32_t n_samples,
                                                    const float2* __restrict__ osc, int period, int ph0)
{
    const uint32_t n = (uint32_t)period, total = gridDim.x * 256u, step = total % n;
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t ph = ((uint32_t)ph0 + i % n) % n;
    for (; i < n_samples; i += total) {
        out[i] = tuner_mul(tuner_sample<FMT>(in, i), osc[ph]);
        ph += step;
        if (ph >= n) ph -= n;
    }
}

template <int D, int P, int FMT, int TC, bool GUARD>
void launch_tuner_c4(hipStream_t s, const Geom& g, const float* taps, const void* in, float* out, bool inline_cross, bool* inlined,
                     const float* d_osc, int period)
{
    constexpr int R = 2, NT = 256;
    using T = Tile<D, P, R, NT>;
    // the dynamic-LDS attribute is per device: one flag per (instantiation, device); idempotent, a race only repeats the call
    static std::atomic<bool> attr_set[64];
    auto kern = k_tuner_c4<D, P, R, NT, FMT, TC, GUARD>;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_BYTES);
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    const int tiles = (g.count + T::OUTS - 1) / T::OUTS;
    const int grid = ((tiles + 63) / 64) * 64;       // whole groups of 64: the kernel permutes blockIdx -> tile within a group
    const int64_t x0 = g.k_begin * D - g.in_base;
    int inl_seam = 0, inl_r0 = 0;
    if (inline_cross && g.seamBI >= (int64_t)T::OUTS * D + g.Lp && g.seamBI < (1 << 30)) {   // a tile spans less than one buffer
        inl_seam = (int)g.seamBI;
        inl_r0 = (int)((g.k_begin * D) % g.seamBI);
    }
    *inlined = inl_seam > 0;
    const int ph_launch = (int)((g.k_begin * D) % period);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), T::LDS_BYTES, s, in, x0, g.count, taps, out, g.Lp, inl_seam, inl_r0,
                       reinterpret_cast<const float2*>(d_osc), period, ph_launch);
}

// the instantiation that serves the launch's shape (tuner_fused_fits has admitted it)
template <int FMT>
void launch_tuner_c4_shape(hipStream_t s, const Geom& g, int P, const float* taps, const void* in, float* out, bool inl, bool* inlined,
                           const float* d_osc, int period)
{
#define TUNER(DV, TCV, GV) launch_tuner_c4<DV, 128, FMT, TCV, GV>(s, g, taps, in, out, inl, inlined, d_osc, period)
    if (g.D == 4) TUNER(4, 4, true);
    else if (g.D == 16) { if (P % 8 == 0) TUNER(16, 8, true); else TUNER(16, 4, true); }
    else if (P == 128) TUNER(8, 8, false);           // the exact-length walk for the full 128 taps
    else if (P % 8 == 0) TUNER(8, 8, true);
    else TUNER(8, 4, true);
#undef TUNER
}

}  // namespace

bool tuner_fused_fits(const Geom& g, int P, bool has_cross_taps, const void* d_in, InFmt fmt, const void* d_out, int period)
{
    if (g.I != 1 || g.count <= 0 || g.seamBI < 0 || g.k_begin < 0 || period < 1) return false;
    // the shapes decimate_tile.hpp serves up to 128 prepared taps: decimation 4 / 8 / 16, a multiple of 4 taps (mkDecimatorC pads to that)
    if (!((g.D == 8 || g.D == 4 || g.D == 16) && P >= 8 && P <= 128 && P % 4 == 0 && g.Lp == P && P > g.D)) return false;
    if (g.seamBI != 0 && !has_cross_taps) return false;
    // vector loads need 16-byte aligned tile starts (tiles begin at multiples of 8 samples from x0).  Each format keeps the conditions
    // it was measured and tested with: int16 alone refuses a first window before d_in and a d_in off its 4-byte samples
    struct Fit { bool x0_nonneg; uintptr_t base_mask; };
    static const Fit kFit[3] = {/* IN_CF32 */ {false, 0}, /* IN_U8 */ {false, 0}, /* IN_I16 */ {true, 3}};
    const Fit& f = kFit[fmt];
    const int64_t x0 = g.k_begin * g.D - g.in_base;
    if (f.x0_nonneg && x0 < 0) return false;
    const uintptr_t base = reinterpret_cast<uintptr_t>(d_in);
    if ((base & f.base_mask) != 0 || ((base + (uintptr_t)in_fmt_bytes(fmt) * (uintptr_t)x0) & 15) != 0) return false;
    return (reinterpret_cast<uintptr_t>(d_out) & 7) == 0;
}

bool launch_tuner_fused(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                        InFmt fmt, float* d_out, const float* d_osc, int period)
{
    if (fmt == IN_I16) {
        // the bank's tile kernel with one channel (its table at offset 0): there is no one-row int16 kernel
        const int off0 = 0;
        return launch_tuner_bank(s, g, d_plain_taps, P, d_cross_taps, d_in, fmt, d_out, 0, d_osc, 1, &off0, &period, false);
    }
    if (!tuner_fused_fits(g, P, d_cross_taps != nullptr, d_in, fmt, d_out, period)) return false;
    // launch-bound sizes compute their Cross outputs inside the tile kernel, as the decimator does (abi_device.cpp: the 5v row)
    const bool inl = g.seamBI > 0 && g.count <= 5 * (int64_t)small_launch_outputs();
    bool inlined = false;
    const bool u8 = fmt == IN_U8;
    if (u8) launch_tuner_c4_shape<IN_U8>(s, g, P, d_plain_taps, d_in, d_out, inl, &inlined, d_osc, period);
    else launch_tuner_c4_shape<IN_CF32>(s, g, P, d_plain_taps, d_in, d_out, inl, &inlined, d_osc, period);
    g_tuner_fused_launches.fetch_add(1, std::memory_order_relaxed);

    const SeamSpan sp = seam_span(g);
    if (sp.nseams > 0 && !inlined) {
        const dim3 grid((unsigned)(((int64_t)sp.nseams * sp.per + 255) / 256)), block(256);
        const float2* o2 = reinterpret_cast<const float2*>(d_osc);
        auto fix = u8 ? k_tuner_crossfix<IN_U8> : k_tuner_crossfix<IN_CF32>;
        hipLaunchKernelGGL(fix, grid, block, 0, s, g, d_cross_taps, d_in, d_out, sp.first, sp.nseams, sp.per, o2, period);
    }
    return true;
}

void launch_tuner_mix(hipStream_t s, const void* d_in, InFmt fmt, float* d_out, int64_t n, const float* d_osc, int period, int ph0)
{
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    auto mix = fmt == IN_U8 ? k_tuner_mix<IN_U8> : fmt == IN_I16 ? k_tuner_mix<IN_I16> : k_tuner_mix<IN_CF32>;
    hipLaunchKernelGGL(mix, dim3((unsigned)blocks), dim3(256), 0, s, d_in, reinterpret_cast<float2*>(d_out), (uint32_t)n,
                       reinterpret_cast<const float2*>(d_osc), period, ph0);
}

}  // namespace sdrhip
