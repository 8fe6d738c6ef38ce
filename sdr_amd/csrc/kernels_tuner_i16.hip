// kernels_tuner_i16.hip -- the tuner family on 16-bit signed IQ (sdrhip_tuner_run_i16, sdrhip_tuner_bank_run_i16 and the bank's i16
// Pipe): interleaved int16 (I, Q), 4 bytes per sample, converted by (float)s * 2^-11 (convertCBladeRF, convert.c:52-85) in the tile
// loader.  Every launch writes the bits of the cfloat launch on the buffer sdrhip_convert_i16_run makes of the same samples.
//
// k_tuner_bank_c4_i16 is k_tuner_bank_c4 (kernels_tuner_bank.hip) around the int16 staging of tuner_i16.hpp: the flat 1-D grid with
// the channel fastest, the per-channel off / period / ph in the kernel's arguments, the MAC walk, fold and in-tile Cross outputs of
// decimate_tile.hpp and the 16-byte / 8-byte output store rule are that kernel's, line for line.  The one-row tuner's fused route is
// this kernel with ONE channel (table offset 0): there is no separate one-row kernel.  k_tuner_bank_crossfix_i16, k_tuner_bank_cross_i16
// and k_tuner_mix_i16 are the sequential-order kernels and the two-pass route's first pass reading short2.
//
// Nothing here is shared with the cfloat / u8 kernels beyond the headers they include: those translation units compile as they did.
#include "decimate_tile.hpp"
#include "tuner_i16.hpp"
#include "tuner_mix.hpp"

namespace sdrhip {

static std::atomic<long long> g_tuner_i16_launches{0};
long long tuner_i16_launch_count() { return g_tuner_i16_launches.load(); }
static std::atomic<long long> g_tuner_i16_bank_launches{0};
long long tuner_i16_bank_launch_count() { return g_tuner_i16_bank_launches.load(); }
static std::atomic<long long> g_tuner_i16_cross_launches{0};
long long tuner_i16_bank_cross_launch_count() { return g_tuner_i16_cross_launches.load(); }

namespace {

struct BankChannelsI16 {
    int64_t out_stride;                        // floats between the channels' output rows
    int channels;
    int off[kTunerBankMaxChannels];            // first entry of the channel's table, in (re, im) pairs
    int period[kTunerBankMaxChannels];
    int ph[kTunerBankMaxChannels];             // (k_begin D) mod period: the host's one 64-bit modulo per channel and launch
};

template <int D, int P, int R, int NT, int TC, bool GUARD>
__global__ void __launch_bounds__(NT) k_tuner_bank_c4_i16(const void* __restrict__ in, int64_t x0 /* sample index of output 0's window in `in` */,
                                                          int count, const float* __restrict__ taps /* plain */, float* __restrict__ out,
                                                          int p_eff /* GUARD: taps of the filter (multiple of TC, <= P) */,
                                                          int inl_seam /* > 0: compute the Cross outputs of buffers this long HERE */,
                                                          int inl_r0 /* window start of output 0 inside its buffer */,
                                                          const float2* __restrict__ osc /* every table */, BankChannelsI16 bank)
{
    using T = Tile<D, P, R, NT>;
    using St = StageI16<T, NT>;
    constexpr int NP = 4, ORD = 0;                           // the AVX "RC" order
    extern __shared__ __attribute__((aligned(16))) unsigned char tuner_i16_smem[];
    float2* lds = reinterpret_cast<float2*>(tuner_i16_smem);

    const int ntiles = (count + T::OUTS - 1) / T::OUTS;
    const unsigned nch = (unsigned)bank.channels;
    const unsigned j = blockIdx.x % nch;
    const int tile = (int)(blockIdx.x / nch);
    if (tile >= ntiles) return;
    osc += bank.off[j];
    out += (int64_t)j * bank.out_stride;

    const int out0 = tile * T::OUTS;
    const int64_t s0 = (int64_t)out0 * D;                     // first sample of the tile, relative to x0
    {
        St st;
        const int64_t total_avail = (int64_t)(count - 1) * D + (GUARD ? p_eff : P);      // samples that exist from x0 on
        const int64_t av = total_avail - s0;
        st.load(in, x0 + s0, av > T::SPAN ? T::SPAN : (int)av);
        const uint32_t n = (uint32_t)bank.period[j];
        constexpr uint32_t TS = (uint32_t)T::OUTS * D;
        const uint32_t ph = ((uint32_t)bank.ph[j] + (((uint32_t)tile % n) * (TS % n)) % n + (uint32_t)(threadIdx.x * St::SPV)) % n;
        tuner_store_i16<T, NT>(st.r, lds, osc, n, ph);
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
    // the ROW's pointer decides: an odd row of a stride that is 2 (mod 4), or a launch cut at an odd output, takes the float2 stores
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

// Cross outputs of every channel, one thread per candidate slot of a seam and channel (k_tuner_bank_crossfix reading short2)
__global__ void __launch_bounds__(256) k_tuner_bank_crossfix_i16(Geom g, const float* __restrict__ xtaps, const short2* __restrict__ in,
                                                                  float* __restrict__ out, int64_t first_seam, int nseams, int per_seam,
                                                                  const float2* __restrict__ osc, BankChannelsI16 bank)
{
    const unsigned nch = (unsigned)bank.channels;
    const unsigned c = blockIdx.x % nch;
    const int t = (int)(blockIdx.x / nch) * (int)blockDim.x + (int)threadIdx.x;
    if (t >= nseams * per_seam) return;
    osc += bank.off[c];
    out += (int64_t)c * bank.out_stride;
    const int si = t / per_seam, ci = t - si * per_seam;
    const int64_t edge = (first_seam + si) * g.seamBI;
    const int64_t m = (edge + g.D - 1) / g.D - 1 - ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    const uint32_t n = (uint32_t)bank.period[c];
    uint32_t ph = (uint32_t)((uint64_t)v % n);
    float re = 0.0f, im = 0.0f;
    for (int j = 0; j < g.Lp; j++) {
        const short2 u = in[v - g.in_base + j];
        const float2 mx = tuner_mul(tuner_i16(u.x, u.y), osc[ph]);
        ph = wrap_inc(ph, n);
        re = re + mx.x * xtaps[j];
        im = im + mx.y * xtaps[j];
    }
    *reinterpret_cast<float2*>(out + 2 * (m - g.k_begin)) = make_float2(re, im);
}

// Outputs [g.k_begin, g.k_begin + g.count) of every channel, ALL of them Cross (k_tuner_bank_cross reading short2).  Block b: channel
// b % K, outputs of block b / K.
__global__ void __launch_bounds__(256) k_tuner_bank_cross_i16(Geom g, const float* __restrict__ xtaps, const short2* __restrict__ in,
                                                               float* __restrict__ out, const float2* __restrict__ osc, BankChannelsI16 bank)
{
    const unsigned nch = (unsigned)bank.channels;
    const unsigned c = blockIdx.x % nch;
    const int t = (int)(blockIdx.x / nch) * (int)blockDim.x + (int)threadIdx.x;
    if (t >= g.count) return;
    osc += bank.off[c];
    out += (int64_t)c * bank.out_stride;
    const int64_t v = (g.k_begin + t) * g.D;
    const uint32_t n = (uint32_t)bank.period[c];
    uint32_t ph = (uint32_t)((uint64_t)v % n);
    float re = 0.0f, im = 0.0f;
    for (int j = 0; j < g.Lp; j++) {
        const short2 u = in[v - g.in_base + j];
        const float2 mx = tuner_mul(tuner_i16(u.x, u.y), osc[ph]);
        ph = wrap_inc(ph, n);
        re = re + mx.x * xtaps[j];
        im = im + mx.y * xtaps[j];
    }
    *reinterpret_cast<float2*>(out + 2 * (int64_t)t) = make_float2(re, im);
}

// Two-pass route, first pass (k_tuner_mix reading short2): out[i] = m of sample i, i < n; ph0 = phase of sample 0.
__global__ void __launch_bounds__(256) k_tuner_mix_i16(const short2* __restrict__ in, float2* __restrict__ out, uint32_t n_samples,
                                                        const float2* __restrict__ osc, int period, int ph0)
{
    const uint32_t n = (uint32_t)period, total = gridDim.x * 256u, step = total % n;
    uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t ph = ((uint32_t)ph0 + i % n) % n;
    for (; i < n_samples; i += total) {
        const short2 u = in[i];
        out[i] = tuner_mul(tuner_i16(u.x, u.y), osc[ph]);
        ph += step;
        if (ph >= n) ph -= n;
    }
}

template <int D, int P, int TC, bool GUARD>
void launch_tuner_bank_c4_i16(hipStream_t s, const Geom& g, const float* taps, const void* in, float* out, bool inline_cross, bool* inlined,
                              const float* d_tables, const BankChannelsI16& bank)
{
    constexpr int R = 2, NT = 256;
    using T = Tile<D, P, R, NT>;
    // the dynamic-LDS attribute is per device: one flag per (instantiation, device); idempotent, a race only repeats the call
    static std::atomic<bool> attr_set[64];
    auto kern = k_tuner_bank_c4_i16<D, P, R, NT, TC, GUARD>;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)T::LDS_BYTES);
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    const int tiles = (g.count + T::OUTS - 1) / T::OUTS;       // at most 2^22: tiles * channels fits a 1-D grid
    const unsigned grid = (unsigned)tiles * (unsigned)bank.channels;
    const int64_t x0 = g.k_begin * D - g.in_base;
    int inl_seam = 0, inl_r0 = 0;
    if (inline_cross && g.seamBI >= (int64_t)T::OUTS * D + g.Lp && g.seamBI < (1 << 30)) {   // a tile spans less than one buffer
        inl_seam = (int)g.seamBI;
        inl_r0 = (int)((g.k_begin * D) % g.seamBI);
    }
    *inlined = inl_seam > 0;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), T::LDS_BYTES, s, in, x0, g.count, taps, out, g.Lp, inl_seam, inl_r0,
                       reinterpret_cast<const float2*>(d_tables), bank);
}

}  // namespace

bool tuner_i16_fused_fits(const Geom& g, int P, bool has_cross_taps, const void* d_in, const void* d_out, int period)
{
    if (g.I != 1 || g.count <= 0 || g.seamBI < 0 || g.k_begin < 0 || period < 1) return false;
    // the shapes decimate_tile.hpp serves up to 128 prepared taps: decimation 4 / 8 / 16, a multiple of 4 taps (mkDecimatorC pads to that)
    if (!((g.D == 8 || g.D == 4 || g.D == 16) && P >= 8 && P <= 128 && P % 4 == 0 && g.Lp == P && P > g.D)) return false;
    if (g.seamBI != 0 && !has_cross_taps) return false;
    // vector loads need 16-byte aligned tile starts (tiles begin at multiples of 8 samples from x0); a sample is one 4-byte word
    const int64_t x0 = g.k_begin * g.D - g.in_base;
    if (x0 < 0) return false;
    const uintptr_t base = reinterpret_cast<uintptr_t>(d_in);
    if ((base & 3) != 0 || ((base + 4 * (uintptr_t)x0) & 15) != 0) return false;
    return (reinterpret_cast<uintptr_t>(d_out) & 7) == 0;
}

bool launch_tuner_bank_i16(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                           float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods,
                           bool counts_as_bank)
{
    if (channels < 1 || channels > kTunerBankMaxChannels || (out_stride & 1) != 0) return false;
    if (channels > 1 && out_stride < 2 * (int64_t)g.count) return false;
    for (int j = 0; j < channels; j++)
        if (!tuner_i16_fused_fits(g, P, d_cross_taps != nullptr, d_in, d_out, periods[j])) return false;
    BankChannelsI16 bank = {};
    bank.out_stride = out_stride;
    bank.channels = channels;
    for (int j = 0; j < channels; j++) {
        bank.off[j] = offsets[j];
        bank.period[j] = periods[j];
        bank.ph[j] = (int)((g.k_begin * g.D) % periods[j]);
    }
    // launch-bound sizes compute their Cross outputs inside the tile kernel: launch_tuner_fused's decision
    const bool inl = g.seamBI > 0 && g.count <= 5 * (int64_t)small_launch_outputs();
    bool inlined = false;
#define TUNER_BANK_I16(DV, TCV, GV) launch_tuner_bank_c4_i16<DV, 128, TCV, GV>(s, g, d_plain_taps, d_in, d_out, inl, &inlined, d_tables, bank)
    if (g.D == 4) TUNER_BANK_I16(4, 4, true);
    else if (g.D == 16) { if (P % 8 == 0) TUNER_BANK_I16(16, 8, true); else TUNER_BANK_I16(16, 4, true); }
    else if (P == 128) TUNER_BANK_I16(8, 8, false);      // the exact-length walk for the full 128 taps
    else if (P % 8 == 0) TUNER_BANK_I16(8, 8, true);
    else TUNER_BANK_I16(8, 4, true);
#undef TUNER_BANK_I16
    g_tuner_i16_launches.fetch_add(1, std::memory_order_relaxed);
    if (counts_as_bank) g_tuner_i16_bank_launches.fetch_add(1, std::memory_order_relaxed);

    const SeamSpan sp = seam_span(g);
    if (sp.nseams > 0 && !inlined) {
        const unsigned per_channel = (unsigned)(((int64_t)sp.nseams * sp.per + 255) / 256);
        const dim3 grid(per_channel * (unsigned)channels), block(256);
        hipLaunchKernelGGL(k_tuner_bank_crossfix_i16, grid, block, 0, s, g, d_cross_taps, reinterpret_cast<const short2*>(d_in), d_out,
                           sp.first, sp.nseams, sp.per, reinterpret_cast<const float2*>(d_tables), bank);
    }
    return true;
}

bool launch_tuner_bank_cross_i16(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, float* d_out,
                                 int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods)
{
    // launch_tuner_bank_cross's refusals; one thread reads its window sample by sample: no alignment beyond the sample's own 4 bytes
    if (channels < 1 || channels > kTunerBankMaxChannels || (out_stride & 1) != 0) return false;
    if (channels > 1 && out_stride < 2 * (int64_t)g.count) return false;
    if (g.I != 1 || g.count <= 0 || g.k_begin < 0 || g.k_begin * g.D < g.in_base || d_cross_taps == nullptr) return false;
    if ((reinterpret_cast<uintptr_t>(d_out) & 7) != 0 || (reinterpret_cast<uintptr_t>(d_in) & 3) != 0) return false;
    BankChannelsI16 bank = {};
    bank.out_stride = out_stride;
    bank.channels = channels;
    for (int j = 0; j < channels; j++) {
        if (periods[j] < 1) return false;
        bank.off[j] = offsets[j];
        bank.period[j] = periods[j];
    }
    const unsigned per_channel = (unsigned)(((int64_t)g.count + 255) / 256);        // at most 2^23: times 32 channels fits a 1-D grid
    const dim3 grid(per_channel * (unsigned)channels), block(256);
    hipLaunchKernelGGL(k_tuner_bank_cross_i16, grid, block, 0, s, g, d_cross_taps, reinterpret_cast<const short2*>(d_in), d_out,
                       reinterpret_cast<const float2*>(d_tables), bank);
    g_tuner_i16_cross_launches.fetch_add(1, std::memory_order_relaxed);
    return true;
}

void launch_tuner_mix_i16(hipStream_t s, const void* d_in, float* d_out, int64_t n, const float* d_osc, int period, int ph0)
{
    if (n <= 0) return;
    int64_t blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    hipLaunchKernelGGL(k_tuner_mix_i16, dim3((unsigned)blocks), dim3(256), 0, s, reinterpret_cast<const short2*>(d_in),
                       reinterpret_cast<float2*>(d_out), (uint32_t)n, reinterpret_cast<const float2*>(d_osc), period, ph0);
}

}  // namespace sdrhip
