// kernels_tuner_bank.hip -- the tuner bank (sdrhip_tuner_bank_run): K tuners of the same decimator over ONE input in one launch.
//
// k_tuner_bank_c4 is k_tuner_c4 (kernels_tuner.hip) with a channel axis: tile geometry, raw loads, mixing loader (tuner_mix.hpp), MAC
// walk, fold and in-tile Cross outputs are that kernel's, line for line; a channel index j selects the table (osc + off[j],
// period[j] entries), the phase of the launch's first sample (ph[j] = (k_begin D) mod period[j], the host's one 64-bit modulo per
// channel and launch) and the output row (out + j * out_stride), nothing else.  The per-channel values travel in the kernel's
// arguments (BankChannels, 400 bytes, as BankStations of kernels_small.hip): j is uniform over the workgroup, so they are scalar loads
// from the argument segment, and a run needs no host-to-device copy.
//
// Dispatch order: a flat 1-D grid of tiles * K workgroups, channel = b % K the FASTEST axis, tile = b / K.  The K workgroups that read
// one input tile are handed out back to back, so the tile comes from HBM once and the other K - 1 readers find it in the Infinity
// Cache while it is fresh there; a 1-D grid has no 65535 limit (a launch of 2^31 outputs x 32 channels is 2^27 workgroups).
// k_tuner_c4's XCD-aware permutation of blockIdx.x is DROPPED here: it was derived for a grid without a channel axis (XCD = b % 8
// takes 8 consecutive tiles of every 64), and with the channel in the low bits of b the XCD of a workgroup is (tile K + j) % 8 -- for
// K a multiple of 8 every channel already stays on one XCD and walks consecutive tiles there, which is what the permutation was
// for.  No re-derived order was tried and the dropped one was not measured against: the figures of profiles/tuner_bank_bench.txt are
// of this plain order.
//
// Output stores: 16-byte stores where the ROW's pointer is 16-byte aligned, else 8-byte ones -- with out_stride = 2 (mod 4) every
// odd row is only 8-byte aligned whatever the base is.
//
// Cross outputs of launches too long to compute them in the tile: k_tuner_bank_crossfix, k_tuner_crossfix's body with the same
// channel axis (block b: channel b % K, slots of block b / K), one launch for all channels over seam_span(g).
//
// The bank's Pipe (pipes.cpp): a block of another size than its predecessors has no seam_block, so its submission is the outputs that
// straddle the boundary (all Cross) and then the outputs inside the block (all One).  k_tuner_bank_cross is the first part for every
// channel in one launch: k_tuner_bank_crossfix's body over an explicit output range.  sdrhip_tuner_bank_run never takes it.
//
// Input formats: every kernel here takes the format as FMT (InFmt: cfloat, u8 IQ, int16 IQ); the staging and the mixing store of a
// tile are Stage<T, FMT, NT> and tuner_store<T, FMT, NT>, one sample of the sequential-order kernels is tuner_sample<FMT>.  Every
// launch writes the bits of the cfloat launch on the converted samples.  The one-row tuner on int16 has no kernel of its own: its
// fused route is k_tuner_bank_c4 with ONE channel (table offset 0), a launch that counts as an int16 launch and not as a banked one.
//
// Output kinds: k_tuner_bank_c4, k_tuner_bank_crossfix and k_tuner_bank_cross take OUT beside FMT.  OUT_IQ stores the finished (re, im), as above.  OUT_ENV
// (the AM bank, am_bank.cpp) stores am_magnitude(re, im) (am.hpp: Data.Complex.magnitude at Float) of the SAME finished output, one
// float per output, into float rows out_stride floats apart: staging, mix, MAC walk, fold and Cross outputs are untouched, so the
// value under the magnitude is the OUT_IQ launch's bit for bit.  Any out_stride >= count, any float-aligned row: a thread's pair is one
// 8-byte store where row pointer + output index is 8-byte aligned and both outputs exist, 4-byte stores otherwise (the two
// sequential-order kernels hold one output a thread: 4-byte stores).
//
// OUT_FM (the narrow-band FM bank, nfm_bank.cpp) stores fm_phase(y[k], y[k - 1]) (demod.hpp: fmDemod, Demod.hs:25-28) of the SAME finished
// outputs, one float per output, with OUT_ENV's store rule.  fmDemod is not point-wise, so:
//   - inside a tile a thread's first output takes its predecessor from the previous thread's second one, through NT pairs of LDS behind
//     the tile (one barrier after the MAC walk and the Cross outputs);
//   - across tiles NO workgroup waits on another: the tiles OVERLAP.  A tile still computes T::OUTS outputs but advances by T::OUTS - 2;
//     thread 0's pair of every tile but the first is computed as a predecessor only and not stored, the first tile stores all of its
//     outputs and its output 0 takes the predecessor from bank.fm_state (channel j's decimated output k_begin - 1; null = (0, 0),
//     Demod.hs:41).  2 of 512 outputs are computed twice (0.4 %), tile starts stay multiples of 16 bytes (510 D samples of 2, 4 or 8
//     bytes, D = 4 / 8 / 16), and the oscillator phase and the seam arithmetic of a tile follow the advance;
//   - Cross outputs are ALWAYS computed in the tile (a later fix-up launch could not repair the two phase differences a Cross output
//     takes part in), for any seam_block in [Lp, 2^30): the in-tile test reduces by a modulo where the other kinds subtract once, so a
//     tile may hold any number of seams.  k_tuner_bank_crossfix has no OUT_FM form;
//   - the thread that stores output count - 1 also writes its (re, im) to bank.fm_final[j] (null = not wanted): the next launch's state.
// k_tuner_bank_cross<FMT, OUT_FM>: thread t computes y[t] and recomputes y[t - 1], both in sequential order; thread 0 takes fm_state.
#include "am.hpp"
#include "demod.hpp"
#include "decimate_tile.hpp"
#include "tuner_mix.hpp"

namespace sdrhip {

static std::atomic<long long> g_tuner_bank_launches{0};
long long tuner_bank_launch_count() { return g_tuner_bank_launches.load(); }
static std::atomic<long long> g_tuner_bank_cross_launches{0};
long long tuner_bank_cross_launch_count() { return g_tuner_bank_cross_launches.load(); }
static std::atomic<long long> g_tuner_i16_launches{0};
long long tuner_i16_launch_count() { return g_tuner_i16_launches.load(); }
static std::atomic<long long> g_am_bank_launches{0};
long long am_bank_launch_count() { return g_am_bank_launches.load(); }
static std::atomic<long long> g_am_bank_fixup_launches{0};
long long am_bank_fixup_launch_count() { return g_am_bank_fixup_launches.load(); }
static std::atomic<long long> g_am_bank_cross_launches{0};
long long am_bank_cross_launch_count() { return g_am_bank_cross_launches.load(); }
static std::atomic<long long> g_nfm_bank_launches{0};
long long nfm_bank_launch_count() { return g_nfm_bank_launches.load(); }
static std::atomic<long long> g_nfm_bank_cross_launches{0};
long long nfm_bank_cross_launch_count() { return g_nfm_bank_cross_launches.load(); }

namespace {

struct BankChannels {
    int64_t out_stride;                        // floats between the channels' output rows
    int channels;
    int off[kTunerBankMaxChannels];            // first entry of the channel's table, in (re, im) pairs
    int period[kTunerBankMaxChannels];
    int ph[kTunerBankMaxChannels];             // (k_begin D) mod period: the host's one 64-bit modulo per channel and launch
};
// OUT_FM's argument: the channels and the two state arrays, K (re, im) pairs each.  A type of its own, so that the argument segment of
// the other kinds (and with it the offsets of their hidden arguments) stays what it was.
struct BankChannelsFm : BankChannels {
    const float* fm_state;                     // channel j's decimated output k_begin - 1; null = (0, 0)
    float* fm_final;                           // receives output k_end - 1; null = not wanted
};
template <int OUT> struct BankArg { using type = BankChannels; };
template <> struct BankArg<OUT_FM> { using type = BankChannelsFm; };

// outputs a tile advances by, and the tiles of a launch: OUT_FM's tiles overlap by one thread's pair (see the head of this file)
template <class T, int OUT>
constexpr int tile_advance() { return OUT == OUT_FM ? T::OUTS - 2 : T::OUTS; }
template <class T, int OUT>
__host__ __device__ __forceinline__ int tile_count(int count)
{
    if constexpr (OUT == OUT_FM) return count <= T::OUTS ? 1 : (count - 2 + tile_advance<T, OUT>() - 1) / tile_advance<T, OUT>();
    else return (count + T::OUTS - 1) / T::OUTS;
}

template <int D, int P, int R, int NT, int FMT, int OUT, int TC, bool GUARD>
__global__ void __launch_bounds__(NT) k_tuner_bank_c4(const void* __restrict__ in, int64_t x0 /* sample index of output 0's window in `in` */,
                                                      int count, const float* __restrict__ taps /* plain */, float* __restrict__ out,
                                                      int p_eff /* GUARD: taps of the filter (multiple of TC, <= P) */,
                                                      int inl_seam /* > 0: compute the Cross outputs of buffers this long HERE */,
                                                      int inl_r0 /* window start of output 0 inside its buffer */,
                                                      const float2* __restrict__ osc /* every table */, typename BankArg<OUT>::type bank)
{
    using T = Tile<D, P, R, NT>;
    using St = Stage<T, FMT, NT>;
    constexpr int NP = 4, ORD = 0;                           // the AVX "RC" order
    extern __shared__ __attribute__((aligned(16))) unsigned char tuner_bank_smem[];
    float2* lds = reinterpret_cast<float2*>(tuner_bank_smem);

    const int ntiles = tile_count<T, OUT>(count);
    const unsigned nch = (unsigned)bank.channels;
    const unsigned j = blockIdx.x % nch;
    const int tile = (int)(blockIdx.x / nch);
    if (tile >= ntiles) return;
    osc += bank.off[j];
    out += (int64_t)j * bank.out_stride;

    const int out0 = tile * tile_advance<T, OUT>();
    const int64_t s0 = (int64_t)out0 * D;                     // first sample of the tile, relative to x0
    {
        St st;
        const int64_t total_avail = (int64_t)(count - 1) * D + (GUARD ? p_eff : P);      // samples that exist from x0 on
        const int64_t av = total_avail - s0;
        st.load(in, x0 + s0, av > T::SPAN ? T::SPAN : (int)av);
        const uint32_t n = (uint32_t)bank.period[j];
        constexpr uint32_t TS = (uint32_t)tile_advance<T, OUT>() * D;
        const uint32_t ph = ((uint32_t)bank.ph[j] + (((uint32_t)tile % n) * (TS % n)) % n + (uint32_t)(threadIdx.x * St::SPV)) % n;
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
            if constexpr (OUT == OUT_FM) rr %= inl_seam;      // any seam >= plen: a tile may hold several (rr < 2^30 + OUTS D)
            else if (rr >= inl_seam) rr -= inl_seam;
            cross[r] = rr + plen > inl_seam;
            any |= cross[r];
        }
        if (any) inline_cross_outputs<D, R, T, TC, GUARD>(win, taps, plen, cross, res);
    }
    if constexpr (OUT == OUT_FM) {
        // the predecessor of a thread's first output is the previous thread's last one: NT pairs behind the tile (the tile itself
        // may still be being read by slower waves)
        float2* edge = lds + T::LDS_F2;
        edge[threadIdx.x] = res[R - 1];
        __syncthreads();
        // thread 0 of a later tile holds predecessors only: nothing of it is stored, and it takes its own last output for a
        // predecessor so that it does not send its wave into the full form
        const bool lead = tile > 0 && threadIdx.x == 0;
        float2 v[R + 1];
        if (threadIdx.x > 0) v[0] = edge[threadIdx.x - 1];
        else if (tile > 0) v[0] = res[R - 1];
        else if (bank.fm_state != nullptr) v[0] = make_float2(bank.fm_state[2 * j], bank.fm_state[2 * j + 1]);
        else v[0] = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int r = 0; r < R; r++) v[r + 1] = res[r];
        float y[R];
        fm_phase_voted<R>(v, y);
        if (lead) return;
        float* dst = out + o;
        if (R == 2 && o + R <= count && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
            *reinterpret_cast<float2*>(dst) = make_float2(y[0], y[R - 1]);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (o + r < count) dst[r] = y[r];
        }
        // the state of the next launch, by the thread that has stored the launch's last output
        if (bank.fm_final != nullptr) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (o + r == count - 1) {
                    bank.fm_final[2 * j] = res[r].x;
                    bank.fm_final[2 * j + 1] = res[r].y;
                }
        }
        return;
    }
    if constexpr (OUT == OUT_ENV) {
        // one float per output: the pair as ONE 8-byte store where the row's pointer plus the output index is 8-byte aligned (the
        // ROW's pointer decides again: an odd stride or a launch cut at an odd output moves it) and both lie inside count
        float env[R];
#pragma unroll
        for (int r = 0; r < R; r++) env[r] = am_magnitude(res[r].x, res[r].y);
        float* dst = out + o;
        if (R == 2 && o + R <= count && (reinterpret_cast<uintptr_t>(dst) & 7) == 0) {
            *reinterpret_cast<float2*>(dst) = make_float2(env[0], env[R - 1]);
        } else {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (o + r < count) dst[r] = env[r];
        }
        return;
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

// Cross outputs of every channel, one thread per candidate slot of a seam and channel (k_tuner_crossfix with the channel axis)
template <int FMT, int OUT>
__global__ void __launch_bounds__(256) k_tuner_bank_crossfix(Geom g, const float* __restrict__ xtaps, const void* __restrict__ in,
                                                              float* __restrict__ out, int64_t first_seam, int nseams, int per_seam,
                                                              const float2* __restrict__ osc, BankChannels bank)
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
        const float2 mx = tuner_mul(tuner_sample<FMT>(in, v - g.in_base + j), osc[ph]);
        ph = wrap_inc(ph, n);
        re = re + mx.x * xtaps[j];
        im = im + mx.y * xtaps[j];
    }
    if constexpr (OUT == OUT_ENV) out[m - g.k_begin] = am_magnitude(re, im);
    else *reinterpret_cast<float2*>(out + 2 * (m - g.k_begin)) = make_float2(re, im);
}

// Outputs [g.k_begin, g.k_begin + g.count) of every channel, ALL of them Cross (the straddlers of a boundary between two blocks of
// unequal size, which no seam_block describes): k_tuner_bank_crossfix's body on an explicit range instead of a seam's candidate
// slots.  Block b: channel b % K, outputs of block b / K.
template <int FMT, int OUT>
__global__ void __launch_bounds__(256) k_tuner_bank_cross(Geom g, const float* __restrict__ xtaps, const void* __restrict__ in,
                                                           float* __restrict__ out, const float2* __restrict__ osc,
                                                           typename BankArg<OUT>::type bank)
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
        const float2 mx = tuner_mul(tuner_sample<FMT>(in, v - g.in_base + j), osc[ph]);
        ph = wrap_inc(ph, n);
        re = re + mx.x * xtaps[j];
        im = im + mx.y * xtaps[j];
    }
    if constexpr (OUT == OUT_FM) {
        // the predecessor: output t - 1 once more, the same loop one window earlier (at most 16 outputs a channel in the Pipe's
        // launches); thread 0 takes the state
        float2 prev = make_float2(0.0f, 0.0f);
        if (t > 0) {
            const int64_t u = v - g.D;
            uint32_t pq = (uint32_t)((uint64_t)u % n);
            float pr = 0.0f, pi = 0.0f;
            for (int j = 0; j < g.Lp; j++) {
                const float2 mx = tuner_mul(tuner_sample<FMT>(in, u - g.in_base + j), osc[pq]);
                pq = wrap_inc(pq, n);
                pr = pr + mx.x * xtaps[j];
                pi = pi + mx.y * xtaps[j];
            }
            prev = make_float2(pr, pi);
        } else if (bank.fm_state != nullptr) {
            prev = make_float2(bank.fm_state[2 * c], bank.fm_state[2 * c + 1]);
        }
        out[t] = fm_phase_sel(make_float2(re, im), prev);
        if (t == g.count - 1 && bank.fm_final != nullptr) {
            bank.fm_final[2 * c] = re;
            bank.fm_final[2 * c + 1] = im;
        }
        return;
    }
    if constexpr (OUT == OUT_ENV) out[t] = am_magnitude(re, im);
    else *reinterpret_cast<float2*>(out + 2 * (int64_t)t) = make_float2(re, im);
}

template <int D, int P, int FMT, int OUT, int TC, bool GUARD>
void launch_tuner_bank_c4(hipStream_t s, const Geom& g, const float* taps, const void* in, float* out, bool inline_cross, bool* inlined,
                          const float* d_tables, const typename BankArg<OUT>::type& bank)
{
    constexpr int R = 2, NT = 256;
    using T = Tile<D, P, R, NT>;
    // OUT_FM: NT pairs behind the tile, the threads' last outputs (the predecessors of their right neighbours' first ones)
    constexpr size_t lds_bytes = T::LDS_BYTES + (OUT == OUT_FM ? NT * sizeof(float2) : 0);
    // the dynamic-LDS attribute is per device: one flag per (instantiation, device); idempotent, a race only repeats the call
    static std::atomic<bool> attr_set[64];
    auto kern = k_tuner_bank_c4<D, P, R, NT, FMT, OUT, TC, GUARD>;
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    const int tiles = tile_count<T, OUT>(g.count);             // at most 2^22 + 2^14: tiles * channels fits a 1-D grid
    const unsigned grid = (unsigned)tiles * (unsigned)bank.channels;
    const int64_t x0 = g.k_begin * D - g.in_base;
    int inl_seam = 0, inl_r0 = 0;
    // a tile spans less than one buffer; OUT_FM's modulo takes any seam the launcher has admitted (Lp <= seam < 2^30)
    if (inline_cross && (OUT == OUT_FM || g.seamBI >= (int64_t)T::OUTS * D + g.Lp) && g.seamBI < (1 << 30)) {
        inl_seam = (int)g.seamBI;
        inl_r0 = (int)((g.k_begin * D) % g.seamBI);
    }
    *inlined = inl_seam > 0;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT), lds_bytes, s, in, x0, g.count, taps, out, g.Lp, inl_seam, inl_r0,
                       reinterpret_cast<const float2*>(d_tables), bank);
}

// the instantiation that serves the launch's shape (tuner_fused_fits has admitted it)
template <int FMT, int OUT>
void launch_tuner_bank_c4_shape(hipStream_t s, const Geom& g, int P, const float* taps, const void* in, float* out, bool inl, bool* inlined,
                                const float* d_tables, const typename BankArg<OUT>::type& bank)
{
#define TUNER_BANK(DV, TCV, GV) launch_tuner_bank_c4<DV, 128, FMT, OUT, TCV, GV>(s, g, taps, in, out, inl, inlined, d_tables, bank)
    if (g.D == 4) TUNER_BANK(4, 4, true);
    else if (g.D == 16) { if (P % 8 == 0) TUNER_BANK(16, 8, true); else TUNER_BANK(16, 4, true); }
    else if (P == 128) TUNER_BANK(8, 8, false);      // the exact-length walk for the full 128 taps
    else if (P % 8 == 0) TUNER_BANK(8, 8, true);
    else TUNER_BANK(8, 4, true);
#undef TUNER_BANK
}

// launch_tuner_bank (OUT_IQ: out_stride in floats of complex rows), launch_am_bank (OUT_ENV: one float per output) and
// launch_nfm_bank (OUT_FM: one float per output, the state pairs fm_state / fm_final, every Cross output in the tile launch)
template <int OUT>
bool launch_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in, InFmt fmt,
                 float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods,
                 bool counts_as_bank, const float* fm_state = nullptr, float* fm_final = nullptr)
{
    constexpr int64_t FPO = OUT == OUT_IQ ? 2 : 1;          // floats per output
    if (channels < 1 || channels > kTunerBankMaxChannels) return false;
    if (OUT == OUT_IQ && (out_stride & 1) != 0) return false;
    if (channels > 1 && out_stride < FPO * (int64_t)g.count) return false;
    // tuner_fused_fits reads d_out for the 8-byte alignment of complex rows alone; envelope and phase rows are floats at any float address
    if (OUT != OUT_IQ && (reinterpret_cast<uintptr_t>(d_out) & 3) != 0) return false;
    if (OUT == OUT_FM && g.seamBI >= ((int64_t)1 << 30)) return false;      // the in-tile seam test works in 32 bits
    const void* fit_out = OUT != OUT_IQ ? nullptr : d_out;
    for (int j = 0; j < channels; j++)
        if (!tuner_fused_fits(g, P, d_cross_taps != nullptr, d_in, fmt, fit_out, periods[j])) return false;
    typename BankArg<OUT>::type bank = {};
    bank.out_stride = out_stride;
    bank.channels = channels;
    if constexpr (OUT == OUT_FM) {
        bank.fm_state = fm_state;
        bank.fm_final = fm_final;
    }
    for (int j = 0; j < channels; j++) {
        bank.off[j] = offsets[j];
        bank.period[j] = periods[j];
        bank.ph[j] = (int)((g.k_begin * g.D) % periods[j]);
    }
    // launch-bound sizes compute their Cross outputs inside the tile kernel: launch_tuner_fused's decision
    // (OUT_FM: always, whatever the size)
    const bool inl = g.seamBI > 0 && (OUT == OUT_FM || g.count <= 5 * (int64_t)small_launch_outputs());
    bool inlined = false;
    switch (fmt) {
    case IN_U8: launch_tuner_bank_c4_shape<IN_U8, OUT>(s, g, P, d_plain_taps, d_in, d_out, inl, &inlined, d_tables, bank); break;
    case IN_I16: launch_tuner_bank_c4_shape<IN_I16, OUT>(s, g, P, d_plain_taps, d_in, d_out, inl, &inlined, d_tables, bank); break;
    default: launch_tuner_bank_c4_shape<IN_CF32, OUT>(s, g, P, d_plain_taps, d_in, d_out, inl, &inlined, d_tables, bank); break;
    }
    if (fmt == IN_I16) g_tuner_i16_launches.fetch_add(1, std::memory_order_relaxed);
    if (OUT == OUT_ENV) g_am_bank_launches.fetch_add(1, std::memory_order_relaxed);
    else if (OUT == OUT_FM) g_nfm_bank_launches.fetch_add(1, std::memory_order_relaxed);
    else if (counts_as_bank) g_tuner_bank_launches.fetch_add(1, std::memory_order_relaxed);

    if constexpr (OUT != OUT_FM) {
    const SeamSpan sp = seam_span(g);
    if (sp.nseams > 0 && !inlined) {
        const unsigned per_channel = (unsigned)(((int64_t)sp.nseams * sp.per + 255) / 256);
        const dim3 grid(per_channel * (unsigned)channels), block(256);
        auto fix = fmt == IN_U8 ? k_tuner_bank_crossfix<IN_U8, OUT> : fmt == IN_I16 ? k_tuner_bank_crossfix<IN_I16, OUT>
                                                                                    : k_tuner_bank_crossfix<IN_CF32, OUT>;
        hipLaunchKernelGGL(fix, grid, block, 0, s, g, d_cross_taps, d_in, d_out, sp.first, sp.nseams, sp.per,
                           reinterpret_cast<const float2*>(d_tables), bank);
        if (OUT == OUT_ENV) g_am_bank_fixup_launches.fetch_add(1, std::memory_order_relaxed);
    }
    }
    return true;
}

}  // namespace

bool launch_tuner_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                       InFmt fmt, float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets,
                       const int* periods, bool counts_as_bank)
{
    return launch_bank<OUT_IQ>(s, g, d_plain_taps, P, d_cross_taps, d_in, fmt, d_out, out_stride, d_tables, channels, offsets, periods,
                               counts_as_bank);
}

bool launch_am_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                    InFmt fmt, float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets,
                    const int* periods)
{
    return launch_bank<OUT_ENV>(s, g, d_plain_taps, P, d_cross_taps, d_in, fmt, d_out, out_stride, d_tables, channels, offsets, periods,
                                false);
}

bool launch_nfm_bank(hipStream_t s, const Geom& g, const float* d_plain_taps, int P, const float* d_cross_taps, const void* d_in,
                     InFmt fmt, float* d_out, int64_t out_stride, const float* d_tables, int channels, const int* offsets,
                     const int* periods, const float* d_state, float* d_final)
{
    return launch_bank<OUT_FM>(s, g, d_plain_taps, P, d_cross_taps, d_in, fmt, d_out, out_stride, d_tables, channels, offsets, periods,
                               false, d_state, d_final);
}

namespace {
// launch_tuner_bank_cross (OUT_IQ), launch_am_bank_cross (OUT_ENV: float rows, any out_stride >= g.count, 4-byte stores) and
// launch_nfm_bank_cross (OUT_FM: as OUT_ENV, with the state pairs)
template <int OUT>
bool launch_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                       int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods,
                       const float* fm_state = nullptr, float* fm_final = nullptr)
{
    // launch_tuner_bank's refusals for channels and stride; one thread reads its window sample by sample: no alignment beyond the
    // element's own (a float, a u8 pair, an int16 pair)
    static const uintptr_t kInMask[3] = {/* IN_CF32 */ 7, /* IN_U8 */ 1, /* IN_I16 */ 3};
    constexpr int64_t FPO = OUT == OUT_IQ ? 2 : 1;          // floats per output
    if (channels < 1 || channels > kTunerBankMaxChannels) return false;
    if (OUT == OUT_IQ && (out_stride & 1) != 0) return false;
    if (channels > 1 && out_stride < FPO * (int64_t)g.count) return false;
    if (g.I != 1 || g.count <= 0 || g.k_begin < 0 || g.k_begin * g.D < g.in_base || d_cross_taps == nullptr) return false;
    if ((reinterpret_cast<uintptr_t>(d_out) & (OUT != OUT_IQ ? 3 : 7)) != 0 || (reinterpret_cast<uintptr_t>(d_in) & kInMask[fmt]) != 0) return false;
    typename BankArg<OUT>::type bank = {};
    bank.out_stride = out_stride;
    bank.channels = channels;
    if constexpr (OUT == OUT_FM) {
        bank.fm_state = fm_state;
        bank.fm_final = fm_final;
    }
    for (int j = 0; j < channels; j++) {
        if (periods[j] < 1) return false;
        bank.off[j] = offsets[j];
        bank.period[j] = periods[j];
    }
    const unsigned per_channel = (unsigned)(((int64_t)g.count + 255) / 256);        // at most 2^23: times 32 channels fits a 1-D grid
    const dim3 grid(per_channel * (unsigned)channels), block(256);
    auto cross = fmt == IN_U8 ? k_tuner_bank_cross<IN_U8, OUT> : fmt == IN_I16 ? k_tuner_bank_cross<IN_I16, OUT> : k_tuner_bank_cross<IN_CF32, OUT>;
    hipLaunchKernelGGL(cross, grid, block, 0, s, g, d_cross_taps, d_in, d_out, reinterpret_cast<const float2*>(d_tables), bank);
    (OUT == OUT_ENV ? g_am_bank_cross_launches : OUT == OUT_FM ? g_nfm_bank_cross_launches : g_tuner_bank_cross_launches)
        .fetch_add(1, std::memory_order_relaxed);
    return true;
}
}  // namespace

bool launch_tuner_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                             int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods)
{
    return launch_bank_cross<OUT_IQ>(s, g, d_cross_taps, d_in, fmt, d_out, out_stride, d_tables, channels, offsets, periods);
}

bool launch_am_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                          int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods)
{
    return launch_bank_cross<OUT_ENV>(s, g, d_cross_taps, d_in, fmt, d_out, out_stride, d_tables, channels, offsets, periods);
}

bool launch_nfm_bank_cross(hipStream_t s, const Geom& g, const float* d_cross_taps, const void* d_in, InFmt fmt, float* d_out,
                           int64_t out_stride, const float* d_tables, int channels, const int* offsets, const int* periods,
                           const float* d_state, float* d_final)
{
    return launch_bank_cross<OUT_FM>(s, g, d_cross_taps, d_in, fmt, d_out, out_stride, d_tables, channels, offsets, periods, d_state,
                                     d_final);
}

}  // namespace sdrhip
