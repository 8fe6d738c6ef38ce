// kernels_agc.hip -- agc / agcPipe (hs_sources/SDR/Util.hs:325-348).
//
//     corrected = x[i] `cmul` state                              (two f32 multiplies: the output sample)
//     state'    = state + mu * (reference - magnitude corrected)  (f32, evaluated as written, no FMA)
//
// `magnitude` is GHC base's Data.Complex.magnitude at Float: scale both parts by 2^-k, k the larger frexp exponent, square,
// add, sqrt, scale back (agc_magnitude below).  Not sqrtf(re*re + im*im): the two differ where a square under- or overflows.
//
// The state is rounded every step, so no associative scan gives the reference's bits.  As for dcBlocker (kernels_iir.hip):
// state' = state * (1 - mu*|x|) + mu*reference up to rounding is a contraction wherever 0 < mu*|x| < 2, so a lane that
// starts W samples before its chunk from a guessed state meets the true trajectory bit for bit, after which the two are
// identical for good.
//   1. k_agc_speculate: one lane per chunk of C samples runs in from W samples earlier, starting from the state the call
//      started with (the best guess there is: a Pipe in steady state hands over a state near the equilibrium), records
//      the state it reaches at the chunk start, writes its chunk, records its end state.  Chunks whose run-in reaches
//      sample 0 start there from the true state and are exact.
//   2. k_agc_repair (a few rounds, all chunks in parallel): a chunk whose start state differs from its predecessor's current
//      end state is recomputed from that state.
//   3. k_agc_settle (one workgroup) checks the chain once more in parallel.  What is still inconsistent is walked by one
//      lane.  Unlike dcBlocker's, the output is NOT the state (x = 0 gives equal outputs from any state), so the walk
//      cannot stop at "my value equals what is stored": it recomputes a whole chunk from the true state, compares the
//      chunk's END state with the stored one, and goes on into the next chunk while that chunk's stored start state
//      differs from the end state just computed.
// The result is the sequential result by construction, whatever the input, mu or run-in (a non-contracting mu*|x| > 2
// only makes it slow).  The contraction rate is mu*|x|, so the run-in is a function of mu (agc_default_run_in) and the
// chunk length is tied to it: a chunk shorter than the run-in would spend most of a lane on redundant work.
#include <stdlib.h>

#include <atomic>

#include "kernels.hpp"

namespace sdrhip {

// Data.Complex.magnitude at Float: exponent 0 = 0, otherwise frexp's exponent (denormals normalised); scaleFloat = ldexpf
// with one rounding; sqrtf is correctly rounded (hipcc's default).  Zero passes through ldexpf unchanged.
__device__ __forceinline__ float agc_magnitude(float re, float im)
{
    int er, ei;
    (void)frexpf(re, &er);
    (void)frexpf(im, &ei);
    const int k = er > ei ? er : ei;
    const float a = ldexpf(re, -k), b = ldexpf(im, -k);
    return ldexpf(sqrtf(a * a + b * b), k);
}

// one sample: the corrected sample goes to (ore, oim), the new state is returned
__device__ __forceinline__ float agc_step(float re, float im, float s, float mu, float ref, float& ore, float& oim)
{
    ore = re * s;
    oim = im * s;
    return s + mu * (ref - agc_magnitude(ore, oim));
}

// Samples [i, end) from state s; returns the state after them.  A = access width both pointers allow: 2 = 16-byte (two
// samples; i is even then), 1 = 8-byte, 0 = 4-byte.  Loads run ahead of the dependent chain: the next group of eight
// samples is requested before the current one is consumed.
template <int A, bool WRITE>
__device__ __forceinline__ float agc_walk_a(const float* __restrict__ in, float* __restrict__ out, int64_t i, int64_t end,
                                            float s, float mu, float ref)
{
    if (A == 2) {
        if (i + 8 <= end) {
            const float4* p = reinterpret_cast<const float4*>(in + 2 * i);
            float4 v0 = p[0], v1 = p[1], v2 = p[2], v3 = p[3];
            for (; i + 8 <= end; i += 8) {
                const int64_t nx = i + 16 <= end ? i + 8 : i;   // the last group re-reads itself
                const float4* q = reinterpret_cast<const float4*>(in + 2 * nx);
                const float4 n0 = q[0], n1 = q[1], n2 = q[2], n3 = q[3];
                float4 o0, o1, o2, o3;
                s = agc_step(v0.x, v0.y, s, mu, ref, o0.x, o0.y);
                s = agc_step(v0.z, v0.w, s, mu, ref, o0.z, o0.w);
                s = agc_step(v1.x, v1.y, s, mu, ref, o1.x, o1.y);
                s = agc_step(v1.z, v1.w, s, mu, ref, o1.z, o1.w);
                s = agc_step(v2.x, v2.y, s, mu, ref, o2.x, o2.y);
                s = agc_step(v2.z, v2.w, s, mu, ref, o2.z, o2.w);
                s = agc_step(v3.x, v3.y, s, mu, ref, o3.x, o3.y);
                s = agc_step(v3.z, v3.w, s, mu, ref, o3.z, o3.w);
                if (WRITE) {
                    float4* w = reinterpret_cast<float4*>(out + 2 * i);
                    w[0] = o0; w[1] = o1; w[2] = o2; w[3] = o3;
                }
                v0 = n0; v1 = n1; v2 = n2; v3 = n3;
            }
        }
        for (; i + 2 <= end; i += 2) {
            const float4 v = *reinterpret_cast<const float4*>(in + 2 * i);
            float4 o;
            s = agc_step(v.x, v.y, s, mu, ref, o.x, o.y);
            s = agc_step(v.z, v.w, s, mu, ref, o.z, o.w);
            if (WRITE) *reinterpret_cast<float4*>(out + 2 * i) = o;
        }
    }
    for (; i < end; i++) {
        float re, im, ore, oim;
        if (A >= 1) {
            const float2 v = *reinterpret_cast<const float2*>(in + 2 * i);
            re = v.x; im = v.y;
        } else {
            re = in[2 * i]; im = in[2 * i + 1];
        }
        s = agc_step(re, im, s, mu, ref, ore, oim);
        if (WRITE) {
            if (A >= 1) {
                *reinterpret_cast<float2*>(out + 2 * i) = make_float2(ore, oim);
            } else {
                out[2 * i] = ore; out[2 * i + 1] = oim;
            }
        }
    }
    return s;
}

template <bool WRITE>
__device__ __forceinline__ float agc_walk(int acc, const float* __restrict__ in, float* __restrict__ out, int64_t i,
                                          int64_t end, float s, float mu, float ref)
{
    if (acc == 2) return agc_walk_a<2, WRITE>(in, out, i, end, s, mu, ref);
    if (acc == 1) return agc_walk_a<1, WRITE>(in, out, i, end, s, mu, ref);
    return agc_walk_a<0, WRITE>(in, out, i, end, s, mu, ref);
}

// C and W are multiples of 8 samples: with 16-byte aligned pointers every lane walks whole 64-byte groups except at the end.
__global__ void __launch_bounds__(64)
k_agc_speculate(int64_t num, int64_t C, int64_t W, float mu, float ref, float state, const float* __restrict__ d_state,
                const float* __restrict__ in, float* __restrict__ out, uint32_t* __restrict__ s_start,
                uint32_t* __restrict__ s_end, int nchunks, int acc)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nchunks) return;
    const int64_t begin = (int64_t)j * C;
    const int64_t end = begin + C < num ? begin + C : num;
    int64_t i = begin - W;
    if (i < 0) i = 0;
    float s = d_state ? d_state[0] : state;   // a Pipe keeps the state on the device between blocks
    s = agc_walk<false>(acc, in, out, i, begin, s, mu, ref);
    s_start[j] = __float_as_uint(s);
    s = agc_walk<true>(acc, in, out, begin, end, s, mu, ref);
    s_end[j] = __float_as_uint(s);
}

// One repair round.  s_end_prev is read, s_end_next written (ping-pong: a round must not see its own updates).
__global__ void __launch_bounds__(64)
k_agc_repair(int64_t num, int64_t C, int64_t W, float mu, float ref, const float* __restrict__ in, float* __restrict__ out,
             uint32_t* __restrict__ s_start, const uint32_t* __restrict__ s_end_prev, uint32_t* __restrict__ s_end_next,
             int nchunks, uint32_t* __restrict__ stats, int acc)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= nchunks) return;
    const int64_t begin = (int64_t)j * C;
    uint32_t e = s_end_prev[j];
    if (begin - W > 0) {
        const uint32_t s_true = s_end_prev[j - 1];
        if (s_start[j] != s_true) {
            const int64_t end = begin + C < num ? begin + C : num;
            e = __float_as_uint(agc_walk<true>(acc, in, out, begin, end, __uint_as_float(s_true), mu, ref));
            s_start[j] = s_true;
            atomicAdd(&stats[2], 1u);
        }
    }
    s_end_next[j] = e;
}

// One workgroup.  stats[0] = chunks still inconsistent after the parallel rounds, stats[1] = samples this lane rewrote
// (stats[2], counted by k_agc_repair = chunks recomputed in the parallel rounds), stats[3] = chunks of the launch.
__global__ void __launch_bounds__(1024)
k_agc_settle(int64_t num, int64_t C, int64_t W, float mu, float ref, const float* __restrict__ in, float* __restrict__ out,
             uint32_t* __restrict__ s_start, uint32_t* __restrict__ s_end, int nchunks, uint8_t* __restrict__ bad,
             float* __restrict__ fin, uint32_t* __restrict__ stats, int acc)
{
    __shared__ int nbad;
    if (threadIdx.x == 0) nbad = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < nchunks; j += blockDim.x) {
        const bool exact_start = (int64_t)j * C - W <= 0;
        const bool b = !exact_start && s_start[j] != s_end[j - 1];
        bad[j] = b;
        mine += b;
    }
    if (mine) atomicAdd(&nbad, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t rewritten = 0;
    if (nbad > 0) {
        int j = 1;
        while (j < nchunks) {
            // everything before chunk j is final here.  (A chunk flagged against an end state the walk has since replaced
            // may have become consistent: look again.)
            if (!bad[j] || s_start[j] == s_end[j - 1]) { j++; continue; }
            uint32_t s = s_end[j - 1];
            do {
                const int64_t begin = (int64_t)j * C;
                const int64_t end = begin + C < num ? begin + C : num;
                s_start[j] = s;
                s = __float_as_uint(agc_walk<true>(acc, in, out, begin, end, __uint_as_float(s), mu, ref));
                s_end[j] = s;
                rewritten += (uint32_t)(end - begin);
                j++;
            } while (j < nchunks && s_start[j] != s);   // an end state that changed invalidates the next chunk's start
        }
    }
    stats[0] = (uint32_t)nbad;
    stats[1] = rewritten;
    stats[3] = (uint32_t)nchunks;
    fin[0] = __uint_as_float(s_end[nchunks - 1]);
}

// plain sequential walk: short blocks (the run-in would cost more than the block), a null workspace, and num == 0
// (which only hands the state on)
__global__ void k_agc_sequential(int64_t num, float mu, float ref, float state, const float* d_state,
                                 const float* __restrict__ in, float* __restrict__ out, float* fin,
                                 uint32_t* __restrict__ stats, int acc)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    float s = d_state ? d_state[0] : state;
    s = agc_walk<true>(acc, in, out, 0, num, s, mu, ref);
    fin[0] = s;
    if (stats) { stats[0] = 0; stats[1] = 0; stats[2] = 0; stats[3] = 0; }
}

namespace {
constexpr int AGC_REPAIR_ROUNDS = 3;
constexpr int64_t kAgcMinChunk = 256;
// as kDcMaxLanes: every lane walks run-in + chunk at the latency of the dependent chain, so more lanes than the device
// holds at once only add redundant run-in traffic
constexpr int64_t kAgcMaxLanes = 32768;
constexpr int64_t kAgcMaxRunIn = (int64_t)1 << 22;

// Speculative starts merge with the true trajectory after 11-21 time constants of 1 / (mu * |x|) samples on ordinary
// signals (noise, FM, AM, tones at levels 0.3 - 0.8: 27 / mu .. 84 / mu samples, DESIGN.md "AGC").  128 / mu covers the
// worst of them 1.5 times; a weaker signal merges later and is left to the repair rounds.
int64_t agc_default_run_in(float mu)
{
    const float a = mu < 0.0f ? -mu : mu;
    if (!(a > 128.0f / (float)kAgcMaxRunIn)) return kAgcMaxRunIn;   // also mu = 0, NaN
    const int64_t w = (int64_t)(128.0f / a) + 1;
    return w < kAgcMinChunk ? kAgcMinChunk : w;
}
}  // namespace

AgcPlan agc_plan(int64_t num, float mu, int run_in)
{
    AgcPlan p;
    int64_t W = run_in > 0 ? (int64_t)run_in : agc_default_run_in(mu);
    W = (W + 7) & ~(int64_t)7;
    p.W = W;
    int64_t C = (num + kAgcMaxLanes - 1) / kAgcMaxLanes;
    if (C < kAgcMinChunk) C = kAgcMinChunk;
    if (C < W) C = W;
    C = (C + 7) & ~(int64_t)7;
    p.C = C;
    p.nchunks = num >= 2 * W ? (int)((num + C - 1) / C) : 0;
    return p;
}

size_t agc_workspace_bytes(int64_t num)
{
    // the most chunks any run-in gives: the shortest chunk
    if (num < 1) num = 1;
    int64_t C = (num + kAgcMaxLanes - 1) / kAgcMaxLanes;
    if (C < kAgcMinChunk) C = kAgcMinChunk;
    C = (C + 7) & ~(int64_t)7;
    const size_t nchunks = (size_t)((num + C - 1) / C);
    return nchunks * 13 + 64;   // stats, s_start, s_end x2 (u32 each), bad (u8)
}

void launch_agc(hipStream_t s, int64_t num, float mu, float reference, float state, const float* d_in, float* d_out,
                float* d_final, void* d_ws, int run_in, const float* d_state)
{
    if (num < 0) return;
    const uintptr_t both = (uintptr_t)d_in | (uintptr_t)d_out;
    const int acc = (both & 15) == 0 ? 2 : (both & 7) == 0 ? 1 : 0;
    uint32_t* stats = reinterpret_cast<uint32_t*>(d_ws);
    const AgcPlan p = agc_plan(num, mu, run_in);
    if (d_ws == nullptr || p.nchunks == 0) {
        hipLaunchKernelGGL(k_agc_sequential, dim3(1), dim3(64), 0, s, num, mu, reference, state, d_state, d_in, d_out, d_final,
                           stats, acc);
        return;
    }
    uint32_t* s_start = stats + 16;
    uint32_t* s_end[2] = {s_start + p.nchunks, s_start + 2 * (size_t)p.nchunks};
    uint8_t* bad = reinterpret_cast<uint8_t*>(s_start + 3 * (size_t)p.nchunks);
    const dim3 grid((p.nchunks + 63) / 64);
    (void)hipMemsetAsync(stats, 0, 16, s);
    hipLaunchKernelGGL(k_agc_speculate, grid, dim3(64), 0, s, num, p.C, p.W, mu, reference, state, d_state, d_in, d_out, s_start,
                       s_end[0], p.nchunks, acc);
    int cur = 0;
    for (int r = 0; r < AGC_REPAIR_ROUNDS; r++, cur ^= 1)
        hipLaunchKernelGGL(k_agc_repair, grid, dim3(64), 0, s, num, p.C, p.W, mu, reference, d_in, d_out, s_start, s_end[cur],
                           s_end[cur ^ 1], p.nchunks, stats, acc);
    hipLaunchKernelGGL(k_agc_settle, dim3(1), dim3(1024), 0, s, num, p.C, p.W, mu, reference, d_in, d_out, s_start, s_end[cur],
                       p.nchunks, bad, d_final, stats, acc);
}

// ---- rows: every row of a bank in one launch set ----------------------------------------------------------------------------
// Row r is in + r * in_stride -> out + r * out_stride (strides in floats, every offset 64-bit); its state is d_state[r], its
// final state fin[r], its statistics stats[4r .. 4r+3].  The walks are agc_walk as above, so a row's bits are those of the
// one-row kernels on that row alone.  acc is decided on the host from the base pointers AND the strides: one value for all rows.
//
// Sequential rows: one workgroup per row, one walking lane in it (k_agc_sequential with blockIdx.x = the row): every row's
// dependent chain runs at the rate of the one-row kernel, on a compute unit of its own, with the same load pattern.
__global__ void __launch_bounds__(64)
k_agc_rows_sequential(int64_t num, float mu, float ref, const float* d_state, const float* __restrict__ in, int64_t in_stride,
                      float* __restrict__ out, int64_t out_stride, float* fin, uint32_t* __restrict__ stats, int acc)
{
    if (threadIdx.x != 0) return;
    const int64_t row = blockIdx.x;
    float s = d_state[row];
    s = agc_walk<true>(acc, in + row * in_stride, out + row * out_stride, 0, num, s, mu, ref);
    fin[row] = s;
    if (stats) { uint32_t* st = stats + 4 * row; st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0; }
}

// lane = (row, chunk), rows packed densely into waves: lane g walks chunk g % nchunks of row g / nchunks.  The lane of chunk 0
// clears its row's statistics words (the repair rounds add to word 2 in later launches of the same stream).
__global__ void __launch_bounds__(64)
k_agc_rows_speculate(int64_t num, int64_t C, int64_t W, float mu, float ref, const float* __restrict__ d_state,
                     const float* __restrict__ in, int64_t in_stride, float* __restrict__ out, int64_t out_stride,
                     uint32_t* __restrict__ s_start, uint32_t* __restrict__ s_end, int nchunks, int lanes,
                     uint32_t* __restrict__ stats, int acc)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    const int64_t row = g / nchunks;
    const int j = g - (int)row * nchunks;
    in += row * in_stride;
    out += row * out_stride;
    if (j == 0) { uint32_t* st = stats + 4 * row; st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0; }
    const int64_t begin = (int64_t)j * C;
    const int64_t end = begin + C < num ? begin + C : num;
    int64_t i = begin - W;
    if (i < 0) i = 0;
    float s = d_state[row];
    s = agc_walk<false>(acc, in, out, i, begin, s, mu, ref);
    s_start[g] = __float_as_uint(s);
    s = agc_walk<true>(acc, in, out, begin, end, s, mu, ref);
    s_end[g] = __float_as_uint(s);
}

__global__ void __launch_bounds__(64)
k_agc_rows_repair(int64_t num, int64_t C, int64_t W, float mu, float ref, const float* __restrict__ in, int64_t in_stride,
                  float* __restrict__ out, int64_t out_stride, uint32_t* __restrict__ s_start,
                  const uint32_t* __restrict__ s_end_prev, uint32_t* __restrict__ s_end_next, int nchunks, int lanes,
                  uint32_t* __restrict__ stats, int acc)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    const int64_t row = g / nchunks;
    const int j = g - (int)row * nchunks;
    const int64_t begin = (int64_t)j * C;
    uint32_t e = s_end_prev[g];
    if (begin - W > 0) {
        const uint32_t s_true = s_end_prev[g - 1];   // j >= 1 here: the same row's chunk before
        if (s_start[g] != s_true) {
            const int64_t end = begin + C < num ? begin + C : num;
            e = __float_as_uint(agc_walk<true>(acc, in + row * in_stride, out + row * out_stride, begin, end,
                                               __uint_as_float(s_true), mu, ref));
            s_start[g] = s_true;
            atomicAdd(&stats[4 * row + 2], 1u);
        }
    }
    s_end_next[g] = e;
}

// One workgroup per row: k_agc_settle's check and whole-chunk walk on the row's own arrays, all rows at the same time.
__global__ void __launch_bounds__(256)
k_agc_rows_settle(int64_t num, int64_t C, int64_t W, float mu, float ref, const float* __restrict__ in, int64_t in_stride,
                  float* __restrict__ out, int64_t out_stride, uint32_t* __restrict__ s_start, uint32_t* __restrict__ s_end,
                  int nchunks, uint8_t* __restrict__ bad, float* fin, uint32_t* __restrict__ stats, int acc)
{
    const int64_t row = blockIdx.x;
    in += row * in_stride;
    out += row * out_stride;
    s_start += row * nchunks;
    s_end += row * nchunks;
    bad += row * nchunks;
    stats += 4 * row;
    __shared__ int nbad;
    if (threadIdx.x == 0) nbad = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < nchunks; j += blockDim.x) {
        const bool exact_start = (int64_t)j * C - W <= 0;
        const bool b = !exact_start && s_start[j] != s_end[j - 1];
        bad[j] = b;
        mine += b;
    }
    if (mine) atomicAdd(&nbad, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t rewritten = 0;
    if (nbad > 0) {
        int j = 1;
        while (j < nchunks) {
            if (!bad[j] || s_start[j] == s_end[j - 1]) { j++; continue; }
            uint32_t s = s_end[j - 1];
            do {
                const int64_t begin = (int64_t)j * C;
                const int64_t end = begin + C < num ? begin + C : num;
                s_start[j] = s;
                s = __float_as_uint(agc_walk<true>(acc, in, out, begin, end, __uint_as_float(s), mu, ref));
                s_end[j] = s;
                rewritten += (uint32_t)(end - begin);
                j++;
            } while (j < nchunks && s_start[j] != s);
        }
    }
    stats[0] = (uint32_t)nbad;
    stats[1] = rewritten;
    stats[3] = (uint32_t)nchunks;
    fin[row] = __uint_as_float(s_end[nchunks - 1]);
}

namespace {
std::atomic<long long> g_rows_launches{0};
}  // namespace

// the shortest chunk a row may have when `rows` rows share a lane cap: a multiple of 8 samples
int64_t rows_min_chunk(int rows, int64_t num, int64_t cap)
{
    int64_t per_row = cap / (rows > 0 ? rows : 1);
    if (per_row < 1) per_row = 1;
    const int64_t C = (num + per_row - 1) / per_row;
    return (C + 7) & ~(int64_t)7;
}

void rows_launches_add(int launches) { g_rows_launches.fetch_add(launches); }
long long rows_launch_count() { return g_rows_launches.load(); }

AgcPlan agc_rows_plan(int rows, int64_t num, float mu, int run_in)
{
    AgcPlan p = agc_plan(num, mu, run_in);
    if ((int64_t)rows * p.nchunks > kAgcMaxLanes) {
        const int64_t C = rows_min_chunk(rows, num, kAgcMaxLanes);
        if (C > p.C) p.C = C;
        p.nchunks = (int)((num + p.C - 1) / p.C);
    }
    return p;
}

size_t agc_rows_workspace_bytes(int rows, int64_t num)
{
    if (num < 1) num = 1;
    int64_t C = (num + kAgcMaxLanes - 1) / kAgcMaxLanes;   // as agc_workspace_bytes: the shortest chunk any run-in gives
    if (C < kAgcMinChunk) C = kAgcMinChunk;
    C = (C + 7) & ~(int64_t)7;
    const int64_t Cr = rows_min_chunk(rows, num, kAgcMaxLanes);
    if ((int64_t)rows * ((num + C - 1) / C) > kAgcMaxLanes && Cr > C) C = Cr;
    const size_t nchunks = (size_t)((num + C - 1) / C);
    return (size_t)rows * 16 + (size_t)rows * nchunks * 13 + 64;   // per row: stats; s_start, s_end x2 (u32 each), bad (u8)
}

void launch_agc_rows(hipStream_t s, int rows, int64_t num, float mu, float reference, const float* d_in, int64_t in_stride,
                     float* d_out, int64_t out_stride, const float* d_state, float* d_final, void* d_ws, int run_in)
{
    if (num < 0 || rows < 1) return;
    uintptr_t both = (uintptr_t)d_in | (uintptr_t)d_out;
    if (rows > 1) both |= (uintptr_t)(in_stride * 4) | (uintptr_t)(out_stride * 4);   // row r starts at base + r * stride
    const int acc = (both & 15) == 0 ? 2 : (both & 7) == 0 ? 1 : 0;
    uint32_t* stats = reinterpret_cast<uint32_t*>(d_ws);
    const AgcPlan p = agc_rows_plan(rows, num, mu, run_in);
    if (d_ws == nullptr || p.nchunks == 0) {
        hipLaunchKernelGGL(k_agc_rows_sequential, dim3(rows), dim3(64), 0, s, num, mu, reference, d_state, d_in, in_stride, d_out,
                           out_stride, d_final, stats, acc);
        rows_launches_add(1);
        return;
    }
    const int lanes = rows * p.nchunks;
    uint32_t* s_start = stats + 4 * (size_t)rows;
    uint32_t* s_end[2] = {s_start + lanes, s_start + 2 * (size_t)lanes};
    uint8_t* bad = reinterpret_cast<uint8_t*>(s_start + 3 * (size_t)lanes);
    const dim3 grid((lanes + 63) / 64);
    hipLaunchKernelGGL(k_agc_rows_speculate, grid, dim3(64), 0, s, num, p.C, p.W, mu, reference, d_state, d_in, in_stride, d_out,
                       out_stride, s_start, s_end[0], p.nchunks, lanes, stats, acc);
    int cur = 0;
    for (int r = 0; r < AGC_REPAIR_ROUNDS; r++, cur ^= 1)
        hipLaunchKernelGGL(k_agc_rows_repair, grid, dim3(64), 0, s, num, p.C, p.W, mu, reference, d_in, in_stride, d_out, out_stride,
                           s_start, s_end[cur], s_end[cur ^ 1], p.nchunks, lanes, stats, acc);
    hipLaunchKernelGGL(k_agc_rows_settle, dim3(rows), dim3(256), 0, s, num, p.C, p.W, mu, reference, d_in, in_stride, d_out,
                       out_stride, s_start, s_end[cur], p.nchunks, bad, d_final, stats, acc);
    rows_launches_add(2 + AGC_REPAIR_ROUNDS);
}

}  // namespace sdrhip
