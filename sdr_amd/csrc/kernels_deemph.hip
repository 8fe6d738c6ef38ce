// kernels_deemph.hip -- de-emphasis: the one-pole low-pass behind an FM receiver's audio (75 us / 50 us), this project's definition,
// written as the reference writes agc (Util.hs:335-341): a mapAccum at Float.
//
//     y[i] = y[i-1] + alpha * (x[i] - y[i-1])        y[-1] = state
//
// Three f32 operations per sample, each rounded to nearest, in this order: subtract, multiply, add (the library is built with
// -ffp-contract=off).  deemph_step is the only statement of the arithmetic.
//
// The rounded recurrence is no associative scan, but it is a contraction by 1 - alpha (the argument of kernels_iir.hip:5-18): a lane
// that starts W samples early from state 0 forgets its error, and two trajectories that are equal as bits stay equal.  A de-emphasis pole
// is weak (alpha 0.24 at 48 kHz / 75 us against the dcBlocker's 0.003), so the run-in is a few hundred samples and a live block of 1024
// samples can be cut into 64 chunks that ONE workgroup speculates on and verifies in ONE launch with no workspace:
//   SEQ  one workgroup per row, its first lane walks the row.  Blocks shorter than two run-ins; rows past the WG bound with no workspace.
//   WG   one workgroup per row, lane j owns chunk j: run in, write the chunk, leave the end state in LDS; then rounds in which every chunk
//        whose recorded start state differs from its predecessor's end state of the round before is recomputed from that state, until a
//        round finds no difference.  n <= 65536 (auto: n < 32768 when a workspace is given).
//   LS   the dcBlocker rows launch set (speculate, three repair rounds, settle; lane = (row, chunk), at most 32768 lanes) for rows of
//        32768 samples and more when a workspace is given.
// The result is the sequential result by construction on every route; only the time depends on the convergence.  Trajectories do NOT
// meet on an exactly constant input (they stall a few ULP apart), so such rows are repaired chunk by chunk, up to a sequential walk.
//
// Samples are read straight from global memory on every route (as k_dc_speculate does): a row at the WG bound is 256 KiB, more than the
// 160 KiB of LDS, so a kernel that serves the whole range cannot stage its row.  Loads do not depend on the chain: every walk requests
// its next 16 samples before it consumes the current 16.  Access width (16 / 8 / 4 bytes) is chosen on the host from the base pointers
// and, with more than one row, the strides -- that is, from every row's own pointer.
#include <atomic>

#include "deemph.hpp"
#include "kernels.hpp"

namespace sdrhip {

__device__ __forceinline__ float deemph_step(float x, float y, float alpha)
{
    const float d = x - y;
    const float m = alpha * d;
    return y + m;
}

namespace {
constexpr int DE_G = 16;   // samples per group: one group of loads is in flight while the previous one is walked

// DE_G floats at p by accesses of V floats; p is V * 4 bytes aligned
template <int V>
__device__ __forceinline__ void de_load(const float* __restrict__ p, float (&x)[DE_G])
{
    if constexpr (V == 4) {
#pragma unroll
        for (int k = 0; k < DE_G; k += 4) {
            const float4 v = *reinterpret_cast<const float4*>(p + k);
            x[k] = v.x; x[k + 1] = v.y; x[k + 2] = v.z; x[k + 3] = v.w;
        }
    } else if constexpr (V == 2) {
#pragma unroll
        for (int k = 0; k < DE_G; k += 2) {
            const float2 v = *reinterpret_cast<const float2*>(p + k);
            x[k] = v.x; x[k + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < DE_G; k++) x[k] = p[k];
    }
}

template <int V>
__device__ __forceinline__ void de_store(float* __restrict__ p, const float (&o)[DE_G])
{
    if constexpr (V == 4) {
#pragma unroll
        for (int k = 0; k < DE_G; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(o[k], o[k + 1], o[k + 2], o[k + 3]);
    } else if constexpr (V == 2) {
#pragma unroll
        for (int k = 0; k < DE_G; k += 2) *reinterpret_cast<float2*>(p + k) = make_float2(o[k], o[k + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < DE_G; k++) p[k] = o[k];
    }
}

// Samples [i, end) of a row from state y; STORE: out[i .. end) is written.  i is a multiple of 4 samples from the row's first (so the
// groups keep the row's alignment).  Whole groups first, the next group's loads ahead of the chain; then the < DE_G samples left, their
// loads issued together.  Returns the state after sample end - 1.
template <int V, bool STORE>
__device__ __forceinline__ float de_walk(const float* __restrict__ in, float* __restrict__ out, int64_t i, int64_t end, float y, float alpha)
{
    if (end - i >= DE_G) {
        float x[DE_G];
        de_load<V>(in + i, x);
        for (;;) {
            const bool more = end - (i + DE_G) >= DE_G;
            float xn[DE_G];
            de_load<V>(in + (more ? i + DE_G : i), xn);
            float o[DE_G];
#pragma unroll
            for (int k = 0; k < DE_G; k++) o[k] = y = deemph_step(x[k], y, alpha);
            if (STORE) de_store<V>(out + i, o);
            i += DE_G;
            if (!more) break;
#pragma unroll
            for (int k = 0; k < DE_G; k++) x[k] = xn[k];
        }
    }
    const int rem = (int)(end - i);
    if (rem > 0) {
        float x[DE_G];
#pragma unroll
        for (int k = 0; k < DE_G; k++) x[k] = k < rem ? in[i + k] : 0.0f;
#pragma unroll
        for (int k = 0; k < DE_G; k++)
            if (k < rem) {
                y = deemph_step(x[k], y, alpha);
                if (STORE) out[i + k] = y;
            }
    }
    return y;
}
}  // namespace

// ---- SEQ: one workgroup per row, one walking lane in it ---------------------------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(64)
k_deemph_seq(int64_t n, float alpha, float state, const float* d_state, const float* __restrict__ in, int64_t in_stride,
             float* __restrict__ out, int64_t out_stride, float* fin, uint32_t* __restrict__ stats)
{
    if (threadIdx.x != 0) return;
    const int64_t row = blockIdx.x;
    const float y = de_walk<V, true>(in + row * in_stride, out + row * out_stride, 0, n, d_state ? d_state[row] : state, alpha);
    fin[row] = y;
    if (stats) { uint32_t* st = stats + 4 * row; st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0; }
}

// ---- WG: one launch, one workgroup per row, no workspace --------------------------------------------------------------------------
// Lane j owns chunk j = samples [j * C, j * C + C) of the row; blockDim.x >= nchunks, a multiple of 64, at most 1024.
// stats (may be null): {rounds that recomputed a chunk, 0, chunks whose start state was replaced (summed over the rounds), chunks}.
template <int V>
__global__ void __launch_bounds__(1024)
k_deemph_wg(int64_t n, int C, int64_t W, int nchunks, float alpha, float state, const float* d_state, const float* __restrict__ in,
            int64_t in_stride, float* __restrict__ out, int64_t out_stride, float* fin, uint32_t* __restrict__ stats)
{
    __shared__ uint32_t s_end[2][kDeemphWgChunks];   // the chunks' end states: a round reads one array and writes the other
    __shared__ uint32_t s_replaced;
    const int64_t row = blockIdx.x;
    const int j = threadIdx.x;
    const bool live = j < nchunks;
    in += row * in_stride;
    out += row * out_stride;
    const float y0 = d_state ? d_state[row] : state;   // read before the first barrier: fin may be d_state
    const int64_t begin = (int64_t)j * C;
    const int64_t end = begin + C < n ? begin + C : n;
    uint32_t y_start = 0;
    bool exact = true;                                 // the run-in reached sample 0: the start state is the true one
    if (j == 0) s_replaced = 0;
    if (live) {
        int64_t i = begin - W;
        float y = 0.0f;
        exact = i <= 0;
        if (exact) { i = 0; y = y0; }
        y = de_walk<V, false>(in, nullptr, i, begin, y, alpha);
        y_start = __float_as_uint(y);
        y = de_walk<V, true>(in, out, begin, end, y, alpha);
        s_end[0][j] = __float_as_uint(y);
    }
    __syncthreads();
    int cur = 0;
    uint32_t rounds = 0;
    // After round r the first r chunks that did not start exact have started from their true state, so nchunks rounds make every chunk
    // final whatever the input: the bound is explicit, every lane takes every barrier, and the exit condition is workgroup-uniform.
    for (int r = 0; r < nchunks; r++) {
        int redo = 0;
        if (live) {
            uint32_t e = s_end[cur][j];
            if (!exact) {
                const uint32_t s_true = s_end[cur][j - 1];   // !exact: j >= 1
                if (s_true != y_start) {
                    e = __float_as_uint(de_walk<V, true>(in, out, begin, end, __uint_as_float(s_true), alpha));
                    y_start = s_true;
                    redo = 1;
                    atomicAdd(&s_replaced, 1u);
                }
            }
            s_end[cur ^ 1][j] = e;
        }
        const int any = __syncthreads_or(redo);   // the barrier between this round's reads and the next round's writes
        cur ^= 1;
        if (!any) break;
        rounds++;
    }
    if (j == 0) {
        fin[row] = __uint_as_float(s_end[cur][nchunks - 1]);
        if (stats) { uint32_t* st = stats + 4 * row; st[0] = rounds; st[1] = 0; st[2] = s_replaced; st[3] = (uint32_t)nchunks; }
    }
}

// ---- LS: the dcBlocker rows launch set (kernels_iir.hip "rows") on deemph_step ------------------------------------------------------
// lane = (row, chunk), packed densely: lane g walks chunk g % nchunks of row g / nchunks; chunk 0's lane clears the row's statistics
template <int V>
__global__ void __launch_bounds__(64)
k_deemph_ls_speculate(int64_t n, int64_t C, int64_t W, float alpha, float state, const float* __restrict__ d_state,
                      const float* __restrict__ in, int64_t in_stride, float* __restrict__ out, int64_t out_stride,
                      uint32_t* __restrict__ y_start, uint32_t* __restrict__ y_end, int nchunks, int lanes, uint32_t* __restrict__ stats)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    const int64_t row = g / nchunks;
    const int j = g - (int)row * nchunks;
    in += row * in_stride;
    out += row * out_stride;
    if (j == 0) { uint32_t* st = stats + 4 * row; st[0] = 0; st[1] = 0; st[2] = 0; st[3] = 0; }
    const int64_t begin = (int64_t)j * C;
    const int64_t end = begin + C < n ? begin + C : n;
    int64_t i = begin - W;
    float y = 0.0f;
    if (i <= 0) { i = 0; y = d_state ? d_state[row] : state; }
    y = de_walk<V, false>(in, nullptr, i, begin, y, alpha);
    y_start[g] = __float_as_uint(y);
    y = de_walk<V, true>(in, out, begin, end, y, alpha);
    y_end[g] = __float_as_uint(y);
}

// One repair round.  y_end_prev is read, y_end_next written (ping-pong: a round must not see its own updates).
template <int V>
__global__ void __launch_bounds__(64)
k_deemph_ls_repair(int64_t n, int64_t C, int64_t W, float alpha, const float* __restrict__ in, int64_t in_stride, float* __restrict__ out,
                   int64_t out_stride, uint32_t* __restrict__ y_start, const uint32_t* __restrict__ y_end_prev,
                   uint32_t* __restrict__ y_end_next, int nchunks, int lanes, uint32_t* __restrict__ stats)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= lanes) return;
    const int64_t row = g / nchunks;
    const int j = g - (int)row * nchunks;
    const int64_t begin = (int64_t)j * C;
    uint32_t e = y_end_prev[g];
    if (begin - W > 0) {
        const uint32_t s_true = y_end_prev[g - 1];   // j >= 1 here: the same row's chunk before
        if (y_start[g] != s_true) {
            const int64_t end = begin + C < n ? begin + C : n;
            e = __float_as_uint(de_walk<V, true>(in + row * in_stride, out + row * out_stride, begin, end, __uint_as_float(s_true), alpha));
            y_start[g] = s_true;
            atomicAdd(&stats[4 * row + 2], 1u);
        }
    }
    y_end_next[g] = e;
}

// One workgroup per row.  stats: {chunks still inconsistent after the parallel rounds, samples this lane rewrote, (word 2, counted by
// the repair rounds: chunks recomputed there), chunks of the row}
__global__ void __launch_bounds__(256)
k_deemph_ls_settle(int64_t n, int64_t C, int64_t W, float alpha, const float* __restrict__ in, int64_t in_stride, float* __restrict__ out,
                   int64_t out_stride, const uint32_t* __restrict__ y_start, const uint32_t* __restrict__ y_end, int nchunks,
                   uint8_t* __restrict__ bad, float* fin, uint32_t* __restrict__ stats)
{
    const int64_t row = blockIdx.x;
    in += row * in_stride;
    out += row * out_stride;
    y_start += row * nchunks;
    y_end += row * nchunks;
    bad += row * nchunks;
    stats += 4 * row;
    __shared__ int nbad;
    if (threadIdx.x == 0) nbad = 0;
    __syncthreads();
    int mine = 0;
    for (int j = threadIdx.x; j < nchunks; j += blockDim.x) {
        const bool exact_start = (int64_t)j * C - W <= 0;
        const bool b = !exact_start && y_start[j] != y_end[j - 1];
        bad[j] = b;
        mine += b;
    }
    if (mine) atomicAdd(&nbad, mine);
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t rewritten = 0;
    if (nbad > 0) {
        int64_t reach = -1;   // everything up to here is final
        for (int j = 1; j < nchunks; j++) {
            if (!bad[j]) continue;
            int64_t i = (int64_t)j * C;
            if (i <= reach) continue;
            float y = out[i - 1];
            for (; i < n; i++) {
                y = deemph_step(in[i], y, alpha);
                if (__float_as_uint(y) == __float_as_uint(out[i])) break;   // met the stored trajectory: the rest is right
                out[i] = y;
                rewritten++;
            }
            reach = i;
        }
    }
    stats[0] = (uint32_t)nbad;
    stats[1] = rewritten;
    stats[3] = (uint32_t)nchunks;
    fin[row] = out[n - 1];
}

// ---- host: the plan and the launcher ----------------------------------------------------------------------------------------------
namespace {
constexpr int DE_REPAIR_ROUNDS = 3;
constexpr int64_t kDeemphMaxLanes = 32768;   // LS: as kDcMaxLanes (kernels_iir.hip)
std::atomic<long long> g_deemph_launches{0};
std::atomic<int> g_deemph_route{DEEMPH_AUTO};

int64_t ls_chunk(int rows, int64_t n)
{
    int64_t C = (n + kDeemphMaxLanes - 1) / kDeemphMaxLanes;
    if (C < 256) C = 256;
    C = (C + 3) & ~(int64_t)3;
    if ((int64_t)rows * ((n + C - 1) / C) > kDeemphMaxLanes) {
        const int64_t Cr = rows_min_chunk(rows, n, kDeemphMaxLanes);
        if (Cr > C) C = Cr;
    }
    return C;
}

int64_t wg_chunk(int64_t n)
{
    int64_t C = (n + kDeemphWgChunks - 1) / kDeemphWgChunks;
    if (C < 16) C = 16;
    return (C + 3) & ~(int64_t)3;
}
}  // namespace

int64_t deemph_default_run_in(float alpha)
{
    const double w = ceil(40.0 / (double)alpha);
    const int64_t W = w < 0x1p60 ? (int64_t)w : (int64_t)1 << 60;
    return (W + 3) & ~(int64_t)3;
}

// Auto rule: below two run-ins SEQ (the run-in would cost more than the block); up to the WG bound WG, except that with a workspace LS
// takes over from 32768 samples on, where the sweep found it ahead; past the bound LS with a workspace, SEQ without one.  The run-in is kept in 64 bits and the route is decided on it before anything is narrowed.
bool deemph_plan(int rows, int64_t n, float alpha, int run_in, bool has_workspace, int forced, DeemphPlan* plan)
{
    DeemphPlan p;
    p.W = run_in > 0 ? ((int64_t)run_in + 3) & ~(int64_t)3 : deemph_default_run_in(alpha);
    const bool two = n >= 2 * p.W;
    int route = forced;
    if (route == DEEMPH_AUTO) route = !two ? DEEMPH_SEQ : n <= kDeemphWgMax && !(has_workspace && n >= kDeemphWgAuto) ? DEEMPH_WG : has_workspace ? DEEMPH_LS : DEEMPH_SEQ;
    if (route == DEEMPH_WG && !(two && n <= kDeemphWgMax)) return false;
    if (route == DEEMPH_LS && !(two && has_workspace)) return false;
    p.route = route;
    p.C = route == DEEMPH_WG ? wg_chunk(n) : ls_chunk(rows, n > 0 ? n : 1);
    p.nchunks = route == DEEMPH_SEQ ? 0 : (int)((n + p.C - 1) / p.C);
    *plan = p;
    return true;
}

size_t deemph_rows_workspace_bytes(int rows, int64_t n)
{
    if (n < 1) n = 1;
    const int64_t C = ls_chunk(rows, n);
    const size_t nchunks = (size_t)((n + C - 1) / C);
    return (size_t)rows * 16 + (size_t)rows * nchunks * 13 + 64;   // per row: stats; y_start, y_end x2 (u32 each), bad (u8)
}

long long deemph_launch_count() { return g_deemph_launches.load(); }
void deemph_set_route(int route) { g_deemph_route.store(route); }
int deemph_forced_route() { return g_deemph_route.load(); }

#define DEEMPH_BY_ACCESS(KERNEL, grid, block, ...)                                                     \
    do {                                                                                               \
        if (acc == 4) hipLaunchKernelGGL(KERNEL<4>, grid, block, 0, s, __VA_ARGS__);                   \
        else if (acc == 2) hipLaunchKernelGGL(KERNEL<2>, grid, block, 0, s, __VA_ARGS__);              \
        else hipLaunchKernelGGL(KERNEL<1>, grid, block, 0, s, __VA_ARGS__);                            \
    } while (0)

void launch_deemph_rows(hipStream_t s, const DeemphPlan& p, int rows, int64_t n, float alpha, float state, const float* d_state,
                        const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, float* d_final, void* d_ws)
{
    if (n < 0 || rows < 1) return;
    uintptr_t both = (uintptr_t)d_in | (uintptr_t)d_out;
    if (rows > 1) both |= (uintptr_t)(in_stride * 4) | (uintptr_t)(out_stride * 4);   // row r starts at base + r * stride
    const int acc = (both & 15) == 0 ? 4 : (both & 7) == 0 ? 2 : 1;
    uint32_t* stats = reinterpret_cast<uint32_t*>(d_ws);
    if (p.route == DEEMPH_SEQ || n == 0) {
        DEEMPH_BY_ACCESS(k_deemph_seq, dim3(rows), dim3(64), n, alpha, state, d_state, d_in, in_stride, d_out, out_stride, d_final, stats);
        g_deemph_launches.fetch_add(1);
        return;
    }
    if (p.route == DEEMPH_WG) {
        DEEMPH_BY_ACCESS(k_deemph_wg, dim3(rows), dim3((p.nchunks + 63) / 64 * 64), n, (int)p.C, p.W, p.nchunks, alpha, state, d_state, d_in,
                         in_stride, d_out, out_stride, d_final, stats);
        g_deemph_launches.fetch_add(1);
        return;
    }
    const int lanes = rows * p.nchunks;
    uint32_t* y_start = stats + 4 * (size_t)rows;
    uint32_t* y_end[2] = {y_start + lanes, y_start + 2 * (size_t)lanes};
    uint8_t* bad = reinterpret_cast<uint8_t*>(y_start + 3 * (size_t)lanes);
    const dim3 grid((lanes + 63) / 64);
    DEEMPH_BY_ACCESS(k_deemph_ls_speculate, grid, dim3(64), n, p.C, p.W, alpha, state, d_state, d_in, in_stride, d_out, out_stride, y_start,
                     y_end[0], p.nchunks, lanes, stats);
    int cur = 0;
    for (int r = 0; r < DE_REPAIR_ROUNDS; r++, cur ^= 1)
        DEEMPH_BY_ACCESS(k_deemph_ls_repair, grid, dim3(64), n, p.C, p.W, alpha, d_in, in_stride, d_out, out_stride, y_start, y_end[cur],
                         y_end[cur ^ 1], p.nchunks, lanes, stats);
    hipLaunchKernelGGL(k_deemph_ls_settle, dim3(rows), dim3(256), 0, s, n, p.C, p.W, alpha, d_in, in_stride, d_out, out_stride, y_start,
                       y_end[cur], p.nchunks, bad, d_final, stats);
    g_deemph_launches.fetch_add(kDeemphLsLaunches);
    static_assert(kDeemphLsLaunches == 2 + DE_REPAIR_ROUNDS, "the launch set is speculate, the repair rounds and settle");
}

}  // namespace sdrhip
