// kernels_squelch.hip -- the squelch: a gate decision per block from the block's mean power, this project's definition (the reference
// has none; tests/squelch_model.py is its model, include/sdr_hip.h "squelch" its statement).
//
//   level   256 slots; slot[j] = the sum of the block's powers p_i with i mod 256 == j in ascending i; fold slot[j] += slot[j + w] for
//           w = 128 .. 1; level = slot[0] * (float)(1.0 / block_det).  p = x * x, or re * re + im * im with each product rounded
//           (the library is built with -ffp-contract=off).  sq_block_level is the only statement of that order.
//   gate    det follows the last decisive block (level past the open level: 1, past the close level: 0); the gate is open while
//           det is 1 and for `hang` blocks behind it.  Sequential as defined, two max-scans as computed (sq_gate_group).
//   apply   the block's signal floats are copied as bits where the gate is open, +0 where it is shut.
//
// The level order is laid out for ONE WAVE per block: lane l holds slots 4l .. 4l + 3, which are 16 consecutive bytes of a real
// detector row (32 of a complex one) in every stretch of 256 samples, so a stretch is one 16-byte load per lane (two when complex);
// the fold's steps w = 128 .. 4 are lane l += lane l + w / 4, the steps 2 and 1 stay inside lane 0.  No LDS, no barrier, and the
// same function serves both routes:
//   WG   one launch, one workgroup of 16 waves per row: the waves share out the row's blocks; levels to LDS; the gate of up to 1024
//        blocks by two max-scans across the workgroup; the gated copy; the state.  A row of more than 1024 blocks is walked in groups
//        of 1024, the state passing from group to group as it passes from call to call.
//   LS   levels (grid over blocks x rows), gate (one workgroup per row, the same scans), apply (grid over signal tiles x rows).
// Loads and stores are 16 / 8 / 4 bytes wide as the host finds the detector, the signal and the output aligned, each on its own; the
// width is a kernel argument, uniform over the grid.
#include <atomic>

#include "kernels.hpp"
#include "squelch.hpp"

namespace sdrhip {

namespace {
constexpr int SQ_T = 1024;            // threads of the WG and gate kernels: thread t owns block t of a group
constexpr int SQ_WAVES = SQ_T / 64;
constexpr int SQ_TILE = 8192;         // signal floats per workgroup of the apply kernel
static_assert(SQ_T == kSquelchGroup, "one thread per block of a group");

struct SqGate { float open, close; int hang, above; };

struct SqRows {
    const float* det; int64_t det_stride; int block_det, wd; float inv;
    const uint32_t* in; int64_t in_stride; uint32_t* out; int64_t out_stride; int block_sig, wi, wo;
    int64_t n_blocks;
    SqGate g;
    int det0, hang0; const int32_t* state; int32_t* fin;
    float* levels; uint8_t* gates;
};

// four floats at p by accesses of w floats; p is w * 4 bytes aligned
__device__ __forceinline__ float4 sq_ld4(const float* p, int w)
{
    if (w == 4) return *reinterpret_cast<const float4*>(p);
    if (w == 2) {
        const float2 a = *reinterpret_cast<const float2*>(p), b = *reinterpret_cast<const float2*>(p + 2);
        return make_float4(a.x, a.y, b.x, b.y);
    }
    return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ uint4 sq_ld4u(const uint32_t* p, int w)
{
    if (w == 4) return *reinterpret_cast<const uint4*>(p);
    if (w == 2) {
        const uint2 a = *reinterpret_cast<const uint2*>(p), b = *reinterpret_cast<const uint2*>(p + 2);
        return make_uint4(a.x, a.y, b.x, b.y);
    }
    return make_uint4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ void sq_st4u(uint32_t* p, uint4 v, int w)
{
    if (w == 4) *reinterpret_cast<uint4*>(p) = v;
    else if (w == 2) { *reinterpret_cast<uint2*>(p) = make_uint2(v.x, v.y); *reinterpret_cast<uint2*>(p + 2) = make_uint2(v.z, v.w); }
    else { p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w; }
}

__device__ __forceinline__ float sq_power(float re, float im)
{
    const float a = re * re;
    const float b = im * im;
    return a + b;
}

// The level of the block of m detector samples at blk, computed by one whole wave; the value is lane 0's.  blk is w * 4 bytes aligned.
template <bool CPLX>
__device__ __forceinline__ float sq_block_level(const float* __restrict__ blk, int m, int w, float inv, int lane)
{
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f;
    const int full = m & ~255;
    int i = 4 * lane;
#pragma unroll 4
    for (; i < full; i += 256) {
        if (CPLX) {
            const float4 a = sq_ld4(blk + 2 * (int64_t)i, w), b = sq_ld4(blk + 2 * (int64_t)i + 4, w);
            s0 = s0 + sq_power(a.x, a.y); s1 = s1 + sq_power(a.z, a.w); s2 = s2 + sq_power(b.x, b.y); s3 = s3 + sq_power(b.z, b.w);
        } else {
            const float4 a = sq_ld4(blk + i, w);
            s0 = s0 + a.x * a.x; s1 = s1 + a.y * a.y; s2 = s2 + a.z * a.z; s3 = s3 + a.w * a.w;
        }
    }
    // the stretch that is not whole: sample by sample, an absent sample adds nothing (an empty slot is +0)
    float p[4];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        p[t] = 0.0f;
        if (i + t < m) p[t] = CPLX ? sq_power(blk[2 * (int64_t)(i + t)], blk[2 * (int64_t)(i + t) + 1]) : blk[i + t] * blk[i + t];
    }
    s0 = s0 + p[0]; s1 = s1 + p[1]; s2 = s2 + p[2]; s3 = s3 + p[3];
    // fold: w = 128 .. 4 is lane l += lane l + w / 4 on each of the four slots (the lanes at and above w / 4 hold values nobody reads)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        s0 = s0 + __shfl_down(s0, off); s1 = s1 + __shfl_down(s1, off); s2 = s2 + __shfl_down(s2, off); s3 = s3 + __shfl_down(s3, off);
    }
    s0 = s0 + s2;     // w = 2
    s1 = s1 + s3;
    s0 = s0 + s1;     // w = 1
    return s0 * inv;
}

// inclusive max-scan over the SQ_T threads of the workgroup; every thread calls it; s_w: SQ_WAVES ints of LDS
__device__ __forceinline__ int sq_max_scan(int v, int* s_w, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int u = __shfl_up(v, off);
        if (lane >= off) v = max(v, u);
    }
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    int pre = -1;
    for (int k = 0; k < wave; k++) pre = max(pre, s_w[k]);
    __syncthreads();
    return max(v, pre);
}

// The gate of one group of nb <= SQ_T blocks: thread tid holds block tid's level (tid < nb) and gets its gate.  s_state is the
// {det, hang_left} carried in (already clamped) and, behind the barrier that ends the function, the one carried out.  Every thread of
// the workgroup calls it.  det_b = the value of the last decisive block <= b, or the one carried in; last_open_b = the last block
// <= b with det 1; the gate is open within `hang` blocks of last_open_b, or, where there is none yet, while the carried-in hang lasts.
__device__ __forceinline__ int sq_gate_group(float level, int nb, const SqGate& g, int* s_w, int* s_state, int tid)
{
    const int det_in = s_state[0], left_in = s_state[1];
    const bool live = tid < nb;
    int key = -1;
    if (live) {
        const bool want_open = g.above ? level >= g.open : level <= g.open;
        const bool want_close = g.above ? level < g.close : level > g.close;
        if (want_open) key = 2 * tid + 1;
        else if (want_close) key = 2 * tid;
    }
    const int last = sq_max_scan(key, s_w, tid);
    const int det = last < 0 ? det_in : (last & 1);
    const int lo = sq_max_scan(live && det ? tid : -1, s_w, tid);
    const int gate = lo >= 0 ? (tid - lo <= g.hang) : (tid < left_in);
    if (tid == nb - 1) {
        s_state[0] = det;
        s_state[1] = det ? g.hang : lo >= 0 ? max(0, g.hang - (nb - 1 - lo)) : max(0, left_in - nb);
    }
    __syncthreads();
    return gate;
}

// `count` signal floats at in -> out: float k belongs to block (rem0 + k) / bs counted from the block gates[0] speaks of.  in and out
// are 16 bytes aligned as far as wi / wo say; in may be out.  Threads tid of nthr share the span out four floats at a time.
__device__ __forceinline__ void sq_apply_span(const uint32_t* in, uint32_t* out, const uint8_t* gates, uint32_t rem0, uint32_t count,
                                              uint32_t bs, int wi, int wo, int tid, int nthr)
{
    const bool inplace = in == out;
    for (uint32_t o = 4u * tid; o < count; o += 4u * nthr) {
        const uint32_t pos = rem0 + o;
        const uint32_t q = pos / bs, r = pos - q * bs;
        if (o + 4 <= count) {
            uint32_t gt[4];
#pragma unroll
            for (uint32_t t = 0; t < 4; t++) gt[t] = gates[bs >= 4 ? q + (r + t >= bs ? 1u : 0u) : (pos + t) / bs];
            const uint32_t all = gt[0] & gt[1] & gt[2] & gt[3], any = gt[0] | gt[1] | gt[2] | gt[3];
            if (inplace && all) continue;
            uint4 x = make_uint4(0, 0, 0, 0);
            if (any) x = sq_ld4u(in + o, wi);
            x.x = gt[0] ? x.x : 0u; x.y = gt[1] ? x.y : 0u; x.z = gt[2] ? x.z : 0u; x.w = gt[3] ? x.w : 0u;
            sq_st4u(out + o, x, wo);
        } else {
            for (uint32_t t = 0; o + t < count; t++) {
                const uint32_t gate = gates[(pos + t) / bs];
                if (inplace && gate) continue;
                out[o + t] = gate ? in[o + t] : 0u;
            }
        }
    }
}

__device__ __forceinline__ void sq_read_state(const SqRows& p, int64_t row, int* s_state)
{
    const int det = p.state ? p.state[2 * row] : p.det0;
    const int left = p.state ? p.state[2 * row + 1] : p.hang0;
    s_state[0] = det != 0;
    s_state[1] = min(max(left, 0), p.g.hang);
}
}  // namespace

// ---- WG: one launch, one workgroup per row, no workspace --------------------------------------------------------------------------
template <bool CPLX>
__global__ void __launch_bounds__(SQ_T)
k_squelch_wg(SqRows p)
{
    __shared__ float s_level[SQ_T];
    __shared__ uint8_t s_gate[SQ_T];
    __shared__ int s_w[SQ_WAVES];
    __shared__ int s_state[2];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) sq_read_state(p, row, s_state);      // the row's state is read before it is written: fin may be state
    __syncthreads();
    const float* det = p.det + row * p.det_stride;
    const int64_t blk_floats = (int64_t)p.block_det * (CPLX ? 2 : 1);
    for (int64_t g0 = 0; g0 < p.n_blocks; g0 += SQ_T) {
        const int nb = (int)(p.n_blocks - g0 < SQ_T ? p.n_blocks - g0 : SQ_T);
        for (int b = wave; b < nb; b += SQ_WAVES) {
            const float level = sq_block_level<CPLX>(det + (g0 + b) * blk_floats, p.block_det, p.wd, p.inv, lane);
            if (lane == 0) {
                s_level[b] = level;
                if (p.levels) p.levels[row * p.n_blocks + g0 + b] = level;
            }
        }
        __syncthreads();                               // every level of the group is taken before any of its signal is written
        const int gate = sq_gate_group(tid < nb ? s_level[tid] : 0.0f, nb, p.g, s_w, s_state, tid);
        if (tid < nb) {
            s_gate[tid] = (uint8_t)gate;
            if (p.gates) p.gates[row * p.n_blocks + g0 + tid] = (uint8_t)gate;
        }
        __syncthreads();
        if (p.out)
            sq_apply_span(p.in + row * p.in_stride + g0 * p.block_sig, p.out + row * p.out_stride + g0 * p.block_sig, s_gate, 0u,
                          (uint32_t)nb * (uint32_t)p.block_sig, (uint32_t)p.block_sig, p.wi, p.wo, tid, SQ_T);
        __syncthreads();                               // s_level and s_gate are the next group's from here on
    }
    if (tid == 0 && p.fin) { p.fin[2 * row] = s_state[0]; p.fin[2 * row + 1] = s_state[1]; }
}

// ---- LS: levels, gate, apply ------------------------------------------------------------------------------------------------------
// one wave per block, four blocks per workgroup; the grid's x strides over the row's blocks, its y is the row
template <bool CPLX>
__global__ void __launch_bounds__(256)
k_squelch_levels(const float* __restrict__ det, int64_t det_stride, int block_det, int wd, float inv, int64_t n_blocks,
                 float* __restrict__ levels)
{
    const int64_t row = blockIdx.y;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t blk_floats = (int64_t)block_det * (CPLX ? 2 : 1);
    det += row * det_stride;
    for (int64_t b = (int64_t)blockIdx.x * 4 + wave; b < n_blocks; b += (int64_t)gridDim.x * 4) {
        const float level = sq_block_level<CPLX>(det + b * blk_floats, block_det, wd, inv, lane);
        if (lane == 0) levels[row * n_blocks + b] = level;
    }
}

// one workgroup per row: the row's levels in groups of SQ_T, the state passing from group to group
__global__ void __launch_bounds__(SQ_T)
k_squelch_gate(SqRows p, const float* __restrict__ levels, uint8_t* __restrict__ gates)
{
    __shared__ int s_w[SQ_WAVES];
    __shared__ int s_state[2];
    const int64_t row = blockIdx.x;
    const int tid = threadIdx.x;
    if (tid == 0) sq_read_state(p, row, s_state);
    __syncthreads();
    for (int64_t g0 = 0; g0 < p.n_blocks; g0 += SQ_T) {
        const int nb = (int)(p.n_blocks - g0 < SQ_T ? p.n_blocks - g0 : SQ_T);
        const float level = tid < nb ? levels[row * p.n_blocks + g0 + tid] : 0.0f;
        const int gate = sq_gate_group(level, nb, p.g, s_w, s_state, tid);
        if (tid < nb) gates[row * p.n_blocks + g0 + tid] = (uint8_t)gate;
    }
    if (tid == 0 && p.fin) { p.fin[2 * row] = s_state[0]; p.fin[2 * row + 1] = s_state[1]; }
}

// grid x: tiles of SQ_TILE signal floats of a row; y: the row
__global__ void __launch_bounds__(256)
k_squelch_apply(const uint32_t* in, int64_t in_stride, uint32_t* out, int64_t out_stride, int block_sig, int wi, int wo, int64_t n_blocks,
                const uint8_t* __restrict__ gates)
{
    const int64_t row = blockIdx.y;
    const int64_t total = n_blocks * block_sig;
    const int64_t t0 = (int64_t)blockIdx.x * SQ_TILE;
    if (t0 >= total) return;
    const int64_t b0 = t0 / block_sig;
    const uint32_t count = (uint32_t)(total - t0 < SQ_TILE ? total - t0 : SQ_TILE);
    sq_apply_span(in + row * in_stride + t0, out + row * out_stride + t0, gates + row * n_blocks + b0, (uint32_t)(t0 - b0 * block_sig), count,
                  (uint32_t)block_sig, wi, wo, threadIdx.x, 256);
}

// ---- host: the route and the launcher ---------------------------------------------------------------------------------------------
namespace {
std::atomic<long long> g_squelch_launches{0};
std::atomic<int> g_squelch_route{SQUELCH_AUTO};

// floats per access (4 / 2 / 1) that every address of the form bits + k * 16 bytes allows
int width_of(uintptr_t bits) { return (bits & 15) == 0 ? 4 : (bits & 7) == 0 ? 2 : 1; }
}  // namespace

// Auto rule (the starting values; profiles/squelch_bench.txt): WG while the row has at most 1024 blocks and its detector plus signal
// bytes are at most 256 KiB; past either, LS when a workspace is given, WG (walking the row in groups of 1024 blocks) when not.
int squelch_route(int64_t n_blocks, int block_det, int det_complex, int block_sig, bool has_workspace, int forced)
{
    if (forced == SQUELCH_WG || n_blocks == 0) return SQUELCH_WG;
    if (forced == SQUELCH_LS) return has_workspace ? SQUELCH_LS : 0;
    const int64_t row_bytes = 4 * n_blocks * ((int64_t)block_det * (det_complex ? 2 : 1) + block_sig);
    if (n_blocks <= kSquelchWgBlocks && row_bytes <= kSquelchWgBytes) return SQUELCH_WG;
    return has_workspace ? SQUELCH_LS : SQUELCH_WG;
}

int squelch_launches_of(int route, bool detect_only) { return route == SQUELCH_LS ? (detect_only ? 2 : 3) : 1; }

// levels (rows x n_blocks floats) then gates (rows x n_blocks bytes), behind up to 15 bytes that align the levels
size_t squelch_rows_workspace_bytes(int rows, int64_t n_blocks)
{
    if (n_blocks < 0) n_blocks = 0;
    return (size_t)rows * (size_t)n_blocks * 5 + 64;
}

long long squelch_launch_count() { return g_squelch_launches.load(); }
void squelch_set_route(int route) { g_squelch_route.store(route); }
int squelch_forced_route() { return g_squelch_route.load(); }

void launch_squelch_rows(hipStream_t s, int route, const SquelchArgs& a, void* d_ws)
{
    if (a.rows < 1 || a.n_blocks < 0) return;
    const bool cplx = a.det_complex != 0, detect_only = a.out == nullptr;
    const int64_t blk_floats = (int64_t)a.block_det * (cplx ? 2 : 1);
    // row r starts at base + r * stride, and block b of it b * block floats further on
    uintptr_t det_bits = (uintptr_t)a.det | (uintptr_t)(a.n_blocks > 1 ? blk_floats * 4 : 0);
    uintptr_t in_bits = (uintptr_t)a.in, out_bits = (uintptr_t)a.out;
    if (a.rows > 1) {
        det_bits |= (uintptr_t)(a.det_stride * 4);
        in_bits |= (uintptr_t)(a.in_stride * 4);
        out_bits |= (uintptr_t)(a.out_stride * 4);
    }
    SqRows p;
    p.det = a.det; p.det_stride = a.det_stride; p.block_det = a.block_det; p.wd = width_of(det_bits);
    p.inv = (float)(1.0 / (double)a.block_det);
    p.in = reinterpret_cast<const uint32_t*>(a.in); p.in_stride = a.in_stride;
    p.out = reinterpret_cast<uint32_t*>(a.out); p.out_stride = a.out_stride;
    p.block_sig = detect_only ? 1 : a.block_sig; p.wi = width_of(in_bits); p.wo = width_of(out_bits);
    p.n_blocks = a.n_blocks;
    p.g.open = a.open_level; p.g.close = a.close_level; p.g.hang = a.hang; p.g.above = a.open_above;
    p.det0 = a.det0; p.hang0 = a.hang0; p.state = a.state; p.fin = a.fin;
    p.levels = a.levels; p.gates = a.gates;
    if (route != SQUELCH_LS || a.n_blocks == 0) {
        if (cplx) hipLaunchKernelGGL(k_squelch_wg<true>, dim3(a.rows), dim3(SQ_T), 0, s, p);
        else hipLaunchKernelGGL(k_squelch_wg<false>, dim3(a.rows), dim3(SQ_T), 0, s, p);
        g_squelch_launches.fetch_add(1);
        return;
    }
    const size_t cells = (size_t)a.rows * (size_t)a.n_blocks;
    float* ws_levels = reinterpret_cast<float*>(((uintptr_t)d_ws + 15) & ~(uintptr_t)15);
    uint8_t* ws_gates = reinterpret_cast<uint8_t*>(ws_levels + cells);
    float* levels = a.levels ? a.levels : ws_levels;
    uint8_t* gates = a.gates ? a.gates : ws_gates;
    const int64_t wgs = (a.n_blocks + 3) / 4;
    const dim3 lgrid((unsigned)(wgs < (1 << 20) ? wgs : (1 << 20)), a.rows);
    if (cplx) hipLaunchKernelGGL(k_squelch_levels<true>, lgrid, dim3(256), 0, s, p.det, p.det_stride, p.block_det, p.wd, p.inv, p.n_blocks, levels);
    else hipLaunchKernelGGL(k_squelch_levels<false>, lgrid, dim3(256), 0, s, p.det, p.det_stride, p.block_det, p.wd, p.inv, p.n_blocks, levels);
    hipLaunchKernelGGL(k_squelch_gate, dim3(a.rows), dim3(SQ_T), 0, s, p, levels, gates);
    if (!detect_only) {
        const int64_t tiles = (a.n_blocks * a.block_sig + SQ_TILE - 1) / SQ_TILE;
        hipLaunchKernelGGL(k_squelch_apply, dim3((unsigned)tiles, a.rows), dim3(256), 0, s, p.in, p.in_stride, p.out, p.out_stride, p.block_sig,
                           p.wi, p.wo, p.n_blocks, gates);
    }
    g_squelch_launches.fetch_add(squelch_launches_of(SQUELCH_LS, detect_only));
}

}  // namespace sdrhip
