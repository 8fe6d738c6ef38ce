// kernels_tail_any.hip -- the audio tail over rows for ANY down-sampling ratio a narrow receiver uses, as ONE kernel:
//     y[k] (a row of real demodulated samples)  --firResampler I/D-->  z[m]  --firFilter(sym) * gain-->  audio[q]
//                                                 resample.c:70-87 (AVX order)   filter.c:60-68 (AVX order)
// It is k_audio_tail_rows (kernels_tail_rows.hip) without that kernel's compile-time shape (3/10, 64-float groups, 64 half-taps) and
// without its one-boundary-per-tile shortcut: I, D, the group length, the tap counts and the block are run-time numbers, and every
// output decides One / Cross on its own, so a tile may hold any number of buffer boundaries of both stages (the narrow Pipe's blocks
// are a few hundred outputs).  The summation orders are those kernels' and the reference's; nothing new is argued here.
//
// Tile.  A = kTailAnyTileOutputs = 840 audio outputs of one row per workgroup -- a multiple of every I <= 8, so every tile starts on
// a polyphase cycle: qa = I * floor(q0 / I) + 840 * blockIdx.x, first cycle c0 = qa / I, first input y0 = D * c0.  The tile needs the
// z values [qa, qa + 840 + Lf - 1), i.e. at most NC = ceil((840 + Lf - 1) / I) cycles, and the y window of those cycles; a short
// launch computes only the cycles and outputs it owns.
//   phase 1  the y window -> LDS.  It is staged from the 16-byte boundary at or below its first element (`sh` floats early, from the
//            row's base and stride), so every load is 16 bytes wide whatever the base; all of a thread's loads are issued before its
//            first LDS store, none behind a branch; a vector that is not wholly inside [y_base, y_base + n_y) is loaded from the first
//            whole vector of the readable range instead and replaced by zeros, its readable elements then one float at a time.  No
//            byte outside the readable range is read.  LDS index i + i / 32 (k_narrow_rows' skew): phase 2's lanes read at a stride
//            of D floats, which would conflict for D = 4, 8, 16.
//   phase 2  one thread per cycle, the I groups in a rolled loop, the group's nloop taps in rolled chunks of eight from wave-uniform
//            scalar loads: eight lane partials, ((a0+a1)+(a2+a3))+((a4+a5)+(a6+a7)).  An output whose window straddles a boundary of
//            the resampler's buffers (block * I upsampled units) is Cross when seam_has_crossover says so and it is not the late first
//            output of an output block (late_output_is_one): resampleCrossHighLevel (FilterInternal.hs:410-423), stride I through the
//            unpadded taps, sequential, from the same LDS window.  z lives only in LDS.
//   phase 3  four consecutive outputs per thread: pair-add first, eight lanes, the same tree (filter.c's AVX order), half-taps by
//            scalar loads in chunks of eight; an output whose window straddles a boundary of the filter's buffers (block z samples) is
//            recomputed sequentially over the Lf plain taps (filterCrossHighLevel); then `* gain` as a separate multiply.
// Window positions inside a buffer are (tile base + offset) mod buffer in 32 bits: the base by one 64-bit remainder per thread.
//
// Shapes: audio_tail_any_fits below, the one predicate.  Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
// 76 VGPRs, 94 SGPRs, 27696 bytes of LDS, no scratch, 5 workgroups per CU (160 KiB of LDS / 27696; 5 waves per SIMD).
#include "kernels.hpp"

#include <atomic>

namespace sdrhip {

namespace {

constexpr int TA_NT = 256;
constexpr int TA_A = kTailAnyTileOutputs;
constexpr int TA_LF_MAX = kTailAnyMaxFilter;                       // audio filter length (2 x half-taps) at most
constexpr int TA_NL_MAX = kTailAnyMaxGroup;                        // resampler group length (padded) at most
constexpr int TA_I_MAX = kTailAnyMaxInterp;
constexpr int TA_NZ = TA_A + TA_LF_MAX - 1 + TA_I_MAX - 1;         // z values of a tile at most (whole cycles): 974
constexpr int TA_NY = kTailAnyWindowFloats;                        // y floats of a tile at most, the early floats and rounding included
constexpr int TA_ROUNDS = (TA_NY / 4 + TA_NT - 1) / TA_NT;
static_assert(TA_A % 840 == 0 && TA_A % 4 == 0, "a tile starts on a polyphase cycle for every I <= 8; phase 3 takes 4 outputs per thread");
static_assert(TA_NY % 4 == 0, "whole 16-byte vectors");

struct TailAnyParams {
    int64_t y_base, n_y, y_stride, audio_stride, q0, q1;
    int64_t seam;            // block size B of every Pipe (0 = contiguous stream)
    int I, D;
    int nloop;               // floats a group's One walk takes (a multiple of 8)
    int row_stride;          // floats between the resampler's group rows
    int ntaps;               // resampler taps (unpadded)
    int rLp;                 // numCoeffsR
    int Lf;                  // numCoeffsF = 2 x half-taps
    int premax;              // pre[I - 1]
    int pre[TA_I_MAX];       // inputs between a cycle's first window and group g's
    float gain;
};

typedef float ta_f8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ ta_f8 ta_taps8(const float* base, int chunk)
{
    typedef const __attribute__((address_space(4))) ta_f8* cp;
    uint64_t a = reinterpret_cast<uint64_t>(base) + 32u * (uint32_t)chunk;
    asm volatile("" : "+s"(a));
    return *reinterpret_cast<cp>(a);
}

__device__ __forceinline__ int ta_sk(int i) { return i + (i >> 5); }

// ys[sk(i)] <- src[i] for i in [i0, i1) (i0 a multiple of 4), zeros outside [lo, hi); src + 4 k is 16-byte aligned, hi - lo >= 7
__device__ __forceinline__ void ta_load_tile(float* ys, const float* src, int64_t lo, int64_t hi, int i0, int i1, int tid)
{
    const int64_t safe = (lo + 3) & ~(int64_t)3;
    float4 v[TA_ROUNDS];
    bool whole[TA_ROUNDS];
#pragma unroll
    for (int j = 0; j < TA_ROUNDS; j++) {
        const int i = i0 + 4 * (tid + j * TA_NT);
        whole[j] = i < i1 && i >= lo && i + 4 <= hi;
        v[j] = *reinterpret_cast<const float4*>(src + (whole[j] ? (int64_t)i : safe));
    }
#pragma unroll
    for (int j = 0; j < TA_ROUNDS; j++) {
        const int i = i0 + 4 * (tid + j * TA_NT);
        if (i < i1) {
            float* d = ys + ta_sk(i);                                  // i is a multiple of 4: the four share one skew
            d[0] = whole[j] ? v[j].x : 0.0f;
            d[1] = whole[j] ? v[j].y : 0.0f;
            d[2] = whole[j] ? v[j].z : 0.0f;
            d[3] = whole[j] ? v[j].w : 0.0f;
            if (!whole[j] && i + 4 > lo && i < hi) {                   // straddles an end of the readable range
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (i + e >= lo && i + e < hi) d[e] = src[i + e];
            }
        }
    }
}

// y / audio: row r at y + r * y_stride / audio + r * audio_stride; audio[0] of a row = its output q0; groups: I rows of row_stride
// floats (row g = outputs m = I c + g); rplain: the resampler's plain taps; fhalf / fplain: the filter's half-taps / Lf plain taps
__global__ void __launch_bounds__(TA_NT, 4) k_audio_tail_rows_any(const float* __restrict__ y, float* __restrict__ audio_rows,
                                                                  const float* __restrict__ groups, const float* __restrict__ rplain,
                                                                  const float* __restrict__ fhalf, const float* __restrict__ fplain,
                                                                  TailAnyParams p)
{
    __shared__ __attribute__((aligned(16))) float ys[TA_NY + TA_NY / 32 + 4];
    __shared__ __attribute__((aligned(16))) float zs[TA_NZ + 18];
    __shared__ float rpl[TA_I_MAX * TA_NL_MAX];                       // the un-grouped taps of the two sequential (Cross) kernels
    __shared__ float fpl[TA_LF_MAX];
    __shared__ int pre_s[TA_I_MAX];
    const int tid = threadIdx.x;
    for (int i = tid; i < p.ntaps; i += TA_NT) rpl[i] = rplain[i];
    if (tid < p.Lf) fpl[tid] = fplain[tid];
    {
        int v = 0;
#pragma unroll
        for (int i = 0; i < TA_I_MAX; i++)
            if (tid == i) v = p.pre[i];
        if (tid < TA_I_MAX) pre_s[tid] = v;
    }
    const int I = p.I, D = p.D;
    const int64_t qa = (p.q0 / I) * I + (int64_t)blockIdx.x * TA_A;     // first audio output of the tile (cycle aligned)
    const int64_t c0 = qa / I;                                           // first resampler cycle
    const int64_t y0 = D * c0;                                           // first y of the tile
    float* audio = audio_rows + (int64_t)blockIdx.y * p.audio_stride;

    // z values this launch needs from the tile: m in [max(q0, qa), min(q1, qa + A) + Lf - 1)
    const int64_t m_need_lo = p.q0 > qa ? p.q0 : qa;
    const int64_t m_need_hi = (p.q1 < qa + TA_A ? p.q1 : qa + TA_A) + p.Lf - 1;
    const int cl_lo = (int)(m_need_lo - qa) / I;
    const int cl_hi = ((int)(m_need_hi - qa) + I - 1) / I;             // one past the last cycle needed

    // ---- phase 1: the tile's y values, ys[sk(i)] = stream element y0 - sh + i
    const float* row0 = y + (int64_t)blockIdx.y * p.y_stride + (y0 - p.y_base);     // formed, not read, outside the readable range
    const int sh = (int)((reinterpret_cast<uintptr_t>(row0) & 15) >> 2);
    {
        const int i0 = (D * cl_lo + sh) & ~3;
        const int i1 = D * (cl_hi - 1) + p.premax + p.nloop + sh;        // <= TA_NY - 4 (audio_tail_any_fits)
        const int64_t lo = p.y_base - y0 + sh, hi = lo + p.n_y;
        ta_load_tile(ys, row0 - sh, lo, hi, i0, i1, tid);
    }
    __syncthreads();

    // ---- phase 2: polyphase resampler, one cycle (I outputs) per thread and round
    const uint32_t sBI = (uint32_t)(p.seam * I);
    const uint32_t rz0 = sBI > 0 ? (uint32_t)((uint64_t)(qa * D) % sBI) : 0;     // the tile's first window inside its buffer (upsampled units)
    const uint32_t seam = (uint32_t)p.seam;
    const uint32_t rq0 = seam > 0 ? (uint32_t)((uint64_t)qa % seam) : 0;         // ... of the filter (z samples)
    const int nch = p.nloop >> 3;
#pragma unroll 1
    for (int cl = cl_lo + tid; cl < cl_hi; cl += TA_NT) {
#pragma unroll 1
        for (int g = 0; g < I; g++) {
            const int ws = D * cl + pre_s[g] + sh;                       // window start in the tile
            const float* grow = groups + g * p.row_stride;
            float acc[8];
#pragma unroll
            for (int l = 0; l < 8; l++) acc[l] = 0.0f;
#pragma unroll 1
            for (int k = 0; k < nch; k++) {
                const ta_f8 c8 = ta_taps8(grow, k);
                const int e = ws + 8 * k;
                float w[8];
#pragma unroll
                for (int l = 0; l < 8; l++) w[l] = ys[ta_sk(e + l)];
#pragma unroll
                for (int l = 0; l < 8; l++) acc[l] = acc[l] + c8[l] * w[l];
            }
            float res = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
            if (sBI > 0) {
                const int j = I * cl + g;                              // z index in the tile
                const uint32_t rv = (rz0 + (uint32_t)(D * j)) % sBI;   // window start inside its buffer
                if (rv + (uint32_t)p.rLp > sBI) {                      // the window straddles a boundary
                    const int64_t m = qa + j;
                    const int64_t v = m * D;
                    const int64_t edge = v + (sBI - rv);
                    if (seam_has_crossover(edge, I, D, p.rLp) && !late_output_is_one(m, edge, I, D, p.seam)) {
                        // the window starts at the output's first input, ceil(v / I), as the One walk's does
                        const int fo = (int)(((v + I - 1) / I) * I - v);
                        const int nterms = (p.ntaps - fo + I - 1) / I;    // taps fo, fo + I, .. < ntaps (<= nloop inputs)
                        float r = 0.0f;
#pragma unroll 4
                        for (int l = 0; l < nterms; l++) r = r + ys[ta_sk(ws + l)] * rpl[fo + I * l];
                        res = r;
                    }
                }
            }
            zs[I * cl + g] = res;
        }
    }
    __syncthreads();

    // ---- phase 3: symmetric audio filter (pair-add first, 8 lanes, tree) + gain; 4 consecutive outputs per thread
    const int Lf = p.Lf;
    const int nfc = Lf >> 4;                                           // chunks of 8 half-taps
    const int t_lo = (int)(m_need_lo - qa) / 4;
    const int o_hi = (int)((p.q1 < qa + TA_A ? p.q1 : qa + TA_A) - qa);   // one past the last output of the tile this launch owns
#pragma unroll 1
    for (int t = t_lo + tid; 4 * t < o_hi; t += TA_NT) {
        const float* win = zs + 4 * t;
        float acc[4][8];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int l = 0; l < 8; l++) acc[r][l] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < nfc; j++) {
            const ta_f8 c8 = ta_taps8(fhalf, j);
            const float* fp = win + 8 * j;
            const float* bp = win + Lf - 8 - 8 * j;
            float fw[12], bw[12];
#pragma unroll
            for (int qd = 0; qd < 3; qd++) {
                const float4 a = *reinterpret_cast<const float4*>(fp + 4 * qd);
                fw[4 * qd] = a.x; fw[4 * qd + 1] = a.y; fw[4 * qd + 2] = a.z; fw[4 * qd + 3] = a.w;
                const float4 b = *reinterpret_cast<const float4*>(bp + 4 * qd);
                bw[4 * qd] = b.x; bw[4 * qd + 1] = b.y; bw[4 * qd + 2] = b.z; bw[4 * qd + 3] = b.w;
            }
#pragma unroll
            for (int kk = 0; kk < 8; kk++)
#pragma unroll
                for (int r = 0; r < 4; r++) acc[r][kk] = acc[r][kk] + c8[kk] * (fw[r + kk] + bw[r + 7 - kk]);
        }
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int o = 4 * t + r;
            const int64_t q = qa + o;
            float res = ((acc[r][0] + acc[r][1]) + (acc[r][2] + acc[r][3])) + ((acc[r][4] + acc[r][5]) + (acc[r][6] + acc[r][7]));
            if (seam > 0) {
                const uint32_t rq = (rq0 + (uint32_t)o) % seam;        // window start inside its buffer of z samples
                if (rq + (uint32_t)Lf > seam) {
                    // filterCrossHighLevel (FilterInternal.hs:404-408) on coeffs ++ reverse coeffs: sequential, no pair-add
                    float s = 0.0f;
#pragma unroll 8
                    for (int j = 0; j < Lf; j++) s = s + zs[o + j] * fpl[j];
                    res = s;
                }
            }
            res = res * p.gain;
            if (o < TA_A && q >= p.q0 && q < p.q1) audio[q - p.q0] = res;
        }
    }
}

std::atomic<long long> g_tail_any_launches{0};

}  // namespace

long long audio_tail_any_launch_count() { return g_tail_any_launches.load(std::memory_order_relaxed); }

bool audio_tail_any_fits(const TailAnyShape& s, int64_t block)
{
    if (s.cplx || s.rlanes != 8 || s.flanes != 8 || !s.fsym || s.ffactor != 1) return false;      // real data, AVX orders, symmetric filter
    if (s.I < 1 || s.I > kTailAnyMaxInterp || s.D <= s.I || s.ngroups != s.I) return false;       // a cycle is I outputs: gcd(I, D) = 1
    if (s.nloop < 8 || s.nloop % 8 != 0 || s.nloop > kTailAnyMaxGroup || s.row_stride < s.nloop || s.row_stride > kTailAnyMaxGroup) return false;
    if (s.ntaps < 1 || s.ntaps > s.I * kTailAnyMaxGroup || s.rLp < s.D) return false;
    if (s.fLp < 16 || s.fLp % 16 != 0 || s.fLp > kTailAnyMaxFilter) return false;
    // the tile's y window: NC cycles, the last one's last group, the staging shift and the rounding to whole vectors
    int premax = 0;
    for (int g = 0; g + 1 < s.I; g++) premax += s.increments[g];
    const int64_t NC = (kTailAnyTileOutputs + s.fLp - 1 + s.I - 1) / s.I;
    if ((int64_t)s.D * (NC - 1) + premax + s.nloop + 8 > kTailAnyWindowFloats) return false;
    // any block the tail's create admits (no tighter lower bound: every output decides One / Cross on its own), below 2^27:
    // positions inside a buffer are 32-bit
    if (block < 0 || block > ((int64_t)1 << 27)) return false;
    if (block > 0 && (block * s.I < s.rLp || block < s.fLp)) return false;
    return true;
}

void launch_audio_tail_rows_any(hipStream_t st, const float* d_y, int64_t y_stride, int64_t y_base, int64_t n_y, float* d_audio,
                                int64_t audio_stride, int rows, int64_t q0, int64_t q1, const TailAnyShape& s, const FmTailTables& t)
{
    TailAnyParams p;
    p.y_base = y_base; p.n_y = n_y; p.y_stride = y_stride; p.audio_stride = audio_stride; p.q0 = q0; p.q1 = q1;
    p.seam = t.seam; p.I = s.I; p.D = s.D; p.nloop = s.nloop; p.row_stride = t.row_stride; p.ntaps = t.ntaps; p.rLp = t.rLp;
    p.Lf = s.fLp; p.gain = t.gain; p.premax = 0;
    int acc = 0;
    for (int g = 0; g < kTailAnyMaxInterp; g++) {
        p.pre[g] = g < s.I ? acc : 0;
        if (g < s.I) { p.premax = acc; acc += s.increments[g]; }
    }
    const int64_t qa0 = (q0 / s.I) * s.I;
    const int64_t tiles = (q1 - qa0 + TA_A - 1) / TA_A;
    g_tail_any_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_audio_tail_rows_any, dim3((unsigned)tiles, (unsigned)rows), dim3(TA_NT), 0, st, d_y, d_audio, t.d_groups, t.d_rplain,
                       t.d_fhalf, t.d_fplain, p);
}

}  // namespace sdrhip
