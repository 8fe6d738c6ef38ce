// kernels_tail_rows.hip -- the audio tail behind a bank as ONE kernel over rows:
//     y[k] (a row of real demodulated samples)  --firResampler 3/10-->  z[m]  --firFilter(sym) * gain-->  audio[q]
//                                                 resample.c:70-87 (AVX order)    filter.c:60-68 (AVX order)
// It is k_fm_tail (kernels_tail.hip) with the row on blockIdx.y and phase 1 (fmDemod of the decimator's output) replaced by a
// load of the tile's y values from the row: the AM bank's envelope and the narrow-band FM bank's phase are already real rows.
// Phases 2 and 3 -- the tile of A = 2046 audio outputs, the seam predicates, the sequential recomputation of the Cross outputs
// of both stages from the same LDS tile, the late first output of an output block, the gain -- are k_fm_tail's, statement
// for statement (its body stays written in place there, so that its machine code does not move); what they argue about bits
// is argued there.  z lives only in LDS; y is read once per tile (7 % overlap between neighbouring tiles), audio written once.
//
// The loader.  The tile's y window starts at stream index y0 = 10 * (qa / 3), an even index: with the row's base and stride it
// is 16-, 8- or 4-byte aligned, the same for every lane of the workgroup, and the loads are that wide (as kernels_am.hip picks
// its access from base and stride).  Only the floats the cycles of this launch read are loaded; all of a thread's loads are
// issued before the first is stored to LDS, none behind a branch.  Stream indices outside [y_base, y_base + n_y) become zeros --
// the host refuses a launch whose receptive field does not lie inside, so they feed no owned output.
//
// Host side: audio_tail.cpp asks fm_tail_shape_ok and fm_tail_fused_fits (the tile is k_fm_tail's, so is the fit) before it launches.
#include "kernels.hpp"

#include <atomic>

namespace sdrhip {

namespace {

constexpr int TR_NT = 256;
constexpr int TR_A = kTailTileOutputs;                            // audio outputs per tile (multiple of 3)
constexpr int TR_LF = 128;                                        // audio filter length (64 half-taps)
constexpr int TR_NC = (TR_A + TR_LF - 1 + 2) / 3;                 // resampler cycles per tile: 725
constexpr int TR_NZ = 3 * TR_NC;                                  // z values per tile
constexpr int TR_NL = 64;                                         // resampler group length (padded)
constexpr int TR_WIN = 7 + TR_NL;                                 // y floats one cycle's three windows span: 71
constexpr int TR_NY_PAD = (10 * (TR_NC - 1) + TR_WIN + 3 + 8) & ~3;   // as k_fm_tail's: 7320
static_assert(TR_A % 3 == 0, "a tile starts on a polyphase cycle");
static_assert(10 * (TR_NC - 1) + TR_WIN + 1 <= TR_NY_PAD, "phase 2 reads 72 floats per cycle");

struct TailRowsParams {
    int64_t y_base;          // stream index of each row's y[0]
    int64_t n_y;             // readable elements per row
    int64_t y_stride;        // floats between rows of y
    int64_t audio_stride;    // floats between rows of audio
    int64_t q0, q1;          // audio outputs of this launch
    int row_stride;          // floats between the resampler's group rows
    int ntaps;               // resampler taps (unpadded)
    int rLp;                 // numCoeffsR (192)
    float gain;
    int64_t seam;            // block size B of every Pipe (0 = contiguous stream)
};

typedef float tr_f8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ tr_f8 tr_taps8(const float* base, int chunk)
{
    typedef const __attribute__((address_space(4))) tr_f8* cp;
    uint64_t a = reinterpret_cast<uint64_t>(base) + 32u * (uint32_t)chunk;
    asm volatile("" : "+s"(a));
    return *reinterpret_cast<cp>(a);
}

// ys[i0 + W * (tid + j * NT) ...] <- the row's floats, W per load, all ROUNDS loads of a thread in flight before the first store.
// src = the address of ys[0]'s stream element (readable only at [lo, hi) relative to it, hi - lo >= 8: a receptive field is longer);
// [i0, i1) = the LDS range to fill.  No load sits behind a branch: a vector that does not lie wholly inside [lo, hi) (or behind i1)
// is loaded from the first whole vector of the readable range instead and replaced by zeros; the at most two vectors that straddle
// lo or hi get their readable elements afterwards, one float at a time.
template <int W, int ROUNDS>
__device__ __forceinline__ void tr_load_tile(float* ys, const float* src, int64_t lo, int64_t hi, int i0, int i1, int tid)
{
    const int64_t safe = (lo + (W - 1)) & ~(int64_t)(W - 1);
    float v[ROUNDS][W];
    bool whole[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {
        const int i = i0 + W * (tid + j * TR_NT);
        whole[j] = i < i1 && i >= lo && i + W <= hi;
        const float* a = src + (whole[j] ? (int64_t)i : safe);
        if (W == 4) {
            const float4 t = *reinterpret_cast<const float4*>(a);
            v[j][0] = t.x; v[j][1] = t.y; v[j][W - 2] = t.z; v[j][W - 1] = t.w;
        } else if (W == 2) {
            const float2 t = *reinterpret_cast<const float2*>(a);
            v[j][0] = t.x; v[j][W - 1] = t.y;
        } else {
            v[j][0] = a[0];
        }
    }
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {
        const int i = i0 + W * (tid + j * TR_NT);
        if (i < i1) {
            const float z0 = whole[j] ? v[j][0] : 0.0f, z1 = whole[j] ? v[j][1 % W] : 0.0f, z2 = whole[j] ? v[j][W - 2 < 0 ? 0 : W - 2] : 0.0f,
                        z3 = whole[j] ? v[j][W - 1] : 0.0f;
            if (W == 4) *reinterpret_cast<float4*>(ys + i) = make_float4(z0, z1, z2, z3);
            else if (W == 2) *reinterpret_cast<float2*>(ys + i) = make_float2(z0, z3);
            else ys[i] = z0;
            if (W > 1 && !whole[j] && i + W > lo && i < hi) {                // straddles an end of the readable range
#pragma unroll
                for (int e = 0; e < W; e++)
                    if (i + e >= lo && i + e < hi) ys[i + e] = src[i + e];
            }
        }
    }
}

// y / audio: row r at y + r * y_stride / audio + r * audio_stride; audio[0] of a row = its output q0; groups: 3 rows of row_stride
// floats (group g = outputs m = 3c + g); rplain: the resampler's plain taps; fhalf / fplain: the audio filter's 64 half-taps / 128
// plain taps
__global__ void __launch_bounds__(TR_NT, 4) k_audio_tail_rows(const float* __restrict__ y, float* __restrict__ audio_rows,
                                                              const float* __restrict__ groups, const float* __restrict__ rplain,
                                                              const float* __restrict__ fhalf, const float* __restrict__ fplain,
                                                              TailRowsParams p)
{
    __shared__ __attribute__((aligned(16))) float ys[TR_NY_PAD];
    __shared__ __attribute__((aligned(16))) float zs[TR_NZ + 16];
    // the un-grouped taps of the two sequential (Cross) kernels: read per lane at data-dependent offsets
    __shared__ float rpl[3 * TR_NL];
    __shared__ float fpl[TR_LF];
    if (threadIdx.x < 3 * TR_NL) rpl[threadIdx.x] = threadIdx.x < p.ntaps ? rplain[threadIdx.x] : 0.0f;
    if (threadIdx.x < TR_LF) fpl[threadIdx.x] = fplain[threadIdx.x];
    const int tid = threadIdx.x;
    const int64_t qa = (p.q0 / 3) * 3 + (int64_t)blockIdx.x * TR_A;     // first audio output of the tile (cycle aligned)
    const int64_t c0 = qa / 3;                                           // first resampler cycle
    const int64_t y0 = 10 * c0;                                          // first y of the tile
    float* audio = audio_rows + (int64_t)blockIdx.y * p.audio_stride;

    // z values this launch needs from the tile: m in [max(q0, qa), min(q1, qa + A) + 127) -- a short launch (one source
    // block per push) fills only the front of its single tile, and the rest is neither loaded nor computed
    const int64_t m_need_lo = p.q0 > qa ? p.q0 : qa;
    const int64_t m_need_hi = (p.q1 < qa + TR_A ? p.q1 : qa + TR_A) + TR_LF - 1;
    const int cl_lo = (int)((m_need_lo - qa) / 3);
    const int cl_hi0 = (int)((m_need_hi - qa + 2) / 3);                // one past the last cycle needed (<= NC)
    const int cl_hi = cl_hi0 < TR_NC ? cl_hi0 : TR_NC;

    // ---- phase 1: the tile's y values, ys[i] = stream element y0 + i, for the 72 floats each needed cycle reads
    {
        const int i0 = (10 * cl_lo) & ~3;                                 // whole quads: LDS stores stay 16-byte aligned
        const int i1 = 10 * (cl_hi - 1) + TR_WIN + 1;                    // <= TR_NY_PAD - 8
        const float* src = y + (int64_t)blockIdx.y * p.y_stride + (y0 - p.y_base);   // formed, not read, outside [lo, hi)
        const int64_t lo = p.y_base - y0, hi = lo + p.n_y;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(src);
        if ((bits & 15) == 0) tr_load_tile<4, (TR_NY_PAD / 4 + TR_NT - 1) / TR_NT>(ys, src, lo, hi, i0, i1, tid);
        else if ((bits & 7) == 0) tr_load_tile<2, (TR_NY_PAD / 2 + TR_NT - 1) / TR_NT>(ys, src, lo, hi, i0, i1, tid);
        else tr_load_tile<1, (TR_NY_PAD + TR_NT - 1) / TR_NT>(ys, src, lo, hi, i0, i1, tid);
    }
    __syncthreads();

    // ---- phase 2: polyphase resampler, one cycle (3 outputs) per thread and round.
    // Seam classification in 32-bit arithmetic relative to the tile (the launcher guarantees a tile spans less than one
    // buffer of the reference's Pipes, so at most one boundary crosses it): rz0 / rq0 = position of the tile's first z
    // window / first audio window inside its buffer, in upsampled units / z samples.
    const int sBI = (int)(p.seam * 3);
    const int rz0 = sBI > 0 ? (int)((30 * c0) % sBI) : 0;
    const int rq0 = p.seam > 0 ? (int)(qa % p.seam) : 0;
#pragma unroll 1
    for (int cl = cl_lo + tid; cl < cl_hi; cl += TR_NT) {
        constexpr int PRE[3] = {0, 4, 7};
        float w[TR_WIN + 1];
        const float* win = ys + 10 * cl;                               // 8-byte aligned; 10-dword lane stride: conflict-free
#pragma unroll
        for (int i = 0; i < (TR_WIN + 1) / 2; i++) {
            const float2 t = *reinterpret_cast<const float2*>(win + 2 * i);
            w[2 * i] = t.x;
            w[2 * i + 1] = t.y;
        }
        float res[3];
#pragma unroll
        for (int g = 0; g < 3; g++) {
            // the 64 taps of the group are wave-uniform: scalar loads (constant address space) from an address the compiler
            // cannot see through (k_fm_tail: no hoisting of all 192 taps across the `cl` loop)
            uint64_t ca = reinterpret_cast<uint64_t>(groups + g * p.row_stride);
            asm volatile("" : "+s"(ca));
            const __attribute__((address_space(4))) float* c = reinterpret_cast<const __attribute__((address_space(4))) float*>(ca);
            float acc[8];
#pragma unroll
            for (int l = 0; l < 8; l++) acc[l] = 0.0f;
#pragma unroll
            for (int j = 0; j < TR_NL; j++) acc[j & 7] = acc[j & 7] + c[j] * w[PRE[g] + j];
            res[g] = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
        }
        if (sBI > 0) {
#pragma unroll
            for (int g = 0; g < 3; g++) {
                int rv = rz0 + 10 * (3 * cl + g);                      // window start inside its buffer (upsampled units)
                if (rv >= sBI) rv -= sBI;
                if (rv + p.rLp <= sBI) continue;                       // the window lies inside one buffer: a One output
                const int64_t m = 3 * (c0 + cl) + g;
                const int64_t v = m * 10;
                const int64_t edge = v + (sBI - rv);                   // the buffer boundary the window straddles
                if (seam_has_crossover(edge, 3, 10, p.rLp) && !late_output_is_one(m, edge, 3, 10, p.seam)) {
                    // resampleCrossHighLevel (FilterInternal.hs:410-423): stride 3 through the unpadded taps, sequential
                    const int64_t pos = (v + 2) / 3;
                    const int fo = (int)(pos * 3 - v);
                    const float* x = ys + (pos - y0);
                    const int nterms = (p.ntaps - fo + 2) / 3;            // taps fo, fo+3, .. < ntaps
                    const float* tp = rpl + fo;
                    float r = 0.0f;
#pragma unroll 8
                    for (int l = 0; l < nterms; l++) r = r + x[l] * tp[3 * l];
                    res[g] = r;
                }
            }
        }
        zs[3 * cl] = res[0];
        zs[3 * cl + 1] = res[1];
        zs[3 * cl + 2] = res[2];
    }
    __syncthreads();

    // ---- phase 3: symmetric audio filter (pair-add first, 8 lanes, tree) + gain; 4 consecutive outputs per thread.
    constexpr int NK = TR_LF / 2;
    const int t_lo = (int)((m_need_lo - qa) / 4);
    const int o_hi = (int)((p.q1 < qa + TR_A ? p.q1 : qa + TR_A) - qa);   // one past the last output of the tile this launch owns
#pragma unroll 1
    for (int t = t_lo + tid; 4 * t < o_hi; t += TR_NT) {
        const float* win = zs + 4 * t;
        float acc[4][8];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int l = 0; l < 8; l++) acc[r][l] = 0.0f;
#pragma unroll 1
        for (int j = 0; j < NK / 8; j++) {
            const tr_f8 c8 = tr_taps8(fhalf, j);
            const float* fp = win + 8 * j;
            const float* bp = win + 2 * NK - 8 - 8 * j;
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
            if (p.seam > 0) {
                int rq = rq0 + o;                                      // window start inside its buffer of z samples
                if (rq >= (int)p.seam) rq -= (int)p.seam;
                if (rq + TR_LF > (int)p.seam) {
                    // filterCrossHighLevel (FilterInternal.hs:404-408) on coeffs ++ reverse coeffs: sequential, no pair-add
                    float s = 0.0f;
#pragma unroll 16
                    for (int j = 0; j < TR_LF; j++) s = s + zs[o + j] * fpl[j];
                    res = s;
                }
            }
            res = res * p.gain;
            if (o < TR_A && q >= p.q0 && q < p.q1) audio[q - p.q0] = res;
        }
    }
}

std::atomic<long long> g_audio_tail_launches{0};

}  // namespace

long long audio_tail_launch_count() { return g_audio_tail_launches.load(std::memory_order_relaxed); }

void launch_audio_tail_rows(hipStream_t s, const float* d_y, int64_t y_stride, int64_t y_base, int64_t n_y, float* d_audio,
                            int64_t audio_stride, int rows, int64_t q0, int64_t q1, const FmTailTables& t)
{
    TailRowsParams p;
    p.y_base = y_base; p.n_y = n_y; p.y_stride = y_stride; p.audio_stride = audio_stride; p.q0 = q0; p.q1 = q1;
    p.row_stride = t.row_stride; p.ntaps = t.ntaps; p.rLp = t.rLp; p.gain = t.gain; p.seam = t.seam;
    const int64_t qa0 = (q0 / 3) * 3;
    const int64_t tiles = (q1 - qa0 + TR_A - 1) / TR_A;
    g_audio_tail_launches.fetch_add(1, std::memory_order_relaxed);
    hipLaunchKernelGGL(k_audio_tail_rows, dim3((unsigned)tiles, (unsigned)rows), dim3(TR_NT), 0, s, d_y, d_audio, t.d_groups, t.d_rplain,
                       t.d_fhalf, t.d_fplain, p);
}

}  // namespace sdrhip
