// kernels_narrow.hip -- the narrow-channel bank (sdrhip_narrow_bank_run, narrow_bank.cpp): everything behind the tuner bank in ONE launch.
//
// k_narrow_rows<FORM> is the complex second decimator over the rows the tuner bank has written, with the demodulator as its store:
// row j's stage-2 output k is summed from its stage-1 outputs [k D2, k D2 + Lp2) and leaves the kernel as am_magnitude(re, im)
// (NARROW_ENV) or as fm_phase(y[k], y[k - 1]) (NARROW_FM).  No stage-2 complex row is written or read back.
//
// Geometry.  One workgroup per (tile, channel), flat 1-D grid, channel = b % K.  A tile is NT = 256 consecutive outputs, one thread
// each; its input span of (NT - 1) D2 + Lp2 complex samples is staged into LDS with 16-byte loads (rows are 16-byte aligned and the
// span starts at an even sample: an odd tile start stages one sample more in front), every load issued before the first LDS store,
// zeros where the row has no readable sample.  The LDS index of sample i is i + i / 32: with D2 = 4 / 8 / 16 the 32 lanes of a group
// read samples D2 apart, which without the skew are 2 .. 16 lanes a bank.
//
// Arithmetic: nothing new.  A One output is decimateAVXRC's: four complex lane partials (eight float lanes), partial l over taps
// l, l + 4, ..., each product rounded before it is added (the first addition, to +0, is first_mac), then (p0 + p1) + (p2 + p3) --
// the CO_L4 order of kernels_generic.hip and split_tile.hpp.  A Cross output (its window straddles a multiple of seam_block2) is the
// sequential sum over the Lp2 plain taps, k_fir_cplx_crossfix's loop, by the same thread; the One / Cross rule is is_cross of
// kernels.hpp for I = 1, reduced in 32 bits (seam_block2 < 2^30; any seam_block2 >= Lp2: a tile may hold several seams).
//
// NARROW_FM: the finished pairs go to NT pairs of LDS, and after a barrier thread t stores fm_phase(y[t], y[t - 1]).  Tiles OVERLAP
// by one output so that no workgroup waits on another: a tile advances by NT - 1, thread 0 of every tile but the first computes a
// predecessor only and stores nothing; the launch's output 0 takes its predecessor from d_state (null = (0, 0)), and the thread that
// stores the last output writes its pair to d_final -- the steps of kernels_tuner_bank.hip's OUT_FM form.
#include <atomic>

#include "am.hpp"
#include "demod.hpp"
#include "first_mac.hpp"
#include "kernels.hpp"

namespace sdrhip {

static std::atomic<long long> g_narrow_bank_launches{0};
long long narrow_bank_launch_count() { return g_narrow_bank_launches.load(); }

namespace {

constexpr int NT = kNarrowTileThreads;
constexpr int SPAN_MAX = (NT - 1) * kNarrowMaxFactor + kNarrowMaxTaps + 1;      // + 1: an odd tile start stages from the sample before
constexpr int PAIRS_MAX = (SPAN_MAX + 1) / 2;
constexpr int LOADS = (PAIRS_MAX + NT - 1) / NT;                                // 16-byte loads a thread issues at most
__host__ __device__ constexpr int skew(int i) { return i + (i >> 5); }

struct NarrowArgs {
    const float* in;        // row 0's stage-1 output in_base; rows in_stride floats apart, 16-byte aligned
    int64_t in_stride;
    int64_t x0;             // k_begin * D2 - in_base: output 0's first sample in its row
    int64_t n_in;           // readable complex samples per row
    float* out;
    int64_t out_stride;
    const float* taps;      // Lp2 plain prepared taps
    const float* state;     // NARROW_FM: K (re, im) pairs, output k_begin - 1; null = zeros
    float* final_;          // NARROW_FM: K pairs that receive output k_end - 1; null = not wanted
    int count, channels, D, Lp;
    int seam;               // 0 = contiguous; else Lp <= seam < 2^30
    int r0;                 // (k_begin * D2) mod seam
};

template <int FORM>
__global__ void __launch_bounds__(NT) k_narrow_rows(NarrowArgs a)
{
    constexpr int ADV = narrow_tile_advance(FORM);
    __shared__ __attribute__((aligned(16))) float2 lds[skew(SPAN_MAX) + 1];
    __shared__ float2 edge[FORM == NARROW_FM ? NT : 1];

    const unsigned nch = (unsigned)a.channels;
    const unsigned j = blockIdx.x % nch;
    const int tile = (int)(blockIdx.x / nch);
    const int tid = (int)threadIdx.x;
    const int out0 = tile * ADV;
    const int nout = a.count - out0 < NT ? a.count - out0 : NT;          // outputs this tile computes
    const float* row = a.in + (int64_t)j * a.in_stride;

    // ---- stage [s0, s0 + span) of the row: pairs of samples from the even sample at or before s0
    const int64_t s0 = a.x0 + (int64_t)out0 * a.D;
    const int odd = (int)(s0 & 1);
    const int64_t e0 = s0 - odd;
    const int span = (nout - 1) * a.D + a.Lp + odd;
    const int npairs = (span + 1) >> 1;
    float4 r[LOADS];
#pragma unroll
    for (int q = 0; q < LOADS; q++) {
        const int p = q * NT + tid;
        const int64_t s = e0 + 2 * (int64_t)p;
        r[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (p < npairs) {
            if (s + 1 < a.n_in) {
                r[q] = *reinterpret_cast<const float4*>(row + 2 * s);
            } else if (s < a.n_in) {
                const float2 v = *reinterpret_cast<const float2*>(row + 2 * s);
                r[q].x = v.x;
                r[q].y = v.y;
            }
        }
    }
#pragma unroll
    for (int q = 0; q < LOADS; q++) {
        const int p = q * NT + tid;
        if (p < npairs) {
            lds[skew(2 * p)] = make_float2(r[q].x, r[q].y);
            lds[skew(2 * p + 1)] = make_float2(r[q].z, r[q].w);
        }
    }
    __syncthreads();

    float2 res = make_float2(0.0f, 0.0f);
    if (tid < nout) {
        const int w = odd + tid * a.D;                                   // the window's first sample in the tile
        bool cross = false;
        if (a.seam > 0) {
            // is_cross for I = 1: the window [v, v + Lp) of output m, v = m D2, passes the end of the buffer v lies in
            const uint32_t rt = (uint32_t)(((uint64_t)a.r0 + (uint64_t)out0 * (uint64_t)a.D) % (uint32_t)a.seam);
            const uint32_t rr = (rt + (uint32_t)(tid * a.D)) % (uint32_t)a.seam;
            cross = rr + (uint32_t)a.Lp > (uint32_t)a.seam;
        }
        if (cross) {
            float re = 0.0f, im = 0.0f;
            for (int t = 0; t < a.Lp; t++) {
                const float2 s = lds[skew(w + t)];
                re = re + s.x * a.taps[t];
                im = im + s.y * a.taps[t];
            }
            res = make_float2(re, im);
        } else {
            float2 acc[4];
#pragma unroll
            for (int l = 0; l < 4; l++) {
                const float2 s = lds[skew(w + l)];
                acc[l] = make_float2(first_mac(a.taps[l], s.x), first_mac(a.taps[l], s.y));
            }
            for (int t = 4; t < a.Lp; t += 4) {
#pragma unroll
                for (int l = 0; l < 4; l++) {
                    const float2 s = lds[skew(w + t + l)];
                    acc[l].x = acc[l].x + a.taps[t + l] * s.x;
                    acc[l].y = acc[l].y + a.taps[t + l] * s.y;
                }
            }
            res = make_float2((acc[0].x + acc[1].x) + (acc[2].x + acc[3].x), (acc[0].y + acc[1].y) + (acc[2].y + acc[3].y));
        }
    }

    float* dst = a.out + (int64_t)j * a.out_stride + out0 + tid;
    if constexpr (FORM == NARROW_FM) {
        edge[tid] = res;
        __syncthreads();
        if (tid >= nout) return;
        // thread 0 of a later tile holds a predecessor only
        if (tile > 0 && tid == 0) return;
        float2 v[2];
        if (tid > 0) v[0] = edge[tid - 1];
        else if (a.state != nullptr) v[0] = make_float2(a.state[2 * j], a.state[2 * j + 1]);
        else v[0] = make_float2(0.0f, 0.0f);
        v[1] = res;
        float y[1];
        fm_phase_voted<1>(v, y);
        *dst = y[0];
        if (a.final_ != nullptr && out0 + tid == a.count - 1) {
            a.final_[2 * j] = res.x;
            a.final_[2 * j + 1] = res.y;
        }
    } else {
        if (tid < nout) *dst = am_magnitude(res.x, res.y);
    }
}

}  // namespace

int narrow_tile_count(int form, int count)
{
    const int adv = narrow_tile_advance(form);
    if (form == NARROW_FM) return count <= NT ? 1 : (int)(((int64_t)count - 1 + adv - 1) / adv);
    return (int)(((int64_t)count + adv - 1) / adv);
}

bool narrow_rows_fits(const Geom& g, ComplexOrder corder, int channels, const float* d_in, int64_t in_stride)
{
    if (corder != CO_L4 || g.I != 1 || g.count <= 0 || channels < 1 || channels > kTunerBankMaxChannels) return false;
    if (g.D < 1 || g.D > kNarrowMaxFactor || g.Lp < 4 || g.Lp > kNarrowMaxTaps || (g.Lp & 3) != 0) return false;
    if (g.seamBI != 0 && (g.seamBI < g.Lp || g.seamBI >= ((int64_t)1 << 30))) return false;
    if (g.k_begin < 0 || g.k_begin * g.D < g.in_base) return false;
    // 16-byte loads: aligned rows
    if ((reinterpret_cast<uintptr_t>(d_in) & 15) != 0 || (in_stride & 3) != 0) return false;
    return true;
}

bool launch_narrow_rows(hipStream_t s, const Geom& g, int form, ComplexOrder corder, const float* d_plain_taps, const float* d_in,
                        int64_t in_stride, int64_t n_in, float* d_out, int64_t out_stride, int channels, const float* d_state, float* d_final)
{
    if (form != NARROW_ENV && form != NARROW_FM) return false;
    if (!narrow_rows_fits(g, corder, channels, d_in, in_stride)) return false;
    if (d_plain_taps == nullptr || d_out == nullptr || (reinterpret_cast<uintptr_t>(d_out) & 3) != 0) return false;
    if (channels > 1 && (out_stride < g.count || in_stride < 2 * n_in)) return false;
    // every window of the launch lies in the readable part of its row
    if (n_in < (g.k_begin + g.count - 1) * g.D - g.in_base + g.Lp) return false;
    NarrowArgs a = {};
    a.in = d_in;
    a.in_stride = in_stride;
    a.x0 = g.k_begin * g.D - g.in_base;
    a.n_in = n_in;
    a.out = d_out;
    a.out_stride = out_stride;
    a.taps = d_plain_taps;
    a.state = form == NARROW_FM ? d_state : nullptr;
    a.final_ = form == NARROW_FM ? d_final : nullptr;
    a.count = g.count;
    a.channels = channels;
    a.D = g.D;
    a.Lp = g.Lp;
    a.seam = (int)g.seamBI;
    a.r0 = g.seamBI > 0 ? (int)((g.k_begin * g.D) % g.seamBI) : 0;
    const unsigned grid = (unsigned)narrow_tile_count(form, g.count) * (unsigned)channels;      // at most 2^23 + 1 tiles x 32 channels
    if (form == NARROW_FM) hipLaunchKernelGGL(k_narrow_rows<NARROW_FM>, dim3(grid), dim3(NT), 0, s, a);
    else hipLaunchKernelGGL(k_narrow_rows<NARROW_ENV>, dim3(grid), dim3(NT), 0, s, a);
    g_narrow_bank_launches.fetch_add(1, std::memory_order_relaxed);
    return true;
}

}  // namespace sdrhip
