// kernels_crossfix.hip -- the generic "Cross" (seam) fix-up kernels and their two host launchers.
//
// One thread per candidate slot of a seam (SeamSpan, kernels.hpp: nseams * per of them), any D / Lp / I, every sample read from
// global memory: what a launcher's tier table ends in when no LDS-staged fix-up fits the shape (crossfix.hpp, decimate_tile.hpp,
// the filters' own next to their kernels).  The sequential order of the reference's Haskell fallbacks (FilterInternal.hs:397-423).
#include "kernels.hpp"

namespace sdrhip {
namespace {

// Cross outputs of a complex filter / decimator: sequential over the Lp plain taps
// (filterCrossHighLevel with Mult (Complex a) a, FilterInternal.hs:397-408, Util.hs:87-88).
template <bool U8 = false>
__global__ void __launch_bounds__(256) k_fir_cplx_crossfix(Geom g, const float* __restrict__ xtaps,
                                                            const void* __restrict__ in, float* __restrict__ out,
                                                            int64_t first_seam, int nseams, int per_seam)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseams * per_seam) return;
    const int si = t / per_seam, ci = t - si * per_seam;
    const int64_t edge = (first_seam + si) * g.seamBI;
    const int64_t m = (edge + g.D - 1) / g.D - 1 - ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    float re = 0.0f, im = 0.0f;
    if constexpr (U8) {   // interleaved u8 IQ: convert.c's (u - 128) / 128 on the way in (exact)
        const uchar2* x = reinterpret_cast<const uchar2*>(in) + (v - g.in_base);
        for (int j = 0; j < g.Lp; j++) {
            const uchar2 u = x[j];
            re = re + (((float)u.x - 128.0f) * (1.0f / 128.0f)) * xtaps[j];
            im = im + (((float)u.y - 128.0f) * (1.0f / 128.0f)) * xtaps[j];
        }
    } else {
        const float2* x = reinterpret_cast<const float2*>(in) + (v - g.in_base);
        for (int j = 0; j < g.Lp; j++) {
            const float2 s = x[j];
            re = re + s.x * xtaps[j];
            im = im + s.y * xtaps[j];
        }
    }
    *reinterpret_cast<float2*>(out + 2 * (m - g.k_begin)) = make_float2(re, im);
}

// Cross outputs of a real FIR / decimator: sequential over the Lp plain taps
// (filterCrossHighLevel / decimateCrossHighLevel, FilterInternal.hs:397-408).
__global__ void __launch_bounds__(256) k_fir_real_crossfix(Geom g, const float* __restrict__ xtaps,
                                                            const float* __restrict__ in, float* __restrict__ out,
                                                            int64_t first_seam, int nseams, int per_seam, float gain,
                                                            int apply_gain)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseams * per_seam) return;
    const int si = t / per_seam, ci = t - si * per_seam;
    const int64_t edge = (first_seam + si) * g.seamBI;
    const int64_t m = (edge + g.D - 1) / g.D - 1 - ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    const float* x = in + (v - g.in_base);
    float r = 0.0f;
    for (int j = 0; j < g.Lp; j++) r = r + x[j] * xtaps[j];
    if (apply_gain) r = r * gain;
    out[m - g.k_begin] = r;
}

// Cross outputs of a resampler, real or complex data (resampleCrossHighLevel, FilterInternal.hs:410-423):
// taps = stride I (drop filterOffset coeffs) over the UNPADDED taps, sequential.
template <bool CPLX>
__global__ void __launch_bounds__(256) k_resample_crossfix(Geom g, const float* __restrict__ plain, int ntaps,
                                                            const float* __restrict__ in, float* __restrict__ out,
                                                            int64_t first_seam, int nseams, int per_seam)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nseams * per_seam) return;
    const int si = t / per_seam, ci = t - si * per_seam;
    const int64_t edge = (first_seam + si) * g.seamBI;           // upsampled units
    const int64_t m = (edge + g.D - 1) / g.D - 1 - ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    if (!seam_has_crossover(edge, g.I, g.D, g.Lp)) return;       // the Pipe goes straight to the next buffer here
    if (late_output_is_one(m, edge, g.I, g.D, g.outB)) return;   // first output of an output block, first input beyond the seam
    const int64_t pos = (v + g.I - 1) / g.I;                     // inOff(m)
    const int fo = (int)(pos * g.I - v);
    if constexpr (CPLX) {
        const float2* x = reinterpret_cast<const float2*>(in) + (pos - g.in_base);
        float re = 0.0f, im = 0.0f;
        for (int l = 0, j = fo; j < ntaps; l++, j += g.I) {
            const float2 sv = x[l];
            re = re + sv.x * plain[j];
            im = im + sv.y * plain[j];
        }
        *reinterpret_cast<float2*>(out + 2 * (m - g.k_begin)) = make_float2(re, im);
    } else {
        const float* x = in + (pos - g.in_base);
        float r = 0.0f;
        for (int l = 0, j = fo; j < ntaps; l++, j += g.I) r = r + x[l] * plain[j];
        out[m - g.k_begin] = r;
    }
}

inline dim3 slot_grid(const SeamSpan& sp) { return dim3((unsigned)(((int64_t)sp.nseams * sp.per + 255) / 256)); }

}  // namespace

void launch_fir_crossfix(hipStream_t s, const Geom& g, const SeamSpan& sp, bool cplx, bool in_is_u8, const float* d_cross_taps,
                         const void* d_in, float* d_out, float gain, bool apply_gain)
{
    if (sp.nseams <= 0) return;
    const dim3 grid = slot_grid(sp), block(256);
    if (!cplx)
        hipLaunchKernelGGL(k_fir_real_crossfix, grid, block, 0, s, g, d_cross_taps, (const float*)d_in, d_out, sp.first, sp.nseams, sp.per, gain,
                           apply_gain ? 1 : 0);
    else if (in_is_u8) hipLaunchKernelGGL(k_fir_cplx_crossfix<true>, grid, block, 0, s, g, d_cross_taps, d_in, d_out, sp.first, sp.nseams, sp.per);
    else hipLaunchKernelGGL(k_fir_cplx_crossfix<false>, grid, block, 0, s, g, d_cross_taps, d_in, d_out, sp.first, sp.nseams, sp.per);
}

void launch_resample_crossfix(hipStream_t s, const Geom& g, const SeamSpan& sp, bool cplx, const float* d_plain_taps, int ntaps,
                              const float* d_in, float* d_out)
{
    if (sp.nseams <= 0) return;
    const dim3 grid = slot_grid(sp), block(256);
    if (cplx) hipLaunchKernelGGL(k_resample_crossfix<true>, grid, block, 0, s, g, d_plain_taps, ntaps, d_in, d_out, sp.first, sp.nseams, sp.per);
    else hipLaunchKernelGGL(k_resample_crossfix<false>, grid, block, 0, s, g, d_plain_taps, ntaps, d_in, d_out, sp.first, sp.nseams, sp.per);
}

}  // namespace sdrhip
