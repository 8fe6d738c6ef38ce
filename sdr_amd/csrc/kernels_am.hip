// kernels_am.hip -- amDemod: the AM receiver's envelope detector, `P.map (VG.map magnitude)` of the reference's Readme.
//
//     out[i] = magnitude (in[2i] :+ in[2i+1])
//
// `magnitude` is GHC base's Data.Complex.magnitude at Float, the function agc steps with (kernels_agc.hip: agc_magnitude, restated
// as am_magnitude in am.hpp so that file's code stays as it is): scale both parts by 2^-k, k the larger frexp exponent, square, add,
// sqrt, scale back.  Not sqrtf(re*re + im*im) and not hypotf: they differ where a square under- or overflows, and a correctly rounded hypot
// differs on about one ordinary sample in six.  The build's -ffp-contract=off keeps a*a + b*b unfused.
//
// Non-finite input: frexpf's exponent of Inf and NaN is 0 on the device (v_frexp_exp_i32_f32) as in the model, so k is the finite
// part's exponent; ldexpf (v_ldexp_f32) passes Inf and NaN through, the finite part is scaled to below 1, and the sum is +Inf or
// NaN: a NaN part gives NaN, otherwise an infinite part gives +Inf.
//
// Nothing is carried from sample to sample, so there is one kernel: a thread takes four samples (32 bytes in, 16 bytes out) per
// step, the row is blockIdx.y, and the one-row call is rows == 1 of it.
#include <atomic>

#include "am.hpp"

namespace sdrhip {

// am_magnitude (Data.Complex.magnitude at Float): am.hpp, shared with the envelope form of the tuner bank's kernels.

// LA / SA = access width the row starts allow on the load / store side: 2 = 16-byte, 1 = 8-byte, 0 = 4-byte (any float pointer).
// Quad q of a row is its input floats [8q, 8q + 8) and output floats [4q, 4q + 4): a multiple of 16 bytes from the row start on
// both sides, so the row start's alignment is the access's.  Quads exist for q < n / 4 only, the n % 4 samples behind them go
// element-wise: no float outside the row's [0, 2n) is read and none outside its [0, n) written.
template <int LA, int SA>
__global__ void __launch_bounds__(256) k_am_demod_rows(const float* __restrict__ in, int64_t in_stride, float* __restrict__ out,
                                                        int64_t out_stride, int64_t n)
{
    const int64_t row = blockIdx.y;
    in += row * in_stride;
    out += row * out_stride;
    const int64_t nquad = n >> 2;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nquad; q += stride) {
        const float* p = in + 8 * q;
        float4 v0, v1;   // both loads are issued before the first use
        if (LA == 2) {
            v0 = reinterpret_cast<const float4*>(p)[0];
            v1 = reinterpret_cast<const float4*>(p)[1];
        } else if (LA == 1) {
            const float2 a = reinterpret_cast<const float2*>(p)[0], b = reinterpret_cast<const float2*>(p)[1];
            const float2 c = reinterpret_cast<const float2*>(p)[2], d = reinterpret_cast<const float2*>(p)[3];
            v0 = make_float4(a.x, a.y, b.x, b.y);
            v1 = make_float4(c.x, c.y, d.x, d.y);
        } else {
            v0 = make_float4(p[0], p[1], p[2], p[3]);
            v1 = make_float4(p[4], p[5], p[6], p[7]);
        }
        const float4 r = make_float4(am_magnitude(v0.x, v0.y), am_magnitude(v0.z, v0.w), am_magnitude(v1.x, v1.y),
                                     am_magnitude(v1.z, v1.w));
        float* w = out + 4 * q;
        if (SA == 2) {
            *reinterpret_cast<float4*>(w) = r;
        } else if (SA == 1) {
            reinterpret_cast<float2*>(w)[0] = make_float2(r.x, r.y);
            reinterpret_cast<float2*>(w)[1] = make_float2(r.z, r.w);
        } else {
            w[0] = r.x; w[1] = r.y; w[2] = r.z; w[3] = r.w;
        }
    }
    // the ragged end (< 4 samples)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = (nquad << 2) + threadIdx.x;
        out[i] = am_magnitude(in[2 * i], in[2 * i + 1]);
    }
}

namespace {
std::atomic<long long> g_am_launches{0};

int access_of(uintptr_t bits) { return (bits & 15) == 0 ? 2 : (bits & 7) == 0 ? 1 : 0; }

template <int LA>
void launch_la(int sa, dim3 grid, hipStream_t s, const float* in, int64_t in_stride, float* out, int64_t out_stride, int64_t n)
{
    if (sa == 2) hipLaunchKernelGGL((k_am_demod_rows<LA, 2>), grid, dim3(256), 0, s, in, in_stride, out, out_stride, n);
    else if (sa == 1) hipLaunchKernelGGL((k_am_demod_rows<LA, 1>), grid, dim3(256), 0, s, in, in_stride, out, out_stride, n);
    else hipLaunchKernelGGL((k_am_demod_rows<LA, 0>), grid, dim3(256), 0, s, in, in_stride, out, out_stride, n);
}
}  // namespace

long long am_demod_launch_count() { return g_am_launches.load(); }

void launch_am_demod_rows(hipStream_t s, int rows, const float* d_in_iq, int64_t in_stride, float* d_out, int64_t out_stride,
                          int64_t n)
{
    if (n <= 0 || rows < 1) return;
    if (rows == 1) in_stride = out_stride = 0;
    // row r starts at base + r * stride: one width for all rows, the two sides independently
    const int la = access_of((uintptr_t)d_in_iq | ((uintptr_t)in_stride << 2));
    const int sa = access_of((uintptr_t)d_out | ((uintptr_t)out_stride << 2));
    // the workgroups loop over the row's quads, so any rows x n is one launch; 256 * 64 workgroups shared among the rows (as
    // fmDemod's row form) keep every compute unit busy and the grid small
    int64_t blocks = ((n >> 2) + 255) / 256;
    int64_t cap = 256 * 64 / rows;
    if (cap < 1) cap = 1;
    if (blocks > cap) blocks = cap;
    if (blocks < 1) blocks = 1;
    const dim3 grid((unsigned)blocks, (unsigned)rows);
    if (la == 2) launch_la<2>(sa, grid, s, d_in_iq, in_stride, d_out, out_stride, n);
    else if (la == 1) launch_la<1>(sa, grid, s, d_in_iq, in_stride, d_out, out_stride, n);
    else launch_la<0>(sa, grid, s, d_in_iq, in_stride, d_out, out_stride, n);
    g_am_launches.fetch_add(1);
}

}  // namespace sdrhip
