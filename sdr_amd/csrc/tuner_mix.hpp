// tuner_mix.hpp -- the oscillator mix as device functions, shared by the tuner's kernels (kernels_tuner.hip) and the tuned
// one-kernel FM chain (kernels_small.hip): convert, multiply (Data.Complex's (*) at Float: four products and two sums, each
// rounded, no shortcut for entries that are 0 or +-1) and the loader that puts a tile's mixed samples into the padded LDS layout.
#pragma once
#include "decimate_tile.hpp"

namespace sdrhip {
namespace {

__device__ __forceinline__ float2 tuner_mul(const float2 x, const float2 o)
{
    return make_float2(x.x * o.x - x.y * o.y, x.x * o.y + x.y * o.x);
}
// convert.c: (u - 128) / 128, both steps exact in f32
__device__ __forceinline__ float2 tuner_u8(uint32_t re, uint32_t im)
{
    return make_float2(((float)re - 128.0f) * (1.0f / 128.0f), ((float)im - 128.0f) * (1.0f / 128.0f));
}
__device__ __forceinline__ uint32_t wrap_inc(uint32_t p, uint32_t n) { return p + 1 == n ? 0u : p + 1; }

// The raw vectors of Stage::load -> mixed samples in the padded LDS layout.  ph = phase of the thread's first sample.
template <class T, bool U8, int NT>
__device__ __forceinline__ void tuner_store(const uint4 (&r)[Stage<T, U8, NT>::PER], float2* __restrict__ lds,
                                            const float2* __restrict__ osc, uint32_t n, uint32_t ph)
{
    using St = Stage<T, U8, NT>;
    constexpr int SPV = St::SPV, NV = St::NV, PER = St::PER;
    const uint32_t step = (uint32_t)(NT * SPV) % n;       // between a thread's consecutive vectors
    // every oscillator load of the thread in flight before the first use (they hit L2; the raw loads are already out)
    float2 o[PER][SPV];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        uint32_t p = ph;
#pragma unroll
        for (int k = 0; k < SPV; k++) {
            o[i][k] = osc[p];
            p = wrap_inc(p, n);
        }
        ph += step;
        if (ph >= n) ph -= n;
    }
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int v = threadIdx.x + i * NT;
        const int s = v * SPV;
        if (v >= NV) continue;
        if constexpr (!U8) {
            const float2 m0 = tuner_mul(make_float2(__uint_as_float(r[i].x), __uint_as_float(r[i].y)), o[i][0]);
            const float2 m1 = tuner_mul(make_float2(__uint_as_float(r[i].z), __uint_as_float(r[i].w)), o[i][1]);
            *reinterpret_cast<float4*>(&lds[T::lds_idx(s)]) = make_float4(m0.x, m0.y, m1.x, m1.y);
        } else {
            const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const float2 m0 = tuner_mul(tuner_u8(w[k] & 0xff, (w[k] >> 8) & 0xff), o[i][2 * k]);
                const float2 m1 = tuner_mul(tuner_u8((w[k] >> 16) & 0xff, w[k] >> 24), o[i][2 * k + 1]);
                const int ss = s + 2 * k;
                if (ss < T::SPAN + 1) *reinterpret_cast<float4*>(&lds[T::lds_idx(ss)]) = make_float4(m0.x, m0.y, m1.x, m1.y);
            }
        }
    }
}

}  // namespace
}  // namespace sdrhip
