// tuner_mix.hpp -- the oscillator mix as device functions, shared by the tuner's kernels (kernels_tuner.hip, kernels_tuner_bank.hip)
// and the tuned one-kernel FM chain (kernels_small.hip): convert, multiply (Data.Complex's (*) at Float: four products and two sums,
// each rounded, no shortcut for entries that are 0 or +-1) and the loader that puts a tile's mixed samples into the padded LDS
// layout, for every input format (FMT: InFmt, kernels.hpp).
// Convert FIRST, then tuner_mul, then the taps, for u8 and int16 alike: the mix rounds on the converted sample, and with subnormal
// table entries a product that underflows does not commute with a power of two, so neither the 1/128 nor the 2^-11 moves into the
// taps or into the table.  u8 therefore keeps the full (u - 128) * (1/128) here, unlike the decimator's own loader (Stage::store_regs).
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
// convertCBladeRF (convert.c:52-85): s / 2048, exact in f32 over the whole int16 range, 0 -> +0
__device__ __forceinline__ float2 tuner_i16(int re, int im)
{
    return make_float2((float)re * (1.0f / 2048.0f), (float)im * (1.0f / 2048.0f));
}
// one 32-bit word = one sample, I in the low half: sign-extended in plain C++
__device__ __forceinline__ float2 tuner_i16_word(uint32_t w)
{
    return tuner_i16((int)(int16_t)(w & 0xffff), (int32_t)w >> 16);
}
__device__ __forceinline__ uint32_t wrap_inc(uint32_t p, uint32_t n) { return p + 1 == n ? 0u : p + 1; }

// sample i of `in`, converted: what the sequential-order kernels and the two-pass route's first pass read one at a time
template <int FMT>
__device__ __forceinline__ float2 tuner_sample(const void* __restrict__ in, int64_t i)
{
    if constexpr (FMT == IN_U8) {
        const uchar2 u = reinterpret_cast<const uchar2*>(in)[i];
        return tuner_u8(u.x, u.y);
    } else if constexpr (FMT == IN_I16) {
        const short2 u = reinterpret_cast<const short2*>(in)[i];
        return tuner_i16(u.x, u.y);
    } else {
        return reinterpret_cast<const float2*>(in)[i];
    }
}

// samples 2k and 2k + 1 of a raw 16-byte vector, converted: cfloat has the one pair, int16 two (a word each), u8 four (word k)
template <int FMT>
__device__ __forceinline__ void tuner_pair(const uint32_t (&w)[4], int k, float2& x0, float2& x1)
{
    if constexpr (FMT == IN_U8) {
        x0 = tuner_u8(w[k] & 0xff, (w[k] >> 8) & 0xff);
        x1 = tuner_u8((w[k] >> 16) & 0xff, w[k] >> 24);
    } else if constexpr (FMT == IN_I16) {
        x0 = tuner_i16_word(w[2 * k]);
        x1 = tuner_i16_word(w[2 * k + 1]);
    } else {
        x0 = make_float2(__uint_as_float(w[0]), __uint_as_float(w[1]));
        x1 = make_float2(__uint_as_float(w[2]), __uint_as_float(w[3]));
    }
}

// The raw vectors of Stage::load -> mixed samples in the padded LDS layout.  ph = phase of the thread's first sample.
template <class T, int FMT, int NT>
__device__ __forceinline__ void tuner_store(const uint4 (&r)[Stage<T, FMT, NT>::PER], float2* __restrict__ lds,
                                            const float2* __restrict__ osc, uint32_t n, uint32_t ph)
{
    using St = Stage<T, FMT, NT>;
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
        const uint32_t w[4] = {r[i].x, r[i].y, r[i].z, r[i].w};
#pragma unroll
        for (int k = 0; k < SPV / 2; k++) {
            float2 x0, x1;
            tuner_pair<FMT>(w, k, x0, x1);
            const float2 m0 = tuner_mul(x0, o[i][2 * k]);
            const float2 m1 = tuner_mul(x1, o[i][2 * k + 1]);
            const int ss = s + 2 * k;
            // (a cfloat vector IS one pair, and v < NV has placed it inside the tile)
            if (SPV == 2 || ss < T::SPAN + 1) *reinterpret_cast<float4*>(&lds[T::lds_idx(ss)]) = make_float4(m0.x, m0.y, m1.x, m1.y);
        }
    }
}

}  // namespace
}  // namespace sdrhip
