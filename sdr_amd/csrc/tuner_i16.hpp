// tuner_i16.hpp -- 16-bit signed IQ (the BladeRF's samples, convert.c:52-85) in front of the tuner family's tile kernel: the staging
// of one tile and the mixing store, the int16 siblings of Stage (decimate_tile.hpp) and tuner_store (tuner_mix.hpp).  Convert FIRST
// ((float)s * 2^-11, exact in f32 over the whole int16 range, 0 -> +0), then tuner_mul, then the taps: the mix rounds on the converted
// sample, and with subnormal table entries a product that underflows does not commute with the power of two, so the 2^-11 moves
// neither into the taps nor into the table.
#pragma once
#include "decimate_tile.hpp"
#include "tuner_mix.hpp"

namespace sdrhip {
namespace {

// convertCBladeRF: s / 2048
__device__ __forceinline__ float2 tuner_i16(int re, int im)
{
    return make_float2((float)re * (1.0f / 2048.0f), (float)im * (1.0f / 2048.0f));
}
// one 32-bit word = one sample, I in the low half: sign-extended in plain C++
__device__ __forceinline__ float2 tuner_i16_word(uint32_t w)
{
    return tuner_i16((int)(int16_t)(w & 0xffff), (int32_t)w >> 16);
}

// Staging of one tile of int16 IQ: Stage's two loaders with 4 samples per 16-byte vector.  T::SPAN is a multiple of 4 for every shape
// the fit predicate admits (D and P multiples of 4), so the whole-tile loader reads exactly SPAN samples.
template <class T, int NT>
struct StageI16 {
    static constexpr int SPV = 4;                                // samples per 16-byte vector
    static constexpr int NV = (T::SPAN + SPV - 1) / SPV;         // vectors per tile
    static constexpr int PER = (NV + NT - 1) / NT;               // vectors per thread
    static_assert(T::SPAN % SPV == 0, "a whole tile is whole vectors: no read past the tile's last sample");
    uint4 r[PER];

    __device__ __forceinline__ void load(const void* __restrict__ src_v, int64_t sample0, int avail)
    {
        const char* src = reinterpret_cast<const char*>(src_v) + 4 * sample0;
        if (avail >= T::SPAN) {
            // every tile but the last: unconditional 16-byte loads, all in flight together
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const int v = threadIdx.x + i * NT;
                if (i + 1 < PER || v < NV) r[i] = *reinterpret_cast<const uint4*>(src + 16 * (int64_t)v);
            }
            return;
        }
        // ragged end of the stream (one workgroup per launch and channel): element-wise, zero-filled (int16 0 == +0.0f)
#pragma unroll 1
        for (int i = 0; i < PER; i++) {
            const int v = threadIdx.x + i * NT;
            const int s = v * SPV;
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            if (v < NV) {
                const uint16_t* h = reinterpret_cast<const uint16_t*>(src) + 8 * (int64_t)v;
                for (int e = 0; e < 8; e++)
                    if (s + e / 2 < avail) w[e >> 1] |= (uint32_t)h[e] << (16 * (e & 1));
            }
            // PER is small and compile-time: a select chain keeps r[] in registers
#pragma unroll
            for (int q = 0; q < PER; q++)
                if (q == i) r[q] = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
};

// The raw vectors of StageI16::load -> mixed samples in the padded LDS layout.  ph = phase of the thread's first sample.
template <class T, int NT>
__device__ __forceinline__ void tuner_store_i16(const uint4 (&r)[StageI16<T, NT>::PER], float2* __restrict__ lds,
                                                const float2* __restrict__ osc, uint32_t n, uint32_t ph)
{
    using St = StageI16<T, NT>;
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
        for (int k = 0; k < 2; k++) {
            const float2 m0 = tuner_mul(tuner_i16_word(w[2 * k]), o[i][2 * k]);
            const float2 m1 = tuner_mul(tuner_i16_word(w[2 * k + 1]), o[i][2 * k + 1]);
            const int ss = s + 2 * k;
            if (ss < T::SPAN + 1) *reinterpret_cast<float4*>(&lds[T::lds_idx(ss)]) = make_float4(m0.x, m0.y, m1.x, m1.y);
        }
    }
}

}  // namespace
}  // namespace sdrhip
