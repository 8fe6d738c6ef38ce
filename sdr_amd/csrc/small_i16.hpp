// small_i16.hpp -- 16-bit signed IQ in front of the tuned one-kernel FM chain (kernels_small.hip, the receiver bank's int16 launch):
// the staging of one tile whose BOTH ends may lie outside the launch's input.  Stage::load (decimate_tile.hpp) cuts a tile at its far
// end only -- the tuner's tiles start at the first window -- while the chain's first tile starts one decimator output before the
// first y, before sample 0 at the stream's start, and its last tile runs past the receptive field.  The raw vectors land in the int16
// Stage's register layout, so tuner_store (tuner_mix.hpp: convert, then mix) takes them as they are.
#pragma once
#include "tuner_mix.hpp"

namespace sdrhip {
namespace {

// Samples [rel0, rel0 + T::SPAN) relative to in[0], rel0 a multiple of 4 and `in` 16-byte aligned (the launcher's fit predicate), of
// an input of n_in samples.  Interior tiles: unconditional 16-byte loads, all in flight before the first wait.  Ragged tiles: whole
// vectors where all 4 samples exist, else sample by sample (one 32-bit word each); samples outside [0, n_in) read as int16 0 = +0.0f.
// No byte outside [in, in + 4 n_in) is read.
template <class T, int NT>
__device__ __forceinline__ void small_load_i16(Stage<T, IN_I16, NT>& st, const void* __restrict__ in, int64_t rel0, int64_t n_in)
{
    using St = Stage<T, IN_I16, NT>;
    auto& r = st.r;
    constexpr int SPV = St::SPV, NV = St::NV, PER = St::PER;
    const int tid = threadIdx.x;
    const bool interior = rel0 >= 0 && rel0 + T::SPAN <= n_in;
    if (interior) {
        const char* src = reinterpret_cast<const char*>(in) + 4 * rel0;
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int v = tid + i * NT;
            if (i + 1 < PER || v < NV) r[i] = *reinterpret_cast<const uint4*>(src + 16 * (int64_t)v);
        }
        return;
    }
    const uint32_t* words = reinterpret_cast<const uint32_t*>(in);       // one word = one sample
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int v = tid + i * NT;
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (v < NV) {
            const int64_t r4 = rel0 + SPV * (int64_t)v;
            if (r4 >= 0 && r4 + SPV <= n_in) {
                const uint4 q = *reinterpret_cast<const uint4*>(words + r4);
                w[0] = q.x; w[1] = q.y; w[2] = q.z; w[3] = q.w;
            } else {
#pragma unroll
                for (int e = 0; e < SPV; e++) {
                    const int64_t sidx = r4 + e;
                    if (sidx >= 0 && sidx < n_in) w[e] = words[sidx];
                }
            }
        }
        r[i] = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

}  // namespace
}  // namespace sdrhip
