// am.hpp -- amDemod, the AM receiver's envelope detector `P.map (VG.map magnitude)`: launcher of kernels_am.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrhip {

// Row r: n interleaved complex samples at d_in_iq + r * in_stride -> n floats at d_out + r * out_stride (strides in floats, unused
// with rows == 1).  One launch for any rows >= 1 and n > 0; n <= 0 launches nothing.
void launch_am_demod_rows(hipStream_t s, int rows, const float* d_in_iq, int64_t in_stride, float* d_out, int64_t out_stride,
                          int64_t n);
long long am_demod_launch_count();   // diagnostics: kernel launches so far

// Data.Complex.magnitude at Float: exponent 0 = 0, otherwise frexp's exponent (denormals normalised); scaleFloat = ldexpf with one
// rounding; sqrtf is correctly rounded (hipcc's default).  One copy for kernels_am.hip and the envelope form of the tuner bank's
// kernels (kernels_tuner_bank.hip); kernels_agc.hip keeps its own.
__device__ __forceinline__ float am_magnitude(float re, float im)
{
    int er, ei;
    (void)frexpf(re, &er);
    (void)frexpf(im, &ei);
    const int k = er > ei ? er : ei;
    const float a = ldexpf(re, -k), b = ldexpf(im, -k);
    return ldexpf(sqrtf(a * a + b * b), k);
}

}  // namespace sdrhip
