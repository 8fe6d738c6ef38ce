// spectrum.hpp -- launchers of kernels_spectrum.hip (internal header; the host side is fft.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrhip {

// what the kernels need to know about one sdrhip_spectrum_run_device call
struct SpectrumArgs {
    const void* in;         // raw IQ: interleaved u8 (format 0) or float32 (format 1)
    int format;
    int64_t hop;            // samples between row starts
    int64_t rows;
    int n;
    int shift;              // 1: multiply sample j by (-1)^j
    double scale;
    const double* window;   // n doubles, device
    const double2* twiddle; // exp(-2 pi i m / n), m in [0, n), device (one-kernel route only)
};

// sizes the one-kernel route serves: powers of two from 64 to 8192
inline bool spectrum_fused_size(int n) { return n >= 64 && n <= 8192 && (n & (n - 1)) == 0; }

// one launch: raw IQ -> rows x n float32 magnitudes, the transform resident in LDS
hipError_t launch_spectrum_fused(hipStream_t stream, const SpectrumArgs& a, float* out);
// hipFFT route, rows [row0, row0 + nrows): raw IQ -> complex doubles, and complex doubles -> float32 magnitudes
hipError_t launch_spectrum_prepare(hipStream_t stream, const SpectrumArgs& a, int64_t row0, int64_t nrows, double2* work);
hipError_t launch_spectrum_magnitude(hipStream_t stream, const double2* work, int64_t count, double scale, float* out);

}  // namespace sdrhip
