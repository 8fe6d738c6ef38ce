// spectrum.hpp -- launchers of kernels_spectrum.hip (internal header; the host side is fft.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrhip {

// what the kernels need to know about one sdrhip_spectrum_run_device call
struct SpectrumArgs {
    const void* in;         // raw IQ: interleaved u8 (format 0), float32 (format 1) or int16 (format 2)
    int format;
    int64_t hop;            // samples between row starts
    int64_t rows;
    int n;
    int shift;              // 1: multiply sample j by (-1)^j
    double scale;
    const double* window;   // n doubles, device
    const double2* twiddle; // exp(-2 pi i m / n), m in [0, n), device (one-kernel route only)
};

// what the reducing form adds (sdrhip_spectrum_reduce_run_device): SpectrumArgs::rows then counts OUTPUT rows, each made of `group`
// consecutive input rows
struct SpectrumReduce {
    int group;
    int reduce;             // SDRHIP_REDUCE_*
    int unit;               // SDRHIP_UNIT_*
    double floor_db;
};

// rows per chunk of the defined summation order (include/sdr_hip.h): part of the definition, not a tuning knob
constexpr int SPECTRUM_REDUCE_CHUNK = 32;

// sizes the one-kernel route serves: powers of two from 64 to 8192
inline bool spectrum_fused_size(int n) { return n >= 64 && n <= 8192 && (n & (n - 1)) == 0; }

// one launch: raw IQ -> rows x n float32 magnitudes, the transform resident in LDS
hipError_t launch_spectrum_fused(hipStream_t stream, const SpectrumArgs& a, float* out);
// hipFFT route, rows [row0, row0 + nrows): raw IQ -> complex doubles, and complex doubles -> float32 magnitudes
hipError_t launch_spectrum_prepare(hipStream_t stream, const SpectrumArgs& a, int64_t row0, int64_t nrows, double2* work);
hipError_t launch_spectrum_magnitude(hipStream_t stream, const double2* work, int64_t count, double scale, float* out);

// the reducing form of the one-kernel route over chunks [chunk0, chunk1) of every group.  partial == nullptr (a group of one chunk
// only: chunk0 = 0, chunk1 = 1): one launch writes `out`.  Otherwise work items of `per_item` chunks each write every chunk's sums to
// layer (chunk - chunk0) of `partial` (layers of rows x n doubles) for launch_spectrum_reduce_finalise, and `out` is not touched.
hipError_t launch_spectrum_fused_reduce(hipStream_t stream, const SpectrumArgs& a, const SpectrumReduce& f, int chunk0, int chunk1, int per_item,
                                        double* partial, float* out);
// `layers` layers of `count` doubles, in ascending order, onto `total` (taken as 0.0 when `first`); `last` writes `out` instead
hipError_t launch_spectrum_reduce_finalise(hipStream_t stream, const double* partial, int layers, int64_t count, double* total, bool first, bool last,
                                           const SpectrumReduce& f, float* out);
// hipFFT route: transformed input rows [b0, b0 + nrows) (numbered from the first row of out's first output row) into chunk / total
// (output rows x n doubles each); a group's last row writes its output row
hipError_t launch_spectrum_accumulate(hipStream_t stream, const double2* work, int64_t b0, int64_t nrows, int n, double scale, const SpectrumReduce& f,
                                      double* chunk, double* total, float* out);

}  // namespace sdrhip

// what the waterfall Pipe (sdrhip_pipe_spectrum, pipes_spectrum.cpp) asks of the object it borrows (fft.cpp): its size, its SDRHIP_IQ_*
// format, and whether a reduce run of this group length goes through the object's one scratch buffer (the hipFFT route, or layers)
struct sdrhip_spectrum;
namespace sdrhip {
int spectrum_size_of(const sdrhip_spectrum* s);
int spectrum_format_of(const sdrhip_spectrum* s);
bool spectrum_reduce_uses_scratch(const sdrhip_spectrum* s, int group);
void spectrum_forget_stream(sdrhip_spectrum* s, hipStream_t stream);      // before `stream` is destroyed
}  // namespace sdrhip
