// tail_plan.hpp -- the receptive-field arithmetic of the low-rate tail (firResampler -> firFilter), in y samples, stated once:
// the FM chain's plan functions (chain.cpp) put fmDemod and the decimator in front of it, the rows tail (audio_tail.cpp) uses it as it is.
#pragma once
#include "descriptors.hpp"

namespace sdrhip {

// the first y index audio output q reads
inline int64_t tail_first_y(const ResampDesc& r, int64_t q) { return r.in_offset(q); }
// one past the last y index audio output q reads: its last z window, and the nloop floats the One kernel walks there (the Cross
// kernel at most ceil(ntaps / I) <= nloop)
inline int64_t tail_end_y(const ResampDesc& r, const FirDesc& a, int64_t q) { return r.in_offset(q + a.Lp - 1) + r.nloop; }

// the number of outputs q whose end(q) <= n, for a non-decreasing end()
template <class End>
inline int64_t ready_by_end(End&& end, int64_t n)
{
    if (end(0) > n) return 0;
    int64_t lo = 0, hi = 1;                        // invariant: end(lo) <= n < end(hi)
    while (end(hi) <= n) { lo = hi; hi *= 2; }
    while (lo + 1 < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (end(mid) <= n) lo = mid; else hi = mid;
    }
    return hi;
}

// the longest receptive field of any output: the geometry repeats with the resampler's cycle of I outputs
template <class Start, class End>
inline int64_t longest_field(Start&& start, End&& end, int I)
{
    int64_t worst = 0;
    for (int64_t q = 0; q <= 2 * I + 2; q++) {
        const int64_t len = end(q) - start(q);
        if (len > worst) worst = len;
    }
    return worst;
}

}  // namespace sdrhip
