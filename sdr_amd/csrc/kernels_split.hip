// kernels_split.hip -- one LDS-tiled kernel for every FIR family that has no hand-specialised kernel
// (real decimators, complex decimators with any factor / tap count, rational resamplers with any
// I/D, real or complex, the SSE orders, the symmetric variants).
//
// The reference's SIMD kernels keep M partial sums per output -- partial l accumulates taps j = l, l+M, l+2M, ... in
// increasing j from +0 -- and fold them with a fixed tree (common.h:18-29,58-72,82-90,108-155).  Here those M partial
// sums are M LANES of a wavefront: lane (o, l) walks  acc = acc + h[M*i + l] * x[start_o + M*i + l]  for i = 0, 1, ..,
// so a wave works on 64/M outputs at a time and
//   * its LDS reads are runs of M consecutive samples per output: conflict-free for every decimation factor whose
//     runs do not wrap the 32 banks (all D <= 8; two-way at worst for the other usual ones),
//   * each lane's taps h[l], h[M+l], ... sit in registers for as long as the wave stays on one tap row,
//   * the tree is a butterfly over the M lanes (xor 1, 2, 4 for the RR / RC kernels; xor M/2 first for the "RC2" order,
//     whose partials are folded q_l = p_l + p_{l+M/2} before the tree, common.h:142-155).  Lane 0 always adds
//     (its own) + (the other's), so operand order is the reference's as well.
// A resampler is NC = numGroups interleaved decimators: outputs i = n*NC + c share tap row (group0 + c) % NC and start
// at pos0 + n*period + pre[c] (Filter.hs:613-641, resample.c:70-87), so a wave stays on one row for a whole run of n.
// One workgroup stages the input span of NN cycles once, computes its NN*NC outputs, and stores them coalesced from LDS.
// Seam straddlers ("Cross" outputs) are rewritten afterwards by the generic kernels of kernels_crossfix.hip.
#include <atomic>

#include "crossfix.hpp"
#include "split_tile.hpp"

namespace sdrhip {

namespace {

// the tile itself (arguments, staging, walk, fold, store) and plan_tile: split_tile.hpp, shared with kernels_fir_rows.hip
template <bool CPLX, int M, int ORD, bool SYM, int NCHMAX, int U, bool EXACT>
__global__ void __launch_bounds__(256) k_split(SplitArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    split_tile<CPLX, M, ORD, SYM, NCHMAX, U, EXACT>(a, a.in, a.out, blockIdx.x, smem_raw);
}

template <bool CPLX, int M, int ORD, bool SYM, int NCHMAX, int U, bool EXACT>
void launch_kernel(hipStream_t s, const SplitArgs& a, unsigned grid, size_t lds_bytes)
{
    auto kern = k_split<CPLX, M, ORD, SYM, NCHMAX, U, EXACT>;
    // per instantiation and device: tiles of large decimation factors exceed the 64 KiB default cap
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds_bytes, s, a);
}

template <bool CPLX, int M, int ORD, bool SYM, int U>
void launch_variant_u(hipStream_t s, const SplitArgs& a)
{
    const int64_t ncyc = ((int64_t)a.count + a.NC - 1) / a.NC;
    const unsigned grid = (unsigned)((ncyc + a.NN - 1) / a.NN);
    const size_t esz = CPLX ? 8 : 4;
    const size_t lds_bytes = ((size_t)((a.span + 7) & ~3) + (size_t)a.NN * a.NC) * esz;
    // Real data, exact tap-chunk counts of the usual filter lengths: guard-free code (measured +20 % on the 128-tap real
    // decimator; on complex data the scheduler hoists more reads than there are registers for and it is 2x slower).
    constexpr bool EX = U == SPLIT_U && !CPLX;
    if (EX && a.nch == 8) launch_kernel<CPLX, M, ORD, SYM, 8, U, EX>(s, a, grid, lds_bytes);
    else if (EX && a.nch == 16) launch_kernel<CPLX, M, ORD, SYM, 16, U, EX>(s, a, grid, lds_bytes);
    else if (EX && a.nch == 32) launch_kernel<CPLX, M, ORD, SYM, 32, U, EX>(s, a, grid, lds_bytes);
    else if (a.nch <= 8) launch_kernel<CPLX, M, ORD, SYM, 8, U, false>(s, a, grid, lds_bytes);
    else if (a.nch <= 16) launch_kernel<CPLX, M, ORD, SYM, 16, U, false>(s, a, grid, lds_bytes);
    else if (a.nch <= 32) launch_kernel<CPLX, M, ORD, SYM, 32, U, false>(s, a, grid, lds_bytes);
    else launch_kernel<CPLX, M, ORD, SYM, 64, U, false>(s, a, grid, lds_bytes);
}

template <bool CPLX, int M, int ORD, bool SYM>
void launch_variant(hipStream_t s, const SplitArgs& a, int U)
{
    if (U == SPLIT_U) launch_variant_u<CPLX, M, ORD, SYM, SPLIT_U>(s, a);
    else launch_variant_u<CPLX, M, ORD, SYM, 1>(s, a);
}

template <bool CPLX>
bool dispatch(hipStream_t s, SplitArgs& a, OrderInfo o, bool sym)
{
    if (a.nch < 1 || a.nch > 64) return false;   // the taps of a lane live in registers
    int U = 1;
    if (!plan_tile(a, o.M, CPLX, U)) return false;
    if constexpr (!CPLX) {
        if (o.M == 8) { if (sym) launch_variant<false, 8, 0, true>(s, a, U); else launch_variant<false, 8, 0, false>(s, a, U); }
        else { if (sym) launch_variant<false, 4, 0, true>(s, a, U); else launch_variant<false, 4, 0, false>(s, a, U); }
    } else {
        if (sym) return false;   // no descriptor builds the symmetric complex kernels (drop-in symbols only): generic path
        if (o.ord == 0) {
            if (o.M == 4) launch_variant<true, 4, 0, false>(s, a, U); else launch_variant<true, 2, 0, false>(s, a, U);
        } else if (o.M == 8) {
            launch_variant<true, 8, 1, false>(s, a, U);
        } else {
            launch_variant<true, 4, 1, false>(s, a, U);
        }
    }
    return true;
}

std::atomic<long long> g_split_launches{0};

constexpr int SPLIT_MIN_OUTPUTS = 4096;   // below this a launch is latency-bound either way: leave it to the generic kernel

}  // namespace

long long split_launch_count() { return g_split_launches.load(); }

// Filter / decimator on real or complex data.  d_taps: plain taps (sym: the half taps), ntaps of them.
bool launch_fir_split(hipStream_t s, const Geom& g, bool cplx, int lanes, ComplexOrder corder, bool sym, const float* d_taps,
                      int ntaps, const float* d_cross_taps, const float* d_in, float* d_out, float gain, bool apply_gain)
{
    if (g.count < SPLIT_MIN_OUTPUTS) return false;
    if (g.seamBI != 0 && d_cross_taps == nullptr) return false;
    if (cplx && apply_gain) return false;
    SplitArgs a{};
    OrderInfo o;
    if (!split_fill_fir(a, o, g, cplx, lanes, corder, sym, ntaps)) return false;   // the shapes: split_tile.hpp, shared with the row form
    a.in = d_in;
    a.out = d_out;
    a.taps = d_taps;
    a.gain = gain;
    a.apply_gain = apply_gain ? 1 : 0;
    if (!(cplx ? dispatch<true>(s, a, o, sym) : dispatch<false>(s, a, o, sym))) return false;
    g_split_launches++;
    launch_fir_crossfix(s, g, seam_span(g), cplx, false, d_cross_taps, d_in, d_out, gain, apply_gain);
    return true;
}

// Rational resampler on real or complex data (groups = prepareCoeffs rows, FilterInternal.hs:297-319).
bool launch_resample_split(hipStream_t s, const Geom& g, bool cplx, int lanes, ComplexOrder corder, const ResampTable& t,
                           const float* d_groups, const float* d_plain_taps, const float* d_in, float* d_out)
{
    if (g.count < SPLIT_MIN_OUTPUTS) return false;
    if (g.seamBI != 0 && d_plain_taps == nullptr) return false;
    SplitArgs a{};
    OrderInfo o;
    if (!split_fill_resample(a, o, g, cplx, lanes, corder, t)) return false;
    a.in = d_in;
    a.out = d_out;
    a.taps = d_groups;
    if (!(cplx ? dispatch<true>(s, a, o, false) : dispatch<false>(s, a, o, false))) return false;
    g_split_launches++;
    launch_resample_crossfix(s, g, seam_span(g), cplx, d_plain_taps, t.ntaps_plain, d_in, d_out);
    return true;
}

}  // namespace sdrhip
