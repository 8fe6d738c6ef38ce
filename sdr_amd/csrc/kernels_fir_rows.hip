// kernels_fir_rows.hip -- the row forms of the FIR filter, decimator and resampler (sdrhip_*_run_rows): every row of a bank in one
// tile launch and at most one seam fix-up launch.
//
// k_split_rows is kernels_split.hip's tile (split_tile.hpp: staging, the lanes-as-partial-sums walk, the DPP fold, the store) with
// the row on blockIdx.y.  The row selects an input base and an output base and nothing else, so row r's One outputs are what k_split
// gives that row alone; the per-workgroup 16-byte `shift` of the staging loop absorbs whatever alignment a row base and stride have.
// The Cross outputs are rewritten by row-axis copies of the three generic fix-up kernels of kernels_crossfix.hip, one thread per
// (row, seam, slot), one launch for all rows, only when there is a seam inside the range.
//
// Plan: plan_tile sizes a tile for long launches (up to 1024 outputs, a 32 KiB span).  A row of a live block holds 38 .. 1024
// outputs, so the rows plan caps the tile at the row's own cycle count, rounded up to a whole run of U groups of G = 64/M outputs,
// and takes U = 1 where a row is shorter than the 4 * SPLIT_U * G cycles that keep four waves busy with U = 2; a long row gets
// exactly plan_tile's tile.  One workgroup per (tile, row): short rows are not packed into one workgroup (README, "And for the FIR
// rows").
#include <atomic>

#include "split_tile.hpp"

namespace sdrhip {

namespace {

template <bool CPLX, int M, int ORD, bool SYM, int NCHMAX, int U, bool EXACT>
__global__ void __launch_bounds__(256) k_split_rows(SplitArgs a, int64_t in_stride, int64_t out_stride)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int64_t row = blockIdx.y;
    split_tile<CPLX, M, ORD, SYM, NCHMAX, U, EXACT>(a, reinterpret_cast<const float*>(a.in) + row * in_stride, a.out + row * out_stride,
                                                    blockIdx.x, smem_raw);
}

// ---- seam fix-ups: kernels_crossfix.hip's generic kernels with a row axis (t = (row * nseams + seam) * per_seam + slot) ----
struct RowSlot { int64_t row; int si, ci; bool live; };
__device__ __forceinline__ RowSlot row_slot(int rows, int nseams, int per_seam)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t per_row = (int64_t)nseams * per_seam;
    RowSlot s;
    s.live = t < per_row * rows;
    s.row = t / per_row;
    const int q = (int)(t - s.row * per_row);
    s.si = q / per_seam;
    s.ci = q - s.si * per_seam;
    return s;
}

// Cross outputs of a complex filter / decimator: sequential over the Lp plain taps
// (filterCrossHighLevel with Mult (Complex a) a, FilterInternal.hs:397-408, Util.hs:87-88).
__global__ void __launch_bounds__(256) k_fir_cplx_crossfix_rows(Geom g, const float* __restrict__ xtaps, const float* __restrict__ in0,
                                                                 int64_t in_stride, float* __restrict__ out0, int64_t out_stride, int rows,
                                                                 int64_t first_seam, int nseams, int per_seam)
{
    const RowSlot s = row_slot(rows, nseams, per_seam);
    if (!s.live) return;
    const int64_t edge = (first_seam + s.si) * g.seamBI;
    const int64_t m = (edge + g.D - 1) / g.D - 1 - s.ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    const float2* x = reinterpret_cast<const float2*>(in0 + s.row * in_stride) + (v - g.in_base);
    float re = 0.0f, im = 0.0f;
    for (int j = 0; j < g.Lp; j++) {
        const float2 sv = x[j];
        re = re + sv.x * xtaps[j];
        im = im + sv.y * xtaps[j];
    }
    *reinterpret_cast<float2*>(out0 + s.row * out_stride + 2 * (m - g.k_begin)) = make_float2(re, im);
}

// Cross outputs of a real FIR / decimator: sequential over the Lp plain taps
// (filterCrossHighLevel / decimateCrossHighLevel, FilterInternal.hs:397-408).
__global__ void __launch_bounds__(256) k_fir_real_crossfix_rows(Geom g, const float* __restrict__ xtaps, const float* __restrict__ in0,
                                                                 int64_t in_stride, float* __restrict__ out0, int64_t out_stride, int rows,
                                                                 int64_t first_seam, int nseams, int per_seam)
{
    const RowSlot s = row_slot(rows, nseams, per_seam);
    if (!s.live) return;
    const int64_t edge = (first_seam + s.si) * g.seamBI;
    const int64_t m = (edge + g.D - 1) / g.D - 1 - s.ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    const float* x = in0 + s.row * in_stride + (v - g.in_base);
    float r = 0.0f;
    for (int j = 0; j < g.Lp; j++) r = r + x[j] * xtaps[j];
    out0[s.row * out_stride + (m - g.k_begin)] = r;
}

// Cross outputs of a resampler, real or complex data (resampleCrossHighLevel, FilterInternal.hs:410-423):
// taps = stride I (drop filterOffset coeffs) over the UNPADDED taps, sequential.
template <bool CPLX>
__global__ void __launch_bounds__(256) k_resample_crossfix_rows(Geom g, const float* __restrict__ plain, int ntaps,
                                                                 const float* __restrict__ in0, int64_t in_stride, float* __restrict__ out0,
                                                                 int64_t out_stride, int rows, int64_t first_seam, int nseams, int per_seam)
{
    const RowSlot s = row_slot(rows, nseams, per_seam);
    if (!s.live) return;
    const int64_t edge = (first_seam + s.si) * g.seamBI;           // upsampled units
    const int64_t m = (edge + g.D - 1) / g.D - 1 - s.ci;
    if (m < g.k_begin || m >= g.k_begin + g.count) return;
    const int64_t v = m * g.D;
    if (!(v < edge && v + g.Lp > edge)) return;
    if (!seam_has_crossover(edge, g.I, g.D, g.Lp)) return;       // the Pipe goes straight to the next buffer here
    if (late_output_is_one(m, edge, g.I, g.D, g.outB)) return;   // first output of an output block, first input beyond the seam
    const int64_t pos = (v + g.I - 1) / g.I;                     // inOff(m)
    const int fo = (int)(pos * g.I - v);
    const float* in = in0 + s.row * in_stride;
    float* out = out0 + s.row * out_stride;
    if constexpr (CPLX) {
        const float2* x = reinterpret_cast<const float2*>(in) + (pos - g.in_base);
        float re = 0.0f, im = 0.0f;
        for (int l = 0, j = fo; j < ntaps; l++, j += g.I) {
            const float2 sv = x[l];
            re = re + sv.x * plain[j];
            im = im + sv.y * plain[j];
        }
        *reinterpret_cast<float2*>(out + 2 * (m - g.k_begin)) = make_float2(re, im);
    } else {
        const float* x = in + (pos - g.in_base);
        float r = 0.0f;
        for (int l = 0, j = fo; j < ntaps; l++, j += g.I) r = r + x[l] * plain[j];
        out[m - g.k_begin] = r;
    }
}

// ---- the rows plan ----
// plan_tile's tile, capped at the row: NN = the row's cycles rounded up to a whole run of U * G where that is less; U = 1 for a row
// shorter than 4 * SPLIT_U * G cycles.  A long row keeps plan_tile's NN, U and span untouched.
bool plan_rows_tile(SplitArgs& a, int M, bool cplx, int& U)
{
    if (!plan_tile(a, M, cplx, U)) return false;
    const int G = 64 / M;
    const int64_t ncyc = ((int64_t)a.count + a.NC - 1) / a.NC;
    if (ncyc < 4 * SPLIT_U * G) U = 1;
    const int64_t run = (int64_t)U * G;
    const int64_t cap = (ncyc + run - 1) / run * run;
    if (cap < a.NN) {
        a.NN = (int)cap;
        a.span = (int)((cap - 1) * a.period + a.pre[a.NC - 1] + a.reach);
    }
    return true;
}

template <bool CPLX, int M, int ORD, bool SYM, int NCHMAX, int U, bool EXACT>
void launch_kernel(hipStream_t s, const SplitArgs& a, dim3 grid, size_t lds_bytes, int64_t in_stride, int64_t out_stride)
{
    auto kern = k_split_rows<CPLX, M, ORD, SYM, NCHMAX, U, EXACT>;
    // per instantiation and device: tiles of large decimation factors exceed the 64 KiB default cap
    static std::atomic<bool> attr_set[64];
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= 64 || !attr_set[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
        if (dev >= 0 && dev < 64) attr_set[dev] = true;
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds_bytes, s, a, in_stride, out_stride);
}

struct RowsLaunch { hipStream_t s; int rows; int64_t in_stride, out_stride; };

// the instantiation ladder of kernels_split.hip's launch_variant_u (guard-free code for real data with 8 / 16 / 32 chunks and U = 2)
template <bool CPLX, int M, int ORD, bool SYM, int U>
void launch_variant_u(const RowsLaunch& r, const SplitArgs& a)
{
    const int64_t ncyc = ((int64_t)a.count + a.NC - 1) / a.NC;
    const dim3 grid((unsigned)((ncyc + a.NN - 1) / a.NN), (unsigned)r.rows);
    const size_t lds = split_lds_bytes(a, CPLX);
    constexpr bool EX = U == SPLIT_U && !CPLX;
    if (EX && a.nch == 8) launch_kernel<CPLX, M, ORD, SYM, 8, U, EX>(r.s, a, grid, lds, r.in_stride, r.out_stride);
    else if (EX && a.nch == 16) launch_kernel<CPLX, M, ORD, SYM, 16, U, EX>(r.s, a, grid, lds, r.in_stride, r.out_stride);
    else if (EX && a.nch == 32) launch_kernel<CPLX, M, ORD, SYM, 32, U, EX>(r.s, a, grid, lds, r.in_stride, r.out_stride);
    else if (a.nch <= 8) launch_kernel<CPLX, M, ORD, SYM, 8, U, false>(r.s, a, grid, lds, r.in_stride, r.out_stride);
    else if (a.nch <= 16) launch_kernel<CPLX, M, ORD, SYM, 16, U, false>(r.s, a, grid, lds, r.in_stride, r.out_stride);
    else if (a.nch <= 32) launch_kernel<CPLX, M, ORD, SYM, 32, U, false>(r.s, a, grid, lds, r.in_stride, r.out_stride);
    else launch_kernel<CPLX, M, ORD, SYM, 64, U, false>(r.s, a, grid, lds, r.in_stride, r.out_stride);
}

template <bool CPLX, int M, int ORD, bool SYM>
void launch_variant(const RowsLaunch& r, const SplitArgs& a, int U)
{
    if (U == SPLIT_U) launch_variant_u<CPLX, M, ORD, SYM, SPLIT_U>(r, a);
    else launch_variant_u<CPLX, M, ORD, SYM, 1>(r, a);
}

void dispatch(const RowsLaunch& r, const SplitArgs& a, bool cplx, OrderInfo o, bool sym, int U)
{
    if (!cplx) {
        if (o.M == 8) { if (sym) launch_variant<false, 8, 0, true>(r, a, U); else launch_variant<false, 8, 0, false>(r, a, U); }
        else { if (sym) launch_variant<false, 4, 0, true>(r, a, U); else launch_variant<false, 4, 0, false>(r, a, U); }
    } else if (o.ord == 0) {
        if (o.M == 4) launch_variant<true, 4, 0, false>(r, a, U); else launch_variant<true, 2, 0, false>(r, a, U);
    } else if (o.M == 8) {
        launch_variant<true, 8, 1, false>(r, a, U);
    } else {
        launch_variant<true, 4, 1, false>(r, a, U);
    }
}

std::atomic<long long> g_rows_tile_launches{0}, g_rows_fixup_launches{0};

// the fix-up grid exists: one thread per (row, seam, slot), 256 a block, the block count within a grid dimension
bool fixup_grid(const SeamSpan& sp, int rows, unsigned* blocks)
{
    const int64_t threads = (int64_t)sp.nseams * sp.per * rows;
    const int64_t b = (threads + 255) / 256;
    if (b > 0x7fffffff) return false;
    *blocks = (unsigned)b;
    return true;
}

void fill_plan(const SplitArgs& a, int U, FirRowsPlan* p)
{
    if (!p) return;
    const int64_t ncyc = ((int64_t)a.count + a.NC - 1) / a.NC;
    p->cycles_per_tile = a.NN;
    p->tiles_per_row = (int)((ncyc + a.NN - 1) / a.NN);
    p->U = U;
    p->outputs_per_cycle = a.NC;
}

}  // namespace

long long fir_rows_launch_count() { return g_rows_tile_launches.load(); }
long long fir_rows_fixup_count() { return g_rows_fixup_launches.load(); }

bool fir_rows_plan(const Geom& g, int rows, bool cplx, int lanes, ComplexOrder corder, bool sym, int ntaps, FirRowsPlan* rows_plan,
                   FirRowsPlan* one_row_split_plan)
{
    SplitArgs a{};
    OrderInfo o;
    int U = 1;
    unsigned blocks = 0;
    if (g.count <= 0 || !split_fill_fir(a, o, g, cplx, lanes, corder, sym, ntaps)) return false;
    if (one_row_split_plan) {
        SplitArgs b = a;
        if (!plan_tile(b, o.M, cplx, U)) return false;
        fill_plan(b, U, one_row_split_plan);
    }
    if (!plan_rows_tile(a, o.M, cplx, U) || !fixup_grid(seam_span(g), rows, &blocks)) return false;
    fill_plan(a, U, rows_plan);
    return true;
}

bool resample_rows_plan(const Geom& g, int rows, bool cplx, int lanes, ComplexOrder corder, const ResampTable& t, FirRowsPlan* rows_plan,
                        FirRowsPlan* one_row_split_plan)
{
    SplitArgs a{};
    OrderInfo o;
    int U = 1;
    unsigned blocks = 0;
    if (g.count <= 0 || !split_fill_resample(a, o, g, cplx, lanes, corder, t)) return false;
    if (one_row_split_plan) {
        SplitArgs b = a;
        if (!plan_tile(b, o.M, cplx, U)) return false;
        fill_plan(b, U, one_row_split_plan);
    }
    if (!plan_rows_tile(a, o.M, cplx, U) || !fixup_grid(seam_span(g), rows, &blocks)) return false;
    fill_plan(a, U, rows_plan);
    return true;
}

bool launch_fir_rows(hipStream_t s, const Geom& g, int rows, int64_t in_stride, int64_t out_stride, bool cplx, int lanes,
                     ComplexOrder corder, bool sym, const float* d_taps, int ntaps, const float* d_cross_taps, const float* d_in, float* d_out)
{
    SplitArgs a{};
    OrderInfo o;
    int U = 1;
    unsigned blocks = 0;
    const SeamSpan sp = seam_span(g);
    if (g.count <= 0 || rows < 1 || !split_fill_fir(a, o, g, cplx, lanes, corder, sym, ntaps)) return false;
    if (g.seamBI != 0 && d_cross_taps == nullptr) return false;
    if (!plan_rows_tile(a, o.M, cplx, U) || !fixup_grid(sp, rows, &blocks)) return false;
    a.in = d_in;
    a.out = d_out;
    a.taps = d_taps;
    dispatch(RowsLaunch{s, rows, in_stride, out_stride}, a, cplx, o, sym, U);
    g_rows_tile_launches++;
    if (sp.nseams > 0) {
        if (cplx)
            hipLaunchKernelGGL(k_fir_cplx_crossfix_rows, dim3(blocks), dim3(256), 0, s, g, d_cross_taps, d_in, in_stride, d_out, out_stride, rows,
                               sp.first, sp.nseams, sp.per);
        else
            hipLaunchKernelGGL(k_fir_real_crossfix_rows, dim3(blocks), dim3(256), 0, s, g, d_cross_taps, d_in, in_stride, d_out, out_stride, rows,
                               sp.first, sp.nseams, sp.per);
        g_rows_fixup_launches++;
    }
    return true;
}

bool launch_resample_rows(hipStream_t s, const Geom& g, int rows, int64_t in_stride, int64_t out_stride, bool cplx, int lanes,
                          ComplexOrder corder, const ResampTable& t, const float* d_groups, const float* d_plain_taps, const float* d_in,
                          float* d_out)
{
    SplitArgs a{};
    OrderInfo o;
    int U = 1;
    unsigned blocks = 0;
    const SeamSpan sp = seam_span(g);
    if (g.count <= 0 || rows < 1 || !split_fill_resample(a, o, g, cplx, lanes, corder, t)) return false;
    if (g.seamBI != 0 && d_plain_taps == nullptr) return false;
    if (!plan_rows_tile(a, o.M, cplx, U) || !fixup_grid(sp, rows, &blocks)) return false;
    a.in = d_in;
    a.out = d_out;
    a.taps = d_groups;
    dispatch(RowsLaunch{s, rows, in_stride, out_stride}, a, cplx, o, false, U);
    g_rows_tile_launches++;
    if (sp.nseams > 0) {
        if (cplx)
            hipLaunchKernelGGL(k_resample_crossfix_rows<true>, dim3(blocks), dim3(256), 0, s, g, d_plain_taps, t.ntaps_plain, d_in, in_stride,
                               d_out, out_stride, rows, sp.first, sp.nseams, sp.per);
        else
            hipLaunchKernelGGL(k_resample_crossfix_rows<false>, dim3(blocks), dim3(256), 0, s, g, d_plain_taps, t.ntaps_plain, d_in, in_stride,
                               d_out, out_stride, rows, sp.first, sp.nseams, sp.per);
        g_rows_fixup_launches++;
    }
    return true;
}

}  // namespace sdrhip
