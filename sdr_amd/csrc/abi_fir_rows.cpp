// abi_fir_rows.cpp -- the row forms of the FIR operators (include/sdr_hip.h, "row forms"): sdrhip_filter_run_rows,
// sdrhip_decimator_run_rows, sdrhip_resampler_run_rows.  Route 1 = the banked launch set of kernels_fir_rows.hip, route 2 = the
// one-row fir_run / resamp_run per row on the caller's stream, route 0 = auto (the rule below).  Every refusal comes before any
// device work, the descriptor's first-use upload included.
#include "descriptors.hpp"

namespace sdrhip {
namespace {

enum { ROUTE_AUTO = 0, ROUTE_BANKED = 1, ROUTE_ROWS = 2 };
enum { FAM_FILTER = 0, FAM_DECIMATOR = 1, FAM_RESAMPLER = 2 };

// The auto rule (sdr_hip.h states it with the points it was read from; profiles/fir_rows_bench.txt).  Measured: 2 / 8 / 32 rows (and
// one) x 128 / 1024 / 16384 / 2^20 outputs per row, a complex decimator, a real resampler and a real filter, each contiguous and with
// one seam inside the range.  kMinRows[shape][seamed][size]: the fewest measured rows from which the rows form's slowest round was
// below the K calls' fastest at that size and at every measured row count above it.  A launch between two measured sizes takes the
// larger of their two entries; one row, more than 32 rows, sizes outside 128 .. 2^20 and shapes of another family or data type were
// not measured and go row by row.  (One row was ahead only at 128 outputs, an edge of the sweep, and stays row by row.)
constexpr int64_t kAutoSizes[4] = {128, 1024, 16384, 1 << 20};
constexpr int kAutoMaxRows = 32;
constexpr int kMinRows[3][2][4] = {
    /* real filter        */ {{2, 2, 8, 32}, {2, 8, 8, 8}},
    /* complex decimator  */ {{2, 2, 2, 8}, {2, 8, 8, 8}},
    /* real resampler     */ {{2, 2, 2, 2}, {2, 8, 8, 8}},
};

bool auto_banks(int family, bool cplx, int rows, int64_t outputs, int64_t seam_block, bool seam_inside)
{
    if (cplx != (family == FAM_DECIMATOR)) return false;           // measured: complex decimator, real resampler, real filter
    if (rows < 2 || rows > kAutoMaxRows || outputs < kAutoSizes[0] || outputs > kAutoSizes[3]) return false;
    int hi = 0;
    while (kAutoSizes[hi] < outputs) hi++;
    const int lo = kAutoSizes[hi] == outputs ? hi : hi - 1;
    int need = 0;
    for (int seamed = 0; seamed < 2; seamed++) {
        // seam_block 0: the contiguous row; a seam inside the range: the seamed row; a seam block with no seam inside: neither was
        // measured as such, so both must hold
        if (seam_block == 0 ? seamed == 1 : (seam_inside && seamed == 0)) continue;
        for (int i = lo; i <= hi; i++)
            if (kMinRows[family][seamed][i] > need) need = kMinRows[family][seamed][i];
    }
    return rows >= need;
}

Geom fir_geom(const FirDesc* d, int64_t in_base, int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    Geom g;
    g.in_base = in_base;
    g.k_begin = k_begin;
    g.count = (int)(k_end - k_begin);
    g.I = 1;
    g.D = d->factor;
    g.Lp = d->Lp;
    g.seamBI = seam_block;
    return g;
}

// the taps the lane-split kernels take from a descriptor: plain (sym: the half taps)
int fir_split_ntaps(const FirDesc* d) { return d->sym ? d->ntaps_kernel : d->Lp; }

// as resamp_run_demod builds them
void resamp_geom(const ResampDesc* r, int64_t in_base, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t out_block, Geom& g,
                 ResampTable& t)
{
    g.in_base = in_base;
    g.k_begin = k_begin;
    g.count = (int)(k_end - k_begin);
    g.I = r->I;
    g.D = r->D;
    g.Lp = r->Lp;
    g.seamBI = seam_block < 0 ? -1 : seam_block * r->I;
    g.outB = out_block > 0 ? out_block : 0;
    t.ngroups = r->num_groups;
    t.group0 = r->group(k_begin);
    t.pos0 = r->in_offset(k_begin) - in_base;
    int acc = 0;
    for (int q = 0; q < r->num_groups; q++) {
        if (q < 64) t.pre[q] = acc;
        acc += r->increments[(t.group0 + q) % r->num_groups];
    }
    t.period = acc;
    t.row_stride = r->row_stride;
    t.nloop = r->nloop;
    t.ntaps_plain = r->ntaps;
    t.force_seq = 0;
    for (int q = 0; q < r->num_groups && q < 64; q++) t.fo[q] = r->offsets[q];
    // more than 64 groups: the per-group tables live in device memory (ensure_device); any non-null value keeps such a
    // descriptor off the banked route when the plan is asked before the upload
    if (r->num_groups > 64) t.ext = r->d_ext ? r->d_ext : reinterpret_cast<const int*>(r);
}

// the checks every row form shares, after the one-row call's own; need_in / need_out: floats a row must hold from its base
int rows_args(const char* what, const void* d_in, int64_t in_stride, const void* d_out, int64_t out_stride, int rows, bool cplx,
              int64_t need_in, int64_t need_out)
{
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr, what);
    SDRHIP_REQUIRE(d_in != d_out, what);
    SDRHIP_REQUIRE(!cplx || ((in_stride & 1) == 0 && (out_stride & 1) == 0), what);
    SDRHIP_REQUIRE(rows == 1 || (out_stride >= need_out && in_stride >= need_in), what);
    return SDRHIP_OK;
}

int fir_run_rows(const FirDesc* d, int family, const char* what, hipStream_t s, const float* d_in, int64_t in_stride, int64_t in_base,
                 float* d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block, int route)
{
    SDRHIP_REQUIRE(d != nullptr, what);
    SDRHIP_REQUIRE(k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, what);
    SDRHIP_REQUIRE(k_begin * d->factor >= in_base, what);
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block >= d->Lp, what);
    SDRHIP_REQUIRE(rows >= 1 && rows <= SDRHIP_ROWS_MAX, what);
    SDRHIP_REQUIRE(route >= ROUTE_AUTO && route <= ROUTE_ROWS, what);
    if (k_end == k_begin) return SDRHIP_OK;
    const int esz = d->cplx ? 2 : 1;
    const int64_t need_in = ((k_end - 1) * d->factor + d->Lp - in_base) * esz, need_out = (k_end - k_begin) * esz;
    int rc = rows_args(what, d_in, in_stride, d_out, out_stride, rows, d->cplx, need_in, need_out);
    if (rc != SDRHIP_OK) return rc;
    const Geom g = fir_geom(d, in_base, k_begin, k_end, seam_block);
    const bool served = fir_rows_plan(g, rows, d->cplx, d->lanes, d->corder, d->sym, fir_split_ntaps(d), nullptr);
    if (route == ROUTE_BANKED && !served) {
        set_error("%s: route 1 on a shape the banked kernel does not serve", what);
        return SDRHIP_ERR_ARG;
    }
    if (served && (route == ROUTE_BANKED || (route == ROUTE_AUTO && auto_banks(family, d->cplx, rows, k_end - k_begin, seam_block, seam_span(g).nseams > 0)))) {
        if ((rc = d->ensure_device()) != SDRHIP_OK) return rc;
        if (!launch_fir_rows(s, g, rows, in_stride, out_stride, d->cplx, d->lanes, d->corder, d->sym, d->sym ? d->d_taps : d->d_plain,
                             fir_split_ntaps(d), d->d_cross, d_in, d_out)) {
            set_error("%s: the banked launch refused a shape its plan accepted", what);
            return SDRHIP_ERR_STATE;
        }
        SDRHIP_CHECK_HIP(hipGetLastError());
        return SDRHIP_OK;
    }
    for (int r = 0; r < rows; r++)
        if ((rc = fir_run(d, s, d_in + r * in_stride, false, in_base, d_out + r * out_stride, k_begin, k_end, seam_block)) != SDRHIP_OK) return rc;
    return SDRHIP_OK;
}

int resamp_run_rows(const ResampDesc* r, const char* what, hipStream_t s, const float* d_in, int64_t in_stride, int64_t in_base,
                    float* d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block, int64_t out_block,
                    int route)
{
    SDRHIP_REQUIRE(r != nullptr, what);
    SDRHIP_REQUIRE(k_end >= k_begin && k_end - k_begin < (int64_t)0x7fffffff, what);
    SDRHIP_REQUIRE(k_begin >= 0, what);
    SDRHIP_REQUIRE(seam_block <= 0 || seam_block * r->I >= r->Lp, what);
    SDRHIP_REQUIRE(seam_block <= 0 || r->Lp >= r->D, what);
    SDRHIP_REQUIRE(rows >= 1 && rows <= SDRHIP_ROWS_MAX, what);
    SDRHIP_REQUIRE(route >= ROUTE_AUTO && route <= ROUTE_ROWS, what);
    if (k_end == k_begin) return SDRHIP_OK;
    SDRHIP_REQUIRE(r->in_offset(k_begin) >= in_base, what);
    const int esz = r->cplx ? 2 : 1;
    const int64_t need_in = (r->in_offset(k_end - 1) + r->Lp / r->I - in_base) * esz, need_out = (k_end - k_begin) * esz;
    int rc = rows_args(what, d_in, in_stride, d_out, out_stride, rows, r->cplx, need_in, need_out);
    if (rc != SDRHIP_OK) return rc;
    Geom g;
    ResampTable t;
    resamp_geom(r, in_base, k_begin, k_end, seam_block, out_block, g, t);
    const bool served = resample_rows_plan(g, rows, r->cplx, r->lanes, r->corder, t, nullptr);
    if (route == ROUTE_BANKED && !served) {
        set_error("%s: route 1 on a shape the banked kernel does not serve", what);
        return SDRHIP_ERR_ARG;
    }
    if (served && (route == ROUTE_BANKED || (route == ROUTE_AUTO && auto_banks(FAM_RESAMPLER, r->cplx, rows, k_end - k_begin, seam_block, seam_span(g).nseams > 0)))) {
        if ((rc = r->ensure_device()) != SDRHIP_OK) return rc;
        if (!launch_resample_rows(s, g, rows, in_stride, out_stride, r->cplx, r->lanes, r->corder, t, r->d_groups, r->d_plain, d_in, d_out)) {
            set_error("%s: the banked launch refused a shape its plan accepted", what);
            return SDRHIP_ERR_STATE;
        }
        SDRHIP_CHECK_HIP(hipGetLastError());
        return SDRHIP_OK;
    }
    for (int q = 0; q < rows; q++)
        if ((rc = resamp_run(r, s, d_in + q * in_stride, in_base, d_out + q * out_stride, k_begin, k_end, seam_block, out_block)) != SDRHIP_OK)
            return rc;
    return SDRHIP_OK;
}

void plan_out(const FirRowsPlan& p, const FirRowsPlan& one, int* plan)
{
    if (!plan) return;
    plan[0] = p.cycles_per_tile;
    plan[1] = p.tiles_per_row;
    plan[2] = p.U;
    plan[3] = p.outputs_per_cycle;
    plan[4] = one.cycles_per_tile;
    plan[5] = one.U;
}

}  // namespace

bool fir_rows_banked(const FirDesc* d, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    if (k_end <= k_begin || k_end - k_begin >= (int64_t)0x7fffffff) return false;
    return fir_rows_plan(fir_geom(d, k_begin * d->factor, k_begin, k_end, seam_block), rows, d->cplx, d->lanes, d->corder, d->sym, fir_split_ntaps(d),
                         nullptr);
}

bool resamp_rows_banked(const ResampDesc* r, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block)
{
    if (k_end <= k_begin || k_end - k_begin >= (int64_t)0x7fffffff) return false;
    Geom g;
    ResampTable t;
    resamp_geom(r, r->in_offset(k_begin), k_begin, k_end, seam_block, 0, g, t);
    return resample_rows_plan(g, rows, r->cplx, r->lanes, r->corder, t, nullptr);
}

}  // namespace sdrhip

using namespace sdrhip;

extern "C" {

int sdrhip_filter_run_rows(const sdrhip_filter* f, void* stream, const float* d_in, int64_t in_stride, int64_t in_base, float* d_out,
                           int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block, int route)
{
    return fir_run_rows(f, FAM_FILTER, "sdrhip_filter_run_rows", (hipStream_t)stream, d_in, in_stride, in_base, d_out, out_stride, rows,
                        k_begin, k_end, seam_block, route);
}

int sdrhip_decimator_run_rows(const sdrhip_decimator* d, void* stream, const float* d_in, int64_t in_stride, int64_t in_base,
                              float* d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block, int route)
{
    return fir_run_rows(d, FAM_DECIMATOR, "sdrhip_decimator_run_rows", (hipStream_t)stream, d_in, in_stride, in_base, d_out, out_stride,
                        rows, k_begin, k_end, seam_block, route);
}

int sdrhip_resampler_run_rows(const sdrhip_resampler* r, void* stream, const float* d_in, int64_t in_stride, int64_t in_base,
                              float* d_out, int64_t out_stride, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block,
                              int64_t out_block, int route)
{
    return resamp_run_rows(r, "sdrhip_resampler_run_rows", (hipStream_t)stream, d_in, in_stride, in_base, d_out, out_stride, rows, k_begin,
                           k_end, seam_block, out_block, route);
}

int sdrhip_debug_fir_rows_plan(const void* desc, int kind, int rows, int64_t k_begin, int64_t k_end, int64_t seam_block, int* plan)
{
    SDRHIP_REQUIRE(desc != nullptr && kind >= 0 && kind <= 2, "sdrhip_debug_fir_rows_plan");
    SDRHIP_REQUIRE(rows >= 1 && rows <= SDRHIP_ROWS_MAX && k_begin >= 0 && k_end > k_begin && k_end - k_begin < (int64_t)0x7fffffff,
                   "sdrhip_debug_fir_rows_plan");
    FirRowsPlan p{}, one{};
    bool served;
    if (kind == 2) {
        const ResampDesc* r = static_cast<const sdrhip_resampler*>(desc);
        Geom g;
        ResampTable t;
        resamp_geom(r, r->in_offset(k_begin), k_begin, k_end, seam_block, 0, g, t);
        served = resample_rows_plan(g, rows, r->cplx, r->lanes, r->corder, t, &p, &one);
    } else {
        const FirDesc* d = kind == 0 ? static_cast<const FirDesc*>(static_cast<const sdrhip_filter*>(desc))
                                     : static_cast<const FirDesc*>(static_cast<const sdrhip_decimator*>(desc));
        const Geom g = fir_geom(d, k_begin * d->factor, k_begin, k_end, seam_block);
        served = fir_rows_plan(g, rows, d->cplx, d->lanes, d->corder, d->sym, fir_split_ntaps(d), &p, &one);
    }
    if (!served) return 0;
    plan_out(p, one, plan);
    return 1;
}

long long sdrhip_debug_fir_rows_launches(void) { return fir_rows_launch_count(); }
long long sdrhip_debug_fir_rows_fixups(void) { return fir_rows_fixup_count(); }

}  // extern "C"
