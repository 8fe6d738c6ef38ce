// squelch.cpp -- the C ABI of the squelch (include/sdr_hip.h "squelch"): the checks, all of them before any device work, then the
// route and the launcher of kernels_squelch.hip.  The one-row call is the rows call with one row and the state by value.
#include <math.h>

#include "common.hpp"
#include "squelch.hpp"

using namespace sdrhip;

namespace {
bool level_ok(float v) { return isfinite(v) && v >= 0.0f; }

int run(const char* who, void* stream, const SquelchArgs& a, void* d_workspace, size_t workspace_bytes)
{
    const bool detect_only = a.in == nullptr && a.out == nullptr;
    SDRHIP_REQUIRE(a.rows >= 1 && a.rows <= SDRHIP_ROWS_MAX, who);
    SDRHIP_REQUIRE(a.det_complex == 0 || a.det_complex == 1, who);
    SDRHIP_REQUIRE(a.open_above == 0 || a.open_above == 1, who);
    SDRHIP_REQUIRE(a.block_det >= 1 && a.block_det <= kSquelchBlockMax, who);
    SDRHIP_REQUIRE(detect_only || (a.block_sig >= 1 && a.block_sig <= kSquelchBlockMax), who);
    SDRHIP_REQUIRE(a.n_blocks >= 0 && a.n_blocks <= kSquelchRowMax, who);          // ... so that the products below stay in 64 bits
    const int64_t det_row = a.n_blocks * a.block_det * (a.det_complex ? 2 : 1);
    SDRHIP_REQUIRE(det_row <= kSquelchRowMax, who);
    const int64_t sig_row = detect_only ? 0 : a.n_blocks * a.block_sig;
    SDRHIP_REQUIRE(sig_row <= kSquelchRowMax, who);
    SDRHIP_REQUIRE(level_ok(a.open_level) && level_ok(a.close_level), who);
    SDRHIP_REQUIRE(a.open_above ? a.close_level <= a.open_level : a.close_level >= a.open_level, who);
    SDRHIP_REQUIRE(a.hang >= 0 && a.hang <= (1 << 30), who);
    SDRHIP_REQUIRE(a.det != nullptr, who);
    SDRHIP_REQUIRE((a.in == nullptr) == (a.out == nullptr), who);
    SDRHIP_REQUIRE(!a.det_complex || a.det_stride % 2 == 0, who);
    SDRHIP_REQUIRE(a.rows == 1 || (a.det_stride >= det_row && (detect_only || (a.in_stride >= sig_row && a.out_stride >= sig_row))), who);
    // aliasing: in place needs the rows to coincide; the detector may be written only where it is the signal, block for block
    SDRHIP_REQUIRE(detect_only || a.out != a.in || a.out_stride == a.in_stride, who);
    SDRHIP_REQUIRE(detect_only || (const float*)a.out != a.det || a.in == a.det, who);
    SDRHIP_REQUIRE(detect_only || (const float*)a.out != a.det || (!a.det_complex && a.block_det == a.block_sig && a.det_stride == a.in_stride), who);
    SDRHIP_REQUIRE(d_workspace == nullptr || workspace_bytes >= squelch_rows_workspace_bytes(a.rows, a.n_blocks), who);
    const int route = squelch_route(a.n_blocks, a.block_det, a.det_complex, detect_only ? 0 : a.block_sig, d_workspace != nullptr,
                                    squelch_forced_route());
    if (route == 0) {
        set_error("%s: the forced route does not fit: LS needs a workspace", who);
        return SDRHIP_ERR_ARG;
    }
    launch_squelch_rows((hipStream_t)stream, route, a, d_workspace);
    SDRHIP_CHECK_HIP(hipGetLastError());
    return SDRHIP_OK;
}
}  // namespace

extern "C" {

size_t sdrhip_squelch_rows_workspace_bytes(int rows, int64_t n_blocks)
{
    return rows >= 1 && rows <= SDRHIP_ROWS_MAX && n_blocks >= 0 && n_blocks <= kSquelchRowMax ? squelch_rows_workspace_bytes(rows, n_blocks) : 0;
}

int sdrhip_squelch_run_rows(void* stream, const float* d_det, int64_t det_stride, int det_complex, int block_det, const float* d_in,
                            int64_t in_stride, float* d_out, int64_t out_stride, int block_sig, int rows, int64_t n_blocks, float open_level,
                            float close_level, int hang_blocks, int open_above, const int32_t* d_state, int32_t* d_final, float* d_levels,
                            uint8_t* d_gates, void* d_workspace, size_t workspace_bytes)
{
    const SquelchArgs a = {d_det, det_stride, det_complex, block_det, d_in, in_stride, d_out, out_stride, block_sig, rows, n_blocks,
                           open_level, close_level, hang_blocks, open_above, 0, 0, d_state, d_final, d_levels, d_gates};
    return run("sdrhip_squelch_run_rows", stream, a, d_workspace, workspace_bytes);
}

int sdrhip_squelch_run(void* stream, const float* d_det, int det_complex, int block_det, const float* d_in, float* d_out, int block_sig,
                       int64_t n_blocks, float open_level, float close_level, int hang_blocks, int open_above, int32_t det, int32_t hang_left,
                       int32_t* d_final, float* d_levels, uint8_t* d_gates, void* d_workspace, size_t workspace_bytes)
{
    const SquelchArgs a = {d_det, 0, det_complex, block_det, d_in, 0, d_out, 0, block_sig, 1, n_blocks,
                           open_level, close_level, hang_blocks, open_above, det, hang_left, nullptr, d_final, d_levels, d_gates};
    return run("sdrhip_squelch_run", stream, a, d_workspace, workspace_bytes);
}

int sdrhip_debug_squelch_plan(int rows, int64_t n_blocks, int block_det, int det_complex, int block_sig, int has_workspace, int* route)
{
    const char* who = "sdrhip_debug_squelch_plan";
    SDRHIP_REQUIRE(rows >= 1 && rows <= SDRHIP_ROWS_MAX && (det_complex == 0 || det_complex == 1), who);
    SDRHIP_REQUIRE(block_det >= 1 && block_det <= kSquelchBlockMax && block_sig >= 0 && block_sig <= kSquelchBlockMax, who);
    SDRHIP_REQUIRE(n_blocks >= 0 && n_blocks <= kSquelchRowMax && n_blocks * block_det * (det_complex ? 2 : 1) <= kSquelchRowMax &&
                   n_blocks * block_sig <= kSquelchRowMax, who);
    const int r = squelch_route(n_blocks, block_det, det_complex, block_sig, has_workspace != 0, squelch_forced_route());
    if (r == 0) {
        set_error("%s: the forced route does not fit: LS needs a workspace", who);
        return SDRHIP_ERR_ARG;
    }
    if (route) *route = r;
    return squelch_launches_of(r, block_sig == 0);
}

void sdrhip_debug_set_squelch_route(int route) { squelch_set_route(route == SQUELCH_WG || route == SQUELCH_LS ? route : SQUELCH_AUTO); }

long long sdrhip_debug_squelch_launches(void) { return squelch_launch_count(); }

}  // extern "C"
