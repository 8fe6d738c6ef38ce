// deemph.cpp -- the C ABI of de-emphasis (include/sdr_hip.h "de-emphasis"): the checks, all of them before any device work, then the
// plan and the launcher of kernels_deemph.hip.  The one-row call is the rows call with one row and the state by value.
#include <math.h>

#include "common.hpp"
#include "deemph.hpp"

using namespace sdrhip;

namespace {
bool alpha_ok(float alpha) { return isfinite(alpha) && alpha > 0.0f && alpha <= 1.0f; }

int run(const char* who, void* stream, const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int rows, int64_t n, float alpha,
        float state, const float* d_state, bool need_state, float* d_final, void* d_workspace, size_t workspace_bytes, int run_in)
{
    SDRHIP_REQUIRE(alpha_ok(alpha), who);
    SDRHIP_REQUIRE(rows >= 1 && rows <= SDRHIP_ROWS_MAX, who);
    SDRHIP_REQUIRE(n >= 0 && run_in >= 0 && (d_state != nullptr || !need_state) && d_final != nullptr, who);
    SDRHIP_REQUIRE(d_in != nullptr && d_out != nullptr && d_in != d_out, who);
    SDRHIP_REQUIRE(rows == 1 || (in_stride >= n && out_stride >= n), who);
    SDRHIP_REQUIRE(d_workspace == nullptr || workspace_bytes >= deemph_rows_workspace_bytes(rows, n), who);
    if (n == 0) d_workspace = nullptr;       // n == 0 copies the states and touches nothing else
    DeemphPlan p;
    if (!deemph_plan(rows, n, alpha, run_in, d_workspace != nullptr, n > 0 ? deemph_forced_route() : DEEMPH_AUTO, &p)) {
        set_error("%s: the forced route does not fit: WG needs 2 * run-in <= n <= 65536, LS a workspace and n >= 2 * run-in", who);
        return SDRHIP_ERR_ARG;
    }
    launch_deemph_rows((hipStream_t)stream, p, rows, n, alpha, state, d_state, d_in, in_stride, d_out, out_stride, d_final, d_workspace);
    SDRHIP_CHECK_HIP(hipGetLastError());
    return SDRHIP_OK;
}
}  // namespace

extern "C" {

float sdrhip_deemph_alpha(double tau_seconds, double sample_rate)
{
    if (!(isfinite(tau_seconds) && isfinite(sample_rate) && tau_seconds > 0.0 && sample_rate > 0.0)) return 0.0f;
    return (float)(1.0 - exp(-1.0 / (tau_seconds * sample_rate)));
}

size_t sdrhip_deemph_workspace_bytes(int64_t n) { return deemph_rows_workspace_bytes(1, n); }

size_t sdrhip_deemph_rows_workspace_bytes(int rows, int64_t n)
{
    return rows >= 1 && rows <= SDRHIP_ROWS_MAX ? deemph_rows_workspace_bytes(rows, n) : 0;
}

int sdrhip_deemph_run(void* stream, const float* d_in, float* d_out, int64_t n, float alpha, float state, float* d_final, void* d_workspace,
                      size_t workspace_bytes, int run_in)
{
    return run("sdrhip_deemph_run", stream, d_in, n, d_out, n, 1, n, alpha, state, nullptr, false, d_final, d_workspace, workspace_bytes, run_in);
}

int sdrhip_deemph_run_rows(void* stream, const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, int rows, int64_t n,
                           float alpha, const float* d_state, float* d_final, void* d_workspace, size_t workspace_bytes, int run_in)
{
    return run("sdrhip_deemph_run_rows", stream, d_in, in_stride, d_out, out_stride, rows, n, alpha, 0.0f, d_state, true, d_final, d_workspace,
               workspace_bytes, run_in);
}

int sdrhip_debug_deemph_plan(int rows, int64_t n, float alpha, int run_in, int has_workspace, int* route, int64_t* chunk, int64_t* run_in_used)
{
    SDRHIP_REQUIRE(alpha_ok(alpha) && rows >= 1 && rows <= SDRHIP_ROWS_MAX && n >= 0 && run_in >= 0, "sdrhip_debug_deemph_plan");
    DeemphPlan p;
    if (!deemph_plan(rows, n, alpha, run_in, has_workspace != 0 && n > 0, n > 0 ? deemph_forced_route() : DEEMPH_AUTO, &p)) {
        set_error("sdrhip_debug_deemph_plan: the forced route does not fit");
        return SDRHIP_ERR_ARG;
    }
    if (route) *route = p.route;
    if (chunk) *chunk = p.C;
    if (run_in_used) *run_in_used = p.W;
    return p.nchunks;
}

void sdrhip_debug_set_deemph_route(int route) { deemph_set_route(route >= DEEMPH_SEQ && route <= DEEMPH_LS ? route : DEEMPH_AUTO); }

long long sdrhip_debug_deemph_launches(void) { return deemph_launch_count(); }

}  // extern "C"
