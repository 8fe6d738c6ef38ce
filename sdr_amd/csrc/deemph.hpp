// deemph.hpp -- de-emphasis (kernels_deemph.hip, deemph.cpp, and the Pipe's map stage): the plan and the launcher.
//
//     y[i] = y[i-1] + alpha * (x[i] - y[i-1])        three f32 operations per sample: subtract, multiply, add
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdrhip {

enum DeemphRoute : int { DEEMPH_AUTO = 0, DEEMPH_SEQ = 1, DEEMPH_WG = 2, DEEMPH_LS = 3 };
constexpr int64_t kDeemphWgMax = 65536;       // the WG route's bound: 1024 chunks of 64 samples
constexpr int64_t kDeemphWgAuto = 32768;      // auto, with a workspace: from here on LS is ahead of WG (profiles/deemph_bench.txt, part C)
constexpr int kDeemphWgChunks = 1024;         // chunks (= lanes of the one workgroup) a row may have on WG
constexpr int kDeemphLsLaunches = 5;          // LS: speculate, three repair rounds, settle

// route: DEEMPH_SEQ / _WG / _LS; C: chunk length; W: the run-in used; nchunks: chunks per row (0 on SEQ)
struct DeemphPlan { int route; int64_t C, W; int nchunks; };

// ceil(40 / alpha) rounded up to a multiple of 4 (alpha in (0, 1])
int64_t deemph_default_run_in(float alpha);
// The plan of a run: forced = DEEMPH_AUTO follows the auto rule, anything else asks for that route.  false: the forced route does not
// fit (WG past its bound, LS without a workspace, either below two run-ins).  Host arithmetic only.
bool deemph_plan(int rows, int64_t n, float alpha, int run_in, bool has_workspace, int forced, DeemphPlan* plan);
size_t deemph_rows_workspace_bytes(int rows, int64_t n);
// Row r is d_in + r * in_stride -> d_out + r * out_stride (floats); its state d_state[r] (d_state null: `state`, one row), its final
// state d_final[r] (d_final may be d_state); d_ws (may be null unless the plan is LS) starts with four statistics words per row.
void launch_deemph_rows(hipStream_t s, const DeemphPlan& plan, int rows, int64_t n, float alpha, float state, const float* d_state,
                        const float* d_in, int64_t in_stride, float* d_out, int64_t out_stride, float* d_final, void* d_ws);
long long deemph_launch_count();              // kernel launches so far, process-wide: 1 per SEQ or WG run, kDeemphLsLaunches per LS run
void deemph_set_route(int route);
int deemph_forced_route();

}  // namespace sdrhip
