// squelch.hpp -- the squelch (kernels_squelch.hip, squelch.cpp): the plan and the launcher.
//
//     level of a block = (256-slot sum of its detector powers, folded by halves) * (float)(1.0 / block_det)
//     gate: open / close levels with a hang, walked over the blocks of a row; the block's signal floats are copied or +0
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace sdrhip {

enum SquelchRoute : int { SQUELCH_AUTO = 0, SQUELCH_WG = 1, SQUELCH_LS = 2 };
constexpr int kSquelchGroup = 1024;                  // blocks whose levels and gates one workgroup holds in LDS at a time
constexpr int64_t kSquelchWgBlocks = 1024;           // auto: WG while a row has at most this many blocks ...
constexpr int64_t kSquelchWgBytes = 256 * 1024;      // ... and its detector plus signal bytes are at most this
constexpr int kSquelchBlockMax = 1 << 20;            // block_det, block_sig
constexpr int64_t kSquelchRowMax = (int64_t)1 << 40; // floats of a row

struct SquelchArgs {
    const float* det; int64_t det_stride; int det_complex; int block_det;
    const float* in; int64_t in_stride; float* out; int64_t out_stride; int block_sig;   // in == out == null: detect-only
    int rows; int64_t n_blocks;
    float open_level, close_level; int hang; int open_above;
    int32_t det0, hang0; const int32_t* state; int32_t* fin;                             // state null: {det0, hang0} (one row)
    float* levels; uint8_t* gates;
};

// The route of a call: forced = SQUELCH_AUTO follows the auto rule.  block_sig = 0: detect-only.  0: the forced route does not fit
// (LS without a workspace).  Host arithmetic only.
int squelch_route(int64_t n_blocks, int block_det, int det_complex, int block_sig, bool has_workspace, int forced);
int squelch_launches_of(int route, bool detect_only);   // 1 on WG; 3 on LS, 2 when detect-only
size_t squelch_rows_workspace_bytes(int rows, int64_t n_blocks);
void launch_squelch_rows(hipStream_t s, int route, const SquelchArgs& a, void* d_ws);
long long squelch_launch_count();
void squelch_set_route(int route);
int squelch_forced_route();

}  // namespace sdrhip
