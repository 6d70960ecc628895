// What the two picks of a decode step share (decode.hip: vq3_greedy_pick, sample.hip: vq3_sample_pick): phase 1 of either reduces each
// of PICK_SLICES slices of a row's vocabulary to (best value, smallest index); the final kernel of decode.hip combines the slices and
// does the bookkeeping (finished rows emit pad, eos marks a row finished, generated / next_ids are written).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace vq3pick {

constexpr int PICK_SLICES = 64;     // partials per row: pval / pidx are [B, PICK_SLICES]
constexpr int PICK_MAX_IDS = 512;   // columns of `generated` (prompt + new ids) the penalty / ban overlay is sized for

// greedy_pick_final_kernel on `stream`: one 64-lane workgroup per row. A slice with nothing to offer holds (-inf, 0x7fffffff).
void launch_pick_final(const float* pval, const int32_t* pidx, int64_t* generated, int max_new, const int32_t* step, int32_t* finished,
                       const int64_t* eos_ids, int n_eos, long pad_id, int32_t* next_ids, int B, hipStream_t stream);

}  // namespace vq3pick
