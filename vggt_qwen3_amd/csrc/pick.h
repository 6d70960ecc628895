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

// ---- decoding constraints (vq3_pick_mask of include/vq3_hip.h): three bit planes of `words` 32-bit words each over the vocabulary,
// shared by all rows - plane 0 masks always, plane 1 while n_new < min_new, plane 2 at n_new == 0, with n_new = *step - prompt_cols
// read on the device, so a captured step gates itself. A block stages the effective words of the ids it streams in LDS once (whole
// words, one load per 32 ids and plane) and tests bits there. Only words that hold an id < V are read, and only bits of ids < V are
// tested: what the planes hold at or past V never matters.
struct MaskArgs {
  const uint32_t* planes;
  int words, min_new, prompt_cols;
};
constexpr int MASK_SLICE_WORDS = 256;   // LDS words of a pick's slice stage: slices of up to 254 * 32 ids, V <= 520 192

__device__ __forceinline__ uint32_t mask_word(const MaskArgs& m, int w, int n_new) {
  uint32_t x = m.planes[w];
  if (n_new < m.min_new) x |= m.planes[m.words + w];
  if (n_new == 0) x |= m.planes[2 * m.words + w];
  return x;
}
// the effective words of ids [c0, c1) into mw[0 ..]: mw[k] is word (c0 >> 5) + k. Every thread of the block calls it; sync before mask_bit
__device__ __forceinline__ void mask_stage(const MaskArgs& m, int n_new, int c0, int c1, uint32_t* mw) {
  if (c1 <= c0) return;
  const int w0 = c0 >> 5, nw = ((c1 - 1) >> 5) - w0 + 1;
  for (int k = threadIdx.x; k < nw; k += blockDim.x) mw[k] = mask_word(m, w0 + k, n_new);
}
__device__ __forceinline__ bool mask_bit(const uint32_t* mw, int c0, int i) { return (mw[(i >> 5) - (c0 >> 5)] >> (i & 31)) & 1u; }
// host side of the masked entries: the argument checks they share; returns nullptr or what is wrong
inline const char* mask_args_error(const void* planes, int words, int min_new, int prompt_cols, int V) {
  if (!planes) return "null mask planes";
  if ((long)words * 32 < V) return "mask planes shorter than the vocabulary";
  if (min_new < 0 || prompt_cols < 0) return "min_new and prompt_cols must be >= 0";
  return nullptr;
}

}  // namespace vq3pick
