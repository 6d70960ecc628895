// Per-token log-probabilities over bf16 logits rows: what transformers callers get from `output_logits` + log_softmax + gather and
// from GenerationMixin.compute_transition_scores. One read-only streaming pass per row gives, in f32,
//   lse = logsumexp(row[:V]),  logprob = row[t] - lse,  rank = #{j : row[j] > row[t]} + #{j < t : row[j] == row[t]}
// (rank == 0 exactly when the first-index argmax of vq3_greedy_pick would pick t). The bound is the bytes of the rows, read once.
//
// One body (slice_stats), two launch shapes:
//  * rows   - grid (1, n), 1024 threads: one workgroup per row, which also writes the row's results. Scoring: many rows.
//  * slices - grid (64, n), 256 threads: a workgroup owns 1/64 of the vocabulary and leaves (max, sum, count); a second launch of one
//             wave per row combines the 64 partials in a fixed order. Decode: 1..8 rows of 300 KB must not hang off 1..8 workgroups.
// The running maximum is kept per thread (online softmax), so a row is read once and rows offset by hundreds stay finite. No atomics:
// every sum is a fixed tree, the same bits run after run - of ONE shape: the two shapes sum in different orders, so a caller whose
// results must not depend on its row count (score()'s chunks) names the shape. Columns [V, ld) are never loaded into a result; -inf
// inside [0, V) is legal: a -inf target gives logprob -inf, and so does every target of a row that is -inf throughout (lse -inf).
#include <math.h>

#include "common.h"
#include "vq3_hip.h"

namespace {

constexpr int LP_SLICES = 64;          // vocabulary slices of the decode shape (the combine kernel is one wave: one partial per lane)
// Rows from which one workgroup per row is the faster shape at V = 151 936 (tools/bench_logprob.py, profiles/logprob_bench.json:
// split is faster up to 64 rows, one workgroup per row from 128).
constexpr int LP_ROWS_SWITCH = 128;

// (m, s): a running maximum and the sum of exp(x - m) over what has been seen; (-inf, 0) is the empty state
__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  if (M == -INFINITY) return;          // both empty (or all -inf so far): exp(-inf - -inf) would be NaN
  s = s * __expf(m - M) + os * __expf(om - M);
  m = M;
}

// K logits starting at column `col` into one thread's state. cnt: columns that beat the target (greater, or equal and to its left);
// tv is NaN for a row without a target, which no comparison satisfies.
template <int K>
__device__ __forceinline__ void lse_take(const float* f, int col, float tv, int t, float& m, float& s, int& cnt) {
  float mk = f[0];
#pragma unroll
  for (int j = 1; j < K; ++j) mk = fmaxf(mk, f[j]);
  if (mk > m) {                        // (m = -inf: s is 0 and stays 0)
    s *= __expf(m - mk);
    m = mk;
  }
  if (m > -INFINITY) {
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) a += __expf(f[j] - m);
    s += a;
  }
#pragma unroll
  for (int j = 0; j < K; ++j) cnt += (f[j] > tv || (f[j] == tv && col + j < t)) ? 1 : 0;
}

// The body of both shapes: columns [c0, c1) of one row, reduced over the NT threads of the workgroup. c0 is a multiple of 8; `vec`:
// the row starts 16-byte aligned, so whole groups of 8 columns go through one 16-byte load each. Thread 0 returns the result.
template <int NT>
__device__ __forceinline__ void slice_stats(const bf16_t* __restrict__ lg, int c0, int c1, bool vec, float tv, int t, float& m,
                                            float& s, int& cnt) {
  __shared__ float red_m[NT / 64], red_s[NT / 64];
  __shared__ int red_c[NT / 64];
  const int tid = threadIdx.x;
  m = -INFINITY;
  s = 0.f;
  cnt = 0;
  int tail0 = c0;
  if (vec && c1 > c0) {
    const int g1 = c1 >> 3;            // whole groups only: the last, partial one is the scalar tail (nothing past c1 <= V is loaded)
#pragma unroll 2
    for (int g = (c0 >> 3) + tid; g < g1; g += NT) {
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(lg + (long)g * 8), f);
      lse_take<8>(f, g * 8, tv, t, m, s, cnt);
    }
    tail0 = max(c0, g1 * 8);
  }
  for (int j = tail0 + tid; j < c1; j += NT) {
    const float f = bf2f(lg[j]);
    lse_take<1>(&f, j, tv, t, m, s, cnt);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if ((tid & 63) == 0) { red_m[tid >> 6] = m; red_s[tid >> 6] = s; red_c[tid >> 6] = cnt; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < NT / 64; ++k) {
      lse_merge(m, s, red_m[k], red_s[k]);
      cnt += red_c[k];
    }
  }
}

// Where a row's results go. Plain form: logprob / lse / rank are [n]. Step form (step != NULL): logprob / rank are [B, cols] and the
// column is *step - off; `done` is this kernel's own copy of the finished flags as they stood BEFORE the pick it follows.
struct LpOut {
  float* logprob;
  float* lse;
  int32_t* rank;
  const int32_t* step;
  const int32_t* finished;
  int32_t* done;
  int off, cols;
};

__device__ __forceinline__ void write_row(const LpOut& o, int row, float m, float s, int cnt, float tv, bool valid) {
  const float lse = m + logf(s);       // a row that is -inf throughout: m = -inf, s = 0, lse = -inf
  float lp = valid ? (tv == -INFINITY ? -INFINITY : tv - lse) : 0.f;   // (-inf - -inf would be NaN there: such a row gives -inf too)
  int rk = valid ? cnt : -1;
  if (o.step == nullptr) {
    o.logprob[row] = lp;
    if (o.lse) o.lse[row] = lse;
    if (o.rank) o.rank[row] = rk;
    return;
  }
  // a row that had finished before this step's pick emitted a pad: exactly 0. The step that emits the eos itself is a real one.
  const bool was_done = o.done[row] != 0;
  o.done[row] = o.finished[row];
  const int col = *o.step - o.off;
  if (col < 0 || col >= o.cols) return;
  if (was_done) { lp = 0.f; rk = -1; }
  o.logprob[(long)row * o.cols + col] = lp;
  if (o.rank) o.rank[(long)row * o.cols + col] = rk;
}

__device__ __forceinline__ float target_logit(const bf16_t* lg, int t, int V, bool& valid) {
  valid = (unsigned)t < (unsigned)V;   // -100 and anything else outside [0, V) never indexes memory
  return valid ? bf2f(lg[t]) : __builtin_nanf("");
}

// grid (nsl, n). nsl == 1: the workgroup writes the row's results; else its partial (pm / ps / pc are [n, nsl]).
template <int NT>
__global__ __launch_bounds__(NT) void logprob_slice_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                           const int32_t* __restrict__ targets, int per, bool vec,
                                                           float* __restrict__ pm, float* __restrict__ ps, int32_t* __restrict__ pc,
                                                           LpOut out) {
  const int row = blockIdx.y, sl = blockIdx.x, nsl = gridDim.x;
  const bf16_t* lg = logits + (long)row * ld;
  const int t = targets[row];
  bool valid;
  const float tv = target_logit(lg, t, V, valid);
  const int c0 = min(V, sl * per), c1 = min(V, c0 + per);
  float m, s;
  int cnt;
  slice_stats<NT>(lg, c0, c1, vec, tv, t, m, s, cnt);
  if (threadIdx.x != 0) return;
  if (nsl == 1) {
    write_row(out, row, m, s, cnt, tv, valid);
  } else {
    pm[(long)row * nsl + sl] = m;
    ps[(long)row * nsl + sl] = s;
    pc[(long)row * nsl + sl] = cnt;
  }
}

// grid n, one wave: lane k holds partial k (nsl <= 64); a butterfly in a fixed order, lane 0 writes.
__global__ __launch_bounds__(64) void logprob_combine_kernel(const bf16_t* __restrict__ logits, long ld, int V,
                                                             const int32_t* __restrict__ targets, int nsl,
                                                             const float* __restrict__ pm, const float* __restrict__ ps,
                                                             const int32_t* __restrict__ pc, LpOut out) {
  const int row = blockIdx.x, lane = threadIdx.x;
  float m = -INFINITY, s = 0.f;
  int cnt = 0;
  if (lane < nsl) { m = pm[(long)row * nsl + lane]; s = ps[(long)row * nsl + lane]; cnt = pc[(long)row * nsl + lane]; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane != 0) return;
  bool valid;
  const float tv = target_logit(logits + (long)row * ld, targets[row], V, valid);
  write_row(out, row, m, s, cnt, tv, valid);
}

// slices == 0: the measured choice
int pick_slices(int n, int slices) {
  if (slices > 0) return slices;
  return n >= LP_ROWS_SWITCH ? 1 : LP_SLICES;
}

int launch_logprob(const char* name, const void* logits, int64_t ld, int n, int V, const int32_t* targets, int nsl, void* work,
                   const LpOut& out, hipStream_t s) {
  const bool vec = (uintptr_t)logits % 16 == 0 && ld % 8 == 0;
  const bf16_t* lg = (const bf16_t*)logits;
  if (nsl == 1) {
    hipLaunchKernelGGL(logprob_slice_kernel<1024>, dim3(1, n), dim3(1024), 0, s, lg, (long)ld, V, targets, V, vec, (float*)nullptr,
                       (float*)nullptr, (int32_t*)nullptr, out);
  } else {
    // work: [n * nsl] maxima, [n * nsl] sums (f32), [n * nsl] counts (i32)
    float* pm = (float*)work;
    float* ps = pm + (long)n * nsl;
    int32_t* pc = (int32_t*)(ps + (long)n * nsl);
    const int per = ((V + nsl - 1) / nsl + 7) / 8 * 8;       // slices start on a multiple of 8 columns: 16-byte loads stay aligned
    hipLaunchKernelGGL(logprob_slice_kernel<256>, dim3(nsl, n), dim3(256), 0, s, lg, (long)ld, V, targets, per, vec, pm, ps, pc, out);
    hipLaunchKernelGGL(logprob_combine_kernel, dim3(n), dim3(64), 0, s, lg, (long)ld, V, targets, nsl, pm, ps, pc, out);
  }
  VQ3_CHECK_LAUNCH(name);
  return 0;
}

}  // namespace

extern "C" int vq3_token_logprob(const void* logits_bf16, int64_t ld_logits, int32_t n, int32_t V, const int32_t* targets,
                                 float* logprob_f32, float* lse_f32, int32_t* rank_i32, void* work, int32_t slices, void* stream) {
  VQ3_CHECK_ARG(logits_bf16 && targets && logprob_f32, "token_logprob: null pointer");
  VQ3_CHECK_ARG(n > 0 && V > 0 && ld_logits >= V, "token_logprob: bad shape (n %d, V %d, ld %lld: need n > 0 and ld >= V > 0)", n, V,
                (long long)ld_logits);
  VQ3_CHECK_ARG(n <= 65535, "token_logprob: at most 65535 rows per call, got %d", n);
  VQ3_CHECK_ARG(slices >= 0 && slices <= LP_SLICES, "token_logprob: slices must be 0 (automatic) or 1..%d, got %d", LP_SLICES, slices);
  const int nsl = pick_slices(n, slices);
  VQ3_CHECK_ARG(nsl == 1 || work, "token_logprob: null pointer (work is needed when the vocabulary is split)");
  const LpOut out = {logprob_f32, lse_f32, rank_i32, nullptr, nullptr, nullptr, 0, 0};
  return launch_logprob("token_logprob", logits_bf16, ld_logits, n, V, targets, nsl, work, out, (hipStream_t)stream);
}

extern "C" int vq3_token_logprob_step(const void* logits_bf16, int64_t ld_logits, int32_t B, int32_t V, const int32_t* next_ids,
                                      const int32_t* step, int32_t prompt_offset, const int32_t* finished, int32_t* done,
                                      float* logprob_f32, int32_t* rank_i32, int32_t cols, void* work, void* stream) {
  VQ3_CHECK_ARG(logits_bf16 && next_ids && step && finished && done && logprob_f32 && work, "token_logprob_step: null pointer");
  VQ3_CHECK_ARG(B > 0 && B <= 65535 && V > 0 && ld_logits >= V && cols > 0 && prompt_offset >= 0,
                "token_logprob_step: bad shape (B %d, V %d, ld %lld, cols %d, prompt offset %d)", B, V, (long long)ld_logits, cols,
                prompt_offset);
  const LpOut out = {logprob_f32, nullptr, rank_i32, step, finished, done, prompt_offset, cols};
  return launch_logprob("token_logprob_step", logits_bf16, ld_logits, B, V, next_ids, pick_slices(B, 0), work, out,
                        (hipStream_t)stream);
}
