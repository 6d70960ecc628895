// Greedy decoding for Qwen3 with a resident KV cache (the reference's inference callers:
// src/inference/qa_inference.py:207-216, arkit_inference.py:274-284 -> transformers generate(), greedy, with
// repetition_penalty and no_repeat_ngram_size). The projections of a step are the skinny GEMMs of skinny_gemm.hip; this
// file holds what runs between them.
//
// All step state lives in device memory (per-row cache lengths, step counter, generated ids, finished flags), so one
// decode step is a fixed sequence of launches with fixed arguments - capturable in a HIP graph and replayed per token.
//
//  * vq3_qwen_decode_qkprep q/k RMSNorm + RoPE at position lens[b], K and V written straight into the cache slot.
//  * vq3_qwen_decode_attn   softmax(q K^T / sqrt(D)) V over the row's lens[b]+1 cached positions, GQA by indexing.
//  * vq3_greedy_pick        repetition penalty -> n-gram ban -> argmax -> eos/pad bookkeeping, one workgroup per row.
//  * vq3_decode_advance     lens[b]++, step++ (single thread; runs last in the step).
#include "common.h"
#include "pick.h"
#include "vq3_hip.h"

namespace {

constexpr int D = 128;

// ------------------------------------------------------------------------------------------------ decode q/k prep
// grid (B, ceil(heads/4)): one head per wave; lane i holds elements i and i+64 (the rotate_half pair)
__global__ __launch_bounds__(256) void decode_qkprep_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ q_w,
                                                           const bf16_t* __restrict__ k_w, const bf16_t* __restrict__ cs,
                                                           const bf16_t* __restrict__ sn, const int32_t* __restrict__ lens,
                                                           bf16_t* __restrict__ Q, bf16_t* __restrict__ Kc,
                                                           bf16_t* __restrict__ Vc, int Hq, int Hkv, int Lmax, float eps) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b = blockIdx.x;
  const int pos = lens[b];
  if (pos >= Lmax) return;   // cache full: the host checks capacity before launching; never write out of bounds
  const int HT = Hq + 2 * Hkv;
  const bf16_t* row = qkv + (long)b * HT * D;
  const float c1 = bf2f(cs[(long)pos * D + lane]), c2 = bf2f(cs[(long)pos * D + lane + 64]);
  const float s1 = bf2f(sn[(long)pos * D + lane]), s2 = bf2f(sn[(long)pos * D + lane + 64]);
  {
    const int h = blockIdx.y * 4 + wid;
    if (h >= HT) return;
    const float x1 = bf2f(row[h * D + lane]), x2 = bf2f(row[h * D + lane + 64]);
    if (h >= Hq + Hkv) {
      bf16_t* o = Vc + (((long)b * Hkv + (h - Hq - Hkv)) * Lmax + pos) * D;
      o[lane] = f2bf(x1);
      o[lane + 64] = f2bf(x2);
      return;
    }
    const bool isq = h < Hq;
    const bf16_t* w = isq ? q_w : k_w;
    const float rs = rsqrtf(wave_sum(x1 * x1 + x2 * x2) / (float)D + eps);
    const float n1 = rbf(bf2f(w[lane]) * rbf(x1 * rs));
    const float n2 = rbf(bf2f(w[lane + 64]) * rbf(x2 * rs));
    const float o1 = rbf(rbf(n1 * c1) + rbf(-n2 * s1));
    const float o2 = rbf(rbf(n2 * c2) + rbf(n1 * s2));
    bf16_t* o = isq ? Q + ((long)b * Hq + h) * D : Kc + (((long)b * Hkv + (h - Hq)) * Lmax + pos) * D;
    o[lane] = f2bf(o1);
    o[lane + 64] = f2bf(o2);
  }
}

// ------------------------------------------------------------------------------------------------ decode attention
// one block (4 waves) per (b, q-head); T = lens[b] + 1 keys. 16 lanes x 16 bytes cover one 128-element K or V row, so a
// wave handles 4 cache rows per load instruction (fully coalesced 1 KiB) and the block 16. Scores and probabilities
// live in LDS (dynamic: Lmax floats).
__global__ __launch_bounds__(256) void decode_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Kc,
                                                         const bf16_t* __restrict__ Vc, const int32_t* __restrict__ lens,
                                                         bf16_t* __restrict__ O, int Hq, int Hkv, int Lmax, float scale) {
  extern __shared__ float sc[];      // [Lmax] scores, then probabilities
  __shared__ float red[4];
  __shared__ float opart[4][D];
  const int b = blockIdx.x / Hq, h = blockIdx.x % Hq;
  const int hk = h / (Hq / Hkv);
  const int T = min(lens[b] + 1, Lmax);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int sub = lane >> 4, dl = (lane & 15) * 8;     // which of the wave's 4 rows, which 8 elements of the row
  float qf[8];
  unpack8(*(const u32x4*)(Q + ((long)b * Hq + h) * D + dl), qf);
  const bf16_t* Kb = Kc + ((long)b * Hkv + hk) * Lmax * D;
  const bf16_t* Vb = Vc + ((long)b * Hkv + hk) * Lmax * D;
  float mx = -INFINITY;
  for (int l0 = wid * 4; l0 < T; l0 += 64) {          // 4 row-quads per trip: their loads are issued together
    u32x4 kr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) kr[i] = *(const u32x4*)(Kb + (long)min(l0 + 16 * i + sub, T - 1) * D + dl);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int l = l0 + 16 * i + sub;
      float kf[8];
      unpack8(kr[i], kf);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) s = fmaf(qf[j], kf[j], s);
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      s *= scale;                     // fp32 scores, like the prefill path's QK^T GEMM (alpha applied in fp32)
      if (l < T) {
        if ((lane & 15) == 0) sc[l] = s;
        mx = fmaxf(mx, s);
      }
    }
  }
  mx = block_max<4>(mx, red);
  float sum = 0.f;
  for (int l = tid; l < T; l += 256) {
    const float e = __expf(sc[l] - mx);
    sc[l] = e;
    sum += e;
  }
  sum = block_sum<4>(sum, red);
  const float inv = 1.f / sum;
  __syncthreads();
  float of[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) of[j] = 0.f;
  for (int l0 = wid * 4; l0 < T; l0 += 64) {
    u32x4 vr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) vr[i] = *(const u32x4*)(Vb + (long)min(l0 + 16 * i + sub, T - 1) * D + dl);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int l = l0 + 16 * i + sub;
      const float p = l < T ? rbf(sc[l] * inv) : 0.f;   // probabilities are a bf16 tensor before the PV product
      float vf[8];
      unpack8(vr[i], vf);
#pragma unroll
      for (int j = 0; j < 8; ++j) of[j] = fmaf(p, vf[j], of[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    of[j] += __shfl_xor(of[j], 16, 64);
    of[j] += __shfl_xor(of[j], 32, 64);
  }
  if (sub == 0) {
#pragma unroll
    for (int j = 0; j < 8; ++j) opart[wid][dl + j] = of[j];
  }
  __syncthreads();
  if (tid < D) O[((long)b * Hq + h) * D + tid] = f2bf(opart[0][tid] + opart[1][tid] + opart[2][tid] + opart[3][tid]);
}

// ------------------------------------------------------------------------------------------------ greedy pick
// transformers: RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor, argmax, eos/pad handling of
// GenerationMixin._sample (greedy). Phase 1, grid (NCH, B): a block owns one slice of the vocabulary - it applies the
// penalty and the bans that fall into its slice (kept in a small LDS overlay, so the logits are read once and never
// rewritten) and reduces the slice to (best value, smallest index). Phase 2, grid B: combines the NCH partials and
// does the bookkeeping.
constexpr int PICK_NCH = 64;
constexpr int PICK_OVL = 1024;  // overlay capacity per vocabulary slice: <= 512 penalised + <= 512 banned entries

// MASKED: the constraint planes of pick.h, staged for the slice in mw - a masked id is -inf wherever the walk or the penalty meets it
template <bool MASKED>
__device__ __forceinline__ void greedy_pick_partial_body(const bf16_t* __restrict__ logits, long ldl, int V,
                                                         const int64_t* __restrict__ gen, int max_new,
                                                         const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                         float* __restrict__ pval, int32_t* __restrict__ pidx,
                                                         int32_t* __restrict__ overflow, const vq3pick::MaskArgs& m, uint32_t* mw) {
  __shared__ int ov_id[PICK_OVL];
  __shared__ float ov_val[PICK_OVL];
  __shared__ int ov_n;
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int step = *step_p;
  const int per = (V + PICK_NCH - 1) / PICK_NCH;
  const int c0 = c * per, c1 = min(V, c0 + per);
  const bf16_t* lg = logits + (long)b * ldl;
  const int64_t* g = gen + (long)b * max_new;
  if (tid == 0) ov_n = 0;
  if constexpr (MASKED) vq3pick::mask_stage(m, step - m.prompt_cols, c0, c1, mw);
  __syncthreads();
  // penalty: distinct generated ids in this slice (first occurrence only: gather - rescale - scatter semantics)
  if (penalty != 1.0f) {
    for (int i = tid; i < step; i += 256) {
      const long t = g[i];
      if (t < c0 || t >= c1) continue;
      bool first = true;
      for (int j = 0; j < i; ++j) first &= (g[j] != t);
      if (!first) continue;
      float sv = bf2f(lg[t]);
      sv = sv < 0.f ? sv * penalty : sv / penalty;
      if constexpr (MASKED) {
        if (vq3pick::mask_bit(mw, c0, (int)t)) sv = -INFINITY;
      }
      const int at = atomicAdd(&ov_n, 1);
      if (at < PICK_OVL) { ov_id[at] = (int)t; ov_val[at] = sv; }
    }
  }
  __syncthreads();
  const int n_pen = min(ov_n, PICK_OVL);
  // n-gram ban overrides the penalised value: reuse the entry if the id is already in the overlay
  if (ngram > 0 && step + 1 >= ngram) {
    const int pre = ngram - 1;
    for (int i = tid; i + ngram <= step; i += 256) {
      const long t = g[i + pre];
      if (t < c0 || t >= c1) continue;
      bool match = true;
      for (int j = 0; j < pre; ++j) match &= (g[i + j] == g[step - pre + j]);
      if (!match) continue;
      bool found = false;
      for (int k = 0; k < n_pen; ++k)
        if (ov_id[k] == (int)t) { ov_val[k] = -INFINITY; found = true; }
      if (!found) {
        const int at = atomicAdd(&ov_n, 1);
        if (at < PICK_OVL) { ov_id[at] = (int)t; ov_val[at] = -INFINITY; }
      }
    }
  }
  __syncthreads();
  const int n_ov = ov_n;
  if (n_ov > PICK_OVL) {            // cannot happen for max_new <= PICK_OVL; flagged, never silently wrong
    if (tid == 0) atomicExch(overflow, 1);
    return;
  }
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int i = c0 + tid; i < c1; i += 256) {
    float v = bf2f(lg[i]);
    for (int k = 0; k < n_ov; ++k)
      if (ov_id[k] == i) v = ov_val[k];       // duplicates of a banned id all hold -inf; penalised ids are unique
    if constexpr (MASKED) {
      if (vq3pick::mask_bit(mw, c0, i)) v = -INFINITY;
    }
    if (v > best) { best = v; bi = i; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ovv = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ovv > best || (ovv == best && oi < bi)) { best = ovv; bi = oi; }
  }
  if ((tid & 63) == 0) { rv[tid >> 6] = best; ri[tid >> 6] = bi; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k)
      if (rv[k] > best || (rv[k] == best && ri[k] < bi)) { best = rv[k]; bi = ri[k]; }
    pval[b * PICK_NCH + c] = best;
    pidx[b * PICK_NCH + c] = bi;
  }
}

__global__ __launch_bounds__(256) void greedy_pick_partial_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                                  const int64_t* __restrict__ gen, int max_new,
                                                                  const int32_t* __restrict__ step_p, float penalty,
                                                                  int ngram, float* __restrict__ pval,
                                                                  int32_t* __restrict__ pidx, int32_t* __restrict__ overflow) {
  greedy_pick_partial_body<false>(logits, ldl, V, gen, max_new, step_p, penalty, ngram, pval, pidx, overflow, vq3pick::MaskArgs{}, nullptr);
}

__global__ __launch_bounds__(256) void greedy_pick_partial_masked_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                                         const int64_t* __restrict__ gen, int max_new,
                                                                         const int32_t* __restrict__ step_p, float penalty,
                                                                         int ngram, float* __restrict__ pval,
                                                                         int32_t* __restrict__ pidx, int32_t* __restrict__ overflow,
                                                                         vq3pick::MaskArgs m) {
  __shared__ uint32_t mw[vq3pick::MASK_SLICE_WORDS];
  greedy_pick_partial_body<true>(logits, ldl, V, gen, max_new, step_p, penalty, ngram, pval, pidx, overflow, m, mw);
}

__global__ __launch_bounds__(64) void greedy_pick_final_kernel(const float* __restrict__ pval, const int32_t* __restrict__ pidx,
                                                              int64_t* __restrict__ gen, int max_new,
                                                              const int32_t* __restrict__ step_p, int32_t* __restrict__ finished,
                                                              const int64_t* __restrict__ eos_ids, int n_eos, long pad_id,
                                                              int32_t* __restrict__ next_ids) {
  const int b = blockIdx.x, lane = threadIdx.x;
  float best = pval[b * PICK_NCH + lane];
  int bi = pidx[b * PICK_NCH + lane];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
  }
  if (lane == 0) {
    const int step = *step_p;
    long tok = bi == 0x7fffffff ? 0 : bi;
    const bool fin = finished[b] != 0;
    if (fin) tok = pad_id;
    if (step < max_new) gen[(long)b * max_new + step] = tok;
    next_ids[b] = (int32_t)tok;
    bool is_eos = false;
    for (int k = 0; k < n_eos; ++k) is_eos |= (tok == eos_ids[k]);
    if (!fin && is_eos) finished[b] = 1;
  }
}

__global__ void advance_kernel(int32_t* lens, int B, int32_t* step) {
  if (lens && threadIdx.x < B) lens[threadIdx.x] += 1;
  if (step && threadIdx.x == 0) *step += 1;
}

}  // namespace

extern "C" int vq3_qwen_decode_qkprep(const void* qkv, const void* q_w, const void* k_w, const void* cos, const void* sin,
                                      const int32_t* lens, void* Q, void* Kcache, void* Vcache, int32_t B, int32_t Hq,
                                      int32_t Hkv, int32_t Dh, int32_t Lmax, float eps, void* stream) {
  VQ3_CHECK_ARG(qkv && q_w && k_w && cos && sin && lens && Q && Kcache && Vcache, "decode_qkprep: null pointer");
  VQ3_CHECK_ARG(Dh == D, "decode_qkprep: head_dim must be %d, got %d", D, Dh);
  VQ3_CHECK_ARG(B > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Lmax > 0, "decode_qkprep: bad shape");
  hipLaunchKernelGGL(decode_qkprep_kernel, dim3(B, (Hq + 2 * Hkv + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv,
                     (const bf16_t*)q_w, (const bf16_t*)k_w, (const bf16_t*)cos, (const bf16_t*)sin, lens, (bf16_t*)Q,
                     (bf16_t*)Kcache, (bf16_t*)Vcache, Hq, Hkv, Lmax, eps);
  VQ3_CHECK_LAUNCH("decode_qkprep");
  return 0;
}

extern "C" int vq3_qwen_decode_attn(const void* Q, const void* Kcache, const void* Vcache, const int32_t* lens, void* O,
                                    int32_t B, int32_t Hq, int32_t Hkv, int32_t Dh, int32_t Lmax, float scale,
                                    void* stream) {
  VQ3_CHECK_ARG(Q && Kcache && Vcache && lens && O, "decode_attn: null pointer");
  VQ3_CHECK_ARG(Dh == D, "decode_attn: head_dim must be %d, got %d", D, Dh);
  VQ3_CHECK_ARG(B > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0, "decode_attn: bad shape");
  VQ3_CHECK_ARG(Lmax >= 64 && Lmax <= 12288, "decode_attn: cache capacity %d outside [64, 12288]", Lmax);
  hipLaunchKernelGGL(decode_attn_kernel, dim3(B * Hq), dim3(256), (size_t)Lmax * sizeof(float), (hipStream_t)stream,
                     (const bf16_t*)Q, (const bf16_t*)Kcache, (const bf16_t*)Vcache, lens, (bf16_t*)O, Hq, Hkv, Lmax, scale);
  VQ3_CHECK_LAUNCH("decode_attn");
  return 0;
}

extern "C" int vq3_greedy_pick(const void* logits_bf16, int64_t ld_logits, float* work, int32_t B, int32_t V,
                               int64_t* generated, int32_t max_new, const int32_t* step, int32_t* finished,
                               float repetition_penalty, int32_t no_repeat_ngram, const int64_t* eos_ids, int32_t n_eos,
                               int64_t pad_id, int32_t* next_ids, void* stream) {
  VQ3_CHECK_ARG(logits_bf16 && work && generated && step && finished && next_ids, "greedy_pick: null pointer");
  VQ3_CHECK_ARG(B > 0 && V > 0 && max_new > 0 && ld_logits >= V, "greedy_pick: bad shape");
  VQ3_CHECK_ARG(max_new <= PICK_OVL / 2, "greedy_pick: at most %d ids per row (prompt + new), got %d", PICK_OVL / 2, max_new);
  VQ3_CHECK_ARG(repetition_penalty > 0.f, "greedy_pick: repetition_penalty must be > 0, got %f", (double)repetition_penalty);
  VQ3_CHECK_ARG(no_repeat_ngram >= 0 && n_eos >= 0 && (n_eos == 0 || eos_ids), "greedy_pick: bad ngram / eos arguments");
  // work: [B * 64] partial values, [B * 64] partial indices, 1 overflow flag (f32 / i32 slots)
  float* pval = work;
  int32_t* pidx = (int32_t*)(work + (long)B * PICK_NCH);
  int32_t* overflow = pidx + (long)B * PICK_NCH;
  hipLaunchKernelGGL(greedy_pick_partial_kernel, dim3(PICK_NCH, B), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)logits_bf16, (long)ld_logits, V, generated, max_new, step, repetition_penalty,
                     no_repeat_ngram, pval, pidx, overflow);
  hipLaunchKernelGGL(greedy_pick_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pval, pidx, generated, max_new,
                     step, finished, eos_ids, n_eos, (long)pad_id, next_ids);
  VQ3_CHECK_LAUNCH("greedy_pick");
  return 0;
}

extern "C" int vq3_greedy_pick_masked(const void* logits_bf16, int64_t ld_logits, float* work, int32_t B, int32_t V,
                                      int64_t* generated, int32_t max_new, const int32_t* step, int32_t* finished,
                                      float repetition_penalty, int32_t no_repeat_ngram, const int64_t* eos_ids, int32_t n_eos,
                                      int64_t pad_id, int32_t* next_ids, const vq3_pick_mask* mask, void* stream) {
  VQ3_CHECK_ARG(logits_bf16 && work && generated && step && finished && next_ids && mask, "greedy_pick_masked: null pointer");
  VQ3_CHECK_ARG(B > 0 && V > 0 && max_new > 0 && ld_logits >= V, "greedy_pick_masked: bad shape");
  VQ3_CHECK_ARG(max_new <= PICK_OVL / 2, "greedy_pick_masked: at most %d ids per row (prompt + new), got %d", PICK_OVL / 2, max_new);
  VQ3_CHECK_ARG(repetition_penalty > 0.f, "greedy_pick_masked: repetition_penalty must be > 0, got %f", (double)repetition_penalty);
  VQ3_CHECK_ARG(no_repeat_ngram >= 0 && n_eos >= 0 && (n_eos == 0 || eos_ids), "greedy_pick_masked: bad ngram / eos arguments");
  const char* bad = vq3pick::mask_args_error(mask->planes, mask->words, mask->min_new, mask->prompt_cols, V);
  VQ3_CHECK_ARG(bad == nullptr, "greedy_pick_masked: %s", bad);
  VQ3_CHECK_ARG((V + PICK_NCH - 1) / PICK_NCH <= (vq3pick::MASK_SLICE_WORDS - 2) * 32, "greedy_pick_masked: V %d exceeds %d", V,
                PICK_NCH * (vq3pick::MASK_SLICE_WORDS - 2) * 32);
  float* pval = work;                     // work as in vq3_greedy_pick
  int32_t* pidx = (int32_t*)(work + (long)B * PICK_NCH);
  int32_t* overflow = pidx + (long)B * PICK_NCH;
  const vq3pick::MaskArgs m{mask->planes, mask->words, mask->min_new, mask->prompt_cols};
  hipLaunchKernelGGL(greedy_pick_partial_masked_kernel, dim3(PICK_NCH, B), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)logits_bf16, (long)ld_logits, V, generated, max_new, step, repetition_penalty,
                     no_repeat_ngram, pval, pidx, overflow, m);
  hipLaunchKernelGGL(greedy_pick_final_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, pval, pidx, generated, max_new,
                     step, finished, eos_ids, n_eos, (long)pad_id, next_ids);
  VQ3_CHECK_LAUNCH("greedy_pick_masked");
  return 0;
}

// the bookkeeping half of a pick for sample.hip, which brings its own phase 1 (pick.h)
static_assert(PICK_NCH == vq3pick::PICK_SLICES && PICK_OVL / 2 == vq3pick::PICK_MAX_IDS, "pick.h restates this file's constants");
void vq3pick::launch_pick_final(const float* pval, const int32_t* pidx, int64_t* generated, int max_new, const int32_t* step,
                                int32_t* finished, const int64_t* eos_ids, int n_eos, long pad_id, int32_t* next_ids, int B,
                                hipStream_t stream) {
  hipLaunchKernelGGL(greedy_pick_final_kernel, dim3(B), dim3(64), 0, stream, pval, pidx, generated, max_new, step, finished, eos_ids,
                     n_eos, pad_id, next_ids);
}

extern "C" int vq3_decode_advance(int32_t* lens, int32_t B, int32_t* step, void* stream) {
  VQ3_CHECK_ARG((lens || step) && B > 0 && B <= 64, "decode_advance: bad argument");
  hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, lens, B, step);
  VQ3_CHECK_LAUNCH("decode_advance");
  return 0;
}
