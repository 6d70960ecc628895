// Beam search for Qwen3 with a resident KV cache: transformers 5.15 GenerationMixin._beam_search (the vectorised, static-shape form,
// do_sample=False), as the step that replaces the pick of decode.hip. Row b * num_beams + j is beam j of prompt b; at most 8 rows,
// 4 prompts, K = max(2, 1 + n_eos) * num_beams <= 32 candidates per prompt. Every quantity that varies per step is read from device
// memory, so both entries sit in the captured step.
//
//  * vq3_beam_step     three launches.
//      1. grid (64, R): (max, sum exp) of one vocabulary slice of one row (logprob.hip's split shape).
//      2. grid (64, R): the row's logsumexp from the 64 partials (a fixed butterfly: every workgroup of a row gets the same bits); the
//         slice's acc = (z - lse) + run_score staged in LDS; the repetition penalty and the n-gram ban - applied to the LOG-PROBABILITY,
//         as transformers does in beam search - written over the staged values (idempotent stores: no overlay table, no atomics); then
//         K rounds of workgroup arg-max leave the slice's top K as (value, flat index parent * V + token), best first, -inf padded.
//      3. one workgroup: wave p merges the nb * 64 sorted lists of prompt p to its top K (a lane owns slice `lane` of every beam), lane 0
//         runs the bookkeeping of the reference (stopping criteria, next running beams, finished slots, early-stopping heuristic, loop
//         condition); the sequences are gathered through LDS - all rows are read before any is written.
//     Order everywhere: the higher value first, then the smaller flat index (candidates) or the smaller rank (the two selections
//     among the K candidates; in the finished-slot merge the old slots come before the candidates). No atomics; the same bits run
//     after run.
//     Steps replayed after all_done is set change nothing: every kernel returns at once. (The reference's own -1e9 terms would keep
//     the finished slots unchanged, but its running beams would move on; the explicit return covers both.)
//  * vq3_beam_reorder  cache row r <- cache row src_row[r], in place, all layers, both operands, positions 0 .. lens inclusive. A
//     thread loads its 16-byte piece of every source row of its prompt, then stores the rows that moved: plain vector loads and
//     stores, nothing for an identity map.
#include <math.h>

#include "common.h"
#include "pick.h"
#include "vq3_hip.h"

namespace {

constexpr int BM_SLICES = 64;                       // vocabulary slices per row (pass 3 gives one to each lane of a wave)
constexpr int BM_KMAX = 32;                         // candidates per prompt: max(2, 1 + 3 eos ids) * 8 beams
constexpr int BM_ROWS = 8, BM_PROMPTS = 4;
constexpr int BM_MAX_IDS = vq3pick::PICK_MAX_IDS;   // columns of run_seq / fin_seq (prompt + new ids), as for the picks
constexpr int BM_SLICE_MAX = 4096;                  // ids per slice that fit the LDS stage: V <= 262 144
constexpr int BM_PAD = 0x7fffffff;                  // the index of a list entry that does not exist
constexpr float BM_NEG = -1.0e9f;
static_assert(VQ3_BEAM_WORK_PER_ROW == BM_SLICES * (2 + 2 * BM_KMAX), "work: per (row, slice) one (max, sum) and K (value, index)");

__device__ __forceinline__ void lse_merge(float& m, float& s, float om, float os) {
  const float M = fmaxf(m, om);
  if (M == -INFINITY) return;
  s = s * __expf(m - M) + os * __expf(om - M);
  m = M;
}
// (ov, oi) comes before (v, i)
__device__ __forceinline__ bool before(float ov, int oi, float v, int i) { return ov > v || (ov == v && oi < i); }

__device__ __forceinline__ void wave_best(float& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o, 64);
    const int oi = __shfl_xor(i, o, 64);
    if (before(ov, oi, v, i)) { v = ov; i = oi; }
  }
}

// ------------------------------------------------------------------------------------------------ pass 1: (max, sum exp) per slice
__global__ __launch_bounds__(256) void beam_lse_partial_kernel(const bf16_t* __restrict__ logits, long ld, int V, int per, bool vec,
                                                               const int32_t* __restrict__ all_done, float* __restrict__ pm,
                                                               float* __restrict__ ps) {
  __shared__ float red_m[4], red_s[4];
  if (*all_done != 0) return;
  const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
  const bf16_t* lg = logits + (long)row * ld;
  const int c0 = min(V, sl * per), c1 = min(V, c0 + per);
  float m = -INFINITY, s = 0.f;
  int tail0 = c0;
  if (vec && c1 > c0) {                 // c0 is a multiple of 8; whole groups of 8 only, nothing at or past c1 <= V is loaded
    const int g1 = c1 >> 3;
    for (int g = (c0 >> 3) + tid; g < g1; g += 256) {
      float f[8];
      unpack8(*reinterpret_cast<const u32x4*>(lg + (long)g * 8), f);
      float mk = f[0];
#pragma unroll
      for (int j = 1; j < 8; ++j) mk = fmaxf(mk, f[j]);
      if (mk > -INFINITY) {
        float a = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) a += __expf(f[j] - mk);
        lse_merge(m, s, mk, a);
      }
    }
    tail0 = max(c0, g1 * 8);
  }
  for (int j = tail0 + tid; j < c1; j += 256) {
    const float f = bf2f(lg[j]);
    if (f > -INFINITY) lse_merge(m, s, f, 1.f);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
  if ((tid & 63) == 0) { red_m[tid >> 6] = m; red_s[tid >> 6] = s; }
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < 4; ++k) lse_merge(m, s, red_m[k], red_s[k]);
    pm[row * BM_SLICES + sl] = m;
    ps[row * BM_SLICES + sl] = s;
  }
}

// ------------------------------------------------------------------------------------------------ pass 2: top K of a slice
__global__ __launch_bounds__(256) void beam_slice_topk_kernel(const bf16_t* __restrict__ logits, long ld, int V, int per, int nb, int K,
                                                              const int32_t* __restrict__ step_p, const int32_t* __restrict__ all_done,
                                                              const int32_t* __restrict__ run_seq, int max_len,
                                                              const float* __restrict__ run_score, float penalty, int ngram,
                                                              const float* __restrict__ pm, const float* __restrict__ ps,
                                                              float* __restrict__ cv, int32_t* __restrict__ ci) {
  __shared__ float sv[BM_SLICE_MAX];
  __shared__ float s_lse;
  __shared__ float rv[4];
  __shared__ int ri[4];
  if (*all_done != 0) return;
  const int row = blockIdx.y, sl = blockIdx.x, tid = threadIdx.x;
  const int step = min(*step_p, max_len);
  const bf16_t* lg = logits + (long)row * ld;
  const int32_t* g = run_seq + (long)row * max_len;
  const int c0 = min(V, sl * per), c1 = min(V, c0 + per), n = c1 - c0;
  if (tid < 64) {
    float m = pm[row * BM_SLICES + tid], s = ps[row * BM_SLICES + tid];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) lse_merge(m, s, __shfl_xor(m, o, 64), __shfl_xor(s, o, 64));
    if (tid == 0) s_lse = m + logf(s);
  }
  __syncthreads();
  const float lse = s_lse, score = run_score[row];
  for (int i = tid; i < n; i += 256) sv[i] = (bf2f(lg[c0 + i]) - lse) + score;
  __syncthreads();
  // repetition penalty on the log-probability of every id of the running sequence: recomputed from the logit, so the stores of a
  // repeated id all carry the same value
  if (penalty != 1.0f) {
    for (int i = tid; i < step; i += 256) {
      const int t = g[i];
      if (t < c0 || t >= c1) continue;
      const float lp = bf2f(lg[t]) - lse;
      sv[t - c0] = (lp < 0.f ? __fmul_rn(lp, penalty) : __fdiv_rn(lp, penalty)) + score;
    }
  }
  __syncthreads();
  // n-gram ban (NoRepeatNGramLogitsProcessor): the id that followed an earlier occurrence of the last ngram - 1 ids
  if (ngram > 0 && step + 1 >= ngram) {
    const int pre = ngram - 1;
    for (int i = tid; i + ngram <= step; i += 256) {
      const int t = g[i + pre];
      if (t < c0 || t >= c1) continue;
      bool match = true;
      for (int j = 0; j < pre; ++j) match &= (g[i + j] == g[step - pre + j]);
      if (match) sv[t - c0] = -INFINITY;
    }
  }
  __syncthreads();
  const long out = ((long)row * BM_SLICES + sl) * BM_KMAX;
  const int flat0 = (row % nb) * V + c0;
  for (int k = 0; k < K; ++k) {
    float best = -INFINITY;
    int bi = BM_PAD;
    for (int i = tid; i < n; i += 256) {
      const float v = sv[i];
      if (v > best) { best = v; bi = i; }      // ascending i: the smallest index of equal values; -inf (banned, taken) is never live
    }
    wave_best(best, bi);
    if ((tid & 63) == 0) { rv[tid >> 6] = best; ri[tid >> 6] = bi; }
    __syncthreads();
    best = rv[0];
    bi = ri[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
      if (before(rv[w], ri[w], best, bi)) { best = rv[w]; bi = ri[w]; }
    if (tid == 0) {
      cv[out + k] = best;
      ci[out + k] = bi == BM_PAD ? BM_PAD : flat0 + bi;
      if (bi != BM_PAD) sv[bi] = -INFINITY;
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------------------------------------ pass 3: merge + bookkeeping
struct BeamArgs {
  const int32_t* step;
  int32_t* run_seq;
  float* run_score;
  int32_t* fin_seq;
  float* fin_score;
  int32_t* fin_len;
  int32_t* fin_flag;
  int32_t* heur;
  int32_t* all_done;
  int32_t* next_ids;
  int32_t* src_row;
  int32_t* trace_parent;
  int32_t* trace_token;
  float* trace_score;
  const float* cv;
  const int32_t* ci;
  int V, B, nb, K, max_len, prompt_len, trace_rows, n_eos, eos[3], early;
  float length_penalty;
};

__global__ __launch_bounds__(256) void beam_final_kernel(BeamArgs a) {
  __shared__ int s_run[BM_ROWS * BM_MAX_IDS], s_fin[BM_ROWS * BM_MAX_IDS];      // every row is read before any is written
  __shared__ float c_v[BM_PROMPTS][BM_KMAX], c_run[BM_PROMPTS][BM_KMAX], c_fin[BM_PROMPTS][BM_KMAX];
  __shared__ int c_i[BM_PROMPTS][BM_KMAX], c_hit[BM_PROMPTS][BM_KMAX];
  __shared__ float m_score[BM_PROMPTS][BM_ROWS + BM_KMAX];
  __shared__ float n_run_score[BM_ROWS], n_fin_score[BM_ROWS];
  __shared__ int n_parent[BM_ROWS], n_token[BM_ROWS], n_fin_len[BM_ROWS], n_fin_flag[BM_ROWS];
  __shared__ int n_fin_old[BM_ROWS], n_fin_parent[BM_ROWS], n_fin_token[BM_ROWS];   // old: the slot (row) it was, or -1: a candidate
  __shared__ int p_heur[BM_PROMPTS], p_all_hit[BM_PROMPTS], p_all_fin[BM_PROMPTS];
  if (*a.all_done != 0) return;
  const int cur = *a.step;
  if (cur < 0 || cur >= a.max_len) return;          // no column left for another id (the last step sets all_done: not reached)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int R = a.B * a.nb, nb = a.nb, K = a.K, V = a.V, ML = a.max_len;
  for (int i = tid; i < R * ML; i += 256) {
    const int r = i / ML, c = i - r * ML;
    if (c < cur) s_run[r * BM_MAX_IDS + c] = a.run_seq[i];
    s_fin[r * BM_MAX_IDS + c] = a.fin_seq[i];
  }
  if (wid < a.B) {
    const int p = wid, r0 = p * nb;
    // ---- merge: lane owns the list of slice `lane` of each of the prompt's beams; heads live in registers
    float hv[BM_ROWS];
    int hi[BM_ROWS], hp[BM_ROWS];
#pragma unroll
    for (int j = 0; j < BM_ROWS; ++j) {
      hv[j] = -INFINITY; hi[j] = BM_PAD; hp[j] = 0;
      if (j < nb) {
        const long base = ((long)(r0 + j) * BM_SLICES + lane) * BM_KMAX;
        hv[j] = a.cv[base]; hi[j] = a.ci[base];
      }
    }
    for (int k = 0; k < K; ++k) {
      float best = hv[0];
      int bi = hi[0];
#pragma unroll
      for (int j = 1; j < BM_ROWS; ++j)
        if (before(hv[j], hi[j], best, bi)) { best = hv[j]; bi = hi[j]; }
      wave_best(best, bi);
      if (lane == 0) { c_v[p][k] = best; c_i[p][k] = bi; }
      if (bi != BM_PAD) {
#pragma unroll
        for (int j = 0; j < BM_ROWS; ++j) {
          if (j < nb && hi[j] == bi) {               // flat indices are unique: one list of one lane
            hp[j] += 1;
            const long base = ((long)(r0 + j) * BM_SLICES + lane) * BM_KMAX;
            hv[j] = hp[j] < K ? a.cv[base + hp[j]] : -INFINITY;
            hi[j] = hp[j] < K ? a.ci[base + hp[j]] : BM_PAD;
          }
        }
      }
    }
    // ---- the reference's bookkeeping, serial: K <= 32 candidates, nb <= 8 beams
    if (lane == 0) {
      const float lpow = a.length_penalty;
      const bool last = cur + 1 == ML;
      bool all_hit = true;
      // d. stopping criteria; e. the running beams of the next step: top nb of acc + hit * -1e9
      for (int c = 0; c < K; ++c) {
        const int fi = c_i[p][c];
        const int tok = fi == BM_PAD ? 0 : fi % V;
        bool hit = last;
        for (int e = 0; e < a.n_eos; ++e) hit |= tok == a.eos[e];
        c_hit[p][c] = hit;
        all_hit &= hit;
        c_run[p][c] = c_v[p][c] + (hit ? BM_NEG : 0.f);
      }
      unsigned taken = 0;
      for (int j = 0; j < nb; ++j) {
        int bc = -1;
        for (int c = 0; c < K; ++c)
          if (!((taken >> c) & 1u) && (bc < 0 || c_run[p][c] > c_run[p][bc])) bc = c;
        taken |= 1u << bc;
        const int fi = c_i[p][bc];
        n_parent[r0 + j] = r0 + (fi == BM_PAD ? 0 : fi / V);
        n_token[r0 + j] = fi == BM_PAD ? 0 : fi % V;
        n_run_score[r0 + j] = c_run[p][bc];
      }
      // f. _update_finished_beams: the adds in the reference's order, each rounded to f32
      const float div = powf((float)(cur + 1 - a.prompt_len), lpow);
      bool full = true;
      for (int j = 0; j < nb; ++j) full &= a.fin_flag[r0 + j] != 0;
      const bool heur_old = a.heur[p] != 0;
      for (int j = 0; j < nb; ++j) m_score[p][j] = a.fin_score[r0 + j];
      for (int c = 0; c < K; ++c) {
        float f = c_v[p][c] / div;
        f += (full && a.early == 1) ? BM_NEG : 0.f;
        f += heur_old ? 0.f : BM_NEG;
        f += (c_hit[p][c] && c < nb) ? 0.f : BM_NEG;
        c_fin[p][c] = f;
        m_score[p][nb + c] = f;
      }
      unsigned long long mtaken = 0;
      bool all_fin = true;
      float min_fin = INFINITY;
      for (int j = 0; j < nb; ++j) {
        int bm = -1;
        for (int m = 0; m < nb + K; ++m)
          if (!((mtaken >> m) & 1ull) && (bm < 0 || m_score[p][m] > m_score[p][bm])) bm = m;
        mtaken |= 1ull << bm;
        const int r = r0 + j;
        n_fin_score[r] = m_score[p][bm];
        if (bm < nb) {
          n_fin_old[r] = r0 + bm;
          n_fin_len[r] = a.fin_len[r0 + bm];
          n_fin_flag[r] = a.fin_flag[r0 + bm];
        } else {
          const int c = bm - nb, fi = c_i[p][c];
          n_fin_old[r] = -1;
          n_fin_parent[r] = r0 + (fi == BM_PAD ? 0 : fi / V);
          n_fin_token[r] = fi == BM_PAD ? 0 : fi % V;
          n_fin_len[r] = cur + 1;
          n_fin_flag[r] = (c_hit[p][c] && c < nb) ? 1 : 0;
        }
        all_fin &= n_fin_flag[r] != 0;
        min_fin = fminf(min_fin, n_fin_score[r]);
      }
      // _check_early_stop_heuristic, at cur_len + 1
      const int hyp = (a.early == 2 && lpow > 0.f) ? ML - a.prompt_len : cur + 1 - a.prompt_len;
      const float best_run = n_run_score[r0] / powf((float)hyp, lpow);
      bool any = false;
      for (int j = 0; j < nb; ++j) any |= best_run > (n_fin_flag[r0 + j] ? min_fin : BM_NEG);
      p_heur[p] = (heur_old && any) ? 1 : 0;
      p_all_hit[p] = all_hit;
      p_all_fin[p] = all_fin;
    }
  }
  __syncthreads();
  // ---- sequences: new running row r = its parent's ids + the new id; a finished slot = an old slot, or a candidate's sequence
  for (int i = tid; i < R * ML; i += 256) {
    const int r = i / ML, c = i - r * ML;
    if (c < cur) {
      if (n_parent[r] != r) a.run_seq[i] = s_run[n_parent[r] * BM_MAX_IDS + c];
    } else if (c == cur) {
      a.run_seq[i] = n_token[r];
    }
    const int old = n_fin_old[r];
    if (old >= 0) {
      if (old != r && c < n_fin_len[r]) a.fin_seq[i] = s_fin[old * BM_MAX_IDS + c];
    } else if (c < cur) {
      a.fin_seq[i] = s_run[n_fin_parent[r] * BM_MAX_IDS + c];
    } else if (c == cur) {
      a.fin_seq[i] = n_fin_token[r];
    }
  }
  const int t = cur - a.prompt_len;
  if (tid < R) {
    const int r = tid;
    a.run_score[r] = n_run_score[r];
    a.fin_score[r] = n_fin_score[r];
    a.fin_len[r] = n_fin_len[r];
    a.fin_flag[r] = n_fin_flag[r];
    a.next_ids[r] = n_token[r];
    a.src_row[r] = n_parent[r];
    if (a.trace_parent && t >= 0 && t < a.trace_rows) {
      a.trace_parent[(long)t * R + r] = n_parent[r];
      a.trace_token[(long)t * R + r] = n_token[r];
      a.trace_score[(long)t * R + r] = n_run_score[r];
    }
  }
  if (tid == 0) {
    // _beam_search_has_unfinished_sequences, over the whole batch
    bool improve = false, all_fin = true, all_hit = true;
    for (int p = 0; p < a.B; ++p) {
      a.heur[p] = p_heur[p];
      improve |= p_heur[p] != 0;
      all_fin &= p_all_fin[p] != 0;
      all_hit &= p_all_hit[p] != 0;
    }
    const bool unfinished = improve && !(all_fin && a.early == 1) && !all_hit;
    if (!unfinished) *a.all_done = 1;
  }
}

// ------------------------------------------------------------------------------------------------ cache reorder
// grid (chunks of 256 * U pieces, layers * Hkv, prompts * 2 operands). A piece is 16 bytes; a (row, head)'s positions 0 .. L are one
// contiguous run of (L + 1) * 16 pieces. The map is uniform over the workgroup: branches on it are scalar.
constexpr int RO_U = 2;

__global__ __launch_bounds__(256) void beam_reorder_kernel(bf16_t* __restrict__ Kc, bf16_t* __restrict__ Vc,
                                                           const int32_t* __restrict__ src_row, const int32_t* __restrict__ lens,
                                                           const int32_t* __restrict__ all_done, int R, int nb, int Hkv, int Lmax) {
  if (all_done != nullptr && *all_done != 0) return;
  const int p = blockIdx.z >> 1, r0 = p * nb;
  int src[BM_ROWS];
  unsigned need = 0;
#pragma unroll
  for (int j = 0; j < BM_ROWS; ++j) {
    int s = j;
    if (j < nb) {
      s = src_row[r0 + j] - r0;
      if (s < 0 || s >= nb) s = j;                  // never index outside the prompt's rows
    }
    src[j] = s;
    if (s != j) need |= 1u << s;
  }
  if (need == 0) return;
  const int L = min(max(lens[r0], 0), Lmax - 1);
  const int npieces = (L + 1) * 16;
  const int first = blockIdx.x * 256 * RO_U;
  if (first >= npieces) return;
  const int layer = blockIdx.y / Hkv, head = blockIdx.y - layer * Hkv;
  bf16_t* base = (blockIdx.z & 1) ? Vc : Kc;
  const long row_stride = (long)Hkv * Lmax * 128;
  base += ((long)layer * R + r0) * row_stride + (long)head * Lmax * 128;
  u32x4 v[RO_U][BM_ROWS];
#pragma unroll
  for (int u = 0; u < RO_U; ++u) {
    const int piece = first + u * 256 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < BM_ROWS; ++j)
    {
      v[u][j] = u32x4{0u, 0u, 0u, 0u};
      if (((need >> j) & 1u) && piece < npieces) v[u][j] = *reinterpret_cast<const u32x4*>(base + j * row_stride + (long)piece * 8);
    }
  }
#pragma unroll
  for (int u = 0; u < RO_U; ++u) {
    const int piece = first + u * 256 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < BM_ROWS; ++j) {
      if (j < nb && src[j] != j && piece < npieces) {
        u32x4 o = v[u][0];
#pragma unroll
        for (int s = 1; s < BM_ROWS; ++s)
          if (src[j] == s) o = v[u][s];
        *reinterpret_cast<u32x4*>(base + j * row_stride + (long)piece * 8) = o;
      }
    }
  }
}

}  // namespace

extern "C" int vq3_beam_step(const vq3_beam_step_desc* d, void* stream) {
  VQ3_CHECK_ARG(d && d->logits_bf16 && d->step && d->run_seq && d->run_score && d->fin_seq && d->fin_score && d->fin_len && d->fin_flag &&
                    d->heur && d->all_done && d->next_ids && d->src_row && d->work,
                "beam_step: null pointer");
  VQ3_CHECK_ARG((d->trace_parent != nullptr) == (d->trace_token != nullptr) && (d->trace_parent != nullptr) == (d->trace_score != nullptr),
                "beam_step: the three trace buffers come together or not at all");
  VQ3_CHECK_ARG(d->num_beams >= 2 && d->num_beams <= BM_ROWS, "beam_step: num_beams must be 2..%d, got %d", BM_ROWS, d->num_beams);
  VQ3_CHECK_ARG(d->n_prompts >= 1 && d->n_prompts <= BM_PROMPTS && d->n_prompts * d->num_beams <= BM_ROWS,
                "beam_step: at most %d rows in at most %d prompts, got %d x %d", BM_ROWS, BM_PROMPTS, d->n_prompts, d->num_beams);
  VQ3_CHECK_ARG(d->n_eos >= 0 && d->n_eos <= 3, "beam_step: at most 3 eos ids, got %d", d->n_eos);
  VQ3_CHECK_ARG(d->V > 0 && d->ld_logits >= d->V && d->V <= BM_SLICES * BM_SLICE_MAX, "beam_step: bad shape (V %d, ld %lld; V <= %d)", d->V,
                (long long)d->ld_logits, BM_SLICES * BM_SLICE_MAX);
  VQ3_CHECK_ARG(d->max_len >= 1 && d->max_len <= BM_MAX_IDS, "beam_step: at most %d ids per row (prompt + new), got %d", BM_MAX_IDS,
                d->max_len);
  VQ3_CHECK_ARG(d->prompt_len >= 0 && d->prompt_len < d->max_len && d->trace_rows >= 0, "beam_step: bad prompt_len / trace_rows");
  VQ3_CHECK_ARG(d->repetition_penalty > 0.f, "beam_step: repetition_penalty must be > 0, got %f", (double)d->repetition_penalty);
  VQ3_CHECK_ARG(d->no_repeat_ngram >= 0, "beam_step: no_repeat_ngram must be >= 0");
  VQ3_CHECK_ARG(d->early_stopping >= 0 && d->early_stopping <= 2, "beam_step: early_stopping is 0 (False), 1 (True) or 2 (never)");
  VQ3_CHECK_ARG(fabsf(d->length_penalty) < INFINITY, "beam_step: length_penalty must be finite");
  const int R = d->n_prompts * d->num_beams, nb = d->num_beams, V = d->V;
  const int K = (d->n_eos + 1 > 2 ? d->n_eos + 1 : 2) * nb;
  hipStream_t s = (hipStream_t)stream;
  // work: [R * 64] maxima, [R * 64] sums, [R * 64 * 32] candidate values (f32), [R * 64 * 32] candidate flat indices (i32)
  float* pm = (float*)d->work;
  float* ps = pm + (long)R * BM_SLICES;
  float* cv = ps + (long)R * BM_SLICES;
  int32_t* ci = (int32_t*)(cv + (long)R * BM_SLICES * BM_KMAX);
  const int per = ((V + BM_SLICES - 1) / BM_SLICES + 7) / 8 * 8;     // slices start on a multiple of 8 columns
  const bool vec = (uintptr_t)d->logits_bf16 % 16 == 0 && d->ld_logits % 8 == 0;
  const bf16_t* lg = (const bf16_t*)d->logits_bf16;
  hipLaunchKernelGGL(beam_lse_partial_kernel, dim3(BM_SLICES, R), dim3(256), 0, s, lg, (long)d->ld_logits, V, per, vec, d->all_done, pm,
                     ps);
  hipLaunchKernelGGL(beam_slice_topk_kernel, dim3(BM_SLICES, R), dim3(256), 0, s, lg, (long)d->ld_logits, V, per, nb, K, d->step,
                     d->all_done, d->run_seq, d->max_len, d->run_score, d->repetition_penalty, d->no_repeat_ngram, pm, ps, cv, ci);
  BeamArgs a;
  a.step = d->step; a.run_seq = d->run_seq; a.run_score = d->run_score; a.fin_seq = d->fin_seq; a.fin_score = d->fin_score;
  a.fin_len = d->fin_len; a.fin_flag = d->fin_flag; a.heur = d->heur; a.all_done = d->all_done; a.next_ids = d->next_ids;
  a.src_row = d->src_row; a.trace_parent = d->trace_parent; a.trace_token = d->trace_token; a.trace_score = d->trace_score;
  a.cv = cv; a.ci = ci; a.V = V; a.B = d->n_prompts; a.nb = nb; a.K = K; a.max_len = d->max_len; a.prompt_len = d->prompt_len;
  a.trace_rows = d->trace_rows; a.n_eos = d->n_eos;
  for (int e = 0; e < 3; ++e) a.eos[e] = d->eos_ids[e];
  a.early = d->early_stopping; a.length_penalty = d->length_penalty;
  hipLaunchKernelGGL(beam_final_kernel, dim3(1), dim3(256), 0, s, a);
  VQ3_CHECK_LAUNCH("beam_step");
  return 0;
}

extern "C" int vq3_beam_reorder(void* Kcache, void* Vcache, const int32_t* src_row, const int32_t* lens, const int32_t* all_done,
                                int32_t layers, int32_t n_prompts, int32_t num_beams, int32_t Hkv, int32_t Lmax, int32_t head_dim,
                                void* stream) {
  VQ3_CHECK_ARG(Kcache && Vcache && src_row && lens, "beam_reorder: null pointer");
  VQ3_CHECK_ARG(head_dim == 128, "beam_reorder: head_dim must be 128, got %d", head_dim);
  VQ3_CHECK_ARG(num_beams >= 1 && num_beams <= BM_ROWS && n_prompts >= 1 && n_prompts * num_beams <= 64,
                "beam_reorder: 1..%d beams per prompt, at most 64 rows, got %d x %d", BM_ROWS, n_prompts, num_beams);
  VQ3_CHECK_ARG(layers > 0 && Hkv > 0 && Lmax > 0 && (long)layers * Hkv <= 65535, "beam_reorder: bad shape");
  VQ3_CHECK_ARG((uintptr_t)Kcache % 16 == 0 && (uintptr_t)Vcache % 16 == 0, "beam_reorder: the caches must be 16-byte aligned");
  const int chunks = (Lmax * 16 + 256 * RO_U - 1) / (256 * RO_U);
  hipLaunchKernelGGL(beam_reorder_kernel, dim3(chunks, layers * Hkv, n_prompts * 2), dim3(256), 0, (hipStream_t)stream, (bf16_t*)Kcache,
                     (bf16_t*)Vcache, src_row, lens, all_done, n_prompts * num_beams, num_beams, Hkv, Lmax);
  VQ3_CHECK_LAUNCH("beam_reorder");
  return 0;
}
