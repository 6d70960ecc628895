// Seeded temperature / top-k / top-p sampling for a decode step (transformers GenerationMixin._sample with do_sample=True:
// RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor -> TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper ->
// a draw), on the bf16 logits of vq3_greedy_pick and with its bookkeeping. Contract: include/vq3_hip.h, vq3_sample_pick.
//
// No sort: a bf16 row has at most 65536 distinct values, so an integer histogram over the order-preserving 16-bit key gives both
// cut-offs exactly. Three phases and the shared final kernel of decode.hip, every varying quantity read from device memory:
//   1. sample_hist_kernel, grid (64, B): a block streams one slice of the row and counts its keys (int32 atomics on the row's 65536
//      bins in the workspace). Ids the penalty or the ban has changed are not bf16-exact: they stay out of the histogram.
//   2. sample_walk_kernel, grid B, 1024 threads: thread t owns 64 consecutive bins, highest keys first, plus the changed ids whose
//      value falls between its bins (<= 512 per row, rebuilt here from `generated` and sorted by value). Two passes over the thread's
//      values in descending order, each behind a fixed-order block scan: the count of tokens above gives the top-k cut, the mass above
//      (integer count x exp, summed in f64) the top-p cut. Equal values form one group, so ties stand or fall together. The thread
//      then clears the bins it read: the histogram is zero again when the next step starts.
//   3. sample_draw_kernel, grid (64, B): a block streams its slice again, keeps what reaches the threshold, adds the Philox / Gumbel
//      noise and reduces to (best, smallest index) in the layout of greedy_pick_partial_kernel.
// Nothing depends on the order in which atomics land or on the launch geometry: the counts are integers and every sum has a fixed order.
#include "common.h"
#include "pick.h"
#include "vq3_hip.h"

#include <math.h>

namespace {

using vq3pick::PICK_SLICES;
constexpr int OVL = 2 * vq3pick::PICK_MAX_IDS;   // overlay capacity: <= 512 penalised + <= 512 banned entries
constexpr int BINS = 65536;
constexpr int WALK_THREADS = 1024;
constexpr int WALK_WAVES = WALK_THREADS / 64;
constexpr int PER_THREAD = BINS / WALK_THREADS;  // 64 bins per thread
constexpr int THR_SLOT = BINS;                   // the row's threshold (f32) follows its bins in the workspace
static_assert(VQ3_SAMPLE_WORK_PER_ROW >= BINS + 1, "the workspace row holds the histogram and the threshold");
static_assert(PER_THREAD == 64, "the walk marks a thread's nonempty bins in one 64-bit mask");

// order-preserving key of a bf16 value (larger value = larger key); -0 is +0; -1 for what is never kept (NaN, -inf)
__device__ __forceinline__ int key_of(bf16_t u) {
  if ((u & 0x7fff) > 0x7f80 || u == 0xff80) return -1;
  if (u == 0x8000) u = 0;
  return (u & 0x8000) ? (int)(uint16_t)~u : (int)(u | 0x8000);
}
__device__ __forceinline__ float val_of_key(int k) { return bf2f((k & 0x8000) ? (bf16_t)(k & 0x7fff) : (bf16_t)~k); }
// the value at which the bins from key k upwards start, for the keys that bound a thread's bins (multiples of 64): NaN patterns at
// either end of the key space count as the infinity on their side
__device__ __forceinline__ float bound_of_key(int k) { return k > 0xff80 ? INFINITY : (k <= 0x7f ? -INFINITY : val_of_key(k)); }

// The ids of generated[0, n) that fall into [c0, c1) and whose logit the processors change, as vq3_greedy_pick applies them
// (greedy_pick_partial_kernel): entries [0, n_pen) are the distinct penalised ids (first occurrence; value < 0 ? value * penalty :
// value / penalty), overwritten by -inf where the n-gram ban also hits; entries [n_pen, n_ov) are banned ids that were not penalised.
// Every thread of the block calls it; returns false (block-uniform) on overflow, which max_new <= 512 rules out.
// masked(id): the constraint planes' verdict on an id of [c0, c1) - a penalised id that is masked enters as -inf, never as a finite value.
struct NoMask {
  __device__ __forceinline__ bool operator()(int) const { return false; }
};
template <class MF>
__device__ bool build_overlay(const bf16_t* __restrict__ lg, const int64_t* __restrict__ g, int n, int c0, int c1, float penalty,
                              int ngram, int* ov_id, float* ov_val, int* ov_n, int& n_pen, int& n_ov, MF masked) {
  const int tid = threadIdx.x, nt = blockDim.x;
  if (tid == 0) *ov_n = 0;
  __syncthreads();
  if (penalty != 1.0f) {
    for (int i = tid; i < n; i += nt) {
      const long t = g[i];
      if (t < c0 || t >= c1) continue;
      bool first = true;
      for (int j = 0; j < i; ++j) first &= (g[j] != t);
      if (!first) continue;
      const float sv = bf2f(lg[t]);
      const int at = atomicAdd(ov_n, 1);
      if (at < OVL) { ov_id[at] = (int)t; ov_val[at] = masked((int)t) ? -INFINITY : (sv < 0.f ? sv * penalty : sv / penalty); }
    }
  }
  __syncthreads();
  n_pen = min(*ov_n, OVL);
  if (ngram > 0 && n + 1 >= ngram) {
    const int pre = ngram - 1;
    for (int i = tid; i + ngram <= n; i += nt) {
      const long t = g[i + pre];
      if (t < c0 || t >= c1) continue;
      bool match = true;
      for (int j = 0; j < pre; ++j) match &= (g[i + j] == g[n - pre + j]);
      if (!match) continue;
      bool found = false;
      for (int k = 0; k < n_pen; ++k)
        if (ov_id[k] == (int)t) { ov_val[k] = -INFINITY; found = true; }
      if (!found) {
        const int at = atomicAdd(ov_n, 1);
        if (at < OVL) { ov_id[at] = (int)t; ov_val[at] = -INFINITY; }
      }
    }
  }
  __syncthreads();
  n_ov = *ov_n;
  return n_ov <= OVL;
}

// ------------------------------------------------------------------------------------------------ phase 1: histogram
// the verdict of a slice's staged words (pick.h), for the kernels that stream a slice
struct SliceMask {
  const uint32_t* mw;
  int c0;
  __device__ __forceinline__ bool operator()(int i) const { return vq3pick::mask_bit(mw, c0, i); }
};
// the same from the planes themselves, for the few changed ids the walk meets anywhere in the row
struct RowMask {
  vq3pick::MaskArgs m;
  int n_new;
  __device__ __forceinline__ bool operator()(int i) const { return (vq3pick::mask_word(m, i >> 5, n_new) >> (i & 31)) & 1u; }
};

// MASKED (here and in the draw): a masked id is not counted, so it carries no mass in either cut; mw is the slice's stage
template <bool MASKED>
__device__ __forceinline__ void sample_hist_body(const bf16_t* __restrict__ logits, long ldl, int V, const int64_t* __restrict__ gen,
                                                 int max_new, const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                 int32_t* __restrict__ ws, int32_t* __restrict__ overflow, const vq3pick::MaskArgs& m,
                                                 uint32_t* mw) {
  __shared__ int ov_id[OVL];
  __shared__ float ov_val[OVL];
  __shared__ int ov_n;
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int n = min(*step_p, max_new);
  const int per = (V + PICK_SLICES - 1) / PICK_SLICES;
  const int c0 = min(V, c * per), c1 = min(V, c0 + per);
  const bf16_t* lg = logits + (long)b * ldl;
  int n_pen, n_ov;
  bool fits;
  if constexpr (MASKED) {
    vq3pick::mask_stage(m, *step_p - m.prompt_cols, c0, c1, mw);     // (build_overlay syncs before it reads)
    fits = build_overlay(lg, gen + (long)b * max_new, n, c0, c1, penalty, ngram, ov_id, ov_val, &ov_n, n_pen, n_ov, SliceMask{mw, c0});
  } else {
    fits = build_overlay(lg, gen + (long)b * max_new, n, c0, c1, penalty, ngram, ov_id, ov_val, &ov_n, n_pen, n_ov, NoMask{});
  }
  if (!fits) {
    if (tid == 0) atomicExch(overflow, 1);
    return;
  }
  int32_t* hist = ws + (long)b * VQ3_SAMPLE_WORK_PER_ROW;
  for (int i = c0 + tid; i < c1; i += 256) {
    bool changed = false;
    for (int k = 0; k < n_ov; ++k) changed |= (ov_id[k] == i);
    if constexpr (MASKED) changed |= vq3pick::mask_bit(mw, c0, i);
    const int key = key_of(lg[i]);
    if (!changed && key >= 0) atomicAdd(hist + key, 1);
  }
}

__global__ __launch_bounds__(256) void sample_hist_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                          const int64_t* __restrict__ gen, int max_new,
                                                          const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                          int32_t* __restrict__ ws, int32_t* __restrict__ overflow) {
  sample_hist_body<false>(logits, ldl, V, gen, max_new, step_p, penalty, ngram, ws, overflow, vq3pick::MaskArgs{}, nullptr);
}

__global__ __launch_bounds__(256) void sample_hist_masked_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                                 const int64_t* __restrict__ gen, int max_new,
                                                                 const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                                 int32_t* __restrict__ ws, int32_t* __restrict__ overflow,
                                                                 vq3pick::MaskArgs m) {
  __shared__ uint32_t mw[vq3pick::MASK_SLICE_WORDS];
  sample_hist_body<true>(logits, ldl, V, gen, max_new, step_p, penalty, ngram, ws, overflow, m, mw);
}

// ------------------------------------------------------------------------------------------------ phase 2: the two cut-offs
// exclusive prefix over the block's threads in thread order, and the block total; red holds >= WALK_WAVES values
template <class T>
__device__ __forceinline__ T block_excl_scan(T v, T* red, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T up = __shfl_up(inc, o, 64);
    if (lane >= o) inc += up;
  }
  __syncthreads();
  if (lane == 63) red[w] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < WALK_WAVES; ++i) {
    if (i < w) base += red[i];
    tot += red[i];
  }
  total = tot;
  return base + inc - v;
}

// A thread's values in descending order: its nonempty bins (bit j of `mask`: key key_hi - j, count read from hist) merged with the
// side entries sv[sp, s_end) (sorted descending, every one inside the thread's value range). f(value, count) once per distinct value.
template <class F>
__device__ __forceinline__ void walk_values(unsigned long long mask, const int32_t* hist, int key_hi, const float* sv, int sp, int s_end,
                                            F&& f) {
  while (mask) {
    const int key = key_hi - (__ffsll(mask) - 1);
    mask &= mask - 1;
    const int c = hist[key];
    const float v = val_of_key(key);
    while (sp < s_end && sv[sp] > v) {
      const float x = sv[sp];
      int m = 1;
      while (sp + m < s_end && sv[sp + m] == x) ++m;
      f(x, m);
      sp += m;
    }
    int m = 0;
    while (sp + m < s_end && sv[sp + m] == v) ++m;
    f(v, c + m);
    sp += m;
  }
  while (sp < s_end) {
    const float x = sv[sp];
    int m = 1;
    while (sp + m < s_end && sv[sp + m] == x) ++m;
    f(x, m);
    sp += m;
  }
}

// MASKED: the histogram holds no masked id already; what is left is to keep a penalised id that is masked out of the side values
// (M: nothing, or one vq3pick::MaskArgs - the unmasked instantiation is the kernel as it always was, argument for argument)
template <class... M>
__global__ __launch_bounds__(WALK_THREADS) void sample_walk_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                                   const int64_t* __restrict__ gen, int max_new,
                                                                   const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                                   float temperature, int top_k, float top_p,
                                                                   int32_t* __restrict__ ws, int32_t* __restrict__ overflow,
                                                                   int32_t* __restrict__ n_kept_out, float* __restrict__ min_kept_out,
                                                                   M... m) {
  constexpr bool MASKED = sizeof...(M) == 1;
  __shared__ int ov_id[OVL];
  __shared__ float ov_val[OVL];
  __shared__ int ov_n;
  __shared__ float side[vq3pick::PICK_MAX_IDS];       // the penalised, not banned, finite values, descending
  __shared__ int side_n;
  __shared__ int red_i[WALK_WAVES];
  __shared__ double red_d[WALK_WAVES];
  __shared__ float red_f[WALK_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int n = min(*step_p, max_new);
  int32_t* hist = ws + (long)b * VQ3_SAMPLE_WORK_PER_ROW;
  float* thr_out = (float*)(hist + THR_SLOT);

  // the thread's bins, highest key first: bit j of `mask` = bin key_hi - j holds tokens (a row fills a few thousand of its 65536 bins)
  const int key_hi = BINS - 1 - tid * PER_THREAD, key_lo = key_hi - (PER_THREAD - 1);
  unsigned long long mask = 0;
  int mine = 0;
  {
    const int4* src = (const int4*)(hist + key_lo);
#pragma unroll
    for (int q = 0; q < PER_THREAD / 4; ++q) {
      const int4 v4 = src[q];
      mine += v4.x + v4.y + v4.z + v4.w;
      const unsigned long long nib = (v4.x ? 8ull : 0ull) | (v4.y ? 4ull : 0ull) | (v4.z ? 2ull : 0ull) | (v4.w ? 1ull : 0ull);
      mask |= nib << (PER_THREAD - 4 - 4 * q);          // key key_lo + 4q + e is bit 63 - 4q - e
    }
  }
  // the row's changed ids, then the finite penalised values among them sorted by value
  int n_pen, n_ov;
  bool fits;
  if constexpr (MASKED)
    fits = build_overlay(logits + (long)b * ldl, gen + (long)b * max_new, n, 0, V, penalty, ngram, ov_id, ov_val, &ov_n, n_pen, n_ov,
                         RowMask{m..., *step_p - (m.prompt_cols + ...)});
  else
    fits = build_overlay(logits + (long)b * ldl, gen + (long)b * max_new, n, 0, V, penalty, ngram, ov_id, ov_val, &ov_n, n_pen, n_ov,
                         NoMask{});
  if (tid == 0) side_n = 0;
  __syncthreads();
  if (fits) {
    for (int k = tid; k < n_pen; k += WALK_THREADS) {
      const float x = ov_val[k];
      if (x > -INFINITY && x < INFINITY) ov_id[atomicAdd(&side_n, 1)] = k;      // (ov_id is free from here on: it holds positions)
    }
  } else if (tid == 0) {
    atomicExch(overflow, 1);
  }
  __syncthreads();
  const int ns = min(side_n, vq3pick::PICK_MAX_IDS);
  for (int e = tid; e < ns; e += WALK_THREADS) {
    const float x = ov_val[ov_id[e]];
    int rank = 0;
    for (int j = 0; j < ns; ++j) {
      const float y = ov_val[ov_id[j]];
      rank += (y > x || (y == x && j < e)) ? 1 : 0;
    }
    side[rank] = x;
  }
  __syncthreads();
  // the side entries between this thread's bins: bound(key_hi + 1) > value >= bound(key_lo)
  const float top = bound_of_key(key_hi + 1), bot = bound_of_key(key_lo);
  int s_begin = 0, s_end = 0;
  for (int lo = 0, hi = ns; ; ) {       // first index whose value is < top
    if (lo >= hi) { s_begin = lo; break; }
    const int mid = (lo + hi) >> 1;
    if (side[mid] < top) hi = mid; else lo = mid + 1;
  }
  for (int lo = 0, hi = ns; ; ) {       // first index whose value is < bot
    if (lo >= hi) { s_end = lo; break; }
    const int mid = (lo + hi) >> 1;
    if (side[mid] < bot) hi = mid; else lo = mid + 1;
  }
  if (tid == 0) s_begin = 0;
  if (tid == WALK_THREADS - 1) s_end = ns;
  s_end = max(s_end, s_begin);

  // tokens above this thread's values, and the row maximum
  float zmax = mask ? val_of_key(key_hi - (__ffsll(mask) - 1)) : -INFINITY;
  if (ns > 0) zmax = fmaxf(zmax, side[0]);
  int total_bins;
  const int above0 = block_excl_scan<int>(mine, red_i, total_bins) + s_begin;
  zmax = wave_max(zmax);
  __syncthreads();
  if (lane == 0) red_f[w] = zmax;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < WALK_WAVES; ++i) zmax = fmaxf(zmax, red_f[i]);

  // pass A: the mass of the top-k set below each thread's start
  double mass = 0.0;
  {
    int above = above0;
    walk_values(mask, hist, key_hi, side, s_begin, s_end, [&](float v, int c) {
      if (top_k == 0 || above < top_k) mass += (double)c * (double)expf((v - zmax) / temperature);
      above += c;
    });
  }
  double Z;
  const double mass0 = block_excl_scan<double>(mass, red_d, Z);
  // pass B: kept = inside top-k and the mass strictly above is < top_p (top_p = 1 keeps the whole top-k set)
  int kept = 0;
  float vmin = INFINITY;
  {
    int above = above0;
    double m = mass0;
    const double cut = (double)top_p * Z;
    walk_values(mask, hist, key_hi, side, s_begin, s_end, [&](float v, int c) {
      const bool in_k = top_k == 0 || above < top_k;
      if (in_k && (top_p >= 1.0f || m < cut)) { kept += c; vmin = fminf(vmin, v); }
      if (in_k) m += (double)c * (double)expf((v - zmax) / temperature);
      above += c;
    });
  }
  int total_kept;
  block_excl_scan<int>(kept, red_i, total_kept);
  vmin = -wave_max(-vmin);
  __syncthreads();
  if (lane == 0) red_f[w] = vmin;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < WALK_WAVES; ++i) vmin = fminf(vmin, red_f[i]);
  if (tid == 0) {
    *thr_out = vmin;                                   // +inf when nothing is kept (a row that is -inf throughout)
    if (n_kept_out) n_kept_out[b] = total_kept;
    if (min_kept_out) min_kept_out[b] = vmin / temperature;
  }
  // leave the bins zero for the next step (each thread read only its own)
  for (; mask; mask &= mask - 1) hist[key_hi - (__ffsll(mask) - 1)] = 0;
}

// ------------------------------------------------------------------------------------------------ phase 3: the draw
// Philox4x32-10 (Salmon et al., SC'11)
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// g = -log(-log(u)), u = ((r >> 8) + 0.5) * 2^-24. n + 0.5 needs 25 bits from n = 2^23 on, where f32 would round u (to 1.0 at the
// top): that half goes through 1 - u, which is exact there.
__device__ __forceinline__ float gumbel_of(uint32_t r) {
  const uint32_t n = r >> 8;
  float nl;                                    // -log(u)
  if (n >= (1u << 23)) nl = -log1pf(-(((float)((1u << 24) - 1u - n) + 0.5f) * 0x1p-24f));
  else nl = -logf(((float)n + 0.5f) * 0x1p-24f);
  return -logf(nl);
}

template <bool MASKED>
__device__ __forceinline__ void sample_draw_body(const bf16_t* __restrict__ logits, long ldl, int V, const int64_t* __restrict__ gen,
                                                 int max_new, const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                 float temperature, uint32_t seed_lo, uint32_t seed_hi, const int32_t* __restrict__ ws,
                                                 float* __restrict__ pval, int32_t* __restrict__ pidx, int32_t* __restrict__ overflow,
                                                 const vq3pick::MaskArgs& m, uint32_t* mw) {
  __shared__ int ov_id[OVL];
  __shared__ float ov_val[OVL];
  __shared__ int ov_n;
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int step = *step_p;
  const int n = min(step, max_new);
  const int per = (V + PICK_SLICES - 1) / PICK_SLICES;
  const int c0 = min(V, c * per), c1 = min(V, c0 + per);
  const bf16_t* lg = logits + (long)b * ldl;
  int n_pen, n_ov;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  bool fits;
  if constexpr (MASKED) {
    vq3pick::mask_stage(m, step - m.prompt_cols, c0, c1, mw);        // (build_overlay syncs before it reads)
    fits = build_overlay(lg, gen + (long)b * max_new, n, c0, c1, penalty, ngram, ov_id, ov_val, &ov_n, n_pen, n_ov, SliceMask{mw, c0});
  } else {
    fits = build_overlay(lg, gen + (long)b * max_new, n, c0, c1, penalty, ngram, ov_id, ov_val, &ov_n, n_pen, n_ov, NoMask{});
  }
  if (!fits && tid == 0) atomicExch(overflow, 1);
  if (fits && c0 < c1) {
    const float thr = *(const float*)(ws + (long)b * VQ3_SAMPLE_WORK_PER_ROW + THR_SLOT);
    // one Philox block serves ids 4q .. 4q + 3: a thread takes whole blocks, the slice's ragged ends are masked
    for (int q = (c0 >> 2) + tid; q <= ((c1 - 1) >> 2); q += 256) {
      float v[4];
      bool any = false;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * q + e;
        v[e] = -INFINITY;
        if (i >= c0 && i < c1) {
          float x = bf2f(lg[i]);
          for (int k = 0; k < n_ov; ++k)
            if (ov_id[k] == i) x = ov_val[k];
          if constexpr (MASKED) {
            if (vq3pick::mask_bit(mw, c0, i)) x = -INFINITY;
          }
          if (x >= thr && x < INFINITY) { v[e] = x; any = true; }
        }
      }
      if (!any) continue;
      uint32_t r[4];
      philox4x32_10((uint32_t)q, (uint32_t)step, (uint32_t)b, 0u, seed_lo, seed_hi, r);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (v[e] == -INFINITY) continue;
        const float s = v[e] / temperature + gumbel_of(r[e]);
        if (s > best) { best = s; bi = 4 * q + e; }      // ids ascend within a thread: the first of equal scores stays
      }
    }
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
    pval[b * PICK_SLICES + c] = best;
    pidx[b * PICK_SLICES + c] = bi;
  }
}

__global__ __launch_bounds__(256) void sample_draw_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                          const int64_t* __restrict__ gen, int max_new,
                                                          const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                          float temperature, uint32_t seed_lo, uint32_t seed_hi,
                                                          const int32_t* __restrict__ ws, float* __restrict__ pval,
                                                          int32_t* __restrict__ pidx, int32_t* __restrict__ overflow) {
  sample_draw_body<false>(logits, ldl, V, gen, max_new, step_p, penalty, ngram, temperature, seed_lo, seed_hi, ws, pval, pidx, overflow,
                          vq3pick::MaskArgs{}, nullptr);
}

__global__ __launch_bounds__(256) void sample_draw_masked_kernel(const bf16_t* __restrict__ logits, long ldl, int V,
                                                                 const int64_t* __restrict__ gen, int max_new,
                                                                 const int32_t* __restrict__ step_p, float penalty, int ngram,
                                                                 float temperature, uint32_t seed_lo, uint32_t seed_hi,
                                                                 const int32_t* __restrict__ ws, float* __restrict__ pval,
                                                                 int32_t* __restrict__ pidx, int32_t* __restrict__ overflow,
                                                                 vq3pick::MaskArgs m) {
  __shared__ uint32_t mw[vq3pick::MASK_SLICE_WORDS];
  sample_draw_body<true>(logits, ldl, V, gen, max_new, step_p, penalty, ngram, temperature, seed_lo, seed_hi, ws, pval, pidx, overflow, m,
                         mw);
}

}  // namespace

// both entries: `mask` NULL is vq3_sample_pick, launch for launch
static int sample_pick_impl(const char* who, const void* logits_bf16, int64_t ld_logits, float* work, int32_t B, int32_t V,
                            int64_t* generated, int32_t max_new, const int32_t* step, int32_t* finished, float repetition_penalty,
                            int32_t no_repeat_ngram, const int64_t* eos_ids, int32_t n_eos, int64_t pad_id, int32_t* next_ids,
                            float temperature, int32_t top_k, float top_p, uint64_t seed, void* sample_work, int32_t* n_kept,
                            float* min_kept, const vq3_pick_mask* mask, void* stream) {
  VQ3_CHECK_ARG(logits_bf16 && work && generated && step && finished && next_ids && sample_work, "%s: null pointer", who);
  VQ3_CHECK_ARG(B > 0 && V > 0 && max_new > 0 && ld_logits >= V, "%s: bad shape", who);
  VQ3_CHECK_ARG(max_new <= vq3pick::PICK_MAX_IDS, "%s: at most %d ids per row (prompt + new), got %d", who, vq3pick::PICK_MAX_IDS, max_new);
  VQ3_CHECK_ARG(repetition_penalty > 0.f, "%s: repetition_penalty must be > 0, got %f", who, (double)repetition_penalty);
  VQ3_CHECK_ARG(no_repeat_ngram >= 0 && n_eos >= 0 && (n_eos == 0 || eos_ids), "%s: bad ngram / eos arguments", who);
  VQ3_CHECK_ARG(temperature > 0.f && temperature < INFINITY, "%s: temperature must be > 0 and finite, got %f", who, (double)temperature);
  VQ3_CHECK_ARG(top_k >= 0, "%s: top_k must be >= 0 (0 = off), got %d", who, top_k);
  VQ3_CHECK_ARG(top_p > 0.f && top_p <= 1.f, "%s: top_p must be in (0, 1], got %f", who, (double)top_p);
  VQ3_CHECK_ARG(((uintptr_t)sample_work & 15) == 0, "%s: the workspace must be 16-byte aligned", who);
  if (mask) {
    const char* bad = vq3pick::mask_args_error(mask->planes, mask->words, mask->min_new, mask->prompt_cols, V);
    VQ3_CHECK_ARG(bad == nullptr, "%s: %s", who, bad);
    VQ3_CHECK_ARG((V + PICK_SLICES - 1) / PICK_SLICES <= (vq3pick::MASK_SLICE_WORDS - 2) * 32, "%s: V %d exceeds %d", who, V,
                  PICK_SLICES * (vq3pick::MASK_SLICE_WORDS - 2) * 32);
  }
  // work as in vq3_greedy_pick: [B * 64] partial values, [B * 64] partial indices, 1 overflow flag
  float* pval = work;
  int32_t* pidx = (int32_t*)(work + (long)B * PICK_SLICES);
  int32_t* overflow = pidx + (long)B * PICK_SLICES;
  int32_t* ws = (int32_t*)sample_work;
  const hipStream_t s = (hipStream_t)stream;
  const bf16_t* lg = (const bf16_t*)logits_bf16;
  if (mask) {
    const vq3pick::MaskArgs m{mask->planes, mask->words, mask->min_new, mask->prompt_cols};
    hipLaunchKernelGGL(sample_hist_masked_kernel, dim3(PICK_SLICES, B), dim3(256), 0, s, lg, (long)ld_logits, V, generated, max_new, step,
                       repetition_penalty, no_repeat_ngram, ws, overflow, m);
    hipLaunchKernelGGL(sample_walk_kernel<vq3pick::MaskArgs>, dim3(B), dim3(WALK_THREADS), 0, s, lg, (long)ld_logits, V, generated, max_new, step,
                       repetition_penalty, no_repeat_ngram, temperature, top_k, top_p, ws, overflow, n_kept, min_kept, m);
    hipLaunchKernelGGL(sample_draw_masked_kernel, dim3(PICK_SLICES, B), dim3(256), 0, s, lg, (long)ld_logits, V, generated, max_new, step,
                       repetition_penalty, no_repeat_ngram, temperature, (uint32_t)seed, (uint32_t)(seed >> 32), ws, pval, pidx, overflow,
                       m);
  } else {
    hipLaunchKernelGGL(sample_hist_kernel, dim3(PICK_SLICES, B), dim3(256), 0, s, lg, (long)ld_logits, V, generated, max_new, step,
                       repetition_penalty, no_repeat_ngram, ws, overflow);
    hipLaunchKernelGGL(sample_walk_kernel<>, dim3(B), dim3(WALK_THREADS), 0, s, lg, (long)ld_logits, V, generated, max_new, step,
                       repetition_penalty, no_repeat_ngram, temperature, top_k, top_p, ws, overflow, n_kept, min_kept);
    hipLaunchKernelGGL(sample_draw_kernel, dim3(PICK_SLICES, B), dim3(256), 0, s, lg, (long)ld_logits, V, generated, max_new, step,
                       repetition_penalty, no_repeat_ngram, temperature, (uint32_t)seed, (uint32_t)(seed >> 32), ws, pval, pidx, overflow);
  }
  vq3pick::launch_pick_final(pval, pidx, generated, max_new, step, finished, eos_ids, n_eos, (long)pad_id, next_ids, B, s);
  VQ3_CHECK_LAUNCH(who);
  return 0;
}

extern "C" int vq3_sample_pick(const void* logits_bf16, int64_t ld_logits, float* work, int32_t B, int32_t V, int64_t* generated,
                               int32_t max_new, const int32_t* step, int32_t* finished, float repetition_penalty,
                               int32_t no_repeat_ngram, const int64_t* eos_ids, int32_t n_eos, int64_t pad_id, int32_t* next_ids,
                               float temperature, int32_t top_k, float top_p, uint64_t seed, void* sample_work, int32_t* n_kept,
                               float* min_kept, void* stream) {
  return sample_pick_impl("sample_pick", logits_bf16, ld_logits, work, B, V, generated, max_new, step, finished, repetition_penalty,
                          no_repeat_ngram, eos_ids, n_eos, pad_id, next_ids, temperature, top_k, top_p, seed, sample_work, n_kept,
                          min_kept, nullptr, stream);
}

extern "C" int vq3_sample_pick_masked(const void* logits_bf16, int64_t ld_logits, float* work, int32_t B, int32_t V, int64_t* generated,
                                      int32_t max_new, const int32_t* step, int32_t* finished, float repetition_penalty,
                                      int32_t no_repeat_ngram, const int64_t* eos_ids, int32_t n_eos, int64_t pad_id, int32_t* next_ids,
                                      float temperature, int32_t top_k, float top_p, uint64_t seed, void* sample_work, int32_t* n_kept,
                                      float* min_kept, const vq3_pick_mask* mask, void* stream) {
  VQ3_CHECK_ARG(mask, "sample_pick_masked: null mask");
  return sample_pick_impl("sample_pick_masked", logits_bf16, ld_logits, work, B, V, generated, max_new, step, finished,
                          repetition_penalty, no_repeat_ngram, eos_ids, n_eos, pad_id, next_ids, temperature, top_k, top_p, seed,
                          sample_work, n_kept, min_kept, mask, stream);
}
