// LoRA adapter kernels (include/vq3_hip.h "LoRA"): peft's lora.Linear.forward, y = base(x) + lora_B(lora_A(dropout(x))) * s,
// as three memory-bound products around the base GEMMs, and their backward.
//   down    U[M, t*r + j]  = sum_k (mask_t o X)[m, x_col0_t + k] . W_t(j, k)              (one X pass for targets that share it)
//   up-add  Y[m, y_col0_t + n] = bf16(Y + s * sum_t mask_t(m, n) . sum_j U[m, u_col0_t + j] . W_t(n, j))   (one rounding)
//   wgrad   part[slice, out_off_t + p * nQ + q] = alpha * sum_{m in slice} L[m, lcol0_t + p] . (mask_t o R)[m, rcol0_t + q]
// The masks are vq3_dropout's: element (m, c) of target t is kept when drop_bits(seed, offset_t + m * mask_ld + c) >= p * 2^24, and a
// kept bf16 value becomes bf16(x / (1 - p)) exactly as the in-place kernel leaves it, so the masked X never needs to be stored.
// All three are plain fp32 FMA kernels on LDS tiles: the contraction of the down / up products is r <= 64 per target, so the MFMA
// would idle on the operand traffic; the weight gradients are long reductions over M that are sliced into fixed partial slabs
// (summed by vq3_colsum_f32 / vq3_colsum_f32_to_bf16 in slice order: no atomics, the same bits on every run).
#include "common.h"
#include "vq3_hip.h"

namespace {

struct DropMask {
  unsigned thresh;
  float scale;
  unsigned long long seed;
  bool on;
};

__device__ __forceinline__ float drop_apply(const DropMask& d, unsigned long long idx, float x) {
  if (!d.on) return x;
  return drop_bits(d.seed, idx) >= d.thresh ? rbf(x * d.scale) : 0.f;
}
__device__ __forceinline__ float drop_scale(const DropMask& d, unsigned long long idx) {
  if (!d.on) return 1.f;
  return drop_bits(d.seed, idx) >= d.thresh ? d.scale : 0.f;
}

struct Targets {
  vq3_lora_target t[VQ3_LORA_MAX_TARGETS];
  int n;
};

// ------------------------------------------------------------------------------------------------ down
// Block: 32 rows x every target's r columns; 256 threads = 16 row pairs x 16 column lanes; a lane owns local columns lane + 16 c of
// every target. K walks in chunks of 32: the X chunk is loaded once (8 bytes per thread when aligned) and written to LDS once per
// target of the group with that target's mask applied; W chunks are staged as f32 [KC][r] per target.
constexpr int DN_ROWS = 32, DN_KC = 32;

template <int CR>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ X, long ldx, int M, Targets tg, int r, int shared,
                                                        bf16_t* __restrict__ U, long ldu, DropMask dm, long mask_ld) {
  extern __shared__ float dn_lds[];
  const int T = tg.n;
  const int TG = shared ? T : 1;                    // targets per group (the host sizes the LDS for TG)
  float* Xs = dn_lds;                               // [TG][KC][DN_ROWS]
  float* Ws = dn_lds + TG * DN_KC * DN_ROWS;        // [TG][KC][r]
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int m0 = blockIdx.x * DN_ROWS;
  float acc[VQ3_LORA_MAX_TARGETS][CR][2];
#pragma unroll
  for (int t = 0; t < VQ3_LORA_MAX_TARGETS; ++t)
#pragma unroll
    for (int c = 0; c < CR; ++c) acc[t][c][0] = acc[t][c][1] = 0.f;

  const int ngroups = shared ? 1 : T;
  for (int g = 0; g < ngroups; ++g) {
    const int t_lo = shared ? 0 : g, t_hi = shared ? T : g + 1;
    const int xc0 = tg.t[t_lo].x_col0, K = tg.t[t_lo].k;
    for (int k0 = 0; k0 < K; k0 += DN_KC) {
      // X chunk: thread -> row tid / 8, columns (tid % 8) * 4 .. + 3
      {
        const int row = tid >> 3, kk = (tid & 7) * 4, m = m0 + row;
        float xv[4];
        const long base = (long)m * ldx + xc0 + k0 + kk;
        if (m < M && k0 + kk + 4 <= K && (reinterpret_cast<uintptr_t>(X + base) & 7) == 0) {
          const u32x2 w = *reinterpret_cast<const u32x2*>(X + base);
          const f32x2_t a = unpack2bf(w[0]), b = unpack2bf(w[1]);
          xv[0] = a[0]; xv[1] = a[1]; xv[2] = b[0]; xv[3] = b[1];
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) xv[e] = (m < M && k0 + kk + e < K) ? bf2f(X[base + e]) : 0.f;
        }
        for (int t = t_lo; t < t_hi; ++t) {
          DropMask d = dm;
          d.on = dm.on && tg.t[t].mask;
          const unsigned long long mi = tg.t[t].mask_offset + (unsigned long long)((long)m * mask_ld + xc0 + k0 + kk);
#pragma unroll
          for (int e = 0; e < 4; ++e)
            Xs[((t - t_lo) * DN_KC + kk + e) * DN_ROWS + row] = (m < M && k0 + kk + e < K) ? drop_apply(d, mi + e, xv[e]) : 0.f;
        }
      }
      // W chunks: [KC][r] per target of the group
      for (int t = t_lo; t < t_hi; ++t) {
        const vq3_lora_target& tt = tg.t[t];
        const bf16_t* w = (const bf16_t*)tt.w;
        for (int i = tid; i < DN_KC * r; i += 256) {
          int k, j;
          if (tt.w_kmajor) { j = i % r; k = i / r; } else { k = i % DN_KC; j = i / DN_KC; }
          const int kg = k0 + k;
          float v = 0.f;
          if (kg < K) v = bf2f(tt.w_kmajor ? w[(long)kg * tt.ldw + j] : w[(long)j * tt.ldw + kg]);
          Ws[((t - t_lo) * DN_KC + k) * r + j] = v;
        }
      }
      __syncthreads();
      const int kn = min(DN_KC, K - k0);
      for (int t = t_lo; t < t_hi; ++t) {
        const float* xs = Xs + (t - t_lo) * DN_KC * DN_ROWS + tr * 2;
        const float* ws = Ws + (t - t_lo) * DN_KC * r;
        for (int k = 0; k < kn; ++k) {
          const float x0 = xs[k * DN_ROWS], x1 = xs[k * DN_ROWS + 1];
#pragma unroll
          for (int c = 0; c < CR; ++c) {
            const int j = tc + 16 * c;
            const float wv = j < r ? ws[k * r + j] : 0.f;
#pragma unroll
            for (int tt = 0; tt < VQ3_LORA_MAX_TARGETS; ++tt)
              if (tt == t) {
                acc[tt][c][0] = fmaf(x0, wv, acc[tt][c][0]);
                acc[tt][c][1] = fmaf(x1, wv, acc[tt][c][1]);
              }
          }
        }
      }
      __syncthreads();
    }
  }
#pragma unroll
  for (int t = 0; t < VQ3_LORA_MAX_TARGETS; ++t) {
    if (t >= T) break;
#pragma unroll
    for (int c = 0; c < CR; ++c) {
      const int j = tc + 16 * c;
      if (j >= r) continue;
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int m = m0 + tr * 2 + i;
        if (m < M) U[(long)m * ldu + tg.t[t].u_col0 + j] = f2bf(acc[t][c][i]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ up-add
// Block: 64 x 64 outputs of Y, 4 x 4 per thread (four contiguous columns: one 8-byte read-modify-write per row). Every target whose
// column range meets the tile contributes its rank-r product (U and W staged as f32 [r][64] in LDS), masked per element, into one f32
// sum; Y is read, added to and rounded once. A tile no target meets leaves at once.
constexpr int UP_TM = 64, UP_TN = 64;
// y + s * d, leaving y's bits alone where the product is zero (a -0 stays -0: B = 0 adapters change nothing)
__device__ __forceinline__ float add_lora(float y, float s, float d) {
  const float v = s * d;
  return v == 0.f ? y : y + v;
}

__global__ __launch_bounds__(256) void lora_up_add_kernel(bf16_t* __restrict__ Y, long ldy, int M, const bf16_t* __restrict__ U, long ldu,
                                                          Targets tg, int r, float s, DropMask dm, long mask_ld) {
  __shared__ __attribute__((aligned(16))) float Us[64 * UP_TM];
  __shared__ __attribute__((aligned(16))) float Bs[64 * UP_TN];
  const int tid = threadIdx.x, tr = tid >> 4, tc = tid & 15;
  const int m0 = blockIdx.x * UP_TM, n0 = blockIdx.y * UP_TN;
  bool any = false;
  for (int t = 0; t < tg.n; ++t) any |= n0 < tg.t[t].y_col0 + tg.t[t].n && n0 + UP_TN > tg.t[t].y_col0;
  if (!any) return;
  float tot[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) tot[i][e] = 0.f;
  for (int t = 0; t < tg.n; ++t) {
    const vq3_lora_target& tt = tg.t[t];
    if (!(n0 < tt.y_col0 + tt.n && n0 + UP_TN > tt.y_col0)) continue;
    const bf16_t* w = (const bf16_t*)tt.w;
    for (int i = tid; i < r * UP_TM; i += 256) {            // U tile [r][64 rows] (neighbouring lanes: neighbouring LDS words)
      const int row = i % UP_TM, j = i / UP_TM, m = m0 + row;
      Us[j * UP_TM + row] = m < M ? bf2f(U[(long)m * ldu + tt.u_col0 + j]) : 0.f;
    }
    for (int i = tid; i < r * UP_TN; i += 256) {            // W tile [r][64 cols]: W_t(n, j) at w[n ldw + j] or w[j ldw + n] (k-major)
      const int col = i % UP_TN, j = i / UP_TN;
      const int n = n0 + col - tt.y_col0;
      float v = 0.f;
      if (n >= 0 && n < tt.n) v = bf2f(tt.w_kmajor ? w[(long)j * tt.ldw + n] : w[(long)n * tt.ldw + j]);
      Bs[j * UP_TN + col] = v;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
    for (int j = 0; j < r; ++j) {
      const f32x4 u = *reinterpret_cast<const f32x4*>(Us + j * UP_TM + tr * 4);
      const f32x4 b = *reinterpret_cast<const f32x4*>(Bs + j * UP_TN + tc * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(u[i], b[e], acc[i][e]);
    }
    DropMask d = dm;
    d.on = dm.on && tt.mask;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + tr * 4 + i, col = n0 + tc * 4 + e;
        const float ms = (d.on && m < M) ? drop_scale(d, tt.mask_offset + (unsigned long long)((long)m * mask_ld + col)) : 1.f;
        tot[i][e] = fmaf(acc[i][e], ms, tot[i][e]);
      }
    __syncthreads();
  }
  int ncols = 0;
  for (int t = 0; t < tg.n; ++t) ncols = max(ncols, tg.t[t].y_col0 + tg.t[t].n);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + tr * 4 + i, c0 = n0 + tc * 4;
    if (m >= M) continue;
    bf16_t* y = Y + (long)m * ldy + c0;
    if (c0 + 4 <= ncols && (reinterpret_cast<uintptr_t>(y) & 7) == 0) {
      u32x2 v = *reinterpret_cast<const u32x2*>(y);
      const f32x2_t a = unpack2bf(v[0]), b = unpack2bf(v[1]);
      v[0] = pack2bf(add_lora(a[0], s, tot[i][0]), add_lora(a[1], s, tot[i][1]));
      v[1] = pack2bf(add_lora(b[0], s, tot[i][2]), add_lora(b[1], s, tot[i][3]));
      *reinterpret_cast<u32x2*>(y) = v;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (c0 + e < ncols) y[e] = f2bf(add_lora(bf2f(y[e]), s, tot[i][e]));
    }
  }
}

// ------------------------------------------------------------------------------------------------ weight gradients
// Block: a TP x TQ output tile (TP * TQ = 4096, 4 x 4 per thread) of one target over one slice of rows; M walks in chunks of 16 rows
// staged as f32 in LDS. Every slot of the partial slab is written (zeros for a slice past M), so the column sums need no clearing.
constexpr int WG_MC = 16;

struct WgradTiles {
  int first[VQ3_LORA_MAX_TARGETS + 1];   // prefix sums of the targets' tile counts
  int qtiles[VQ3_LORA_MAX_TARGETS];
};

__global__ __launch_bounds__(256) void lora_wgrad_kernel(const bf16_t* __restrict__ L, long ldl, const bf16_t* __restrict__ R, long ldr, int M,
                                                         Targets tg, WgradTiles tl, int TQ, int rows_per_slice, float alpha, DropMask dm,
                                                         long mask_ld, float* __restrict__ part, long part_ld) {
  __shared__ __attribute__((aligned(16))) float Ls[WG_MC * 256];
  __shared__ __attribute__((aligned(16))) float Rs[WG_MC * 256];
  const int TP = 4096 / TQ, tq = TQ / 4;
  const int tid = threadIdx.x, tpi = tid / tq, tqi = tid % tq;
  int t = 0;
  while (t + 1 < tg.n && (int)blockIdx.x >= tl.first[t + 1]) ++t;
  const vq3_lora_target& tt = tg.t[t];
  const int local = blockIdx.x - tl.first[t];
  const int p0 = (local / tl.qtiles[t]) * TP, q0 = (local % tl.qtiles[t]) * TQ;
  const int nP = tt.n, nQ = tt.k;
  const int ms = blockIdx.y * rows_per_slice, me = min(M, ms + rows_per_slice);
  DropMask d = dm;
  d.on = dm.on && tt.mask;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[i][e] = 0.f;
  for (int mc = ms; mc < me; mc += WG_MC) {
    for (int i = tid; i < WG_MC * TP; i += 256) {
      const int row = i / TP, p = i % TP, m = mc + row;
      Ls[row * TP + p] = (m < me && p0 + p < nP) ? bf2f(L[(long)m * ldl + tt.y_col0 + p0 + p]) : 0.f;
    }
    for (int i = tid; i < WG_MC * TQ; i += 256) {
      const int row = i / TQ, q = i % TQ, m = mc + row, c = tt.x_col0 + q0 + q;
      float v = 0.f;
      if (m < me && q0 + q < nQ)
        v = drop_apply(d, tt.mask_offset + (unsigned long long)((long)m * mask_ld + c), bf2f(R[(long)m * ldr + c]));
      Rs[row * TQ + q] = v;
    }
    __syncthreads();
    for (int row = 0; row < WG_MC; ++row) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(Ls + row * TP + tpi * 4);
      const f32x4 b = *reinterpret_cast<const f32x4*>(Rs + row * TQ + tqi * 4);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[i][e] = fmaf(a[i], b[e], acc[i][e]);
    }
    __syncthreads();
  }
  float* out = part + (long)blockIdx.y * part_ld + tt.u_col0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int p = p0 + tpi * 4 + i;
    if (p >= nP) continue;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + tqi * 4 + e;
      if (q < nQ) out[(long)p * nQ + q] = alpha * acc[i][e];
    }
  }
}

DropMask make_mask(float p, uint64_t seed) {
  DropMask d;
  d.on = p > 0.f;
  d.thresh = (unsigned)(p * 16777216.0f);
  d.scale = 1.f / (1.f - p);
  d.seed = (unsigned long long)seed;
  return d;
}

}  // namespace

extern "C" int vq3_lora_down(const void* X, int64_t ldx, int32_t M, const vq3_lora_target* targets, int32_t ntargets, int32_t r,
                             void* U, int64_t ldu, float p, uint64_t seed, int64_t mask_ld, void* stream) {
  VQ3_CHECK_ARG(X && U && M >= 1 && r >= 1 && r <= 64 && p >= 0.f && p < 1.f, "lora_down: bad args (M >= 1, 1 <= r <= 64, 0 <= p < 1)");
  VQ3_CHECK_ARG(targets && ntargets >= 1 && ntargets <= VQ3_LORA_MAX_TARGETS, "lora_down: 1..%d targets", VQ3_LORA_MAX_TARGETS);
  Targets tg{};
  tg.n = ntargets;
  int shared = 1;
  for (int i = 0; i < ntargets; ++i) {
    const vq3_lora_target& t = targets[i];
    VQ3_CHECK_ARG(t.w && t.k >= 1 && t.x_col0 >= 0 && t.x_col0 + t.k <= ldx && t.u_col0 >= 0 && t.u_col0 + r <= ldu && t.ldw >= 1,
                  "lora_down: target %d out of range", i);
    VQ3_CHECK_ARG(t.w_kmajor ? t.ldw >= r : t.ldw >= t.k, "lora_down: target %d: ldw too small", i);
    tg.t[i] = t;
    if (t.x_col0 != targets[0].x_col0 || t.k != targets[0].k) shared = 0;
  }
  const int T = shared ? ntargets : 1;
  const size_t lds = (size_t)T * DN_KC * (DN_ROWS + r) * sizeof(float);
  const dim3 grid((M + DN_ROWS - 1) / DN_ROWS);
  const DropMask dm = make_mask(p, seed);
  const int CR = (r + 15) / 16;
#define VQ3_DN(C) hipLaunchKernelGGL(lora_down_kernel<C>, grid, dim3(256), lds, (hipStream_t)stream, (const bf16_t*)X, (long)ldx, M, tg, r, \
                                     shared, (bf16_t*)U, (long)ldu, dm, (long)mask_ld)
  if (CR == 1) VQ3_DN(1);
  else if (CR == 2) VQ3_DN(2);
  else if (CR == 3) VQ3_DN(3);
  else VQ3_DN(4);
#undef VQ3_DN
  VQ3_CHECK_LAUNCH("lora_down");
  return 0;
}

extern "C" int vq3_lora_up_add(void* Y, int64_t ldy, int32_t M, const void* U, int64_t ldu, const vq3_lora_target* targets, int32_t ntargets,
                               int32_t r, float s, float p, uint64_t seed, int64_t mask_ld, void* stream) {
  VQ3_CHECK_ARG(Y && U && M >= 1 && r >= 1 && r <= 64 && p >= 0.f && p < 1.f, "lora_up_add: bad args (M >= 1, 1 <= r <= 64, 0 <= p < 1)");
  VQ3_CHECK_ARG(targets && ntargets >= 1 && ntargets <= VQ3_LORA_MAX_TARGETS, "lora_up_add: 1..%d targets", VQ3_LORA_MAX_TARGETS);
  Targets tg{};
  tg.n = ntargets;
  int ncols = 0;
  for (int i = 0; i < ntargets; ++i) {
    const vq3_lora_target& t = targets[i];
    VQ3_CHECK_ARG(t.w && t.n >= 1 && t.y_col0 >= 0 && t.y_col0 + t.n <= ldy && t.u_col0 >= 0 && t.u_col0 + r <= ldu && t.ldw >= 1,
                  "lora_up_add: target %d out of range", i);
    VQ3_CHECK_ARG(t.w_kmajor ? t.ldw >= t.n : t.ldw >= r, "lora_up_add: target %d: ldw too small", i);
    tg.t[i] = t;
    ncols = t.y_col0 + t.n > ncols ? t.y_col0 + t.n : ncols;
  }
  const dim3 grid((M + UP_TM - 1) / UP_TM, (ncols + UP_TN - 1) / UP_TN);
  hipLaunchKernelGGL(lora_up_add_kernel, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)Y, (long)ldy, M, (const bf16_t*)U, (long)ldu, tg,
                     r, s, make_mask(p, seed), (long)mask_ld);
  VQ3_CHECK_LAUNCH("lora_up_add");
  return 0;
}

extern "C" int vq3_lora_wgrad_part(const void* L, int64_t ldl, const void* R, int64_t ldr, int32_t M, const vq3_lora_target* targets,
                                   int32_t ntargets, int32_t slices, float alpha, float p, uint64_t seed, int64_t mask_ld, float* part,
                                   int64_t part_ld, void* stream) {
  VQ3_CHECK_ARG(L && R && part && M >= 1 && slices >= 1 && p >= 0.f && p < 1.f, "lora_wgrad_part: bad args");
  VQ3_CHECK_ARG(targets && ntargets >= 1 && ntargets <= VQ3_LORA_MAX_TARGETS, "lora_wgrad_part: 1..%d targets", VQ3_LORA_MAX_TARGETS);
  Targets tg{};
  tg.n = ntargets;
  int minP = 1 << 30, minQ = 1 << 30;
  for (int i = 0; i < ntargets; ++i) {
    const vq3_lora_target& t = targets[i];
    VQ3_CHECK_ARG(t.n >= 1 && t.k >= 1 && t.y_col0 >= 0 && t.y_col0 + t.n <= ldl && t.x_col0 >= 0 && t.x_col0 + t.k <= ldr &&
                      t.u_col0 >= 0 && t.u_col0 + (int64_t)t.n * t.k <= part_ld,
                  "lora_wgrad_part: target %d out of range", i);
    tg.t[i] = targets[i];
    minP = t.n < minP ? t.n : minP;
    minQ = t.k < minQ ? t.k : minQ;
  }
  // tile shape: the narrow side of the product (r) gets 16, the wide one 256; two wide sides take 64 x 64
  const int TQ = minQ <= 16 ? 16 : (minP <= 16 ? 256 : 64);
  const int TP = 4096 / TQ;
  WgradTiles tl{};
  tl.first[0] = 0;
  for (int i = 0; i < ntargets; ++i) {
    tl.qtiles[i] = (targets[i].k + TQ - 1) / TQ;
    tl.first[i + 1] = tl.first[i] + tl.qtiles[i] * ((targets[i].n + TP - 1) / TP);
  }
  const int rows_per_slice = (M + slices - 1) / slices;
  const dim3 grid(tl.first[ntargets], slices);
  hipLaunchKernelGGL(lora_wgrad_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)L, (long)ldl, (const bf16_t*)R, (long)ldr, M, tg,
                     tl, TQ, rows_per_slice, alpha, make_mask(p, seed), (long)mask_ld, part, (long)part_ld);
  VQ3_CHECK_LAUNCH("lora_wgrad_part");
  return 0;
}
