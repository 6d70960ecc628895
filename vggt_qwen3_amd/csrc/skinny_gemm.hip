// Decode-time skinny GEMMs: y[M <= 8, N] = f(x) W^T (+ residual). One new token per row and step, so every contraction is a
// matrix-vector product that streams the weights once: HBM-bound, not MFMA-bound. A wave owns R weight rows, lanes stride K
// in 16-byte pieces (coalesced 1 KiB per row per load), fp32 accumulation, wave reduction at the end.
//
//  * vq3_skinny_gemm_bf16   bf16 weights, M <= 8, bf16 or fp32 output.
//  * vq3_skinny_gemm_fp8    e4m3 weights with per-row scales (config C5), M <= 2: the activation row is quantised per token
//                           exactly as the fp8 GEMM does, so decode and prefill follow one numeric contract; the weight
//                           stream - the only thing that costs time here - is halved.
//
// f (XMODE): 0: x as given. 1: x = ln_w * bf16(x * rstd(x)) (Qwen3RMSNorm fused into the consumer; the K-element rows sit in
// L2). 2: x = bf16(silu(gate) * up) with gate = xin[:, :K], up = xin[:, K:2K] (SwiGLU fused into down_proj). Both are
// bit-identical to vq3_rmsnorm_fwd / vq3_silu_mul_fwd feeding XMODE 0: their rounding points are written once, in decode_x.h.
#include <type_traits>

#include "common.h"
#include "decode_x.h"
#include "vq3_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------ generic kernel
// x streamed per 512-element chunk; every wave recomputes the RMSNorm row statistics
template <int MT, int R, int XMODE>
__global__ __launch_bounds__(256) void skinny_gemm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                         void* __restrict__ y, const bf16_t* __restrict__ res,
                                                         const bf16_t* __restrict__ ln_w, float eps, int M, int N, int K,
                                                         long ldx, long ldw, long ldy, long ldr, int out_f32) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wid) * R;
  if (n0 >= N) return;
  float rstd[MT];
  if (XMODE == 1) {
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      float ss = 0.f;
      const bf16_t* xr = x + (long)min(m, M - 1) * ldx;
      for (int k = lane * 8; k < K; k += 512) {
        float f[8];
        unpack8(*(const u32x4*)(xr + k), f);
        ss = sumsq8(f, ss);
      }
      rstd[m] = rsqrtf(wave_sum(ss) / (float)K + eps);
    }
  }
  float acc[R][MT];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
  const bf16_t* wrow[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wrow[r] = W + (long)min(n0 + r, N - 1) * ldw;
  constexpr int U = R >= 4 ? 1 : (R == 2 ? 2 : 4);   // K chunks in flight: R * U 16-byte weight loads per lane
  for (int k0 = lane * 8; k0 < K; k0 += 512 * U) {   // K % 8 == 0
    u32x4 wv[U][R];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = min(k0 + 512 * u, K - 8);        // clamped duplicate loads are masked below
#pragma unroll
      for (int r = 0; r < R; ++r) wv[u][r] = __builtin_nontemporal_load((const u32x4*)(wrow[r] + k));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int k = k0 + 512 * u;
      if (k >= K) break;
      float xf[MT][8];
      u32x4 lwv;
      if (XMODE == 1) lwv = *(const u32x4*)(ln_w + k);
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        load_x8<XMODE>(x + (long)min(m, M - 1) * ldx, k, K, xf[m]);
        if (XMODE == 1) rmsnorm8(xf[m], lwv, rstd[m]);
      }
#pragma unroll
      for (int r = 0; r < R; ++r) {
        float wf[8];
        unpack8(wv[u][r], wf);
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[r][m] = fmaf(wf[j], xf[m][j], acc[r][m]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float s = wave_sum(acc[r][m]);
      if (lane == 0 && m < M && n0 + r < N) store_out<false>(y, res, s, m, n0 + r, ldy, ldr, out_f32);
    }
}

// ------------------------------------------------------------------------------------------------ register-resident x
// Weight formats of the register-resident kernel: E weights per 16-byte piece, CH chunks of 64 * E elements per K slice held
// in registers (x costs MT * CH * E VGPRs), and whether the prepared row goes through the e4m3 quantisation.
struct Bf16Weights {
  typedef bf16_t elem;
  static constexpr int E = 8, CH = 5;
  static constexpr bool QUANT = false;
  static __device__ __forceinline__ void unpack(const u32x4 v, float* f) { unpack8(v, f); }
};
struct E4m3Weights {
  typedef uint8_t elem;
  static constexpr int E = 16, CH = 3;
  static constexpr bool QUANT = true;
  static __device__ __forceinline__ void unpack(const u32x4 v, float* f) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], false);
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[w], true);
      f[4 * w + 0] = lo[0]; f[4 * w + 1] = lo[1]; f[4 * w + 2] = hi[0]; f[4 * w + 3] = hi[1];
    }
  }
};

// v[m]: one value per lane -> combined over the wave and then over the KS waves (K slices) of row group g through LDS
template <bool MAX, int MT, int KS>
__device__ __forceinline__ void combine_slices(float (&v)[MT], float (*red)[MT], int lane, int wid, int g) {
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const float w = MAX ? wave_max(v[m]) : wave_sum(v[m]);
    if (lane == 0) red[wid][m] = w;
  }
  __syncthreads();
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    v[m] = 0.f;
#pragma unroll
    for (int q = 0; q < KS; ++q) v[m] = MAX ? fmaxf(v[m], red[g * KS + q][m]) : v[m] + red[g * KS + q][m];
  }
}

// For 1-2 rows (the reference's callers decode one prompt at a time): a block of 4 waves is split into 4/KS row groups x KS
// K-slices (chunks interleaved across the slices). Each wave loads its slice of x ONCE (<= CH chunks, transformed in
// registers: RMSNorm statistics are combined across the slices through LDS; SwiGLU is evaluated once per wave), then streams
// R weight rows with all R*CH 16-byte loads of a row group in flight before the first FMA. More waves per weight byte than
// the generic kernel -> enough loads in flight to approach HBM bandwidth at N = 2560.
template <class F, int MT, int R, int KS, int XMODE>
__global__ __launch_bounds__(256) void skinny_regx_kernel(const bf16_t* __restrict__ x, const typename F::elem* __restrict__ W,
                                                         const float* __restrict__ wscale, void* __restrict__ y,
                                                         const bf16_t* __restrict__ res, const bf16_t* __restrict__ ln_w,
                                                         float eps, int M, int N, int K, long ldx, long ldw, long ldy, long ldr,
                                                         int out_f32) {
  constexpr int E = F::E, CH = F::CH, P = E / 8, G = 4 / KS;
  __shared__ float red[4][MT];
  __shared__ float redm[4][MT];
  __shared__ float part[4][R][MT];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int g = wid / KS, ks = wid % KS;
  const int n0 = (blockIdx.x * G + g) * R;
  int kof[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) kof[c] = (c * KS + ks) * (64 * E) + lane * E;
  // the weight stream does not depend on x: put all of this wave's weight loads in flight first, then prepare x under them
  const bool active = n0 < N;
  u32x4 wv[R][CH];
  if (active) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const typename F::elem* wr = W + (long)min(n0 + r, N - 1) * ldw;
#pragma unroll
      for (int c = 0; c < CH; ++c) wv[r][c] = __builtin_nontemporal_load((const u32x4*)(wr + min(kof[c], K - E)));
    }
  }
  u32x4 lwv[CH][P];
  if (XMODE == 1) {
#pragma unroll
    for (int c = 0; c < CH; ++c)
#pragma unroll
      for (int p = 0; p < P; ++p) lwv[c][p] = *(const u32x4*)(ln_w + min(kof[c], K - E) + 8 * p);
  }
  float xf[MT][CH][E];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const bf16_t* xr = x + (long)min(m, M - 1) * ldx;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int p = 0; p < P; ++p) {
        if (kof[c] < K) {
          load_x8<XMODE>(xr, kof[c] + 8 * p, K, xf[m][c] + 8 * p);
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) xf[m][c][8 * p + j] = 0.f;
        }
      }
    }
  }
  if (XMODE == 1) {
    float ss[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      ss[m] = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p) ss[m] = sumsq8(xf[m][c] + 8 * p, ss[m]);
    }
    combine_slices<false, MT, KS>(ss, red, lane, wid, g);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float rstd = rsqrtf(ss[m] / (float)K + eps);
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int p = 0; p < P; ++p)
          if (kof[c] < K) rmsnorm8(xf[m][c] + 8 * p, lwv[c][p], rstd);
    }
  }
  // per-token e4m3 quantisation of the prepared row (vq3_quant_fp8_rows contract): q = e4m3(x * 448 / amax)
  float sx[MT];
  if (F::QUANT) {
    float am[MT];
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      am[m] = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < E; ++j) am[m] = fmaxf(am[m], fabsf(xf[m][c][j]));
    }
    combine_slices<true, MT, KS>(am, redm, lane, wid, g);
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const float inv = am[m] > 0.f ? 448.0f / am[m] : 1.0f;
      sx[m] = am[m] > 0.f ? am[m] / 448.0f : 1.0f;
#pragma unroll
      for (int c = 0; c < CH; ++c)
#pragma unroll
        for (int j = 0; j < E; j += 2) {
          const int pk = __builtin_amdgcn_cvt_pk_fp8_f32(xf[m][c][j] * inv, xf[m][c][j + 1] * inv, 0, false);
          const auto back = __builtin_amdgcn_cvt_pk_f32_fp8(pk, false);
          xf[m][c][j] = back[0];
          xf[m][c][j + 1] = back[1];
        }
    }
  }
  float acc[R][MT];
  if (active) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
      for (int m = 0; m < MT; ++m) acc[r][m] = 0.f;
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        float wf[E];
        F::unpack(wv[r][c], wf);          // chunks past K meet x == 0
#pragma unroll
        for (int m = 0; m < MT; ++m)
#pragma unroll
          for (int j = 0; j < E; ++j) acc[r][m] = fmaf(wf[j], xf[m][c][j], acc[r][m]);
      }
    }
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        acc[r][m] = wave_sum(acc[r][m]);
        if (KS > 1 && lane == 0) part[wid][r][m] = acc[r][m];
      }
  }
  if (KS > 1) __syncthreads();
  if (!active || ks != 0 || lane != 0) return;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      if (m >= M || n0 + r >= N) continue;
      float v = acc[r][m];
#pragma unroll
      for (int q = 1; q < KS; ++q) v += part[wid + q][r][m];
      if (F::QUANT) v = rbf(v * (sx[m] * wscale[n0 + r]));
      store_out<F::QUANT>(y, res, v, m, n0 + r, ldy, ldr, out_f32);
    }
}

// ------------------------------------------------------------------------------------------------ dispatch
struct SkinnyArgs {
  const void *x, *W;
  const float* wscale;   // e4m3 only
  void* y;
  const void *res, *ln_w;
  float eps;
  int xmode, M, N, K;
  long ldx, ldw, ldy, ldr;
  int out_f32;
  hipStream_t stream;
};
struct SkinnyPlan {
  bool regx;   // register-resident x, else the generic kernel
  int MT, R, KS;
};

SkinnyPlan plan_bf16(int M, int N, int K, int xmode) {
  const int MT = M <= 2 ? M : (M <= 4 ? 4 : 8);
  const int chunks = (K + 511) / 512;
  // generic kernel: rows per wave so that enough waves cover the chip (256 CUs x >= 8 waves) before growing R
  if (MT > 2) return {false, MT, 4, 1};
  if (chunks > 20) return {false, MT, N >= 16384 ? 4 : (N >= 4096 ? 2 : 1), 1};
  // rows per wave: every wave keeps R * CH 16-byte loads in flight, so few waves per CU already saturate HBM; larger R
  // divides the x traffic from L2 and the per-wave x preparation (RMSNorm / SwiGLU) by R
  const int KS = chunks <= 5 ? 1 : (chunks <= 10 ? 2 : 4);
  const int R = (xmode != 0 || (long)N * KS >= 8192) ? (N >= 1024 ? 4 : (N >= 512 ? 2 : 1)) : 1;
  return {true, MT, R, KS};
}
SkinnyPlan plan_fp8(int M, int K) {
  const int chunks = (K + 1023) / 1024;
  return {true, M, 4, chunks <= 3 ? 1 : (chunks <= 6 ? 2 : 4)};
}

// f(std::integral_constant<int, V>) for the V among Vs that equals v
template <int... Vs, class Fn>
void with_constant(int v, Fn&& f) {
  (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

// Launches the plan's instantiation. Only what a plan can name is built: MT > 2 is generic with R = 4; e4m3 has R = 4; and
// R = 2 never meets xmode 0 in the register-resident kernel (N * KS >= 8192 with KS <= 4 already means N >= 1024, R = 4).
template <class F>
bool launch_skinny(const SkinnyPlan& p, const SkinnyArgs& a) {
  bool launched = false;
  with_constant<1, 2, 4, 8>(p.MT, [&](auto mt) {
    with_constant<1, 2, 4>(p.R, [&](auto r) {
      with_constant<1, 2, 4>(p.KS, [&](auto ks) {
        with_constant<0, 1, 2>(a.xmode, [&](auto xm) {
          constexpr int MT = decltype(mt)::value, R = decltype(r)::value, KS = decltype(ks)::value, XM = decltype(xm)::value;
          const dim3 block(256);
          if constexpr (MT <= 2 && (R == 4 || (!F::QUANT && !(R == 2 && XM == 0)))) {
            if (p.regx) {
              const int rows_per_block = (4 / KS) * R;
              hipLaunchKernelGGL((skinny_regx_kernel<F, MT, R, KS, XM>), dim3((a.N + rows_per_block - 1) / rows_per_block), block,
                                 0, a.stream, (const bf16_t*)a.x, (const typename F::elem*)a.W, a.wscale, a.y, (const bf16_t*)a.res,
                                 (const bf16_t*)a.ln_w, a.eps, a.M, a.N, a.K, a.ldx, a.ldw, a.ldy, a.ldr, a.out_f32);
              launched = true;
            }
          }
          if constexpr (!F::QUANT && KS == 1 && (MT <= 2 || R == 4)) {
            if (!p.regx) {
              hipLaunchKernelGGL((skinny_gemm_kernel<MT, R, XM>), dim3((a.N + 4 * R - 1) / (4 * R)), block, 0, a.stream,
                                 (const bf16_t*)a.x, (const bf16_t*)a.W, a.y, (const bf16_t*)a.res, (const bf16_t*)a.ln_w, a.eps, a.M,
                                 a.N, a.K, a.ldx, a.ldw, a.ldy, a.ldr, a.out_f32);
              launched = true;
            }
          }
        });
      });
    });
  });
  return launched;
}

}  // namespace

extern "C" int vq3_skinny_gemm_bf16(const void* x, const void* W, void* y, const void* residual, const void* ln_w,
                                    float eps, int32_t xmode, int32_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw,
                                    int64_t ldy, int64_t ldr, int32_t out_f32, void* stream) {
  VQ3_CHECK_ARG(x && W && y, "skinny_gemm: null pointer");
  VQ3_CHECK_ARG(M >= 1 && M <= 8, "skinny_gemm: M must be in [1, 8], got %d (use vq3_gemm_bf16_nt)", M);
  VQ3_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0, "skinny_gemm: need N > 0 and K %% 8 == 0 (N=%d K=%d)", N, K);
  VQ3_CHECK_ARG(xmode >= 0 && xmode <= 2 && (xmode != 1 || ln_w), "skinny_gemm: xmode must be 0, 1 (needs ln_w) or 2");
  VQ3_CHECK_ARG(ldx % 8 == 0 && ldw % 8 == 0 && ldx >= (xmode == 2 ? 2l * K : (long)K) && ldw >= K,
                "skinny_gemm: row strides must cover the row and be multiples of 8");
  VQ3_CHECK_ARG(((uintptr_t)x % 16 == 0) && ((uintptr_t)W % 16 == 0) && (!ln_w || (uintptr_t)ln_w % 16 == 0),
                "skinny_gemm: operands must be 16-byte aligned");
  const SkinnyArgs a{x, W, nullptr, y, residual, ln_w, eps, xmode, M, N, K, ldx, ldw, ldy, ldr, out_f32, (hipStream_t)stream};
  VQ3_CHECK_ARG(launch_skinny<Bf16Weights>(plan_bf16(M, N, K, xmode), a), "skinny_gemm: no kernel for M=%d N=%d K=%d", M, N, K);
  VQ3_CHECK_LAUNCH("skinny_gemm");
  return 0;
}

extern "C" int vq3_skinny_gemm_fp8(const void* x, const void* Wq, const float* w_scale, void* y, const void* residual,
                                   const void* ln_w, float eps, int32_t xmode, int32_t M, int32_t N, int32_t K, int64_t ldx,
                                   int64_t ldw, int64_t ldy, int64_t ldr, void* stream) {
  VQ3_CHECK_ARG(x && Wq && w_scale && y, "skinny_gemm_fp8: null pointer");
  VQ3_CHECK_ARG(M >= 1 && M <= 2, "skinny_gemm_fp8: M must be 1 or 2, got %d (prefill / larger batches use vq3_gemm_fp8_nt)", M);
  VQ3_CHECK_ARG(N > 0 && K > 0 && K % 16 == 0 && K <= 12288, "skinny_gemm_fp8: need K %% 16 == 0 and K <= 12288 (N=%d K=%d)", N, K);
  VQ3_CHECK_ARG(xmode >= 0 && xmode <= 2 && (xmode != 1 || ln_w), "skinny_gemm_fp8: xmode must be 0, 1 (needs ln_w) or 2");
  VQ3_CHECK_ARG(ldx % 8 == 0 && ldw % 16 == 0 && ldx >= (xmode == 2 ? 2l * K : (long)K) && ldw >= K,
                "skinny_gemm_fp8: row strides must cover the row (x: multiple of 8, W: multiple of 16)");
  VQ3_CHECK_ARG(((uintptr_t)x % 16 == 0) && ((uintptr_t)Wq % 16 == 0) && (!ln_w || (uintptr_t)ln_w % 16 == 0),
                "skinny_gemm_fp8: operands must be 16-byte aligned");
  const SkinnyArgs a{x, Wq, w_scale, y, residual, ln_w, eps, xmode, M, N, K, ldx, ldw, ldy, ldr, 0, (hipStream_t)stream};
  VQ3_CHECK_ARG(launch_skinny<E4m3Weights>(plan_fp8(M, K), a), "skinny_gemm_fp8: no kernel for M=%d N=%d K=%d", M, N, K);
  VQ3_CHECK_LAUNCH("skinny_gemm_fp8");
  return 0;
}
