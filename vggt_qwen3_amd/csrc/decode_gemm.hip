// Decode-time weight-streaming GEMM for 1..64 rows: y[M, N] = f(x) W^T (+ residual), the contract of vq3_skinny_gemm_bf16 (same
// xmode transforms and rounding points, decode_x.h) on the matrix cores. One new token per row and step: the weights are streamed
// once, so the kernel is HBM-bound like the FMA kernels of skinny_gemm.hip - at MT = 4 the MFMA rate corresponds to ~38 TB/s of weights.
//
//  * A workgroup (4 waves) owns 64 weight rows and one K slice; a wave owns 16 of the rows: they are the A operand of
//    v_mfma_f32_16x16x32_bf16, 16 batch rows are the B operand, so one weight fragment feeds MT = ceil(M / 16) MFMAs.
//  * W goes straight to VGPRs by nontemporal 16-byte loads, never through LDS: a chunk of 256 k is 8 loads per lane, and the next
//    chunk's 8 are issued before this chunk's MFMAs. An MFMA sums over k in any order, so inside a 64-wide K block lane (row i, group g)
//    takes k = 16 g + 8 p + j for its two fragments p: 32 contiguous bytes per lane, the block's whole 128-byte line of row i per
//    4 lanes. x is laid out in LDS with the same assignment.
//  * x is prepared once per workgroup and chunk (RMSNorm weight, or SwiGLU), written to LDS as bf16 in B-fragment order and shared
//    by the 4 waves: x bytes from L2 per weight byte from HBM = M / 64 <= 1. The RMSNorm statistic is taken once per workgroup,
//    summed exactly as skinny_gemm_kernel sums it (lane-strided 8-element pieces, 512 per trip, then wave_sum).
//  * N < 16384 does not fill 256 CUs with 64-row workgroups: K is cut into KS = 2, 4 or 8 slices over gridDim.y. Every slice stores
//    its fp32 tile to the caller's workspace with plain 16-byte stores, and a second, small kernel adds the KS tiles in slice order
//    0 .. KS - 1 and runs the epilogue. The kernel boundary is the only synchronisation: no tickets, no fences, no floating-point
//    atomics, and the bits do not depend on the order in which the slices finish. (A first version combined inside the launch, the
//    last workgroup to draw a ticket adding the tiles: its agent-scope release / acquire pair per workgroup cost more than the
//    boundary - o_proj at 16 rows took 23 us.)
#include <type_traits>

#include "common.h"
#include "decode_x.h"
#include "vq3_hip.h"

namespace {

constexpr int DG_ROWS = 64;      // weight rows per workgroup
constexpr int DG_KB = 64;        // k per block: two MFMAs per batch tile
constexpr int DG_KC = 256;       // k per LDS chunk of x: MT * 8 KiB
constexpr int DG_NB = DG_KC / DG_KB;
constexpr int DG_MAX_KS = 8;
constexpr int DG_FILL = 256;     // workgroups wanted before K is left whole (one per CU)

template <int MT, int XMODE>
__global__ __launch_bounds__(256) void decode_gemm_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ W,
                                                         void* __restrict__ y, const bf16_t* __restrict__ res,
                                                         const bf16_t* __restrict__ ln_w, float eps, int M, int N, int K, long ldx,
                                                         long ldw, long ldy, long ldr, int out_f32, int chunks_per_slice,
                                                         f32x4* __restrict__ slabs) {
  __shared__ u32x4 xs[DG_NB][MT][2][64];     // [K block][batch tile][fragment p][lane]: what lane reads for MFMA (block, tile, p)
  __shared__ float rstd_s[MT * 16];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int fi = lane & 15, fg = lane >> 4;
  const int n0 = blockIdx.x * DG_ROWS + wid * 16;
  const bool active = n0 < N;               // wave-uniform: a wave past N streams nothing and stores nothing
  const int KS = gridDim.y, ks = blockIdx.y;
  const int c_begin = ks * chunks_per_slice;
  const int c_end = min((K + DG_KC - 1) / DG_KC, c_begin + chunks_per_slice);      // an empty slice contributes zeros

  const bf16_t* wrow = W + (long)min(n0 + fi, N - 1) * ldw;
  // the 8 weight pieces of chunk c; a piece past K is a clamped duplicate that meets x == 0
  auto load_w = [&](int c, u32x4 (&wv)[DG_NB][2]) {
#pragma unroll
    for (int b = 0; b < DG_NB; ++b)
#pragma unroll
      for (int p = 0; p < 2; ++p)
        wv[b][p] = __builtin_nontemporal_load((const u32x4*)(wrow + min(c * DG_KC + b * DG_KB + fg * 16 + p * 8, K - 8)));
  };
  // chunk c of f(x) goes to LDS in two halves, so that its loads (from L2) are in flight under the chunk before it. A wave's job is
  // one (K block, batch tile, half h): lane (i, q) prepares the 8 elements k = 8 (q + 4 h) of batch row i - 64 contiguous bytes per
  // row from L2, 256 contiguous bytes per 16 lanes into LDS
  u32x4 xr[2 * MT], xe[XMODE == 0 ? 1 : 2 * MT];          // raw x pieces; xe: the RMSNorm weight (xmode 1) or the up half (xmode 2)
  auto job_k = [&](int c, int u) {
    const int job = wid + 4 * u;
    return c * DG_KC + ((job >> 1) / MT) * DG_KB + (fg + 4 * (job & 1)) * 8;
  };
  auto job_m = [&](int u) { return min((((wid + 4 * u) >> 1) % MT) * 16 + fi, M - 1); };
  auto load_x = [&](int c) {
#pragma unroll
    for (int u = 0; u < 2 * MT; ++u) {
      const int k = job_k(c, u);
      if (k < K) {
        const bf16_t* row = x + (long)job_m(u) * ldx;
        xr[u] = *(const u32x4*)(row + k);
        if (XMODE == 1) xe[u] = *(const u32x4*)(ln_w + k);
        if (XMODE == 2) xe[u] = *(const u32x4*)(row + K + k);
      }
    }
  };
  auto store_x = [&](int c) {
#pragma unroll
    for (int u = 0; u < 2 * MT; ++u) {
      const int job = wid + 4 * u;
      const int q = fg + 4 * (job & 1), t = (job >> 1) % MT, b = (job >> 1) / MT;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (job_k(c, u) < K) {
        float f[8];
        unpack8(xr[u], f);
        if (XMODE == 1) rmsnorm8(f, xe[u], rstd_s[job_m(u)]);
        if (XMODE == 2) swiglu8(f, xe[u]);
        v = u32x4{pack2bf(f[0], f[1]), pack2bf(f[2], f[3]), pack2bf(f[4], f[5]), pack2bf(f[6], f[7])};
      }
      xs[b][t][q & 1][(q >> 1) * 16 + fi] = v;
    }
  };

  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  u32x4 wa[DG_NB][2], wb[DG_NB][2];
  if (c_begin < c_end) {                                    // the weight stream does not depend on x: first in flight
    if (active) load_w(c_begin, wa);
    load_x(c_begin);
  }

  if (XMODE == 1) {
    // the statistic of a row as skinny_gemm_kernel takes it: lane-strided 8-element pieces, 512 per trip, then wave_sum. A wave
    // takes 8 rows at a time so that 8 (16 with the unrolled trip) loads are in flight, not one
    constexpr int SR = 8;
    for (int m0 = wid * SR; m0 < M; m0 += 4 * SR) {
      float ss[SR];
#pragma unroll
      for (int j = 0; j < SR; ++j) ss[j] = 0.f;
#pragma unroll 2
      for (int k = lane * 8; k < K; k += 512) {
        u32x4 v[SR];
#pragma unroll
        for (int j = 0; j < SR; ++j) v[j] = *(const u32x4*)(x + (long)min(m0 + j, M - 1) * ldx + k);
#pragma unroll
        for (int j = 0; j < SR; ++j) {
          float f[8];
          unpack8(v[j], f);
          ss[j] = sumsq8(f, ss[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < SR; ++j) {
        const float s = wave_sum(ss[j]);
        if (lane == 0 && m0 + j < M) rstd_s[m0 + j] = rsqrtf(s / (float)K + eps);
      }
    }
    __syncthreads();
  }

  // one chunk: the next chunk's weights are requested into wn before this chunk's x is written, and the next chunk's x before
  // this chunk is multiplied with wc
  auto step = [&](int c, u32x4 (&wc)[DG_NB][2], u32x4 (&wn)[DG_NB][2]) {
    if (active && c + 1 < c_end) load_w(c + 1, wn);
    store_x(c);
    __syncthreads();
    if (c + 1 < c_end) load_x(c + 1);
    if (active) {
#pragma unroll
      for (int b = 0; b < DG_NB; ++b)
#pragma unroll
        for (int p = 0; p < 2; ++p)
#pragma unroll
          for (int t = 0; t < MT; ++t)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, wc[b][p]),
                                                            __builtin_bit_cast(bf16x8, xs[b][t][p][lane]), acc[t], 0, 0, 0);
    }
    __syncthreads();                       // xs is rewritten by the next chunk
  };
  for (int c = c_begin; c < c_end; c += 2) {
    step(c, wa, wb);
    if (c + 1 < c_end) step(c + 1, wb, wa);
  }

  // lane (fi, fg) holds y[m = 16 t + fi][n = n0 + 4 fg + r] in acc[t][r]
  if (!active) return;
  if (KS > 1) {          // slice ks of the tile: [workgroup][wave][batch tile][lane] x 4 floats; decode_combine_kernel finishes
    f32x4* mine = slabs + (((long)ks * gridDim.x + blockIdx.x) * 4 + wid) * (MT * 64) + lane;
#pragma unroll
    for (int t = 0; t < MT; ++t) mine[t * 64] = acc[t];
    return;
  }
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = t * 16 + fi, n = n0 + 4 * fg + r;
      if (m < M && n < N) store_out<false>(y, res, acc[t][r], m, n, ldy, ldr, out_f32);
    }
}

// The K slices of decode_gemm_kernel, added in slice order, and its epilogue. One thread per f32x4 of a tile, in the slabs' own order.
template <int MT>
__global__ __launch_bounds__(256) void decode_combine_kernel(const f32x4* __restrict__ slabs, void* __restrict__ y,
                                                            const bf16_t* __restrict__ res, int M, int N, long ldy, long ldr,
                                                            int out_f32, int KS) {
  const int lane = threadIdx.x & 63;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;           // ((workgroup * 4 + wave) * MT + batch tile) * 64 + lane
  const long wave = e / (MT * 64);
  const int t = (int)((e >> 6) % MT);
  const int n0 = (int)wave * 16;
  if (n0 >= N) return;                                           // that wave stored nothing
  const long slice = (long)gridDim.x * 256;
  f32x4 part[DG_MAX_KS];
#pragma unroll
  for (int s = 0; s < DG_MAX_KS; ++s)
    if (s < KS) part[s] = slabs[s * slice + e];
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < DG_MAX_KS; ++s)
    if (s < KS) v += part[s];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = t * 16 + (lane & 15), n = n0 + 4 * (lane >> 4) + r;
    if (m < M && n < N) store_out<false>(y, res, v[r], m, n, ldy, ldr, out_f32);
  }
}

// ------------------------------------------------------------------------------------------------ dispatch
struct DecodePlan {
  int MT;                 // batch tiles of 16 rows
  int KS;                 // K slices (gridDim.y)
  int chunks_per_slice;   // chunks of DG_KC per slice
  int groups;             // workgroups per slice (gridDim.x)
};

// Every (MT, xmode) is one instantiation and KS is a run-time grid dimension: 12 kernels and 4 combine kernels, all reachable. K is
// halved while the grid has fewer than one workgroup per CU, a slice keeps at least two chunks, and KS stops at 8.
DecodePlan plan_decode(int M, int N, int K) {
  const int groups = (N + DG_ROWS - 1) / DG_ROWS, chunks = (K + DG_KC - 1) / DG_KC;
  int KS = 1;
  while (KS < DG_MAX_KS && groups * KS < DG_FILL && 2 * KS <= chunks) KS *= 2;
  return {(M + 15) / 16, KS, (chunks + KS - 1) / KS, groups};
}

// workspace: KS slices of [groups][4 waves][MT][64 lanes] x 4 floats
size_t workspace_bytes(const DecodePlan& p) { return p.KS == 1 ? 0 : (size_t)p.KS * p.groups * 4 * p.MT * 256 * sizeof(float); }

template <int... Vs, class Fn>
void with_constant(int v, Fn&& f) {
  (void)((v == Vs && (f(std::integral_constant<int, Vs>{}), true)) || ...);
}

}  // namespace

extern "C" int64_t vq3_decode_gemm_workspace_bytes(int32_t M, int32_t N, int32_t K) {
  if (M < 1 || M > 64 || N < 1 || K < 8) return 0;
  return (int64_t)workspace_bytes(plan_decode(M, N, K));
}

extern "C" int vq3_decode_gemm_bf16(const void* x, const void* W, void* y, const void* residual, const void* ln_w, float eps,
                                    int32_t xmode, int32_t M, int32_t N, int32_t K, int64_t ldx, int64_t ldw, int64_t ldy,
                                    int64_t ldr, int32_t out_f32, void* workspace, int64_t workspace_bytes_given, void* stream) {
  VQ3_CHECK_ARG(x && W && y, "decode_gemm: null pointer");
  VQ3_CHECK_ARG(M >= 1 && M <= 64, "decode_gemm: M must be in [1, 64], got %d (use vq3_gemm_bf16_nt)", M);
  VQ3_CHECK_ARG(N > 0 && K > 0 && K % 8 == 0, "decode_gemm: need N > 0 and K %% 8 == 0 (N=%d K=%d)", N, K);
  VQ3_CHECK_ARG(xmode >= 0 && xmode <= 2 && (xmode != 1 || ln_w), "decode_gemm: xmode must be 0, 1 (needs ln_w) or 2");
  VQ3_CHECK_ARG(ldx % 8 == 0 && ldw % 8 == 0 && ldx >= (xmode == 2 ? 2l * K : (long)K) && ldw >= K,
                "decode_gemm: row strides must cover the row and be multiples of 8");
  VQ3_CHECK_ARG(((uintptr_t)x % 16 == 0) && ((uintptr_t)W % 16 == 0) && (!ln_w || (uintptr_t)ln_w % 16 == 0),
                "decode_gemm: operands must be 16-byte aligned");
  const DecodePlan p = plan_decode(M, N, K);
  const size_t need = workspace_bytes(p);
  VQ3_CHECK_ARG(need == 0 || (workspace && (uintptr_t)workspace % 16 == 0 && workspace_bytes_given >= (int64_t)need),
                "decode_gemm: M=%d N=%d K=%d is cut into %d K slices and needs %zu bytes of 16-byte aligned workspace "
                "(vq3_decode_gemm_workspace_bytes), got %lld", M, N, K, p.KS, need, (long long)(workspace ? workspace_bytes_given : 0));
  hipStream_t s = (hipStream_t)stream;
  f32x4* slabs = (f32x4*)workspace;
  bool launched = false;
  with_constant<1, 2, 3, 4>(p.MT, [&](auto mt) {
    with_constant<0, 1, 2>(xmode, [&](auto xm) {
      hipLaunchKernelGGL((decode_gemm_kernel<decltype(mt)::value, decltype(xm)::value>), dim3(p.groups, p.KS), dim3(256), 0, s,
                         (const bf16_t*)x, (const bf16_t*)W, y, (const bf16_t*)residual, (const bf16_t*)ln_w, eps, M, N, K, (long)ldx,
                         (long)ldw, (long)ldy, (long)ldr, out_f32, p.chunks_per_slice, slabs);
      if (p.KS > 1)
        hipLaunchKernelGGL((decode_combine_kernel<decltype(mt)::value>), dim3(p.groups * decltype(mt)::value), dim3(256), 0, s, slabs, y,
                           (const bf16_t*)residual, M, N, (long)ldy, (long)ldr, out_f32, p.KS);
      launched = true;
    });
  });
  VQ3_CHECK_ARG(launched, "decode_gemm: no kernel for M=%d N=%d K=%d", M, N, K);
  VQ3_CHECK_LAUNCH("decode_gemm");
  return 0;
}
