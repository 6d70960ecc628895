// GEMM v2 for gfx950: LDS-DMA (global_load_lds_dwordx4) staged small-tile kernels, counted vmcnt + raw s_barrier.
//
// C = epilogue(alpha * A[M,K] . B[N,K]^T), NT, K % 64 == 0, bf16 in / f32 MFMA accumulate. The operands never pass through
// VGPRs: the issuing waves send 1-KiB DMA pieces (8 tile rows x 128 B) straight into the
// XOR-swizzled LDS image. The DMA destination is lane-linear (wave-uniform base + lane*16), so the swizzle
// chunk' = chunk ^ (row & 7) is applied to each lane's SOURCE address (lane l reads k-chunk (l&7)^(l>>3) of row l>>3)
// and again on the fragment reads - the same involution on both sides.
// Two schedules, one barrier per 64-deep K step (the configurations are listed at launch_gemm_v2 and in gemm_config.h):
//   NLOAD > 0: an NSTAGE-deep ring (3 or 4) filled by NLOAD dedicated loader waves, one workgroup per CU;
//   NLOAD = 0: two stages, every wave issues its share of tile t+1 before it multiplies tile t, two workgroups per CU.
#include "gemm_common.h"

namespace vq3gemm {
namespace {

constexpr int BK = 64;

template <int BM, int BN, int WM, int WN, int NSTAGE, int NLOAD, bool OUT_F32>
__global__ __launch_bounds__(64 * (WM * WN + NLOAD), (NSTAGE == 2 ? 2 : 1) * ((WM * WN + NLOAD + 3) / 4)) void gemm_v2_kernel(GemmParams p) {
  constexpr int NW = WM * WN;
  constexpr int TM = BM / WM / 16, TN = BN / WN / 16;   // 16x16 MFMA tiles per wave
  constexpr int STAGE = (BM + BN) * 128;                 // bytes per stage
  constexpr int NPIECE = (BM + BN) / 8;                  // 1-KiB pieces per stage
  // NLOAD > 0: dedicated DMA waves (wid >= NW) issue every piece; the compute waves never leave the MFMA/ds_read stream
  constexpr int NISS = NLOAD > 0 ? NLOAD : NW;            // waves that issue DMA
  constexpr int PPW = NPIECE / NISS;                     // pieces per issuing wave per stage
  static_assert(NPIECE % NISS == 0, "pieces must divide evenly over the issuing waves");
  static_assert(NLOAD > 0 ? (NSTAGE == 3 || NSTAGE == 4) : NSTAGE == 2, "a loader ring of 3 or 4 stages, or two stages without loader waves");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = NLOAD > 0 && wid >= NW;
  const int iw = NLOAD > 0 ? (wid >= NW ? wid - NW : 0) : wid;   // index among the issuing waves
  const int wm = (wid % NW) / WN, wn = wid % WN;
  int m0, n0;
  tile_coords(p, BM, BN, m0, n0);
  float ln_mu = 0.f, ln_rs = 0.f;
  ln_row_early<BM, 64 * NW>(p, m0, tid, ln_mu, ln_rs);
  VQ3_BATCH_OPERANDS(p, A, B, coff, roff);

  // ---- DMA source pointers: piece pi = wid + NW*j covers tile rows 8*pi .. 8*pi+7 of [A rows | B rows]
  const int prow = lane >> 3;                       // row inside the piece (== row & 7 of the tile row)
  const int kch = (lane & 7) ^ prow;                // pre-swizzled k-chunk
  const bf16_t* gsrc[PPW];
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    const int pi = iw + NISS * j;
    const int trow = pi * 8 + prow;                 // row in the stacked [A|B] tile
    if (trow < BM) {
      int r = m0 + trow; r = r < p.M ? r : p.M - 1;
      gsrc[j] = A + (long)r * p.lda + kch * 8;
    } else {
      int r = n0 + (trow - BM); r = r < p.N ? r : p.N - 1;
      gsrc[j] = B + (long)r * p.ldb + kch * 8;
    }
  }
  auto issue = [&](int tile, int stage) {
    char* sb = smem + stage * STAGE;
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int pi = iw + NISS * j;
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gsrc[j] + (long)tile * BK),
                                       (__attribute__((address_space(3))) void*)(sb + pi * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int fr = lane & 15, fq = lane >> 4;
  int a_off[TM], b_off[TN];
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int row = wm * (BM / WM) + i * 16 + fr;
    a_off[i] = row * 128 + ((fq ^ (row & 7)) << 4);
  }
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int row = wn * (BN / WN) + j * 16 + fr;
    b_off[j] = BM * 128 + row * 128 + ((fq ^ (row & 7)) << 4);
  }

  const int nt = p.K / BK;
  const int last = nt - 1;
  auto compute = [&](int stage) {
    const char* sb = smem + stage * STAGE;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 xa[TM], wb[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) xa[i] = *reinterpret_cast<const bf16x8*>(sb + (a_off[i] ^ (ks << 6)));
#pragma unroll
      for (int j = 0; j < TN; ++j) wb[j] = *reinterpret_cast<const bf16x8*>(sb + (b_off[j] ^ (ks << 6)));
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wb[j], xa[i], acc[i][j], 0, 0, 0);
    }
  };
  // Epilogue operands (bias / LayerScale column vectors, residual quads) are fetched before the LAST K step's MFMAs so
  // their L2 round trip is hidden; only for the common case (bf16 output, 4-wide aligned rows).
  constexpr bool PRE_RES = TM * TN <= 8;      // the 256-row tiles have no registers to spare for the residual quads
  f32x4 bias_r[TN], cs_r[TN];
  u32x2 res_r[PRE_RES ? TM : 1][TN];
  const bool staged = !OUT_F32 && staged_ok(p, coff, roff);     // LDS-staged epilogue (whole-row stores): gemm_common.h
  const bool pre_ok = !staged && !OUT_F32 && p.vec_ok && (p.bias || p.colscale || p.R);
  auto prefetch_epilogue = [&]() {
    if (!pre_ok) return;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      int n = n0 + wn * (BN / WN) + j * 16 + 4 * fq;
      n = quad_col(p, n);
      if (p.bias) bias_r[j] = *reinterpret_cast<const f32x4*>(p.bias + n);
      if (p.colscale) cs_r[j] = *reinterpret_cast<const f32x4*>(p.colscale + n);
      if (PRE_RES && p.R) {
#pragma unroll
        for (int i = 0; i < (PRE_RES ? TM : 1); ++i) {
          int m = m0 + wm * (BM / WM) + i * 16 + fr;
          m = m < p.M ? m : p.M - 1;
          res_r[i][j] = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(p.R) + roff + (long)m * p.ldr + n);
        }
      }
    }
  };
  if (NLOAD > 0) {
    // producer / consumer split inside the workgroup (one s_barrier per K step for everybody):
    //   loader waves:  wait until their pieces of tile t landed -> barrier -> issue tile t+2
    //   compute waves: barrier -> fragments of tile t -> MFMAs
    if (loader) {
      VQ3_LOADER_RING(NSTAGE, PPW, nt, issue);
      return;
    }
    int stage = 0;
    for (int t = 0; t < last; ++t) {
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      compute(stage);
      stage = stage == NSTAGE - 1 ? 0 : stage + 1;
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    prefetch_epilogue();
    compute(stage);
  } else {
    // two stages, two workgroups per CU: tile t+1 streams in while tile t is multiplied; the co-resident workgroup
    // (its own barrier, naturally out of phase) fills the MFMA pipe while this one waits.
    issue(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    for (int t = 0; t < last; ++t) {
      issue(t + 1, (t + 1) & 1);
      compute(t & 1);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
    }
    prefetch_epilogue();
    compute(last & 1);
  }

  if (!OUT_F32 && staged) {
    VQ3_STAGED_EPILOGUE_RM();
    return;
  }
  VQ3_DIRECT_STORE(TM, TN, m0 + wm * (BM / WM) + i * 16 + fr, n0 + wn * (BN / WN) + j * 16 + 4 * fq, {
    if (pre_ok && n + 3 < p.N) {
      u32x2 rv = res_r[PRE_RES ? i : 0][j];
      if (!PRE_RES && p.R)
        rv = *reinterpret_cast<const u32x2*>(reinterpret_cast<const bf16_t*>(p.R) + roff + (long)m * p.ldr + n);
      store_quad_pre(p, coff, m, n, acc[i][j], bias_r[j], cs_r[j], rv);
    }
    else store_quad<OUT_F32>(p, coff, roff, m, n, acc[i][j]);
  });
}

template <int BM, int BN, int WM, int WN, int NSTAGE, int NLOAD = 0>
int launch_cfg(GemmParams& p, int nbatch, hipStream_t stream) {
  constexpr int SMEM = NSTAGE * (BM + BN) * 128;
  if (int rc = prepare_launch<gemm_v2_kernel<BM, BN, WM, WN, NSTAGE, NLOAD, true>, gemm_v2_kernel<BM, BN, WM, WN, NSTAGE, NLOAD, false>>(
          p, "gemm v2", SMEM, BM, BN, NSTAGE == 2 ? 2 : 1))
    return rc;
  dim3 grid(p.mtiles * p.ntiles, 1, nbatch);
  if (p.out_f32)
    hipLaunchKernelGGL((gemm_v2_kernel<BM, BN, WM, WN, NSTAGE, NLOAD, true>), grid, dim3(64 * (WM * WN + NLOAD)), SMEM, stream, p);
  else
    hipLaunchKernelGGL((gemm_v2_kernel<BM, BN, WM, WN, NSTAGE, NLOAD, false>), grid, dim3(64 * (WM * WN + NLOAD)), SMEM, stream, p);
  return 0;
}

}  // namespace

int launch_gemm_v2(GemmParams& p, int cfg, int nbatch, hipStream_t stream) {
  switch (cfg) {
    case 7: return launch_cfg<128, 128, 4, 2, 2>(p, nbatch, stream);
    case 9: return launch_cfg<128, 128, 4, 2, 3, 4>(p, nbatch, stream);
    case 11: return launch_cfg<256, 128, 4, 2, 3, 2>(p, nbatch, stream);
    case 13: return launch_cfg<128, 128, 4, 2, 4, 2>(p, nbatch, stream);
    // 224 x 128 / 192 x 128 (7 x 2 / 6 x 2 MFMA tiles per wave): M = 6174 = 27.6 x 224 gives 224 tiles for N = 1024 (0.875 fill in
    // one round instead of 0.78) - measured: ties 256 x 128 (the 7 x 2 wave tile moves 0.64 KB of LDS per MFMA, and a single
    // round lasts as long as its slowest tile either way), so the tuner does not list them; kept for vq3_gemm_force_config
    case 15: return launch_cfg<224, 128, 2, 4, 3, 2>(p, nbatch, stream);
    case 16: return launch_cfg<192, 128, 2, 4, 3, 2>(p, nbatch, stream);
    // 192 x 128, FOUR waves (96 x 64 each: 0.42 KB of LDS per MFMA), 2 stages = 80 KiB: TWO workgroups per CU, each one wave per SIMD.
    // At K = 1024 a tile's epilogue (staging C through LDS + the row stores: 8-9 us of a 24 us tile on the 8-wave kernels, during which
    // the MFMA pipe idles - tools/gemm_stamps.py) runs under the co-resident workgroup's main loop; M = 49 392 = 257.25 x 192.
    case 17: return launch_cfg<192, 128, 2, 2, 2>(p, nbatch, stream);
    default: return -1;      // not a configuration of this file (gemm_config.h lists them): nothing launched
  }
}

}  // namespace vq3gemm
