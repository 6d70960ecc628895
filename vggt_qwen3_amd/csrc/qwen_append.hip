// A chunk of n > 1 new positions against the resident KV cache: what transformers reaches through `past_key_values`
// (modeling_qwen3.py:237-280 with a DynamicCache: q_norm / k_norm + RoPE at the positions behind the cached prefix, the cache update,
// then causal attention of the new queries over prefix + chunk). qwen_flash.hip assumes query i sits at position i of a
// [B, H, L, 128] tensor of its own length; decode.hip handles one query per row. These two entries fill the gap, so that a cached
// prefix can be extended (multi-turn sessions, chunked prefill) without recomputing it.
//
//  * vq3_qwen_append_qkprep  token t of row b sits at position lens[b] + t: split q|k|v, per-head RMSNorm on q and k, RoPE; K and V go
//                            straight into cache rows lens[b] + t, Q to [B, Hq, Ln, 128]. Rounding points of qkprep_fwd_kernel.
//  * vq3_qwen_append_attn    query t of row b attends cache rows 0 .. lens[b] + t. fwd_block's structure (qwen_flash.hip): one wave per
//                            32-query block and query head, S^T = K Q^T, online softmax per lane, P from the accumulator registers.
// Both launch with fixed arguments and read lens / new_lens from device memory; tokens t >= new_lens[b] are padding (no cache write,
// Q and O rows exactly 0). No atomics: the same bits run after run.
#include "common.h"
#include "qwen_flash_common.h"
#include "vq3_hip.h"

namespace {

constexpr int QK_IT = 6;     // heads per half-wave whose loads are in flight together (48 heads / 8 half-waves)

__device__ __forceinline__ float half_sum(float v) {
#pragma unroll
  for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ void ld2(const bf16_t* p, float& a, float& b) {
  const uint32_t r = *reinterpret_cast<const uint32_t*>(p);
  a = bf2f((bf16_t)(r & 0xffff));
  b = bf2f((bf16_t)(r >> 16));
}

// ------------------------------------------------------------------------------------------------ q/k prep of a chunk
// grid B * Ln, one token per workgroup; a HALF wave owns one head: lane j holds elements 2j, 2j+1 and their rotate-half partners
// 2j+64, 2j+65 (the lane layout and the arithmetic of qkprep_fwd_kernel, qwen_attn.hip - the results are bit-equal to it).
__global__ __launch_bounds__(256) void append_qkprep_kernel(const bf16_t* __restrict__ qkv, const bf16_t* __restrict__ q_w,
                                                           const bf16_t* __restrict__ k_w, const bf16_t* __restrict__ cs,
                                                           const bf16_t* __restrict__ sn, const int32_t* __restrict__ lens,
                                                           const int32_t* __restrict__ new_lens, bf16_t* __restrict__ Q,
                                                           bf16_t* __restrict__ Kc, bf16_t* __restrict__ Vc, int Ln, int Hq,
                                                           int Hkv, int Lmax, float eps) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int j = lane & 31, half = lane >> 5;
  const int e = 2 * j;                       // elements e, e+1 and e+64, e+65
  const long tok = blockIdx.x;               // b*Ln + t
  const int b = (int)(tok / Ln), t = (int)(tok - (long)b * Ln);
  const int HT = Hq + 2 * Hkv;
  const int len = lens[b];
  const int pos = len + t;
  if (t >= new_lens[b] || len < 0 || pos >= Lmax) {
    // padding of the chunk (or a position the cache cannot hold: the host checks capacity first): nothing is cached, Q rows are 0
    for (int h = 2 * wid + half; h < Hq; h += 8) {
      bf16_t* o = Q + (((long)b * Hq + h) * Ln + t) * D;
      *reinterpret_cast<uint32_t*>(o + e) = 0u;
      *reinterpret_cast<uint32_t*>(o + e + 64) = 0u;
    }
    return;
  }
  const bf16_t* row = qkv + tok * (long)HT * D;
  float c1a, c1b, c2a, c2b, s1a, s1b, s2a, s2b;
  ld2(cs + (long)pos * D + e, c1a, c1b); ld2(cs + (long)pos * D + e + 64, c2a, c2b);
  ld2(sn + (long)pos * D + e, s1a, s1b); ld2(sn + (long)pos * D + e + 64, s2a, s2b);
  float wq1a, wq1b, wq2a, wq2b, wk1a, wk1b, wk2a, wk2b;
  ld2(q_w + e, wq1a, wq1b); ld2(q_w + e + 64, wq2a, wq2b);
  ld2(k_w + e, wk1a, wk1b); ld2(k_w + e + 64, wk2a, wk2b);
  for (int hb = 2 * wid + half; hb < HT; hb += 8 * QK_IT) {
    uint32_t xr1[QK_IT], xr2[QK_IT];
#pragma unroll
    for (int i = 0; i < QK_IT; ++i) {
      const int h = hb + 8 * i;
      const int hc = h < HT ? h : HT - 1;
      xr1[i] = *reinterpret_cast<const uint32_t*>(row + hc * D + e);
      xr2[i] = *reinterpret_cast<const uint32_t*>(row + hc * D + e + 64);
    }
#pragma unroll
    for (int i = 0; i < QK_IT; ++i) {
      const int h = hb + 8 * i;
      if (h >= HT) break;
      const float x1a = bf2f((bf16_t)(xr1[i] & 0xffff)), x1b = bf2f((bf16_t)(xr1[i] >> 16));
      const float x2a = bf2f((bf16_t)(xr2[i] & 0xffff)), x2b = bf2f((bf16_t)(xr2[i] >> 16));
      if (h >= Hq + Hkv) {  // value head: plain copy into the cache row
        bf16_t* o = Vc + (((long)b * Hkv + (h - Hq - Hkv)) * Lmax + pos) * D;
        *reinterpret_cast<uint32_t*>(o + e) = pack2bf(x1a, x1b);
        *reinterpret_cast<uint32_t*>(o + e + 64) = pack2bf(x2a, x2b);
        continue;
      }
      const bool isq = h < Hq;
      const float w1a = isq ? wq1a : wk1a, w1b = isq ? wq1b : wk1b, w2a = isq ? wq2a : wk2a, w2b = isq ? wq2b : wk2b;
      const float rs = rsqrtf(half_sum(x1a * x1a + x1b * x1b + x2a * x2a + x2b * x2b) / (float)D + eps);
      const float n1a = rbf(w1a * rbf(x1a * rs)), n1b = rbf(w1b * rbf(x1b * rs));
      const float n2a = rbf(w2a * rbf(x2a * rs)), n2b = rbf(w2b * rbf(x2b * rs));
      // q*cos + rotate_half(q)*sin, each product and the sum rounded to bf16 as the PyTorch bf16 ops do
      const float o1a = rbf(rbf(n1a * c1a) + rbf(-n2a * s1a)), o1b = rbf(rbf(n1b * c1b) + rbf(-n2b * s1b));
      const float o2a = rbf(rbf(n2a * c2a) + rbf(n1a * s2a)), o2b = rbf(rbf(n2b * c2b) + rbf(n1b * s2b));
      bf16_t* o = isq ? Q + (((long)b * Hq + h) * Ln + t) * D : Kc + (((long)b * Hkv + (h - Hq)) * Lmax + pos) * D;
      *reinterpret_cast<uint32_t*>(o + e) = pack2bf(o1a, o1b);
      *reinterpret_cast<uint32_t*>(o + e + 64) = pack2bf(o2a, o2b);
    }
  }
}

// ------------------------------------------------------------------------------------------------ attention of a chunk over the cache
// grid: B * Hkv * nqb blocks of 4 waves (nqb = ceil(Ln / 32)); wave g = query head hk*G + g (G = Hq / Hkv <= 4; spare waves idle).
// fwd_block of qwen_flash.hip with the K / V row stride of the cache, the causal bound key <= lens[b] + q and no key mask (a cache row
// below lens[b] + new_lens[b] is never padding). Query block qb walks the key tiles of rows 0 .. lens[b] + min(32 (qb + 1), new) - 1;
// every K / V row index is clamped to the row's last valid cache row, so what lies behind it (stale rows, NaN) is never loaded. A query
// t >= new has every key masked: its probabilities and its O row are exact zeros; a block without a live query walks no tile at all.
__global__ __launch_bounds__(256) void append_attn_kernel(const bf16_t* __restrict__ Q, const bf16_t* __restrict__ Kc,
                                                         const bf16_t* __restrict__ Vc, const int32_t* __restrict__ lens,
                                                         const int32_t* __restrict__ new_lens, bf16_t* __restrict__ O, int Ln,
                                                         int Hq, int Hkv, int Lmax, long ldo, float scale) {
  __shared__ __attribute__((aligned(16))) char ostage[4][32 * 256];
  const int g = threadIdx.x >> 6;
  const int nqb = (Ln + 31) / 32;
  const int nbh = gridDim.x / nqb;                            // B * Hkv
  const int qb = nqb - 1 - (int)(blockIdx.x / nbh);           // heaviest blocks first (see qwen_flash_fwd_kernel)
  const int hk = (blockIdx.x % nbh) % Hkv, b = (blockIdx.x % nbh) / Hkv;
  const int G = Hq / Hkv, hq = hk * G + g;
  if (g >= G) return;
  const int lane = threadIdx.x & 63;
  const int r = lane & 31, h = lane >> 5;
  // the row's cached and new counts, held to what the cache can hold (the host checks both before it launches)
  int len = lens[b], nw = new_lens[b];
  len = len < 0 ? 0 : (len < Lmax ? len : Lmax);
  nw = nw < 0 ? 0 : (nw < Ln ? nw : Ln);
  nw = nw < Lmax - len ? nw : Lmax - len;
  const int q = qb * 32 + r, qc = q < Ln ? q : Ln - 1;
  const int live = nw - qb * 32;                              // live queries of this block (<= 0: none)
  const int nkeys = live > 0 ? len + (live < 32 ? nw : qb * 32 + 32) : 0;
  const int ntiles = (nkeys + 31) / 32;
  const int maxrow = len + nw > 0 ? len + nw - 1 : 0;         // last valid cache row of (b, hk): < Lmax
  const int qlim = q < nw ? len + q : -1;                     // the last key query q may see; -1: a padded query sees none
  const bf16_t* Qr = Q + (((long)b * Hq + hq) * Ln + qc) * D + 8 * h;
  const bf16_t* Kb = Kc + ((long)b * Hkv + hk) * Lmax * D;
  const bf16_t* Vb = Vc + ((long)b * Hkv + hk) * Lmax * D;
  bf16x8 qf[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) qf[s] = ld8(Qr + 16 * s);
  f32x16 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int i = 0; i < 16; ++i) o[db][i] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float sl2e = scale * LOG2E;
  for (int kb = 0; kb < ntiles; ++kb) {
    // every load of the tile is issued before its first use: one memory round trip per tile; the next tile is touched into L2 meanwhile
    bf16x8 kc[8];
    u32x2 vc[2][8];
    const int nkb = kb + 1 < ntiles ? kb + 1 : kb;
    const unsigned tk = touch_tile(Kb, D, nkb * 32, maxrow), tv = touch_tile(Vb, D, nkb * 32, maxrow);
    rows_load(Kb, D, kb * 32 + r, h, maxrow, kc);
    gather_load(Vb, D, kb * 32, h, r, maxrow, vc);
    f32x16 s;
#pragma unroll
    for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kc[t], qf[t], s, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const bool ok = kb * 32 + rho(i, h) <= qlim;
      s[i] = ok ? s[i] : -INFINITY;
      mx = fmaxf(mx, s[i]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx * sl2e);
    const float m_safe = m_new == -INFINITY ? 0.f : m_new;
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_safe);
    float ps = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      s[i] = __builtin_amdgcn_exp2f(__builtin_fmaf(s[i], sl2e, -m_safe));
      ps += s[i];
    }
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * alpha + ps;
    m_run = m_new;
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int i = 0; i < 16; ++i) o[db][i] *= alpha;
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      bf16x8 vf[4];
      gather_split(vc[sp], vf);
      const bf16x8 pf = pack8(s, sp);
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[db], pf, o[db], 0, 0, 0);
    }
    asm volatile("" ::"v"(tk), "v"(tv));   // keeps the touch loads alive; their wait lands here, after the tile's MFMAs
  }
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    u32x2 w;
    w[0] = pack2bf(o[0][i] * inv, o[1][i] * inv);
    w[1] = pack2bf(o[2][i] * inv, o[3][i] * inv);
    tile_put8(ostage[g], r, rho(i, h), w);
  }
  tile_flush(ostage[g], O + (long)b * Ln * ldo + (long)hq * D, ldo, qb * 32, Ln, lane);
}

}  // namespace

static int append_check(const char* who, int B, int Ln, int Hq, int Hkv, int Dh, int Lmax) {
  VQ3_CHECK_ARG(Dh == D, "%s: head_dim must be %d, got %d", who, D, Dh);
  VQ3_CHECK_ARG(B > 0 && Hq > 0 && Hkv > 0 && Hq % Hkv == 0 && Hq / Hkv <= 4,
                "%s: need 1..4 query heads per kv head (B=%d Hq=%d Hkv=%d)", who, B, Hq, Hkv);
  VQ3_CHECK_ARG(Lmax >= 64 && Lmax <= 12288 && Lmax % 64 == 0, "%s: cache capacity %d must be a multiple of 64 in [64, 12288]", who,
                Lmax);
  VQ3_CHECK_ARG(Ln >= 1 && Ln <= 8192, "%s: chunk length %d outside [1, 8192]", who, Ln);
  VQ3_CHECK_ARG((long)B * Ln < (1l << 31) && (long)B * Hkv * ((Ln + 31) / 32) < (1l << 31), "%s: grid too large", who);
  return 0;
}

extern "C" int vq3_qwen_append_qkprep(const void* qkv, const void* q_w, const void* k_w, const void* cos, const void* sin,
                                      const int32_t* lens, const int32_t* new_lens, void* Q, void* Kcache, void* Vcache, int32_t B,
                                      int32_t Ln, int32_t Hq, int32_t Hkv, int32_t Dh, int32_t Lmax, float eps, void* stream) {
  VQ3_CHECK_ARG(qkv && q_w && k_w && cos && sin && lens && new_lens && Q && Kcache && Vcache, "append_qkprep: null pointer");
  if (append_check("append_qkprep", B, Ln, Hq, Hkv, Dh, Lmax)) return 1;
  hipLaunchKernelGGL(append_qkprep_kernel, dim3(B * Ln), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, (const bf16_t*)q_w,
                     (const bf16_t*)k_w, (const bf16_t*)cos, (const bf16_t*)sin, lens, new_lens, (bf16_t*)Q, (bf16_t*)Kcache,
                     (bf16_t*)Vcache, Ln, Hq, Hkv, Lmax, eps);
  VQ3_CHECK_LAUNCH("append_qkprep");
  return 0;
}

extern "C" int vq3_qwen_append_attn(const void* Q, const void* Kcache, const void* Vcache, const int32_t* lens,
                                    const int32_t* new_lens, void* O, int32_t B, int32_t Ln, int32_t Hq, int32_t Hkv, int32_t Dh,
                                    int32_t Lmax, int64_t ldo, float scale, void* stream) {
  VQ3_CHECK_ARG(Q && Kcache && Vcache && lens && new_lens && O, "append_attn: null pointer");
  if (append_check("append_attn", B, Ln, Hq, Hkv, Dh, Lmax)) return 1;
  VQ3_CHECK_ARG(ldo >= (long)Hq * D && ldo % 8 == 0, "append_attn: bad output row stride");
  const int nqb = (Ln + 31) / 32;
  hipLaunchKernelGGL(append_attn_kernel, dim3(B * Hkv * nqb), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)Q,
                     (const bf16_t*)Kcache, (const bf16_t*)Vcache, lens, new_lens, (bf16_t*)O, Ln, Hq, Hkv, Lmax, (long)ldo, scale);
  VQ3_CHECK_LAUNCH("append_attn");
  return 0;
}
