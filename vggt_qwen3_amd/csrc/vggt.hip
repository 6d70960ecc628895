// VGGT aggregator kernels (multi-view ViT) in front of the attention: patch im2col with fused ImageNet normalisation, and per-head
// q/k LayerNorm + 2-D RoPE + head split. The attention itself is vggt_flash.hip.
#include <cstdlib>

#include "common.h"
#include "vq3_hip.h"

namespace {

// ------------------------------------------------------------------------------------------------ im2col
// images f32 [NI, 3, H, W] in [0,1]; out bf16 [NI*Hp*Wp, Kp], k = c*p*p + ky*p + kx, columns >= 3*p*p zero.
// The reference casts images to bf16 first and normalises in bf16 (two rounded ops).
__global__ __launch_bounds__(256) void im2col_norm_kernel(const float* __restrict__ img, bf16_t* __restrict__ out,
                                                          int H, int W, int p, int Hp, int Wp, int Kp, float m0,
                                                          float m1, float m2, float s0, float s1, float s2) {
  const long patch = blockIdx.x;  // ni*Hp*Wp + py*Wp + px
  const int px = (int)(patch % Wp), py = (int)((patch / Wp) % Hp);
  const long ni = patch / ((long)Wp * Hp);
  const int K = 3 * p * p;
  bf16_t* o = out + patch * (long)Kp;
  for (int k = threadIdx.x; k < Kp; k += 256) {
    float v = 0.f;
    if (k < K) {
      const int c = k / (p * p), r = k - c * p * p, ky = r / p, kx = r - ky * p;
      const float x = rbf(img[((ni * 3 + c) * H + (py * p + ky)) * (long)W + (px * p + kx)]);
      const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2);
      const float sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
      v = rbf(rbf(x - rbf(mean)) / rbf(sd));
    }
    o[k] = f2bf(v);
  }
}

// ------------------------------------------------------------------------------------------------ q/k prep
// qkv bf16 [T, 3*C] (columns: q heads | k heads | v heads, head-major) -> Q,K,V bf16 [G, NH, N, 64], T = G*N.
// Optional LayerNorm over the 64 head features (qk_norm) and 2-D RoPE: the first 32 features rotate with the
// patch row (y), the last 32 with the patch column (x), rotate-half inside each 32-block; tokens < patch_start of a
// frame sit at position 0 (identity). cos/sin tables bf16 [maxpos+1, 32].
__global__ __launch_bounds__(256) void vit_qkprep_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ qn_w,
                                                         const float* __restrict__ qn_b, const float* __restrict__ kn_w,
                                                         const float* __restrict__ kn_b, const bf16_t* __restrict__ cs,
                                                         const bf16_t* __restrict__ sn, bf16_t* __restrict__ Q,
                                                         bf16_t* __restrict__ K, bf16_t* __restrict__ V, int N, int NH,
                                                         int P, int patch_start, int Wp, int use_norm, int use_rope,
                                                         float eps) {
  // A wave handles two heads per pass (lanes 0-31 / 32-63), a lane two adjacent features (one 4-byte access):
  // the LayerNorm sums stay inside a 32-lane half, the rotate-half partner of feature e is e^16 = lane^8.
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l32 = lane & 31, half = lane >> 5;
  const long t = blockIdx.x;
  const long g = t / N;
  const int n = (int)(t - g * N);
  const int C = NH * 64;
  const bf16_t* row = qkv + t * 3L * C;
  int py = 0, px = 0;
  if (use_rope) {
    const int tp = n % P;
    if (tp >= patch_start) {
      py = (tp - patch_start) / Wp + 1;
      px = (tp - patch_start) % Wp + 1;
    }
  }
  const int e0 = 2 * l32;                       // features e0, e0+1 of the head
  const int pos = l32 < 16 ? py : px;
  const int f0 = e0 & 31;
  float c0 = 1.f, c1 = 1.f, s0 = 0.f, s1 = 0.f;
  if (use_rope) {
    c0 = bf2f(cs[pos * 32 + f0]); c1 = bf2f(cs[pos * 32 + f0 + 1]);
    s0 = bf2f(sn[pos * 32 + f0]); s1 = bf2f(sn[pos * 32 + f0 + 1]);
  }
  const bool neg = (l32 & 8) == 0;              // (e & 16) == 0 -> rotate-half takes -x[e+16]
  for (int hp = wid; hp < (3 * NH) / 2; hp += 4) {
    const int hh = 2 * hp + half;
    const int which = hh / NH, h = hh - which * NH;
    const uint32_t raw = *reinterpret_cast<const uint32_t*>(row + which * C + h * 64 + e0);
    float x0 = bf2f((bf16_t)(raw & 0xffff)), x1 = bf2f((bf16_t)(raw >> 16));
    bf16_t* dst = (which == 0 ? Q : (which == 1 ? K : V)) + ((g * NH + h) * (long)N + n) * 64 + e0;
    if (which < 2) {
      if (use_norm) {
        float sum = x0 + x1;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float mean = sum * (1.f / 64.f);
        const float d0 = x0 - mean, d1 = x1 - mean;
        float sq = d0 * d0 + d1 * d1;
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        const float rs = rsqrtf(sq * (1.f / 64.f) + eps);
        const float* w = which == 0 ? qn_w : kn_w;
        const float* b = which == 0 ? qn_b : kn_b;
        x0 = rbf(d0 * rs * w[e0] + b[e0]);
        x1 = rbf(d1 * rs * w[e0 + 1] + b[e0 + 1]);
      }
      if (use_rope) {
        const float p0 = __shfl_xor(x0, 8, 64), p1 = __shfl_xor(x1, 8, 64);
        const float r0 = neg ? -p0 : p0, r1 = neg ? -p1 : p1;
        x0 = rbf(rbf(x0 * c0) + rbf(r0 * s0));
        x1 = rbf(rbf(x1 * c1) + rbf(r1 * s1));
      }
    }
    *reinterpret_cast<uint32_t*>(dst) = pack2bf(x0, x1);
  }
}

// Same contract with 4 features (8 bytes) per lane: 16 lanes per head, four heads per wave pass - half the memory
// instructions of the 2-feature form. Needs NH % 4 == 0. LayerNorm sums stay inside a 16-lane quarter, the rotate-half
// partner of feature e is e ^ 16 = lane ^ 4 (same element slot).
__global__ __launch_bounds__(256) void vit_qkprep4_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ qn_w,
                                                          const float* __restrict__ qn_b, const float* __restrict__ kn_w,
                                                          const float* __restrict__ kn_b, const bf16_t* __restrict__ cs,
                                                          const bf16_t* __restrict__ sn, bf16_t* __restrict__ Q,
                                                          bf16_t* __restrict__ K, bf16_t* __restrict__ V, int N, int NH,
                                                          int P, int patch_start, int Wp, int use_norm, int use_rope,
                                                          float eps) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int l16 = lane & 15, quarter = lane >> 4;
  const long t = blockIdx.x;
  const long g = t / N;
  const int n = (int)(t - g * N);
  const int C = NH * 64;
  const bf16_t* row = qkv + t * 3L * C;
  int py = 0, px = 0;
  if (use_rope) {
    const int tp = n % P;
    if (tp >= patch_start) {
      py = (tp - patch_start) / Wp + 1;
      px = (tp - patch_start) % Wp + 1;
    }
  }
  const int e0 = 4 * l16;                       // features e0 .. e0+3 of the head
  const int pos = l16 < 8 ? py : px;
  const int f0 = e0 & 31;
  float c[4] = {1.f, 1.f, 1.f, 1.f}, sv[4] = {0.f, 0.f, 0.f, 0.f};
  if (use_rope) {
    const u32x2 cr = *reinterpret_cast<const u32x2*>(cs + pos * 32 + f0);
    const u32x2 sr = *reinterpret_cast<const u32x2*>(sn + pos * 32 + f0);
    c[0] = bf2f((bf16_t)(cr[0] & 0xffff)); c[1] = bf2f((bf16_t)(cr[0] >> 16));
    c[2] = bf2f((bf16_t)(cr[1] & 0xffff)); c[3] = bf2f((bf16_t)(cr[1] >> 16));
    sv[0] = bf2f((bf16_t)(sr[0] & 0xffff)); sv[1] = bf2f((bf16_t)(sr[0] >> 16));
    sv[2] = bf2f((bf16_t)(sr[1] & 0xffff)); sv[3] = bf2f((bf16_t)(sr[1] >> 16));
  }
  const bool neg = (l16 & 4) == 0;              // (e & 16) == 0 -> rotate-half takes -x[e+16]
  for (int hq = wid; hq < (3 * NH) / 4; hq += 4) {
    const int hh = 4 * hq + quarter;
    const int which = hh / NH, h = hh - which * NH;
    const u32x2 raw = *reinterpret_cast<const u32x2*>(row + which * C + h * 64 + e0);
    float x[4] = {bf2f((bf16_t)(raw[0] & 0xffff)), bf2f((bf16_t)(raw[0] >> 16)), bf2f((bf16_t)(raw[1] & 0xffff)),
                  bf2f((bf16_t)(raw[1] >> 16))};
    bf16_t* dst = (which == 0 ? Q : (which == 1 ? K : V)) + ((g * NH + h) * (long)N + n) * 64 + e0;
    if (which < 2) {
      if (use_norm) {
        float sum = (x[0] + x[1]) + (x[2] + x[3]);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        const float mean = sum * (1.f / 64.f);
        float d[4], sq = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) { d[j] = x[j] - mean; sq = fmaf(d[j], d[j], sq); }
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sq += __shfl_xor(sq, o, 64);
        const float rs = rsqrtf(sq * (1.f / 64.f) + eps);
        const f32x4 w = *reinterpret_cast<const f32x4*>((which == 0 ? qn_w : kn_w) + e0);
        const f32x4 b = *reinterpret_cast<const f32x4*>((which == 0 ? qn_b : kn_b) + e0);
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = rbf(d[j] * rs * w[j] + b[j]);
      }
      if (use_rope) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float pj = __shfl_xor(x[j], 4, 64);
          const float rj = neg ? -pj : pj;
          x[j] = rbf(rbf(x[j] * c[j]) + rbf(rj * sv[j]));
        }
      }
    }
    u32x2 o;
    o[0] = pack2bf(x[0], x[1]);
    o[1] = pack2bf(x[2], x[3]);
    *reinterpret_cast<u32x2*>(dst) = o;
  }
}

}  // namespace

extern "C" int vq3_im2col_norm(const float* images, void* patches, int32_t NI, int32_t H, int32_t W, int32_t p,
                               int32_t Kp, const float* mean3_host, const float* std3_host, void* stream) {
  VQ3_CHECK_ARG(images && patches && mean3_host && std3_host, "im2col_norm: null pointer");
  VQ3_CHECK_ARG(NI > 0 && p > 0 && H % p == 0 && W % p == 0 && Kp >= 3 * p * p, "im2col_norm: bad shape");
  const int Hp = H / p, Wp = W / p;
  hipLaunchKernelGGL(im2col_norm_kernel, dim3((unsigned)((long)NI * Hp * Wp)), dim3(256), 0, (hipStream_t)stream, images,
                     (bf16_t*)patches, H, W, p, Hp, Wp, Kp, mean3_host[0], mean3_host[1], mean3_host[2], std3_host[0],
                     std3_host[1], std3_host[2]);
  VQ3_CHECK_LAUNCH("im2col_norm");
  return 0;
}

extern "C" int vq3_vit_qkprep(const void* qkv, const float* qn_w, const float* qn_b, const float* kn_w,
                              const float* kn_b, const void* cos, const void* sin, void* Q, void* K, void* V, int64_t T,
                              int32_t N, int32_t NH, int32_t head_dim, int32_t tokens_per_frame, int32_t patch_start,
                              int32_t Wp, int32_t use_norm, int32_t use_rope, float eps, void* stream) {
  VQ3_CHECK_ARG(qkv && Q && K && V, "vit_qkprep: null pointer");
  VQ3_CHECK_ARG(head_dim == 64, "vit_qkprep: head_dim must be 64, got %d", head_dim);
  VQ3_CHECK_ARG(T > 0 && N > 0 && T % N == 0 && NH > 0 && NH % 2 == 0, "vit_qkprep: bad shape (NH must be even)");
  VQ3_CHECK_ARG(!use_norm || (qn_w && qn_b && kn_w && kn_b), "vit_qkprep: norm weights missing");
  VQ3_CHECK_ARG(!use_rope || (cos && sin && tokens_per_frame > 0 && Wp > 0), "vit_qkprep: rope tables missing");
  const char* force2 = getenv("VQ3_VIT_QKPREP_VEC2");   // tests: compare the two lane layouts on the same input
  const bool vec4 = !(force2 && force2[0] == '1') && NH % 4 == 0 && (!use_norm || (((uintptr_t)qn_w | (uintptr_t)qn_b | (uintptr_t)kn_w | (uintptr_t)kn_b) % 16 == 0)) &&
                    (!use_rope || (((uintptr_t)cos | (uintptr_t)sin) % 8 == 0));
  if (vec4)
    hipLaunchKernelGGL(vit_qkprep4_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, qn_w,
                       qn_b, kn_w, kn_b, (const bf16_t*)cos, (const bf16_t*)sin, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)V, N, NH,
                       tokens_per_frame, patch_start, Wp, use_norm, use_rope, eps);
  else
    hipLaunchKernelGGL(vit_qkprep_kernel, dim3((unsigned)T), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)qkv, qn_w,
                       qn_b, kn_w, kn_b, (const bf16_t*)cos, (const bf16_t*)sin, (bf16_t*)Q, (bf16_t*)K, (bf16_t*)V, N, NH,
                       tokens_per_frame, patch_start, Wp, use_norm, use_rope, eps);
  VQ3_CHECK_LAUNCH("vit_qkprep");
  return 0;
}
