// Shared device helpers for the gfx950 (MI355X / CDNA4) kernels of the VGGT -> Perceiver -> Qwen3 path.
// Wave = 64 lanes everywhere; bf16 is carried as raw uint16 and converted through the native __bf16 type
// (v_cvt_pk_bf16_f32: round-to-nearest-even, NaN stays NaN).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

typedef uint16_t bf16_t;
typedef __attribute__((ext_vector_type(8))) short bf16x8;   // one MFMA A/B fragment (4 VGPRs)
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;

#define VQ3_WAVE 64

__device__ __forceinline__ float bf2f(bf16_t v) {
  return __builtin_bit_cast(float, (uint32_t)v << 16);
}
__device__ __forceinline__ bf16_t f2bf(float f) {
  __bf16 b = (__bf16)f;
  return __builtin_bit_cast(bf16_t, b);
}
// round a float through bf16 (emulates a PyTorch op that returns a bf16 tensor)
__device__ __forceinline__ float rbf(float f) { return bf2f(f2bf(f)); }

// two floats -> one dword of two bf16 (lo in bits 0-15): ONE v_cvt_pk_bf16_f32 (round-to-nearest-even, NaN stays NaN). Written as
// two scalar casts + shift + or, hipcc 7.2 emits two conversions, a shift and an SDWA or - four instructions for every pair of every
// epilogue and element-wise kernel.
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 vq3_bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pack2bf(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{lo, hi}, vq3_bf16x2_t));
}
__device__ __forceinline__ f32x2_t unpack2bf(uint32_t u) {
  return f32x2_t{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}
// one 16-byte piece of 8 bf16 -> 8 floats
__device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
  f[0] = __builtin_bit_cast(float, v.x << 16); f[1] = __builtin_bit_cast(float, v.x & 0xffff0000u);
  f[2] = __builtin_bit_cast(float, v.y << 16); f[3] = __builtin_bit_cast(float, v.y & 0xffff0000u);
  f[4] = __builtin_bit_cast(float, v.z << 16); f[5] = __builtin_bit_cast(float, v.z & 0xffff0000u);
  f[6] = __builtin_bit_cast(float, v.w << 16); f[7] = __builtin_bit_cast(float, v.w & 0xffff0000u);
}
// a pair rounded through bf16 (three instructions: the conversion, a shift and a mask)
__device__ __forceinline__ f32x2_t rbf2(f32x2_t v) {
  const uint32_t u = pack2bf(v[0], v[1]);
  return f32x2_t{__builtin_bit_cast(float, u << 16), __builtin_bit_cast(float, u & 0xffff0000u)};
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// Block-wide sum for blocks of NW waves. `red` must hold >= NW floats of LDS.
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  if (NW == 1) return v;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) t += red[i];
  return t;
}
template <int NW>
__device__ __forceinline__ float block_max(float v, float* red) {
  v = wave_max(v);
  if (NW == 1) return v;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  float t = red[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) t = fmaxf(t, red[i]);
  return t;
}

// A row walked by NT threads (a wave, by default) in chunks of W consecutive elements per thread: f(chunk index, the thread's first
// column in that chunk). NCH > 0: NCH chunks, fully unrolled, a chunk past `cols` skipped - the form for rows that live in registers
// indexed by the chunk. NCH == 0: any width, a run-time loop.
template <int NCH, int W, int NT = 64, class F>
__device__ __forceinline__ void for_chunks(int t, int cols, F&& f) {
  if constexpr (NCH > 0) {
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      const int c = t * W + ch * NT * W;
      if (c < cols) f(ch, c);
    }
  } else {
    int ch = 0;
    for (int c = t * W; c < cols; c += NT * W, ++ch) f(ch, c);
  }
}

// relu(x) for the two GELU forms below, as x - min(x, 0): exact (x - 0 or x - x), a NaN stays a NaN (v_min hands back the 0, NaN - 0 is
// NaN; v_max(x, 0) alone would drop it) and no finite x overflows ((x + |x|) / 2, the form until now, is inf from x = 2^127 on: the 128
// largest bf16 values). Two v_min_f32 and one v_pk_add_f32 a pair.
__device__ __forceinline__ f32x2_t relu2_keep_nan(f32x2_t x) { return x - f32x2_t{fminf(x[0], 0.f), fminf(x[1], 0.f)}; }
// Exact-form (erf) GELU, torch.nn.GELU()'s default, two values per VALU instruction: GELU(x) = relu(x) - a * Phi(-a) with
//   Phi(-a) = 2^q(a),  a = min(|x|, 5.5),  q = degree-7 fit of log2 Phi(-a) on [0, 5.5]      (x > 0: x (1 - Phi(-a)) = x - a Phi(-a))
// log2 Phi(-a) is smooth (it does not saturate as erf does), so 7 packed FMAs + one v_exp_f32 give |error| <= 7e-7 absolute and
// 1.2e-5 relative for |x| <= 5.5 (the fit is good to 4.3e-6 of Phi(-a); q's seven f32 roundings at |q| <= 26 add at most 3.4e-6).
// Phi of the negative tail is the quantity that is computed and it is multiplied by a, never added to 0.5: the tail keeps that relative
// accuracy down to x = -5.5. (Until this form, phi = 0.5 + copysign(0.5 - 2^q, x) rounded Phi(-a) to multiples of 2^-25: 4 % off at
// x = -5, and x * 2^-25 below -5.5 - unbounded in |x|.) Below -5.5 the result is the constant -5.5 Phi(-5.5) = -1.04e-7 where the
// function has decayed to 0 (|GELU(x)| < 1.04e-7 there); above 5.5 it is x - 1.04e-7 rounded to f32, which is x itself (half an ulp is 2.4e-7 there).
// This is the form for f32 results; values that are rounded to bf16 right after take gelu_erf2_b below.
__device__ __forceinline__ f32x2_t gelu_erf2(f32x2_t x) {
  const f32x2_t a = {fminf(fabsf(x[0]), 5.5f), fminf(fabsf(x[1]), 5.5f)};
  f32x2_t q = {-1.921234625e-06f, -1.921234625e-06f};
  q = __builtin_elementwise_fma(q, a, f32x2_t{6.328849712e-05f, 6.328849712e-05f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-9.434208502e-04f, -9.434208502e-04f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{8.556272268e-03f, 8.556272268e-03f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-5.405228293e-02f, -5.405228293e-02f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-4.583817849e-01f, -4.583817849e-01f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-1.151278331e+00f, -1.151278331e+00f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-9.999938561e-01f, -9.999938561e-01f});
  const f32x2_t e = {__builtin_amdgcn_exp2f(q[0]), __builtin_amdgcn_exp2f(q[1])};
  return __builtin_elementwise_fma(-a, e, relu2_keep_nan(x));
}
// The same function for values that are ROUNDED TO BF16 right after (GEMM epilogues with a bf16 output, gelu_fwd): GELU(x) = relu(x) - a * Phi(-a) with
//   Phi(-a) = 2^q(a),  a = min(|x|, 5.5),  q = degree-5 fit of log2 Phi(-a) on [0, 5.5]      (x > 0: x (1 - Phi(-a)) = x - a Phi(-a))
// log2 Phi(-a) is smooth (it does not saturate as erf does), so 5 FMAs + one v_exp_f32 give |q error| <= 3.7e-4: GELU within 2.51e-4
// relative on |x| < 5.5 (Phi of the negative tail is the quantity computed directly, so it keeps its relative accuracy) = 0.064 ulp of
// the bf16 the result is rounded to right after; 3.4e-5 absolute. Below -5.5 the result is the constant -5.5 Phi(-5.5) = -1.04e-7
// (|GELU(x)| is smaller than that there: an absolute error of at most 1.04e-7, where torch returns -0).
// No v_rcp, no log2(e) multiply, none of libm erff's range checks: on the VGGT fc1 GEMM (25 M outputs per launch, one workgroup per
// CU: nothing overlaps the epilogue) the activation is what the tile's tail costs, and the VALU's ISSUE slots are what it costs in
// (packed f32 and v_exp_f32 take two each): 12 slots per value here (11 before relu stopped overflowing) against 13 for the degree-7 form and ~30 for the
// Abramowitz-Stegun 7.1.26 form (v_rcp + v_exp + 12 scalar-lane ops).
__device__ __forceinline__ f32x2_t gelu_erf2_b(f32x2_t x) {
#pragma clang fp contract(off)      // a * 2^q rounds on its own, as it did when the last step was fma(x + |x|, 0.5, -t): the same bits
  const f32x2_t a = {fminf(fabsf(x[0]), 5.5f), fminf(fabsf(x[1]), 5.5f)};
  f32x2_t q = {-2.3323995992541313e-04f, -2.3323995992541313e-04f};
  q = __builtin_elementwise_fma(q, a, f32x2_t{4.869441967457533e-03f, 4.869441967457533e-03f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-4.4596340507268906e-02f, -4.4596340507268906e-02f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-4.6968939900398254e-01f, -4.6968939900398254e-01f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-1.1462510824203491e+00f, -1.1462510824203491e+00f});
  q = __builtin_elementwise_fma(q, a, f32x2_t{-1.0003620386123657e+00f, -1.0003620386123657e+00f});
  const f32x2_t t = {a[0] * __builtin_amdgcn_exp2f(q[0]), a[1] * __builtin_amdgcn_exp2f(q[1])};
  return relu2_keep_nan(x) - t;
}
__device__ __forceinline__ float gelu_erf(float x) { return gelu_erf2(f32x2_t{x, x})[0]; }
__device__ __forceinline__ float gelu_erf_b(float x) { return gelu_erf2_b(f32x2_t{x, x})[0]; }
// sigmoid through v_rcp_f32 (1 ulp) instead of the correctly rounded f32 division hipcc emits for `1.f / y` (v_div_scale x 2, v_rcp,
// four FMAs, v_div_fmas, v_div_fixup: ~10 VALU issue slots per value in epilogues whose results are rounded to bf16 right after - the
// SwiGLU forward / backward tails of the two widest text GEMMs). Every SiLU / sigmoid of the library goes through these two, so fused and
// unfused forms of an op stay bit-identical to each other.
__device__ __forceinline__ float sigmoid_f(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float silu_f(float x) { return x * sigmoid_f(x); }
// d(silu(g) * u) / dg * d = d * u * sigma * (1 + g * (1 - sigma)), sg = sigmoid_f(g). The bounded factor (|sigma (1 + g (1 - sigma))| <= 1.1)
// is multiplied in first: d * u formed first overflows to inf for huge d and u, and inf times a sigmoid that v_rcp_f32 flushed to 0
// (g < -87) is NaN where the true gradient is 0. (u * factor can itself overflow only for |u| within 10 % of the f32 maximum.)
// Shared by the stand-alone kernel and the GEMM epilogue so the two stay bit-identical.
__device__ __forceinline__ float swiglu_dgate_f(float d, float u, float g, float sg) { return d * (u * (sg * (1.f + g * (1.f - sg)))); }

// Counter-based dropout decision (vq3_dropout, the fused Perceiver cross-attention): 24 uniform bits from (seed, element index);
// an element is kept when they are >= (unsigned)(p * 2^24). Stateless, so a re-run with the same (seed, offset) repeats the mask.
__device__ __forceinline__ unsigned drop_bits(unsigned long long seed, unsigned long long idx) {
  unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (unsigned)((z ^ (z >> 31)) >> 40);      // 24 uniform bits
}

// ---- host side error plumbing (C ABI returns int, message kept per thread) ----
#ifdef __cplusplus
extern "C" const char* vq3_last_error(void);
#endif
void vq3_set_error(const char* fmt, ...);

#define VQ3_CHECK_ARG(cond, ...)            \
  do {                                      \
    if (!(cond)) {                          \
      vq3_set_error(__VA_ARGS__);           \
      return 1;                             \
    }                                       \
  } while (0)

// Host: the launch for a row of `need` chunks. f(std::integral_constant<int, NCH>) is called with the first NCH of the list that holds
// the row (a 0 in the list is the any-width kernel); the entry's own argument check is what makes the last one fit.
template <int NCH, int... More, class F>
void for_nch(int need, F&& f) {
  if constexpr (sizeof...(More) > 0) {
    if (NCH != 0 && need > NCH) return for_nch<More...>(need, f);
  }
  f(std::integral_constant<int, NCH>{});
}

#define VQ3_CHECK_LAUNCH(name)                                                    \
  do {                                                                            \
    hipError_t e__ = hipGetLastError();                                           \
    if (e__ != hipSuccess) {                                                      \
      vq3_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));       \
      return 2;                                                                   \
    }                                                                             \
  } while (0)
