// bf16 GEMM entry points of the C ABI:  C[M,N] = epilogue(alpha * A[M,K] . B[N,K]^T)
//
// The six extern "C" GEMM calls all go through gemm_dispatch: validate the descriptor, fill GemmParams, attach the fused epilogue
// (ViT q|k|v / SwiGLU backward / SwiGLU forward / LayerNorm fold), choose a kernel configuration (gemm_config.h: forced, table /
// measurement - gemm_tune.hip - or the fill heuristics below) and launch it through launch_config, the one id -> launcher map.
// The kernels themselves live in gemm2.hip / gemm3.hip / gemm6.hip / gemm7.hip.
#include <cstdlib>
#include <vector>

#include "gemm_config.h"
#include "vq3_hip.h"

using namespace vq3gemm;

namespace {

constexpr int BK = 64;

// Kernel choice per shape, from measurements on MI355X (tools/bench_gemm.py, tools/bench_gemm_layouts.py,
// tools/diag/run_stamps.py). Candidates:
//   cfg 7  : 128x128 tile, 8 waves, 2 stages, two workgroups per CU (512 tile slots)  - best for short K (<= 1536)
//   cfg 13 : 128x128 tile, 8 compute + 2 DMA-loader waves, 4-stage ring, one workgroup per CU (256 slots)
//   cfg 11 : 256x128 tile, 8 compute + 2 DMA-loader waves, 3-stage ring, one workgroup per CU (256 slots)
// score = (measured relative speed of the schedule) x (fraction of tile slots busy over all rounds).
double fill(long tiles, long slots) { return (double)tiles / (double)(((tiles + slots - 1) / slots) * slots); }

int g_forced_cfg = CFG_FROM_ENV;   // CFG_FROM_ENV / CFG_AUTO / a forced NT configuration
int g_forced_any = 0;              // vq3_gemm_force_config(102 .. 107): pins the configuration of the any-layout path (0 = none)

int choose_config(int M, int N, int K, int nbatch) {
  if (g_forced_cfg != CFG_AUTO) return g_forced_cfg;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * nbatch;
  const long t256 = (long)((M + 255) / 256) * ((N + 127) / 128) * nbatch;
  const bool shortk = K <= 1536;
  const double s7 = (shortk ? 1.00 : 0.93) * fill(t128, 512);
  const double s12 = (shortk ? 0.85 : 0.95) * fill(t128, 256);
  const double s11 = (shortk ? 0.90 : 1.00) * fill(t256, 256) * ((double)M / (double)(((M + 255) / 256) * 256)) /
                     ((double)M / (double)(((M + 127) / 128) * 128));
  // (the measured choice usually lands on the 256 x 256 8-phase kernel once its tile grid fills most of a round: this is what a launch
  // gets when nothing may be measured - under graph capture, or in a multi-rank job without a table entry)
  if ((long)((M + 255) / 256) * ((N + 255) / 256) * nbatch >= 192 && K >= 256) return CFG_V6_256x256;
  if (s11 >= s12 && s11 >= s7) return CFG_V2_256x128;
  return s12 >= s7 ? CFG_V2_RING4 : CFG_V2_2STAGE;
}

// any layout (k-major operands / K tails), 128x128 tiles: 3-stage ring + loader waves vs 2 stages x 2 workgroups.
int choose_any_config(int M, int N, int K, int nbatch) {
  if (g_forced_any) return g_forced_any;
  static int forced = -1;
  if (forced < 0) {
    const char* e = getenv("VQ3_GEMM_V3_STAGES");   // benchmarking override: 2, 3 or 5 (256x128 tile)
    forced = e ? atoi(e) : 0;
  }
  if (forced == 2 || forced == 3 || forced == 5) return CFG_V3_BASE + forced;
  const long t128 = (long)((M + 127) / 128) * ((N + 127) / 128) * nbatch;
  const bool shortk = K <= 1536;
  const double s2 = (shortk ? 1.00 : 0.93) * fill(t128, 512);
  const double s3 = (shortk ? 0.85 : 0.95) * fill(t128, 256);
  return s3 >= s2 ? CFG_V3_RING : CFG_V3_2STAGE;
}

// cfg 30: the 256 x 256 kernel on the row tiles that make WHOLE rounds of the chip, the remaining rows as a second small-tile launch.
// M = 49 392 (8 views x 6 x 1029 tokens), N = 1024 is 193 x 4 = 772 tiles = 3 rounds of 256 CUs + 4 tiles: the 4 cost a fourth round
// (fc2: 500 us where 3 rounds take 375). Rows 0 .. 192 * 256 - 1 are exactly 3 rounds; the last 240 rows are 16 tiles of 128 x 128.
int g_num_cu = 0;
int num_cus() {
  if (!g_num_cu) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
    (void)hipGetLastError();
    g_num_cu = n;
  }
  return g_num_cu;
}
// rows the 256 x 256 launch takes (0 = the split does not apply to this shape)
int split_rows_main(const GemmParams& p, int nbatch) {
  if (nbatch != 1 || p.epi == 2 || p.M < 512) return 0;
  const long nt = (p.N + 255) / 256, mt = (p.M + 255) / 256, cu = num_cus();
  const long rounds = mt * nt / cu, rem = mt * nt % cu;
  if (rounds < 1 || rem == 0 || rem * 2 > cu) return 0;         // a last round at least half full is left alone
  const long mt_main = rounds * cu / nt;
  const long tail = p.M - mt_main * 256;
  if (mt_main < 1 || tail <= 0 || tail > 2048) return 0;
  return (int)(mt_main * 256);
}
int launch_split_rows(GemmParams p, int nbatch, hipStream_t s) {
  const int m_main = split_rows_main(p, nbatch);
  if (!m_main) return launch_gemm_v6(p, 0, nbatch, s);
  GemmParams a = p, b = p;
  a.M = m_main;
  b.M = p.M - m_main;
  const size_t esz = p.out_f32 ? 4 : 2;
  b.A = p.A + (long)m_main * p.lda;
  b.C = (char*)p.C + (size_t)m_main * p.ldc * esz;
  if (p.R) b.R = (const char*)p.R + (size_t)m_main * p.ldr * esz;
  if (p.epi == 1) { b.C = p.C; b.vit.m_off = m_main; }      // Q / K / V are addressed by token index, C is a placeholder
  if (p.ln_in) b.ln_in = p.ln_in + (long)m_main * p.ln_parts * 2;
  if (p.st_out) b.st_out = p.st_out + (long)m_main * (p.N >> 7) * 2;
  // (tried: the row tail on a side stream forked from / joined to `s` by events so that it overlaps the main launch instead of following it -
  // no gain, fc1 +3 %: the dispatcher does not interleave the two grids; gpurun_out r3_diag9 epi_30 vs epi_30_serial. Second try: the tail
  // FIRST, on a HIGH-priority side stream, the main launch behind it on `s` - fc1 519 -> 507 us, q|k|v-shaped 338 -> 335, fc2 374 -> 379,
  // proj 156 -> 166: the two event hops cost what the overlap gives)
  int rc = launch_gemm_v6(a, 0, nbatch, s);
  if (rc) return rc;
  const long t128 = (long)((b.M + 127) / 128) * ((b.N + 127) / 128);
  return launch_gemm_v2(b, (p.K <= 1536 && t128 > num_cus()) ? CFG_V2_2STAGE : CFG_V2_RING4, nbatch, s);
}

// applies what VQ3_GEMM_CFG / vq3_gemm_force_config ask for
int force_config(int cfg) {
  if (cfg == CFG_AUTO) {
    g_forced_cfg = CFG_AUTO;
    g_forced_any = 0;
    return 0;
  }
  const GemmConfig* c = find_config(cfg);
  VQ3_CHECK_ARG(c != nullptr, "gemm_force_config: %d is not a GEMM kernel configuration (gemm_config.h)", cfg);
  (c->serves == SERVES_ANY ? g_forced_any : g_forced_cfg) = cfg;
  return 0;
}

// VQ3_GEMM_CFG, read once: before the first GEMM call or the first vq3_gemm_force_config, whichever comes first, so that a call of
// the hook always has the last word. An id the registry does not hold fails every GEMM call until the hook sets a valid one.
int read_env_config() {
  if (g_forced_cfg != CFG_FROM_ENV) return 0;
  const char* e = getenv("VQ3_GEMM_CFG");
  g_forced_cfg = CFG_AUTO;
  const int rc = e ? force_config(atoi(e)) : 0;
  if (rc) g_forced_cfg = CFG_FROM_ENV;
  return rc;
}

// launches cfg; where its launcher answers -1 the registry's fallback runs instead
int run_config(GemmParams& p, int cfg, int transA, int transB, int nbatch, hipStream_t s) {
  for (;;) {
    const GemmConfig* c = find_config(cfg);
    VQ3_CHECK_ARG(c != nullptr, "gemm: %d is not a GEMM kernel configuration (gemm_config.h)", cfg);
    const int rc = launch_config(p, cfg, transA, transB, nbatch, s);
    if (rc > 0) return rc;
    if (rc == 0) {
      VQ3_CHECK_LAUNCH(c->name);
      return 0;
    }
    const int next = p.epi == 3 ? c->fallback_swiglu_fwd : c->fallback;
    VQ3_CHECK_ARG(next != 0, "gemm: configuration %d (%s) declined this call and has no fallback", cfg, c->name);
    cfg = next;
  }
}

// ---- the steps of gemm_dispatch ----------------------------------------------------------------------------------------
// own_output: a fused epilogue that stores through pointers of its own, not C; own_ld: ... that does not read ldc as C's row stride
int validate_desc(const vq3_gemm_desc* d, bool own_output, bool own_ld) {
  VQ3_CHECK_ARG(d != nullptr, "gemm: null descriptor");
  VQ3_CHECK_ARG(d->A && d->B && (d->C || own_output), "gemm: null operand pointer");
  VQ3_CHECK_ARG(d->M > 0 && d->N > 0 && d->K > 0, "gemm: bad shape M=%d N=%d K=%d", d->M, d->N, d->K);
  VQ3_CHECK_ARG(d->K % 8 == 0 && d->K >= 8, "gemm: K=%d must be a positive multiple of 8", d->K);
  VQ3_CHECK_ARG(d->lda % 8 == 0 && d->ldb % 8 == 0, "gemm: lda=%d / ldb=%d must be multiples of 8", d->lda, d->ldb);
  VQ3_CHECK_ARG(d->lda >= (d->transA ? d->M : d->K) && d->ldb >= (d->transB ? d->N : d->K),
                "gemm: leading dims smaller than the operand's inner extent");
  VQ3_CHECK_ARG(!d->transA || (d->M % 8 == 0), "gemm: a k-major A needs M %% 8 == 0 (M=%d)", d->M);
  VQ3_CHECK_ARG(!d->transB || (d->N % 8 == 0), "gemm: a k-major B needs N %% 8 == 0 (N=%d)", d->N);
  VQ3_CHECK_ARG(((uintptr_t)d->A % 16 == 0) && ((uintptr_t)d->B % 16 == 0), "gemm: A/B must be 16-byte aligned");
  VQ3_CHECK_ARG(d->sA1 % 8 == 0 && d->sA2 % 8 == 0 && d->sB1 % 8 == 0 && d->sB2 % 8 == 0,
                "gemm: batch strides of A/B must be multiples of 8 elements");
  VQ3_CHECK_ARG(own_ld || d->ldc >= d->N, "gemm: ldc=%d < N=%d", d->ldc, d->N);
  VQ3_CHECK_ARG(d->nb1 >= 1 && d->nb2 >= 1 && d->b2divB >= 1, "gemm: bad batch dims");
  VQ3_CHECK_ARG((long)d->nb1 * d->nb2 <= 65535, "gemm: too many batches");
  VQ3_CHECK_ARG(d->act >= 0 && d->act <= 2, "gemm: bad activation %d", d->act);
  VQ3_CHECK_ARG(!(d->R) || d->ldr >= d->N, "gemm: ldr < N");
  VQ3_CHECK_ARG((!d->bias || (uintptr_t)d->bias % 16 == 0) && (!d->colscale || (uintptr_t)d->colscale % 16 == 0),
                "gemm: bias / colscale must be 16-byte aligned");
  return 0;
}

void fill_params(GemmParams& p, const vq3_gemm_desc* d) {
  p.A = (const bf16_t*)d->A; p.B = (const bf16_t*)d->B; p.C = d->C;
  p.bias = (const float*)d->bias; p.colscale = (const float*)d->colscale; p.R = d->R;
  p.M = d->M; p.N = d->N; p.K = d->K; p.lda = d->lda; p.ldb = d->ldb; p.ldc = d->ldc; p.ldr = d->ldr;
  p.sA1 = d->sA1; p.sA2 = d->sA2; p.sB1 = d->sB1; p.sB2 = d->sB2;
  p.sC1 = d->sC1; p.sC2 = d->sC2; p.sR1 = d->sR1; p.sR2 = d->sR2;
  p.nb2 = d->nb2; p.b2divB = d->b2divB;
  p.act = d->act; p.out_f32 = d->out_f32; p.accumulate = d->accumulate; p.alpha = d->alpha;
  p.kper = d->K; p.nsplit = 1;
  p.epi = 0;
  p.stamps = nullptr;
  p.nbw = 1;
  p.stagger = 0;
  p.sk_full = p.sk_rem = p.sk_s = 0; p.sk_ws = nullptr; p.sk_cnt = nullptr; p.sk_err = nullptr; p.sk_spin = 1u << 23; p.f8_rs = p.f8_cs = nullptr;
  p.sw_gu = nullptr; p.sw_dgu = nullptr;
  p.ln_in = nullptr; p.ln_c = nullptr; p.ln_parts = 0; p.ln_eps = 0.f; p.st_out = nullptr;
}

int attach_vit_qkv(GemmParams& p, const vq3_gemm_desc* d, const vq3_vit_qkv_epilogue* ve) {
  VQ3_CHECK_ARG(ve->Q && ve->K && ve->V, "gemm_vit_qkv: null output pointer");
  VQ3_CHECK_ARG(!d->transA && !d->transB && d->K % BK == 0 && !d->out_f32 && !d->accumulate && !d->R && !d->colscale && d->act == 0 &&
                    d->ksplit <= 1 && d->nb1 == 1 && d->nb2 == 1,
                "gemm_vit_qkv: plain NT bf16 GEMM with K %% 64 == 0 and at most a bias");
  VQ3_CHECK_ARG(ve->NH > 0 && d->N == 3 * ve->NH * 64 && ve->N > 0 && d->M % ve->N == 0, "gemm_vit_qkv: N must be 3*NH*64 and M a multiple of the group length");
  VQ3_CHECK_ARG(!ve->use_norm || (ve->qn_w && ve->qn_b && ve->kn_w && ve->kn_b), "gemm_vit_qkv: norm weights missing");
  VQ3_CHECK_ARG(!ve->use_rope || (ve->cos && ve->sin && ve->tokens_per_frame > 0 && ve->Wp > 0), "gemm_vit_qkv: rope tables missing");
  VQ3_CHECK_ARG(((uintptr_t)ve->Q | (uintptr_t)ve->K | (uintptr_t)ve->V | (uintptr_t)ve->cos | (uintptr_t)ve->sin) % 16 == 0,
                "gemm_vit_qkv: Q/K/V and the rope tables must be 16-byte aligned");
  p.epi = 1;
  p.vit.Q = (bf16_t*)ve->Q; p.vit.K = (bf16_t*)ve->K; p.vit.V = (bf16_t*)ve->V;
  p.vit.qn_w = ve->qn_w; p.vit.qn_b = ve->qn_b; p.vit.kn_w = ve->kn_w; p.vit.kn_b = ve->kn_b;
  p.vit.cos = (const bf16_t*)ve->cos; p.vit.sin = (const bf16_t*)ve->sin;
  p.vit.N = ve->N; p.vit.NH = ve->NH; p.vit.P = ve->tokens_per_frame; p.vit.patch_start = ve->patch_start; p.vit.Wp = ve->Wp;
  {   // the largest table row the epilogue asks for is max(patch rows, patch columns) (positions are 1-based; 0 = special tokens)
    const int P_ = ve->tokens_per_frame > 0 ? ve->tokens_per_frame : ve->N, np = P_ - ve->patch_start;
    const int hp = ve->Wp > 0 && np > 0 ? (np + ve->Wp - 1) / ve->Wp : 0;
    p.vit.rope_rows = (hp > ve->Wp ? hp : ve->Wp) + 1;
  }
  p.vit.use_norm = ve->use_norm; p.vit.use_rope = ve->use_rope; p.vit.eps = ve->eps;
  p.vit.m_off = 0;
  p.C = ve->Q; p.ldc = d->N;          // placeholders: the staged epilogue checks their alignment, nothing is stored through them
  p.sC1 = p.sC2 = 0;
  return 0;
}

int attach_swiglu_bwd(GemmParams& p, const vq3_gemm_desc* d, const void* sw_gu, void* sw_dgu) {
  VQ3_CHECK_ARG(sw_gu != nullptr, "gemm_swiglu_bwd: null gate|up pointer");
  VQ3_CHECK_ARG(!d->out_f32 && !d->accumulate && !d->R && !d->colscale && !d->bias && d->act == 0 && d->ksplit <= 1 && d->nb1 == 1 &&
                    d->nb2 == 1 && d->N % 8 == 0 && d->alpha == 1.f,
                "gemm_swiglu_bwd: plain bf16 GEMM (no epilogue, no batch), N %% 8 == 0");
  VQ3_CHECK_ARG(((uintptr_t)sw_gu | (uintptr_t)sw_dgu) % 16 == 0, "gemm_swiglu_bwd: gu / dgu must be 16-byte aligned");
  p.epi = 2;
  p.sw_gu = (const bf16_t*)sw_gu; p.sw_dgu = (bf16_t*)sw_dgu;
  p.C = sw_dgu; p.ldc = d->N;         // placeholders (alignment checks only)
  p.sC1 = p.sC2 = 0;
  return 0;
}

char kSwigluNoGu;      // vq3_gemm_swiglu_fwd without a gate|up output (a forward that no backward follows): "mode on, pointer null"
int attach_swiglu_fwd(GemmParams& p, const vq3_gemm_desc* d, void* sw_fwd_gu, bool other_epilogue) {
  VQ3_CHECK_ARG(!other_epilogue, "gemm_swiglu_fwd: no other fused epilogue");
  VQ3_CHECK_ARG(!d->transA && !d->transB && d->K % BK == 0 && !d->out_f32 && !d->accumulate && !d->R && !d->colscale && !d->bias &&
                    d->act == 0 && d->ksplit <= 1 && d->nb1 == 1 && d->nb2 == 1 && d->alpha == 1.f,
                "gemm_swiglu_fwd: plain NT bf16 GEMM (no epilogue, no batch), K %% 64 == 0");
  VQ3_CHECK_ARG(d->N % 256 == 0 && d->ldc >= d->N / 2 && d->ldc % 8 == 0, "gemm_swiglu_fwd: N = 2 I with I %% 128 == 0, act rows of >= I elements (ld %% 8)");
  if (sw_fwd_gu == (void*)&kSwigluNoGu) sw_fwd_gu = nullptr;
  VQ3_CHECK_ARG(((uintptr_t)sw_fwd_gu | (uintptr_t)d->C) % 16 == 0, "gemm_swiglu_fwd: gate|up / act must be 16-byte aligned");
  p.epi = 3;
  p.sw_dgu = (bf16_t*)sw_fwd_gu;                 // null: the epilogue stores act only
  p.sC1 = p.sC2 = 0;
  return 0;
}

int attach_ln_fold(GemmParams& p, const vq3_gemm_desc* d, const vq3_gemm_ln_fold* ln, bool vit, bool swiglu_bwd) {
  // both halves live in the LDS-staged epilogue: the conditions of gemm_common.h: staged_ok must hold, or the kernels would
  // silently take the register epilogue
  VQ3_CHECK_ARG(!swiglu_bwd && !d->out_f32 && d->ksplit <= 1 && d->nb1 * d->nb2 == 1 && p.vec_ok && p.ldc % 8 == 0 && ((uintptr_t)p.C % 16 == 0) &&
                    (!d->R || (d->ldr % 8 == 0 && (uintptr_t)d->R % 16 == 0)),
                "gemm ln fold: needs the staged bf16 epilogue (bf16 C, one batch, 16-byte aligned rows)");
  if (ln->stats_in) {
    VQ3_CHECK_ARG(ln->colsum && ln->parts_in > 0 && ln->parts_in <= 64 && ((uintptr_t)ln->stats_in % 8 == 0) && ((uintptr_t)ln->colsum % 16 == 0),
                  "gemm ln fold: stats_in needs colsum [N] (16-byte aligned) and 1..64 (sum, sumsq) pairs per row");
    p.ln_in = ln->stats_in; p.ln_c = ln->colsum; p.ln_parts = ln->parts_in; p.ln_eps = ln->eps;
  }
  if (ln->stats_out) {
    VQ3_CHECK_ARG(!vit && d->N % 128 == 0 && ((uintptr_t)ln->stats_out % 8 == 0), "gemm ln fold: stats_out needs N %% 128 == 0 and a plain C epilogue");
    p.st_out = ln->stats_out;
  }
  return 0;
}

}  // namespace

int vq3gemm::launch_config(GemmParams& p, int cfg, int transA, int transB, int nbatch, hipStream_t s) {
  switch (cfg) {
    case CFG_V2_2STAGE: case CFG_V2_RING3_LOAD4: case CFG_V2_256x128: case CFG_V2_RING4:
    case CFG_V2_224x128: case CFG_V2_192x128: case CFG_V2_192x128_2WG:
      return launch_gemm_v2(p, cfg, nbatch, s);
    case CFG_V6_256x256: case CFG_V6_256x128: case CFG_V6_128x256:
      return launch_gemm_v6(p, cfg - CFG_V6_256x256, nbatch, s);
    case CFG_V7: return launch_gemm_v7(p, nbatch, s);
    case CFG_V6_SPLIT_LAST: return launch_gemm_v6(p, 3, nbatch, s);
    case CFG_SPLIT_ROWS: return launch_split_rows(p, nbatch, s);
    case CFG_V3_2STAGE: case CFG_V3_RING: case CFG_V3_256x128:
      return launch_gemm_v3(p, transA, transB, cfg - CFG_V3_BASE, nbatch, s);
    case CFG_V6_KM: case CFG_V6_KM_SPLIT:
      return (transA && transB) ? launch_gemm_v6_km(p, nbatch, s, cfg == CFG_V6_KM_SPLIT) : -1;
  }
  return -1;
}

static int gemm_dispatch(const vq3_gemm_desc* d, const vq3_vit_qkv_epilogue* ve, void* stream, const void* sw_gu = nullptr,
                         void* sw_dgu = nullptr, const vq3_gemm_ln_fold* ln = nullptr, void* sw_fwd_gu = nullptr) {
  if (int rc = read_env_config()) return rc;       // (first: a bad VQ3_GEMM_CFG is reported before anything about this call)
  if (int rc = validate_desc(d, ve || sw_dgu, ve || sw_dgu || sw_fwd_gu)) return rc;
  GemmParams p;
  fill_params(p, d);
  if (ve)
    if (int rc = attach_vit_qkv(p, d, ve)) return rc;
  if (sw_dgu)
    if (int rc = attach_swiglu_bwd(p, d, sw_gu, sw_dgu)) return rc;
  if (sw_fwd_gu)
    if (int rc = attach_swiglu_fwd(p, d, sw_fwd_gu, ve || sw_dgu || ln)) return rc;
  p.vec_ok = host_vec_ok(p) ? 1 : 0;

  hipStream_t s = (hipStream_t)stream;
  const int nbatch = d->nb1 * d->nb2;
  if (ln && (ln->stats_in || ln->stats_out))
    if (int rc = attach_ln_fold(p, d, ln, ve != nullptr, sw_dgu != nullptr)) return rc;
  if (d->ksplit > 1) {
    VQ3_CHECK_ARG(d->out_f32 && !d->bias && !d->colscale && !d->R && d->act == 0 && !d->accumulate,
                  "gemm: split-K needs a zero-initialised f32 C and no epilogue");
    int kper = ((d->K + d->ksplit - 1) / d->ksplit + 63) / 64 * 64;
    p.kper = kper;
    p.nsplit = (d->K + kper - 1) / kper;
    VQ3_CHECK_ARG(p.nsplit <= 65535, "gemm: too many K slices");
    const int rc = launch_gemm_v3(p, d->transA, d->transB, 2, nbatch, s);
    if (rc) return rc;
    VQ3_CHECK_LAUNCH("gemm_bf16_nt(v3 split-K)");
    return 0;
  }
  const bool measure = (long)d->M * d->N * d->K >= (1L << 24);       // smaller products are not worth a measurement
  if (d->transA || d->transB || d->K % BK != 0) {
    int cfg = choose_any_config(d->M, d->N, d->K, nbatch);
    if (!g_forced_any && getenv("VQ3_GEMM_V3_STAGES") == nullptr && measure) {
      std::vector<int> cands = {CFG_V3_2STAGE, CFG_V3_RING, CFG_V3_256x128};
      if (d->transA && d->transB && (long)((d->M + 255) / 256) * ((d->N + 255) / 256) >= 64) cands.push_back(CFG_V6_KM);
      cfg = tuned_choice(p, d->transA, d->transB, nbatch, s, cands, cfg, true);
    }
    return run_config(p, cfg, d->transA, d->transB, nbatch, s);
  }
  if (p.epi == 3) {
    // the 8-phase kernels only (the epilogue needs gate and up of a feature in ONE tile: gemm6.hip stages the two weight row ranges)
    int cfg = CFG_V6_256x256;
    if (g_forced_cfg == CFG_AUTO) {
      if (measure) cfg = tuned_choice(p, 0, 0, nbatch, s, {CFG_V6_256x256, CFG_V6_256x128, CFG_V6_128x256}, cfg);
    } else if (find_config(g_forced_cfg)->serves & SERVES_SWIGLU_FWD) {
      cfg = g_forced_cfg;
    }
    return run_config(p, cfg, 0, 0, nbatch, s);
  }
  int cfg = choose_config(d->M, d->N, d->K, nbatch);
  if (g_forced_cfg == CFG_AUTO && measure) {
    // candidates: 2-stage x 2 workgroups (7), 256x128 / 128x128 loader rings (11, 13), 8-wave 128x128 ring (9), and the
    // 256x256 8-phase kernel (20) once the tile grid can feed it
    std::vector<int> cands = {CFG_V2_2STAGE, CFG_V2_256x128, CFG_V2_RING4, CFG_V2_RING3_LOAD4};
    if ((long)((d->M + 255) / 256) * ((d->N + 255) / 256) * nbatch >= 64) cands.push_back(CFG_V6_256x256);
    if ((long)((d->M + 255) / 256) * ((d->N + 127) / 128) * nbatch >= 64) cands.push_back(CFG_V6_256x128);
    if ((long)((d->M + 127) / 128) * ((d->N + 255) / 256) * nbatch >= 64) cands.push_back(CFG_V6_128x256);
    if (split_rows_main(p, nbatch)) cands.push_back(CFG_SPLIT_ROWS);
    cands.push_back(CFG_V6_SPLIT_LAST);          // (skipped by the tuner where the last-round split does not apply: the launcher returns -1)
    if ((long)((d->M + 255) / 256) * ((d->N + 127) / 128) * nbatch >= 256) cands.push_back(CFG_V7);     // two workgroups per CU (gemm7.hip)
    cfg = tuned_choice(p, 0, 0, nbatch, s, cands, cfg);
  }
  return run_config(p, cfg, 0, 0, nbatch, s);
}

extern "C" int vq3_gemm_bf16_nt(const vq3_gemm_desc* d, void* stream) { return gemm_dispatch(d, nullptr, stream); }

extern "C" int vq3_gemm_vit_qkv(const vq3_gemm_desc* d, const vq3_vit_qkv_epilogue* epi, void* stream) {
  VQ3_CHECK_ARG(epi != nullptr, "gemm_vit_qkv: null epilogue descriptor");
  return gemm_dispatch(d, epi, stream);
}

extern "C" int vq3_gemm_bf16_nt_ln(const vq3_gemm_desc* d, const vq3_gemm_ln_fold* ln, void* stream) {
  return gemm_dispatch(d, nullptr, stream, nullptr, nullptr, ln);
}

extern "C" int vq3_gemm_vit_qkv_ln(const vq3_gemm_desc* d, const vq3_vit_qkv_epilogue* epi, const vq3_gemm_ln_fold* ln, void* stream) {
  VQ3_CHECK_ARG(epi != nullptr, "gemm_vit_qkv_ln: null epilogue descriptor");
  return gemm_dispatch(d, epi, stream, nullptr, nullptr, ln);
}

extern "C" int vq3_gemm_swiglu_bwd(const vq3_gemm_desc* d, const void* gu, void* dgu, void* stream) {
  VQ3_CHECK_ARG(dgu != nullptr, "gemm_swiglu_bwd: null output pointer");
  return gemm_dispatch(d, nullptr, stream, gu, dgu);
}

extern "C" int vq3_gemm_swiglu_fwd(const vq3_gemm_desc* d, void* gu, void* stream) {
  VQ3_CHECK_ARG(d != nullptr && d->C != nullptr, "gemm_swiglu_fwd: null output pointer");
  return gemm_dispatch(d, nullptr, stream, nullptr, nullptr, nullptr, gu ? gu : (void*)&kSwigluNoGu);     // gu == NULL: act only
}

extern "C" int vq3_gemm_tile_order(int32_t M, int32_t N, int32_t bm, int32_t bn, int32_t wg_per_cu, int32_t* xm_out, int32_t* band_out,
                                   int32_t* order) {
  VQ3_CHECK_ARG(M > 0 && N > 0 && bm > 0 && bn > 0 && wg_per_cu >= 1, "gemm_tile_order: bad arguments");
  GemmParams p{};
  p.M = M; p.N = N;
  p.mtiles = (M + bm - 1) / bm;
  p.ntiles = (N + bn - 1) / bn;
  VQ3_CHECK_ARG((long)p.mtiles * p.ntiles < (1L << 28), "gemm_tile_order: too many tiles");
  choose_tile_order(p, bm, bn, wg_per_cu);
  if (xm_out) *xm_out = p.xm;
  if (band_out) *band_out = p.nbw;
  if (order) {
    const int n = p.mtiles * p.ntiles;
    for (int i = 0; i < n; ++i) {
      int m0 = 0, n0 = 0;
      tile_coords_id(p, i, bm, bn, m0, n0);
      order[2 * i] = m0 / bm;
      order[2 * i + 1] = n0 / bn;
    }
  }
  return 0;
}

extern "C" int vq3_gemm_split_plan(int32_t M, int32_t N, int32_t K, int32_t ncu, int32_t* full_out, int32_t* rem_out, int32_t* slices_out) {
  VQ3_CHECK_ARG(M > 0 && N > 0 && K > 0 && K % 64 == 0 && ncu >= 8 && slices_out, "gemm_split_plan: bad arguments");
  GemmParams p{};
  p.M = M; p.N = N; p.K = K;
  int full = 0, rem = 0;
  const int sl = gemm_split_plan(p, 1, ncu, &full, &rem);
  *slices_out = sl >= 2 ? sl : 0;
  if (full_out) *full_out = sl >= 2 ? full : 0;
  if (rem_out) *rem_out = sl >= 2 ? rem : 0;
  return 0;
}

extern "C" int vq3_gemm_split_status(void* stream, int32_t* gave_up) {
  VQ3_CHECK_ARG(gave_up != nullptr, "gemm_split_status: null output");
  const int r = gemm_split_gave_up((hipStream_t)stream);
  VQ3_CHECK_ARG(r != -2, "gemm_split_status: could not synchronise the stream");
  *gave_up = r > 0 ? 1 : 0;
  return 0;
}

extern "C" int vq3_gemm_split_debug_spin_bound(int64_t polls) {
  VQ3_CHECK_ARG(polls >= 0 && polls <= (1ll << 31), "gemm_split_debug_spin_bound: polls out of range");
  gemm_split_set_spin_bound(polls ? (unsigned)polls : (1u << 23));
  return 0;
}

extern "C" int vq3_gemm_split_poll(int32_t* gave_up, int32_t clear) {
  VQ3_CHECK_ARG(gave_up != nullptr, "gemm_split_poll: null output");
  *gave_up = gemm_split_poll(clear != 0) > 0 ? 1 : 0;
  return 0;
}

extern "C" int vq3_gemm_force_config(int32_t cfg) {
  (void)read_env_config();      // (the variable is applied first, then overridden: forcing before the first GEMM call holds)
  return force_config(cfg);
}
