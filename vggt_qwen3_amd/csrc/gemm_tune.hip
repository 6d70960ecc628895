// The measured kernel choice of the bf16 GEMM dispatcher (gemm.hip): the tune table and its file, the one-off timing of a call's
// candidate configurations, and the workspace / provider / hold state that the extern "C" setters below control.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

#include "gemm_config.h"
#include "vq3_hip.h"

namespace vq3gemm {
namespace {

// The dispatcher's heuristics rank tile configurations by fill; what a shape really gets also depends on K depth, epilogue and
// cache state, and the ranking is wrong often enough to matter (Perceiver ffn1: 130 us chosen, 94 us available). So the
// FIRST call with a new (shape, layout, epilogue kind) times every candidate on the caller's stream - on scratch output, with
// a 320 MB fill between launches so that the weights come from HBM as they do inside a training step - and the winner
// is remembered for the life of the process. Never while the stream is being captured into a graph (the heuristic answers
// then), never when VQ3_GEMM_AUTOTUNE=0 or a configuration is forced. The first call of a shape therefore synchronises
// the stream and may allocate scratch; every later call only enqueues.
typedef std::tuple<int, int, int, int, int> TuneKey;   // M, N, K, nbatch, flags
std::map<TuneKey, int> g_tuned;
std::mutex g_tune_mutex;
void* g_scratch_c = nullptr;
size_t g_scratch_c_bytes = 0;
void* g_flush = nullptr;
constexpr size_t FLUSH_BYTES = 320u << 20;
int g_autotune = -1;
// vq3_gemm_tune_workspace: trial output + cache-flush buffer come from memory the CALLER owns (a torch tensor) - no hipMalloc / hipFree
// from inside a GEMM call. A registered workspace that is too small for a shape means "do not measure this shape" (the table or the
// heuristic answers), never a silent allocation.
void* g_ws = nullptr;
size_t g_ws_bytes = 0;
int g_ws_dev = -1;                    // device the registered workspace lives on (-1: whatever the caller registered by hand)
// vq3_gemm_workspace_provider: the caller's allocator (a torch tensor factory) asked for device memory the moment a measurement - or a
// split-K launch's first use of a stream - actually needs it: an inference-only process or a multi-rank job (hold on) never pays for it
vq3_ws_provider_t g_provider = nullptr;
// vq3_gemm_autotune_hold: nothing is measured while it is on (multi-rank jobs: a measurement synchronises the device under in-flight
// collectives and every rank would rank near-ties on its own; the table and the heuristic are the same function on every rank)
int g_hold = 0;

bool autotune_on(hipStream_t s) {
  if (g_autotune < 0) {
    const char* e = getenv("VQ3_GEMM_AUTOTUNE");
    g_autotune = e ? atoi(e) : 1;
  }
  if (!g_autotune) return false;
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess || st != hipStreamCaptureStatusNone) return false;
  return true;
}

// returns the fastest candidate, or -1 when tuning could not run (allocation failure, ...)
int tune(const GemmParams& p0, const std::vector<int>& cands, int transA, int transB, int nbatch, hipStream_t s) {
  GemmParams p = p0;
  // tall products are measured on their first 65 536 rows (>= 4 rounds of 256 x 256 tiles for N >= 1024: the ranking no longer depends on
  // M there, and config C4's 395 136-row tower GEMMs would otherwise need 3.2 GB of trial output and 30 ms per trial launch)
  if (!transA && p.M > 65536 && p.epi != 2 && p.epi != 3) p.M = 65536;
  const size_t esz = p.out_f32 ? 4 : 2;
  const size_t need = ((size_t)p.M * p.N * esz * (size_t)nbatch + 256 + 255) & ~(size_t)255;
  void* scratch_c = nullptr;
  void* flush = nullptr;
  if (g_provider) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (!g_ws || g_ws_dev != dev || need + FLUSH_BYTES > g_ws_bytes) {
      // lazily, for THIS device, at least what this shape needs (the provider rounds up to its default size and keeps the tensor alive)
      void* w = g_provider((int64_t)(need + FLUSH_BYTES), dev, 0);
      if (!w) return -1;                                       // no memory to measure in: the table / heuristic answers
      g_ws = w; g_ws_bytes = need + FLUSH_BYTES; g_ws_dev = dev;
    }
  }
  if (g_ws) {
    if (need + FLUSH_BYTES > g_ws_bytes) return -1;           // the caller's workspace decides what may be measured
    scratch_c = g_ws;
    flush = (char*)g_ws + need;
  } else {
    // no workspace registered (a plain C caller): the library's own buffers, allocated on first use
    if (need > g_scratch_c_bytes) {
      if (g_scratch_c) (void)hipFree(g_scratch_c);
      g_scratch_c = nullptr; g_scratch_c_bytes = 0;
      if (hipMalloc(&g_scratch_c, need) != hipSuccess) { (void)hipGetLastError(); return -1; }
      g_scratch_c_bytes = need;
    }
    if (!g_flush && hipMalloc(&g_flush, FLUSH_BYTES) != hipSuccess) { (void)hipGetLastError(); g_flush = nullptr; return -1; }
    scratch_c = g_scratch_c;
    flush = g_flush;
  }
  // trial output: dense scratch, no read-modify-write operands (an in-place residual or accumulate target must not be touched)
  if (p.epi == 0) p.C = scratch_c;      // (epi == 1 writes Q / K / V, epi == 3 gate|up and act: idempotent, no read-modify-write)
  if (p.epi != 3) {
    p.ldc = p.N;
    p.sC1 = (long)p.M * p.N * p.nb2; p.sC2 = (long)p.M * p.N;
    p.vec_ok = (p.N % 4 == 0) ? 1 : 0;
  }
  p.R = nullptr; p.ldr = 0; p.accumulate = 0;
  p.sR1 = p.sR2 = 0;
  (void)hipDeviceSynchronize();   // measure alone: work queued on other streams (the wgrad stream) would skew the ranking
  (void)hipGetLastError();
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { (void)hipGetLastError(); return -1; }
  int best = -1;
  float best_ms = 1e30f;
  const int reps = 5;       // (the minimum of 5 cold launches: with 3 the ranking of near-ties flipped from box to box)
  for (int cand : cands) {
    GemmParams q = p;             // (every launch from the same parameters: a launcher fills in its own tile grid)
    if (launch_config(q, cand, transA, transB, nbatch, s) != 0) continue;      // warm-up (attribute set-up, code load); -1: not for this call
    float tmin = 1e30f;
    for (int r = 0; r < reps; ++r) {
      (void)hipMemsetAsync(flush, r, FLUSH_BYTES, s);
      (void)hipEventRecord(e0, s);
      q = p;
      if (launch_config(q, cand, transA, transB, nbatch, s) != 0) { tmin = 1e30f; break; }
      (void)hipEventRecord(e1, s);
      if (hipEventSynchronize(e1) != hipSuccess) { tmin = 1e30f; break; }
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, e0, e1);
      tmin = std::min(tmin, ms);
    }
    if (tmin < best_ms) { best_ms = tmin; best = cand; }
  }
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  if (hipGetLastError() != hipSuccess) return -1;
  if (getenv("VQ3_GEMM_AUTOTUNE_LOG"))
    fprintf(stderr, "[vq3 gemm autotune] M=%d N=%d K=%d batch=%d tA=%d tB=%d -> %d (%.1f us)\n", p.M, p.N, p.K, nbatch, transA, transB,
            best, best_ms * 1e3f);
  return best;
}

// VQ3_GEMM_TUNE_FILE=<path>: the table is read from that file before the first choice and every newly measured entry is appended to it
// ("M N K batch flags cfg" per line) - a second run, or the other ranks of a job pointed at the same file, then make the SAME choices
// (same kernels, same summation order) without measuring. Without it the choice is timing-based and may differ from run to run and
// from rank to rank (replicas still agree bit for bit: they apply the same all-reduced gradient); VQ3_GEMM_AUTOTUNE=0 turns measuring off.
bool g_tune_file_read = false;
int tune_table_read(const char* path) {
  FILE* f = fopen(path, "r");
  if (!f) return -1;
  int m, n, k, b, fl, cfg, cnt = 0;
  char line[256];
  while (fgets(line, sizeof line, f)) {
    if (line[0] == '#') continue;
    if (sscanf(line, "%d %d %d %d %d %d", &m, &n, &k, &b, &fl, &cfg) == 6) { g_tuned[TuneKey(m, n, k, b, fl)] = cfg; ++cnt; }
  }
  fclose(f);
  return cnt;
}
void tune_file_read() {
  g_tune_file_read = true;
  const char* path = getenv("VQ3_GEMM_TUNE_FILE");
  if (!path || !*path) return;
  (void)tune_table_read(path);
}
void tune_file_append(const TuneKey& key, int cfg) {
  const char* path = getenv("VQ3_GEMM_TUNE_FILE");
  if (!path || !*path) return;
  FILE* f = fopen(path, "a");
  if (!f) return;
  fprintf(f, "%d %d %d %d %d %d\n", std::get<0>(key), std::get<1>(key), std::get<2>(key), std::get<3>(key), std::get<4>(key), cfg);
  fclose(f);
}

}  // namespace

int tuned_choice(const GemmParams& p, int transA, int transB, int nbatch, hipStream_t s, const std::vector<int>& cands, int fallback,
                 bool any_layout) {
  // (the key carries what selects a code path inside the candidates: layout, epilogue kind, and whether the 4-wide / whole-row stores apply)
  const bool rows16 = (p.ldc % 8 == 0) && ((reinterpret_cast<uintptr_t>(p.C) & 15) == 0) &&
                      (!p.R || ((p.ldr % 8 == 0) && ((reinterpret_cast<uintptr_t>(p.R) & 15) == 0)));
  const int flags = (transA ? 1 : 0) | (transB ? 2 : 0) | (p.out_f32 ? 4 : 0) | (p.accumulate ? 8 : 0) | (p.R ? 16 : 0) |
                    (p.bias ? 32 : 0) | (p.act << 6) | (p.colscale ? 256 : 0) | (p.epi << 9) | (p.ln_in ? 4096 : 0) | (p.st_out ? 8192 : 0) |
                    (p.vec_ok ? 0 : 16384) | (rows16 ? 0 : 32768) | (any_layout ? 65536 : 0);
  // small extents are remembered per bucket (M < 256 in steps of 32, K < 512 in steps of 64): the labelled rows of a pass - the lm_head's M,
  // its weight gradient's K - change from pass to pass, and a measurement (a device synchronisation, ~10 ms of trial launches) for every new
  // count landed inside training steps: bench.py's instrumented window showed a 15.6 ms "launch" of the [149, 151 937, 2560] product
  const int mkey = p.M < 256 ? (p.M + 31) / 32 * 32 : p.M;
  const int kkey = p.K < 512 ? (p.K + 63) / 64 * 64 : p.K;
  const TuneKey key(mkey, p.N, kkey, nbatch, flags);
  std::lock_guard<std::mutex> lock(g_tune_mutex);
  if (!g_tune_file_read) tune_file_read();
  static int log_on = -1;
  if (log_on < 0) log_on = getenv("VQ3_GEMM_AUTOTUNE_LOG") ? 1 : 0;
  auto it = g_tuned.find(key);
  // (an entry is only as good as the candidate list it was measured against: a table written by another build, or by the other
  // dispatch path under the same key, may name a configuration this call cannot run - such an entry is measured again / falls back)
  static std::map<TuneKey, int> said;      // (VQ3_GEMM_AUTOTUNE_LOG: every key's choice once, so that two ranks' logs can be compared)
  if (it != g_tuned.end() && std::find(cands.begin(), cands.end(), it->second) != cands.end()) {
    if (log_on && said.emplace(key, it->second).second)
      fprintf(stderr, "[vq3 gemm choice] M=%d N=%d K=%d batch=%d flags=%d -> %d (table)\n", mkey, p.N, kkey, nbatch, flags, it->second);
    return it->second;
  }
  if (!autotune_on(s) || g_hold) {
    // not remembered: a later, tunable call may still measure
    if (log_on && said.emplace(key, fallback).second)
      fprintf(stderr, "[vq3 gemm choice] M=%d N=%d K=%d batch=%d flags=%d -> %d (heuristic)\n", mkey, p.N, kkey, nbatch, flags, fallback);
    return fallback;
  }
  int best = tune(p, cands, transA, transB, nbatch, s);
  if (best < 0) best = fallback;
  g_tuned[key] = best;
  tune_file_append(key, best);
  return best;
}

}  // namespace vq3gemm

using namespace vq3gemm;

extern "C" int vq3_gemm_tune_table_load(const char* path, int32_t* entries_out) {
  VQ3_CHECK_ARG(path && *path, "gemm_tune_table_load: null path");
  std::lock_guard<std::mutex> lock(g_tune_mutex);
  const int n = tune_table_read(path);
  VQ3_CHECK_ARG(n >= 0, "gemm_tune_table_load: cannot read %s", path);
  if (entries_out) *entries_out = n;
  return 0;
}

extern "C" int vq3_gemm_tune_workspace(void* ptr, int64_t bytes) {
  VQ3_CHECK_ARG((ptr == nullptr) == (bytes == 0) && bytes >= 0 && ((uintptr_t)ptr % 256 == 0), "gemm_tune_workspace: bad workspace");
  std::lock_guard<std::mutex> lock(g_tune_mutex);
  g_ws = ptr; g_ws_bytes = (size_t)bytes; g_ws_dev = -1;
  return 0;
}

extern "C" int vq3_gemm_autotune_hold(int32_t on) {
  std::lock_guard<std::mutex> lock(g_tune_mutex);
  g_hold = on ? 1 : 0;
  return 0;
}

extern "C" int vq3_gemm_workspace_provider(vq3_ws_provider_t fn) {
  std::lock_guard<std::mutex> lock(g_tune_mutex);
  g_provider = fn;
  if (g_ws_dev >= 0) { g_ws = nullptr; g_ws_bytes = 0; g_ws_dev = -1; }      // a workspace the old provider gave is no longer ours
  gemm_split_set_provider(fn);
  return 0;
}
