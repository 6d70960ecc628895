// The registry of bf16 GEMM kernel configurations: every id that gemm_tune_gfx950.txt, a VQ3_GEMM_TUNE_FILE, VQ3_GEMM_CFG or
// vq3_gemm_force_config may name is one constant and one row here, and launch_config (gemm.hip) is the only id -> launcher map.
// The numbers are a file format: they never change.
#pragma once
#include <vector>

#include "gemm_common.h"

namespace vq3gemm {

enum : int {
  CFG_AUTO = -3,            // g_forced_cfg: nothing forced (table, measurement, heuristic)
  CFG_FROM_ENV = -2,        // g_forced_cfg: VQ3_GEMM_CFG has not been read yet
  // gemm2.hip (ids are launch_gemm_v2's cfg argument)
  CFG_V2_2STAGE = 7,        // 128x128 tile, 8 waves, 2 stages, two workgroups per CU
  CFG_V2_RING3_LOAD4 = 9,   // 128x128 tile, 8 compute + 4 DMA-loader waves, 3-stage ring
  CFG_V2_256x128 = 11,      // 256x128 tile, 8 compute + 2 DMA-loader waves, 3-stage ring
  CFG_V2_RING4 = 13,        // 128x128 tile, 8 compute + 2 DMA-loader waves, 4-stage ring: takes every NT shape
  CFG_V2_224x128 = 15,
  CFG_V2_192x128 = 16,
  CFG_V2_192x128_2WG = 17,
  // gemm6.hip, 8-phase kernels (id - CFG_V6_256x256 is launch_gemm_v6's shape argument)
  CFG_V6_256x256 = 20,
  CFG_V6_256x128 = 21,
  CFG_V6_128x256 = 22,
  CFG_V7 = 24,              // gemm7.hip: 256x128 tile, two workgroups per CU
  CFG_V6_SPLIT_LAST = 25,   // 256x256 with the last round's tiles split along K
  CFG_SPLIT_ROWS = 30,      // whole rounds of 256x256 tiles + a small-tile launch for the remaining rows
  // any operand layout, K % 8 == 0 (id - CFG_V3_BASE is launch_gemm_v3's nstage argument)
  CFG_V3_2STAGE = 102,
  CFG_V3_RING = 103,
  CFG_V3_256x128 = 105,
  CFG_V6_KM = 106,          // gemm6.hip, both operands k-major
  CFG_V6_KM_SPLIT = 107,    // the same with the last round split along K
};

constexpr int CFG_V3_BASE = 100;      // not a configuration: CFG_V3_* = CFG_V3_BASE + launch_gemm_v3's nstage

enum : int { SERVES_NT = 1, SERVES_SWIGLU_FWD = 2, SERVES_ANY = 4 };     // NT = both operands K-contiguous, K % 64 == 0

struct GemmConfig {
  int id;
  const char* name;             // log / error text
  int serves;                   // dispatch paths that may run it
  int fallback, fallback_swiglu_fwd;      // what runs when the launcher answers -1 ("outside my contract"); 0 = it never does
};

constexpr GemmConfig kGemmConfigs[] = {
    {CFG_V2_2STAGE, "gemm_bf16_nt(v2, 2 stages)", SERVES_NT, 0, 0},
    {CFG_V2_RING3_LOAD4, "gemm_bf16_nt(v2, 3-stage ring, 4 loaders)", SERVES_NT, 0, 0},
    {CFG_V2_256x128, "gemm_bf16_nt(v2, 256x128)", SERVES_NT, 0, 0},
    {CFG_V2_RING4, "gemm_bf16_nt(v2, 4-stage ring)", SERVES_NT, 0, 0},
    {CFG_V2_224x128, "gemm_bf16_nt(v2, 224x128)", SERVES_NT, 0, 0},
    {CFG_V2_192x128, "gemm_bf16_nt(v2, 192x128)", SERVES_NT, 0, 0},
    {CFG_V2_192x128_2WG, "gemm_bf16_nt(v2, 192x128, 2 stages)", SERVES_NT, 0, 0},
    {CFG_V6_256x256, "gemm_bf16_nt(v6, 256x256)", SERVES_NT | SERVES_SWIGLU_FWD, 0, 0},
    {CFG_V6_256x128, "gemm_bf16_nt(v6, 256x128)", SERVES_NT | SERVES_SWIGLU_FWD, 0, 0},
    {CFG_V6_128x256, "gemm_bf16_nt(v6, 128x256)", SERVES_NT | SERVES_SWIGLU_FWD, 0, 0},
    {CFG_V7, "gemm_bf16_nt(v7)", SERVES_NT | SERVES_SWIGLU_FWD, CFG_V2_RING4, CFG_V6_256x256},
    {CFG_V6_SPLIT_LAST, "gemm_bf16_nt(v6, last round split)", SERVES_NT, CFG_V6_256x256, 0},
    {CFG_SPLIT_ROWS, "gemm_bf16_nt(v6 + row tail)", SERVES_NT, 0, 0},
    {CFG_V3_2STAGE, "gemm_bf16_nt(v3, 2 stages)", SERVES_ANY, 0, 0},
    {CFG_V3_RING, "gemm_bf16_nt(v3, loader ring)", SERVES_ANY, 0, 0},
    {CFG_V3_256x128, "gemm_bf16_nt(v3, 256x128)", SERVES_ANY, 0, 0},
    {CFG_V6_KM, "gemm_bf16_nt(v6 k-major)", SERVES_ANY, CFG_V3_256x128, 0},
    {CFG_V6_KM_SPLIT, "gemm_bf16_nt(v6 k-major, last round split)", SERVES_ANY, CFG_V3_256x128, 0},
};

inline const GemmConfig* find_config(int id) {
  for (const GemmConfig& c : kGemmConfigs)
    if (c.id == id) return &c;
  return nullptr;
}

// gemm.hip: launches configuration cfg. 0 = launched, > 0 = error (vq3_set_error called), -1 = outside the kernel's contract or not a
// configuration, nothing launched: the tuner skips such a candidate, the dispatcher follows the registry's fallback column.
int launch_config(GemmParams& p, int cfg, int transA, int transB, int nbatch, hipStream_t stream);

// gemm_tune.hip: the configuration the shipped / loaded table names for this call, else (where measuring is allowed) the fastest of
// cands measured once on the caller's stream and remembered, else `fallback`. any_layout separates the keys of the two dispatch paths.
int tuned_choice(const GemmParams& p, int transA, int transB, int nbatch, hipStream_t stream, const std::vector<int>& cands, int fallback,
                 bool any_layout = false);

}  // namespace vq3gemm
