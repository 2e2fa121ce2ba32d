// Host-side plan of the main GEMM family (gemm_nt, gemm_dgrad, gemm_wgrad): which of the
// instantiated kernels a launch gets -- LDS-DMA ring or the plain K % 64 != 0 kernel, the
// tile after every fallback, waves per workgroup, ring depth -- and its K split and grid.
// Plain C++ (no HIP, no torch): gemm.hip launches from the plan and instantiates its
// kernels against gemm_kernel_built, torch.ops.ddim_cold.gemm_plan reports the same plan,
// and tests/cpp/gemm_plan_check.cpp checks it on its own.  Every rule is written here once.
#pragma once
#include <stdexcept>
#include <string>

enum GemmEpi : int {
  EPI_BF16 = 0,    // C bf16 = acc (+bias)
  EPI_F32 = 1,     // C f32 = acc (+bias)
  EPI_QKV = 2,     // +bias, scatter to head-major [3,B,H,N,hd] bf16
  EPI_RESID = 3,   // C f32 = res + DropPath(Dropout(acc+bias))
  EPI_GELU = 4,    // C = u = acc+bias (bf16) ; C2 = h = Dropout(GELU(u)) (bf16)
  EPI_HEAD = 5,    // +bias, unpatchify token rows into a [B,C,H,W] f32 image
  EPI_EMBED = 6,   // patch rows -> token rows: +bias +pos +temb[t], Dropout, f32
  EPI_DGELU = 7,   // C bf16 = Dropout(acc) * GELU'(aux)
  EPI_ATOMIC = 8,  // C f32 += acc (split-K / gradient accumulate) ; bias -> fused column sum
  EPI_ACC = 9,     // C f32 += acc, one writer per element (no split) ; bias likewise
  EPI_HEADR = 10,  // sampler step on patch rows: +bias, clamp (+DDIM update), f32 [B*P][C*p*p]
                   //   in head-output column order (contiguous: vector epilogue)
  EPI_HEADL = 11,  // training loss on patch rows: smooth-L1 vs a [B*P][C*p*p] target (head order),
                   //   token-layout bf16 gradient, one loss partial per workgroup
  EPI_HEADRS = 12, // EPI_HEADR's DDIM update with noise (eta > 0): x_next += sigma z, z drawn in the
                   //   epilogue (randn_kernel's element at the destination index; rng, site_drop = site)
};

constexpr int GEMM_BK = 64;                  // depth of one k-tile
constexpr int GEMM_LDS_BUDGET = 160 * 1024;  // LDS of one CU: the ring of a workgroup fits in it
constexpr int BIG_M = 16384;                 // rows from which the 8-wave tiles are chosen

// tile configs: 0 = 32x64, 1 = 64x64, 2 = 128x64, 3 = 128x128 (4 waves, 2x2);
// 4 = 256x128, 5 = 128x128, 6 = 256x192 (8 waves, 4x2: 512-thread workgroups, for M >= BIG_M)
struct GemmTile {
  int bm, bn, waves;
};
constexpr int GEMM_CONFIGS = 7;
constexpr GemmTile GEMM_TILES[GEMM_CONFIGS] = {{32, 64, 4},   {64, 64, 4},   {128, 64, 4},  {128, 128, 4},
                                               {256, 128, 8}, {128, 128, 8}, {256, 192, 8}};
constexpr int CFG_W8_256 = 4, CFG_W8_128 = 5, CFG_W8_192 = 6;

// What a launch gets.  stages: the depth of the LDS-DMA ring (2 for the plain kernel, which
// double-buffers).  K runs in `splits` slices of `ktiles_per_split` k-tiles, none empty (the
// requested split count shrinks to that); `tiles` output tiles, grid = tiles x splits workgroups.
struct GemmPlan {
  bool dma = false;
  int bm = 0, bn = 0, waves = 0, stages = 0;
  int ktiles_per_split = 0, splits = 0, tiles = 0, grid = 0;
};

// The (operand layout, epilogue) families with kernels: gemm_nt's eleven epilogues on plain
// operands, gemm_dgrad's three with B transposed, gemm_wgrad's with both transposed.
constexpr bool gemm_family_built(bool at, bool bt, int epi) {
  if (at) return bt && epi == EPI_ATOMIC;
  if (bt) return epi == EPI_BF16 || epi == EPI_F32 || epi == EPI_DGELU;
  return epi >= EPI_BF16 && epi <= EPI_HEADRS && epi != EPI_ATOMIC && epi != EPI_ACC;
}
// epilogues with no 4-wave workgroup reduction (HEAD / HEADL sum loss partials over 4 waves):
// the ones with 8-wave tiles
constexpr bool gemm_wide8_epi(int epi) {
  return epi == EPI_BF16 || epi == EPI_F32 || epi == EPI_QKV || epi == EPI_RESID || epi == EPI_GELU ||
         epi == EPI_EMBED || epi == EPI_DGELU;
}
// ... and those the 256x192 tile is built for (plain operands only)
constexpr bool gemm_big192_epi(bool bt, int epi) {
  return !bt && (epi == EPI_BF16 || epi == EPI_QKV || epi == EPI_GELU);
}
// epilogues with a vector epilogue only: no plain (K % 64 != 0) kernel can run them
constexpr bool gemm_dma_only_epi(int epi) { return epi == EPI_HEADR || epi == EPI_HEADL || epi == EPI_HEADRS; }

// Ring depth of the LDS-DMA GEMM for BM x BN tiles.  Keep every workgroup of the grid
// co-resident (one round): a 4-stage ring allows 160 KiB / (4 x stage) workgroups per CU, a
// 3-stage ring 4/3 of that; 256x128 fits 3 stages only, 256x192 only 2.
constexpr int gemm_stage_bytes(int bm, int bn) { return (bm + bn) * 2 * GEMM_BK; }
constexpr int gemm_ring_stages(int bm, int bn, int workgroups, int ktiles_per_split) {
  const int stage = gemm_stage_bytes(bm, bn);
  if (3 * stage > GEMM_LDS_BUDGET) return 2;
  if (4 * stage > GEMM_LDS_BUDGET) return 3;
  const int per_cu4 = GEMM_LDS_BUDGET / (4 * stage);
  return workgroups > 256 * per_cu4 && ktiles_per_split <= 8 ? 3 : 4;
}
// the depths that rule can produce for a tile
constexpr bool gemm_ring_depth_possible(int bm, int bn, int stages) {
  const int stage = gemm_stage_bytes(bm, bn);
  if (3 * stage > GEMM_LDS_BUDGET) return stages == 2;
  if (4 * stage > GEMM_LDS_BUDGET) return stages == 3;
  return stages == 3 || stages == 4;
}

// Which LDS-DMA ring kernels exist (gemm.hip instantiates exactly these and no launch names
// another).  The plain kernel is built on its two tiles, 32x64 and 64x64, for every family.
constexpr bool gemm_kernel_built(bool at, bool bt, int epi, int bm, int bn, int waves, int stages) {
  if (!gemm_family_built(at, bt, epi) || !gemm_ring_depth_possible(bm, bn, stages)) return false;
  if (at) return bm == 64 && bn == 64 && waves == 4;  // transposed A (wgrad): 64x64
  if (waves == 4) {
    if (bn == 64) return bm == 32 || bm == 64 || bm == 128;
    return !bt && bm == 128 && bn == 128;  // transposed B (dgrad): BN = 64 (4 waves) or 128 (8 waves)
  }
  if (waves != 8 || !gemm_wide8_epi(epi)) return false;
  if (bm == 128 && bn == 128) return true;
  // DGELU at 256x128 spills (88 B/lane of scratch): not built
  if (bm == 256 && bn == 128) return epi != EPI_DGELU;
  return bm == 256 && bn == 192 && gemm_big192_epi(bt, epi);
}
// how many that is (gemm.hip's instantiation list is checked against it)
constexpr int gemm_kernels_built() {
  int n = 0;
  for (int f = 0; f < 4; ++f)
    for (int epi = EPI_BF16; epi <= EPI_HEADRS; ++epi)
      for (const GemmTile& t : GEMM_TILES)
        for (int s = 2; s <= 4; ++s) n += gemm_kernel_built(f & 1, f & 2, epi, t.bm, t.bn, t.waves, s);
  return n;
}

// The tile config that runs where `cfg` is asked for: the fallbacks.
constexpr int gemm_cfg_fallback(int cfg, bool bt, int epi) {
  // 256x192 tiles, 2-stage ring (57 KiB per stage): N = 1152 in 6 column tiles; where it
  // is not built for the epilogue: the 256-row config
  if (cfg == CFG_W8_192 && !gemm_big192_epi(bt, epi)) cfg = CFG_W8_256;
  // DGELU at 256x128 spills (88 B/lane of scratch): its 256-row config is the 128-row one
  if (cfg == CFG_W8_256 && epi == EPI_DGELU) cfg = CFG_W8_128;
  if (cfg == 3 && bt) cfg = 2;  // transposed B (dgrad): BN = 64 on 4 waves
  return cfg;
}

// Tile choice.  M < BIG_M (ViT-tiny / sampler shapes, M = 2-4k): 64x64 when that
// alone gives ~1 workgroup per CU, else 32x64.  A cost model "operand bytes per CU"
// that picked 128x64 / 128x128 for the big shapes of those sizes measured SLOWER
// everywhere (qkv 2080x1152x384: 11.9 us at 128x128 vs 7.5 at 64x64; train step
// -10%): more, smaller workgroups hide latency better than fewer bytes help, and was
// removed.  M >= BIG_M (vit_small_200: M = 20,032): 8-wave 256x128 tiles (4x the
// MFMA work per operand byte of 64x64, one 144 KiB 3-stage ring per CU), for the
// epilogues that support them (gemm_wide8_epi).  `forced` >= 0 (gemm_set_tile_override,
// tests and micro-benchmarks) is the config itself.  The LDS-DMA ring needs K % 64 == 0
// for k-contiguous operands (transposed operands get zero rows past K from the buffer
// bounds check).
inline int gemm_pick_tiles(int M, int N, int splits, bool at, bool wide8, bool qkv, int forced) {
  if (at) return 1;  // transposed A (wgrad): 64x64
  if (forced >= 0) return forced;
  // 8-wave 256x128 tiles only when they still give about one tile per CU: the
  // oxford_flower sampler's N = 256 GEMMs (M = 16,448: 130 such tiles) run faster on
  // 64x64 / 32x64 tiles (tools/ub_gemm_large.py 16448 .. 256: residual 19.7 vs 15.9 us,
  // GELU 16.0 vs 13.2; vit_small_200 N = 384 at M = 20,032: 237 tiles, 8-wave faster)
  // the QKV projection (N = 3D = 1,152 at vit_small_200): 256x192 tiles, 2-stage ring --
  // 474 workgroups (1.85 rounds of 256 CUs) instead of 711 (2.8 rounds): 489 -> 453 us of
  // QKV per step (profiles/qkv192_r6.txt)
  if (wide8 && M >= BIG_M && ((M + 255) / 256) * ((N + 127) / 128) >= 236)
    return qkv && N % 192 == 0 ? CFG_W8_192 : CFG_W8_256;
  return ((M + 63) / 64) * ((N + 63) / 64) * splits >= 240 ? 1 : 0;
}

// The LDS-DMA path's tile config for an epilogue, before the fallbacks.
inline int gemm_dma_cfg(int epi, bool at, int M, int N, int splits, int forced) {
  // DGELU (input gradient through GELU + dropout, bf16 out) stays on 4-wave tiles at
  // every measured M (M = 20,032: 25.5 vs 26.5 us; 40,064: 42.1 vs 49.9)
  int cfg = gemm_pick_tiles(M, N, splits, at, gemm_wide8_epi(epi) && epi != EPI_DGELU, epi == EPI_QKV, forced);
  // the GELU epilogue (erf-GELU + dropout per element, two bf16 outputs) is the
  // heaviest in vector instructions: twice the waves of 32x64 tiles pay off on the
  // sampler shape (M=4160: 6.56 vs 7.14 us, tools/gpu_tile_sweep3.sh); the other
  // epilogues keep 64x64 there (QKV 11.45 vs 13.54, residual 6.65 vs 7.02)
  // the patch embedding likewise (sampler M=4,096: 7.83 vs 9.08 us, tools/ub_sampler_ends.py)
  if ((epi == EPI_GELU || epi == EPI_EMBED) && cfg == 1 && forced < 0 && ((M + 31) / 32) * ((N + 63) / 64) <= 1024)
    cfg = 0;
  return cfg;
}
// the non-DMA GEMM (K % 64 != 0) takes 64x64 tiles from here, 32x64 below; no override
inline bool gemm_plain_big(int M, int N, int splits) { return ((M + 63) / 64) * ((N + 63) / 64) * splits >= 240; }

inline const char* gemm_epi_name(int epi) {
  return epi == EPI_HEADR ? "EPI_HEADR" : epi == EPI_HEADL ? "EPI_HEADL" : epi == EPI_HEADRS ? "EPI_HEADRS" : "epilogue";
}

// The one place that turns a problem into a kernel: the launch of family (at, bt, epi) for
// an [M x N x K] problem asked to run in `splits` K slices, under tile override `forced`
// (-1: automatic).  Throws on sizes < 1 (or an override outside -1..6), on a family without kernels, on a DMA-only
// epilogue at K % 64 != 0 and on an 8-wave override for an epilogue without 8-wave tiles.
inline GemmPlan gemm_plan(int epi, bool at, bool bt, int M, int N, int K, int splits, int forced) {
  if (M < 1 || N < 1 || K < 1 || splits < 1) throw std::runtime_error("gemm_plan: M, N, K, splits >= 1");
  if (forced < -1 || forced >= GEMM_CONFIGS) throw std::runtime_error("gemm_plan: tile override -1 (auto) or 0..6");
  if (!gemm_family_built(at, bt, epi))
    throw std::runtime_error("gemm: no kernel is built for this operand layout and epilogue");
  GemmPlan pl;
  const int total_kt = (K + GEMM_BK - 1) / GEMM_BK;
  pl.ktiles_per_split = (total_kt + splits - 1) / splits;
  pl.splits = (total_kt + pl.ktiles_per_split - 1) / pl.ktiles_per_split;
  pl.dma = at || K % GEMM_BK == 0;
  int cfg;
  if (pl.dma) {
    cfg = gemm_cfg_fallback(gemm_dma_cfg(epi, at, M, N, splits, forced), bt, epi);
    if (GEMM_TILES[cfg].waves == 8 && !gemm_wide8_epi(epi))
      throw std::runtime_error("gemm: 8-wave tiles are not built for this epilogue");
  } else {
    if (gemm_dma_only_epi(epi))
      throw std::runtime_error(std::string("gemm_nt: ") + gemm_epi_name(epi) + " needs the LDS-DMA GEMM");
    cfg = gemm_plain_big(M, N, splits) ? 1 : 0;
  }
  const GemmTile& t = GEMM_TILES[cfg];
  pl.bm = t.bm;
  pl.bn = t.bn;
  pl.waves = t.waves;
  pl.tiles = ((M + t.bm - 1) / t.bm) * ((N + t.bn - 1) / t.bn);
  pl.grid = pl.tiles * pl.splits;
  pl.stages = pl.dma ? gemm_ring_stages(t.bm, t.bn, pl.grid, pl.ktiles_per_split) : 2;  // gemm_kernel double-buffers
  return pl;
}
