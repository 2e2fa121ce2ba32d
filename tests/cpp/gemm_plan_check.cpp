// Stand-alone check of csrc/gemm_plan.h (the host-side plan of gemm_nt / gemm_dgrad /
// gemm_wgrad): over every family, tile override, split count and a grid of sizes around
// every threshold, each plan names a built kernel or throws in a listed case; every built
// kernel is named by some plan; the documented fallbacks; and the plans the project records
// for its own launches.  tests/test_gemm_plan_cpu.py compiles it with the address and
// undefined-behaviour sanitizers and runs it.
#include "gemm_plan.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <tuple>
#include <vector>

static int g_checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    ++g_checks;                                                     \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

struct Family {
  bool at, bt;
  int epi;
};
static const int NT_EPIS[] = {EPI_BF16, EPI_F32,   EPI_QKV,   EPI_RESID, EPI_GELU,  EPI_HEAD,
                              EPI_EMBED, EPI_DGELU, EPI_HEADR, EPI_HEADL, EPI_HEADRS};
static std::vector<Family> families() {
  std::vector<Family> f;
  for (int epi : NT_EPIS) f.push_back({false, false, epi});
  for (int epi : {EPI_BF16, EPI_F32, EPI_DGELU}) f.push_back({false, true, epi});
  f.push_back({true, true, EPI_ATOMIC});
  return f;
}
static const int MS[] = {1, 33, 300, 2080, 4160, 16383, 16384, 16448, 20032};
static const int NS[] = {4, 64, 68, 192, 256, 384, 1152, 1536};
static const int KS[] = {8, 48, 64, 128, 192, 384, 512, 576, 1152, 1536};

// the message a call throws with, or "" if it returns
template <class F>
static std::string thrown(F f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    return e.what();
  }
  return "";
}
static bool has(const std::string& s, const char* part) { return s.find(part) != std::string::npos; }

using Kernel = std::tuple<bool, bool, int, int, int, int, int>;  // at, bt, epi, bm, bn, waves, stages

// the check's own statement of which epilogues have 8-wave tiles and which are DMA-only
static bool wide8(int epi) {
  return epi == EPI_BF16 || epi == EPI_F32 || epi == EPI_QKV || epi == EPI_RESID || epi == EPI_GELU ||
         epi == EPI_EMBED || epi == EPI_DGELU;
}
static bool dma_only(int epi) { return epi == EPI_HEADR || epi == EPI_HEADL || epi == EPI_HEADRS; }

static void check_tuple(const GemmPlan& p, bool dma, int bm, int bn, int waves, int stages) {
  CHECK(p.dma == dma && p.bm == bm && p.bn == bn && p.waves == waves && p.stages == stages);
}

int main() {
  // ---- 1. every plan names a built kernel, or throws in a listed case; 2. the converse
  std::set<Kernel> named;
  long plans = 0, thrown8 = 0, thrown_dma = 0;
  for (const Family& f : families())
    for (int forced = -1; forced <= 6; ++forced)
      for (int splits : {1, 2, 4})
        for (int M : MS)
          for (int N : NS)
            for (int K : KS) {
              GemmPlan p;
              const std::string err = thrown([&] { p = gemm_plan(f.epi, f.at, f.bt, M, N, K, splits, forced); });
              const bool dma = f.at || K % 64 == 0;
              const bool want8 = dma && !f.at && forced >= 4 && !wide8(f.epi);
              const bool want_dma = !dma && dma_only(f.epi);
              if (want8 || want_dma) {
                CHECK(want8 ? has(err, "8-wave tiles are not built for this epilogue")
                            : has(err, "needs the LDS-DMA GEMM") && has(err, "gemm_nt: EPI_HEAD"));
                ++(want8 ? thrown8 : thrown_dma);
                continue;
              }
              CHECK(err.empty());
              ++plans;
              CHECK(p.dma == dma);
              if (p.dma) {
                CHECK(gemm_kernel_built(f.at, f.bt, f.epi, p.bm, p.bn, p.waves, p.stages));
                named.insert(Kernel{f.at, f.bt, f.epi, p.bm, p.bn, p.waves, p.stages});
              } else {  // the plain kernel: its two tiles, double-buffered, whatever the override
                CHECK(!f.at && p.bn == 64 && (p.bm == 32 || p.bm == 64) && p.waves == 4 && p.stages == 2);
              }
              CHECK(p.stages * (p.bm + p.bn) * 128 <= 160 * 1024);
              const int kt = (K + 63) / 64;
              CHECK(p.ktiles_per_split >= 1 && p.splits >= 1 && p.splits <= splits);
              CHECK((p.splits - 1) * p.ktiles_per_split < kt && p.splits * p.ktiles_per_split >= kt);
              CHECK(p.tiles == ((M + p.bm - 1) / p.bm) * ((N + p.bn - 1) / p.bn));
              CHECK(p.grid == p.tiles * p.splits);
            }
  CHECK(plans > 0 && thrown8 > 0 && thrown_dma > 0);
  int built = 0;
  for (int fam = 0; fam < 4; ++fam)
    for (int epi = 0; epi <= EPI_HEADRS; ++epi)
      for (const GemmTile& t : GEMM_TILES)
        for (int s = 1; s <= 5; ++s) {
          const bool at = fam & 1, bt = fam & 2;
          if (!gemm_kernel_built(at, bt, epi, t.bm, t.bn, t.waves, s)) continue;
          ++built;
          if (!named.count(Kernel{at, bt, epi, t.bm, t.bn, t.waves, s}))
            std::fprintf(stderr, "built but never planned: at %d bt %d epi %d %dx%d waves %d stages %d\n", at, bt, epi,
                         t.bm, t.bn, t.waves, s);
          CHECK(named.count(Kernel{at, bt, epi, t.bm, t.bn, t.waves, s}) == 1);
        }
  CHECK(built == (int)named.size() && built == gemm_kernels_built());
  // 11 x 8 + 6 x 3 + 2 + 3 plain-operand, 3 x 6 + 2 x 3 + 2 transposed-B, 2 weight-gradient
  CHECK(built == 139);
  // the 4-stage 256x128 ring (192 KiB) does not fit: not a kernel
  CHECK(!gemm_kernel_built(false, false, EPI_BF16, 256, 128, 8, 4) && !gemm_kernel_built(false, true, EPI_F32, 256, 128, 8, 4));
  CHECK(gemm_kernel_built(false, false, EPI_BF16, 256, 128, 8, 3));

  // ---- the other throws: sizes, families without kernels
  for (int bad = 0; bad < 4; ++bad) {
    const int v[4] = {bad == 0 ? 0 : 64, bad == 1 ? 0 : 64, bad == 2 ? 0 : 64, bad == 3 ? 0 : 1};
    CHECK(has(thrown([&] { gemm_plan(EPI_BF16, false, false, v[0], v[1], v[2], v[3], -1); }), "M, N, K, splits >= 1"));
  }
  CHECK(has(thrown([] { gemm_plan(EPI_BF16, false, false, 64, 64, 64, 1, 7); }), "tile override"));
  CHECK(has(thrown([] { gemm_plan(EPI_BF16, false, false, 64, 64, 64, 1, -2); }), "tile override"));
  for (int fam = 0; fam < 4; ++fam)
    for (int epi = -1; epi <= EPI_HEADRS + 1; ++epi) {
      const bool at = fam & 1, bt = fam & 2;
      bool known = false;
      for (const Family& f : families()) known = known || (f.at == at && f.bt == bt && f.epi == epi);
      CHECK(gemm_family_built(at, bt, epi) == known);
      for (int forced : {-1, 4})
        for (int K : {48, 64}) {
          const std::string err = thrown([&] { gemm_plan(epi, at, bt, 300, 192, K, 1, forced); });
          if (!known) CHECK(has(err, "no kernel is built for this operand layout and epilogue"));
          else CHECK(!has(err, "no kernel is built"));
        }
    }
  CHECK(has(thrown([] { gemm_plan(EPI_RESID, false, true, 20032, 384, 384, 1, 4); }), "no kernel is built"));
  CHECK(has(thrown([] { gemm_plan(EPI_HEADR, false, false, 4160, 192, 48, 1, -1); }), "gemm_nt: EPI_HEADR needs the LDS-DMA GEMM"));
  CHECK(has(thrown([] { gemm_plan(EPI_HEADL, false, false, 4160, 192, 48, 1, -1); }), "gemm_nt: EPI_HEADL needs the LDS-DMA GEMM"));
  CHECK(has(thrown([] { gemm_plan(EPI_HEADRS, false, false, 4160, 192, 48, 1, -1); }), "gemm_nt: EPI_HEADRS needs the LDS-DMA GEMM"));

  // ---- 3. the documented fallbacks, for every epilogue (K % 64 == 0; both depths' sizes)
  for (const Family& f : families()) {
    if (f.at) continue;
    for (int M : {300, 20032})
      for (int N : {192, 1152}) {
        auto tile = [&](int cfg) {
          const GemmPlan p = gemm_plan(f.epi, false, f.bt, M, N, 384, 1, cfg);
          return std::make_tuple(p.bm, p.bn, p.waves);
        };
        CHECK(tile(3) == (f.bt ? std::make_tuple(128, 64, 4) : std::make_tuple(128, 128, 4)));
        if (!wide8(f.epi)) continue;
        const bool dgelu = f.epi == EPI_DGELU;
        CHECK(tile(4) == (dgelu ? std::make_tuple(128, 128, 8) : std::make_tuple(256, 128, 8)));
        CHECK(tile(5) == std::make_tuple(128, 128, 8));
        const bool big192 = !f.bt && (f.epi == EPI_BF16 || f.epi == EPI_QKV || f.epi == EPI_GELU);
        CHECK(tile(6) == (big192 ? std::make_tuple(256, 192, 8) : dgelu ? std::make_tuple(128, 128, 8) : std::make_tuple(256, 128, 8)));
      }
  }
  for (int forced = -1; forced <= 6; ++forced)  // the weight gradient: 64x64 whatever the override
    for (bool big : {false, true}) {
      // 594 x 4 workgroups of 8 k-tiles: over 256 x 2, the 3-stage ring; 36 x 4: the 4-stage one
      const GemmPlan p = gemm_plan(EPI_ATOMIC, true, true, big ? 2080 : 384, big ? 1152 : 384, 2048, 4, forced);
      check_tuple(p, true, 64, 64, 4, big ? 3 : 4);
    }

  // ---- 4. the project's own launches (automatic choice), as recorded from the parent
  auto nt = [](int epi, int M, int N, int K) { return gemm_plan(epi, false, false, M, N, K, 1, -1); };
  check_tuple(nt(EPI_QKV, 2080, 1152, 384), true, 64, 64, 4, 3);     // ViT-tiny
  check_tuple(nt(EPI_RESID, 2080, 384, 384), true, 32, 64, 4, 4);
  check_tuple(nt(EPI_GELU, 2080, 1536, 384), true, 64, 64, 4, 3);
  check_tuple(nt(EPI_RESID, 2080, 384, 1536), true, 32, 64, 4, 4);
  check_tuple(nt(EPI_EMBED, 2048, 384, 192), true, 32, 64, 4, 4);
  check_tuple(nt(EPI_HEADL, 2080, 192, 384), true, 32, 64, 4, 4);
  check_tuple(nt(EPI_QKV, 20032, 1152, 384), true, 256, 192, 8, 2);  // vit_small_200
  check_tuple(nt(EPI_RESID, 20032, 384, 384), true, 256, 128, 8, 3);
  check_tuple(nt(EPI_GELU, 20032, 1536, 384), true, 256, 128, 8, 3);
  check_tuple(nt(EPI_DGELU, 20032, 384, 1536), true, 64, 64, 4, 4);
  check_tuple(gemm_plan(EPI_DGELU, false, true, 20032, 384, 1536, 1, -1), true, 64, 64, 4, 4);
  check_tuple(gemm_plan(EPI_BF16, false, true, 20032, 384, 1152, 1, -1), true, 256, 128, 8, 3);  // QKV input gradient
  check_tuple(nt(EPI_GELU, 4160, 1536, 384), true, 64, 64, 4, 3);    // sampler
  check_tuple(nt(EPI_HEADR, 4160, 192, 384), true, 32, 64, 4, 4);
  check_tuple(gemm_plan(EPI_ATOMIC, true, true, 384, 384, 2080, 4, -1), true, 64, 64, 4, 4);
  check_tuple(nt(EPI_F32, 300, 200, 48), false, 32, 64, 4, 2);
  {  // the split the launch takes: 33 k-tiles in 4 slices of 9, the last of 6
    const GemmPlan p = gemm_plan(EPI_ATOMIC, true, true, 384, 384, 2080, 4, -1);
    CHECK(p.ktiles_per_split == 9 && p.splits == 4 && p.tiles == 36 && p.grid == 144);
    // a request that would leave a slice empty shrinks: 3 k-tiles in "4" slices are 3 of 1
    const GemmPlan q = gemm_plan(EPI_F32, false, true, 300, 64, 192, 4, -1);
    CHECK(q.ktiles_per_split == 1 && q.splits == 3);
  }

  std::printf("gemm_plan_check: %d checks passed (%ld plans, %ld + %ld listed throws, %d kernels)\n", g_checks, plans,
              thrown8, thrown_dma, built);
  return 0;
}
