// Stand-alone check of csrc/attn_plan.h (the host-side plan of attn_fwd_launch /
// attn_bwd_launch): over both directions, both head dims, dropout and keep buffer on and
// off, head counts around the resident threshold and every N in 1..700 (plus 1030, 2501,
// 4096), the path equals a literal transcription of the rule, each plan names a built
// kernel or throws in a listed case, every built kernel is planned, and grid, block, LDS
// and keep words follow the formulas the launches used before the plan existed.
// tests/test_attn_plan_cpu.py compiles it with the address and undefined-behaviour
// sanitizers and runs it.
#include "attn_plan.h"

#include <cstdio>
#include <cstdlib>
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

// the check's own statement of the path rule
static AttnPath path_literal(int B, int H, int N) {
  if (N <= 128) return AttnPath::SHORT;
  if (128 < N && N < 384 && B * H < 192) return AttnPath::V1;
  if (128 < N && N <= 320 && B * H >= 192) return AttnPath::RESIDENT;
  if (N >= 384) return AttnPath::FLASH2;
  return AttnPath::V1;  // 320 < N < 384 with many heads
}
static int cdiv(int a, int b) { return (a + b - 1) / b; }

using Kernel = std::tuple<int, int, int, bool, bool>;  // template, hd, np, drop, keep

int main() {
  const std::pair<int, int> BHS[] = {{1, 1}, {2, 2}, {1, 191}, {48, 4}, {193, 1}, {1, 400}};
  std::vector<int> NS;
  for (int n = 1; n <= 700; ++n) NS.push_back(n);
  for (int n : {1030, 2501, 4096}) NS.push_back(n);

  std::set<Kernel> named;
  long plans = 0, thrown_keep = 0;
  int paths_seen[4] = {0, 0, 0, 0};
  for (int bwd = 0; bwd < 2; ++bwd)
    for (int hd : {32, 64})
      for (int drop = 0; drop < 2; ++drop)
        for (int have_keep = 0; have_keep < 2; ++have_keep)
          for (const auto& bh : BHS)
            for (int N : NS) {
              const int B = bh.first, H = bh.second;
              const long long BH = (long long)B * H;
              const AttnPath want = path_literal(B, H, N);
              AttnPlan p;
              const std::string err = thrown([&] { p = attn_plan(bwd, B, H, N, hd, drop, have_keep); });
              if (want == AttnPath::V1 && drop && have_keep) {  // the listed throw: no stored masks on v1
                CHECK(has(err, "no stored keep masks on this path (attn_keep_words returned 0)"));
                ++thrown_keep;
                continue;
              }
              CHECK(err.empty());
              ++plans;
              CHECK(p.path == want);
              ++paths_seen[(int)p.path];
              CHECK(p.hd == hd && p.drop == (bool)drop && p.keep == (drop && have_keep));
              const bool is_short = want == AttnPath::SHORT;
              const int NP = 32 * cdiv(N, 32);
              CHECK(p.np == (is_short ? NP : 0));
              // the kernels the launch runs: one, or dQ then dK/dV in the long backward
              std::vector<AttnKernel> ks;
              if (bwd) {
                if (is_short) ks = {AttnKernel::BWD_SHORT};
                else ks = {AttnKernel::BWD_DQ, AttnKernel::BWD_DKV};
              } else {
                ks = {want == AttnPath::SHORT      ? AttnKernel::FWD_SHORT
                      : want == AttnPath::V1       ? AttnKernel::FWD_V1
                      : want == AttnPath::RESIDENT ? AttnKernel::FWD_RESIDENT
                                                   : AttnKernel::FWD_FLASH2};
              }
              CHECK(p.kernel == ks[0]);
              for (AttnKernel k : ks) {
                const AttnKernelArgs t = attn_kernel_args(k, p);
                CHECK(attn_kernel_built(k, t.hd, t.np, t.drop, t.keep));
                named.insert(Kernel{(int)k, t.hd, t.np, t.drop, t.keep});
              }
              // geometry: the formulas of the launches before the plan
              const int RS = 2 * hd + 32;
              if (is_short) {
                CHECK(p.grid_x == BH && p.grid_y == 1 && p.block == 4 * NP);
                CHECK(p.lds == (bwd ? 4 * NP * RS + 2 * NP * (2 * NP + 32) : 2 * NP * RS));
              } else if (!bwd && want == AttnPath::RESIDENT) {
                CHECK(p.grid_x == BH && p.grid_y == 1 && p.block == 64 * cdiv(N, 32) && p.block <= 640);
                CHECK(p.lds == 2 * 64 * cdiv(N, 64) * RS);
              } else {
                const bool flash2 = !bwd && want == AttnPath::FLASH2;
                CHECK(p.grid_x == cdiv(N, flash2 ? 128 : 64) && p.grid_y == BH && p.block == 256 && p.lds == 0);
              }
              CHECK(p.block >= 64 && p.block <= 1024 && p.block % 64 == 0);
              CHECK(p.lds >= 0 && p.lds <= 160 * 1024);
              // keep words: none exactly on v1, 4 per padded row on short, one 64-bit word per
              // (query, 64-key tile) otherwise; the exported function agrees
              const long long words = is_short ? BH * NP * 4 : want == AttnPath::V1 ? 0 : BH * N * cdiv(N, 64) * 2;
              CHECK(p.keep_words == words && (words == 0) == (want == AttnPath::V1));
              CHECK(attn_keep_words(B, H, N, hd) == words);
            }
  CHECK(plans > 0 && thrown_keep > 0);
  for (int n : paths_seen) CHECK(n > 0);

  // ---- every built kernel is planned by some point, and there are 58 of them
  int built = 0;
  for (int k = 0; k < ATTN_KERNEL_TEMPLATES + 1; ++k)
    for (int hd : {0, 16, 32, 48, 64, 96, 128})
      for (int np : {0, 16, 32, 64, 96, 128, 160})
        for (int f = 0; f < 4; ++f) {
          const bool drop = f & 1, keep = f & 2;
          if (!attn_kernel_built((AttnKernel)k, hd, np, drop, keep)) continue;
          ++built;
          if (!named.count(Kernel{k, hd, np, drop, keep}))
            std::fprintf(stderr, "built but never planned: template %d hd %d np %d drop %d keep %d\n", k, hd, np, drop, keep);
          CHECK(named.count(Kernel{k, hd, np, drop, keep}) == 1);
        }
  CHECK(built == (int)named.size() && built == attn_kernels_built());
  // 2 v1, 4 flash v2, 4 resident, 8 long backward, 16 short forward, 24 short backward
  CHECK(built == 58);
  static_assert(attn_kernels_built() == 58, "constexpr count");
  CHECK(!attn_kernel_built(AttnKernel::BWD_SHORT, 32, 96, false, true));  // stored flags without dropout
  CHECK(!attn_kernel_built(AttnKernel::FWD_V1, 32, 0, true, false));      // v1 has no dropout template flag
  CHECK(!attn_kernel_built(AttnKernel::FWD_SHORT, 32, 160, false, false));

  // ---- the recorded plans
  CHECK(attn_keep_words(2, 2, 2501, 64) == 2LL * 2 * 2501 * 40 * 2);
  CHECK(attn_keep_words(4, 12, 65, 32) == 4LL * 12 * 96 * 4);
  CHECK(attn_keep_words(1, 4, 257, 64) == 0);
  {  // the ViT-tiny step's attention: 48 heads of 65 tokens in 6-wave workgroups
    const AttnPlan f = attn_plan(false, 4, 12, 65, 32, true, true), b = attn_plan(true, 4, 12, 65, 32, true, true);
    CHECK(f.path == AttnPath::SHORT && f.np == 96 && f.block == 384 && f.grid_x == 48 && f.lds == 2 * 96 * 96);
    CHECK(b.kernel == AttnKernel::BWD_SHORT && b.keep && b.lds == 4 * 96 * 96 + 2 * 96 * 224);
  }
  {  // the largest short backward needs its dynamic-LDS limit raised, and fits
    const AttnPlan b = attn_plan(true, 1, 1, 128, 64, false, false);
    CHECK(b.lds == 155648 && b.lds > ATTN_LDS_DEFAULT && b.lds <= ATTN_LDS_BUDGET);
  }
  // a tiny p rounds to threshold 0: the caller says drop = false and gets the no-dropout kernel
  CHECK(!attn_plan(false, 1, 2, 400, 32, false, true).keep && !attn_plan(false, 1, 2, 400, 32, false, true).drop);

  // ---- the other throws: sizes, head dims
  for (int bwd = 0; bwd < 2; ++bwd) {
    for (int bad = 0; bad < 3; ++bad)
      CHECK(has(thrown([&] { attn_plan(bwd, bad == 0 ? 0 : 2, bad == 1 ? 0 : 2, bad == 2 ? 0 : 65, 32, false, false); }),
                "B, H, N >= 1"));
    for (int hd : {0, 16, 48, 96, 128})
      for (int N : {65, 257, 626})  // before the short branch too
        CHECK(thrown([&] { attn_plan(bwd, 2, 2, N, hd, false, false); }) == "attention: head dim must be 32 or 64");
    CHECK(has(thrown([&] { attn_plan(bwd, 1, 2, 129, 32, true, true); }), "attn_keep_words returned 0"));
    CHECK(has(thrown([&] { attn_plan(bwd, 1, 191, 383, 64, true, true); }), "attn_keep_words returned 0"));
    CHECK(thrown([&] { attn_plan(bwd, 1, 2, 129, 32, false, true); }).empty());  // no dropout: the buffer is unused
    CHECK(thrown([&] { attn_plan(bwd, 1, 192, 129, 32, true, true); }).empty());
  }
  for (int hd : {0, 16, 48}) CHECK(attn_keep_words(2, 2, 65, hd) == 0);  // no throw for a bad head dim
  CHECK(attn_keep_words(0, 2, 65, 32) == 0);

  std::printf("attn_plan_check: %d checks passed (%ld plans, %ld listed throws, %d kernels)\n", g_checks, plans,
              thrown_keep, built);
  return 0;
}
