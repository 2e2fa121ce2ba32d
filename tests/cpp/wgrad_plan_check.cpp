// Stand-alone check of csrc/wgrad_plan.h (the host-side plan of ops.linear_wgrad_multi):
// invariants over a grid of problem lists and CU counts, the error cases, and the values
// the project records for its own workloads at 256 CUs.  tests/test_wgrad_plan_cpu.py
// compiles it with the address and undefined-behaviour sanitizers and runs it.
#include "wgrad_plan.h"

#include <cstdio>
#include <cstdlib>
#include <string>

static int g_checks = 0;
#define CHECK(c)                                                    \
  do {                                                              \
    ++g_checks;                                                     \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

template <class F>
static bool throws_invalid(F f) {
  try {
    f();
  } catch (const std::invalid_argument&) {
    return true;
  }
  return false;
}

using Shapes = std::vector<WgradShape>;

static Shapes cycle(const std::vector<std::pair<int, int>>& dims, int n, int64_t tokens) {
  Shapes s;
  for (int i = 0; i < n; ++i) s.push_back({dims[i % dims.size()].first, dims[i % dims.size()].second, tokens});
  return s;
}

// launches tile [0, n) in order, each within the problem limit; the split fields agree
static void check_plan(const Shapes& shapes, int cus) {
  const WgradPlan p = wgrad_plan(shapes, cus);
  int64_t kmax = 0;
  for (const WgradShape& s : shapes) kmax = std::max(kmax, s.tokens);
  const int T = p.T;
  CHECK(T == (kmax >= 16384 ? 128 : 64));
  CHECK(p.launches.size() >= (shapes.size() + 31) / 32);
  int next = 0;
  for (const WgradLaunch& l : p.launches) {
    CHECK(l.first == next && l.count >= 1 && l.count <= 32);
    next += l.count;
    int64_t tiles = 0;
    for (int i = l.first; i < l.first + l.count; ++i)
      tiles += ((shapes[i].nout + T - 1) / T) * ((shapes[i].k + T - 1) / T);
    CHECK(l.tiles == tiles);
    const int R = l.tiles - l.whole;
    CHECK(l.split >= 1 && l.split <= 6 && l.whole >= 0 && R >= 0);
    CHECK(l.pieces == R * (l.split - 1));
    CHECK(l.ws_floats == (l.split > 1 ? (int64_t)R * l.split * (T * T + T) : 0));
    CHECK(l.split == wgrad_split_factor(l.tiles, T, cus));
    if (l.split > 1) {
      CHECK(T == 128 && R == l.tiles % cus && R > 0 && R <= WGRAD_TICKETS);
      // the split pays: its pieces take fewer tile times than the unsplit tail's one
      CHECK((R * l.split + cus - 1) / cus < l.split);
    } else {
      CHECK(R == 0);
    }
    CHECK(l.ws_floats == wgrad_split_ws_floats(l.tiles, T, cus));
  }
  CHECK(next == (int)shapes.size());
}

// ranges + targets + skipped cover [0, n) exactly once
static void check_cover(const WgradRanges& targets, const WgradRanges& skipped, int64_t n) {
  const WgradTail t = wgrad_tail_ranges(targets, skipped, n);
  CHECK((int)t.ranges.size() <= WSQ_MAX_RANGES);
  std::vector<int> cnt(n, 0);
  int64_t rest = 0;
  for (const WgradRanges* rs : {&targets, &skipped, &t.ranges})
    for (const auto& [lo, hi] : *rs) {
      CHECK(lo >= 0 && hi >= lo && hi <= n);
      for (int64_t i = lo; i < hi; ++i) ++cnt[i];
    }
  for (int64_t i = 0; i < n; ++i) CHECK(cnt[i] == 1);
  for (size_t i = 0; i < t.ranges.size(); ++i) {
    CHECK(t.ranges[i].second > t.ranges[i].first);
    CHECK(i == 0 || t.ranges[i].first > t.ranges[i - 1].second);  // ascending, never adjacent
    rest += t.ranges[i].second - t.ranges[i].first;
  }
  CHECK(t.tail == (int)std::min<int64_t>(64, std::max<int64_t>(1, (rest + 4095) / 4096)));
}

// k targets of 10 elements with a gap of 5 before each and after the last: k + 1 gaps
static WgradRanges spaced(int k) {
  WgradRanges r;
  for (int i = 0; i < k; ++i) r.emplace_back(5 + 15 * i, 15 + 15 * i);
  return r;
}

int main() {
  const std::vector<std::pair<int, int>> block{{1152, 384}, {384, 384}, {384, 384}, {384, 384}};
  const std::vector<std::pair<int, int>> mixed{{1152, 384}, {384, 384}, {384, 384}, {384, 384},
                                               {192, 384},  {384, 192}, {64, 96},   {256, 128}};
  const std::vector<std::pair<int, int>> small{{8, 8}, {72, 192}, {64, 64}, {136, 8}};

  // ---- invariants over a grid
  for (int cus : {1, 7, 64, 256, 304})
    for (int64_t tokens : {8, 520, 16383, 16384, 20032})
      for (const auto* dims : {&block, &mixed, &small})
        for (int n : {1, 2, 5, 17, 31, 32, 33, 36, 64, 65, 97})
          check_plan(cycle(*dims, n, tokens), cus);
  {  // one huge problem in front: the balanced cut would leave > 32 in the second launch -> plain chunks
    Shapes s{{8192, 8192, 64}};
    for (int i = 0; i < 40; ++i) s.push_back({8, 8, 64});
    check_plan(s, 256);
    const WgradPlan p = wgrad_plan(s, 256);
    CHECK(p.launches.size() == 2 && p.launches[0].count == 32 && p.launches[1].count == 9);
    // mixed token counts: the longest reduction decides the tile of every launch
    s.back().tokens = 16384;
    CHECK(wgrad_plan(s, 256).T == 128);
    check_plan(s, 256);
  }
  CHECK(throws_invalid([] { wgrad_plan({}, 256); }));
  CHECK(throws_invalid([] { wgrad_plan({{8, 8, 8}}, 0); }));
  CHECK(throws_invalid([] { wgrad_plan({{8, 0, 8}}, 256); }));

  // ---- recorded values, 256 CUs
  {  // vit_small_200, a 6-block half: one whole round + 68 tiles in 3 K pieces
    const WgradPlan p = wgrad_plan(cycle(block, 24, 20032), 256);
    CHECK(p.T == 128 && p.launches.size() == 1);
    const WgradLaunch& l = p.launches[0];
    CHECK(l.first == 0 && l.count == 24 && l.tiles == 324 && l.whole == 256 && l.tiles - l.whole == 68 && l.split == 3);
    CHECK(l.pieces == 136 && l.ws_floats == (int64_t)68 * 3 * (128 * 128 + 128));
  }
  {  // gemm_check.WGRAD_BIG_SHAPES at 16,392 tokens: 10 tiles, all in the split tail
    const WgradPlan p = wgrad_plan({{192, 192, 16392}, {192, 136, 16392}, {72, 192, 16392}}, 256);
    CHECK(p.T == 128 && p.launches.size() == 1);
    const WgradLaunch& l = p.launches[0];
    CHECK(l.tiles == 10 && l.whole == 0 && l.split == 6 && l.pieces == 50);
  }
  for (int64_t tokens : {16384, 16500, 20032}) {  // test_linear_wgrad_multi, 5 and 36 problems
    const WgradPlan p5 = wgrad_plan(cycle(mixed, 5, tokens), 256);
    CHECK(p5.T == 128 && p5.launches.size() == 1 && p5.launches[0].tiles == 60 && p5.launches[0].split == 4);
    const WgradPlan p36 = wgrad_plan(cycle(mixed, 36, tokens), 256);
    CHECK(p36.launches.size() == 2);
    CHECK(p36.launches[0].first == 0 && p36.launches[0].count == 17 && p36.launches[1].first == 17 &&
          p36.launches[1].count == 19);
    for (const WgradLaunch& l : p36.launches) CHECK(l.tiles == 165 && l.split == 3);
  }
  for (int tiles = 1; tiles <= 2000; ++tiles) {  // under the threshold: 64 x 64 tiles, never split
    CHECK(wgrad_multi_tile(16383) == 64 && wgrad_split_factor(tiles, 64, 256) == 1);
    CHECK(wgrad_split_ws_floats(tiles, 64, 256) == 0);
  }
  CHECK(wgrad_multi_tile(16384) == 128 && wgrad_slots(128, 256) == 256 && wgrad_slots(64, 256) == 768);
  {  // ViT-tiny's 30 problems at 520 tokens
    Shapes s = cycle(block, 28, 520);
    s.push_back({192, 384, 520});
    s.push_back({384, 192, 520});
    const WgradPlan p = wgrad_plan(s, 256);
    CHECK(p.T == 64 && p.launches.size() == 1);
    CHECK(p.launches[0].tiles == 1548 && p.launches[0].split == 1 && p.launches[0].whole == 1548);
  }

  // ---- grad-norm tail ranges
  check_cover({}, {}, 100);
  check_cover({{0, 100}}, {}, 100);
  check_cover({{10, 20}, {20, 30}, {50, 100}}, {}, 100);
  check_cover({{50, 100}, {10, 20}}, {{0, 5}, {30, 40}, {40, 40}}, 100);
  check_cover(spaced(15), {}, 15 * 15 + 5);          // 16 gaps: the most the kernel takes
  check_cover(spaced(16), {{0, 5}}, 16 * 15 + 5);    // 17 gaps, one of them skipped
  check_cover({{4096, 8192}}, {{0, 64}}, 64 * 4096 * 2);  // more than 64 x 4,096 elements: 64 workgroups
  CHECK(wgrad_tail_ranges({}, {}, 64 * 4096 * 2).tail == 64);
  CHECK(wgrad_tail_ranges({}, {}, 4097).tail == 2 && wgrad_tail_ranges({{0, 8}}, {}, 8).tail == 1);
  CHECK(throws_invalid([] { wgrad_tail_ranges(spaced(16), {}, 16 * 15 + 5); }));        // 17 gaps
  CHECK(throws_invalid([] { wgrad_tail_ranges({{10, 20}, {19, 30}}, {}, 100); }));       // overlapping targets
  CHECK(throws_invalid([] { wgrad_tail_ranges({{10, 20}, {10, 20}}, {}, 100); }));
  CHECK(throws_invalid([] { wgrad_tail_ranges({{90, 101}}, {}, 100); }));                // outside the arena
  CHECK(throws_invalid([] { wgrad_tail_ranges({{-1, 10}}, {}, 100); }));
  CHECK(throws_invalid([] { wgrad_tail_ranges({}, {{120, 130}}, 100); }));               // a skipped range too
  try {
    wgrad_tail_ranges({{90, 101}}, {}, 100);
  } catch (const std::invalid_argument& e) {
    CHECK(std::string(e.what()).find("outside the arena") != std::string::npos);
  }

  std::printf("wgrad_plan_check: %d checks passed\n", g_checks);
  return 0;
}
