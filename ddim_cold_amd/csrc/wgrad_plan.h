// Host-side plan of the grouped weight-gradient launch (ops.linear_wgrad_multi): the
// tile edge, the cuts into launches of <= WGRAD_MULTI_MAX problems, the K-split tail of
// each launch and the arena ranges the grad-norm tail workgroups sum.  Plain C++ (no HIP,
// no torch): bindings.cpp plans with it, gemm.hip launches from its records, and
// tests/cpp/wgrad_plan_check.cpp checks it on its own.  Every rule is written here once.
#pragma once
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <utility>
#include <vector>

constexpr int BIG_WG_K = 16384;      // tokens: 128 x 128 weight-gradient tiles from here
constexpr int WGRAD_MULTI_MAX = 32;  // problems per launch (kernel-argument block)
constexpr int WGRAD_MAX_SPLIT = 6;   // K pieces per tail tile, at most
constexpr int WSQ_MAX_RANGES = 16;   // arena ranges the grad-norm tail sums, at most
constexpr int WGRAD_TICKETS = 4096;  // ints of the K-split ticket buffer (one per tail tile)

// output tile edge for reductions over kmax tokens (64 x 64 / 4 waves, or 128 x 128 / 8)
inline int wgrad_multi_tile(int64_t kmax) { return kmax >= BIG_WG_K ? 128 : 64; }
inline int64_t wgrad_tiles(int64_t nout, int64_t k, int T) { return ((nout + T - 1) / T) * ((k + T - 1) / T); }
// workgroup slots of one round: one 128 x 128 (128 KiB ring) or three 64 x 64 (48 KiB)
// weight-gradient workgroups per CU
inline int wgrad_slots(int T, int cus) { return (T == 128 ? 1 : 3) * cus; }
// K pieces for the tail tiles of a wide (one workgroup per CU) launch: with W whole rounds
// of C tiles and R tiles left, R x s pieces take ceil(R s / C) / s tile times instead
// of one (profiles/wgrad_split_r6.txt); s = 1 (no split) when nothing is gained
inline int wgrad_split_factor(int tiles, int T, int cus) {
  const int C = wgrad_slots(T, cus), R = tiles % C;
  // 64 x 64 tiles (three workgroups per CU): splitting ViT-tiny's 12-tile tail in 6 pieces
  // measured slower (0.7107 -> 0.7146 ms/step, profiles/wgrad_split_r6.txt) -- wide tiles only
  if (R == 0 || T != 128) return 1;
  int best = 1;
  double bt = 1.0;
  for (int s = 2; s <= WGRAD_MAX_SPLIT; ++s) {
    const double t = (double)((R * s + C - 1) / C) / s;
    if (t < bt - 1e-9) { bt = t; best = s; }
  }
  return best;
}
// floats of the split workspace: per piece a T x T partial tile + T bias partials
inline int64_t wgrad_split_ws_floats(int tiles, int T, int cus) {
  const int s = wgrad_split_factor(tiles, T, cus);
  return s > 1 ? (int64_t)(tiles % wgrad_slots(T, cus)) * s * (T * T + T) : 0;
}

struct WgradShape {
  int64_t nout, k, tokens;
};
// one launch: problems [first, first + count), `tiles` output tiles of which the first
// `whole` run whole and the other R = tiles - whole in `split` K pieces each (`pieces` =
// R (split - 1) workgroups beyond one per tile, `ws_floats` of workspace, R tickets)
struct WgradLaunch {
  int first = 0, count = 0, tiles = 0, split = 1, whole = 0, pieces = 0;
  int64_t ws_floats = 0;
};
struct WgradPlan {
  int T = 64;
  std::vector<WgradLaunch> launches;
};

// Launches of <= WGRAD_MULTI_MAX problems with balanced tile counts (each launch's K-split
// tail then fills its last round; 32 + 18 problems left a 0.9-round launch): cut when the
// cumulative tiles reach the launch's share or the launch is full; plain chunks where that
// cannot stay within the problem limit.
inline WgradPlan wgrad_plan(const std::vector<WgradShape>& shapes, int cus) {
  if (shapes.empty() || cus < 1) throw std::invalid_argument("wgrad_multi: no problems or no compute units");
  const size_t total = shapes.size();
  int64_t kmax = 0;
  for (const WgradShape& s : shapes) kmax = std::max(kmax, s.tokens);
  WgradPlan plan;
  const int T = plan.T = wgrad_multi_tile(kmax);
  std::vector<int64_t> ptiles(total);
  int64_t all_tiles = 0;
  for (size_t i = 0; i < total; ++i) {
    if (shapes[i].nout < 1 || shapes[i].k < 1 || shapes[i].tokens < 1)
      throw std::invalid_argument("wgrad_multi: empty problem");
    all_tiles += ptiles[i] = wgrad_tiles(shapes[i].nout, shapes[i].k, T);
  }
  if (all_tiles >= (int64_t)1 << 30) throw std::invalid_argument("wgrad_multi: too many output tiles");
  const size_t L = (total + WGRAD_MULTI_MAX - 1) / WGRAD_MULTI_MAX;
  std::vector<size_t> cuts{0};
  int64_t cum = 0;
  for (size_t i = 0; i + 1 < total && cuts.size() < L; ++i) {
    cum += ptiles[i];
    const bool full = i + 1 - cuts.back() == (size_t)WGRAD_MULTI_MAX;
    if (full || cum * (int64_t)L >= all_tiles * (int64_t)cuts.size()) cuts.push_back(i + 1);
  }
  cuts.push_back(total);
  bool ok = true;
  for (size_t c = 0; c + 1 < cuts.size(); ++c) ok = ok && cuts[c + 1] - cuts[c] <= (size_t)WGRAD_MULTI_MAX;
  if (!ok) {  // cannot balance within the problem limit: plain chunks
    cuts.clear();
    for (size_t a = 0; a < total; a += WGRAD_MULTI_MAX) cuts.push_back(a);
    cuts.push_back(total);
  }
  for (size_t c = 0; c + 1 < cuts.size(); ++c) {
    WgradLaunch l;
    l.first = (int)cuts[c];
    l.count = (int)(cuts[c + 1] - cuts[c]);
    for (size_t i = cuts[c]; i < cuts[c + 1]; ++i) l.tiles += (int)ptiles[i];
    l.whole = l.tiles;
    l.split = wgrad_split_factor(l.tiles, T, cus);
    if (l.split > 1) {
      const int R = l.tiles % wgrad_slots(T, cus);
      if (R > WGRAD_TICKETS) throw std::invalid_argument("wgrad_multi: more split tiles than tickets");
      l.whole = l.tiles - R;
      l.pieces = R * (l.split - 1);
      l.ws_floats = wgrad_split_ws_floats(l.tiles, T, cus);
    }
    plan.launches.push_back(l);
  }
  return plan;
}

// Grad-norm tail: the ranges of the arena [0, n) that no weight-gradient tile writes
// (`targets`: the dW / db element intervals) and that are not `skipped` (the lazy range:
// zero forever; the embedding and LayerNorm outputs: their workgroups write their own
// partials), and the workgroups that sum their squares (one per 4,096 elements, 1..64).
struct WgradTail {
  std::vector<std::pair<int64_t, int64_t>> ranges;
  int tail = 0;
};
using WgradRanges = std::vector<std::pair<int64_t, int64_t>>;
inline WgradTail wgrad_tail_ranges(WgradRanges targets, const WgradRanges& skipped, int64_t n) {
  for (const auto& [lo, hi] : targets)
    if (lo < 0 || hi < lo || hi > n)
      throw std::invalid_argument("wgrad_multi: a weight-gradient target lies outside the arena");
  std::sort(targets.begin(), targets.end());
  for (size_t i = 1; i < targets.size(); ++i)
    if (targets[i].first < targets[i - 1].second)
      throw std::invalid_argument(
          "wgrad_multi: overlapping weight-gradient targets (the partials would count them twice)");
  for (const auto& [lo, hi] : skipped) {
    if (lo < 0 || hi < lo || hi > n)
      throw std::invalid_argument("wgrad_multi: a lazy, embedding or LayerNorm gradient range lies outside the arena");
    if (hi > lo) targets.emplace_back(lo, hi);
  }
  std::sort(targets.begin(), targets.end());
  WgradTail out;
  int64_t cur = 0, rest = 0;
  auto gap = [&](int64_t lo, int64_t hi) {
    if (hi <= lo) return;
    if ((int)out.ranges.size() == WSQ_MAX_RANGES)
      throw std::invalid_argument("wgrad_multi: more than 16 arena ranges outside the weight gradients");
    out.ranges.emplace_back(lo, hi);
    rest += hi - lo;
  };
  for (const auto& [lo, hi] : targets) {
    gap(cur, lo);
    cur = std::max(cur, hi);
  }
  gap(cur, n);
  out.tail = (int)std::min<int64_t>(64, std::max<int64_t>(1, (rest + 256 * 16 - 1) / (256 * 16)));
  return out;
}
