// Host-side plan of the attention launches (attn_fwd_launch, attn_bwd_launch): which of the
// four forwards a problem takes -- and with it the layout of the keep words the forward
// stores for the backward -- the kernel instantiation, its grid, block and dynamic LDS.
// Plain C++ (no HIP, no torch): attention.hip launches from the plan and instantiates its
// kernels against attn_kernel_built, torch.ops.ddim_cold.attn_plan reports the same plan,
// and tests/cpp/attn_plan_check.cpp checks it on its own.  Every rule is written here once.
#pragma once
#include <cstdint>
#include <stdexcept>

constexpr int ATTN_HD_SMALL = 32, ATTN_HD_BIG = 64;  // the head dims with kernels
constexpr int ATTN_SHORT_MAX_N = 128;      // up to here: one workgroup per head holds the whole sequence
constexpr int ATTN_RESIDENT_MAX_N = 320;   // up to here, with enough heads: the resident-KV forward
constexpr int ATTN_RESIDENT_MIN_BH = 192;  // ... "enough": B*H from here
constexpr int ATTN_FLASH2_MIN_N = 384;     // from here: flash v2 (128 queries per workgroup)
constexpr int ATTN_LDS_BUDGET = 160 * 1024;  // LDS of one CU
constexpr int ATTN_LDS_DEFAULT = 64 * 1024;  // dynamic LDS a kernel may ask for without raising its limit

// The forward a problem takes.  The backward of a SHORT problem is the one short kernel;
// every other path shares the dQ and dK/dV kernels.
enum class AttnPath : int { SHORT = 0, V1 = 1, RESIDENT = 2, FLASH2 = 3 };

// One workgroup per head (RESIDENT) needs about a workgroup per CU to pay off.  Measured
// N=257 hd=64: B*H=256 20.1 vs 31.9 us (one 64-query workgroup per tile); B*H=128 equal
// without dropout, 27 vs 22 with.  Flash v2 has half the workgroups of v1: measured better
// from ~600 tokens (N=626: 63 vs 71 us without dropout), worse at N=257 with dropout (25
// vs 22 us).
constexpr AttnPath attn_path(long long bh, int N) {
  if (N <= ATTN_SHORT_MAX_N) return AttnPath::SHORT;
  if (N <= ATTN_RESIDENT_MAX_N && bh >= ATTN_RESIDENT_MIN_BH) return AttnPath::RESIDENT;
  if (N >= ATTN_FLASH2_MIN_N) return AttnPath::FLASH2;
  return AttnPath::V1;
}

// LDS layout, in bytes.  Every K / V / Q / dO row image is padded by 32 B (conflict-free
// row reads and transposed reads); the short backward's [query][key] P / dS images
// likewise.  The kernels' strides are static_asserted against these.
constexpr int attn_row_stride(int hd) { return 2 * hd + 32; }
constexpr int attn_short_np(int N) { return 32 * ((N + 31) / 32); }  // padded rows of the short path
constexpr int attn_short_pimg_stride(int np) { return 2 * np + 32; }
constexpr int attn_short_fwd_lds(int hd, int np) { return 2 * np * attn_row_stride(hd); }  // K, V
constexpr int attn_short_bwd_lds(int hd, int np) {  // Q, K, V, dO; P, dS
  return 4 * np * attn_row_stride(hd) + 2 * np * attn_short_pimg_stride(np);
}
constexpr int attn_resident_lds(int hd, int N) { return 2 * (64 * ((N + 63) / 64)) * attn_row_stride(hd); }  // K, V

// The kernel templates of attention.hip and the template arguments each takes (next to
// the head dim): BWD_DQ and BWD_DKV run one after the other in every long backward.
enum class AttnKernel : int { FWD_V1 = 0, FWD_FLASH2, FWD_RESIDENT, FWD_SHORT, BWD_DQ, BWD_DKV, BWD_SHORT };
constexpr int ATTN_KERNEL_TEMPLATES = 7;
constexpr bool attn_kernel_takes_np(AttnKernel k) { return k == AttnKernel::FWD_SHORT || k == AttnKernel::BWD_SHORT; }
constexpr bool attn_kernel_takes_drop(AttnKernel k) {
  return k == AttnKernel::FWD_FLASH2 || k == AttnKernel::FWD_RESIDENT || attn_kernel_takes_np(k);
}
constexpr bool attn_kernel_takes_keep(AttnKernel k) {  // a stored-flag variant of its own
  return k == AttnKernel::BWD_DQ || k == AttnKernel::BWD_DKV || k == AttnKernel::BWD_SHORT;
}

// Which instantiations exist (attention.hip instantiates exactly these and no launch names
// another).  An argument a template does not take is 0 / false.
constexpr bool attn_kernel_built(AttnKernel k, int hd, int np, bool drop, bool keep) {
  if ((int)k < 0 || (int)k >= ATTN_KERNEL_TEMPLATES || (hd != ATTN_HD_SMALL && hd != ATTN_HD_BIG)) return false;
  if (attn_kernel_takes_np(k) ? np < 32 || np > ATTN_SHORT_MAX_N || np % 32 != 0 : np != 0) return false;
  if (drop && !attn_kernel_takes_drop(k)) return false;
  if (keep && !attn_kernel_takes_keep(k)) return false;
  return !(k == AttnKernel::BWD_SHORT && keep && !drop);  // stored flags exist only with dropout
}
// how many that is (attention.hip's kernel list is checked against it): 2 v1, 4 flash v2,
// 4 resident, 16 short forward, 4 + 4 long backward, 24 short backward
constexpr int attn_kernels_built() {
  int n = 0;
  for (int k = 0; k < ATTN_KERNEL_TEMPLATES; ++k)
    for (int hd = 0; hd <= 128; hd += 32)
      for (int np = 0; np <= 160; np += 32)
        for (int f = 0; f < 4; ++f) n += attn_kernel_built((AttnKernel)k, hd, np, f & 1, f & 2);
  return n;
}

// What a launch gets.  keep: the stored-flag variant runs (the forward writes its dropout
// keep flags, the backward reads them instead of re-hashing).  keep_words: the int32 words
// a keep buffer of this problem holds, whatever drop and keep are -- 4 per padded row of
// the short path (one per lane), one 64-bit word per (query, 64-key tile) of the resident
// and flash v2 forwards, none for the v1 forward, which stores no flags.
struct AttnPlan {
  AttnPath path = AttnPath::SHORT;
  AttnKernel kernel = AttnKernel::FWD_SHORT;  // the long backward: BWD_DQ, then BWD_DKV with the same arguments
  int hd = 0;
  int np = 0;  // SHORT: rows padded to 32; else 0
  bool drop = false, keep = false;
  int grid_x = 0, grid_y = 0, block = 0;
  int lds = 0;  // dynamic LDS bytes (the other kernels' LDS is static)
  int64_t keep_words = 0;
};

// the template arguments of kernel k in a launch of plan pl
struct AttnKernelArgs {
  int hd, np;
  bool drop, keep;
};
constexpr AttnKernelArgs attn_kernel_args(AttnKernel k, const AttnPlan& pl) {
  return {pl.hd, attn_kernel_takes_np(k) ? pl.np : 0, attn_kernel_takes_drop(k) && pl.drop,
          attn_kernel_takes_keep(k) && pl.keep};
}

// The one place that turns a problem into a launch.  drop: the dropout threshold of p is
// not 0 (drop_threshold_host; a tiny p > 0 rounds to threshold 0 and runs the no-dropout
// kernels).  have_keep: the caller hands a keep buffer.  Throws on sizes < 1, on a head dim
// without kernels, and where stored flags are asked of the v1 forward's shapes.
inline AttnPlan attn_plan(bool bwd, int B, int H, int N, int hd, bool drop, bool have_keep) {
  if (B < 1 || H < 1 || N < 1) throw std::runtime_error("attn_plan: B, H, N >= 1");
  if (hd != ATTN_HD_SMALL && hd != ATTN_HD_BIG) throw std::runtime_error("attention: head dim must be 32 or 64");
  const long long bh = (long long)B * H;
  AttnPlan pl;
  pl.path = attn_path(bh, N);
  pl.hd = hd;
  pl.drop = drop;
  pl.keep = drop && have_keep;
  if (pl.path == AttnPath::V1 && pl.keep)
    throw std::runtime_error("attention: no stored keep masks on this path (attn_keep_words returned 0)");
  pl.grid_x = (int)bh;
  pl.grid_y = 1;
  pl.block = 256;
  if (pl.path == AttnPath::SHORT) {
    pl.kernel = bwd ? AttnKernel::BWD_SHORT : AttnKernel::FWD_SHORT;
    pl.np = attn_short_np(N);
    pl.block = 4 * pl.np;  // one wave per 16 rows
    pl.lds = bwd ? attn_short_bwd_lds(hd, pl.np) : attn_short_fwd_lds(hd, pl.np);
    pl.keep_words = bh * pl.np * 4;
    return pl;
  }
  pl.keep_words = pl.path == AttnPath::V1 ? 0 : bh * N * ((N + 63) / 64) * 2;
  if (!bwd && pl.path == AttnPath::RESIDENT) {
    pl.kernel = AttnKernel::FWD_RESIDENT;
    pl.block = 64 * ((N + 31) / 32);  // one wave per 32 queries
    pl.lds = attn_resident_lds(hd, N);
    return pl;
  }
  // a workgroup per 64 queries (v1, dQ) or keys (dK/dV), per 128 queries (flash v2)
  const bool flash2 = !bwd && pl.path == AttnPath::FLASH2;
  pl.kernel = bwd ? AttnKernel::BWD_DQ : flash2 ? AttnKernel::FWD_FLASH2 : AttnKernel::FWD_V1;
  pl.grid_x = flash2 ? (N + 127) / 128 : (N + 63) / 64;
  pl.grid_y = (int)bh;
  return pl;
}

// int32 words of the keep buffer a forward of this shape fills (0: none, the v1 forward; or
// no kernels for this shape at all)
inline int64_t attn_keep_words(int B, int H, int N, int hd) {
  if (B < 1 || H < 1 || N < 1 || (hd != ATTN_HD_SMALL && hd != ATTN_HD_BIG)) return 0;
  return attn_plan(false, B, H, N, hd, false, false).keep_words;
}
