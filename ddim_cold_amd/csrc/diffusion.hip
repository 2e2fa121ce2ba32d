// Diffusion-math and on-GPU data kernels.
//
//  * ddim_step: clamp(x0_hat) + eps_hat + DDIM jump in ONE fp32 pass
//        x0 = clamp(f(x_t,t), -1, 1); eps = (x_t - sqrt(a_t) x0)/sqrt(1-a_t)
//        x_{t-k} = sqrt(a_{t-k}) x0 + sqrt(1-a_{t-k}) eps
//    (algebraically the update of ViT.py:229-234).  The 4 coefficients come
//    from a device table so a captured sampler graph has no host scalars.
//  * randn: counter-based normal (Box-Muller over the dropout hash), graph-safe.
//  * q_sample: sqrt(a_t) x0 + sqrt(1-a_t) eps, a_t = 1 - sqrt((t+1)/T)
//    (diffusion_loader.py:50-54), per-sample t.
//  * pixelate_pair / cold_batch: the cold degradation of diffusion_loader.py:79-97
//    (NEAREST down to floor(W/2^t), NEAREST back up) for (t, t-1) in one pass;
//    cold_batch also draws the batch (pool index, t in 1..max_t) on device.
//  * cold_step / repaint_rows: the per-step launches of the cold x0 sampler and of inpainting
//    (paste the kept region at the step's noise level, jump back for a resample), in place
//    on the sampler state.
//  * dpm2m_rows: the per-step launch of the DPM-Solver++(2M) sampler (the DDIM update plus
//    one term from the previous step's x0-hat), in place on the patch-row state.
#include "common.h"
#include "kernels.h"

namespace dc {

__global__ __launch_bounds__(256) void ddim_step_kernel(const float* __restrict__ xt, const float* __restrict__ x0r,
                                                        float* __restrict__ xn, float* __restrict__ x0o,
                                                        const float* __restrict__ coef, int64_t n) {
  const float sa = coef[0], s1a = coef[1], sak = coef[2], s1ak = coef[3];
  const float inv = 1.f / s1a;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float x0 = fminf(fmaxf(x0r[i], -1.f), 1.f);
    const float eps = (xt[i] - sa * x0) * inv;
    if (x0o) x0o[i] = x0;
    xn[i] = sak * x0 + s1ak * eps;
  }
}

__device__ __forceinline__ float u01(uint32_t h) { return ((float)(h >> 8) + 0.5f) * (1.0f / 16777216.0f); }

__global__ __launch_bounds__(256) void randn_kernel(float* __restrict__ out, int64_t n, const int64_t* __restrict__ rng,
                                                    int site) {
  const uint32_t salt = site_salt(rng, site);
  const int64_t pairs = (n + 1) / 2;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < pairs; i += (int64_t)gridDim.x * 256) {
    const float a = u01(mix32(((uint32_t)(2 * i) * 0x9E3779B1u) ^ salt));
    const float b = u01(mix32(((uint32_t)(2 * i + 1) * 0x9E3779B1u) ^ salt));
    const float r = sqrtf(-2.f * __logf(a));
    float s, c;
    __sincosf(6.283185307179586f * b, &s, &c);
    out[2 * i] = r * c;
    if (2 * i + 1 < n) out[2 * i + 1] = r * s;
  }
}

__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x0, const int64_t* __restrict__ t,
                                                       const float* __restrict__ eps, float* __restrict__ out, int B,
                                                       int64_t per, int T) {
  const int64_t n = (int64_t)B * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int b = (int)(i / per);
    const float a = (float)(1.0 - sqrt(((double)t[b] + 1.0) / (double)T));
    out[i] = sqrtf(a) * x0[i] + sqrtf(1.f - a) * eps[i];
  }
}


__global__ __launch_bounds__(256) void pixelate_pair_kernel(const float* __restrict__ img, const int64_t* __restrict__ idx,
                                                            const int64_t* __restrict__ t, float* __restrict__ xt,
                                                            float* __restrict__ xtm1, int B, int C, int H, int W) {
  const int64_t n = (int64_t)B * C * H * W;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int x = (int)(e % W);
    int64_t r = e / W;
    const int y = (int)(r % H);
    r /= H;
    const int c = (int)(r % C);
    const int b = (int)(r / C);
    const int64_t src = idx ? idx[b] : b;
    const int tt = (int)t[b];
    const float* im = img + ((size_t)src * C + c) * H * W;
    const int f1 = 1 << tt, f0 = 1 << (tt - 1);
    xt[e] = im[(size_t)pix_src(y, H, f1) * W + pix_src(x, W, f1)];
    xtm1[e] = im[(size_t)pix_src(y, H, f0) * W + pix_src(x, W, f0)];
  }
}

// The batch draw + pixelate_pair in ONE launch: every element recomputes its sample's
// (pool index, t) from the counter hash (cold_draw_idx / cold_draw_t: two mix32, cheaper
// than a dependent launch); the first element of each sample also stores them for the model.
__global__ __launch_bounds__(256) void cold_batch_kernel(const float* __restrict__ pool, int pool_n,
                                                         const int64_t* __restrict__ rng, int site, int max_t,
                                                         int64_t* __restrict__ idx, int64_t* __restrict__ t,
                                                         int draw_idx, float* __restrict__ xt, float* __restrict__ xtm1,
                                                         int B, int C, int H, int W, const int64_t* __restrict__ idx_ctr,
                                                         int idx_rows, int idx_stride) {
  const uint32_t salt = site_salt(rng, site);
  if (idx_ctr) idx += (idx_ctr[0] % idx_rows) * idx_stride;  // stepped index table row
  const int64_t per = (int64_t)C * H * W;
  const int64_t n = (int64_t)B * per;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const int b = (int)(e / per);
    const int64_t rem = e - (int64_t)b * per;
    const int64_t src = draw_idx ? (int64_t)(uint32_t)cold_draw_idx(salt, b, pool_n) : idx[b];  // (never negative)
    const int tt = cold_draw_t(salt, b, max_t);
    if (rem == 0) {
      if (draw_idx) idx[b] = src;
      t[b] = tt;
    }
    const int x = (int)(rem % W);
    const int64_t r = rem / W;
    const int y = (int)(r % H);
    const int c = (int)(r / H);
    const float* im = pool + ((size_t)src * C + c) * H * W;
    const int f1 = 1 << tt, f0 = 1 << (tt - 1);
    xt[e] = im[(size_t)pix_src(y, H, f1) * W + pix_src(x, W, f1)];
    xtm1[e] = im[(size_t)pix_src(y, H, f0) * W + pix_src(x, W, f0)];
  }
}

// Gaussian DDIM batch in ONE launch (GaussianBatcher; diffusion_loader.py:24-58):
// pool index + t ~ U{0..T-1} per sample from the data site's hash, eps from the
// noise site, x_t = q_sample(x0, t, eps); the fused patch-embed path derives the
// same values (embed.hip).
__global__ __launch_bounds__(256) void gauss_batch_kernel(const float* __restrict__ pool, int pool_n,
                                                          const int64_t* __restrict__ rng, int site, int noise_site,
                                                          int T, int64_t* __restrict__ idx, int64_t* __restrict__ t,
                                                          int draw_idx, float* __restrict__ xt, float* __restrict__ x0o,
                                                          int B, int per, const int64_t* __restrict__ idx_ctr,
                                                          int idx_rows, int idx_stride) {
  const uint32_t salt = site_salt(rng, site), nsalt = site_salt(rng, noise_site);
  if (idx_ctr) idx += (idx_ctr[0] % idx_rows) * idx_stride;  // stepped index table row
  const int n = B * per;
  for (int e = blockIdx.x * 256 + threadIdx.x; e < n; e += gridDim.x * 256) {
    const int b = e / per, rem = e - b * per;
    const int src = draw_idx ? cold_draw_idx(salt, b, pool_n) : (int)idx[b];
    const int tt = gauss_draw_t(salt, b, T);
    if (rem == 0) {
      if (draw_idx) idx[b] = src;
      t[b] = tt;
    }
    float sa, s1a;
    gauss_coef(tt, T, sa, s1a);
    const float x0 = pool[(size_t)src * per + rem];
    x0o[e] = x0;
    xt[e] = sa * x0 + s1a * gauss_eps(nsalt, (uint32_t)e);
  }
}

// Cold-diffusion sampling step for an x0-predicting model (Bansal et al. 2022), in
// place on x, with x0 the clamped prediction and D(., t) = the training degradation
// (pix_src for factor 2^t):
//   algorithm 1: x <- D(x0, t-1)                 algorithm 2: x <- (x - D(x0, t)) + D(x0, t-1)
// Per-sample t from the device; a sample with t <= 0 is skipped (no load, no store).
// ROWS = false: x / x0 are [B,C,H,W]; pout (optional) gets the new x as bf16
// conv-im2col patch rows [B*P][C*p*p] (column c*p*p + a*p + b), p = patch (0: no pout).
// ROWS = true: x / x0 / pout are [B*P][F] patch rows in the head's output column order
// (column (a*p + b)*C + c): element -> pixel (y, x, c) -> the two source pixels ->
// their (row, column) in x0 (other rows once the block outgrows the patch).
// Each thread owns 4 consecutive elements (one sample: C*H*W % 4 == 0): a 16-byte
// load and store of x, scalar gathers from x0, an 8-byte bf16 store.
template <bool ROWS>
__global__ __launch_bounds__(256) void cold_step_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                                        const int64_t* __restrict__ t, bf16* __restrict__ pout,
                                                        int B, int C, int H, int W, int p, int alg) {
  const int per = C * H * W, n4 = B * (per / 4);
  const int Wp = p > 0 ? W / p : 0, F = C * p * p;
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += gridDim.x * 256) {
    const int e = 4 * q, b = e / per, rem0 = e - b * per;
    const int64_t tb = t[b];
    if (tb <= 0) continue;
    const int tt = tb < 30 ? (int)tb : 30;  // (2^t beyond the image: one block, as pix_src clamps)
    const int f1 = 1 << tt, f0 = 1 << (tt - 1);
    const float* s = x0 + (size_t)b * per;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (alg == 2) v = *reinterpret_cast<const f32x4*>(x + e);
    int po[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int rem = rem0 + j;
      int c, yy, xx;
      if (ROWS) {
        const int row = rem / F, col = rem - row * F, ab = col / C, a = ab / p;
        c = col - ab * C;
        yy = (row / Wp) * p + a;
        xx = (row % Wp) * p + (ab - a * p);
      } else {
        const int r = rem / W;
        xx = rem - r * W;
        c = r / H;
        yy = r - c * H;
      }
      const int y1 = pix_src(yy, H, f1), x1 = pix_src(xx, W, f1);
      const int y0 = pix_src(yy, H, f0), x0s = pix_src(xx, W, f0);
      float a1, a0;
      if (ROWS) {
        a1 = s[((y1 / p) * Wp + x1 / p) * F + ((y1 % p) * p + x1 % p) * C + c];
        a0 = s[((y0 / p) * Wp + x0s / p) * F + ((y0 % p) * p + x0s % p) * C + c];
        po[j] = rem;
      } else {
        a1 = s[(c * H + y1) * W + x1];
        a0 = s[(c * H + y0) * W + x0s];
        po[j] = p > 0 ? ((yy / p) * Wp + xx / p) * F + c * p * p + (yy % p) * p + xx % p : 0;
      }
      v[j] = alg == 2 ? (v[j] - a1) + a0 : a0;
    }
    *reinterpret_cast<f32x4*>(x + e) = v;
    if (pout != nullptr) {
      bf16* o = pout + (size_t)b * per;
      if (ROWS || p % 4 == 0) {  // 4 consecutive pixels of one patch line: consecutive columns
        bf16x4 h;
        h[0] = f2bf(v[0]); h[1] = f2bf(v[1]); h[2] = f2bf(v[2]); h[3] = f2bf(v[3]);
        *reinterpret_cast<bf16x4*>(o + po[0]) = h;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[po[j]] = f2bf(v[j]);
      }
    }
  }
}

// Mask step of inpainting (RePaint, Lugmayr et al. 2022), in place on the sampler's fp32
// patch-row state x, after the forward whose head epilogue stepped it.  Per element e
//   y   = mask[e] ? fma(kb, z1[e], rounded(ka known[e])) : x[e]      (paste: known noised to the step's level)
//   out = (ra == 1 && rb == 0) ? y : fma(rb, z2[e], rounded(ra y))   (jump: diffuse forward again)
// coef = {ka, kb, ra, rb} from device memory (a captured loop has no host scalars); z1 / z2 =
// element e of randn_kernel's draw over x at (rng, site_paste) / (rng, site_jump), by gauss_pair.
// Each thread owns 4 consecutive elements: one 4-byte mask load, 16-byte loads of x / known,
// a 16-byte store of x and an 8-byte store of its bf16 rows (pout, optional).  A paste-only
// call (wave-uniform on the loaded coefficients) stores nothing for a 4-vector whose mask bytes
// are all zero, draws z1 only for a pair with a mask byte set and never z2; a jump writes
// every element.  n4 = elements / 4 (elements < 2^31).
__global__ __launch_bounds__(256) void repaint_rows_kernel(float* __restrict__ x, const float* __restrict__ known,
                                                           const uint8_t* __restrict__ mask,
                                                           const float* __restrict__ coef,
                                                           const int64_t* __restrict__ rng, int site_paste,
                                                           int site_jump, bf16* __restrict__ pout, int n4) {
  const float ka = coef[0], kb = coef[1], ra = coef[2], rb = coef[3];
  const bool paste_only = ra == 1.f && rb == 0.f;
  const uint32_t salt_p = site_salt(rng, site_paste), salt_j = site_salt(rng, site_jump);
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += gridDim.x * 256) {
    const int e = 4 * q;
    const uint32_t m = *reinterpret_cast<const uint32_t*>(mask + e);
    if (paste_only && m == 0u) continue;
    f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
    if (m != 0u) {
      const f32x4 kn = *reinterpret_cast<const f32x4*>(known + e);
      float2 z01 = make_float2(0.f, 0.f), z23 = z01;
      if (m & 0x0000FFFFu) z01 = gauss_pair(salt_p, (uint32_t)e);
      if (m & 0xFFFF0000u) z23 = gauss_pair(salt_p, (uint32_t)e + 2u);
      const float z[4] = {z01.x, z01.y, z23.x, z23.y};
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((m >> (8 * j)) & 0xFFu) v[j] = __builtin_fmaf(kb, z[j], rounded(ka * kn[j]));
    }
    if (!paste_only) {
      const float2 z01 = gauss_pair(salt_j, (uint32_t)e), z23 = gauss_pair(salt_j, (uint32_t)e + 2u);
      v[0] = __builtin_fmaf(rb, z01.x, rounded(ra * v[0]));
      v[1] = __builtin_fmaf(rb, z01.y, rounded(ra * v[1]));
      v[2] = __builtin_fmaf(rb, z23.x, rounded(ra * v[2]));
      v[3] = __builtin_fmaf(rb, z23.y, rounded(ra * v[3]));
    }
    *reinterpret_cast<f32x4*>(x + e) = v;
    if (pout != nullptr) {
      bf16x4 h;
      h[0] = f2bf(v[0]); h[1] = f2bf(v[1]); h[2] = f2bf(v[2]); h[3] = f2bf(v[3]);
      *reinterpret_cast<bf16x4*>(pout + e) = h;
    }
  }
}

// DPM-Solver++(2M) step (Lu et al. 2022) of an x0-predicting model, in place on the sampler's
// fp32 patch-row state x, after the forward that wrote the clamped x0-hat (HEAD_CLAMP) into x0;
// x0p is the previous step's x0-hat.  Per element, every rounding as written:
//   de  = rounded(c3 * (fma(-c0, x0, x) / c1))
//   det = fma(c2, x0, de)                                   (the DDIM step)
//   out = g == 0 ? det : fma(g, rounded(x0 - x0p), det)     (the second-order term)
// coef = rows {c0, c1, c2, c3, g, 0, 0, 0} from device memory (schedule.dpm2m_row; a captured
// loop has no host scalars): one row (each = 0), or one per sample [B][8] (each = 1), the sample
// of 4-vector q being q / per4 (per4 = elements per sample / 4, so a thread's 4 elements share
// one row).  A row with g == 0 never loads x0p (wave-uniform for each = 0, a branch on the
// thread's row otherwise): a sample's first step has no history to read.  Each thread owns 4
// consecutive elements: 16-byte loads of x / x0 / x0p, a 16-byte store of x and an 8-byte
// store of its bf16 rows (pout, optional).  n4 = elements / 4 (elements < 2^31).
__global__ __launch_bounds__(256) void dpm2m_rows_kernel(float* __restrict__ x, const float* __restrict__ x0,
                                                         const float* __restrict__ x0p,
                                                         const float* __restrict__ coef, int each, int per4,
                                                         bf16* __restrict__ pout, int n4) {
  float c0 = coef[0], c1 = coef[1], c2 = coef[2], c3 = coef[3], g = coef[4];
  for (int q = blockIdx.x * 256 + threadIdx.x; q < n4; q += gridDim.x * 256) {
    const int e = 4 * q;
    if (each) {
      const float* cf = coef + (q / per4) * 8;
      c0 = cf[0]; c1 = cf[1]; c2 = cf[2]; c3 = cf[3]; g = cf[4];
    }
    f32x4 v = *reinterpret_cast<const f32x4*>(x + e);
    const f32x4 p = *reinterpret_cast<const f32x4*>(x0 + e);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float de = rounded(c3 * (__builtin_fmaf(-c0, p[j], v[j]) / c1));
      v[j] = __builtin_fmaf(c2, p[j], de);
    }
    if (g != 0.f) {
      const f32x4 pp = *reinterpret_cast<const f32x4*>(x0p + e);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = __builtin_fmaf(g, rounded(p[j] - pp[j]), v[j]);
    }
    *reinterpret_cast<f32x4*>(x + e) = v;
    if (pout != nullptr) {
      bf16x4 h;
      h[0] = f2bf(v[0]); h[1] = f2bf(v[1]); h[2] = f2bf(v[2]); h[3] = f2bf(v[3]);
      *reinterpret_cast<bf16x4*>(pout + e) = h;
    }
  }
}

static int g_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

}  // namespace dc

using namespace dc;

void ddim_step_launch(const float* x_t, const float* x0_raw, float* x_next, float* x0_out, const float* coef,
                      int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(ddim_step_kernel, dim3(g_grid(n)), dim3(256), 0, stream, x_t, x0_raw, x_next, x0_out, coef, n);
}

void cold_step_launch(float* x, const float* x0, const int64_t* t, void* patches_out, int B, int C, int H, int W,
                      int patch, int algorithm, bool rows, hipStream_t stream) {
  const dim3 grid(g_grid((int64_t)B * C * H * W / 4));
  bf16* po = reinterpret_cast<bf16*>(patches_out);
  if (rows)
    hipLaunchKernelGGL(cold_step_kernel<true>, grid, dim3(256), 0, stream, x, x0, t, po, B, C, H, W, patch, algorithm);
  else
    hipLaunchKernelGGL(cold_step_kernel<false>, grid, dim3(256), 0, stream, x, x0, t, po, B, C, H, W, patch,
                       algorithm);
}

void repaint_rows_launch(float* x, const float* known, const uint8_t* mask, const float* coef, const int64_t* rng,
                         int site_paste, int site_jump, void* patches_out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(repaint_rows_kernel, dim3(g_grid(n / 4)), dim3(256), 0, stream, x, known, mask, coef, rng,
                     site_paste, site_jump, reinterpret_cast<bf16*>(patches_out), (int)(n / 4));
}

void dpm2m_rows_launch(float* x, const float* x0, const float* x0_prev, const float* coef, int batch, bool each,
                       void* patches_out, int64_t n, hipStream_t stream) {
  hipLaunchKernelGGL(dpm2m_rows_kernel, dim3(g_grid(n / 4)), dim3(256), 0, stream, x, x0, x0_prev, coef, each ? 1 : 0,
                     (int)(n / 4 / batch), reinterpret_cast<bf16*>(patches_out), (int)(n / 4));
}

void randn_launch(float* out, int64_t n, const int64_t* rng, int site, hipStream_t stream) {
  hipLaunchKernelGGL(randn_kernel, dim3(g_grid((n + 1) / 2)), dim3(256), 0, stream, out, n, rng, site);
}

void q_sample_launch(const float* x0, const int64_t* t, const float* eps, float* out, int B, int64_t per,
                     int total_steps, hipStream_t stream) {
  hipLaunchKernelGGL(q_sample_kernel, dim3(g_grid((int64_t)B * per)), dim3(256), 0, stream, x0, t, eps, out, B, per,
                     total_steps);
}

void pixelate_pair_launch(const float* img, const int64_t* idx, const int64_t* t, float* x_t, float* x_tm1, int B,
                          int C, int H, int W, hipStream_t stream) {
  hipLaunchKernelGGL(pixelate_pair_kernel, dim3(g_grid((int64_t)B * C * H * W)), dim3(256), 0, stream, img, idx, t,
                     x_t, x_tm1, B, C, H, W);
}

void gauss_batch_launch(const ColdSrc& cs, const int64_t* rng, int B, int C, int H, int W, hipStream_t stream) {
  const int per = C * H * W;
  hipLaunchKernelGGL(gauss_batch_kernel, dim3(g_grid((int64_t)B * per)), dim3(256), 0, stream, cs.pool, cs.pool_n, rng,
                     cs.site, cs.noise_site, cs.gauss_T, cs.idx, cs.t_out, cs.draw_idx ? 1 : 0, cs.x_t, cs.target, B,
                     per, cs.idx_ctr, cs.idx_rows, cs.idx_stride);
}

void cold_batch_launch(const ColdSrc& cs, const int64_t* rng, int B, int C, int H, int W, hipStream_t stream) {
  hipLaunchKernelGGL(cold_batch_kernel, dim3(g_grid((int64_t)B * C * H * W)), dim3(256), 0, stream, cs.pool, cs.pool_n,
                     rng, cs.site, cs.max_t, cs.idx, cs.t_out, cs.draw_idx ? 1 : 0, cs.x_t, cs.target, B, C, H, W,
                     cs.idx_ctr, cs.idx_rows, cs.idx_stride);
}
