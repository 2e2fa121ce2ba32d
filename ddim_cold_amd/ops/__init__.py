"""Fused-op layer: one Python entry point per HIP kernel op.

GPU tensors go to ``torch.ops.ddim_cold.<op>`` (hand-written gfx950 kernels in
``csrc/``); CPU tensors go to the bit-compatible PyTorch reference in
:mod:`.reference`.  On a GPU the native path is mandatory (see
:mod:`._ext`): a missing extension raises instead of silently running eager
PyTorch.
"""
from __future__ import annotations

import math
from typing import NamedTuple, Optional

import torch

from . import _ext
from . import reference as ref
from ._ext import force_reference

__all__ = [
    "native_available", "patch_embed_fwd", "layernorm_fwd", "qkv_fwd", "attn_fwd", "attn_keep_buffer", "attn_plan",
    "linear_residual_fwd", "linear_gelu_fwd", "head_fwd", "smooth_l1_fwd_bwd", "img_to_tokgrad",
    "linear_dgrad", "linear_dgrad_gelu", "linear_wgrad", "layernorm_bwd", "attn_bwd", "embed_bwd",
    "sqnorm", "adamw_step", "weight_ema_decay", "advance_counters", "ddim_step", "ddim_step_", "randn_", "q_sample",
    "pixelate_pair", "cold_batch", "gauss_batch", "batch_draw", "BatchSource", "head_step_rows_", "cold_step_", "cold_step_rows_",
    "image_to_rows", "rows_to_image", "embed_weight_rows", "patch_embed_cold_fwd", "ln_fold_", "SITE_STEP_NOISE",
    "repaint_rows_", "dpm2m_rows_", "SITE_PASTE_NOISE", "SITE_JUMP_NOISE", "SITE_LOOP_FORWARDS",
    "HEAD_DDIM", "HEAD_CLAMP", "HEAD_DDIM_EACH", "HEAD_ETA", "HEAD_ETA_EACH",
]


def native_available() -> bool:
    return _ext.available()


def _hip(t: torch.Tensor) -> bool:
    return _ext.require_for(t)


def _ops():
    return torch.ops.ddim_cold


# ----------------------------------------------------------------------------- forward
def patch_embed_fwd(img, t, w_pe, b_pe, cls, pos, temb, rng, site: int, p: float, patch: int, ln_st=None,
                    xb_out=None, patches_in=None):
    """Tokens + bf16 patches.  LayerNorm fold: ``ln_st`` ([B*N, D/32, 2]) gets the
    tokens' row statistics ({sum, sum^2} per 32-column slot); ``xb_out`` their
    bf16 copy (the A operand of the first QKV GEMM).  ``patches_in``: the bf16
    patch rows of ``img`` already exist (a sampler step's :func:`head_step_` wrote
    them) -- on a GPU the patchify launch is skipped (the GEMM writes the cls rows)."""
    if _hip(img):
        return _ops().patch_embed_fwd(img, t, w_pe, b_pe, cls, pos, temb, rng, site, float(p), patch, ln_st, xb_out,
                                      patches_in)
    return ref.patch_embed_fwd(img, t, w_pe, b_pe, cls, pos, temb, rng, site, p, patch, ln_st, xb_out)


def patch_embed_cold_fwd(cold, img, t, w_pe, b_pe, cls, pos, temb, rng, site: int, p: float, patch: int,
                         ln_st=None, xb_out=None, target_rows: bool = False):
    """The draw of the :class:`BatchSource` ``cold`` (a plain tuple of its order is taken
    too) fused into :func:`patch_embed_fwd`, one launch fewer per training step: the
    patch rows come straight from the pool, ``img`` (x_t) and ``t`` are outputs.  Same
    values as :func:`batch_draw` then ``patch_embed_fwd``.  ``target_rows``: the target is
    written as patch rows in the head's output column order (:func:`image_to_rows`) into
    the same buffer, for :func:`head_loss` with ``target_rows``."""
    src = BatchSource(*cold)
    if _hip(img):
        ctr, off = src.idx_step if src.idx_step is not None else (None, 0)
        return _ops().patch_embed_cold_fwd(src.pool, int(src.site), int(src.max_t), bool(src.draw_idx),
                                           bool(src.target_x0), img, src.target, t, src.idx, bool(src.write_xt), w_pe,
                                           b_pe, cls, pos, temb, rng, site, float(p), patch, ln_st, xb_out,
                                           int(src.gauss_T), int(src.noise_site), bool(target_rows), ctr, int(off))
    batch_draw(src, rng, img, t)
    if target_rows:
        src.target.copy_(image_to_rows(src.target.clone(), patch).reshape(src.target.shape))
    return patch_embed_fwd(img, t, w_pe, b_pe, cls, pos, temb, rng, site, p, patch, ln_st, xb_out)


def layernorm_fwd(x, gamma, beta, eps: float = 1e-5):
    if _hip(x):
        return _ops().layernorm_fwd(x, gamma, beta, float(eps))
    return ref.layernorm_fwd(x, gamma, beta, eps)


def linear_fwd(a, w, b=None, out_fp32: bool = False, fold=None):
    """Plain ``a @ w.T + b`` on the MFMA GEMM (bf16 or fp32 output).  ``fold =
    (ln_st, ln_c, eps)``: LayerNorm folded in (``a`` = raw rows, ``w``/``b`` folded)."""
    st, c, eps = fold if fold is not None else (None, None, 1e-5)
    if _hip(a):
        return _ops().linear_fwd(a, w, b, bool(out_fp32), st, c, float(eps))
    return ref.linear_fwd(a, w, b, out_fp32, st, c, eps)


def _fold_args(fold):
    """``fold = (ln_st, ln_c, eps[, mean_out, rstd_out])`` -> op keyword tuple."""
    if fold is None:
        return None, None, 1e-5, None, None
    st, c, eps = fold[:3]
    mean, rstd = (fold[3], fold[4]) if len(fold) > 3 else (None, None)
    return st, c, float(eps), mean, rstd


def qkv_fwd(a, w, b, B: int, N: int, H: int, fold=None):
    """QKV projection, head-major [3,B,H,N,hd].  ``fold = (ln_st, ln_c, eps, mean_out,
    rstd_out)``: the preceding LayerNorm folded in (``a`` = bf16 residual rows,
    ``w``/``b`` from :func:`ln_fold_`); mean/rstd of the rows written for the backward."""
    st, c, eps, mean, rstd = _fold_args(fold)
    if _hip(a):
        return _ops().qkv_fwd(a, w, b, B, N, H, st, c, eps, mean, rstd)
    return ref.qkv_fwd(a, w, b, B, N, H, st, c, eps, mean, rstd)


class gemm_tile:
    """Context manager forcing the GEMM tile config of every launch inside it
    (csrc/gemm_plan.h: 0 = 32x64, 1 = 64x64, 2 = 128x64, 3 = 128x128 with 4 waves;
    4 = 256x128, 5 = 128x128, 6 = 256x192 with 8 waves; -1 = automatic).  Config 6 is
    built for the plain-operand BF16 / QKV / GELU epilogues only: elsewhere it runs as
    256x128 (128x128 for the GELU input gradient); config 3 is 128x64 for transposed B
    (``gemm_cfg_fallback``).  The launch follows ``gemm_plan`` of that header, and
    ``torch.ops.ddim_cold.gemm_plan`` is the same function: it names the tile and ring
    depth a launch takes and raises where the launch would (an 8-wave config on an
    epilogue without 8-wave tiles, a sampler / loss head epilogue at K % 64 != 0, an
    operand layout and epilogue without kernels).  Tests and micro-benchmarks; the
    automatic choice is the production path."""

    def __init__(self, cfg: int):
        self.cfg = int(cfg)
        self.prev = -1

    def __enter__(self):
        _ext.load(raise_on_error=True)
        self.prev = int(_ops().gemm_tile_override(self.cfg))
        return self

    def __exit__(self, *exc):
        _ops().gemm_tile_override(self.prev)
        return False


ATTN_PATHS = ("short", "v1", "resident", "flash2")


class AttnPlan(NamedTuple):
    """What an attention launch gets (csrc/attn_plan.h): the forward ``path`` of the shape
    (one of :data:`ATTN_PATHS`; the backward of every path but ``short`` is the dQ and dK/dV
    kernel pair), the short path's padded rows ``np`` (else 0), whether the dropout kernels
    run (``drop``) and whether they store / read keep flags (``keep``), the launch geometry,
    and the int32 ``keep_words`` a keep buffer of the shape holds."""
    path: str
    hd: int
    np: int
    drop: bool
    keep: bool
    grid_x: int
    grid_y: int
    block: int
    lds: int
    keep_words: int


def attn_plan(bwd: bool, B: int, H: int, N: int, hd: int, drop: bool, have_keep: bool) -> AttnPlan:
    """The plan ``attn_fwd`` (``bwd`` false) / ``attn_bwd`` follow: the same function as the
    launches call, so it raises where they would (a head dim other than 32 or 64, a keep
    buffer with dropout on where the v1 forward runs).  ``drop``: the dropout threshold of
    ``p`` is not 0.  Host only: launches nothing."""
    _ext.load(raise_on_error=True)
    v = [int(x) for x in _ops().attn_plan(bool(bwd), B, H, N, hd, bool(drop), bool(have_keep))]
    return AttnPlan(ATTN_PATHS[v[0]], v[1], v[2], bool(v[3]), bool(v[4]), *v[5:])


def attn_keep_buffer(qkv, p: float):
    """int32 buffer for the attention-dropout keep flags the forward stores for its
    backward (short sequences: one word per lane; long ones: one 64-bit word per
    query and 64-key tile), so the backward reads masks instead of re-hashing them;
    None when there is nothing to store (p = 0, CPU, or the one long-sequence
    forward that keeps no words, v1: 128 < N < 384 with fewer than 192 heads, and
    320 < N < 384 with any number)."""
    if p <= 0 or not _hip(qkv):
        return None
    _, B, H, N, hd = qkv.shape
    n = int(_ops().attn_keep_words(B, H, N, hd))
    return torch.empty(n, dtype=torch.int32, device=qkv.device) if n > 0 else None


def attn_fwd(qkv, scale: float, rng, site: int, p: float, keep_out=None):
    """``keep_out`` (:func:`attn_keep_buffer`): also store the dropout keep flags."""
    if _hip(qkv):
        return _ops().attn_fwd(qkv, float(scale), rng, site, float(p), keep_out)
    return ref.attn_fwd(qkv, scale, rng, site, p)


def linear_residual_fwd(a, w, b, x, N: int, rng, site_drop: int, p_drop: float, site_dp: int, p_dp: float,
                        st_out=None, xb_out=None):
    """x + DropPath(Dropout(a w^T + b)).  LayerNorm fold producer: ``st_out`` ([M, D/32, 2])
    gets the new rows' {sum, sum^2} per 32-column slot, ``xb_out`` their bf16 copy."""
    if _hip(a):
        return _ops().linear_residual_fwd(a, w, b, x, N, rng, site_drop, float(p_drop), site_dp, float(p_dp),
                                          st_out, xb_out)
    return ref.linear_residual_fwd(a, w, b, x, N, rng, site_drop, p_drop, site_dp, p_dp, st_out, xb_out)


def linear_gelu_fwd(a, w, b, rng, site: int, p: float, fold=None):
    st, c, eps, mean, rstd = _fold_args(fold)
    if _hip(a):
        return _ops().linear_gelu_fwd(a, w, b, rng, site, float(p), st, c, eps, mean, rstd)
    return ref.linear_gelu_fwd(a, w, b, rng, site, p, st, c, eps, mean, rstd)


def _ddim_coef(coef, x):
    """4 DDIM coefficients as python floats (one row) or [B,1,1,1] tensors (one row per sample)."""
    if coef.dim() == 2:
        return [coef[:, i].reshape(-1, 1, 1, 1).to(x.dtype) for i in range(4)]
    return [float(c) for c in coef.tolist()[:4]]


def head_step_(a, w, b, x, x0_out, coef, patch: int, mode: int, fold=None, patches_out=None):
    """Head GEMM + sampler step in its epilogue (in place on ``x``): mode 1 = clamp +
    DDIM update (``x0_out`` gets the clamped x0-hat; ``coef`` a device row of
    ``ddim_coefficients``), mode 2 = clamp only (cold sampler), mode 4 = mode 1 with
    one coefficient row per sample (``coef`` [B, 4]; img2img: the row {0, 1, 0, 1}
    leaves a sample that has not reached its start step unchanged).  ``patches_out``:
    also the new ``x`` as bf16 patch rows, for the next step's
    :func:`patch_embed_fwd` (``patches_in``)."""
    st, c, eps, _, _ = _fold_args(fold)
    if _hip(a):
        return _ops().head_step_(a, w, b, x, x0_out, coef, patch, mode, st, c, eps, patches_out)
    B, C, H, W = x.shape
    x0_raw = ref.head_fwd(a, w, b, B, C, H, W, patch, st, c, eps)
    if mode == HEAD_CLAMP:
        x.copy_(torch.clamp(x0_raw, -1.0, 1.0))
    else:
        xn, x0 = ref.ddim_step(x, x0_raw, _ddim_coef(coef, x))
        x.copy_(xn)
        x0_out.copy_(x0)
    if patches_out is not None:
        patches_out.copy_(ref.patchify_bf16(x, patch).view(patches_out.shape))


def image_to_rows(x, patch: int):
    """[B,C,H,W] -> [B*P, C*p*p] patch rows in the head's output column order
    ((a*p + b)*C + c for pixel (a, b) of the patch, channel c; ViT.py:214-217 unpatchify)."""
    B, C, H, W = x.shape
    p = patch
    return x.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 3, 5, 1).reshape(B * (H // p) * (W // p), p * p * C)


def rows_to_image(xr, B: int, C: int, H: int, W: int, patch: int):
    """Inverse of :func:`image_to_rows`."""
    p = patch
    return xr.reshape(B, H // p, W // p, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)


def embed_weight_rows(w_pe, C: int, patch: int):
    """Patch-embedding weight [D, C*p*p] (conv order c, a, b) with its columns permuted
    to the head's output order, so bf16 patch rows in that order (:func:`head_step_rows_`
    ``patches_out``) feed :func:`patch_embed_fwd` ``patches_in`` directly."""
    D = w_pe.shape[0]
    return w_pe.reshape(D, C, patch, patch).permute(0, 2, 3, 1).reshape(D, C * patch * patch)


# noise site of sampling step i (0-based from the top of the grid): SITE_STEP_NOISE + i, clear
# of the model's sites (1, 16 + 8 block + 0..5) and the data sites (3, 4)
SITE_STEP_NOISE = 4096
# inpainting (repaint_rows_): forward n of a loop pastes the known region with the noise of site
# SITE_PASTE_NOISE + n and jumps back with that of SITE_JUMP_NOISE + n; the three ranges are 4096
# apart, so a loop has fewer than SITE_LOOP_FORWARDS forwards
SITE_PASTE_NOISE = 8192
SITE_JUMP_NOISE = 12288
SITE_LOOP_FORWARDS = 4096
# head-step modes (csrc/kernels.h enum HeadMode, same names and values): clamp + DDIM update
# with one coefficient row / clamp only / DDIM with one row per sample / the stochastic
# (eta > 0) DDIM step with one row of 8 / with one row of 8 per sample
HEAD_DDIM, HEAD_CLAMP, HEAD_DDIM_EACH, HEAD_ETA, HEAD_ETA_EACH = 1, 2, 4, 5, 6


def head_step_rows_(a, w, b, x, x0_out, coef, batch: int, mode: int, fold=None, patches_out=None, noise=None):
    """:func:`head_step_` on patch rows (``x``/``x0_out``/``patches_out`` [B*P, F] in the
    head's output column order, :func:`image_to_rows`): every epilogue access is a
    contiguous vector instead of a scattered pixel.  Same math per element.

    Modes 5 / 6: the stochastic step of the DDIM family (eta > 0), ``x <- c2 x0 + dir (x -
    c0 x0) / c1 + sigma z`` from coefficient rows of 8 floats ``{c0, c1, c2, dir, sigma, 0,
    0, 0}`` (``schedule.eta_row``; mode 5 one row, mode 6 ``coef`` [B, 8], a sample that has
    not started ``{0, 1, 0, 1, 0, ..}``).  ``noise = (rng, site)``: ``z`` is element (row,
    column) of ``randn_(buf like x, rng, site)``, drawn inside the head epilogue on a GPU (no
    noise buffer, no extra launch); ``rng`` a device int64[2] ``{seed, 0}``."""
    st, c, eps, _, _ = _fold_args(fold)
    noisy = int(mode) in (HEAD_ETA, HEAD_ETA_EACH)
    if noisy != (noise is not None):
        raise ValueError("head_step_rows_: modes 5 / 6 take noise=(rng, site), the other modes take none")
    if _hip(a):
        if noisy:
            return _ops().head_step_rows_(a, w, b, x, x0_out, coef, int(batch), int(mode), st, c, eps, patches_out,
                                          noise[0], int(noise[1]))
        return _ops().head_step_rows_(a, w, b, x, x0_out, coef, int(batch), int(mode), st, c, eps, patches_out)
    F = w.shape[0]
    NP = x.shape[0] // batch
    y = ref._lin(a, w, b, st, c, eps)
    y = y.reshape(batch, NP + 1, F)[:, 1:].reshape(batch * NP, F)
    x0 = torch.clamp(y, -1.0, 1.0)
    if mode == HEAD_CLAMP:
        x.copy_(x0)
    elif noisy:
        if coef.numel() != (8 * batch if mode == HEAD_ETA_EACH else 8):
            raise ValueError("head_step_rows_: modes 5 / 6 take coefficient rows of 8 floats")
        z = torch.empty_like(x)
        randn_(z, noise[0], int(noise[1]))
        cf = coef.reshape(-1, 8).float()
        cf = cf.repeat_interleave(NP, 0) if mode == HEAD_ETA_EACH else cf.expand(x.shape[0], 8)
        xn, _ = ref.ddim_step_eta(x, y, cf, z)
        x.copy_(xn)
        x0_out.copy_(x0)
    else:
        cf = coef.reshape(-1, 4).float()
        each = cf.shape[0] == batch and mode == HEAD_DDIM_EACH
        cf = cf.repeat_interleave(NP, 0) if each else cf[:1].expand(x.shape[0], 4)
        eps_hat = (x - cf[:, 0:1] * x0) / cf[:, 1:2]
        x.copy_(cf[:, 2:3] * x0 + cf[:, 3:4] * eps_hat)
        x0_out.copy_(x0)
    if patches_out is not None:
        patches_out.copy_(x)


def head_fwd(a, w, b, B: int, C: int, H: int, W: int, patch: int, fold=None):
    st, c, eps, mean, rstd = _fold_args(fold)
    if _hip(a):
        return _ops().head_fwd(a, w, b, B, C, H, W, patch, st, c, eps, mean, rstd)
    return ref.head_fwd(a, w, b, B, C, H, W, patch, st, c, eps, mean, rstd)


def head_loss(a, w, b, target, patch: int, beta: float = 1.0, fold=None, target_rows: bool = False):
    """Head GEMM + mean smooth-L1 vs ``target`` + its gradient in the token layout, in
    one launch: ``(loss_parts, dtok)`` -- the loss is ``loss_parts.sum()`` (finished by
    the step tail of :func:`ln_fold_`); the predicted image is never materialised.
    ``target_rows``: the [B, C, H, W]-shaped ``target`` buffer holds patch rows in the
    head's output order (:func:`image_to_rows`; vector epilogue on a GPU)."""
    st, c, eps, mean, rstd = _fold_args(fold)
    if _hip(a):
        return _ops().head_loss(a, w, b, target, patch, float(beta), st, c, eps, mean, rstd, bool(target_rows))
    B, C, H, W = target.shape
    if target_rows:
        target = rows_to_image(target.reshape(-1, C * patch * patch), B, C, H, W, patch)
    out = ref.head_fwd(a, w, b, B, C, H, W, patch, st, c, eps, mean, rstd)
    N = a.shape[0] // B
    loss, dtok = ref.smooth_l1_fwd_bwd(out, target, N, patch, beta)
    return loss.reshape(1), dtok


def smooth_l1_fwd_bwd(pred, target, N: int, patch: int, beta: float = 1.0, loss_last=None, loss_ema=None,
                      ema_decay: float = 0.99, finish: bool = True):
    """Mean smooth-L1 loss and its token-layout gradient; optionally also writes
    ``loss_last`` and updates ``loss_ema`` (decay) in the same launch.  ``finish=False``
    returns the loss as per-block partials (summed later by the step tail of
    :func:`ln_fold_`) instead of launching the finishing reduction."""
    if _hip(pred):
        return _ops().smooth_l1_fwd_bwd(pred, target, N, patch, float(beta), loss_last, loss_ema, float(ema_decay),
                                        bool(finish))
    loss, dtok = ref.smooth_l1_fwd_bwd(pred, target, N, patch, beta)
    if not finish:
        return loss.reshape(1), dtok
    if loss_last is not None:
        loss_last.copy_(loss.reshape(loss_last.shape))
    if loss_ema is not None:
        loss_ema.mul_(ema_decay).add_(loss.reshape(loss_ema.shape), alpha=1.0 - ema_decay)
    return loss, dtok


def img_to_tokgrad(dimg, N: int, patch: int):
    if _hip(dimg):
        return _ops().img_to_tokgrad(dimg.contiguous(), N, patch)
    return ref.img_to_tokgrad(dimg, N, patch)


# ----------------------------------------------------------------------------- backward
def linear_dgrad(dy, w, out_fp32: bool, splits: int = 1):
    """``dy @ W``.  ``splits`` > 1: ``[splits, M, K]`` partial products (fp32 or
    bf16) over slices of the reduction dim, written without atomics or zeroing;
    :func:`layernorm_bwd` sums them (in fp32) as it loads ``dy``."""
    if _hip(dy):
        return _ops().linear_dgrad(dy, w, bool(out_fp32), int(splits))
    return ref.linear_dgrad(dy, w, out_fp32, splits)


def linear_dgrad_gelu(dy, w, u, rng, site: int, p: float, wt=None):
    """``(dy @ W) * gelu'(u)`` with the dropout mask of ``site``; ``wt`` (= W^T, bf16
    [in][out]): the product on the k-contiguous operand path."""
    if _hip(dy):
        if wt is not None:
            return _ops().linear_dgrad_gelu_t(dy, wt, u, rng, site, float(p))
        return _ops().linear_dgrad_gelu(dy, w, u, rng, site, float(p))
    return ref.linear_dgrad_gelu(dy, w, u, rng, site, p)


def linear_wgrad(dy, x, dw, db: Optional[torch.Tensor]):
    if _hip(dy):
        return _ops().linear_wgrad(dy, x, dw, db)
    return ref.linear_wgrad(dy, x, dw, db)


def wire_pack(src, dst):
    """fp32 -> bf16 (round to nearest even) into ``dst`` (gradient wire format)."""
    if _hip(src):
        return _ops().wire_pack(src, dst)
    if src.numel() != dst.numel():
        raise RuntimeError("wire_pack: sizes")
    dst.copy_(src)


def wire_unpack(src, dst):
    """bf16 -> fp32 into ``dst``."""
    if _hip(src):
        return _ops().wire_unpack(src, dst)
    if src.numel() != dst.numel():
        raise RuntimeError("wire_unpack: sizes")
    dst.copy_(src)


WGRAD_WIDE_TOKENS = 16384  # csrc/wgrad_plan.h BIG_WG_K
WGRAD_TICKETS = 4096       # csrc/wgrad_plan.h


def wgrad_embed_slots(B: int, N: int, D: int, owners: int, n_ln: int, ln_C: int, tokens: int) -> int:
    """Grad-norm partial slots (= extra workgroups) the embedding parts of
    :func:`linear_wgrad_multi` take in a launch whose longest reduction runs over
    ``tokens`` rows (512-thread workgroups from ``WGRAD_WIDE_TOKENS``, 256-thread ones
    below).  The loaded extension's own count when there is one, like :func:`ln_ws_rows`."""
    if native_available():
        return int(_ops().wgrad_embed_slots(B, N, D, owners, n_ln, ln_C, tokens))
    nt = 512 if tokens >= WGRAD_WIDE_TOKENS else 256
    return -(-(N * D) // nt) + owners * -(-D // 16) + (n_ln * -(-ln_C // 16) if n_ln else 0)


def wgrad_tickets(device) -> torch.Tensor:
    """A zeroed ticket buffer for the K-split tail tiles of :func:`linear_wgrad_multi`
    (``tickets=``).  Its owner allocates it outside any graph capture and keeps it as long
    as a graph that uses it; every launch leaves it zero, so launches ordered on one stream
    share one buffer."""
    return torch.zeros(WGRAD_TICKETS, dtype=torch.int32, device=device)


class GradNorm(NamedTuple):
    """``linear_wgrad_multi(sq=)``: the launch is the last writer of the gradient ``arena``
    (every dw / db a view of it) and writes the grad-norm ``parts`` :func:`sqnorm` would (same
    layout, scale 1, instead of that pass): each output tile the sum of squares of its final
    values, extra workgroups the arena outside every target and outside ``lazy`` = (lo, hi)."""
    parts: torch.Tensor
    arena: torch.Tensor
    lazy: Optional[tuple] = None


class LnFinal(NamedTuple):
    """The LayerNorm slot finalize (:func:`replica_reduce_` of ``ws`` [G, R, width] into the
    addresses ``dst_ptrs``) riding in another launch (GPU only); ``store``: the destinations
    get the sum instead of having it added.  ``offs`` (their element offsets in the gradient
    arena): only the weight-gradient launch needs them, for its grad-norm partials."""
    ws: torch.Tensor
    dst_ptrs: torch.Tensor
    width: int
    rows: int
    store: bool = False
    offs: Optional[list] = None


class EmbedGrads(NamedTuple):
    """``linear_wgrad_multi(embed=)``: the cls / pos / time-embedding gradients of
    :func:`embed_bwd` (``g`` .. ``dtemb`` as there; ``owners`` >= the distinct timesteps a
    batch can hold) and, with ``ln``, the LayerNorm finalize ride in the launch as extra
    workgroups (each writing the grad-norm partials of its outputs); the patch-row gradient
    comes from the last LayerNorm backward (:func:`layernorm_bwd` ``gp_out``).  Deterministic."""
    g: torch.Tensor
    t: torch.Tensor
    rng: torch.Tensor
    site: int
    p: float
    dcls: torch.Tensor
    dpos: torch.Tensor
    dtemb: torch.Tensor
    owners: int
    ln: Optional[LnFinal] = None


class BatchSource(NamedTuple):
    """A training batch source, from the batcher (``data.synthetic``) to the kernels
    (``ColdSrc`` in csrc/kernels.h): the draw of one batch (x_t, target, t), either fused into
    the patch embedding (:func:`patch_embed_cold_fwd`) or on its own (:func:`batch_draw`).

    ``pool`` [n,C,H,W]: the images drawn from.  ``site``: the RNG site of the pool index and of
    t.  ``max_t``: t ~ U{1..max_t} and x_t = the pool image pixelated by 2^t (cold
    diffusion).  ``draw_idx``: the pool indices are drawn and written to ``idx``; else ``idx``
    holds them.  ``target_x0``: the target is the pool image x0, else x_{t-1}.  ``target``
    [B,C,H,W] and ``idx`` [B]: written (idx only if drawn).  ``write_xt``: the fused draw
    writes the x_t image as well as its patch rows (the draw on its own always does).
    ``gauss_T`` > 0: the Gaussian DDIM batch instead -- t ~ U{0..gauss_T-1}, x_t =
    q_sample(x0, t, eps) with eps = :func:`randn_` at ``noise_site``, target x0 (``max_t``
    unused).  ``idx_step = (ctr, off)``: ``idx`` is a stepped table read at row ``ctr[0] %
    rows``, elements ``off .. off+B`` (:func:`stepped_idx`).

    Field order is the op's positional order: a plain tuple of the first 8, 10 or all 11
    entries is taken wherever a ``BatchSource`` is."""
    pool: torch.Tensor
    site: int
    max_t: int
    draw_idx: bool
    target_x0: bool
    target: torch.Tensor
    idx: torch.Tensor
    write_xt: bool
    gauss_T: int = 0
    noise_site: int = 0
    idx_step: Optional[tuple] = None

    @classmethod
    def cold(cls, pool, site: int, max_t: int, target, idx, draw_idx: bool = True, target_x0: bool = False,
             write_xt: bool = False, idx_step=None):
        return cls(pool, site, max_t, draw_idx, target_x0, target, idx, write_xt, 0, 0, idx_step)

    @classmethod
    def gaussian(cls, pool, site: int, noise_site: int, total_steps: int, x0, idx, draw_idx: bool = True,
                 write_xt: bool = False, idx_step=None):
        return cls(pool, site, 1, draw_idx, True, x0, idx, write_xt, total_steps, noise_site, idx_step)


class StepTail(NamedTuple):
    """``ln_fold_(tail=)``: the training step's tail rides in the fold launch -- the loss
    from the smooth-L1 partials ``loss_parts`` (``loss_last``, and ``loss_ema`` with
    ``ema_decay``) and the counter advance of :func:`advance_counters` on ``step`` / ``rng``
    (optimizer step only if the grad norm ``sq`` is finite)."""
    loss_parts: torch.Tensor
    loss_last: Optional[torch.Tensor]
    loss_ema: Optional[torch.Tensor]
    ema_decay: float
    step: torch.Tensor
    rng: torch.Tensor
    sq: Optional[torch.Tensor]


def linear_wgrad_multi(jobs, store: bool = False, sq=None, embed=None, tickets=None):
    """Every ``(dy, x, dw, db)`` weight-gradient job of a step (<= 32) in ONE launch
    (csrc/gemm.hip ``gemm_wgrad_multi_kernel``; unsplit, deterministic).  ``store``:
    the targets are zero (``dW = dy^T x`` written, not added: no read of dW).
    ``sq``: a :class:`GradNorm`; ``embed``: an :class:`EmbedGrads` (plain tuples of the
    same order are taken too).

    ``tickets`` (:func:`wgrad_tickets`): reductions over >= 16,384 tokens run the tiles
    past the last whole round of workgroups as K pieces that take a ticket each.  Without
    it an eager call zero-fills a buffer of its own; a call inside a graph capture that
    needs tickets raises.  ``torch.ops.ddim_cold.wgrad_multi_plan`` reports the launches."""
    if not jobs:
        return
    sq = None if sq is None else GradNorm(*sq)
    embed = None if embed is None else EmbedGrads(*embed)
    ln = None if embed is None or embed.ln is None else LnFinal(*embed.ln)
    if ln is not None and ln.offs is None:
        raise ValueError("the LayerNorm finalize in the weight-gradient launch needs LnFinal.offs")
    if _hip(jobs[0][0]):  # (more than 32 jobs: consecutive launches of <= 32)
        dys, xs, dws, dbs = (list(z) for z in zip(*jobs))
        parts, arena, lazy = sq if sq is not None else (None, None, None)
        lo, hi = lazy if lazy is not None else (0, 0)
        if embed is None:
            _ops().linear_wgrad_multi(dys, xs, dws, dbs, bool(store), parts, arena, int(lo), int(hi),
                                      split_tickets=tickets)
            return
        e = embed
        if ln is None:
            ln = LnFinal(None, None, 0, 0, False, [])
        _ops().linear_wgrad_multi(dys, xs, dws, dbs, bool(store), parts, arena, int(lo), int(hi), e.g, e.t, e.rng,
                                  int(e.site), float(e.p), e.dcls, e.dpos, e.dtemb, int(e.owners), ln.ws,
                                  ln.dst_ptrs, [int(o) for o in ln.offs], int(ln.width), int(ln.rows),
                                  bool(ln.store), tickets)
        return
    for dy, x, dw, db in jobs:
        if store:
            dw.zero_()
            if db is not None:
                db.zero_()
        ref.linear_wgrad(dy, x, dw, db)
    if embed is not None:
        ref.embed_bwd(*embed[:8])
        if ln is not None:
            raise ValueError("the LayerNorm finalize in the weight-gradient launch needs the HIP extension")
    if sq is not None:
        sqnorm(sq.arena, sq.parts, 1.0, lazy=sq.lazy)


def transpose_bf16_(srcs, dsts):
    """``dsts[i] = srcs[i].T`` for bf16 matrices (one launch per 96; csrc/transpose.hip):
    the transposed weight shadows the input-gradient GEMMs read k-contiguous."""
    if srcs and _hip(srcs[0]):
        _ops().transpose_bf16_(list(srcs), list(dsts))
        return
    for s_, d_ in zip(srcs, dsts):
        d_.copy_(s_.t())


def ln_ws_rows(M: int) -> int:
    """Rows ([rows, 2D] floats) of the dgamma||dbeta workspace :func:`layernorm_bwd`
    takes for ``M`` rows: one slot per backward workgroup (csrc/layernorm.hip: 8 rows per
    workgroup, at most 512 workgroups), each overwritten by its workgroup, summed in slot
    order by :func:`replica_reduce_` (deterministic, no atomics).  The loaded extension's
    own count when there is one (one source of truth; A/B runs load other builds)."""
    if native_available():
        return int(_ops().ln_ws_rows(int(M)))
    return max(1, min(-(-M // 8), 512))


def layernorm_bwd(dy, x, mean, rstd, gamma, g_res, dgamma, dbeta, N: int, rng, site_drop: int, p_drop: float,
                  site_dp: int, p_dp: float, emit_gy: bool, ws: Optional[torch.Tensor] = None, beta=None,
                  y_out=None, gp_out=None, site_emb: int = 0, p_emb: float = 0.0):
    """LayerNorm backward.  With ``ws`` ([ln_ws_rows(M), 2D]) the dgamma||dbeta
    partials stay in the workspace slots (finalise later with :func:`replica_reduce_`;
    deterministic, no atomics); otherwise they are added into dgamma / dbeta.
    ``y_out`` (with ``beta``): also write the LayerNorm output (bf16) — the
    forward folded the LayerNorm into the next GEMM and never stored it.
    ``gp_out`` ([B*(N-1), D] bf16; the last LayerNorm of the backward): also write the
    patch-embedding input gradient, g_out's token rows 1..N-1 with the embedding
    dropout (``site_emb``, ``p_emb``) -- what :func:`embed_bwd` returns."""
    if _hip(x):
        g_out, gy = _ops().layernorm_bwd(dy, x, mean, rstd, gamma, g_res, dgamma, dbeta, N, rng, site_drop,
                                         float(p_drop), site_dp, float(p_dp), bool(emit_gy), ws, beta, y_out,
                                         gp_out, int(site_emb), float(p_emb))
        return g_out, (gy if emit_gy else None)
    if ws is not None:
        D = x.shape[-1]
        dgamma, dbeta = ws[0, :D], ws[0, D:]
    if y_out is not None:
        ref.layernorm_out_(x, mean, rstd, gamma, beta, y_out)
    g_out, gy = ref.layernorm_bwd(dy, x, mean, rstd, gamma, g_res, dgamma, dbeta, N, rng, site_drop, p_drop,
                                  site_dp, p_dp, emit_gy)
    if gp_out is not None:
        gp_out.copy_(ref.embed_patch_grad(g_out.view(-1, N, x.shape[-1]), rng, site_emb, p_emb))
    return g_out, gy


def ln_fold_(ws, gammas, betas, biases, wfs, cs, bfs, tail=None):
    """LayerNorm fold weights for GEMMs that consume a LayerNorm (one launch on GPU):
    ``wf = bf16(gamma o W)``, ``c = rowsum(wf)``, ``bf = b + W beta``.

    ``tail``: a :class:`StepTail`, the training step's tail in the same launch."""
    if not ws:
        return
    t = StepTail(*tail) if tail is not None else StepTail(None, None, None, 0.99, None, None, None)
    if _hip(ws[0]):
        return _ops().ln_fold_(list(ws), list(gammas), list(betas), list(biases), list(wfs), list(cs), list(bfs),
                               t.loss_parts, t.loss_last, t.loss_ema, float(t.ema_decay), t.step, t.rng, t.sq)
    for w, g, be, b, wf, c, bf in zip(ws, gammas, betas, biases, wfs, cs, bfs):
        ref.ln_fold(w, g, be, b, wf, c, bf)
    if tail is not None:
        loss = t.loss_parts.float().sum().reshape(1)
        if t.loss_last is not None:
            t.loss_last.copy_(loss.reshape(t.loss_last.shape))
        if t.loss_ema is not None:
            t.loss_ema.mul_(t.ema_decay).add_(loss.reshape(t.loss_ema.shape), alpha=1.0 - t.ema_decay)
        advance_counters(t.step, t.rng, t.sq)


def replica_reduce_(ws, dst_ptrs, C: int, R: int, dsts=None):
    """dst[g] += ws[g, :R].sum(0) (rows in order) for G LayerNorm workspaces
    ([G, rows, C]; ``R`` = :func:`ln_ws_rows` of the backward's row count).

    ``dst_ptrs`` is a device int64 tensor of destination addresses (GPU); the
    CPU path takes the destination tensors in ``dsts`` instead (and re-zeroes the
    rows: its LayerNorm backward accumulates into row 0)."""
    if _hip(ws):
        return _ops().replica_reduce_(ws, dst_ptrs, C, int(R))
    for g, d in enumerate(dsts):
        d.add_(ws[g, :R].sum(0))
    ws[:, :R].zero_()


def attn_bwd(do, qkv, o, lse, scale: float, rng, site: int, p: float, keep=None):
    """``keep``: the keep flags :func:`attn_fwd` stored (same masks as re-hashing)."""
    if _hip(qkv):
        return _ops().attn_bwd(do, qkv, o, lse, float(scale), rng, site, float(p), keep)
    return ref.attn_bwd(do, qkv, o, lse, scale, rng, site, p)


def embed_bwd(g, t, rng, site: int, p: float, dcls, dpos, dtemb, ln_final=None):
    """``ln_final``: an :class:`LnFinal` riding in the same launch.  Deterministic: no
    fp32 atomics (the time-embedding rows are summed per distinct timestep)."""
    if _hip(g):
        ln = LnFinal(*ln_final) if ln_final is not None else LnFinal(None, None, 0, 0)
        return _ops().embed_bwd(g, t, rng, site, float(p), dcls, dpos, dtemb, ln.ws, ln.dst_ptrs, int(ln.width),
                                bool(ln.store), int(ln.rows))
    if ln_final is not None:
        raise ValueError("ln_final needs the HIP extension (use replica_reduce_ on CPU)")
    return ref.embed_bwd(g, t, rng, site, p, dcls, dpos, dtemb)


# ----------------------------------------------------------------------------- optimizer
SQ_PARTS = 1024  # csrc/kernels.h


def sq_parts_size(n_tiles: int) -> int:
    """Grad-norm partial buffer size (floats) for a fused weight-gradient launch of
    ``n_tiles`` 64x64 tiles: room for the tiles, up to 64 tail workgroups, >= SQ_PARTS,
    a multiple of 256 (what every consumer kernel accepts)."""
    n = max(SQ_PARTS, n_tiles + 64)
    return (n + 255) // 256 * 256


def sqnorm(g, out, scale: float = 1.0, lazy=None):
    """Per-block partial sums of (g*scale)^2 into ``out`` (>= SQ_PARTS floats, a multiple
    of 256, fully overwritten).
    ``lazy`` = (lo, hi): an arena range whose gradient is identically zero (skipped: not
    read; whole 16-byte vectors inside the arena, anything else raises)."""
    lo, hi = lazy if lazy is not None else (0, 0)
    if _hip(g):
        return _ops().sqnorm(g, out, float(scale), int(lo), int(hi))
    n = g.numel()
    if hi > lo and (lo < 0 or hi > n // 4 * 4 or lo % 4 or hi % 4):
        raise RuntimeError("optimizer lazy range must be whole 16-B vectors inside the arena")
    flat = g.reshape(-1).float()
    if hi > lo:
        flat = torch.cat((flat[:lo], flat[hi:]))
    out.zero_()
    out[0] = (flat * scale).pow(2).sum()


def weight_ema_decay(decay: float, t: int, warmup: bool) -> torch.Tensor:
    """The weight EMA's decay for the update that follows ``t`` completed Adam steps, as
    a fp32 scalar: ``decay``, or with ``warmup`` min(decay, (1 + t) / (10 + t)) evaluated
    in fp32 (0.1 at the first update; what the kernel computes from ``step[0]``)."""
    d = torch.tensor(float(decay), dtype=torch.float32)
    if not warmup:
        return d
    ts = torch.tensor(int(t), dtype=torch.int64).to(torch.float32)
    return torch.minimum(d, (1.0 + ts) / (10.0 + ts))


def adamw_step(p, g, m, v, pbf, sq, step, hyper, grad_scale: float = 1.0, zero_hi: Optional[int] = None,
               lazy=None, lazy_decay=None, ema=None, ema_decay: float = 0.0, ema_warmup: bool = False):
    """Fused AdamW over a flat arena (see csrc/optim.hip for the exact math).
    ``zero_hi``: zero the gradients only below this element (the producers of the
    rest overwrite them next step); default: all.  ``lazy`` = (lo, hi) with
    ``lazy_decay`` (fp32 [1]): parameters whose gradient and moments are identically
    zero; they are not touched, their weight decay (1 - lr*wd per step) accumulates
    into ``lazy_decay`` for ``TrainEngine.materialize_lazy``.
    ``ema`` (fp32, the arena's size): an exponential moving average of the parameters
    updated in the same pass, ``e <- p_new + d * (e - p_new)`` as three separately rounded
    fp32 operations, with ``d`` = :func:`weight_ema_decay` (``ema_decay``, ``step[0]``,
    ``ema_warmup``); left alone on a skipped step; not together with ``lazy``."""
    lo, hi = lazy if lazy is not None and lazy_decay is not None else (0, 0)
    if _hip(p):
        if ema is None:
            return _ops().adamw_step(p, g, m, v, pbf, sq, step, hyper, float(grad_scale),
                                     -1 if zero_hi is None else int(zero_hi), int(lo), int(hi), lazy_decay)
        return _ops().adamw_step(p, g, m, v, pbf, sq, step, hyper, float(grad_scale),
                                 -1 if zero_hi is None else int(zero_hi), int(lo), int(hi), lazy_decay,
                                 ema, float(ema_decay), bool(ema_warmup))
    if ema is not None:
        if hi > lo:
            raise RuntimeError("adamw_step: a lazy range cannot be combined with a weight EMA")
        if ema.dtype != torch.float32 or ema.numel() != p.numel():
            raise RuntimeError("adamw_step: ema must be fp32 of the arena's size")
        if not 0.0 <= float(ema_decay) < 1.0:
            raise RuntimeError(f"adamw_step: ema_decay must be in [0, 1), got {ema_decay}")
    sqv = float(sq.sum())
    base_lr, b1, b2, eps, wd, max_norm, tmax, eta_min = (float(x) for x in hyper.tolist()[:8])
    coef = grad_scale
    if max_norm > 0:
        coef *= min(1.0, max_norm / (math.sqrt(sqv) + 1e-6)) if math.isfinite(sqv) else 1.0
    gi = g * coef
    g_lazy = g[lo:hi].clone()  # the lazy range is not touched, its gradient included
    g[: (g.numel() if zero_hi is None else zero_hi)].zero_()
    g[lo:hi] = g_lazy
    if not math.isfinite(sqv):
        return
    t = int(step[0]) + 1
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    lr = base_lr
    if tmax > 0:
        lr = eta_min + (base_lr - eta_min) * 0.5 * (1 + math.cos(math.pi * int(step[1]) / tmax))
    if hi > lo:  # the lazy range: untouched, its decay accumulated (same as the kernel)
        keep = (p[lo:hi].clone(), m[lo:hi].clone(), v[lo:hi].clone())
        lazy_decay.mul_(1 - lr * wd)
    p.mul_(1 - lr * wd)
    m.mul_(b1).add_(gi, alpha=1 - b1)
    v.mul_(b2).addcmul_(gi, gi, value=1 - b2)
    p.addcdiv_(m, v.sqrt() / math.sqrt(bc2) + eps, value=-lr / bc1)
    if hi > lo:
        p[lo:hi], m[lo:hi], v[lo:hi] = keep
    if pbf is not None:
        pb_lazy = pbf[lo:hi].clone()
        pbf.copy_(p.to(torch.bfloat16))
        pbf[lo:hi] = pb_lazy
    if ema is not None:  # e <- p + d (e - p): sub, mul, add, each rounded to fp32
        d = weight_ema_decay(ema_decay, t - 1, ema_warmup).to(p.device)
        ema.sub_(p).mul_(d).add_(p)


def advance_counters(step, rng, sq=None):
    if _hip(step):
        return _ops().advance_counters(step, rng, sq)
    if sq is None or math.isfinite(float(sq.sum())):
        step[0] += 1
    step[1] += 1
    rng[1] += 1


# ----------------------------------------------------------------------------- diffusion / data
def ddim_step(x_t, x0_raw, coef):
    if _hip(x_t):
        return _ops().ddim_step(x_t, x0_raw, coef)
    return ref.ddim_step(x_t, x0_raw, [float(c) for c in coef.tolist()[:4]])


def ddim_step_(x, x0_raw, x0_out, coef):
    """In-place DDIM step; ``coef`` one row of 4 (GPU kernel) or [B, 4] per sample (torch ops)."""
    if _hip(x) and coef.dim() == 1:
        return _ops().ddim_step_(x, x0_raw, x0_out, coef)
    xn, x0 = ref.ddim_step(x, x0_raw, _ddim_coef(coef, x))
    x.copy_(xn)
    x0_out.copy_(x0)


def _cold_rows_out(patches_out, rows_bf16, t, batch: int):
    """CPU: the patch rows of the samples a cold step updated (t >= 1); the others stay."""
    if patches_out is None:
        return
    keep = (t.reshape(-1) >= 1).repeat_interleave(rows_bf16.shape[0] // batch)
    patches_out[keep] = rows_bf16[keep]


def cold_step_(x, x0, t, algorithm: int = 2, patches_out=None):
    """Cold-diffusion sampling step of an x0-predicting model, in place on ``x``
    (:func:`reference.cold_step`: algorithm 1 ``D(x0, t-1)``, algorithm 2 ``(x - D(x0, t))
    + D(x0, t-1)``; per-sample ``t``, a sample with ``t <= 0`` is not touched).  ``x`` /
    ``x0`` fp32 [B,C,H,W], distinct buffers, ``x0`` already clamped.  ``patches_out``
    (bf16 [B*P, C*p*p], the patch size taken from its width): also the new ``x`` as
    conv-order patch rows, the next step's :func:`patch_embed_fwd` ``patches_in``."""
    C = x.shape[1]
    patch = 0 if patches_out is None else math.isqrt(patches_out.shape[1] // C)
    if patches_out is not None and patch * patch * C != patches_out.shape[1]:
        raise ValueError("cold_step_: patches_out must be [B*P, C*p*p]")
    if _hip(x):
        return _ops().cold_step_(x, x0, t, int(algorithm), patch, patches_out)
    x.copy_(ref.cold_step(x, x0, t, algorithm))
    if patches_out is not None:
        _cold_rows_out(patches_out, ref.patchify_bf16(x, patch), t, x.shape[0])


def cold_step_rows_(x, x0, t, batch: int, C: int, H: int, W: int, patch: int, algorithm: int = 2, patches_out=None):
    """:func:`cold_step_` on patch rows (``x`` / ``x0`` / ``patches_out`` [B*P, C*p*p] in the
    head's output column order, :func:`image_to_rows`): the sampler's patch-row state is
    updated where it lives and handed to the next step's patch embedding as bf16."""
    if _hip(x):
        return _ops().cold_step_rows_(x, x0, t, int(batch), int(C), int(H), int(W), int(patch), int(algorithm),
                                      patches_out)
    xi, x0i = (rows_to_image(v, batch, C, H, W, patch) for v in (x, x0))
    x.copy_(image_to_rows(ref.cold_step(xi, x0i, t, algorithm), patch))
    _cold_rows_out(patches_out, x.to(torch.bfloat16), t, batch)


def repaint_rows_(x, known, mask, coef, rng, site_paste: int, site_jump: int, patches_out=None):
    """Mask step of inpainting (RePaint), in place on the sampler's fp32 patch rows ``x`` [B*P, F]
    (:func:`reference.repaint_rows`): where ``mask`` (uint8, same shape) is non-zero ``x <- ka
    known + kb z1``, then, unless ``{ra, rb}`` is ``{1, 0}``, ``x <- ra x + rb z2`` everywhere.
    ``coef`` a device fp32 ``{ka, kb, ra, rb}`` (``schedule.repaint_row``), ``z1`` / ``z2`` =
    :func:`randn_` over a buffer like ``x`` at ``(rng, site_paste)`` / ``(rng, site_jump)``, ``rng``
    an int64[2] ``{seed, 0}``.  ``patches_out`` (bf16, same shape): the bf16 of every element
    written; a paste-only call writes nothing where four consecutive mask bytes are zero."""
    if _hip(x):
        return _ops().repaint_rows_(x, known, mask, coef, rng, int(site_paste), int(site_jump), patches_out)
    if min(int(site_paste), int(site_jump)) < 0:
        raise ValueError("repaint_rows_: noise sites must be non-negative")
    out, wrote = ref.repaint_rows(x, known, mask, coef, rng, int(site_paste), int(site_jump))
    x.copy_(out)
    if patches_out is not None:
        patches_out[wrote] = out.to(torch.bfloat16)[wrote]


def dpm2m_rows_(x, x0, x0_prev, coef, batch: int, each: bool = False, patches_out=None):
    """DPM-Solver++(2M) step, in place on the sampler's fp32 patch rows ``x`` [B*P, F]
    (:func:`reference.dpm2m_rows`): ``x <- c2 x0 + c3 (x - c0 x0) / c1 + g (x0 - x0_prev)`` with
    ``x0`` the clamped prediction of this step's forward and ``x0_prev`` the previous step's
    (distinct buffers of ``x``'s shape).  ``coef``: device fp32 rows ``{c0, c1, c2, c3, g, 0, 0,
    0}`` (``schedule.dpm2m_row``), one, or with ``each`` one per sample [batch, 8].  A row with
    ``g == 0`` is the DDIM step and does not read ``x0_prev``.  ``patches_out`` (bf16, same
    shape): the bf16 of the new ``x``, the next step's patch rows."""
    if _hip(x):
        return _ops().dpm2m_rows_(x, x0, x0_prev, coef, int(batch), bool(each), patches_out)
    out = ref.dpm2m_rows(x, x0, x0_prev, coef, int(batch), bool(each))
    x.copy_(out)
    if patches_out is not None:
        patches_out.copy_(out.to(torch.bfloat16))


def randn_(out, rng, site: int):
    if _hip(out):
        return _ops().randn_(out, rng, site)
    salt = ref.site_salt(rng, site)
    n = out.numel()
    pairs = (n + 1) // 2
    i = torch.arange(pairs, dtype=torch.int64)
    ha = ref.mix32(ref._mul32((2 * i) & ref.MASK32, ref.GOLDEN) ^ salt)
    hb = ref.mix32(ref._mul32((2 * i + 1) & ref.MASK32, ref.GOLDEN) ^ salt)
    a = ((ha >> 8).double() + 0.5) / 16777216.0
    b = ((hb >> 8).double() + 0.5) / 16777216.0
    r = torch.sqrt(-2.0 * torch.log(a))
    z = torch.stack((r * torch.cos(2 * torch.pi * b), r * torch.sin(2 * torch.pi * b)), dim=1).reshape(-1)[:n]
    out.copy_(z.float().view(out.shape))


def q_sample(x0, t, eps, total_steps: int):
    if _hip(x0):
        return _ops().q_sample(x0, t, eps, total_steps)
    return ref.q_sample(x0, t, eps, total_steps)


def pixelate_pair(img, idx, t, B: int):
    if _hip(img):
        return _ops().pixelate_pair(img, idx, t, B)
    src = img if idx is None else img[idx]
    xt = torch.stack([ref.pixelate(src[i:i + 1], 2 ** int(t[i]))[0] for i in range(B)])
    xtm1 = torch.stack([ref.pixelate(src[i:i + 1], 2 ** (int(t[i]) - 1))[0] for i in range(B)])
    return xt, xtm1


def stepped_idx(idx, idx_step, B: int):
    """The [B] pool indices a batch source reads: ``idx`` itself, or with ``idx_step =
    (ctr, off)`` row ``ctr[0] % rows`` of the stepped table ``idx`` ([rows, ...]),
    elements ``off .. off+B`` (the trainer's epoch table indexed by the device step
    counter, so a K-step graph needs no host copy per step)."""
    if idx_step is None:
        return idx
    ctr, off = idx_step
    r = torch.remainder(ctr.reshape(-1)[:1], idx.shape[0])  # device ops: graph-capturable, no host sync
    return idx.reshape(idx.shape[0], -1).index_select(0, r)[0, int(off):int(off) + B]


def gauss_batch(pool, rng, site: int, noise_site: int, total_steps: int, x_t, x0, t, idx, draw_idx: bool = True,
                idx_step=None):
    """Gaussian DDIM batch on device in one launch (diffusion_loader.py:24-58): pool
    index (unless ``draw_idx`` is False: ``idx`` holds them; ``idx_step``: see
    :func:`stepped_idx`) and t ~ U{0..T-1} from the ``site`` hash, eps =
    :func:`randn_` of a [B,C,H,W] tensor at ``noise_site``, ``x_t = q_sample(x0, t,
    eps)``; ``x0`` = the pool images."""
    if _hip(pool):
        ctr, off = idx_step if idx_step is not None else (None, 0)
        return _ops().gauss_batch(pool, rng, site, noise_site, total_steps, x_t, x0, t, idx, bool(draw_idx), ctr,
                                  int(off))
    salt = ref.site_salt(rng, site)
    B = x_t.shape[0]
    b = torch.arange(B, dtype=torch.int64)
    idx = stepped_idx(idx, idx_step, B)
    if draw_idx:
        idx.copy_(ref.mix32(ref._mul32((2 * b) & ref.MASK32, ref.GOLDEN) ^ salt) % pool.shape[0])
    t.copy_(ref.mix32(ref._mul32((2 * b + 1) & ref.MASK32, ref.GOLDEN) ^ salt) % total_steps)
    eps = torch.empty_like(x_t)
    randn_(eps, rng, noise_site)
    torch.index_select(pool, 0, idx, out=x0)
    x_t.copy_(ref.q_sample(x0, t, eps, total_steps))


def cold_batch(pool, rng, site: int, x_t, x_tm1, t, idx_ws, max_t: int, draw_idx: bool = True, idx_step=None):
    """Cold pixelation batch on device: t ~ U{1..max_t} (and pool indices unless
    ``draw_idx`` is False, in which case ``idx_ws`` holds them; ``idx_step``: see
    :func:`stepped_idx`), x_t / x_{t-1}."""
    if _hip(pool):
        ctr, off = idx_step if idx_step is not None else (None, 0)
        return _ops().cold_batch(pool, rng, site, x_t, x_tm1, t, idx_ws, max_t, bool(draw_idx), ctr, int(off))
    salt = ref.site_salt(rng, site)
    B = x_t.shape[0]
    b = torch.arange(B, dtype=torch.int64)
    idx_ws = stepped_idx(idx_ws, idx_step, B)
    if draw_idx:
        idx_ws.copy_(ref.mix32(ref._mul32((2 * b) & ref.MASK32, ref.GOLDEN) ^ salt) % pool.shape[0])
    t.copy_(1 + ref.mix32(ref._mul32((2 * b + 1) & ref.MASK32, ref.GOLDEN) ^ salt) % max_t)
    a, c = pixelate_pair(pool, idx_ws, t, B)
    x_t.copy_(a)
    x_tm1.copy_(c)


def batch_draw(src, rng, x_t, t):
    """The draw of a :class:`BatchSource` on its own (not fused into the patch embedding):
    :func:`gauss_batch` when ``src.gauss_T > 0``, else :func:`cold_batch`, whose x_{t-1}
    target the pool images replace when ``src.target_x0``.  Writes ``x_t``, ``t``,
    ``src.target`` and (if drawn) ``src.idx``."""
    src = BatchSource(*src)
    if src.gauss_T > 0:
        gauss_batch(src.pool, rng, src.site, src.noise_site, src.gauss_T, x_t, src.target, t, src.idx, src.draw_idx,
                    idx_step=src.idx_step)
        return
    cold_batch(src.pool, rng, src.site, x_t, src.target, t, src.idx, src.max_t, src.draw_idx, idx_step=src.idx_step)
    if src.target_x0:
        torch.index_select(src.pool, 0, stepped_idx(src.idx, src.idx_step, x_t.shape[0]), out=src.target)
