"""Truths, operands and bounds for the LayerNorm family: ``layernorm_fwd`` /
``layernorm_bwd`` (csrc/layernorm.hip), the fold weights of ``ln_fold_`` and the GEMM
epilogues that consume a folded LayerNorm (csrc/gemm_epi.h).

Two kinds of output, two kinds of bound:

* **bf16-valued outputs** (``y``, ``gy``, ``gp``, ``y_out``, the folded consumers' outputs --
  their fp32 variants too, whose error is the bf16 rounding of the *operands*) are judged
  like the attention kernels (:mod:`.check`): against an fp64 truth, bounded by a multiple
  of the distance the bf16-mirroring reference keeps from the same truth (frob 2x, maxn 3x).
  Drop sets are compared exactly.
* **fp32-valued outputs** (``mean``, ``rstd``, ``g_out``, ``dgamma``, ``dbeta``, ``c``, ``bf``,
  row-statistics slots) carry no bf16 rounding: kernel and mirror differ by summation order
  only, both sit a few fp32 ulps from the truth, and a ratio of two such distances would
  flake.  They get an a-priori bound per element (:func:`term_bound`):

      ``16 * 2^-24 *`` (sum of the absolute values of the terms that make the element),

  the term sum taken in fp64 from the operands the op was given.  2^-24 is the fp32 unit
  roundoff; the factor 16 covers a log-depth reduction of up to 1,024 terms (10 levels), the
  roundings of the terms themselves and the few operations after the reduction.  It is a
  condition, not a measurement: tests/test_ln_check_cpu.py shows the fp32 reference under a
  quarter of it on every shape of the GPU grids.  For ``rstd`` from ``E[x^2] - mean^2`` the
  bound is relative: ``16 * 2^-24 * (1 + r^2)`` with ``r = |mean| / std`` of the row, since
  the subtraction cancels ``mean^2`` out of ``std^2 + mean^2``.

What the fold costs (asserted on the reference in tests/test_ln_check_cpu.py): the folded
GEMM multiplies ``bf16(x)``, rounded relative to ``|x| ~ |mean|``, not the normalised value;
against :func:`fold_truth` its error is ``sqrt(2 + r^2)`` times that of LayerNorm -> bf16 ->
GEMM, up to a few per cent.

Verdicts are appended to the file named by ``DDIM_COLD_LN_ERROR_LOG`` (profiles/ln_error.txt).
Pure PyTorch and device-agnostic; truths and mirrors are computed on the CPU.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Sequence

import torch

from . import check
from . import reference as ref

LOG_ENV = "DDIM_COLD_LN_ERROR_LOG"
U32 = 2.0 ** -24       # fp32 unit roundoff
TERM_FACTOR = 16.0
REF_SHARE = 0.25       # the fp32 reference stays under this share of every term bound

# shape grids of tests/test_layernorm_gpu.py and tests/test_ln_fold_gpu.py (the CPU tests run
# the reference through the same ones)
LN_DS = (128, 256, 384, 512, 768, 1024)
LN_FWD_MS = (1, 3, 4, 5)         # around the 4 rows per forward workgroup
LN_BWD_MS = (1, 7, 8, 9)         # around the 8 rows per backward workgroup
LN_BWD_STRIDED_M = 4107          # > 8 * 512: the workgroup-strided second pass, ragged group
FOLD_RS = (0.0, 1.0, 4.0, 16.0)
FOLD_KS = (128, 256, 384, 512)
FOLD_M, FOLD_NOUT, FOLD_QKV = 264, 192, (8, 33)  # QKV: B, N (hd = 64)
FOLD_EDGE_ROWS = (1, 7, 9, 15, 17, 33)


def _log(line: str):
    path = os.environ.get(LOG_ENV)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _cpu64(t):
    return None if t is None else t.detach().double().cpu()


# ----------------------------------------------------------------------------- operands
def off_centre_rows(M: int, K: int, r: float, gen: torch.Generator) -> torch.Tensor:
    """fp32 rows [M, K] with standard deviation 1 and mean ``+r`` (even rows) / ``-r`` (odd
    rows), drawn on the CPU from ``gen`` and standardised in fp64: |mean| / std = r."""
    z = torch.randn(M, K, generator=gen, dtype=torch.float64)
    z = z - z.mean(-1, keepdim=True)
    z = z / z.pow(2).mean(-1, keepdim=True).sqrt()
    sign = 1.0 - 2.0 * (torch.arange(M) % 2).double()
    return (z + r * sign.unsqueeze(1)).float()


def constant_rows(M: int, K: int) -> torch.Tensor:
    """fp32 rows whose K elements all hold one bf16-representable value (var = 0): values of
    both signs from 0.75 to 96, so fp32 ``E[x^2] - mean^2`` lands on either side of zero."""
    v = torch.tensor([0.75, -1.5, 3.0, -5.0, 11.0, -23.0, 48.0, -96.0])[torch.arange(M) % 8]
    v = v * (1.0 + 0.125 * ((torch.arange(M) // 8) % 4).float())  # 8-bit significands: exact in bf16
    assert torch.equal(v.bfloat16().float(), v)
    return v.unsqueeze(1).expand(M, K).contiguous()


def fp32_constant_rows(M: int, K: int) -> torch.Tensor:
    """Rows of one fp32 value each that is *not* a short significand (about 100 to 400): the
    true variance is 0 and fp32 ``E[x^2] - mean^2`` is rounding residue of either sign, around
    1e-3 >> eps -- the rows on which the clamp at zero decides between rstd <= eps^-1/2 and NaN."""
    v = (100.3 * (1.0 + torch.arange(M, dtype=torch.float64) / 97.0)).float()
    return (v * (1.0 - 2.0 * (torch.arange(M) % 2).float())).unsqueeze(1).expand(M, K).contiguous()


def assert_clamped_rstd(rstd, eps: float, name: str = ""):
    """At a constant row the computed variance is clamped at zero, so 0 < rstd <= eps^-1/2
    (to an fp32 rounding of the reciprocal square root); without the clamp it is NaN or larger."""
    r = _cpu64(rstd)
    top = eps ** -0.5 * (1.0 + 4 * U32)
    bad = int((~((r > 0) & (r <= top))).sum())
    line = f"{name}: {bad} of {r.numel()} rows with rstd outside (0, eps^-1/2] (max {float(r.nan_to_num(float('inf')).max()):.4f})"
    _log(line + ("" if bad == 0 else "  FAILED clamp"))
    assert bad == 0, line


# ----------------------------------------------------------------------------- truths
def ln_truth(x, gamma, beta, eps: float):
    """fp64 ``(y, mean, rstd)`` of LayerNorm over the last dim, no bf16 rounding."""
    xf = _cpu64(x).reshape(-1, x.shape[-1])
    mean = xf.mean(-1)
    var = (xf - mean.unsqueeze(1)).pow(2).mean(-1)
    rstd = (var + eps).rsqrt()
    y = (xf - mean.unsqueeze(1)) * rstd.unsqueeze(1) * _cpu64(gamma) + _cpu64(beta)
    return y, mean, rstd


def fold_truth(x, w, gamma, beta, bias, eps: float):
    """fp64 ``LayerNorm(x) @ w.T + bias``: ``x`` the fp32 rows, ``w`` the weight the fold was
    built from (fp32 master, or the bf16 shadow upcast)."""
    y, _, _ = ln_truth(x, gamma, beta, eps)
    out = y @ _cpu64(w).t()
    return out if bias is None else out + _cpu64(bias)


def unfolded_mirror(x, w, gamma, beta, bias, eps: float):
    """LayerNorm -> bf16 -> GEMM in fp32 on the weights as given: the one rounding the
    unfolded path cannot avoid, the yardstick of the sqrt(2 + r^2) law."""
    y, _, _ = ref.layernorm_fwd(x.cpu(), gamma.cpu(), beta.cpu(), eps)
    return ref._lin(y, w.cpu(), None if bias is None else bias.cpu())


class LnBwdTruth(NamedTuple):
    g_out: torch.Tensor    # [M, D] fp64
    dgamma: torch.Tensor   # [D]: the column sums alone (what the op adds)
    dbeta: torch.Tensor
    gy: torch.Tensor       # [M, D]: g_out with the branch dropout and the drop-path scale
    gp: Optional[torch.Tensor]  # [B*(N-1), D]: patch rows with the embedding dropout (N > 1)
    t_g_out: torch.Tensor  # the term sums :func:`term_bound` takes
    t_dgamma: torch.Tensor
    t_dbeta: torch.Tensor


def ln_bwd_truth(dy_parts, x, mean, rstd, gamma, g_res, N: int, rng, sites: Sequence[int], ps: Sequence[float]):
    """fp64 LayerNorm backward from the tensors the op is given: ``dy_parts`` ([P, M, D] or
    [M, D], fp32 or bf16, summed), ``x`` as passed (fp32, or the bf16 copy upcast), the given
    ``mean`` / ``rstd``.  ``sites`` / ``ps`` = (branch dropout, drop-path, embedding dropout);
    the masks are :mod:`.reference`'s (``_dropout``, ``_sample_scale``)."""
    D = x.shape[-1]
    xf = _cpu64(x).reshape(-1, D)
    M = xf.shape[0]
    parts = _cpu64(dy_parts).reshape(-1, M, D)
    dy, dy_abs = parts.sum(0), parts.abs().sum(0)
    mu, rs, gam = _cpu64(mean).reshape(M, 1), _cpu64(rstd).reshape(M, 1), _cpu64(gamma)
    xh = (xf - mu) * rs
    dxh = dy * gam
    c1, c2 = dxh.mean(-1, keepdim=True), (dxh * xh).mean(-1, keepdim=True)
    g_out = (dxh - c1 - xh * c2) * rs
    adxh = dy_abs * gam.abs()
    t_g = rs * (adxh + adxh.mean(-1, keepdim=True) + xh.abs() * (adxh * xh.abs()).mean(-1, keepdim=True))
    if g_res is not None:
        gr = _cpu64(g_res).reshape(M, D)
        g_out, t_g = g_out + gr, t_g + gr.abs()
    rng = rng.cpu()
    (s_drop, s_dp, s_emb), (p_drop, p_dp, p_emb) = sites, ps
    B = M // N
    keep = (ref._sample_scale(B, rng, s_dp, p_dp, "cpu") != 0).double() / (1.0 - p_dp)
    gy = ref._dropout(g_out, rng, s_drop, p_drop) * keep.repeat_interleave(N).unsqueeze(1)
    gp = None
    if N > 1:
        gp = ref._dropout(g_out.view(B, N, D), rng, s_emb, p_emb)[:, 1:, :].reshape(B * (N - 1), D)
    return LnBwdTruth(g_out, (dy * xh).sum(0), dy.sum(0), gy, gp, t_g, (dy_abs * xh.abs()).sum(0), dy_abs.sum(0))


# ----------------------------------------------------------------------------- a-priori bounds
def term_bound(terms: torch.Tensor) -> torch.Tensor:
    """Per-element bound of an fp32-valued output from the sum of the absolute values of the
    terms that make it (fp64): ``16 * 2^-24 * terms``."""
    return TERM_FACTOR * U32 * terms.double()


def mean_terms(x) -> torch.Tensor:
    xf = _cpu64(x).reshape(-1, x.shape[-1])
    return xf.abs().mean(-1)


def rstd_terms(mean_t: torch.Tensor, rstd_t: torch.Tensor) -> torch.Tensor:
    """``rstd (1 + r^2)``, r = |mean| rstd per row from the truth (the relative bound as a term sum)."""
    return rstd_t * (1.0 + (mean_t * rstd_t).pow(2))


def slot_terms(x) -> torch.Tensor:
    """Term sums of the row-statistics slots [M, D/32, 2]: sum |x| and sum x^2 per slot."""
    xs = _cpu64(x).reshape(-1, x.shape[-1] // ref.LN_SLOT, ref.LN_SLOT)
    return torch.stack((xs.abs().sum(-1), xs.pow(2).sum(-1)), dim=-1)


def c_terms(wf) -> torch.Tensor:
    return _cpu64(wf).abs().sum(-1)


def bf_terms(w, beta, bias) -> torch.Tensor:
    t = (_cpu64(w) * _cpu64(beta)).abs().sum(-1)
    return t if bias is None else t + _cpu64(bias).abs()


def term_ratio(got, truth, terms) -> float:
    """max over elements of |got - truth| / term_bound(terms); inf for a NaN, 0 where both vanish."""
    err = (_cpu64(got).reshape(truth.shape) - truth).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    bound = term_bound(terms).reshape(truth.shape)
    ratio = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    return float(ratio.max()) if ratio.numel() else 0.0


def assert_terms(got, truth, terms, name: str = "", share: float = 1.0) -> float:
    """``|got - truth| <= share * term_bound(terms)`` on every element; returns the worst ratio."""
    ratio = term_ratio(got, truth, terms)
    line = f"{name}: {ratio:.3f} of the term bound (<= {share:g})"
    _log(line + ("" if ratio <= share else "  FAILED term"))
    assert ratio <= share, line
    return ratio


# ----------------------------------------------------------------------------- mirror-relative
def judge(kernel, mirror, truth, name: str = "") -> check.Verdict:
    """:func:`check.judge` on CPU fp64 copies, logged to ``DDIM_COLD_LN_ERROR_LOG``."""
    t = _cpu64(truth)
    v = check.judge(_cpu64(kernel).reshape(t.shape), _cpu64(mirror).reshape(t.shape), t, name)
    _log(v.line())
    return v


def assert_within(kernel, mirror, truth, name: str = "") -> check.Verdict:
    """bf16-valued outputs: frob <= 2x, maxn <= 3x the mirror's distance from the truth."""
    v = judge(kernel, mirror, truth, name)
    assert not v.failed, v.line()
    return v


def assert_drop_set(kernel, mirror, name: str = ""):
    assert torch.equal(kernel.cpu() == 0, mirror.cpu() == 0), f"{name}: drop set differs from the reference's"


# ----------------------------------------------------------------------------- op runs
# One function per grid of the GPU tests: operands from a CPU generator, the op through
# :mod:`ddim_cold_amd.ops` on ``device`` (HIP kernels on a GPU, :mod:`.reference` on the CPU),
# truths and mirrors on the CPU.  ``share``: the share of the term bounds asserted (1 for the
# kernels, REF_SHARE for the reference on the CPU).
def _ops():
    import ddim_cold_amd.ops as ops
    return ops


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _rng(device, seed: int = 1234, step: int = 5):
    return torch.tensor([seed, step], dtype=torch.int64, device=device)


def _affine(D: int, g):
    return 1.0 + 0.3 * torch.randn(D, generator=g), 0.3 * torch.randn(D, generator=g)


def run_ln_fwd(M: int, D: int, r: float, device, share: float = 1.0, seed: int = 20):
    ops, g = _ops(), _gen(seed)
    x = off_centre_rows(M, D, r, g)
    gam, bet = _affine(D, g)
    name = f"layernorm_fwd M={M} D={D} r={r:g}"
    y, mean, rstd = ops.layernorm_fwd(x.to(device), gam.to(device), bet.to(device), 1e-5)
    yt, mt, rt = ln_truth(x, gam, bet, 1e-5)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape and mean.shape == rstd.shape == (M,)
    assert_within(y, ref.layernorm_fwd(x, gam, bet, 1e-5)[0], yt, name + " y")
    assert_terms(mean, mt, mean_terms(x), name + " mean", share)
    assert_terms(rstd, rt, rstd_terms(mt, rt), name + " rstd", share)


class LnBwdCase(NamedTuple):
    M: int
    D: int
    N: int                 # tokens per sample (M % N == 0)
    dy_bf16: bool = False
    x_bf16: bool = False
    parts: int = 1
    g_res: bool = True
    p: float = 0.0         # branch dropout, drop-path and embedding dropout alike
    y_out: bool = False
    gp: bool = False
    ws: bool = False       # workspace slots + replica_reduce_ instead of accumulating
    r: float = 0.5

    def name(self) -> str:
        return "layernorm_bwd " + " ".join(f"{k}={v}" for k, v in self._asdict().items())


def ln_bwd_cases():
    """The grid of tests/test_layernorm_gpu.py (every case a fraction of a second)."""
    cs = []
    for i, D in enumerate(LN_DS):  # every width; y_out + beta once per width, both reductions
        cs.append(LnBwdCase(40, D, 5, p=0.1, y_out=True, gp=True, ws=bool(i % 2)))
        cs.append(LnBwdCase(40, D, 5, dy_bf16=True, x_bf16=True, parts=4, g_res=False, ws=not i % 2))
    for M in LN_BWD_MS:            # around the 8-row group
        cs.append(LnBwdCase(M, 128, 1, p=0.1, ws=bool(M % 2)))
    cs.append(LnBwdCase(LN_BWD_STRIDED_M, 128, 37, p=0.1, gp=True, ws=True))
    cs.append(LnBwdCase(LN_BWD_STRIDED_M, 128, 37, dy_bf16=True, parts=4))
    for N in (2, 5, 40):           # tokens = 2, 5, M with gp_out
        for p in (0.0, 0.1):
            cs.append(LnBwdCase(40, 128, N, p=p, gp=True, ws=N == 5))
    for dyb in (False, True):      # the four kernels x {1, 4} partials x with / without g_res
        for xb in (False, True):
            for parts in (1, 4):
                cs.append(LnBwdCase(41, 256, 41, dyb, xb, parts, g_res=parts == 1, p=0.1 if xb else 0.0,
                                    gp=True, ws=dyb))
    return cs


def run_ln_bwd(case: LnBwdCase, device, share: float = 1.0, seed: int = 21):
    """``layernorm_bwd`` against :func:`ln_bwd_truth`.  ``dgamma`` / ``dbeta`` (and the
    workspace) sit in canaried buffers and start from non-zero values; the workspace path
    runs twice and must be bit-identical."""
    from . import gemm_check as gc
    ops, g = _ops(), _gen(seed)
    M, D, N = case.M, case.D, case.N
    name = case.name()
    x32 = off_centre_rows(M, D, case.r, g) * 1.5
    gam, bet = _affine(D, g)
    _, mean, rstd = ref.layernorm_fwd(x32, gam, bet, 1e-5)
    x = x32.to(torch.bfloat16) if case.x_bf16 else x32
    dy = torch.randn(case.parts, M, D, generator=g)
    dy = dy.to(torch.bfloat16) if case.dy_bf16 else dy
    if case.parts == 1:
        dy = dy[0]
    g_res = torch.randn(M, D, generator=g) if case.g_res else None
    dg0, db0 = torch.randn(D, generator=g), torch.randn(D, generator=g)
    sites, ps = (7, 8, 9), (case.p, case.p, case.p)
    B = M // N
    on_gpu = torch.device(device).type != "cpu"

    def dev(t):
        return None if t is None else t.to(device)

    def launch():
        # dgamma || dbeta in one canaried buffer (the layout the slot finalize adds into)
        dst, dst_ok = gc.canary((2 * D,), 64, torch.float32, device)
        dst.copy_(torch.cat((dg0, db0)))
        dg, db = dst[:D], dst[D:]
        R = ops.ln_ws_rows(M)
        ws = ws_ok = ws_bits = None
        if case.ws:
            ws, ws_ok = gc.canary((R, 2 * D), 2 * D, torch.float32, device)
            if not on_gpu:
                ws.zero_()  # the reference accumulates into row 0
        y_out = torch.empty(M, D, dtype=torch.bfloat16, device=device) if case.y_out else None
        gp = torch.empty(B * (N - 1), D, dtype=torch.bfloat16, device=device) if case.gp and N > 1 else None
        g_out, gy = ops.layernorm_bwd(dev(dy), dev(x), dev(mean), dev(rstd), dev(gam), dev(g_res), dg, db, N,
                                      _rng(device), sites[0], ps[0], sites[1], ps[1], True, ws=ws,
                                      beta=dev(bet) if case.y_out else None, y_out=y_out, gp_out=gp,
                                      site_emb=sites[2], p_emb=ps[2])
        if case.ws:
            assert gc.mismatches(dst, torch.cat((dg0, db0)).to(device)).shape[0] == 0, \
                name + ": the workspace path wrote dgamma / dbeta"
            ws_bits = gc._bits(ws).clone()
            ptrs = torch.tensor([dst.data_ptr()], dtype=torch.int64, device=device) if on_gpu else None
            ops.replica_reduce_(ws.view(1, R, 2 * D), ptrs, 2 * D, R, dsts=[dst])
            ws_ok(name + " ws")
        dst_ok(name + " dgamma || dbeta")
        return g_out, gy, dg.clone(), db.clone(), y_out, gp, ws_bits

    g_out, gy, dg, db, y_out, gp, ws_bits = launch()
    t = ln_bwd_truth(dy, x, mean, rstd, gam, g_res, N, _rng("cpu"), sites, ps)
    dgm, dbm = torch.zeros(D), torch.zeros(D)
    gom, gym = ref.layernorm_bwd(dy, x, mean, rstd, gam, g_res, dgm, dbm, N, _rng("cpu"), sites[0], ps[0],
                                 sites[1], ps[1], True)
    assert_terms(g_out, t.g_out, t.t_g_out, name + " g_out", share)
    assert_terms(dg, t.dgamma + dg0.double(), t.t_dgamma + dg0.double().abs(), name + " dgamma", share)
    assert_terms(db, t.dbeta + db0.double(), t.t_dbeta + db0.double().abs(), name + " dbeta", share)
    assert_within(gy, gym, t.gy, name + " gy")
    assert_drop_set(gy, gym, name + " gy")
    if gp is not None:
        gpm = ref.embed_patch_grad(gom.view(B, N, D), _rng("cpu"), sites[2], ps[2])
        assert_within(gp, gpm, t.gp, name + " gp")
        assert_drop_set(gp, gpm, name + " gp")
    if y_out is not None:
        ym = torch.empty(M, D, dtype=torch.bfloat16)
        ref.layernorm_out_(x, mean, rstd, gam, bet, ym)
        yt = (_cpu64(x) - _cpu64(mean).unsqueeze(1)) * _cpu64(rstd).unsqueeze(1) * gam.double() + bet.double()
        assert_within(y_out, ym, yt, name + " y_out")
    if case.ws:
        again = launch()
        assert torch.equal(again[6], ws_bits), name + ": workspace slots differ between two launches"
        for a, b, what in ((again[0], g_out, "g_out"), (again[2], dg, "dgamma"), (again[3], db, "dbeta")):
            assert gc.mismatches(a, b).shape[0] == 0, f"{name}: {what} differs between two launches"


def run_ln_chain(device, share: float = 1.0, seed: int = 22):
    """The training chain at M = 130, D = 128: ``ln_mean`` / ``ln_rstd`` from a folded
    ``qkv_fwd`` feed ``layernorm_bwd`` with the bf16 ``x``; judged against the fp64 LayerNorm
    backward of the fp32 ``x``, the mirror being the same chain through the reference."""
    ops, g = _ops(), _gen(seed)
    B, N, H, D = 2, 65, 2, 128
    M = B * N
    x = off_centre_rows(M, D, 1.0, g)
    gam, bet = _affine(D, g)
    w, b = torch.randn(3 * D, D, generator=g) * 0.05, torch.randn(3 * D, generator=g)
    dy, g_res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)

    def chain(dv):
        wf = torch.empty(3 * D, D, dtype=torch.bfloat16, device=dv)
        c, bf = torch.empty(3 * D, device=dv), torch.empty(3 * D, device=dv)
        ops.ln_fold_([w.to(dv)], [gam.to(dv)], [bet.to(dv)], [b.to(dv)], [wf], [c], [bf])
        xd = x.to(dv)
        mean, rstd = torch.empty(M, device=dv), torch.empty(M, device=dv)
        ops.qkv_fwd(xd.to(torch.bfloat16), wf, bf, B, N, H, fold=(ref.row_stats(xd), c, 1e-5, mean, rstd))
        dg, db = torch.zeros(D, device=dv), torch.zeros(D, device=dv)
        g_out, gy = ops.layernorm_bwd(dy.to(dv), xd.to(torch.bfloat16), mean, rstd, gam.to(dv), g_res.to(dv), dg, db,
                                      N, _rng(dv), 7, 0.0, 8, 0.0, True)
        return g_out, gy, dg, db

    _, mt, rt = ln_truth(x, gam, bet, 1e-5)
    t = ln_bwd_truth(dy, x, mt, rt, gam, g_res, N, _rng("cpu"), (7, 8, 9), (0.0, 0.0, 0.0))
    got, mir = chain(device), chain("cpu")
    for k, m, tr, what in zip(got, mir, (t.g_out, t.gy, t.dgamma, t.dbeta), ("g_out", "gy", "dgamma", "dbeta")):
        assert_within(k, m, tr, f"chain folded qkv_fwd -> layernorm_bwd (bf16 x) {what}")


class FoldOperands(NamedTuple):
    x: torch.Tensor       # fp32 rows (CPU)
    w: torch.Tensor       # the weight the fold was built from: fp32, or bf16 (the shadow)
    gamma: torch.Tensor
    beta: torch.Tensor
    bias: torch.Tensor


def fold_operands(M: int, K: int, Nout: int, r: float, bf16_w: bool, g, x=None) -> FoldOperands:
    x = off_centre_rows(M, K, r, g) if x is None else x
    w = torch.randn(Nout, K, generator=g) * 0.05
    gam, bet = _affine(K, g)
    return FoldOperands(x, w.to(torch.bfloat16) if bf16_w else w, gam, bet, torch.randn(Nout, generator=g))


def fold_on(o: FoldOperands, dv, st=None):
    """``(xb, st, wf, c, bf)`` on device ``dv``: the folded GEMM's operands from ``ops.ln_fold_``."""
    ops = _ops()
    Nout, K = o.w.shape
    wf = torch.empty(Nout, K, dtype=torch.bfloat16, device=dv)
    c, bf = torch.empty(Nout, device=dv), torch.empty(Nout, device=dv)
    ops.ln_fold_([o.w.to(dv)], [o.gamma.to(dv)], [o.beta.to(dv)], [o.bias.to(dv)], [wf], [c], [bf])
    xd = o.x.to(dv)
    return xd.to(torch.bfloat16), (ref.row_stats(xd) if st is None else st.to(dv)), wf, c, bf


def _fold_consumers(o: FoldOperands, oq: FoldOperands, dv, eps: float):
    """Every folded consumer's output as GEMM rows ([M, Nout]; QKV from ``oq``, whose weight
    is [3 K, K]), and the returned (mean, rstd) of the two ops that return them."""
    from .gemm_check import _qkv_rows
    ops = _ops()
    xb, st, wf, c, bf = fold_on(o, dv)
    M, K = xb.shape
    (B, N), H = FOLD_QKV, K // 64
    assert B * N == M and oq.w.shape[0] == 3 * K
    _, _, wfq, cq, bfq = fold_on(oq, dv)
    mean, rstd = torch.empty(M, device=dv), torch.empty(M, device=dv)
    out = {"qkv": _qkv_rows(ops.qkv_fwd(xb, wfq, bfq, B, N, H, fold=(st, cq, eps, mean, rstd)))}
    m2, r2 = torch.empty(M, device=dv), torch.empty(M, device=dv)
    u, h = ops.linear_gelu_fwd(xb, wf, bf, _rng(dv), 9, 0.0, fold=(st, c, eps, m2, r2))
    out["gelu u"], out["gelu h"] = u, h
    out["linear bf16"] = ops.linear_fwd(xb, wf, bf, False, fold=(st, c, eps))
    out["linear f32"] = ops.linear_fwd(xb, wf, bf, True, fold=(st, c, eps))
    return out, (mean, rstd), (m2, r2)


def run_fold_consumers(K: int, r: float, bf16_w: bool, device, share: float = 1.0, seed: int = 23):
    """``qkv_fwd`` (Nout = 3 K), ``linear_gelu_fwd`` (u, h) and ``linear_fwd`` (bf16 / f32;
    Nout = 192) with ``fold=`` on off-centre rows against :func:`fold_truth`, the folded
    reference as mirror."""
    g = _gen(seed)
    o = fold_operands(FOLD_M, K, FOLD_NOUT, r, bf16_w, g)
    oq = fold_operands(FOLD_M, K, 3 * K, r, bf16_w, g, x=o.x)
    name = f"fold K={K} r={r:g} {'bf16' if bf16_w else 'fp32'} weights"
    truth, truth_q = fold_truth(*o, 1e-5), fold_truth(*oq, 1e-5)
    got, ms, ms2 = _fold_consumers(o, oq, device, 1e-5)
    mir, _, _ = _fold_consumers(o, oq, "cpu", 1e-5)
    for k in got:
        tr = truth_q if k == "qkv" else (truth if k != "gelu h" else ref.gelu(truth))
        assert_within(got[k], mir[k], tr, f"{name} {k}")
    _, mt, rt = ln_truth(o.x, o.gamma, o.beta, 1e-5)
    for (m, rs), who in ((ms, "qkv"), (ms2, "gelu")):
        assert_terms(m, mt, mean_terms(o.x), f"{name} {who} ln_mean", share)
        assert_terms(rs, rt, rstd_terms(mt, rt), f"{name} {who} ln_rstd", share)
    return got


HEAD_FOLD_GEOM = (4, 3, 16, 16, 4, 128)  # B, C, H, W, p, D


def run_fold_head(r: float, device, share: float = 1.0, seed: int = 24):
    """``head_fwd`` with ``fold=`` (D = 128, 16x16, p = 4) against :func:`fold_truth`."""
    from .gemm_check import _rows_to_head_image
    ops, g = _ops(), _gen(seed)
    B, C, H, W, p, D = HEAD_FOLD_GEOM
    M = B * ((H // p) * (W // p) + 1)
    o = fold_operands(M, D, C * p * p, r, False, g)
    name = f"fold head_fwd r={r:g}"

    def run(dv):
        xb, st, wf, c, bf = fold_on(o, dv)
        mean, rstd = torch.empty(M, device=dv), torch.empty(M, device=dv)
        return ops.head_fwd(xb, wf, bf, B, C, H, W, p, fold=(st, c, 1e-5, mean, rstd)), mean, rstd

    (img, mean, rstd), (imgm, _, _) = run(device), run("cpu")
    assert_within(img, imgm, _rows_to_head_image(fold_truth(*o, 1e-5), B, C, H, W, p), name)
    _, mt, rt = ln_truth(o.x, o.gamma, o.beta, 1e-5)
    assert_terms(mean, mt, mean_terms(o.x), name + " ln_mean", share)
    assert_terms(rstd, rt, rstd_terms(mt, rt), name + " ln_rstd", share)


def run_fold_constant_rows(K: int, device, share: float = 1.0, seed: int = 25):
    """Constant rows (var = 0, rstd = eps^-1/2 ~ 316): ``c`` must cancel what the GEMM
    accumulated, so the output is ``bf`` within ``316 * 16 * 2^-24 * |v| * sum_k |wf|``."""
    ops, g = _ops(), _gen(seed)
    eps = 1e-5
    o = fold_operands(FOLD_M, K, FOLD_NOUT, 0.0, False, g, x=constant_rows(FOLD_M, K))
    xb, st, wf, c, bf = fold_on(o, device)
    y = ops.linear_fwd(xb, wf, bf, True, fold=(st, c, eps))
    terms = eps ** -0.5 * o.x[:, :1].double().abs() * c_terms(wf).unsqueeze(0)
    truth = _cpu64(bf).unsqueeze(0).expand(FOLD_M, -1)
    worst = assert_terms(y, truth, terms, f"fold K={K} constant rows: output = bf", share)
    # rows whose fp32 E[x^2] - mean^2 is rounding residue of either sign: the clamp at zero
    xd = fp32_constant_rows(FOLD_M, K).to(device)
    mean, rstd = torch.empty(FOLD_M, device=device), torch.empty(FOLD_M, device=device)
    u, _ = ops.linear_gelu_fwd(xd.to(torch.bfloat16), wf, bf, _rng(device), 9, 0.0,
                               fold=(ref.row_stats(xd), c, eps, mean, rstd))
    assert_clamped_rstd(rstd, eps, f"fold K={K} fp32-constant rows: variance clamped at zero")
    assert bool(torch.isfinite(u.float()).all()), f"fold K={K} fp32-constant rows: non-finite output"
    return worst


def run_fold_producer_chain(device, share: float = 1.0, seed: int = 26):
    """``linear_residual_fwd(..., st_out, xb_out)`` (K = Nout = 128, M = 130, tokens = 65) with
    a residual at r = 4 feeding ``qkv_fwd(fold=)``: the statistics under test are the
    producer kernel's own.  The truth follows the kernel's own fp32 rows."""
    from .gemm_check import _qkv_rows
    ops, g = _ops(), _gen(seed)
    M, tokens, K, H = 130, 65, 128, 2
    B = M // tokens
    xres = off_centre_rows(M, K, 4.0, g)
    a = (torch.randn(M, K, generator=g) * 0.5).to(torch.bfloat16)
    wr, br = (torch.randn(K, K, generator=g) * 0.05).to(torch.bfloat16), torch.randn(K, generator=g) * 0.1
    o = fold_operands(M, K, 3 * K, 0.0, False, g)  # its rows are replaced by the producer's
    name = "fold producer chain linear_residual_fwd -> qkv_fwd"
    st = torch.full((M, K // 32, 2), float("nan"), device=device)  # every slot must be written
    xb = torch.empty(M, K, dtype=torch.bfloat16, device=device)
    x = ops.linear_residual_fwd(a.to(device), wr.to(device), br.to(device), xres.to(device), tokens, _rng(device),
                                3, 0.0, 4, 0.0, st_out=st, xb_out=xb)
    xk = x.detach().float().cpu()
    assert gc_equal(xb, xk.to(torch.bfloat16)), name + ": xb_out is not bf16(x)"
    xs = xk.double().reshape(M, K // ref.LN_SLOT, ref.LN_SLOT)
    assert_terms(st, torch.stack((xs.sum(-1), xs.pow(2).sum(-1)), dim=-1), slot_terms(xk), name + " st_out", share)
    ok = o._replace(x=xk)

    def consume(dv, stats):
        _, st_d, wf, c, bf = fold_on(ok, dv, stats)
        mean, rstd = torch.empty(M, device=dv), torch.empty(M, device=dv)
        xbd = xk.to(dv).to(torch.bfloat16)
        return _qkv_rows(ops.qkv_fwd(xbd, wf, bf, B, tokens, H, fold=(st_d, c, 1e-5, mean, rstd))), mean, rstd

    out, mean, rstd = consume(device, st)
    mirror, _, _ = consume("cpu", None)  # the reference consumer on the same rows, its own statistics
    _, mt, rt = ln_truth(xk, o.gamma, o.beta, 1e-5)
    assert_terms(mean, mt, mean_terms(xk), name + " ln_mean", share)
    assert_terms(rstd, rt, rstd_terms(mt, rt), name + " ln_rstd", share)
    assert_within(out, mirror, fold_truth(xk, o.w, o.gamma, o.beta, o.bias, 1e-5), name + " output")


def gc_equal(a, b) -> bool:
    from .gemm_check import mismatches
    return mismatches(a.cpu(), b.cpu()).shape[0] == 0


FOLD_EDGE_KS = ((4, False), (36, False), (100, False), (128, False), (512, False),   # (K, bf16 weights)
                (36, True), (100, True),                                            # 4-wide bf16 path
                (8, True), (128, True), (512, True))                                # ln_fold16 (K % 8 == 0)
FOLD_MAX_JOBS = 32  # csrc/kernels.h FOLD_MAX


def run_ln_fold_edges(K: int, bf16_w: bool, device, rows: Sequence[int] = FOLD_EDGE_ROWS, share: float = 1.0,
                      seed: int = 27):
    """``ln_fold_``: ``rows`` as consecutive jobs of one launch (alternate jobs without bias),
    every output in a canary.  ``wf`` bit-equal to ``bf16(gamma * w)``; ``c`` against the fp64
    sum of the *returned* ``wf`` (its contract: the sum of the bf16 values the MFMA multiplies)
    and ``bf`` against fp64 ``bias + w beta``, both at :func:`term_bound`."""
    from . import gemm_check as gc
    ops, g = _ops(), _gen(seed)
    jobs, outs = [], []
    for i, R in enumerate(rows):
        w = torch.randn(R, K, generator=g)
        w = w.to(torch.bfloat16) if bf16_w else w
        gam, bet = _affine(K, g)
        jobs.append((w, gam, bet, torch.randn(R, generator=g) if i % 2 == 0 else None))
        outs.append((gc.canary((R, K), 4 * K, torch.bfloat16, device), gc.canary((R,), 64, torch.float32, device),
                     gc.canary((R,), 64, torch.float32, device)))

    def dev(t):
        return None if t is None else t.to(device)

    ops.ln_fold_(*[[dev(t) for t in z] for z in zip(*jobs)], *[[o[0] for o in z] for z in zip(*outs)])
    worst = 0.0
    for i, ((w, gam, bet, b), ((wf, wf_ok), (c, c_ok), (bf, bf_ok))) in enumerate(zip(jobs, outs)):
        name = f"ln_fold_ K={K} {'bf16' if bf16_w else 'fp32'} weights job {i} of {len(rows)} ({w.shape[0]} rows)"
        gc.assert_exact(wf.cpu(), (w.float() * gam).to(torch.bfloat16), name + " wf")
        worst = max(worst, assert_terms(c, _cpu64(wf).sum(-1), c_terms(wf), name + " c", share))
        truth = w.double() @ bet.double() + (0.0 if b is None else b.double())
        worst = max(worst, assert_terms(bf, truth, bf_terms(w, bet, b), name + " bf", share))
        for ok, what in ((wf_ok, "wf"), (c_ok, "c"), (bf_ok, "bf")):
            ok(f"{name} {what}")
    return worst
