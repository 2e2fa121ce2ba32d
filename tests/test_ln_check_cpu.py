"""The LayerNorm checks (ops/ln_check.py) on the CPU: the fp32 reference passes every grid of
tests/test_layernorm_gpu.py and tests/test_ln_fold_gpu.py at under a quarter of every
a-priori term bound, each kernel-shaped mutant of the reference is rejected by the check
meant to see it, and the cost of the fold -- sqrt(2 + r^2) times the unfolded error at
|mean| / std = r -- is asserted on the reference (a design limit, not a kernel property)."""
import math

import pytest
import torch

from ddim_cold_amd.ops import ln_check as lc
from ddim_cold_amd.ops import reference as ref

CPU = "cpu"
Q = lc.REF_SHARE


def _rejects(fn, match=None):
    with pytest.raises(AssertionError, match=match):
        fn()


# ----------------------------------------------------------------------------- the reference passes
def test_reference_passes_layernorm_fwd_grid():
    for r in (0.0, 16.0):
        for D in lc.LN_DS:
            lc.run_ln_fwd(37, D, r, CPU, Q)
        for M in lc.LN_FWD_MS:
            lc.run_ln_fwd(M, 128, r, CPU, Q)


def test_reference_passes_layernorm_bwd_grid():
    cases = lc.ln_bwd_cases()
    # the grid holds what the kernel can get wrong: every width, both sides of the 8-row group,
    # the strided second pass with a ragged group, tokens = 2 / 5 / M, the four kernels
    assert {c.D for c in cases} == set(lc.LN_DS) and {c.M for c in cases} >= set(lc.LN_BWD_MS) | {lc.LN_BWD_STRIDED_M}
    assert lc.LN_BWD_STRIDED_M > 8 * 512 and lc.LN_BWD_STRIDED_M % 8
    assert {(c.dy_bf16, c.x_bf16, c.parts) for c in cases} >= {(a, b, p) for a in (0, 1) for b in (0, 1) for p in (1, 4)}
    assert {c.N for c in cases if c.gp} >= {2, 5, 40} and {c.D for c in cases if c.y_out} == set(lc.LN_DS)
    for c in cases:
        lc.run_ln_bwd(c, CPU, Q)
    lc.run_ln_chain(CPU, Q)


@pytest.mark.parametrize("K", lc.FOLD_KS)
def test_reference_passes_fold_grid(K):
    for r in lc.FOLD_RS:
        for bf16_w in (False, True):
            lc.run_fold_consumers(K, r, bf16_w, CPU, Q)
    lc.run_fold_constant_rows(K, CPU, Q)


def test_reference_passes_fold_head_chain_and_edges():
    for r in lc.FOLD_RS:
        lc.run_fold_head(r, CPU, Q)
    lc.run_fold_producer_chain(CPU, Q)
    for K, bf16_w in lc.FOLD_EDGE_KS:
        lc.run_ln_fold_edges(K, bf16_w, CPU, share=Q)
    for bf16_w in (False, True):
        lc.run_ln_fold_edges(128, bf16_w, CPU, rows=(lc.FOLD_EDGE_ROWS * 6)[:lc.FOLD_MAX_JOBS], share=Q)


def test_off_centre_rows():
    g = torch.Generator().manual_seed(0)
    x = lc.off_centre_rows(6, 384, 4.0, g).double()
    assert torch.allclose(x.mean(-1), torch.tensor([4.0, -4.0] * 3, dtype=torch.float64), atol=1e-6)
    assert torch.allclose(x.var(-1, unbiased=False), torch.ones(6, dtype=torch.float64), atol=1e-5)
    c = lc.constant_rows(40, 64)
    assert bool((c == c[:, :1]).all()) and c[:, 0].unique().numel() == 32


# ----------------------------------------------------------------------------- the design curve
@pytest.mark.parametrize("K", lc.FOLD_KS)
def test_fold_error_follows_sqrt_2_plus_r2(K):
    """bf16(x) rounds relative to |x| ~ |mean|, so the folded GEMM's distance from the truth is
    sqrt(2 + r^2) times that of LayerNorm -> bf16 -> GEMM on unrounded weights (measured here at K = 384:
    1.36, 1.66, 4.21, 16.53 for r = 0, 1, 4, 16, i.e. 0.96x to 1.03x the law; 1.25x leaves room for
    other seeds and K).  Asserted on the reference: a design limit, not a kernel property."""
    for r in lc.FOLD_RS:
        g = torch.Generator().manual_seed(23)
        o = lc.fold_operands(lc.FOLD_M, K, lc.FOLD_NOUT, r, False, g)
        truth = lc.fold_truth(*o, 1e-5)
        xb, st, wf, c, bf = lc.fold_on(o, CPU)
        folded = lc.check.metrics(ref.linear_fwd(xb, wf, bf, True, st, c, 1e-5), truth).frob
        unfolded = lc.check.metrics(lc.unfolded_mirror(*o, 1e-5), truth).frob
        law = math.sqrt(2.0 + r * r)
        print(f"K={K} r={r:g}: folded / unfolded frob {folded / unfolded:.2f}, sqrt(2 + r^2) = {law:.2f}")
        assert 0.8 * law * unfolded <= folded <= 1.25 * law * unfolded, (K, r, folded / unfolded, law)


# ----------------------------------------------------------------------------- fold mutants
def _folded_linear(o, mutant=None, eps=1e-5):
    """fp32 folded ``linear_fwd`` as the epilogue computes it (statistics times the host's
    rounded 1/K), with one kernel-shaped fault."""
    xb, st, wf, c, bf = lc.fold_on(o, CPU)
    K = o.x.shape[1]
    invd = torch.tensor(1.0 / K, dtype=torch.float32)
    tot = st.sum(1)
    mu = tot[:, 0] * invd
    if mutant == "mean_from_bf16_rows":
        mu = xb.float().sum(-1) * invd
    var = tot[:, 1] * invd - mu * mu
    if mutant != "var_unclamped":
        var = var.clamp_min(0.0)
    if mutant == "c_from_unrounded_weights":
        c = (o.w.float() * o.gamma).sum(1)
    rs = torch.rsqrt(var + eps)
    return (ref._mm(xb, wf) - mu.unsqueeze(1) * c.unsqueeze(0)) * rs.unsqueeze(1) + bf, mu, rs, (wf, c, bf)


def test_mutant_mean_from_bf16_rows():
    g = torch.Generator().manual_seed(1)
    o = lc.fold_operands(lc.FOLD_M, 384, lc.FOLD_NOUT, 16.0, False, g)
    _, mt, rt = lc.ln_truth(o.x, o.gamma, o.beta, 1e-5)
    _, mu, _, _ = _folded_linear(o)
    lc.assert_terms(mu, mt, lc.mean_terms(o.x), "clean")
    _, mu, _, _ = _folded_linear(o, "mean_from_bf16_rows")
    _rejects(lambda: lc.assert_terms(mu, mt, lc.mean_terms(o.x), "mutant"), "term bound")


def test_old_tolerance_is_blind_to_mean_from_bf16_rows():
    """The previous fold tests used rows at |mean| / std = 0.25 and ``close(..., 2e-2, 1e-2)``
    against the mirror: a row mean taken from the bf16 rows passes it; the term bound on the
    returned mean rejects it at the same rows."""
    g = torch.Generator().manual_seed(2)
    x = torch.randn(lc.FOLD_M, 384, generator=g) * 2.0 + 0.5
    o = lc.fold_operands(lc.FOLD_M, 384, lc.FOLD_NOUT, 0.0, False, g, x=x)
    y, _, _, _ = _folded_linear(o)
    ym, mu, _, _ = _folded_linear(o, "mean_from_bf16_rows")
    err = (ym.bfloat16().float() - y.bfloat16().float()).abs()
    assert not torch.equal(ym, y) and bool((err <= 2e-2 + 1e-2 * y.abs()).all())
    _, mt, _ = lc.ln_truth(o.x, o.gamma, o.beta, 1e-5)
    _rejects(lambda: lc.assert_terms(mu, mt, lc.mean_terms(o.x), "mutant"), "term bound")


def test_mutant_c_from_unrounded_weights():
    """``c`` must be the sum of the bf16 values the MFMA multiplies: seen by the constant-row
    cancellation and by ``c`` against the fp64 sum of the returned ``wf``."""
    g = torch.Generator().manual_seed(3)
    eps = 1e-5
    o = lc.fold_operands(lc.FOLD_M, 384, lc.FOLD_NOUT, 0.0, False, g, x=lc.constant_rows(lc.FOLD_M, 384))
    for mutant, ok in ((None, True), ("c_from_unrounded_weights", False)):
        y, _, _, (wf, c, bf) = _folded_linear(o, mutant)
        terms = eps ** -0.5 * o.x[:, :1].double().abs() * lc.c_terms(wf).unsqueeze(0)
        checks = (lambda: lc.assert_terms(y, bf.double().unsqueeze(0).expand(lc.FOLD_M, -1), terms, "output = bf"),
                  lambda: lc.assert_terms(c, wf.double().sum(-1), lc.c_terms(wf), "c"))
        for chk in checks:
            chk() if ok else _rejects(chk, "term bound")


def test_mutant_var_unclamped_at_constant_rows():
    """Short-significand constant rows give var = 0 exactly (no clamp needed); rows of one
    full-precision fp32 value leave rounding residue of either sign, and there the clamp decides."""
    g = torch.Generator().manual_seed(4)
    o = lc.fold_operands(lc.FOLD_M, 384, lc.FOLD_NOUT, 0.0, False, g, x=lc.fp32_constant_rows(lc.FOLD_M, 384))
    y, _, rs, _ = _folded_linear(o)
    lc.assert_clamped_rstd(rs, 1e-5, "clean")
    assert bool(torch.isfinite(y).all())
    y, _, rs, _ = _folded_linear(o, "var_unclamped")
    assert int(torch.isnan(rs).sum()) > lc.FOLD_M // 8  # E[x^2] - mean^2 < -eps on many rows
    _rejects(lambda: lc.assert_clamped_rstd(rs, 1e-5, "mutant"), "outside")


# ----------------------------------------------------------------------------- backward mutants
def _bwd_operands(M, D, N, p, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = lc.off_centre_rows(M, D, 0.5, g) * 1.5
    gam, bet = lc._affine(D, g)
    _, mean, rstd = ref.layernorm_fwd(x, gam, bet, 1e-5)
    dy, g_res = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    return x, gam, mean, rstd, dy, g_res, lc._rng(CPU), (7, 8, 9), (p, p, p), N


def _bwd(x, gam, mean, rstd, dy, g_res, rng, sites, ps, N, mutant=None):
    """fp32 LayerNorm backward (reference.layernorm_bwd + embed_patch_grad) with one fault."""
    M, D = x.shape
    xh = (x - mean.unsqueeze(1)) * rstd.unsqueeze(1)
    rows = M - M % 8 if mutant == "dgamma_misses_ragged_group" else M
    dgamma = (dy * xh)[:rows].sum(0)
    dxh = dy * gam
    c1 = dxh.mean(-1, keepdim=True) if mutant != "c1_dropped" else 0.0
    c2 = (dxh * xh).sum(-1, keepdim=True) / (D - 1 if mutant == "c2_over_d_minus_1" else D)
    g_out = g_res + (dxh - c1 - xh * c2) * rstd.unsqueeze(1)
    B = M // N
    if mutant == "drop_path_per_row":
        sc = ref._sample_scale(M, rng, sites[1], ps[1], CPU)
    else:
        sc = ref._sample_scale(B, rng, sites[1], ps[1], CPU).repeat_interleave(N)
    gy = ref.bf16(ref._dropout(g_out, rng, sites[0], ps[0]) * sc.unsqueeze(1))
    gm = ref._dropout(g_out.view(B, N, D), rng, sites[2], ps[2])
    gp = ref.bf16((gm[:, :-1] if mutant == "gp_includes_cls_row" else gm[:, 1:]).reshape(B * (N - 1), D))
    return g_out, dgamma, gy, gp


def _bwd_checks(ops_, out, t):
    g_out, dgamma, gy, gp = out
    clean = _bwd(*ops_)
    return {"g_out": lambda: lc.assert_terms(g_out, t.g_out, t.t_g_out, "g_out"),
            "dgamma": lambda: lc.assert_terms(dgamma, t.dgamma, t.t_dgamma, "dgamma"),
            "gy": lambda: (lc.assert_within(gy, clean[2], t.gy, "gy"), lc.assert_drop_set(gy, clean[2], "gy")),
            "gp": lambda: (lc.assert_within(gp, clean[3], t.gp, "gp"), lc.assert_drop_set(gp, clean[3], "gp"))}


@pytest.mark.parametrize("mutant,seen_by,M,N", [("c2_over_d_minus_1", "g_out", 40, 5), ("c1_dropped", "g_out", 40, 5),
                                                 ("dgamma_misses_ragged_group", "dgamma", lc.LN_BWD_STRIDED_M, 37),
                                                 ("drop_path_per_row", "gy", 40, 5), ("gp_includes_cls_row", "gp", 40, 5)])
def test_backward_mutants(mutant, seen_by, M, N):
    ops_ = _bwd_operands(M, 128, N, 0.1)
    x, gam, mean, rstd, dy, g_res, rng, sites, ps, _ = ops_
    t = lc.ln_bwd_truth(dy, x, mean, rstd, gam, g_res, N, rng, sites, ps)
    for chk in _bwd_checks(ops_, _bwd(*ops_), t).values():
        chk()  # the clean backward passes every check
    checks = _bwd_checks(ops_, _bwd(*ops_, mutant=mutant), t)
    _rejects(checks[seen_by])


# ----------------------------------------------------------------------------- where the model sits
def test_vit_tiny_layernorm_inputs_at_init():
    """|mean| / std of every LayerNorm input of ``vit_tiny`` at initialisation (one batch of 8
    through the reference program): the model sits at the flat end of the sqrt(2 + r^2) law."""
    from ddim_cold_amd.models import build_model
    from ddim_cold_amd.models import program as pr
    torch.manual_seed(0)
    m = build_model("vit_tiny").eval()
    P = pr.model_tensors(m)
    assert P.folded
    img, t = torch.randn(8, 3, 64, 64), torch.randint(0, 2000, (8,))
    _, S = m.program().forward(P, img, t, lc._rng(CPU), False)
    stats = [(f"block {i} norm1", b[2], b[3]) for i, b in enumerate(S.blocks)] + \
            [(f"block {i} norm2", b[9], b[10]) for i, b in enumerate(S.blocks)] + [("final norm", S.mf, S.rf)]
    worst = 0.0
    for name, mean, rstd in sorted(stats):
        r = float((mean.abs() * rstd).max())
        worst = max(worst, r)
        lc._log(f"vit_tiny at init, {name}: max |mean| / std over the rows = {r:.3f}  (fold cost sqrt(2 + r^2) = "
                f"{math.sqrt(2 + r * r):.2f}x the unfolded error)")
    assert worst < 1.0, worst  # sqrt(2 + r^2) < 1.74: within 23 % of the r = 0 cost
