"""Output stores of the kernels whose cache policy was put to the test (write-through
``sc1`` stores, csrc/common.h ``st_wt*``; profiles/store_writethrough.txt says which
kernels keep them): whatever the policy, every output element is written, nothing
lands outside, and a consumer kernel that follows in a replayed graph reads what the
producer wrote.

* Ragged edges: the smallest shapes that leave partial tiles / rows / vectors.  Buffers
  the caller passes in sit in canaries (guard elements on both sides) and start as NaN;
  outputs an op allocates itself are compared on raw bits against exact integer truths
  (:mod:`ddim_cold_amd.ops.gemm_check`) after a NaN-filled block of their size was
  handed back to the allocator, so an element left unwritten cannot pass as a value.
* Visibility: producer -> consumer pairs captured in one graph (16 workgroups each, so
  every XCD takes part), replayed 20 times on new inputs, bit-equal to the same ops run
  eagerly with a synchronize between them.
"""
import math

import pytest
import torch

from ddim_cold_amd import ops
from ddim_cold_amd.ops import check
from ddim_cold_amd.ops import gemm_check as gc
from ddim_cold_amd.ops import ln_check as lc
from ddim_cold_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)
    torch.manual_seed(0)


def _rng(seed=1234, step=5):
    return torch.tensor([seed, step], dtype=torch.int64, device=DEV)


def _poison(*specs):
    """Free NaN-filled blocks of the given (numel, dtype): the caching allocator hands a
    freed block of the same size to the next request, so an op's own ``empty`` output
    starts as NaN instead of as whatever an earlier test left there."""
    blocks = [torch.full((int(n),), NAN, dtype=dt, device=DEV) for n, dt in specs]
    torch.cuda.synchronize()
    del blocks


def _nan_canary(shape, pad, dtype):
    view, ok = gc.canary(shape, pad, dtype, DEV)
    view.fill_(NAN)
    return view, ok


def _no_nan(t, name):
    bad = int(torch.isnan(t.float()).sum())
    assert bad == 0, f"{name}: {bad} of {t.numel()} elements were never written"


# ------------------------------------------------------------------ GEMM epilogues
M, N, K = 33, 68, 64  # one partial 32-row tile, a 4-column tail past the 64-column tile, one k-tile


def _gemm_bf16_f32():
    gc.run_linear(M, N, K, DEV)


def _gemm_resid():
    # N = 68 (no statistics: they need N % 32 == 0), then 96 columns with st_out / xb_out in canaries
    g = gc._gen(2)
    a, w = gc.int_operands((M, K), -4, 4, g, device=DEV), gc.int_operands((N, K), -4, 4, g, device=DEV)
    b = gc.int_operands((N,), -64, 64, g, torch.float32, DEV)
    x = gc.int_operands((M, N), -64, 64, g, torch.float32, DEV)
    _poison((M * N, torch.float32))
    y = ops.linear_residual_fwd(a, w, b, x, 11, _rng(), 3, 0.0, 4, 0.0)
    gc.assert_exact(y, gc.exact_truth(a, w, b, x, torch.float32), f"linear_residual_fwd M={M} N={N} K={K}", (32, 64))
    gc.run_residual(M, 11, 96, K, DEV)


def _gemm_gelu():
    gc.run_gelu(M, N, K, DEV)


def _gemm_dgelu():
    # the input-gradient binding takes widths that are multiples of 8 only, so 68 columns
    # cannot run: 72 is the nearest width with a partial column tile (8 past the 64-column tile)
    g = gc._gen(8)
    dy, w = gc.int_operands((M, K), -4, 4, g, device=DEV), gc.int_operands((K, N), -4, 4, g, device=DEV)
    with pytest.raises(RuntimeError, match="multiples of 8"):
        ops.linear_dgrad_gelu(dy, w, torch.zeros(M, N, dtype=torch.bfloat16, device=DEV), _rng(), 11, 0.0)
    _poison((M * 72, torch.bfloat16))
    gc.run_dgrad_gelu(M, K, 72, DEV)  # reduction over K = 64, 72 output columns


def _gemm_qkv():
    gc.run_qkv(3, 11, 2, 64, DEV)  # 33 rows, 192 = 2 x 3 hd columns (hd = 32), K = 64


@pytest.mark.parametrize("epi", ["bf16_f32", "resid", "gelu", "dgelu", "qkv"])
def test_gemm_ragged_edges(epi):
    _poison((M * N, torch.float32), (M * N, torch.bfloat16), (M * 192, torch.bfloat16))
    {"bf16_f32": _gemm_bf16_f32, "resid": _gemm_resid, "gelu": _gemm_gelu, "dgelu": _gemm_dgelu,
     "qkv": _gemm_qkv}[epi]()


@pytest.mark.parametrize("store", [False, True])
def test_wgrad_two_problems_ragged(store):
    """Two 72 x 136 problems over 65 tokens in one launch (64 x 64 tiles: partial tiles on
    both edges, two k-tiles with a one-token tail); dw / db in canaries, exact."""
    gc.run_wgrad_multi(65, [(72, 136, True), (72, 136, False)], DEV, store)


# ------------------------------------------------------------------ LayerNorm backward
@pytest.mark.parametrize("bf16_in", [False, True])
@pytest.mark.parametrize("D", [128, 384])
def test_layernorm_bwd_ragged(D, bf16_in):
    """9 rows: one full workgroup of 8 and one with a single live wave.  Values against the
    fp64 truth (ln_check.run_ln_bwd, dgamma / dbeta / slots in canaries); then the same
    launch with y_out / gp_out in NaN-filled canaries: every element written, the guards
    intact, the bits those of a launch into plain buffers."""
    rows, tokens = 9, 3
    for ws in (False, True):
        lc.run_ln_bwd(lc.LnBwdCase(rows, D, tokens, dy_bf16=bf16_in, x_bf16=bf16_in, p=0.1, y_out=True, gp=True,
                                   ws=ws), DEV)
    g = gc._gen(31)
    x32 = lc.off_centre_rows(rows, D, 0.5, g)
    gam, bet = lc._affine(D, g)
    _, mean, rstd = ref.layernorm_fwd(x32, gam, bet, 1e-5)
    dt = torch.bfloat16 if bf16_in else torch.float32
    x, dy = x32.to(dt).to(DEV), torch.randn(rows, D, generator=g).to(dt).to(DEV)
    g_res = torch.randn(rows, D, generator=g).to(DEV)
    mean, rstd, gam, bet = (t.to(DEV) for t in (mean, rstd, gam, bet))
    B = rows // tokens
    R = ops.ln_ws_rows(rows)

    def launch(y_out, gp, ws):
        dg, db = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
        _poison((rows * D, torch.float32), (rows * D, torch.bfloat16))
        g_out, gy = ops.layernorm_bwd(dy, x, mean, rstd, gam, g_res, dg, db, tokens, _rng(), 7, 0.1, 8, 0.1, True,
                                      ws=ws, beta=bet, y_out=y_out, gp_out=gp, site_emb=9, p_emb=0.1)
        return g_out, gy

    y0 = torch.empty(rows, D, dtype=torch.bfloat16, device=DEV)
    gp0 = torch.empty(B * (tokens - 1), D, dtype=torch.bfloat16, device=DEV)
    ws0 = torch.empty(R, 2 * D, device=DEV)
    g0, gy0 = launch(y0, gp0, ws0)
    y1, y_ok = _nan_canary((rows, D), 2 * D, torch.bfloat16)
    gp1, gp_ok = _nan_canary((B * (tokens - 1), D), 2 * D, torch.bfloat16)
    ws1, ws_ok = _nan_canary((R, 2 * D), 2 * D, torch.float32)
    g1, gy1 = launch(y1, gp1, ws1)
    name = f"layernorm_bwd rows={rows} D={D} {'bf16' if bf16_in else 'fp32'} inputs"
    for got, want, what in ((g1, g0, "g_out"), (gy1, gy0, "gy"), (y1, y0, "y_out"), (gp1, gp0, "gp_out"),
                            (ws1, ws0, "slots")):
        _no_nan(got, f"{name} {what}")
        gc.assert_exact(got, want, f"{name} {what}")
    y_ok(name + " y_out")
    gp_ok(name + " gp_out")
    ws_ok(name + " slots")


# ------------------------------------------------------------------ short attention
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_short_attention_ragged(p):
    """B = H = 1, N = 65 (96-row padded kernel: one key past the fourth 16-key tile, a last
    wave with a single live query): o / lse / dqkv against the fp64 truth within what the
    mirror reference achieves, every element written, the keep words in a canary."""
    B, H, n, hd = 1, 1, 65, 32
    qkv = torch.randn(3, B, H, n, hd, device=DEV).to(torch.bfloat16)
    do = torch.randn(B, n, H * hd, device=DEV).to(torch.bfloat16)
    r, scale = _rng(), hd ** -0.5
    keep = keep_ok = None
    kb = ops.attn_keep_buffer(qkv, p)
    if kb is not None:
        keep, keep_ok = gc.canary((kb.numel(),), 64, torch.int32, DEV)
    _poison((B * n * H * hd, torch.bfloat16), (B * H * n, torch.float32), (B * n * 3 * H * hd, torch.bfloat16))
    o, lse = ops.attn_fwd(qkv, scale, r, 5, p, keep_out=keep)
    dq = ops.attn_bwd(do, qkv, o, lse, scale, r, 5, p, keep=keep)
    tag = f"short attention N={n} p={p}"
    for t, what in ((o, "o"), (lse, "lse"), (dq, "dqkv")):
        _no_nan(t, f"{tag} {what}")
    assert o.shape == (B, n, H * hd) and lse.numel() == B * H * n and dq.shape == (B * n, 3 * H * hd)
    o_m, _ = ref.attn_fwd(qkv, scale, r, 5, p)
    dq_m = ref.attn_bwd(do, qkv, o, lse, scale, r, 5, p)
    truth = check.attn_truth(qkv, do, scale, r, 5, p, 0)
    check.assert_lse(lse, truth[1], f"{tag} lse")
    check.assert_within(check.split_o(o, B, H, n, hd), check.split_o(o_m, B, H, n, hd), truth[0], f"{tag} o")
    got, mir = check.split_dqkv(dq, B, H, n, hd), check.split_dqkv(dq_m, B, H, n, hd)
    for i, what in enumerate(("dq", "dk", "dv")):
        check.assert_within(got[i], mir[i], truth[2 + i], f"{tag} {what}")
    if keep is not None:
        keep_ok(tag + " keep words")
        # stored flags == re-hashed masks, and the forward's outputs do not depend on storing them
        assert torch.equal(ops.attn_bwd(do, qkv, o, lse, scale, r, 5, p), dq)
        o2, lse2 = ops.attn_fwd(qkv, scale, r, 5, p)
        assert torch.equal(o2, o) and torch.equal(lse2, lse)
    # exact probe: q = 0, V = 1 -> every probability 1/N; without dropout o = 1 exactly
    qkv[0] = 0
    qkv[2] = 1
    o, lse = ops.attn_fwd(qkv, 0.37, r, 5, 0.0)
    assert torch.equal(o, torch.ones_like(o))
    assert (lse.double() - math.log(n)).abs().max().item() <= 8 * 2.0 ** -23 * math.log(n)


# ------------------------------------------------------------------ AdamW
HYPER = [3e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 10.0, 0.0]


@pytest.mark.parametrize("mode", ["plain", "lazy", "ema"])
def test_adamw_ragged(mode):
    """n = 4k + 3 over five workgroups: 16-byte vectors and a 3-element scalar tail.  Every
    arena sits in a canary; the bf16 shadow starts as NaN.  p / m / v against the reference
    step at the existing fused-AdamW tolerance, the shadow and the EMA exact from the
    kernel's own p, the gradient zeroed below zero_hi only, a lazy range untouched."""
    n = 4 * 1031 + 3
    lo, hi = (256, 1280) if mode == "lazy" else (0, 0)
    zero_hi = 4 * 700
    g = torch.Generator().manual_seed(3)
    init = {"p": torch.randn(n, generator=g), "g": torch.randn(n, generator=g) * 0.1,
            "m": torch.randn(n, generator=g) * 0.01, "v": torch.rand(n, generator=g) * 1e-3,
            "e": torch.randn(n, generator=g)}
    if hi > lo:
        for k in ("g", "m", "v"):
            init[k][lo:hi] = 0
    a, oks = {}, {}
    for k, t in init.items():
        a[k], oks[k] = gc.canary((n,), 64, torch.float32, DEV)
        a[k].copy_(t)
    pb, oks["pb"] = _nan_canary((n,), 64, torch.bfloat16)
    sq = torch.zeros(ops.SQ_PARTS, device=DEV)
    ops.sqnorm(a["g"].clone(), sq, 1.0, lazy=(lo, hi) if hi > lo else None)
    step = torch.tensor([2, 2], dtype=torch.int64, device=DEV)
    hyper = torch.tensor(HYPER, device=DEV)
    lazy_decay = torch.ones(1, device=DEV)
    kw = dict(zero_hi=zero_hi)
    if mode == "lazy":
        kw.update(lazy=(lo, hi), lazy_decay=lazy_decay)
    if mode == "ema":
        kw.update(ema=a["e"], ema_decay=0.9, ema_warmup=False)
    ops.adamw_step(a["p"], a["g"], a["m"], a["v"], pb, sq, step, hyper, 1.0, **kw)
    torch.cuda.synchronize()
    for k, ok in oks.items():
        ok(f"adamw {mode} {k}")
    # reference step on the CPU (ops dispatches CPU tensors to ops/reference-style math)
    c = {k: t.clone() for k, t in init.items()}
    cpb = torch.empty(n, dtype=torch.bfloat16)
    ckw = dict(kw)
    if mode == "lazy":
        ckw["lazy_decay"] = torch.ones(1)
    if mode == "ema":
        ckw["ema"] = c["e"]
    ops.adamw_step(c["p"], c["g"], c["m"], c["v"], cpb, sq.cpu(), step.cpu(), hyper.cpu(), 1.0, **ckw)
    for k in ("p", "m", "v"):
        torch.testing.assert_close(a[k].cpu(), c[k], rtol=1e-5, atol=1e-6, msg=lambda s, k=k: f"adamw {mode} {k}: {s}")
    live = torch.ones(n, dtype=torch.bool)
    live[lo:hi] = False
    p_new = a["p"].cpu()
    assert not torch.equal(p_new[live], init["p"][live])
    assert torch.equal(gc._bits(pb.cpu()[live]), gc._bits(p_new.to(torch.bfloat16)[live])), "bf16 shadow != bf16(p)"
    if hi > lo:  # untouched: p / m / v as they were, the shadow still NaN
        for k in ("p", "m", "v"):
            assert torch.equal(gc._bits(a[k].cpu()[lo:hi]), gc._bits(init[k][lo:hi])), f"lazy range of {k} written"
        assert bool(torch.isnan(pb.cpu()[lo:hi].float()).all()), "lazy range of the bf16 shadow written"
        torch.testing.assert_close(lazy_decay.cpu(), ckw["lazy_decay"], rtol=1e-6, atol=0)
    gz = a["g"].cpu()
    assert torch.equal(gc._bits(gz[zero_hi:]), gc._bits(init["g"][zero_hi:])), "gradient past zero_hi written"
    below = torch.ones(n, dtype=torch.bool)
    below[zero_hi:] = False
    assert bool((gz[below & live] == 0).all()), "gradient below zero_hi not zeroed"
    if mode == "ema":
        want = p_new + torch.tensor(0.9) * (init["e"] - p_new)  # three separately rounded fp32 operations
        assert torch.equal(gc._bits(a["e"].cpu()), gc._bits(want)), "EMA != p + d (e - p)"
    else:
        assert torch.equal(gc._bits(a["e"].cpu()), gc._bits(init["e"])), "EMA arena written without ema="


# ------------------------------------------------------------------ visibility across kernels
VM, VN, VK = 256, 128, 64  # 8 x 2 tiles of 32 x 64 = 16 workgroups per GEMM; 32 of the LayerNorm backward


class _Chain:
    """GEMM -> GEMM on its output, and LayerNorm backward -> GEMM on its gy."""

    def __init__(self):
        g = gc._gen(40)
        self.a = torch.empty(VM, VK, dtype=torch.bfloat16, device=DEV)
        self.dy = torch.empty(VM, VN, device=DEV)
        self.x = torch.empty(VM, VN, device=DEV)
        self.mean = torch.empty(VM, device=DEV)
        self.rstd = torch.empty(VM, device=DEV)
        self.w1 = (torch.randn(VN, VK, generator=g) * 0.2).to(torch.bfloat16).to(DEV)
        self.w2 = (torch.randn(VN, VN, generator=g) * 0.2).to(torch.bfloat16).to(DEV)
        self.w3 = (torch.randn(VN, VN, generator=g) * 0.2).to(torch.bfloat16).to(DEV)
        self.b1 = torch.randn(VN, generator=g).to(DEV)
        self.gam, self.bet = (t.to(DEV) for t in lc._affine(VN, g))
        self.g_res = torch.randn(VM, VN, generator=g).to(DEV)
        self.dg, self.db = torch.zeros(VN, device=DEV), torch.zeros(VN, device=DEV)
        self.ws = torch.zeros(ops.ln_ws_rows(VM), 2 * VN, device=DEV)
        self.rng = _rng()

    def set_inputs(self, i):
        g = torch.Generator(device=DEV).manual_seed(100 + i)
        self.a.copy_(torch.randn(VM, VK, device=DEV, generator=g).to(torch.bfloat16))
        self.dy.copy_(torch.randn(VM, VN, device=DEV, generator=g))
        self.x.copy_(torch.randn(VM, VN, device=DEV, generator=g) * 1.5 + 0.5)
        self.mean.copy_(self.x.mean(-1))
        self.rstd.copy_((self.x.var(-1, unbiased=False) + 1e-5).rsqrt())

    def run(self, between=lambda: None):
        y1 = ops.linear_fwd(self.a, self.w1, self.b1, False)
        between()
        y2 = ops.linear_fwd(y1, self.w2, None, True)
        between()
        g_out, gy = ops.layernorm_bwd(self.dy, self.x, self.mean, self.rstd, self.gam, self.g_res, self.dg, self.db,
                                      VM, self.rng, 7, 0.1, 8, 0.0, True, ws=self.ws)
        between()
        y3 = ops.linear_fwd(gy, self.w3, None, True)
        between()
        return y1, y2, g_out, gy, y3


def test_graph_replay_sees_the_producers_stores():
    ch = _Chain()
    ch.set_inputs(0)
    ch.run()  # warm-up outside the capture (lazy initialisation of the launch paths)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = ch.run()
    names = ("gemm1", "gemm2(gemm1)", "ln_bwd g_out", "ln_bwd gy", "gemm3(gy)")
    for i in range(20):
        ch.set_inputs(i)
        graph.replay()
        torch.cuda.synchronize()
        got = [t.clone() for t in outs] + [ch.ws.clone()]
        want = list(ch.run(torch.cuda.synchronize)) + [ch.ws]
        for t, w, nm in zip(got, want, names + ("ln_bwd slots",)):
            gc.assert_exact(t, w, f"replay {i}: {nm}", (32, 64))
