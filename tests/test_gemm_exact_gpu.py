"""The GEMMs of csrc/gemm.hip against exact integer probes (ops/gemm_check.py), bit for
bit, over every tile configuration, ring depth, operand reader and edge.

With small-integer bf16 operands every partial sum is an exact fp32 integer in any
summation order, so the tolerance is zero; a position probe (one-hot rows against a
coded operand) names the element each output was read from.  Every case asserts through
``torch.ops.ddim_cold.gemm_plan`` the (path, tile, ring depth) of its launch: the op is
``gemm_plan`` of csrc/gemm_plan.h under the current override, the function every launch
calls and follows (``launch_auto`` in gemm.hip launches the instantiation whose tile, waves
and depth equal the plan, or fails), so the kernel it names is the one that ran.  The
mirrors ``expected_tile`` / ``expected_stages`` below are the independent statement of
the rule.  Caller-provided outputs sit in canaried buffers (writes past row M / column N).

Tile configs (``ops.gemm_tile``): 0 = 32x64, 1 = 64x64, 2 = 128x64, 3 = 128x128 (4 waves);
4 = 256x128, 5 = 128x128, 6 = 256x192 (8 waves).  Config 6 is built for the plain-operand
BF16 / QKV / GELU epilogues and runs as 256x128 elsewhere (128x128 for DGELU); config 3 is
128x64 for transposed B; DGELU's 256-row config is the 128-row one (``gemm_cfg_fallback``
in csrc/gemm_plan.h, the one place these are written; tests/cpp/gemm_plan_check.cpp checks
them for every epilogue without a GPU).  Ring depth (``gemm_ring_stages``): 256x192
always 2, 256x128 always 3, the others 3 when the grid exceeds 256 x per_cu4 workgroups
with at most 8 k-tiles per slice, else 4.  ``linear_wgrad_multi`` has its own kernel and
its own plan (csrc/wgrad_plan.h, ``torch.ops.ddim_cold.wgrad_multi_plan``): a 64x64 tile,
or 128x128 from ``ops.WGRAD_WIDE_TOKENS`` tokens, launches of at most 32 problems, and on
the wide tile the tiles past the last whole round of CUs in up to 6 K pieces each.

A new tile configuration joins TILES in ops/gemm_check.py and with it the grids of
sections (a) and (b) here.

The LayerNorm-fold consumers (section (h)) run a probe whose row statistics and column
sums are constructed so that mean, variance and the reciprocal square root are exact too
(ops/gemm_check.py ``run_fold_consumer``); at K = 192 / 384 the host's 1/K is rounded and
the same probe is compared within a bound computed from the operands.

Out of scope here: the non-integer epilogue arithmetic (HEADL and HEAD mode 3, HEAD / HEADR
modes 1 / 4, GELU's ``h``, GELU' in DGELU).  tests/test_epi_values_gpu.py checks it against
fp64 truths with the value entering the epilogue set to the bit (ops/epi_check.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import ops
from ddim_cold_amd.ops import gemm_check as gc

DEV = "cuda"
ALL_TILES = sorted(gc.TILES)
TILES_4W = [0, 1, 2, 3]


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


def plan(epi, M, N, K, at=False, bt=False, splits=1):
    """(dma, BM, BN, waves, stages) of the launch under the current tile override."""
    return tuple(int(v) for v in torch.ops.ddim_cold.gemm_plan(epi, at, bt, M, N, K, splits))


def expected_tile(cfg, epi, bt=False):
    """(BM, BN, waves) of config ``cfg`` after the documented fallbacks."""
    if cfg == 6 and not (not bt and epi in (gc.EPI_BF16, gc.EPI_QKV, gc.EPI_GELU)):
        cfg = 4
    if cfg == 4 and epi == gc.EPI_DGELU:
        cfg = 5
    if cfg == 3 and bt:
        cfg = 2
    return gc.TILES[cfg]


def expected_stages(bm, bn, M, N, K, splits=1):
    stage = (bm + bn) * 128
    if 3 * stage > 160 * 1024:
        return 2
    if 4 * stage > 160 * 1024:
        return 3
    kt = -(-K // 64)
    kps = -(-kt // splits)
    wgs = -(-M // bm) * -(-N // bn) * -(-kt // kps)
    return 3 if wgs > 256 * ((160 * 1024) // (4 * stage)) and kps <= 8 else 4


def assert_plan(cfg, epi, M, N, K, bt=False, splits=1, stages=None):
    """The launch is the LDS-DMA kernel on config ``cfg``'s (documented) tile; returns (BM, BN)."""
    bm, bn, waves = expected_tile(cfg, epi, bt)
    st = expected_stages(bm, bn, M, N, K, splits)
    assert stages is None or st == stages, f"the case was built for ring depth {stages}, the rule gives {st}"
    got = plan(epi, M, N, K, False, bt, splits)
    assert got == (1, bm, bn, waves, st), f"plan {got} != {(1, bm, bn, waves, st)} (cfg {cfg} epi {epi} {M}x{N}x{K})"
    return bm, bn


# ----------------------------------------------------------------------------- (a) tile x edge grid
@pytest.mark.parametrize("K", gc.EDGE_KS)
@pytest.mark.parametrize("cfg", ALL_TILES)
def test_linear_tile_edges(cfg, K):
    bm, bn, _ = gc.TILES[cfg]
    with ops.gemm_tile(cfg):
        for M in gc.edge_ms(bm):
            for N in gc.edge_ns(bn):
                tiles = {f32: assert_plan(cfg, gc.EPI_F32 if f32 else gc.EPI_BF16, M, N, K) for f32 in (False, True)}
                assert tiles[False] == (bm, bn)  # bf16 output: every config is real, 256x192 included
                gc.run_linear(M, N, K, DEV, tile=tiles.get)


# ----------------------------------------------------------------------------- (b) ring depth
PAIRED = ((False, True), (True, False))  # bf16 + bias, fp32 without: output type paired with bias


@pytest.mark.parametrize("K,stages", [(512, 3), (576, 4), (64, 3), (128, 3)])
@pytest.mark.parametrize("cfg", gc.TWO_DEPTH_TILES)
def test_ring_depth_over_threshold(cfg, K, stages):
    """Just over 256 x per_cu4 workgroups: 8 k-tiles take the 3-stage ring, 9 the 4-stage
    one; 1 and 2 k-tiles are fewer than the 3-stage prologue issues."""
    M, N = gc.depth_shape(cfg)
    with ops.gemm_tile(cfg):
        tiles = {f32: assert_plan(cfg, gc.EPI_F32 if f32 else gc.EPI_BF16, M, N, K, stages=stages) for f32 in (False, True)}
        gc.run_linear(M, N, K, DEV, tile=tiles.get, combos=PAIRED)


@pytest.mark.parametrize("K", gc.SHORT_KS)
@pytest.mark.parametrize("cfg", gc.TWO_DEPTH_TILES)
def test_ring_depth4_short_k(cfg, K):
    """Fewer k-tiles than the 4-stage prologue issues."""
    bm, bn, _ = gc.TILES[cfg]
    M, N = bm + 1, bn + 4
    with ops.gemm_tile(cfg):
        tiles = {f32: assert_plan(cfg, gc.EPI_F32 if f32 else gc.EPI_BF16, M, N, K, stages=4) for f32 in (False, True)}
        gc.run_linear(M, N, K, DEV, tile=tiles.get, combos=PAIRED)


@pytest.mark.parametrize("K", gc.FIXED_DEPTH_KS)
@pytest.mark.parametrize("cfg,stages", gc.FIXED_DEPTH_TILES)
def test_ring_depth_fixed(cfg, stages, K):
    """256x128 is always 3 stages deep, 256x192 always 2 (ragged M and N)."""
    bm, bn, _ = gc.TILES[cfg]
    M, N = 2 * bm + 17, bn + 4
    with ops.gemm_tile(cfg):
        assert assert_plan(cfg, gc.EPI_BF16, M, N, K, stages=stages) == (bm, bn)
        gc.run_linear(M, N, K, DEV, tile=(bm, bn), combos=((False, True), (False, False)))


# ----------------------------------------------------------------------------- (c) non-DMA path
@pytest.mark.parametrize("K", gc.PLAIN_KS)
@pytest.mark.parametrize("M,N,bm", [(*gc.PLAIN_SHAPES[0], 32), (*gc.PLAIN_SHAPES[1], 64)])
def test_plain_kernel(M, N, bm, K):
    """K % 64 != 0: ``gemm_kernel`` on 32x64 tiles under 240 64x64 tiles, 64x64 from there;
    the tile override is ignored."""
    want = (0, bm, 64, 4, 2)
    for epi in (gc.EPI_BF16, gc.EPI_F32):
        assert plan(epi, M, N, K) == want
    gc.run_linear(M, N, K, DEV, tile=(bm, 64), combos=PAIRED)
    with ops.gemm_tile(3):
        assert plan(gc.EPI_BF16, M, N, K) == want and plan(gc.EPI_F32, M, N, K) == want
        gc.run_linear(M, N, K, DEV, tile=(bm, 64), combos=PAIRED, seed=12)


# ----------------------------------------------------------------------------- (d) epilogue index maps
@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("B,N,H,D", gc.QKV_SHAPES + (gc.QKV_SHAPE_HD16,))
def test_qkv_exact(cfg, B, N, H, D):
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_QKV, B * N, 3 * D, D)
        assert tile == gc.TILES[cfg][:2]  # QKV: 256x192 is real
        gc.run_qkv(B, N, H, D, DEV, tile=tile)


@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("M,tokens,Dout,K", gc.RESID_SHAPES)
def test_residual_exact(cfg, M, tokens, Dout, K):
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_RESID, M, Dout, K)
        assert cfg != 6 or tile == (256, 128)  # not built for RESID: the documented fallback
        gc.run_residual(M, tokens, Dout, K, DEV, tile=tile)


@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("M,N,K", gc.GELU_SHAPES)
def test_gelu_exact(cfg, M, N, K):
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_GELU, M, N, K)
        assert tile == gc.TILES[cfg][:2]
        gc.run_gelu(M, N, K, DEV, tile=tile)


@pytest.mark.parametrize("cfg", TILES_4W)
@pytest.mark.parametrize("B,C,H,W,p,D", gc.HEAD_GEOMS)
def test_head_exact(cfg, B, C, H, W, p, D):
    N = (H // p) * (W // p) + 1
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_HEAD, B * N, C * p * p, D)
        gc.run_head(B, C, H, W, p, D, DEV, tile=tile)


@pytest.mark.parametrize("cfg", [4, 5, 6])
def test_head_rejects_8_wave_tiles(cfg):
    """The head epilogues reduce over 4 waves: an 8-wave override fails loudly, in the plan
    and in the launch."""
    B, C, H, W, p, D = gc.HEAD_GEOMS[0]
    N = (H // p) * (W // p) + 1
    g = torch.Generator().manual_seed(0)
    a, w = gc.int_operands((B * N, D), -1, 1, g, device=DEV), gc.int_operands((C * p * p, D), -1, 1, g, device=DEV)
    b = torch.zeros(C * p * p, device=DEV)
    with ops.gemm_tile(cfg):
        with pytest.raises(RuntimeError):
            plan(gc.EPI_HEAD, B * N, C * p * p, D)
        with pytest.raises(RuntimeError):
            ops.head_fwd(a, w, b, B, C, H, W, p)
            torch.cuda.synchronize()


@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("B,C,H,W,p,D", gc.EMBED_GEOMS)
def test_patch_embed_exact(cfg, B, C, H, W, p, D):
    M, K = B * (H // p) * (W // p), C * p * p
    with ops.gemm_tile(cfg):
        if K % 64 == 0:
            tile = assert_plan(cfg, gc.EPI_EMBED, M, D, K)
        else:  # p = 4: K = 48, the non-DMA kernel whatever the override
            assert plan(gc.EPI_EMBED, M, D, K) == (0, 32, 64, 4, 2)
            tile = (32, 64)
        gc.run_patch_embed(B, C, H, W, p, D, DEV, tile=tile)


@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("B,C,H,W,p,D", gc.EMBED_STAT_GEOMS)
def test_patch_embed_row_statistics_exact(cfg, B, C, H, W, p, D):
    """The LayerNorm-fold producer of the embedding (``ln_st`` / ``xb_out`` in canaries) at
    widths that are a multiple of 32 but not of the tile: a slot past N must not be written."""
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_EMBED, B * (H // p) * (W // p), D, C * p * p)
        gc.run_patch_embed(B, C, H, W, p, D, DEV, tile=tile, stats=True)


# ----------------------------------------------------------------------------- (e) dropout placement
@pytest.mark.parametrize("p", gc.DROPOUT_PS)
@pytest.mark.parametrize("cfg", ALL_TILES)
def test_dropout_placement(cfg, p):
    """``out == 0`` is the reference's drop set and the survivors its value bit for bit
    (the kernels scale by the fp32 ``1 / (1 - p)`` product the reference's division equals
    at these p and values; GELU's ``h`` keeps the tolerance: erf is not exact), at ragged
    M and N under every tile."""
    bm, bn, _ = gc.TILES[cfg]
    M, N = 2 * bm + 17, bn + 4
    tokens = gc.small_prime_factor(M)
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_RESID, M, N, 64)
        gc.run_dropout("resid_drop", M, N, p, DEV, tile, tokens=tokens)
        gc.run_dropout("resid_dp", M, N, p, DEV, tile, tokens=tokens)
        gc.run_dropout("gelu", M, N, p, DEV, assert_plan(cfg, gc.EPI_GELU, M, N, 64))
        B, H, W, pp = gc.embed_dropout_geom(M)
        gc.run_dropout_embed(B, H, W, pp, N, p, DEV, assert_plan(cfg, gc.EPI_EMBED, B * 81, N, 3 * pp * pp))
        Nd = gc.dgrad_width(cfg) if cfg < 6 else bn + 8
        gc.run_dropout("dgelu", M, Nd, p, DEV, assert_plan(cfg, gc.EPI_DGELU, M, Nd, 64, bt=True))


# ----------------------------------------------------------------------------- (f) dgrad
@pytest.mark.parametrize("Nout", gc.DGRAD_NOUT)
@pytest.mark.parametrize("cfg", ALL_TILES[:6])
def test_dgrad_exact(cfg, Nout):
    K = gc.dgrad_width(cfg)
    splits = [1] + gc.dgrad_splits(Nout)
    with ops.gemm_tile(cfg):
        for M in gc.DGRAD_MS:
            for s in splits:
                for epi in (gc.EPI_F32, gc.EPI_BF16):
                    if Nout % 64 == 0:
                        tile = assert_plan(cfg, epi, M, K, Nout, bt=True, splits=s)
                    else:  # the non-DMA kernel, transposed-B reader
                        tile = (64 if -(-M // 64) * -(-K // 64) * s >= 240 else 32, 64)
                        assert plan(epi, M, K, Nout, bt=True, splits=s) == (0, *tile, 4, 2)
            gc.run_dgrad(M, Nout, K, DEV, tile=tile, splits=splits)


@pytest.mark.parametrize("M,Nout,K,s", gc.DGRAD_LN_CASES)
def test_dgrad_slices_into_layernorm_bwd(M, Nout, K, s):
    assert s == gc.dgrad_splits(Nout)[-1]  # the largest split the binding accepts
    gc.run_dgrad_ln(M, Nout, K, s, DEV)


@pytest.mark.parametrize("with_wt", [False, True])
@pytest.mark.parametrize("cfg", ALL_TILES[:6])
@pytest.mark.parametrize("M,Nout", gc.DGELU_SHAPES)
def test_dgrad_gelu_exact(cfg, M, Nout, with_wt):
    K = gc.dgrad_width(cfg)
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_DGELU, M, K, Nout, bt=not with_wt)
        assert cfg < 4 or tile == (128, 128)  # DGELU's 8-wave tile is always 128x128
        gc.run_dgrad_gelu(M, Nout, K, DEV, tile=tile, with_wt=with_wt)


# ----------------------------------------------------------------------------- (g) wgrad
def _wgrad_splits(T, Nout, K):  # csrc/bindings.cpp linear_wgrad
    tiles = -(-Nout // 64) * -(-K // 64)
    return max(1, min(8, -(-256 // tiles), -(-T // 64)))


@pytest.mark.parametrize("T", gc.WGRAD_TOKENS)
def test_wgrad_exact(T):
    for Nout, K, with_db in gc.wgrad_shapes():
        for db in (with_db, not with_db):
            assert plan(gc.EPI_ATOMIC, Nout, K, T, at=True, bt=True, splits=_wgrad_splits(T, Nout, K))[:4] == (1, 64, 64, 4)
            gc.run_wgrad(T, Nout, K, DEV, db)


def wgrad_multi_plan(shapes, T):
    """(tile edge, [(first, count, tiles, split, whole, pieces, ws_floats) per launch]) of
    ``linear_wgrad_multi`` over ``shapes`` = (Nout, K, ...) at ``T`` tokens."""
    v = [int(i) for i in torch.ops.ddim_cold.wgrad_multi_plan([s[0] for s in shapes], [s[1] for s in shapes],
                                                              [T] * len(shapes))]
    return v[0], [tuple(v[i:i + 7]) for i in range(2, len(v), 7)]


def assert_wgrad_plan(shapes, T, tile, launches=1, split=1, whole=None):
    """The launches are the ones the case names: ``tile`` x ``tile`` output tiles, ``launches``
    launches covering the problems in order, every launch in ``split`` K pieces past its
    first ``whole`` tiles (None: not named)."""
    edge, recs = wgrad_multi_plan(shapes, T)
    assert edge == tile and len(recs) == launches, f"plan {edge, recs}: not {launches} launch(es) of {tile}-tiles"
    nxt = 0
    for first, count, tiles, s, wh, pieces, ws in recs:
        assert first == nxt and 1 <= count <= 32
        nxt += count
        assert tiles == sum(-(-n // tile) * -(-k // tile) for n, k, *_ in shapes[first:first + count])
        assert s == split and (whole is None or wh == whole), f"plan {recs}: not split {split} after {whole} tiles"
        assert pieces == (tiles - wh) * (s - 1) and ws == ((tiles - wh) * s * (tile * tile + tile) if s > 1 else 0)
    assert nxt == len(shapes)
    return recs


@pytest.mark.parametrize("store", [False, True])
@pytest.mark.parametrize("T", gc.WGRAD_TOKENS)
def test_wgrad_multi_exact(T, store):
    assert_wgrad_plan(gc.wgrad_shapes(), T, 64)
    gc.run_wgrad_multi(T, gc.wgrad_shapes(), DEV, store)


@pytest.mark.parametrize("store", [False, True])
def test_wgrad_multi_wide_split_tail(store):
    """>= 16,384 tokens: 128x128 tiles; 10 tiles, all in the K-split tail (6 pieces each):
    exact and bit-identical over three launches."""
    assert assert_wgrad_plan(gc.WGRAD_BIG_SHAPES, gc.WGRAD_BIG_TOKENS, 128, split=6, whole=0)[0][2] == 10
    gc.run_wgrad_multi(gc.WGRAD_BIG_TOKENS, gc.WGRAD_BIG_SHAPES, DEV, store, lo=-2, hi=2, repeats=3)


@pytest.mark.parametrize("T,store", [(200, False), (200, True), (gc.WGRAD_BIG_TOKENS, False), (gc.WGRAD_BIG_TOKENS, True)])
def test_wgrad_multi_sq_partials(T, store):
    assert gc.WGRAD_BIG_TOKENS >= ops.WGRAD_WIDE_TOKENS > 200
    if T < ops.WGRAD_WIDE_TOKENS:
        shapes = gc.wgrad_shapes()
        assert_wgrad_plan(shapes, T, 64)
    else:
        shapes = gc.WGRAD_BIG_SHAPES
        assert_wgrad_plan(shapes, T, 128, split=6, whole=0)
    gc.run_wgrad_sq(T, shapes, DEV, store)


def _big_split_jobs():
    """``WGRAD_BIG_SHAPES`` at 16,392 tokens with zeroed targets (``store=True``): 10 wide
    tiles, all in the split tail, 6 pieces each; fp64 truths and canaries."""
    T, shapes = gc.WGRAD_BIG_TOKENS, gc.WGRAD_BIG_SHAPES
    assert assert_wgrad_plan(shapes, T, 128, split=6, whole=0)[0][2] == 10
    g = gc._gen(10)
    return (list(z) for z in zip(*[gc._wgrad_job(T, n, k, hb, True, g, DEV, -2, 2) for n, k, hb in shapes]))


def _scrub(jobs):
    for _, _, dw, db in jobs:  # store=True never reads the targets: a NaN left over shows a tile not written
        dw.fill_(float("nan"))
        if db is not None:
            db.fill_(float("nan"))


def _bits(jobs):
    return [gc._bits(t).clone() for _, _, dw, db in jobs for t in (dw, db) if t is not None]


def test_wgrad_multi_tickets_across_graphs():
    """One caller-owned ticket buffer serves two graphs captured in two pools, replayed in
    either order: whichever runs first finds the tickets zero and leaves them zero."""
    jobs, truths, oks = _big_split_jobs()
    tickets = ops.wgrad_tickets(DEV)
    assert tickets.dtype == torch.int32 and tickets.numel() == ops.WGRAD_TICKETS and not tickets.any()
    graphs = []
    for _ in range(2):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=torch.cuda.graph_pool_handle()):
            ops.linear_wgrad_multi(jobs, store=True, tickets=tickets)
        graphs.append(g)
    a, b = graphs
    seen = []
    for name, g in (("B", b), ("A", a), ("B again", b)):
        _scrub(jobs)
        g.replay()
        torch.cuda.synchronize()
        gc._wgrad_check(jobs, truths, oks, f"linear_wgrad_multi graph {name}")
        assert not tickets.any(), f"graph {name} left a ticket taken"
        seen.append(_bits(jobs))
    for s in seen[1:]:
        assert all(torch.equal(x, y) for x, y in zip(s, seen[0])), "weight gradients differ between replays"


def test_wgrad_multi_capture_needs_tickets():
    """Inside a capture a launch with split tiles and no ``tickets`` is refused before it
    allocates or launches; the eager call fills its own."""
    jobs, truths, oks = _big_split_jobs()
    _scrub(jobs)
    before = _bits(jobs)
    other = torch.zeros(64, device=DEV)
    with pytest.raises(RuntimeError, match="wgrad_tickets"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            other.add_(1.0)  # the capture holds other work, as a step's does
            ops.linear_wgrad_multi(jobs, store=True)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_bits(jobs), before))
    ops.linear_wgrad_multi(jobs, store=True)
    gc._wgrad_check(jobs, truths, oks, "linear_wgrad_multi after a refused capture")


def _int_jobs(shapes, T, g, arena=None):
    """Integer jobs whose every product is non-zero somewhere; ``arena``: dw / db are views of it."""
    jobs, off = [], 0
    for n, k in shapes:
        dy, x = gc.int_operands((T, n), 1, 3, g, device=DEV), gc.int_operands((T, k), 1, 3, g, device=DEV)
        if arena is None:
            dw, db = gc.int_operands((n, k), -8, 8, g, torch.float32, DEV), gc.int_operands((n,), -8, 8, g, torch.float32, DEV)
        else:
            dw, db = arena[off:off + n * k].view(n, k), arena[off + n * k:off + n * k + n]
            off += n * k + n
        jobs.append((dy, x, dw, db))
    return jobs


def test_wgrad_multi_checks_before_launching():
    """A refused call has written nothing: embedding parts over two launches without ``sq``
    (33 problems), and grad-norm partials too small for the tiles of two launches."""
    g = gc._gen(12)
    jobs = _int_jobs([(8, 8)] * 33, 8, g)
    B, N, D = 2, 3, 8
    emb = [gc.int_operands(s, 1, 3, g, torch.float32, DEV) for s in ((B, N, D), (D,), (N * D,), (4, D))]
    t = torch.tensor([1, 2], device=DEV)
    spec = (emb[0], t, gc._rng(DEV), 3, 0.0, emb[1], emb[2], emb[3], B, None)
    assert_wgrad_plan([(8, 8)] * 33, 8, 64, launches=2)
    before = _bits(jobs) + [gc._bits(e).clone() for e in emb]
    with pytest.raises(RuntimeError, match="one launch"):
        ops.linear_wgrad_multi(jobs, embed=spec)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(_bits(jobs) + [gc._bits(e) for e in emb], before))

    shapes = [(320, 320)] * 44  # 1,100 64x64 tiles in two launches: more than 1,024 slots
    arena = gc.int_operands((sum(n * k + n for n, k in shapes),), -8, 8, g, torch.float32, DEV)
    jobs = _int_jobs(shapes, 8, g, arena)
    recs = assert_wgrad_plan(shapes, 8, 64, launches=2)
    parts = torch.full((1024,), 7.0, device=DEV)
    assert recs[0][2] < parts.numel() < recs[0][2] + recs[1][2]  # the first launch alone would fit
    before = [gc._bits(arena).clone(), gc._bits(parts).clone()]
    with pytest.raises(RuntimeError, match="grad-norm partials"):
        ops.linear_wgrad_multi(jobs, sq=(parts, arena, None))
    with pytest.raises(RuntimeError, match="grad-norm partials"):  # under the buffer's minimum size
        ops.linear_wgrad_multi(jobs, sq=(torch.zeros(256, device=DEV), arena, None))
    torch.cuda.synchronize()
    assert torch.equal(gc._bits(arena), before[0]) and torch.equal(gc._bits(parts), before[1])


def test_engines_own_their_wgrad_tickets():
    from ddim_cold_amd import build_model
    from ddim_cold_amd.train.engine import EngineConfig, TrainEngine
    engines = [TrainEngine(build_model("vit_tiny").cuda().train(), EngineConfig(use_graph=False)) for _ in range(2)]
    a, b = (e.wgrad_tickets for e in engines)
    assert a.data_ptr() != b.data_ptr() and a.numel() == b.numel() == ops.WGRAD_TICKETS
    assert a.dtype == torch.int32 and not a.any() and not b.any()


# ----------------------------------------------------------------------------- (h) LayerNorm-fold consumers
FOLD_KS = gc.FOLD_EXACT_KS + gc.FOLD_BOUNDED_KS


def test_fold_reciprocal_square_root_is_exact_at_probe_sigmas():
    """The one assumption of the exact fold probe: the hardware reciprocal square root the
    epilogue uses (``__builtin_amdgcn_rsqf``) returns exactly 2, 1, 1/2, 1/4 at 1/4, 1, 4, 16.
    Measured on an MI355X: it does, at all four, so the probe keeps every sigma and compares
    on raw bits (no sigma restricted, no truth rebuilt from the returned rstd).  Asserted here
    through the returned ``ln_rstd``; every probe below asserts it again before its output."""
    from ddim_cold_amd.ops import ln_check as lc
    M, K = 64, 128
    mu, sigma, c = gc.fold_codes(M, 3 * K, K)
    mu = torch.zeros_like(mu)
    mean, rstd = torch.empty(M, device=DEV), torch.empty(M, device=DEV)
    a, w = torch.zeros(M, K, dtype=torch.bfloat16, device=DEV), torch.zeros(3 * K, K, dtype=torch.bfloat16, device=DEV)
    ops.qkv_fwd(a, w, torch.zeros(3 * K, device=DEV), 1, M, 2,
                fold=(gc.fold_stats(mu, sigma, K).to(DEV), c.float().to(DEV), 0.0, mean, rstd))
    assert set(sigma.tolist()) == set(gc.FOLD_SIGMAS)
    gc.assert_exact(rstd.cpu(), (1.0 / sigma).float(), "rsqf at sigma^2 in {1/4, 1, 4, 16}")
    lc._log("exact fold probe: the hardware reciprocal square root is exact at 1/4, 1, 4 and 16 (ln_rstd = 2, 1, 1/2, "
            "1/4 to the bit): every sigma kept, outputs compared on raw bits")


@pytest.mark.parametrize("K", FOLD_KS)
@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("kind,epi", [("linear", gc.EPI_BF16), ("gelu", gc.EPI_GELU)])
def test_fold_tile_edges(kind, epi, cfg, K):
    """``ln_st[m][slot]``, ``ln_c[n]``, ``ln_mean[m]`` / ``ln_rstd[m]`` indexing over ragged row
    and column tiles at 2, 4, 8, 16 (exact) and 12 (bounded) statistics slots."""
    bm, bn, _ = gc.TILES[cfg]
    with ops.gemm_tile(cfg):
        for M in gc.edge_ms(bm):
            for N in gc.edge_ns(bn):
                tile = assert_plan(cfg, epi, M, N, K)
                assert tile == (bm, bn)
                if kind == "linear":
                    assert_plan(cfg, gc.EPI_F32, M, N, K)
                gc.run_fold_consumer(kind, M, N, K, DEV, tile=tile)


@pytest.mark.parametrize("cfg", ALL_TILES)
@pytest.mark.parametrize("B,N,H,D", gc.FOLD_QKV_SHAPES + gc.FOLD_QKV_BOUNDED)
def test_fold_qkv_exact(cfg, B, N, H, D):
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_QKV, B * N, 3 * D, D)
        assert tile == gc.TILES[cfg][:2]
        gc.run_fold_consumer("qkv", B * N, 3 * D, D, DEV, tile=tile, geom=(B, N, H))


@pytest.mark.parametrize("cfg", TILES_4W)
@pytest.mark.parametrize("B,C,H,W,p,D", gc.HEAD_GEOMS)
def test_fold_head_exact(cfg, B, C, H, W, p, D):
    M = B * ((H // p) * (W // p) + 1)
    with ops.gemm_tile(cfg):
        tile = assert_plan(cfg, gc.EPI_HEAD, M, C * p * p, D)
        gc.run_fold_consumer("head", M, C * p * p, D, DEV, tile=tile, geom=(B, C, H, W, p))
