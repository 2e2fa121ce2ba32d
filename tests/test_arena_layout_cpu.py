"""train/layout.py: where every parameter lives in the flat arenas and which arena ranges are
exchanged, checked as plain values -- no engine is built.  The table is that of
tools/layout_digest.py: three models under every combination of temb_rows, timestep_embedding,
weight_ema, force_segments, bucket_blocks and embed_bucket."""
import functools
import itertools
import math

import pytest

from ddim_cold_amd import build_model
from ddim_cold_amd.models import DiffusionVisionTransformer
from ddim_cold_amd.parallel import costmodel as cm
from ddim_cold_amd.train.layout import ALIGN, arena_layout, bucket_groups, bucket_layout

MODELS = {
    "vit_tiny": lambda **kw: build_model("vit_tiny", **kw),
    "vit_small_200": lambda **kw: build_model("vit_small_200", **kw),
    "16x16 depth 3": lambda **kw: DiffusionVisionTransformer(img_size=[16, 16], patch_size=4, embed_dim=32, depth=3,
                                                             num_heads=2, **kw),
}
ARENAS = list(itertools.product(MODELS, (7, None), ("learned", "sinusoidal"), (0.0, 0.99)))
BUCKETS = list(itertools.product((True, False), (1, 2, 3, 4, 7, 1 << 16), (True, False)))  # segments, blocks, embed


@functools.lru_cache(maxsize=None)
def _specs(name, temb):
    """``(params, depth, dim, total_steps)`` of a model: all that the layout reads of it."""
    m = MODELS[name](timestep_embedding=temb)
    return (tuple((n, tuple(p.shape), p.requires_grad) for n, p in m.named_parameters()), m.depth, m.embed_dim,
            m.total_steps)


def _arena(name, rows, temb, ema):
    params, depth, dim, total = _specs(name, temb)
    return arena_layout(params, depth, dim, total, rows, ema), dim


def _buckets(arena, temb, segmented, bb, eb):
    # as the engine passes it: EngineConfig.temb_sparse (default on), data parallel, a learned table
    return bucket_layout(arena, bb, eb, sparse_temb=segmented and temb == "learned")


@pytest.mark.parametrize("name,rows,temb,ema", ARENAS)
def test_layout_invariants(name, rows, temb, ema):
    """What the engine tests assert on single engines, for every arena and bucket layout.

    ``reduced_numel``: the bounds tile ``[0, train_hi)`` padding included (the engine reduces
    whole contiguous ranges, as tests/test_engine_cpu.py's data-parallel worker asserts of the
    16x16 model), so the padding is accounted for on both sides: ``train_hi`` is the trainable
    elements plus the padding below it, and ``reduced_numel`` is ``train_hi`` minus the
    unselectable rows and a sparsely exchanged table.  The padding is NOT subtracted: the
    16x16 model (87,184 trainable elements, 496 of padding, ``train_hi`` 87,680) reduces
    23,904 = 87,680 - 1,993 x 32 elements at temb_rows=7, not 23,408; vit_tiny and
    vit_small_200 have no padding."""
    A, D = _arena(name, rows, temb, ema)
    lns = {p + s for p in A.ln_order for s in (".weight", ".bias")}
    assert len(A.ln_order) == len(A.ln_offs) == 2 * len(A.block_starts) + 1 and len(lns) == 2 * len(A.ln_order)
    assert A.ln_order[0] == "norm" and A.ln_order[-1] == "blocks.0.norm1"
    # 64-aligned offsets, a LayerNorm bias directly behind its weight; nothing overlaps
    for n in A.names:
        o, k = A.offsets[n]
        if n in lns and n.endswith(".bias"):
            assert o == A.offsets[n[:-len("bias")] + "weight"][0] + D, n
        else:
            assert o % ALIGN == 0, n
        assert k == math.prod(A.shapes[A.names.index(n)])
    spans = sorted(A.offsets.values())
    assert all(a[0] + a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= A.numel
    assert A.numel % ALIGN == 0 and A.train_hi % ALIGN == 0
    # frozen tensors start at or above train_hi, every trainable one ends below it
    assert A.frozen == {n for n, _, rg in _specs(name, temb)[0] if not rg}
    assert (temb == "sinusoidal") == ("time_embed.weight" in A.frozen)
    assert all((A.offsets[n][0] >= A.train_hi) == (n in A.frozen) for n in A.names)
    assert all(sum(A.offsets[n]) <= A.train_hi for n in A.names if n not in A.frozen)
    trainable = sum(A.offsets[n][1] for n in A.names if n not in A.frozen)
    padding = A.train_hi - trainable  # alignment padding inside [0, train_hi)
    assert 0 <= padding < ALIGN * len(A.names)
    # the accumulated part of the gradient arena ends where the LayerNorms begin
    assert A.acc_hi == min(A.ln_offs) and all(A.offsets[n][0] < A.acc_hi or n in lns or n in A.frozen
                                               or n.startswith(("blocks.", "head.")) for n in A.names)
    assert A.temb == A.offsets["time_embed.weight"]
    to, tn = A.temb
    selectable_all = rows is None or temb == "sinusoidal"
    assert A.temb_active_end == (None if selectable_all else to + rows * D)
    # lazy: inside the table's arena range, both ends multiples of 4; off with a weight EMA
    if selectable_all or ema > 0:
        assert A.lazy is None
    else:
        lo, hi = A.lazy
        assert A.temb_active_end <= lo < hi <= to + tn and lo % 4 == 0 and hi % 4 == 0
        assert lo - A.temb_active_end < 4 and to + tn - hi < 4
    for segmented, bb, eb in BUCKETS:
        Bk = _buckets(A, temb, segmented, bb, eb)
        case = (segmented, bb, eb)
        # the bounds tile [0, train_hi) in descending order
        assert Bk.bounds[0][1] == A.train_hi and Bk.bounds[-1][0] == 0, case
        assert all(a[0] == b[1] for a, b in zip(Bk.bounds, Bk.bounds[1:])) and all(a < b for a, b in Bk.bounds), case
        assert len(Bk.bounds) == len(Bk.ranges) == len(Bk.bucket_after) == len(Bk.ln_done_at), case
        # the ranges lie inside their bounds and are disjoint
        for (a, b), rs in zip(Bk.bounds, Bk.ranges):
            assert rs and rs[0][0] >= a and rs[-1][1] <= b and all(lo < hi for lo, hi in rs), case
            assert all(x[1] <= y[0] for x, y in zip(rs, rs[1:])), case
        # every LayerNorm lies in the last bucket, its [2D] range too
        a, b = Bk.bounds[-1]
        assert all(a <= o and o + 2 * D <= b for o in A.ln_offs), case
        assert all(a <= A.offsets[n][0] < b for n in lns), case
        assert Bk.bucket_after[-1] == len(Bk.bounds) - 1 and Bk.ln_done_at[-1] == len(A.ln_order), case
        assert sorted(Bk.bucket_after.values()) == list(range(len(Bk.bounds))), case
        for blk, k in Bk.bucket_after.items():
            if blk >= 0:  # the bucket closed by block blk's backward starts at that block
                assert Bk.bounds[k][0] == A.block_starts[blk], case
                assert Bk.ln_done_at[blk] == 1 + 2 * (len(A.block_starts) - blk), case
        # what is not all-reduced: the unselectable rows, or a sparsely exchanged table
        sparse = segmented and temb == "learned" and rows is None
        assert (Bk.temb_bucket is not None) == sparse, case
        if sparse:
            a, b = Bk.bounds[Bk.temb_bucket]
            assert a <= to and to + tn <= b, case
        cut = tn if sparse else 0 if selectable_all else to + tn - A.temb_active_end
        assert Bk.reduced_numel == sum(hi - lo for rs in Bk.ranges for lo, hi in rs), case
        assert Bk.reduced_numel == A.train_hi - cut, case
        reduced = [r for rs in Bk.ranges for r in rs]
        if cut:  # exactly the cut is missing
            assert all(hi <= to + tn - cut or lo >= to + tn for lo, hi in reduced), case


def test_layout_values_vit_tiny_single_process():
    """Case A: vit_tiny, temb_rows=7, single process, defaults (values of the engine before
    the layout was a module of its own)."""
    A, _ = _arena("vit_tiny", 7, "learned", 0.0)
    B = _buckets(A, "learned", False, 2, True)
    assert len(A.names) == 93 and A.numel == A.train_hi == 7162176 and A.acc_hi == 867456
    assert A.lazy == (102144, 867456) and A.sq_tiles == 2136
    assert B.bounds == ((5314176, 7162176), (3540096, 5314176), (1766016, 3540096), (878976, 1766016), (0, 878976))
    assert B.ranges[-1] == ((0, 102144), (867456, 878976))
    assert A.block_numel == 887_040 and A.head_numel == 192 * 384 + 192  # the four Linears; the head
    assert all(rs == (b,) for rs, b in zip(B.ranges[:-1], B.bounds))
    assert B.bucket_after == {5: 0, 3: 1, 1: 2, 0: 3, -1: 4}
    assert B.ln_done_at == {5: 5, 3: 9, 1: 13, 0: 15, -1: 15}
    assert A.ln_offs[:3] == (878208, 877440, 876672) and B.temb_bucket is None


def test_layout_values_vit_tiny_sparse_table():
    """Case B: as A with temb_rows=None, force_segments=True."""
    A, _ = _arena("vit_tiny", None, "learned", 0.0)
    B = _buckets(A, "learned", True, 2, True)
    assert len(A.names) == 93 and A.numel == A.train_hi == 7162176 and A.acc_hi == 867456
    assert A.lazy is None and A.sq_tiles == 2136
    assert B.bounds == ((5314176, 7162176), (3540096, 5314176), (1766016, 3540096), (878976, 1766016), (0, 878976))
    assert B.ranges[-1] == ((0, 99456), (867456, 878976)) and B.temb_bucket == 4
    assert all(rs == (b,) for rs, b in zip(B.ranges[:-1], B.bounds))
    assert B.bucket_after == {5: 0, 3: 1, 1: 2, 0: 3, -1: 4}
    assert B.ln_done_at == {5: 5, 3: 9, 1: 13, 0: 15, -1: 15}
    assert A.ln_offs[:3] == (878208, 877440, 876672)


def test_layout_values_vit_tiny_frozen_table():
    """Case C: vit_tiny with timestep_embedding="sinusoidal", temb_rows=7, force_segments=True,
    bucket_blocks=4."""
    A, _ = _arena("vit_tiny", 7, "sinusoidal", 0.0)
    B = _buckets(A, "sinusoidal", True, 4, True)
    assert A.numel == 7162176 and A.train_hi == 6394176 and A.acc_hi == 99456 and A.lazy is None
    assert B.bounds == ((2772096, 6394176), (110976, 2772096), (0, 110976))
    assert B.ranges == tuple((b,) for b in B.bounds)  # each reduced whole
    assert B.bucket_after == {3: 0, 0: 1, -1: 2} and B.ln_done_at == {3: 9, 0: 15, -1: 15}
    assert A.ln_offs[:3] == (110208, 109440, 108672)


def test_layout_values_vit_small_200_no_embed_bucket():
    """Case D: vit_small_200, temb_rows=7, force_segments=True, embed_bucket=False."""
    A, _ = _arena("vit_small_200", 7, "learned", 0.0)
    B = _buckets(A, "learned", True, 2, False)
    assert len(A.names) == 153 and A.numel == 11820480 and A.acc_hi == 1082880
    assert A.lazy == (317568, 1082880) and A.sq_tiles == 6582
    assert len(B.bounds) == 6 and B.bounds[0] == (9972480, 11820480) and B.bounds[-1] == (0, 2876160)
    assert [a for a, _ in B.bounds] == [9972480, 8198400, 6424320, 4650240, 2876160, 0]
    assert B.ranges[-1] == ((0, 317568), (1082880, 2876160))
    assert B.bucket_after == {10: 0, 8: 1, 6: 2, 4: 3, 2: 4, -1: 5}
    assert B.ln_done_at == {10: 5, 8: 9, 6: 13, 4: 17, 2: 21, -1: 25}


def test_layernorm_bias_must_follow_its_weight():
    params, depth, dim, total = _specs("16x16 depth 3", "learned")
    i = [n for n, _, _ in params].index("blocks.1.norm2.weight")
    assert params[i + 1][0] == "blocks.1.norm2.bias"
    arena_layout(params, depth, dim, total, 7, 0.0)
    between = params[:i + 1] + (("blocks.1.norm2.scale", (dim,), True),) + params[i + 1:]
    with pytest.raises(ValueError, match="blocks.1.norm2"):
        arena_layout(between, depth, dim, total, 7, 0.0)


def test_temb_rows_below_one_is_refused_and_the_mappings_are_read_only():
    params, depth, dim, total = _specs("16x16 depth 3", "learned")
    for rows in (0, -3):  # no sample has t < 0
        with pytest.raises(ValueError, match="temb_rows"):
            arena_layout(params, depth, dim, total, rows, 0.0)
    assert arena_layout(params, depth, dim, total, total, 0.0).temb_active_end is None  # every row selectable
    A = arena_layout(params, depth, dim, total, 1, 0.0)
    B = bucket_layout(A, 2, True, False)
    for m, key in ((A.offsets, "norm.weight"), (B.bucket_after, -1), (B.ln_done_at, -1)):
        with pytest.raises(TypeError):
            m[key] = 0


@pytest.mark.parametrize("depth", [7, 12])
def test_bucket_groups_and_cost_model_agree(depth):
    prof = cm.vit_step_profile(depth, 384, 384, 2080, 176_832)
    for bb in range(1, depth + 1):
        for eb in (True, False):
            groups = bucket_groups(depth, bb, eb)
            assert [len(g) for g in groups] == [k for k, _ in cm.bucket_plan(prof, bb, eb)], (bb, eb)
            # every block once, in backward order; bb blocks per bucket until they run out
            assert [i for g in groups for i in g] == list(range(depth - 1, -1, -1))
            blocks = [len(g) for g in groups[:-1]] if eb else [len(g) for g in groups]
            assert groups[-1] == () if eb else groups[-1][-1] == 0
            assert all(k == bb for k in blocks[:-1]) and 1 <= blocks[-1] <= bb
