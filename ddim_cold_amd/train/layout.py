"""Where every parameter lives in the flat arenas, and which arena ranges the ranks exchange.

Both are functions of the parameters' names, shapes and ``requires_grad``, the model's depth,
dim and total steps, and a few ``EngineConfig`` fields: no tensor is needed, so this module is
standard library only.  :class:`TrainEngine` allocates its arenas from an :class:`ArenaLayout`
and issues its collectives from a :class:`BucketLayout`; ``parallel.costmodel`` sizes its
simulated buckets with :func:`bucket_groups`.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from types import MappingProxyType
from typing import Dict, FrozenSet, Mapping, Optional, Sequence, Tuple

ALIGN = 64  # elements (256 B fp32)
TEMB = "time_embed.weight"
Range = Tuple[int, int]


def _align(n: int) -> int:
    return (n + ALIGN - 1) // ALIGN * ALIGN


@dataclass(frozen=True)
class ArenaLayout:
    """``names`` / ``shapes``: the parameters in model order; ``offsets``: ``{name: (offset,
    numel)}`` in arena elements; ``numel``: the arena's size; ``train_hi``: where the frozen
    tensors start (the norm, AdamW and the all-reduce cover ``[0, train_hi)``); ``acc_hi``: the
    gradient arena below it is accumulated (embeddings: atomics in the embedding backward),
    above it every range has a single writer per step; ``ln_order``: the LayerNorms in backward
    order (final norm, then norm2, norm1 of blocks L-1 .. 0) and ``ln_offs`` the offset of each
    one's ``[2 dim]`` weight + bias range; ``block_starts``: the first Linear of each block,
    ``block_numel`` / ``head_numel``: the elements of one block's Linears and of the head's;
    ``temb``: the time-embedding table's ``(offset, numel)`` and ``temb_active_end`` the element
    after the last row a sample can select (None: every row can be, or the table is frozen);
    ``lazy``: the optimizer's lazily decayed ``(lo, hi)`` or None; ``sq_tiles``: the 64x64
    output tiles of the 2-D parameters, which bound the grad-norm partials.  The mapping is a
    read-only view: the value cannot be changed, only replaced."""
    names: Tuple[str, ...]
    shapes: Tuple[Tuple[int, ...], ...]
    offsets: Mapping[str, Range]
    numel: int
    train_hi: int
    acc_hi: int
    frozen: FrozenSet[str]
    ln_order: Tuple[str, ...]
    ln_offs: Tuple[int, ...]
    block_starts: Tuple[int, ...]
    block_numel: int
    head_numel: int
    temb: Range
    temb_active_end: Optional[int]
    lazy: Optional[Range]
    sq_tiles: int


def arena_layout(params: Sequence[Tuple[str, Sequence[int], bool]], depth: int, dim: int, total_steps: int,
                 temb_rows: Optional[int], weight_ema: float) -> ArenaLayout:
    """The arena layout of a model whose ``named_parameters()`` are ``params``, as ``(name,
    shape, requires_grad)`` in model order.  ``temb_rows``: every sample's t is below it (None:
    t spans the whole table)."""
    if temb_rows is not None and temb_rows < 1:
        raise ValueError(f"temb_rows must be None or at least 1 (no sample has t < {temb_rows})")
    names = tuple(n for n, _, _ in params)
    shapes = tuple(tuple(s) for _, s, _ in params)
    frozen = frozenset(n for n, _, rg in params if not rg)
    ln_order = ("norm",) + tuple(f"blocks.{i}.norm{k}" for i in range(depth - 1, -1, -1) for k in (2, 1))
    lns = frozenset(ln_order)

    def is_ln(n):
        return n.rsplit(".", 1)[0] in lns

    # arena order: embeddings, then EVERY LayerNorm, then the blocks' Linear
    # weights, then the head.  The LayerNorm gradients are finalised once, in the
    # embedding-backward launch (their dgamma/dbeta replicas are only complete
    # then); placed here they fall in the last all-reduce bucket, so data
    # parallel needs no replica finalize launch per bucket either.
    # Frozen tensors (requires_grad=False, e.g. the fixed sinusoidal time table,
    # ViT_draft2drawing.py:140-156) go last, past ``train_hi``: the norm, AdamW and
    # the all-reduce buckets cover [0, train_hi) only, so a frozen tensor gets no
    # weight decay, no moments and no optimizer state (torch.optim skips a
    # parameter whose .grad is None).
    def group(n):
        if n in frozen:
            return 4
        if is_ln(n):
            return 1
        if n.startswith("blocks."):
            return 2
        return 3 if n.startswith("head.") else 0
    order = sorted(range(len(names)), key=lambda i: group(names[i]))  # stable: model order within a group
    # LayerNorm weight+bias are packed back to back (one [2D] range for the
    # replica finalize); every other tensor starts 256-B aligned.
    offsets: Dict[str, Range] = {}
    off, train_hi = 0, None
    for i in order:
        n = names[i]
        if not (n.endswith(".bias") and is_ln(n)):
            off = _align(off)
        if n in frozen and train_hi is None:
            train_hi = off
        offsets[n] = (off, math.prod(shapes[i]))
        off += offsets[n][1]
    numel = _align(off)
    if train_hi is None:
        train_hi = numel
    for nm in ln_order:
        if offsets[nm + ".bias"][0] != offsets[nm + ".weight"][0] + dim:
            raise ValueError(f"{nm}: LayerNorm weight and bias must be adjacent in the arena (one [2 dim] range)")
    ln_offs = tuple(offsets[nm + ".weight"][0] for nm in ln_order)
    block_starts = tuple(min(offsets[n][0] for n in names if n.startswith(f"blocks.{i}.") and not is_ln(n))
                         for i in range(depth))

    def linears(prefix):
        return sum(offsets[n][1] for n in names if n.startswith(prefix) and not is_ln(n))
    # time_embed rows no sample can select (t >= temb_rows: cold diffusion draws
    # t in 1..log2 W): zero gradient and zero Adam moments for the whole run, so
    # the all-reduce leaves them out and AdamW reduces to p *= (1 - lr wd).  The
    # optimizer skips them (``lazy``, whole float4s) and accumulates that factor on
    # the device; ~11 % of the ViT-tiny arena.  Off with a weight EMA: the EMA of
    # those rows has to follow them every step.
    to, tn = temb = offsets[TEMB]
    active_end = lazy = None
    if temb_rows is not None and temb_rows < total_steps and TEMB not in frozen:
        active_end = to + temb_rows * dim
        lo, hi = (active_end + 3) // 4 * 4, (to + tn) // 4 * 4
        if hi > lo and not weight_ema > 0:
            lazy = (lo, hi)
    sq_tiles = sum(-(-s[0] // 64) * -(-math.prod(s[1:]) // 64) for s in shapes if len(s) >= 2)
    return ArenaLayout(names, shapes, MappingProxyType(offsets), numel, train_hi, min(ln_offs), frozen, ln_order,
                       ln_offs, block_starts, linears("blocks.0."), linears("head."), temb, active_end, lazy, sq_tiles)


def bucket_groups(depth: int, bucket_blocks: int, embed_bucket: bool) -> Tuple[Tuple[int, ...], ...]:
    """The block indices of each gradient bucket, in backward order: ``bucket_blocks`` blocks
    per bucket from the last block down.  The last bucket also holds the embeddings and every
    LayerNorm; with ``embed_bucket`` it holds nothing else."""
    bb = max(1, bucket_blocks)
    groups = tuple(tuple(range(hi, max(hi - bb, -1), -1)) for hi in range(depth - 1, -1, -bb))
    return groups + ((),) if embed_bucket else groups


@dataclass(frozen=True)
class BucketLayout:
    """``bounds``: each bucket's contiguous arena range, in backward order (they tile ``[0,
    train_hi)`` downwards); ``ranges``: the sub-ranges of each that are all-reduced;
    ``bucket_after``: ``{block: bucket}`` for the blocks whose backward closes a bucket, ``-1``
    for the embedding backward; ``ln_done_at``: under the same keys, how many LayerNorms (of
    ``ln_order``) have their gradient replicas complete there; ``temb_bucket``: the bucket whose
    collective also exchanges the time-embedding gradient as (t, row) pairs, else None;
    ``reduced_numel``: elements all-reduced per step.  The two mappings are read-only views."""
    bounds: Tuple[Range, ...]
    ranges: Tuple[Tuple[Range, ...], ...]
    bucket_after: Mapping[int, int]
    ln_done_at: Mapping[int, int]
    temb_bucket: Optional[int]
    reduced_numel: int


def bucket_layout(arena: ArenaLayout, bucket_blocks: int, embed_bucket: bool, sparse_temb: bool) -> BucketLayout:
    """All-reduce buckets: contiguous arena ranges with boundaries at the first Linear of a
    block (the LayerNorms live with the embeddings, see :func:`arena_layout`); frozen tensors,
    past ``train_hi``, are never reduced.  ``sparse_temb``: a time-embedding table whose every
    row can be selected is exchanged as the rows this step touched instead."""
    depth = len(arena.block_starts)
    groups = bucket_groups(depth, bucket_blocks, embed_bucket)
    bounds, bucket_after, ln_done_at = [], {}, {}
    end = arena.train_hi
    for j, g in enumerate(groups):
        last = j == len(groups) - 1
        key, lo = (-1, 0) if last else (g[-1], arena.block_starts[g[-1]])
        bounds.append((lo, end))
        bucket_after[key] = j
        ln_done_at[key] = len(arena.ln_order) if last else 1 + 2 * (depth - g[-1])
        end = lo
    # the part of the table that is not all-reduced: the rows no sample can select, or
    # (sparse exchange) all of it
    to, tn = arena.temb
    cut = None
    if arena.temb_active_end is not None:
        cut = (arena.temb_active_end, to + tn)
    elif sparse_temb:
        cut = (to, to + tn)
    ranges, temb_bucket = [], None
    for k, (a, b) in enumerate(bounds):
        if cut is not None and a <= cut[0] and cut[1] <= b:
            ranges.append(tuple(r for r in ((a, cut[0]), (cut[1], b)) if r[1] > r[0]))
            if arena.temb_active_end is None:
                temb_bucket = k
        else:
            ranges.append(((a, b),))
    return BucketLayout(tuple(bounds), tuple(ranges), MappingProxyType(bucket_after), MappingProxyType(ln_done_at),
                        temb_bucket, sum(b - a for rs in ranges for a, b in rs))
