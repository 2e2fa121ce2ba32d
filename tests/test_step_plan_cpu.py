"""The training step's decisions are explicit: ``TrainEngine._plan(B)`` (a ``StepPlan`` with its
``BackwardPlan``) for a table of configurations on CPU engines, the GPU-only decisions through
the pure ``step_decisions`` with ``is_cuda=True``, the plan cache's invalidations, the
combinations ``BackwardPlan`` refuses, and plain tuples where the named bundles are consumed."""
import dataclasses

import pytest
import torch

from ddim_cold_amd import ops
from ddim_cold_amd.models import DiffusionVisionTransformer
from ddim_cold_amd.models.program import BackwardPlan
from ddim_cold_amd.train import engine as engine_mod
from ddim_cold_amd.train.engine import EngineConfig, StepPlan, Switches, TrainEngine, step_decisions

CFG = dict(img_size=[16, 16], patch_size=4, embed_dim=32, depth=3, num_heads=2)
SWITCH_NAMES = dict(ln_final="FUSE_LN_FINAL", sqnorm="FUSE_SQNORM", embed_wgrad="FUSE_EMBED_WGRAD",
                    overwrite="GRAD_OVERWRITE")


def _engine(model_kw=None, **cfg):
    torch.manual_seed(0)
    model = DiffusionVisionTransformer(**CFG, **(model_kw or {})).train()
    return TrainEngine(model, EngineConfig(**dict(dict(temb_rows=7, use_graph=False), **cfg)), device="cpu")


# (engine config, model config, switch turned off) -> the StepPlan fields that differ from DEFAULT.
# depth 3 with bucket_blocks 2: a bucket closes after block 1, block 0 only with an embedding bucket
DEFAULT = dict(k_acc=1, tail=True, fused_loss=True, fuse_batch=True, merge=True, flush_at=None, overwrite=False,
               fuse_sq=False, embed_owners=None, ln_final=None)
TABLE = {
    "defaults": ({}, {}, None, {}),
    "grad_accum=2": (dict(grad_accum=2), {}, None, dict(k_acc=2)),
    "segments + embed bucket": (dict(force_segments=True), {}, None, dict(merge=False, flush_at=frozenset({1, 0}))),
    "segments, no embed bucket": (dict(force_segments=True, embed_bucket=False), {}, None,
                                  dict(flush_at=frozenset({1}))),
    "fuse_batch=False": (dict(fuse_batch=False), {}, None, dict(fuse_batch=False)),
    "frozen time embedding": ({}, dict(timestep_embedding="sinusoidal"), None, {}),
    "temb_rows=None": (dict(temb_rows=None), {}, None, {}),
    **{f"{name} off": ({}, {}, name, {}) for name in SWITCH_NAMES},
}


@pytest.mark.parametrize("case", list(TABLE))
def test_cpu_engine_plan(case, monkeypatch):
    cfg, model_kw, off, diff = TABLE[case]
    if off is not None:
        monkeypatch.setattr(engine_mod, SWITCH_NAMES[off], False)
    eng = _engine(model_kw, **cfg)
    plan = eng._plan(4)
    assert isinstance(plan, StepPlan)
    got = {f.name: getattr(plan, f.name) for f in dataclasses.fields(plan) if f.name != "backward"}
    assert got == dict(DEFAULT, **diff)  # (on CPU: overwrite, fuse_sq and ln_final are off)
    b = plan.backward
    assert b.ln_ws is eng.ln_ws and b.embed_with_block0 == plan.merge and b.flush_at == plan.flush_at
    assert b.ln_final is None and b.store is False and b.grad_norm is None and b.owners is None and b.tickets is None
    assert (eng.grad_tensors.temb is None) == (case == "frozen time embedding")
    assert eng._emb_owners(8) == (8 if case == "temb_rows=None" else 7) and eng._emb_owners(4) == 4
    # cached by batch size; dropped with the capture, and when a batch size reallocates the buffers
    assert eng._plan(4) is plan
    eng._drop_capture(rewarm=False)
    plan2 = eng._plan(4)
    assert plan2 is not plan
    ws = eng.ln_ws
    big = eng._plan(64)
    assert eng.ln_ws is not ws and big.backward.ln_ws is eng.ln_ws
    assert eng._plan(4) is not plan2 and eng._plan(4).backward.ln_ws is eng.ln_ws


ON = dict(merge=True, ln_final=True, overwrite=True, fuse_sq=True, embed_fused=True)
# (config, switches off, world, segmented, is_cuda, B, has_temb_grad) -> the decisions that are off
GPU_TABLE = {
    "defaults": (({}, (), 1, False, True, 8, True), ()),
    "B=256": (({}, (), 1, False, True, 256, True), ()),
    "B=257": (({}, (), 1, False, True, 257, True), ("embed_fused",)),
    "grad_accum=2": ((dict(grad_accum=2), (), 1, False, True, 8, True), ("overwrite", "fuse_sq", "embed_fused")),
    "segments + embed bucket": ((dict(force_segments=True), (), 1, True, True, 8, True),
                                ("merge", "fuse_sq", "embed_fused")),
    "segments, no embed bucket": ((dict(force_segments=True, embed_bucket=False), (), 1, True, True, 8, True),
                                  ("fuse_sq", "embed_fused")),
    "two ranks": (({}, (), 2, True, True, 8, True), ("merge", "fuse_sq", "embed_fused")),
    "frozen time embedding": (({}, (), 1, False, True, 8, False), ("embed_fused",)),
    "temb_rows=None": ((dict(temb_rows=None), (), 1, False, True, 8, True), ()),
    "ln_final off": (({}, ("ln_final",), 1, False, True, 8, True),
                     ("ln_final", "overwrite", "fuse_sq", "embed_fused")),
    "sqnorm off": (({}, ("sqnorm",), 1, False, True, 8, True), ("fuse_sq", "embed_fused")),
    "embed_wgrad off": (({}, ("embed_wgrad",), 1, False, True, 8, True), ("embed_fused",)),
    "overwrite off": (({}, ("overwrite",), 1, False, True, 8, True), ("overwrite", "fuse_sq", "embed_fused")),
    "cpu": (({}, (), 1, False, False, 8, True), ("ln_final", "overwrite", "fuse_sq", "embed_fused")),
}


@pytest.mark.parametrize("case", list(GPU_TABLE))
def test_gpu_decisions_without_a_device(case):
    (cfg, off, world, segmented, is_cuda, B, temb), expect_off = GPU_TABLE[case]
    sw = Switches(**{name: False for name in off})
    got = step_decisions(EngineConfig(**cfg), sw, world, segmented, is_cuda, B, temb)
    assert got == {k: k not in expect_off for k in ON}


def test_backward_plan_rejects_illegal_combinations():
    z = torch.zeros(4)
    gn = ops.GradNorm(z, z)
    with pytest.raises(ValueError, match="single deferred"):  # grad-norm partials need the ONE launch
        BackwardPlan(grad_norm=gn, flush_at=frozenset({0}))
    with pytest.raises(ValueError, match="grad_norm and embed_with_block0"):
        BackwardPlan(owners=4, embed_with_block0=True)
    with pytest.raises(ValueError, match="grad_norm and embed_with_block0"):
        BackwardPlan(owners=4, grad_norm=gn, embed_with_block0=False)
    ln = ops.LnFinal(z, z, 4, 1)
    with pytest.raises(ValueError, match="workspace"):
        BackwardPlan(ln_final=ln)
    with pytest.raises(ValueError, match="offs"):
        BackwardPlan(ln_ws=z, ln_final=ln, owners=4, grad_norm=gn, embed_with_block0=True)
    BackwardPlan(ln_ws=z, ln_final=ln._replace(offs=[0]), owners=4, grad_norm=gn, embed_with_block0=True)
    with pytest.raises(dataclasses.FrozenInstanceError):
        BackwardPlan().store = True


def test_wgrad_multi_takes_plain_tuples_on_the_reference_path():
    g = torch.Generator().manual_seed(3)
    T, B, N, D = 6, 2, 3, 8
    arena = torch.zeros(8 * 4 + 8)
    dy, x = torch.randn(T, 8, generator=g), torch.randn(T, 4, generator=g)
    jobs = [(dy, x, arena[:32].view(8, 4), arena[32:])]
    parts = torch.zeros(1024)
    ops.linear_wgrad_multi(jobs, sq=(parts, arena, None))  # a plain 3-tuple
    assert torch.allclose(arena[:32].view(8, 4), dy.t() @ x, atol=1e-5)
    assert float(parts.sum()) == pytest.approx(float(arena.pow(2).sum()), rel=1e-6)

    ge = torch.randn(B, N, D, generator=g)
    t = torch.tensor([1, 3])
    rng = torch.tensor([5, 0], dtype=torch.int64)
    dcls, dpos, dtemb = torch.zeros(D), torch.zeros(N, D), torch.zeros(4, D)
    ops.linear_wgrad_multi(jobs, embed=(ge, t, rng, 1, 0.0, dcls, dpos, dtemb, B, None))  # a plain 10-tuple
    assert torch.allclose(dcls, ge[:, 0].sum(0)) and torch.allclose(dpos, ge.sum(0))
    assert torch.allclose(dtemb[t], ge.sum(1)) and float(dtemb[[0, 2]].abs().max()) == 0.0
    with pytest.raises(ValueError, match="offs"):  # the LayerNorm finalize there needs its arena offsets
        ops.linear_wgrad_multi(jobs, embed=(ge, t, rng, 1, 0.0, dcls, dpos, dtemb, B, (parts, parts, 4, 1)))
