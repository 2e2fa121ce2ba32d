"""The samplers' loop cache (one lookup for every kind of loop) and the named head step that
crosses from the samplers into ``ViTProgram.forward``."""
import pytest
import torch

from ddim_cold_amd import build_model, ops
from ddim_cold_amd.diffusion import samplers as smp
from ddim_cold_amd.models.program import HeadStep, model_tensors
from ddim_cold_amd.models.vit import DiffusionVisionTransformer

CPU = torch.device("cpu")


@pytest.fixture()
def model():
    torch.manual_seed(0)
    return DiffusionVisionTransformer(img_size=[16, 16], patch_size=4, embed_dim=32, depth=2, num_heads=2).eval()


@pytest.fixture()
def built(monkeypatch):
    """Counts ``_Denoiser`` constructions (what a cache hit must not do)."""
    made = []
    init = smp._Denoiser.__init__

    def counting(self, *a, **k):
        made.append(1)
        init(self, *a, **k)
    monkeypatch.setattr(smp._Denoiser, "__init__", counting)
    return made


def _kinds(model):
    return [k[0] for k in smp._cache(model)]


def test_hit_returns_the_same_state_and_builds_no_denoiser(model, built):
    s = smp.DDIMSampler(model, CPU, k=400)
    st = s._state(2, False)
    assert isinstance(st, smp._LoopState) and len(built) == 1
    assert s._state(2, False) is st and smp.DDIMSampler(model, CPU, k=400)._state(2, False) is st
    assert len(built) == 1
    assert s._state(2, True) is not st and len(built) == 2  # another key: another loop
    out = s.sample(2, generator=torch.Generator().manual_seed(1))
    assert torch.equal(out, s.sample(2, generator=torch.Generator().manual_seed(1))) and len(built) == 2


@pytest.mark.parametrize("limit", [None, 3])
def test_stale_entry_is_rebuilt_under_the_same_key(model, built, limit):
    """The key of the captured weights no longer matches (a parameter's ``_version`` moved):
    the loop is rebuilt in place; with a limit the rebuilt key does not count against it."""
    key = ("img2img", 0)
    build = lambda: smp._LoopState(smp._Denoiser(model, CPU).key(), None, None)  # noqa: E731
    others = [("img2img", i) for i in (1, 2)]
    for k in others:
        smp._cached_loop(model, k, build, limit)
    st = smp._cached_loop(model, key, build, limit)
    assert smp._cached_loop(model, key, build, limit) is st and len(built) == 3
    with torch.no_grad():
        model.head.bias.add_(1.0)
    st2 = smp._cached_loop(model, key, build, limit)
    assert st2 is not st and st2.key == smp._Denoiser.key_of(model) and len(built) == 4
    assert smp._cached_loop(model, key, build, limit) is st2 and len(built) == 4
    assert set(smp._cache(model)) == {key, *others}  # limit 3: nothing evicted for the rebuild


def test_sampler_loop_is_rebuilt_after_a_weight_update(model, built):
    s = smp.DDIMSampler(model, CPU, k=400)
    a = s.sample(2, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        model.head.bias.add_(0.25)
    b = s.sample(2, generator=torch.Generator().manual_seed(1))
    assert len(built) == 2 and _kinds(model) == ["ddim"] and not torch.equal(a, b)


def test_img2img_eta_loops_are_capped_like_img2img_loops(model):
    x = torch.randn(2, 3, 16, 16, generator=torch.Generator().manual_seed(5))
    smp.DDIMSampler(model, CPU, k=400).sample(2, generator=torch.Generator().manual_seed(1))
    smp.ddim_from_starts(model, x, [1599, 1999], 400)
    for i in range(smp.IMG2IMG_GRAPHS + 3):  # distinct keys
        smp.ddim_from_starts(model, x, [1999 - 100 * i, 1999], 100, eta=0.5, noise_seed=3)
    kinds = _kinds(model)
    assert kinds.count("img2img_eta") == smp.IMG2IMG_GRAPHS
    # the most recent ones stay, and no other kind paid for them
    last = [k[2] for k in smp._cache(model) if k[0] == "img2img_eta"]
    assert last == [(1999 - 100 * i, 1999) for i in range(3, smp.IMG2IMG_GRAPHS + 3)]
    assert kinds.count("img2img") == 1 and kinds.count("ddim") == 1


def test_one_kind_never_evicts_another(model):
    build = lambda: smp._LoopState(smp._Denoiser.key_of(model), None, None)  # noqa: E731
    for i in range(4):
        smp._cached_loop(model, ("cold_restore", i), build, 2)
    for i in range(3):
        smp._cached_loop(model, ("img2img", i), build, 2)
    smp._cached_loop(model, ("cold", 0), build)
    assert list(smp._cache(model)) == [("cold_restore", 2), ("cold_restore", 3), ("img2img", 1), ("img2img", 2),
                                       ("cold", 0)]
    smp._cached_loop(model, ("cold_restore", 2), build, 2)  # a hit: now the most recent of its kind
    smp._cached_loop(model, ("cold_restore", 4), build, 2)
    assert [k for k in smp._cache(model) if k[0] == "cold_restore"] == [("cold_restore", 2), ("cold_restore", 4)]
    assert _kinds(model).count("img2img") == 2 and _kinds(model).count("cold") == 1


def test_head_step_defaults_and_frozen():
    hs = HeadStep(ops.HEAD_CLAMP)
    assert (hs.x0_out, hs.coef, hs.patches_in, hs.patches_out, hs.rows_w, hs.noise) == (None,) * 6
    with pytest.raises(AttributeError):
        hs.mode = ops.HEAD_DDIM
    assert (ops.HEAD_DDIM, ops.HEAD_CLAMP, ops.HEAD_DDIM_EACH, ops.HEAD_ETA, ops.HEAD_ETA_EACH) == (1, 2, 4, 5, 6)


def test_head_step_rows_noise_goes_with_the_eta_modes_only():
    B, NP, F, D = 2, 16, 48, 32
    a, w, b = torch.zeros(B * (NP + 1), D), torch.zeros(F, D), torch.zeros(F)
    x, x0 = torch.zeros(B * NP, F), torch.zeros(B * NP, F)
    noise = (torch.tensor([1, 0]), ops.SITE_STEP_NOISE)
    for mode, coef in ((ops.HEAD_ETA, torch.zeros(8)), (ops.HEAD_ETA_EACH, torch.zeros(B, 8))):
        with pytest.raises(ValueError, match="modes 5 / 6 take noise"):
            ops.head_step_rows_(a, w, b, x, x0, coef, B, mode)
    for mode, coef in ((ops.HEAD_DDIM, torch.ones(4)), (ops.HEAD_CLAMP, None), (ops.HEAD_DDIM_EACH, torch.ones(B, 4))):
        with pytest.raises(ValueError, match="the other modes take none"):
            ops.head_step_rows_(a, w, b, x, x0, coef, B, mode, noise=noise)
    ops.head_step_rows_(a, w, b, x, x0, torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]), B, ops.HEAD_ETA,
                        noise=noise)  # the right pairing runs


@pytest.mark.gpu
def test_head_step_misuse_raises_on_the_folded_program():
    """A field in the wrong place is an error, not a silent wrong answer: the patch-row state
    without ``patches_in``, and noise without the patch-row state."""
    torch.manual_seed(0)
    m = build_model("vit_tiny").cuda().eval()
    P, prog = model_tensors(m), m.program()
    assert P.folded
    x = torch.randn(2, 3, 64, 64, device="cuda")
    x0, t = torch.zeros_like(x), torch.full((2,), 5, dtype=torch.int64, device="cuda")
    rng = torch.zeros(2, dtype=torch.int64, device="cuda")
    coef4 = torch.tensor([0.0, 1.0, 0.0, 1.0], device="cuda")
    coef8 = torch.tensor([0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0], device="cuda")
    w = ops.embed_weight_rows(P.pe_w, 3, m.patch_size).contiguous()
    noise = (torch.tensor([1, 0], device="cuda"), ops.SITE_STEP_NOISE)

    def forward(hs):
        with torch.no_grad():
            prog.forward(P, x, t, rng, False, save=False, head_step=hs)
    with pytest.raises(ValueError, match="the patch-row sampler state needs patches_in"):
        forward(HeadStep(ops.HEAD_DDIM, x0, coef4, rows_w=w))
    with pytest.raises(ValueError, match="need the patch-row sampler state"):
        forward(HeadStep(ops.HEAD_ETA, x0, coef8, noise=noise))
    forward(HeadStep(ops.HEAD_DDIM, x0, coef4))  # the identity row: x stays, x0 is the clamped prediction
    torch.cuda.synchronize()
    assert torch.isfinite(x0).all() and x0.abs().max() <= 1.0
