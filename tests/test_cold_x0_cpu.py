"""Cold-diffusion sampling and restoration for x0-predicting models, CPU side: the
reference step, the CPU op dispatch, the sampler against exact oracles and an eager
loop, defaults, errors and the command line."""
import os

import pytest
import torch

from ddim_cold_amd import ops
from ddim_cold_amd.diffusion.samplers import ColdSampler
from ddim_cold_amd.diffusion.schedule import cold_steps
from ddim_cold_amd.models.vit import DiffusionVisionTransformer
from ddim_cold_amd.ops import reference as ref


def _tiny(cls=DiffusionVisionTransformer):
    torch.manual_seed(0)
    m = cls(img_size=[16, 16], patch_size=4, embed_dim=64, depth=2, num_heads=2).eval()
    with torch.no_grad():  # a head that predicts something (zero bias at init: x0-hat ~ 0)
        m.head.bias.uniform_(-0.5, 0.5)
    return m


@pytest.mark.parametrize("size", [16, 24, 64, 200])
@pytest.mark.parametrize("C", [1, 3])
def test_reference_algebra_bit_exact(size, C):
    """x = D(img, t), x0 = img: algorithm 2 gives exactly D(img, t-1) (the two D(img, t)
    terms cancel before the addition), algorithm 1 gives D(x0, t-1), t = 0 changes nothing."""
    g = torch.Generator().manual_seed(size + C)
    img = torch.rand(2, C, size, size, generator=g) * 2 - 1
    other = torch.rand(2, C, size, size, generator=g) * 2 - 1
    for t in range(1, cold_steps(size) + 1):
        x = ref.pixelate(img, 2 ** t)
        tt = torch.tensor([t, 0])
        out = ref.cold_step(x, img, tt, 2)
        assert torch.equal(out[0], ref.pixelate(img, 2 ** (t - 1))[0]), t
        assert torch.equal(out[1], x[1]), t
        out1 = ref.cold_step(other, img, tt, 1)
        assert torch.equal(out1[0], ref.pixelate(img, 2 ** (t - 1))[0]), t
        assert torch.equal(out1[1], other[1]), t
    assert torch.equal(ref.cold_step(other, img, torch.tensor([1, 1]), 2),
                       (other - ref.pixelate(img, 2)) + img)  # subtraction first
    with pytest.raises(ValueError):
        ref.cold_step(other, img, torch.tensor([1, 1]), 3)


@pytest.mark.parametrize("alg", [1, 2])
@pytest.mark.parametrize("shape", [(3, 3, 16, 16, 4, [4, 2, 0]), (2, 3, 24, 24, 8, [4, 3]), (2, 1, 16, 16, 4, [1, 3])])
def test_cpu_op_dispatch(shape, alg):
    B, C, H, W, p, t = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, H, W, generator=g)
    x0 = torch.rand(B, C, H, W, generator=g) * 2 - 1
    tt = torch.tensor(t)
    exp = ref.cold_step(x, x0, tt, alg)
    NP, F = (H // p) * (W // p), C * p * p
    sentinel = 7.0
    # image layout: conv-order patch rows of the updated samples
    xi, po = x.clone(), torch.full((B * NP, F), sentinel, dtype=torch.bfloat16)
    ops.cold_step_(xi, x0, tt, alg, patches_out=po)
    assert torch.equal(xi, exp)
    want = ref.patchify_bf16(exp, p)
    # rows layout: the head's column order
    xr, x0r = ops.image_to_rows(x, p).contiguous(), ops.image_to_rows(x0, p).contiguous()
    pr = torch.full((B * NP, F), sentinel, dtype=torch.bfloat16)
    ops.cold_step_rows_(xr, x0r, tt, B, C, H, W, p, alg, patches_out=pr)
    assert torch.equal(ops.rows_to_image(xr, B, C, H, W, p), exp)
    for b in range(B):
        rows = slice(b * NP, (b + 1) * NP)
        if t[b] >= 1:
            assert torch.equal(po[rows], want[rows]) and torch.equal(pr[rows], xr[rows].to(torch.bfloat16))
        else:  # a skipped sample: x and its patch rows untouched
            assert torch.equal(xi[b], x[b]) and (po[rows] == sentinel).all() and (pr[rows] == sentinel).all()
    x2 = x.clone()
    ops.cold_step_(x2, x0, tt, alg)  # patches_out is optional
    assert torch.equal(x2, exp)


class _Oracle(DiffusionVisionTransformer):
    """A perfect x0 predictor: f(x, t) = x_star whatever x and t are."""

    def forward_reference(self, x, t):
        return self.x_star.to(x.device)


def test_oracle_restore_is_exact():
    m = _tiny(_Oracle)
    S = cold_steps(16)
    g = torch.Generator().manual_seed(3)
    m.x_star = torch.rand(4, 3, 16, 16, generator=g) * 2 - 1
    s = ColdSampler(m, "cpu", predict="x0", algorithm=2)
    seq = s.restore(m.x_star, S, sequence=True, unit=False)
    assert len(seq) == S + 1
    for i, t in enumerate(range(S, -1, -1)):
        assert torch.equal(seq[i], ref.pixelate(m.x_star, 2 ** t)), t
    assert torch.equal(s.restore(m.x_star, S, unit=False), m.x_star)
    # every sample joins at its own level and ends at its own x_star
    levels = [0, 1, 2, S]
    seq = s.restore(m.x_star, levels, sequence=True, unit=False)
    assert torch.equal(seq[-1], m.x_star)
    for i, t in enumerate(range(S, -1, -1)):
        for b, lv in enumerate(levels):
            assert torch.equal(seq[i][b], ref.pixelate(m.x_star[b:b + 1], 2 ** min(lv, t))[0]), (t, b)
    assert torch.equal(s.restore(m.x_star, levels), (m.x_star + 1) / 2)
    # algorithm 1 also ends at x_star (D(x_star, 0) = x_star)
    assert torch.equal(ColdSampler(m, "cpu", predict="x0", algorithm=1).restore(m.x_star, levels, unit=False),
                       m.x_star)


@pytest.mark.parametrize("alg", [1, 2])
def test_sampler_matches_eager_loop(alg):
    m = _tiny()
    s = ColdSampler(m, "cpu", predict="x0", algorithm=alg)
    N = 3
    seq = s.sequence(N, generator=torch.Generator().manual_seed(2))
    out = s.sample(N, generator=torch.Generator().manual_seed(2))
    x = s._init(N, torch.Generator().manual_seed(2))
    frames = [x]
    with torch.no_grad():
        for t in range(s.steps, 0, -1):
            x0 = m.forward_reference(x, torch.full((N,), t)).clamp(-1, 1)
            lo = ref.pixelate(x0, 2 ** (t - 1))
            x = (x - ref.pixelate(x0, 2 ** t)) + lo if alg == 2 else lo
            frames.append(x.clamp(-1, 1))
    assert len(seq) == s.steps + 1 == len(frames)
    assert torch.equal(seq[0], (frames[0] + 1) / 2)
    for a, b in zip(seq[1:], frames[1:]):
        assert torch.allclose(a, (b + 1) / 2, atol=1e-6)
    assert torch.allclose(seq[-1], out, atol=1e-6)
    assert (frames[-1] - frames[0].clamp(-1, 1)).abs().mean() > 0.1  # the loop did something


def test_defaults_and_errors():
    m = _tiny()
    a = ColdSampler(m, "cpu").sequence(2, generator=torch.Generator().manual_seed(5))
    b = ColdSampler(m, "cpu", predict="prev").sequence(2, generator=torch.Generator().manual_seed(5))
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(m.cold_sampler("cpu", N=2, generator=torch.Generator().manual_seed(5)), a[-1])
    with pytest.raises(ValueError):
        ColdSampler(m, "cpu", predict="eps")
    with pytest.raises(ValueError):
        ColdSampler(m, "cpu", predict="x0", algorithm=3)
    img = torch.zeros(2, 3, 16, 16)
    S = cold_steps(16)
    for bad in (S + 1, -1, [1, S + 1], [1]):
        with pytest.raises(ValueError):
            ColdSampler(m, "cpu", predict="x0").restore(img, bad)
    with pytest.raises(ValueError):  # the x_{t-1} rule has no per-sample skip
        ColdSampler(m, "cpu").restore(img, [1, 2])
    out = ColdSampler(m, "cpu").restore(img, [2, 2])
    assert out.shape == (2, 3, 16, 16) and out.min() >= 0 and out.max() <= 1
    big = torch.full((1, 3, 16, 16), 1.5)  # level 0: the clamped input comes back
    assert torch.equal(ColdSampler(m, "cpu", predict="x0").restore(big, 0, unit=False), big.clamp(-1, 1))
    out = m.cold_restore(img, [0, S], predict="x0")
    assert out.shape == (2, 3, 16, 16) and torch.equal(out[0], (img[0] + 1) / 2)


def test_restore_graph_cache_is_lru():
    from ddim_cold_amd.diffusion import samplers
    m = _tiny()
    s = ColdSampler(m, "cpu", predict="x0")
    img = torch.zeros(1, 3, 16, 16)
    count = lambda: sum(1 for k in m.__dict__["_sampler_graphs"] if k[0] == "cold_restore")  # noqa: E731
    s.restore(img, 1)
    s.restore(img, 1)
    assert count() == 1
    for alg in (1, 2):
        for lv in (1, 2, 3, 4):
            ColdSampler(m, "cpu", predict="x0", algorithm=alg).restore(torch.zeros(2, 3, 16, 16), [lv, 1])
    assert count() == samplers.COLD_RESTORE_GRAPHS


def test_cli_restore(tmp_path):
    import ViT_draft2drawing
    out = tmp_path / "out"
    out.mkdir()
    missing = str(tmp_path / "no_such_image.png")
    args = ["--ckpt", str(tmp_path / "no_ckpt.pkl"), "--restore", missing, "--out_dir", str(out)]
    assert ViT_draft2drawing.main(["--predict", "x0"] + args) == 0
    assert sorted(os.listdir(out)) == ["denoise_sequence.png", "restore.png"]
    assert ViT_draft2drawing.main(args + ["--algorithm", "1"]) == 0  # prev model: one call per level
    assert sorted(os.listdir(out)) == ["denoise_sequence.png", "denoise_sequence_1.png", "restore.png",
                                       "restore_1.png"]
