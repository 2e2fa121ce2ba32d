"""Cold-diffusion sampling and restoration for x0-predicting models on the GPU: the
cold-step kernel against the CPU reference (bit for bit), and ``ColdSampler(predict=
"x0")`` / ``restore`` (one hipGraph, patch-row state) against the fp32 eager loop."""
import pytest
import torch

from ddim_cold_amd import build_model, ops
from ddim_cold_amd.diffusion import samplers
from ddim_cold_amd.diffusion.samplers import ColdSampler
from ddim_cold_amd.ops import reference as ref

DEV = "cuda"
# the project's cold-sampler bounds (test_sampler_gpu.py), final images in [0, 1]
MEAN_BOUND, MAX_BOUND = 0.01, 0.2

# (B, C, H, W, patch, t): skipped samples, one channel, non-uniform blocks (24, 200), the
# whole image as one block, block == patch, block > patch, block < patch
KERNEL_CASES = [
    (3, 3, 16, 16, 4, [4, 2, 0]),
    (3, 3, 16, 16, 4, [1, 1, 1]),
    (2, 1, 16, 16, 4, [3, 1]),
    (2, 3, 24, 24, 8, [4, 3]),
    (2, 3, 64, 64, 8, [6, 3]),
    (2, 3, 64, 64, 8, [4, 1]),
    (2, 3, 64, 64, 4, [5, 2]),
    (1, 3, 200, 200, 8, [7]),
    (1, 3, 200, 200, 8, [4]),
]
SENTINEL = 7.0


@pytest.mark.gpu
@pytest.mark.parametrize("alg", [1, 2])
@pytest.mark.parametrize("case", KERNEL_CASES, ids=lambda c: "x".join(str(v) for v in c[:5]) + "-t" + "_".join(map(str, c[5])))
def test_cold_step_kernel_matches_reference(case, alg):
    B, C, H, W, p, t = case
    g = torch.Generator().manual_seed(B * 1000 + H + p + sum(t))
    x = torch.randn(B, C, H, W, generator=g)
    x0 = torch.rand(B, C, H, W, generator=g) * 2 - 1
    for b in range(B):
        if t[b] == 0:
            x[b] = SENTINEL
    tt = torch.tensor(t)
    exp = ref.cold_step(x.clone(), x0.clone(), tt, alg)  # CPU reference from copies of the inputs
    NP, F = (H // p) * (W // p), C * p * p
    xi, po = x.to(DEV), torch.full((B * NP, F), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.cold_step_(xi, x0.to(DEV), tt.to(DEV), alg, patches_out=po)
    xr = ops.image_to_rows(x, p).contiguous().to(DEV)
    pr = torch.full((B * NP, F), SENTINEL, dtype=torch.bfloat16, device=DEV)
    ops.cold_step_rows_(xr, ops.image_to_rows(x0, p).contiguous().to(DEV), tt.to(DEV), B, C, H, W, p, alg,
                        patches_out=pr)
    torch.cuda.synchronize()
    xi, po, xr, pr = xi.cpu(), po.cpu(), xr.cpu(), pr.cpu()
    assert torch.equal(xi, exp)
    assert torch.equal(xr, ops.image_to_rows(xi, p))
    want_conv, want_rows = ref.patchify_bf16(exp, p), ops.image_to_rows(exp, p).to(torch.bfloat16)
    for b in range(B):
        rows = slice(b * NP, (b + 1) * NP)
        if t[b] >= 1:
            assert torch.equal(po[rows], want_conv[rows]) and torch.equal(pr[rows], want_rows[rows])
        else:  # skipped: x and the patch rows still hold the sentinel
            assert (xi[b] == SENTINEL).all() and (po[rows] == SENTINEL).all() and (pr[rows] == SENTINEL).all()
    x2 = x.to(DEV)
    ops.cold_step_(x2, x0.to(DEV), tt.to(DEV), alg)  # no patches_out
    assert torch.equal(x2.cpu(), exp)


@pytest.mark.gpu
def test_cold_step_binding_checks():
    x = torch.zeros(2, 3, 16, 16, device=DEV)
    x0 = torch.zeros_like(x)
    t = torch.ones(2, dtype=torch.int64, device=DEV)
    po = torch.zeros(2 * 16, 48, dtype=torch.bfloat16, device=DEV)
    x18 = torch.zeros(2, 3, 18, 18, device=DEV)
    bad = [
        lambda: ops.cold_step_(x, x, t, 2),                                # aliasing
        lambda: ops.cold_step_(x, x0, t, 3),                               # algorithm
        lambda: ops.cold_step_(x, x0, t[:1], 2),                           # t.numel() != B
        lambda: ops.cold_step_(x, x0, t.int(), 2),                         # dtype
        lambda: ops.cold_step_(x, x0.cpu(), t, 2),                         # device
        lambda: ops.cold_step_(x, x0.double(), t, 2),                      # dtype
        lambda: ops.cold_step_(x, x0, t, 2, patches_out=po.float()),       # patches_out dtype
        lambda: ops.cold_step_(x, x0, t, 2, patches_out=po[:16]),          # patches_out shape
        lambda: ops.cold_step_rows_(x.view(32, 48), x0.view(32, 48), t, 2, 3, 16, 16, 8, 2),  # F != C*p*p
        lambda: ops.cold_step_rows_(x18.view(-1, 27), x18.clone().view(-1, 27), t, 2, 3, 18, 18, 3, 2),  # F % 4
        lambda: ops.cold_step_(x.permute(0, 1, 3, 2), x0, t, 2),           # contiguity
    ]
    for f in bad:
        with pytest.raises((RuntimeError, ValueError)):
            f()
    torch.cuda.synchronize()
    assert x.abs().max().item() == 0.0  # nothing was launched


@pytest.fixture(scope="module")
def model():
    """vit_tiny with a loud head bias: at random init the head's output is ~ 0, and a
    sampler whose x0-hat is ~ 0 would test little."""
    torch.manual_seed(0)
    m = build_model("vit_tiny")
    with torch.no_grad():
        m.head.bias.uniform_(-0.5, 0.5)
    return m.to(DEV).eval()


def _eager(model, start, levels, alg):
    """fp32 eager loop (forward_reference + the reference step) from ``start`` ([-1, 1]);
    ``levels[b]``: where sample b joins the grid.  Returns the clamped states."""
    x = start.to(DEV)
    B, top = x.shape[0], max(levels)
    frames = []
    with torch.no_grad():
        for t in range(top, 0, -1):
            x0 = model.forward_reference(x, torch.full((B,), t, device=DEV)).clamp(-1, 1)
            x = ref.cold_step(x, x0, torch.tensor([t if v >= t else 0 for v in levels]), alg)
            frames.append(x.clamp(-1, 1).cpu())
    return frames


@pytest.fixture(scope="module")
def eager_sample(model):
    """The reference trajectories of the sampling test, computed once per algorithm."""
    s = ColdSampler(model, DEV, predict="x0")
    init = s._init(4, torch.Generator().manual_seed(2))
    return init, {alg: _eager(model, init, [s.steps] * 4, alg) for alg in (1, 2)}


@pytest.mark.gpu
@pytest.mark.parametrize("alg", [1, 2])
def test_x0_sampler_matches_eager_reference(model, eager_sample, alg):
    """Graph + patch-row sampler vs the fp32 eager loop from the same start, within the
    project's cold-sampler bounds.  Measured on MI355X: algorithm 1 mean |d| 0.00081, max
    0.0046; algorithm 2 mean 0.00122, max 0.0133 (mean |x_0 - x_T| 0.70 and 0.41)."""
    init, frames = eager_sample
    exp = frames[alg][-1]
    # a condition, not a measurement: a loop that changes nothing must not pass
    moved = (exp - init.clamp(-1, 1)).abs().mean().item()
    assert moved > 0.25, moved
    s = ColdSampler(model, DEV, predict="x0", algorithm=alg)
    assert s.use_graph and samplers.ROWS
    out = s.sample(4, generator=torch.Generator().manual_seed(2))
    d = (out - (exp + 1) / 2).abs()
    print(f"cold x0 algorithm {alg}: mean |x_0 - x_T| {moved:.3f}; vs eager mean |d| {d.mean():.5f} "
          f"max |d| {d.max():.5f}")
    assert d.mean() < MEAN_BOUND and d.max() < MAX_BOUND, (d.mean(), d.max())
    out2 = ColdSampler(model, DEV, predict="x0", algorithm=alg).sample(4, generator=torch.Generator().manual_seed(2))
    assert torch.equal(out, out2)  # a replay
    seq = s.sequence(4, generator=torch.Generator().manual_seed(2))
    assert len(seq) == s.steps + 1 and torch.allclose(seq[-1], out, atol=1e-6)
    assert torch.equal(seq[0], (init + 1) / 2)


@pytest.mark.gpu
@pytest.mark.parametrize("alg", [1, 2])
def test_x0_sampler_rows_match_image_layout(model, alg):
    seqs = {}
    for rows in (True, False):
        samplers.ROWS = rows
        model.__dict__.pop("_sampler_graphs", None)
        try:
            seqs[rows] = ColdSampler(model, DEV, predict="x0", algorithm=alg).sequence(
                4, generator=torch.Generator().manual_seed(2))
        finally:
            samplers.ROWS = True
            model.__dict__.pop("_sampler_graphs", None)
    assert len(seqs[True]) == len(seqs[False]) == 7
    worst = max((a - b).abs().max().item() for a, b in zip(seqs[True], seqs[False]))
    print(f"cold x0 algorithm {alg}: rows vs image layout, max |d| over all frames {worst:.5f}")
    assert worst < 2e-2, worst


@pytest.mark.gpu
def test_restore_mixed_levels(model):
    levels = [0, 1, 3, 6]
    g = torch.Generator().manual_seed(11)
    imgs = torch.rand(4, 3, 64, 64, generator=g) * 2.4 - 1.2  # beyond [-1, 1]: the clamp shows
    start = torch.cat([ref.pixelate(imgs[b:b + 1], 2 ** v) for b, v in enumerate(levels)])
    exp = _eager(model, start, levels, 2)[-1]
    model.__dict__.pop("_sampler_graphs", None)
    s = ColdSampler(model, DEV, predict="x0", algorithm=2)
    out = s.restore(imgs, levels, unit=False)
    assert torch.equal(out[0], imgs[0].clamp(-1, 1))  # level 0: skipped by every step
    d = (out[1:] - exp[1:]).abs() / 2  # on the [0, 1] image scale
    print(f"cold restore levels {levels}: vs eager mean |d| {d.mean():.5f} max |d| {d.max():.5f}")
    assert d.mean() < MEAN_BOUND and d.max() < MAX_BOUND, (d.mean(), d.max())
    assert (out[3] - start[3].clamp(-1, 1)).abs().mean() > 0.25  # the loop did something
    cache = model.__dict__["_sampler_graphs"]
    keys = lambda: [k for k in cache if k[0] == "cold_restore"]  # noqa: E731
    first = cache[keys()[0]].loop
    assert torch.equal(s.restore(imgs, levels, unit=False), out) and first.replays == 1
    # another level tuple: a graph of its own; the first one still replays to the same result
    other = s.restore(imgs, [6, 3, 1, 0], unit=False)
    assert len(keys()) == 2 and torch.equal(other[3], imgs[3].clamp(-1, 1))
    assert torch.equal(s.restore(imgs, levels, unit=False), out) and first.replays == 2
    assert torch.equal(s.restore(imgs, levels), (out + 1) / 2)
