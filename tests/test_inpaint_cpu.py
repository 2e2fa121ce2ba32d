"""Inpainting (mask-conditioned DDIM with RePaint resampling) on the CPU: the schedule's mask-step
coefficients against independent fp64 expressions, the exact probes of the reference mask step
(``ops.repaint_rows_`` / ``reference.repaint_rows``), the sampler on a tiny model against a
hand-written loop and its fixed points, the argument errors, the loop cache and ``--inpaint`` of
the ViT.py CLI."""
import math
import os
import subprocess
import sys

import pytest
import torch

from ddim_cold_amd import ops
from ddim_cold_amd.diffusion import samplers as smp
from ddim_cold_amd.diffusion import schedule as sch
from ddim_cold_amd.models.vit import DiffusionVisionTransformer
from ddim_cold_amd.ops import reference as ref

CPU = "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 2000
K = 500         # the tiny model's grid: t = 1999, 1499, 999, 499, the last jump onto a = 1


# ----------------------------------------------------------------------------- schedule
@pytest.mark.parametrize("k", [1, 10, 400])
def test_repaint_row_against_fp64_expressions(k):
    ts = sch.ddim_timesteps(T, k)
    for t in ts:
        a_t, a_p = 1.0 - math.sqrt((t + 1) / T) + 1e-5, 1.0 - math.sqrt((t + 1 - k) / T)
        for jump in (False, True):
            ka, kb, ra, rb = sch.repaint_row(T, t, k, jump)
            assert (ka, kb) == sch.ddim_coefficients(T, t, k)[2:]          # the very floats
            assert abs(ka - math.sqrt(a_p)) <= 1e-15 and abs(kb - math.sqrt(1 - a_p)) <= 1e-15
            if jump:
                assert abs(ra - math.sqrt(a_t / a_p)) <= 1e-15 and abs(rb - math.sqrt(1 - a_t / a_p)) <= 1e-15
                assert abs(ra * ra + rb * rb - 1.0) <= 1e-12
            else:
                assert (ra, rb) == (1.0, 0.0)
    if ts[-1] + 1 == k:     # the last jump lands on a = 1 (k = 1 ends at t = 1, one step short): known itself
        assert sch.repaint_row(T, ts[-1], k, False) == (1.0, 0.0, 1.0, 0.0)
        assert sch.repaint_row(T, ts[-1], k, True)[:2] == (1.0, 0.0)
    else:
        assert k == 1 and ts[-1] == 1


def test_repaint_row_errors():
    with pytest.raises(ValueError):
        sch.repaint_row(10 ** 6, 10 ** 6 - 1, 1, True)     # a_t (with its 1e-5) above a_(t-k)
    with pytest.raises(ValueError):
        sch.repaint_row(10 ** 6, 10 ** 6 - 1, 1, False)
    with pytest.raises(ValueError):
        sch.repaint_row(T, 100, 400, False)                # t + 1 - k < 0
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            sch.repaint_table(T, 400, bad)


def test_repaint_table():
    ts, rows = sch.repaint_table(T, 400, 3)
    assert ts == [t for t in sch.ddim_timesteps(T, 400) for _ in range(3)]
    assert rows.shape == (15, 4) and rows.dtype == torch.float32
    for n, t in enumerate(ts):
        want = torch.tensor(sch.repaint_row(T, t, 400, jump=n % 3 < 2), dtype=torch.float32)
        assert torch.equal(rows[n], want)
    assert rows[-1].tolist() == [1.0, 0.0, 1.0, 0.0]
    ts1, rows1 = sch.repaint_table(T, 400)
    assert ts1 == sch.ddim_timesteps(T, 400) and torch.equal(rows1[:, 2:], torch.tensor([[1.0, 0.0]] * 5))


def test_sites_are_disjoint_ranges():
    assert (ops.SITE_STEP_NOISE, ops.SITE_PASTE_NOISE, ops.SITE_JUMP_NOISE) == (4096, 8192, 12288)
    assert ops.SITE_LOOP_FORWARDS == 4096


# ----------------------------------------------------------------------------- the reference op
def _rng(seed=77):
    return torch.tensor([seed, 0], dtype=torch.int64)


def _randn(shape, site, seed=77):
    z = torch.empty(shape)
    ops.randn_(z, _rng(seed), site)
    return z


def _masks(shape, seed=0):
    n = shape[0] * shape[1]
    e = torch.arange(n)
    rnd = torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.5
    flat = {"zero": torch.zeros(n, dtype=torch.bool), "one": torch.ones(n, dtype=torch.bool), "alt": e % 2 == 1,
            "alt4": (e // 4) % 2 == 1, "random": rnd}
    return {k: v.to(torch.uint8).view(shape) for k, v in flat.items()}


@pytest.mark.parametrize("shape", [(1, 4), (15, 48)])
@pytest.mark.parametrize("mask_name", ["zero", "one", "alt", "alt4", "random"])
def test_reference_exact_probes(shape, mask_name):
    g = torch.Generator().manual_seed(1)
    x0 = torch.randn(shape, generator=g)
    known = torch.rand(shape, generator=g) * 2 - 1
    mask = _masks(shape)[mask_name]
    keep = mask != 0
    sp, sj = ops.SITE_PASTE_NOISE + 3, ops.SITE_JUMP_NOISE + 3
    z1, z2 = _randn(shape, sp), _randn(shape, sj)

    def run(coef, m=mask, with_rows=True):
        x = x0.clone()
        po = torch.full(shape, 7.0, dtype=torch.bfloat16) if with_rows else None
        ops.repaint_rows_(x, known, m, torch.tensor(coef, dtype=torch.float32), _rng(), sp, sj, po)
        return x, po

    x, po = run([1.0, 0.0, 1.0, 0.0])
    assert torch.equal(x[keep], known[keep]) and torch.equal(x[~keep], x0[~keep])
    wrote = keep.reshape(-1, 4).any(1, keepdim=True).expand(-1, 4).reshape(shape)
    assert torch.equal(po[wrote], x.to(torch.bfloat16)[wrote]) and bool((po[~wrote] == 7.0).all())
    x, _ = run([0.0, 1.0, 1.0, 0.0])
    assert torch.equal(x[keep], z1[keep]) and torch.equal(x[~keep], x0[~keep])
    ka = 0.8125 + 2.0 ** -20
    x, _ = run([ka, 0.0, 1.0, 0.0], with_rows=False)
    assert torch.equal(x[keep], (torch.tensor(ka, dtype=torch.float32) * known)[keep]) and torch.equal(x[~keep], x0[~keep])
    x, po = run([0.3, 0.4, 0.0, 1.0], m=torch.zeros_like(mask))
    assert torch.equal(x, z2) and torch.equal(po, z2.to(torch.bfloat16))      # a jump writes every element
    # the general case against fp64, two roundings per stage
    ka, kb, ra, rb = (float(v) for v in torch.tensor(sch.repaint_row(T, 999, K, True), dtype=torch.float32))
    x, _ = run([ka, kb, ra, rb])
    y = torch.where(keep, ka * known.double() + kb * z1.double(), x0.double())
    want = ra * y + rb * z2.double()
    bound = 4 * 2.0 ** -24 * (torch.where(keep, (ka * known).abs() + (kb * z1).abs(), torch.zeros(shape))
                              + (ra * y).abs().float() + (rb * z2).abs())
    assert bool(((x.double() - want).abs() <= bound).all())


def test_reference_op_argument_errors():
    x, known, mask = torch.zeros(2, 4), torch.zeros(2, 4), torch.zeros(2, 4, dtype=torch.uint8)
    coef = torch.tensor([1.0, 0.0, 1.0, 0.0])
    for bad in (dict(x=torch.zeros(1, 6), known=torch.zeros(1, 6), mask=torch.zeros(1, 6, dtype=torch.uint8)),
                dict(known=torch.zeros(2, 8)), dict(mask=torch.zeros(4, 2, dtype=torch.uint8)),
                dict(coef=torch.zeros(3)), dict(sp=-1), dict(sj=-1)):
        kw = dict(x=x.clone(), known=known, mask=mask, coef=coef, sp=1, sj=2)
        kw.update(bad)
        with pytest.raises(ValueError):
            ops.repaint_rows_(kw["x"], kw["known"], kw["mask"], kw["coef"], _rng(), kw["sp"], kw["sj"])


# ----------------------------------------------------------------------------- the sampler
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = DiffusionVisionTransformer(img_size=[16, 16], patch_size=4, embed_dim=64, depth=1, num_heads=2)
    with torch.no_grad():
        m.head.bias.uniform_(-0.5, 0.5)
    return m.eval()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _case(B=2, seed=3):
    g = _gen(seed)
    image = torch.rand(B, 3, 16, 16, generator=g) * 2 - 1
    noise = torch.randn(B, 3, 16, 16, generator=g)
    keep = torch.ones(16, 16, dtype=torch.bool)
    keep[4:11, 5:13] = False           # a hole that cuts through patches
    return image, noise, keep


def _hand_loop(model, image, keep, noise, k, eta, resample, seed):
    """The inpainting loop written out on images: forward n = forward_reference + ref.ddim_step_eta
    with the noise of site SITE_STEP_NOISE + n, then the paste ``ka known + kb z1`` where ``keep``
    and, on all runs of a grid step but the last, the jump ``ra x + rb z2`` (fp64, rounded once)."""
    B, C, H, W = noise.shape
    p = model.patch_size

    def z(site):
        v = torch.empty(B * (H // p) * (W // p), C * p * p)
        ops.randn_(v, torch.tensor([seed, 0], dtype=torch.int64), site)
        return ops.rows_to_image(v, B, C, H, W, p)

    def f32(v):
        return float(torch.tensor(v, dtype=torch.float32))
    x, n = noise.clone(), 0
    with torch.no_grad():
        for t in sch.ddim_timesteps(model.total_steps, k):
            for j in range(resample):
                raw = model.forward_reference(x, torch.full((B,), t))
                x, _ = ref.ddim_step_eta(x, raw, sch.eta_row(model.total_steps, t, k, eta), z(ops.SITE_STEP_NOISE + n))
                ka, kb, ra, rb = (f32(v) for v in sch.repaint_row(model.total_steps, t, k, j < resample - 1))
                y = torch.where(keep, ka * image.double() + kb * z(ops.SITE_PASTE_NOISE + n).double(), x.double())
                if j < resample - 1:
                    y = ra * y + rb * z(ops.SITE_JUMP_NOISE + n).double()
                x, n = y.float(), n + 1
    return (x + 1) / 2


@pytest.mark.parametrize("eta,resample", [(0.0, 1), (1.0, 1), (0.0, 2), (0.5, 3)])
def test_sampler_matches_hand_written_loop(model, eta, resample):
    image, noise, keep = _case()
    got = smp.inpaint(model, image, keep, k=K, eta=eta, resample=resample, device=CPU, noise=noise, noise_seed=4242)
    want = _hand_loop(model, image, keep, noise, K, eta, resample, 4242)
    d = (got - want).abs().max()
    print(f"eta={eta} resample={resample}: inpaint against the hand-written loop, max |d| {float(d):.3e}")
    # the same operations up to the fp32 roundings of the mask step and the association of the DDIM
    # update's last additions (a few ulp of |x| <= 8 per forward): the bound of
    # tests/test_ddim_eta_cpu.py::test_sampler_matches_hand_written_loop
    assert d <= 1e-5
    assert got.shape == image.shape and torch.isfinite(got).all()
    assert torch.equal(got[:, :, keep], ((image + 1) / 2)[:, :, keep])      # kept pixels: the image to the bit
    raw = smp.inpaint(model, image, keep, k=K, eta=eta, resample=resample, device=CPU, noise=noise, noise_seed=4242,
                      unit=False)
    assert torch.equal(raw[:, :, keep], image[:, :, keep]) and torch.equal((raw + 1) / 2, got)


def test_all_ones_mask_returns_the_image(model):
    image, noise, _ = _case()
    for eta, resample in ((0.0, 1), (1.0, 2)):
        out = smp.inpaint(model, image, torch.ones(16, 16), k=K, eta=eta, resample=resample, device=CPU, noise=noise,
                          unit=False)
        assert torch.equal(out, image)


@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_all_zero_mask_is_the_ddim_sampler(model, eta):
    image, noise, _ = _case()
    got = smp.inpaint(model, image, torch.zeros(16, 16, dtype=torch.bool), k=K, eta=eta, device=CPU, noise=noise,
                      noise_seed=99)
    want = smp.DDIMSampler(model, CPU, k=K, eta=eta).sample(2, noise=noise, noise_seed=99)
    assert torch.equal(got, want)


def test_resampling_and_seeds_change_the_result(model):
    image, noise, keep = _case()
    kw = dict(k=K, device=CPU, noise=noise)
    one = smp.inpaint(model, image, keep, resample=1, noise_seed=5, **kw)
    two = smp.inpaint(model, image, keep, resample=2, noise_seed=5, **kw)
    assert not torch.equal(one, two)
    assert torch.equal(one, smp.inpaint(model, image, keep, resample=1, noise_seed=5, **kw))
    assert not torch.equal(one, smp.inpaint(model, image, keep, resample=1, noise_seed=6, **kw))   # the paste noise
    # the seed is one draw from the generator after x_T, at eta = 0 too; noise_seed= overrides it
    g = _gen(8)
    a = smp.inpaint(model, image, keep, k=K, device=CPU, generator=g)
    g2 = _gen(8)
    x_T = torch.normal(0.0, 1.0, (2, 3, 16, 16), generator=g2)
    b = smp.inpaint(model, image, keep, k=K, device=CPU, noise=x_T, noise_seed=smp.draw_noise_seed(g2))
    assert torch.equal(a, b) and torch.equal(g.get_state(), g2.get_state())


def test_oracle_denoiser_fills_the_hole_with_its_picture(model, monkeypatch):
    image, noise, keep = _case()
    G = torch.randn(2, 3, 16, 16, generator=_gen(11))            # (some of it outside [-1, 1])
    monkeypatch.setattr(model, "forward_reference", lambda x, t: G.clone())
    for eta, resample in ((0.0, 1), (1.0, 2)):
        out = smp.inpaint(model, image, keep, k=K, eta=eta, resample=resample, device=CPU, noise=noise, unit=False)
        assert torch.equal(out[:, :, ~keep], torch.clamp(G, -1.0, 1.0)[:, :, ~keep])
        assert torch.equal(out[:, :, keep], image[:, :, keep])


def test_mask_forms_agree(model):
    image, noise, keep = _case()
    kw = dict(k=K, device=CPU, noise=noise, noise_seed=1)
    base = smp.inpaint(model, image, keep, **kw)
    forms = [keep.float(), keep.float() * 0.9 + 0.05, keep.to(torch.uint8), keep.view(1, 1, 16, 16).expand(2, 1, 16, 16),
             keep.view(1, 1, 16, 16).expand(2, 3, 16, 16).float(), keep.numpy()]
    for m in forms:
        assert torch.equal(smp.inpaint(model, image, m, **kw), base)
    one = smp.inpaint(model, image[0], keep, k=K, device=CPU, noise=noise[:1], noise_seed=1)   # [C, H, W]
    assert one.shape == (1, 3, 16, 16) and (one - base[:1]).abs().max() <= 1e-5
    per_channel = keep.view(1, 1, 16, 16).expand(2, 3, 16, 16).clone()
    per_channel[:, 0] = True                                       # channel 0 kept everywhere
    out = smp.inpaint(model, image, per_channel, unit=False, **kw)
    assert torch.equal(out[:, 0], image[:, 0]) and not torch.equal(out[:, 1], image[:, 1])


def test_errors(model):
    image, noise, keep = _case()
    for bad in (torch.ones(16), torch.ones(8, 8), torch.ones(1, 1, 16, 16), torch.ones(2, 2, 16, 16),
                torch.ones(2, 16, 16), torch.ones(3, 3, 16, 16)):
        with pytest.raises(ValueError, match=r"\[16, 16\], \[2, 1, 16, 16\] or \[2, 3, 16, 16\]"):
            smp.inpaint(model, image, bad, k=K, device=CPU)
    for bad in (0, -2, 1.5, True, "2"):
        with pytest.raises(ValueError, match="resample"):
            smp.inpaint(model, image, keep, k=K, resample=bad, device=CPU)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="eta"):
            smp.inpaint(model, image, keep, k=K, eta=bad, device=CPU)
    with pytest.raises(ValueError, match="image"):
        smp.inpaint(model, torch.zeros(2, 3, 8, 8), keep, k=K, device=CPU)
    with pytest.raises(ValueError):
        smp.inpaint(model, image, keep, k=300, device=CPU)            # not a grid of T
    with pytest.raises(ValueError, match="forwards"):                  # 1999 steps x 3 >= 4096 noise sites
        smp.inpaint(model, image, keep, k=1, resample=3, device=CPU)
    assert not any(c[0] == "inpaint" and c[2] == 1 for c in smp._cache(model))


def test_cache_limit_and_model_method(model):
    image, noise, keep = _case()
    model.__dict__.pop("_sampler_graphs", None)
    assert smp.INPAINT_GRAPHS == 8
    combos = [(eta, r) for eta in (0.0, 1.0) for r in (1, 2, 3, 4, 5)]
    for eta, r in combos:
        smp.inpaint(model, image, keep, k=1000, eta=eta, resample=r, device=CPU, noise=noise)
    keys = [c for c in smp._cache(model) if c[0] == "inpaint"]
    assert len(keys) == 8 and keys == [("inpaint", 2, 1000, eta, r, CPU) for eta, r in combos[2:]]
    st = smp._cache(model)[keys[-1]]
    smp.inpaint(model, -image, ~keep, k=1000, eta=1.0, resample=5, device=CPU, noise=noise)
    assert smp._cache(model)[keys[-1]] is st                       # a new image and mask: the same loop
    a = model.inpaint(image, keep, k=1000, resample=2, device=CPU, generator=_gen(1))
    b = smp.inpaint(model, image, keep, k=1000, resample=2, device=CPU, generator=_gen(1))
    assert torch.equal(a, b)
    model.__dict__.pop("_sampler_graphs", None)


# ----------------------------------------------------------------------------- CLI
def test_vit_cli_inpaint(tmp_path):
    from ddim_cold_amd import build_model
    from ddim_cold_amd.utils.images import save_image
    torch.manual_seed(3)
    ckpt = str(tmp_path / "weights.pkl")
    torch.save(build_model("vit_tiny").state_dict(), ckpt)
    picture = torch.rand(3, 64, 64, generator=_gen(2))
    hole = torch.ones(3, 64, 64)
    hole[:, 8:40, 20:60] = 0.0
    save_image(picture, str(tmp_path / "picture.png"))
    save_image(hole, str(tmp_path / "hole.png"))
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    base = [sys.executable, os.path.join(ROOT, "ViT.py"), "--model", "vit_tiny", "--ckpt", ckpt, "--acc_k", "1000"]
    runs = {}
    for name, extra in (("files", ["--inpaint", str(tmp_path / "picture.png"), "--mask", str(tmp_path / "hole.png"),
                                   "--resample", "2", "--eta", "0.5"]),
                        ("fallback", ["--inpaint", str(tmp_path / "none.png"), "--mask", str(tmp_path / "none_mask.png")])):
        out = tmp_path / name
        r = subprocess.run(base + extra + ["--out_dir", str(out)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        assert os.listdir(str(out)) == ["inpaint.png"]                 # no sample grids in this mode
        with open(str(out / "inpaint.png"), "rb") as f:
            runs[name] = (f.read(), r.stderr)
        assert len(runs[name][0]) > 1000
    assert "warning" not in runs["files"][1]
    assert "none.png not found" in runs["fallback"][1] and "none_mask.png not found" in runs["fallback"][1]
    assert runs["files"][0] != runs["fallback"][0]
    r = subprocess.run(base + ["--inpaint", "x.png", "--resample", "0", "--out_dir", str(tmp_path / "bad")],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode != 0 and "--resample" in r.stderr
