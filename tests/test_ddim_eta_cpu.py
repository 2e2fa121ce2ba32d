"""Stochastic DDIM (eta > 0) on the CPU: the schedule's coefficients against independent fp64
expressions, the checker of the head epilogue's stochastic step (ops/eta_check.py) on the
reference, on the fp32 emulation of the kernel and on its mutants, the statistics of the
per-step noise, the samplers on a tiny model, and ``--eta`` of both CLIs."""
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
from ddim_cold_amd.ops import eta_check as tc
from ddim_cold_amd.ops import reference as ref

CPU = "cpu"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 2000
KS = (1, 2, 10, 20, 400, 500, 1000, 2000)


def _abars(t, k):
    return 1.0 - math.sqrt((t + 1) / T) + 1e-5, 1.0 - math.sqrt((t + 1 - k) / T)


def _grids():
    """Every (t, k) of the sampling grids for k in KS and of the img2img grids from 1599 and 1999 (k = 10)."""
    out = [(t, k) for k in KS for t in sch.ddim_timesteps(T, k)]
    return out + [(t, 10) for s in (1599, 1999) for t in sch.ddim_timesteps(T, 10, s)]


# ----------------------------------------------------------------------------- coefficients
@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_coefficients_against_fp64_expression(eta):
    for t, k in _grids():
        a_t, a_p = _abars(t, k)
        sigma = eta * math.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))
        want = (math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_p), math.sqrt(1 - a_p - sigma ** 2), sigma)
        got = sch.ddim_coefficients_eta(T, t, k, eta)
        assert len(got) == 5
        for g, w in zip(got, want):
            assert abs(g - w) <= 1e-15 * max(1.0, abs(w)), (t, k, got, want)
        mirror = ref.ddim_coeffs_eta(T, t, k, eta)
        assert all(abs(g - m) <= 1e-15 for g, m in zip(got, mirror))


def test_eta_zero_rows_are_the_deterministic_floats():
    for t, k in _grids():
        got = sch.ddim_coefficients_eta(T, t, k, 0.0)
        assert got[:4] == sch.ddim_coefficients(T, t, k) and got[4] == 0.0 and math.copysign(1.0, got[4]) == 1.0
    ts, coef8 = sch.ddim_table_eta(T, 20, 0.0)
    ts4, coef4 = sch.ddim_table(T, 20)
    assert ts == ts4 and coef8.shape == (100, 8) and coef8.dtype == torch.float32
    assert torch.equal(coef8[:, :4], coef4) and int(torch.count_nonzero(coef8[:, 4:])) == 0


@pytest.mark.parametrize("k", [2, 20, 400])
def test_last_step_has_no_noise_and_no_direction(k):
    t = sch.ddim_timesteps(T, k)[-1]
    assert t + 1 == k
    for eta in (0.3, 1.0):
        c = sch.ddim_coefficients_eta(T, t, k, eta)
        assert c[2] == 1.0 and c[3] == 0.0 and c[4] == 0.0


def test_radicands_are_non_negative_at_eta_one():
    for t, k in _grids():
        a_t, a_p = _abars(t, k)
        rad = (1 - a_p) / (1 - a_t) * (1 - a_t / a_p)
        assert rad >= 0.0 and 1 - a_p - rad >= 0.0, (t, k)
        sch.ddim_coefficients_eta(T, t, k, 1.0)  # (raises on a negative radicand)


@pytest.mark.parametrize("eta", [-0.1, 1.0001, 2, float("nan"), float("inf")])
def test_eta_outside_unit_interval_raises(eta):
    with pytest.raises(ValueError):
        sch.ddim_coefficients_eta(T, 1999, 20, eta)
    with pytest.raises(ValueError):
        sch.ddim_table_eta(T, 20, eta)
    with pytest.raises(ValueError):
        ref.ddim_coeffs_eta(T, 1999, 20, eta)


def test_ddpm_posterior_identity_at_eta_one():
    """At eta = 1 the step is the DDPM posterior mean: the coefficient of x_t is sqrt(a_t / a_p)
    (1 - a_p) / (1 - a_t), that of x0 sqrt(a_p) (1 - a_t / a_p) / (1 - a_t)."""
    worst = 0.0
    for k in (1, 10, 20, 400):
        for t in sch.ddim_timesteps(T, k):
            a_t, a_p = _abars(t, k)
            c0, c1, c2, cd, _ = sch.ddim_coefficients_eta(T, t, k, 1.0)
            worst = max(worst, abs(cd / c1 - math.sqrt(a_t / a_p) * (1 - a_p) / (1 - a_t)),
                        abs(c2 - cd * c0 / c1 - math.sqrt(a_p) * (1 - a_t / a_p) / (1 - a_t)))
    print(f"DDPM posterior identity: worst deviation {worst:.3e}")
    assert worst <= 1e-12


def test_tables_have_rows_of_eight():
    ts, coef = sch.ddim_table_eta(T, 400, 1.0)
    assert coef.shape == (5, 8) and int(torch.count_nonzero(coef[:, 5:])) == 0
    assert coef[0].tolist() == [float(torch.tensor(v, dtype=torch.float32)) for v in sch.eta_row(T, 1999, 400, 1.0)]
    ts, rows = smp.starts_table_eta(T, [1199, 1599, 1999], 400, 1.0)
    assert ts == [1999, 1599, 1199, 799, 399] and rows.shape == (5, 3, 8)
    ident = torch.tensor(sch.ETA_IDENT_ROW)
    assert sch.ETA_IDENT_ROW == (0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
    assert torch.equal(rows[0, 0], ident) and torch.equal(rows[0, 1], ident) and torch.equal(rows[1, 0], ident)
    assert torch.equal(rows[0, 2], coef[0]) and torch.equal(rows[2, 0], coef[2]) and float(rows[4, 1, 4]) == 0.0
    assert torch.equal(smp.starts_table_eta(T, [1199, 1999], 400, 0.0)[1][..., :4], smp.starts_table(T, [1199, 1999], 400)[1])


# ----------------------------------------------------------------------------- the checker
@pytest.mark.parametrize("geom", tc.GEOMS)
def test_checker_passes_reference_and_emulation(geom):
    assert tc.run_all(CPU, geom) <= 1.0
    assert tc.run_all(CPU, geom, tc.ddim_eta_f32) <= 1.0


@pytest.mark.parametrize("mutant", tc.MUTANTS)
@pytest.mark.parametrize("geom", tc.GEOMS)
def test_checker_rejects_mutants(geom, mutant):
    with pytest.raises(AssertionError):
        tc.run_all(CPU, geom, tc.mutant_step(mutant))


def test_mutants_fail_where_they_should():
    """The noise mutants fall to the probe, the arithmetic mutants pass it and fall to the bounds."""
    geom = tc.GEOMS[3]
    for m in ("swap_halves", "column_noise", "same_site"):
        with pytest.raises(AssertionError, match="noise probe"):
            tc.run_noise_probe(CPU, geom, tc.mutant_step(m))
    for m in ("sigma_squared", "dir_deterministic", "neighbour_sigma"):
        tc.run_noise_probe(CPU, geom, tc.mutant_step(m))
        tc.run_exact(CPU, geom, tc.mutant_step(m))
        with pytest.raises(AssertionError, match="x_next"):
            tc.run_eta(CPU, geom, tc.mutant_step(m))


def test_head_step_rows_noise_argument_is_checked():
    c = tc.ddim_case(tc.GEOMS[0])
    x_t, _ = tc.case_rows(c)
    with pytest.raises(ValueError):   # mode 5 without noise
        ops.head_step_rows_(c.a, c.w, c.bias, x_t.clone(), torch.empty_like(x_t), torch.tensor(tc.PROBE_ROW), 2, 5)
    with pytest.raises(ValueError):   # mode 1 with noise
        ops.head_step_rows_(c.a, c.w, c.bias, x_t.clone(), torch.empty_like(x_t), torch.tensor(tc.PROBE_ROW[:4]), 2, 1,
                            noise=(tc.rng_of(CPU), 0))
    with pytest.raises(ValueError):   # mode 6 with one row
        ops.head_step_rows_(c.a, c.w, c.bias, x_t.clone(), torch.empty_like(x_t), torch.tensor(tc.PROBE_ROW), 2, 6,
                            noise=(tc.rng_of(CPU), 0))


# ----------------------------------------------------------------------------- noise statistics
def _draw(n, seed, site):
    z = torch.empty(n)
    ops.randn_(z, torch.tensor([seed, 0], dtype=torch.int64), site)
    return z.double()


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / (a.norm() * b.norm()))


@pytest.mark.parametrize("seed", [1234, 7])
@pytest.mark.parametrize("n", [1728, 3840, 5184])
def test_step_noise_statistics(n, seed):
    assert ops.SITE_STEP_NOISE >= 1024
    zs = [_draw(n, seed, ops.SITE_STEP_NOISE + i) for i in range(6)]
    cap = 5.0 / math.sqrt(n)
    z_mean = max(abs(float(z.mean())) for z in zs) * math.sqrt(n)
    z_std = max(abs(float(z.std()) - 1.0) for z in zs) * math.sqrt(2 * n)
    z_site = max(abs(_corr(zs[i], zs[j])) for i in range(6) for j in range(i)) * math.sqrt(n)
    z_seed = abs(_corr(zs[0], _draw(n, seed + 1, ops.SITE_STEP_NOISE))) * math.sqrt(n)
    print(f"n={n} seed={seed}: z-scores mean {z_mean:.2f} std {z_std:.2f} cross-site {z_site:.2f} seed+1 {z_seed:.2f}")
    assert z_mean < 5 and z_std < 5 and z_site < 5 and z_seed < 5, cap


# ----------------------------------------------------------------------------- samplers
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = DiffusionVisionTransformer(img_size=[16, 16], patch_size=4, embed_dim=64, depth=2, num_heads=2)
    with torch.no_grad():
        m.head.bias.uniform_(-0.5, 0.5)
    return m.eval()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _hand_loop(model, noise, k, eta, seed):
    """x_T -> x0-hat of the last step by ref.ddim_step_eta, the noise of step i from ops.randn_
    over the patch-row state at rng = [seed, 0], site SITE_STEP_NOISE + i."""
    N, C, H, W = noise.shape
    p = model.patch_size
    x = noise.clone()
    rng = torch.tensor([seed, 0], dtype=torch.int64)
    with torch.no_grad():
        for i, t in enumerate(sch.ddim_timesteps(model.total_steps, k)):
            raw = model.forward_reference(x, torch.full((N,), t))
            z = torch.empty(N * (H // p) * (W // p), C * p * p)
            ops.randn_(z, rng, ops.SITE_STEP_NOISE + i)
            x, x0 = ref.ddim_step_eta(x, raw, sch.eta_row(model.total_steps, t, k, eta),
                                      ops.rows_to_image(z, N, C, H, W, p))
    return (x0 + 1) / 2


def test_eta_zero_is_the_present_sampler(model):
    g0, g1 = _gen(5), _gen(5)
    old = smp.DDIMSampler(model, CPU, k=400).sample(3, generator=g0)
    new = smp.DDIMSampler(model, CPU, k=400, eta=0.0).sample(3, generator=g1)
    assert torch.equal(old, new)
    assert torch.equal(g0.get_state(), g1.get_state())      # nothing extra drawn
    assert not any(k[0] == "ddim_eta" for k in smp._cache(model))
    a = smp.DDIMSampler(model, CPU, k=400).sequence(2, generator=_gen(6))
    b = smp.DDIMSampler(model, CPU, k=400, eta=0.0).sequence(2, generator=_gen(6))
    assert len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))
    with pytest.raises(ValueError):
        smp.DDIMSampler(model, CPU, k=400, eta=1.5)


def test_eta_one_reproduces_under_the_generator(model):
    s = smp.DDIMSampler(model, CPU, k=400, eta=1.0)
    a, b, c = s.sample(3, generator=_gen(5)), s.sample(3, generator=_gen(5)), s.sample(3, generator=_gen(6))
    assert torch.equal(a, b) and not torch.equal(a, c)
    det = smp.DDIMSampler(model, CPU, k=400).sample(3, generator=_gen(5))
    assert not torch.equal(a, det) and torch.isfinite(a).all() and a.min() >= 0 and a.max() <= 1
    # the same x_T, another noise seed
    noise = torch.randn(3, 3, 16, 16, generator=_gen(1))
    assert not torch.equal(s.sample(3, noise=noise, noise_seed=1), s.sample(3, noise=noise, noise_seed=2))
    assert any(k[0] == "ddim_eta" and k[-1] == 1.0 for k in smp._cache(model))


def test_noise_seed_overrides_the_generator(model):
    s = smp.DDIMSampler(model, CPU, k=400, eta=1.0)
    noise = torch.randn(2, 3, 16, 16, generator=_gen(2))
    a = s.sample(2, noise=noise, generator=_gen(8), noise_seed=99)
    b = s.sample(2, noise=noise, generator=_gen(9), noise_seed=99)
    assert torch.equal(a, b)
    g = _gen(8)
    drawn = smp.draw_noise_seed(_gen(8))
    assert torch.equal(s.sample(2, noise=noise, generator=g), s.sample(2, noise=noise, noise_seed=drawn))


@pytest.mark.parametrize("eta", [0.3, 1.0])
def test_sampler_matches_hand_written_loop(model, eta):
    noise = torch.randn(3, 3, 16, 16, generator=_gen(3))
    s = smp.DDIMSampler(model, CPU, k=400, eta=eta)
    got = s.sample(3, noise=noise, noise_seed=4242)
    want = _hand_loop(model, noise, 400, eta, 4242)
    d = (got - want).abs().max()
    print(f"eta={eta}: sampler against the hand-written loop, max |d| {float(d):.3e}")
    assert d <= 1e-5    # the same fp32 operations up to the association of the last two additions
    seq = s.sequence(3, noise=noise, noise_seed=4242)
    assert len(seq) == 6 and torch.equal(seq[-1], got)
    # sample b's noise does not depend on the batch size
    one = s.sample(1, noise=noise[:1], noise_seed=4242)
    assert (one - got[:1]).abs().max() <= 1e-5


def test_img2img_leaves_a_sample_alone_until_its_start(model, monkeypatch):
    starts, k = [1999, 999, 1999], 1000
    x = torch.randn(3, 3, 16, 16, generator=_gen(4))
    seen = []
    orig = smp._StepNoise.add_

    def spy(self, xs, i, sigma):
        orig(self, xs, i, sigma)
        seen.append(xs.clone())
    monkeypatch.setattr(smp._StepNoise, "add_", spy)
    out = smp.ddim_from_starts(model, x, starts, k, CPU, eta=1.0, noise_seed=11)
    assert len(seen) == 2
    assert torch.equal(seen[0][1], x[1])                      # not started: exactly x_t, no noise
    assert not torch.equal(seen[0][0], x[0]) and not torch.equal(seen[1][1], x[1])
    again = smp.ddim_from_starts(model, x, starts, k, CPU, eta=1.0, noise_seed=11)
    other = smp.ddim_from_starts(model, x, starts, k, CPU, eta=1.0, noise_seed=12)
    assert torch.equal(out, again) and not torch.equal(out, other)
    assert torch.equal(smp.ddim_from_starts(model, x, starts, k, CPU, eta=0.0), smp.ddim_from_starts(model, x, starts, k, CPU))
    # img2img draws the seed from its generator, after the start noise
    draft = torch.rand(3, 16, 16, generator=_gen(5)) * 2 - 1
    a = smp.img2img(model, draft, starts, k, CPU, generator=_gen(6), eta=1.0)
    b = smp.img2img(model, draft, starts, k, CPU, generator=_gen(6), eta=1.0)
    c = smp.img2img(model, draft, starts, k, CPU, generator=_gen(6))
    assert torch.equal(a, b) and not torch.equal(a, c) and a.shape == (3, 3, 16, 16)


def test_model_api_takes_eta(model):
    a = model.sampler(CPU, k=400, N=2, generator=_gen(1), eta=1.0)
    b = model.sampler(CPU, k=400, N=2, generator=_gen(1))
    assert a.shape == b.shape and not torch.equal(a, b)
    s1 = model.diffusion_sequence(CPU, k=400, N=2, generator=_gen(1), eta=1.0)
    s0 = model.diffusion_sequence(CPU, k=400, N=2, generator=_gen(1))
    assert len(s1) == len(s0) == 6 and torch.equal(s1[0], s0[0]) and not torch.equal(s1[-1], s0[-1])


# ----------------------------------------------------------------------------- CLIs
@pytest.fixture(scope="module")
def ckpt(tmp_path_factory):
    """A ViT-tiny state_dict file: both CLIs sample the same (random) weights in every run."""
    from ddim_cold_amd import build_model
    torch.manual_seed(3)
    path = str(tmp_path_factory.mktemp("eta_ckpt") / "weights.pkl")
    torch.save(build_model("vit_tiny").state_dict(), path)
    return path


def _cli(script, args, out, ckpt):
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args + ["--out_dir", str(out), "--ckpt", ckpt],
                          capture_output=True, text=True, env=env, timeout=600)


def _png(d, name):
    with open(os.path.join(str(d), name), "rb") as f:
        return f.read()


def test_vit_cli_eta(tmp_path, ckpt):
    base = ["--model", "vit_tiny", "--sample_n", "1", "--acc_k", "1000", "--seq_n", "1", "--seq_k", "1000"]
    runs = {}
    for name, extra in (("default", []), ("zero", ["--eta", "0"]), ("half", ["--eta", "0.5"])):
        r = _cli("ViT.py", base + extra, tmp_path / name, ckpt)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (_png(tmp_path / name, "samples.png"), _png(tmp_path / name, "denoise_sequence.png"))
    assert runs["default"] == runs["zero"]
    assert runs["half"][0] != runs["default"][0] and runs["half"][1] != runs["default"][1]
    r = _cli("ViT.py", base + ["--eta", "1.5"], tmp_path / "bad", ckpt)
    assert r.returncode != 0 and "--eta" in r.stderr


def test_draft2drawing_cli_eta(tmp_path, ckpt):
    runs = {}
    for name, extra in (("default", []), ("zero", ["--eta", "0.0"]), ("one", ["--eta", "1"])):
        r = _cli("ViT_draft2drawing.py", ["--k", "50"] + extra, tmp_path / name, ckpt)
        assert r.returncode == 0, r.stderr[-2000:]
        runs[name] = (_png(tmp_path / name, "draft2img.png"), _png(tmp_path / name, "denoise_sequence.png"))
    assert runs["default"] == runs["zero"]
    assert runs["one"][0] != runs["default"][0] and runs["one"][1] == runs["default"][1]   # img2img only
    r = _cli("ViT_draft2drawing.py", ["--eta", "-0.5"], tmp_path / "bad", ckpt)
    assert r.returncode != 0 and "--eta" in r.stderr
