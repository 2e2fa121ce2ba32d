"""DPM-Solver++(2M) on the CPU: the coefficient tables (``schedule.dpm2m_row`` / ``dpm2m_table``,
``samplers.starts_table_dpm``), the step ``ops.dpm2m_rows_`` (``reference.dpm2m_rows``) against
an independent fp64 formula and exact probes, its order of convergence on a problem with a
closed-form solution, the samplers against a plain loop, refusals, cache keys and the CLI.

The step is ``x_next = c2 x0 + c3 (x - c0 x0) / c1 + g (x0 - x0_prev)``.  With u = 2^-24 (a
correctly rounded fp32 operation is off by at most u relative) and ``A = |c2 x0| + |c3 / c1| (|x|
+ |c0 x0|)``: the fma ``x - c0 x0``, the division and the product with c3 are three roundings of
a quantity within ``|c3 / c1| (|x| + |c0 x0|)``, the fma with ``c2 x0`` one more on at most A, so
the DDIM part is within 4 u A (to first order); the subtraction ``x0 - x0_prev`` and the last fma
add ``u |g| (|x0| + |x0_prev|)`` and ``u (A + |g| (|x0| + |x0_prev|))``.  In all ``5 u A + 2 u |g|
(|x0| + |x0_prev|)``; the tests allow ``8 u A + 4 u |g| (|x0| + |x0_prev|)``, the 8 being what
``ops/epi_check.py`` allows the DDIM update of the head epilogue."""
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")
T = 2000
U = 2.0 ** -24
NAN = float("nan")


def _f32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ----------------------------------------------------------------------------- tables
@pytest.mark.parametrize("k", [20, 50, 100, 500])
def test_table_columns_and_zero_g(k):
    ts, tab = sch.dpm2m_table(T, k)
    ts4, tab4 = sch.ddim_table(T, k)
    assert ts == ts4 and tab.shape == (len(ts), 8) and tab.dtype == torch.float32
    assert torch.equal(tab[:, :4].view(torch.int32), tab4.view(torch.int32))       # DDIM's floats to the bit
    assert bool((tab[:, 5:] == 0).all())
    assert float(tab[0, 4]) == 0.0                                                 # no history yet
    assert T % k == 0 and float(tab[-1, 3]) == 0.0 and float(tab[-1, 4]) == 0.0    # onto a = 1: first order
    assert bool((tab[1:-1, 4] != 0).all())


def test_middle_row_is_the_formula():
    k = 100
    ts, tab = sch.dpm2m_table(T, k)
    for i in (1, 7, len(ts) - 2):
        c0, c1, c2, c3 = sch.ddim_coefficients(T, ts[i], k)
        p0, p1, p2, p3 = sch.ddim_coefficients(T, ts[i - 1], k)
        h = math.log(c2 / c3) - math.log(c0 / c1)
        h_prev = math.log(p2 / p3) - math.log(p0 / p1)
        g = (c2 - c3 * c0 / c1) * h / (2 * h_prev)
        assert h > 0 and h_prev > 0 and g > 0
        assert float(tab[i, 4]) == _f32(g)
        assert sch.dpm2m_row(T, ts[i], k, h_prev) == (c0, c1, c2, c3, g, 0.0, 0.0, 0.0)
        # the same g from the solver's own quantities: -alpha_next (e^-h - 1) / (2 r), r = h_prev / h
        assert g == pytest.approx(-c2 * math.expm1(-h) * h / (2 * h_prev), rel=1e-12)
    assert sch.dpm2m_row(T, ts[3], k, None)[4] == 0.0
    assert sch.dpm2m_row(T, ts[-1], k, 0.3)[4] == 0.0


def test_table_from_a_start():
    ts, tab = sch.dpm2m_table(T, 500, start=1499)
    assert ts == [1499, 999, 499] and float(tab[0, 4]) == 0.0 and float(tab[1, 4]) != 0.0


def test_per_sample_table():
    starts, k = [1499, 499, 999], 500
    ts, tab = smp.starts_table_dpm(T, starts, k)
    assert ts == [1499, 999, 499] and tab.shape == (3, 3, 8) and tab.dtype == torch.float32
    ident = torch.tensor(sch.ETA_IDENT_ROW)
    assert torch.equal(tab[0, 1], ident) and torch.equal(tab[1, 1], ident) and torch.equal(tab[0, 2], ident)
    for b, s in enumerate(starts):
        own = sch.dpm2m_table(T, k, start=s)[1]                    # the sample's own grid, from its own start
        first = ts.index(s)
        assert torch.equal(tab[first:, b].view(torch.int32), own.view(torch.int32))
        assert float(tab[first, b, 4]) == 0.0                      # the step it starts at: no history
    assert float(tab[1, 0, 4]) != 0.0
    with pytest.raises(ValueError):
        smp.starts_table_dpm(T, [1499, 1000], k)


# ----------------------------------------------------------------------------- the op
def _operands(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * 1.5
    x0 = torch.rand(shape, generator=g) * 2 - 1
    x0p = torch.rand(shape, generator=g) * 2 - 1
    return x, x0, x0p


def _truth(x, x0, x0p, rows, batch):
    """fp64 value and the bound of the module docstring; ``rows`` [1 or batch, 8] fp32."""
    cf = rows.double().reshape(-1, 8)
    xs, p, pp = (v.double().reshape(cf.shape[0], -1) for v in (x, x0, x0p))
    c0, c1, c2, c3, g = (cf[:, i:i + 1] for i in range(5))
    want = c2 * p + c3 * (xs - c0 * p) / c1 + g * (p - pp)
    a = (c2 * p).abs() + (c3 / c1).abs() * (xs.abs() + (c0 * p).abs())
    bound = 8 * U * a + 4 * U * g.abs() * (p.abs() + pp.abs())
    return want.reshape(x.shape), bound.reshape(x.shape)


@pytest.mark.parametrize("each", [False, True])
def test_op_against_fp64_formula(each):
    shape, batch = (12, 192), 3
    x, x0, x0p = _operands(shape, 5)
    tab = sch.dpm2m_table(T, 100)[1]
    rows = tab[[3, 9, 17]] if each else tab[9:10]
    assert bool((rows[:, 4] != 0).all())
    want, bound = _truth(x, x0, x0p, rows, batch)
    out = x.clone()
    po = torch.zeros(shape, dtype=torch.bfloat16)
    ops.dpm2m_rows_(out, x0, x0p, rows.reshape(-1) if not each else rows, batch, each, patches_out=po)
    err = (out.double() - want).abs()
    print(f"each={each}: worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(po.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
    assert torch.equal(out, ref.dpm2m_rows(x, x0, x0p, rows, batch, each))
    with pytest.raises(ValueError):
        ref.dpm2m_rows(x, x0, x0p[:6], rows, batch, each)
    with pytest.raises(ValueError):
        ref.dpm2m_rows(x, x0, x0p, tab[:2], batch, each)
    with pytest.raises(ValueError):
        ref.dpm2m_rows(x[:1, :6], x0[:1, :6], x0p[:1, :6], rows, batch, each)


def exact_case(n_per, batch):
    """Operands of the exact probe: small integers, distinct per element in each of x / x0 /
    x0_prev's own pattern, and one power-of-two row per sample.  Every product, quotient and sum
    of the step is then a dyadic rational below 2^12 with at most 4 fractional bits: exact in
    fp32 in any order, fused or not.  Returns (x, x0, x0_prev, rows [batch, 8])."""
    e = torch.arange(batch * n_per)
    x = ((e * 7) % 13 - 6).float().view(batch, n_per)
    x0 = ((e * 3) % 5 - 2).float().view(batch, n_per)
    x0p = ((e * 5) % 7 - 3).float().view(batch, n_per)
    rows = torch.tensor([[0.5, 2.0, 4.0, 8.0, 16.0, 0, 0, 0], [2.0, 0.5, 8.0, 16.0, 4.0, 0, 0, 0],
                         [4.0, 8.0, 16.0, 0.5, 2.0, 0, 0, 0]])[:batch]
    return x, x0, x0p, rows


def exact_want(x, x0, x0p, rows):
    c0, c1, c2, c3, g = (rows.double()[:, i:i + 1] for i in range(5))
    x, x0, x0p = x.double(), x0.double(), x0p.double()
    return (c2 * x0 + c3 * (x - c0 * x0) / c1 + g * (x0 - x0p)).float()


def check_exact_probe(dev):
    x, x0, x0p, rows = (v.to(dev) for v in exact_case(64, 3))
    want = exact_want(x, x0, x0p, rows)
    out = x.clone()
    ops.dpm2m_rows_(out, x0, x0p, rows, 3, True)
    assert torch.equal(out, want)
    for b in range(3):                                             # each = 0 with every row in turn
        one = x[b:b + 1].clone()
        ops.dpm2m_rows_(one, x0[b:b + 1], x0p[b:b + 1], rows[b], 1, False)
        assert torch.equal(one, want[b:b + 1])
    # what the probe can tell apart: a neighbour's row, and x0 / x0_prev the other way round
    for wrong in (exact_want(x, x0, x0p, rows.roll(1, 0)), exact_want(x, x0, x0p, rows.roll(-1, 0)),
                  exact_want(x, x0p, x0, rows)):
        assert all(not torch.equal(wrong[b], want[b]) for b in range(3))


def test_exact_probe():
    check_exact_probe(CPU)


@pytest.mark.parametrize("each", [False, True])
def test_zero_g_does_not_read_x0_prev(each):
    """With g = 0 the step is DDIM and x0_prev (all NaN here) reaches nothing.  Against
    ``reference.ddim_step`` on pre-clamped input: that one rounds ``c0 x0``, the difference, the
    quotient, the product with c3, ``c2 x0`` and the sum (6 roundings, each within u A), the op 4
    (module docstring): they differ by at most 10 u A to first order; 12 u A allowed."""
    shape, batch = (12, 192), 3
    x, x0, _ = _operands(shape, 6)
    nan = torch.full(shape, NAN)
    tab = sch.dpm2m_table(T, 100)[1].clone()
    tab[:, 4] = 0.0
    rows = tab[[3, 9, 17]] if each else tab[9:10]
    out = x.clone()
    po = torch.zeros(shape, dtype=torch.bfloat16)
    ops.dpm2m_rows_(out, x0, nan, rows, batch, each, patches_out=po)
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(po.float()).all())
    other = x.clone()
    ops.dpm2m_rows_(other, x0, torch.zeros(shape), rows, batch, each)
    assert torch.equal(out, other)
    for b in range(batch):
        r = rows[b if each else 0]
        sl = slice(b * 4, b * 4 + 4)
        want, clamped = ref.ddim_step(x[sl], x0[sl], [float(v) for v in r[:4]])
        assert torch.equal(clamped, x0[sl])
        c0, c1, c2, c3 = (float(v) for v in r[:4])
        a = (c2 * x0[sl]).abs() + abs(c3 / c1) * (x[sl].abs() + (c0 * x0[sl]).abs())
        assert bool(((out[sl] - want).abs() <= 12 * U * a).all())


def test_identity_row_returns_x_to_the_bit():
    shape = (12, 192)
    x, x0, _ = _operands(shape, 7)
    rows = torch.tensor([sch.ETA_IDENT_ROW] * 3)
    for each in (False, True):
        out = x.clone()
        ops.dpm2m_rows_(out, x0, torch.full(shape, NAN), rows if each else rows[0], 3, each)
        assert torch.equal(out.view(torch.int32), x.view(torch.int32))


# ----------------------------------------------------------------------------- convergence
def _analytic_error(k, mu, s, second_order):
    """Max error of the returned x0-hat on the problem x0 ~ N(mu, s^2) per element, whose optimal
    denoiser at level (alpha, sigma) is ``mu + alpha s^2 / (alpha^2 s^2 + sigma^2) (x - alpha mu)``
    and whose probability-flow solution from ``alpha mu + sqrt(alpha^2 s^2 + sigma^2) xi`` keeps
    that form with the same xi at every level.  Also returns max |x0-hat| along the run."""
    ts, tab = sch.dpm2m_table(T, k)
    if not second_order:
        tab = tab.clone()
        tab[:, 4] = 0.0
    xi = torch.linspace(-2.5, 2.5, 101).view(101, 1).expand(101, 4).contiguous()

    def denoise(x, a, sg):
        return mu + a * s * s / (a * a * s * s + sg * sg) * (x - a * mu)

    def level(i):
        return float(tab[i, 0]), float(tab[i, 1])
    a, sg = level(0)
    x = a * mu + math.sqrt(a * a * s * s + sg * sg) * xi
    x0, x0p = torch.zeros_like(x), torch.full_like(x, NAN)         # (the first row has g = 0)
    peak = 0.0
    for i in range(len(ts)):
        x0.copy_(denoise(x, *level(i)))
        peak = max(peak, float(x0.abs().max()))
        ops.dpm2m_rows_(x, x0, x0p, tab[i], 1, False)
        x0, x0p = x0p, x0
    a, sg = level(len(ts) - 1)
    exact = denoise(a * mu + math.sqrt(a * a * s * s + sg * sg) * xi.double(), a, sg)
    return float((x0p.double() - exact).abs().max()), peak


@pytest.mark.parametrize("mu,s", [(0.2, 0.3), (-0.1, 0.35), (0.0, 0.2)])
def test_second_order_on_the_analytic_problem(mu, s):
    err = {(k, so): _analytic_error(k, mu, s, so) for k, so in ((100, False), (100, True), (50, False), (50, True),
                                                                  (20, False))}
    print(f"mu={mu} s={s}: " + ", ".join(f"k={k} {'2M' if so else 'ddim'} {e:.2e}" for (k, so), (e, _) in err.items()))
    assert max(p for _, p in err.values()) < 1.0                   # the clamp never engages: the closed form holds
    assert err[100, False][0] / err[100, True][0] >= 3
    assert err[50, False][0] / err[50, True][0] >= 6
    assert err[100, True][0] < err[20, False][0]


# ----------------------------------------------------------------------------- the sampler
N = 2


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = DiffusionVisionTransformer(img_size=[16, 16], patch_size=8, embed_dim=64, depth=1, num_heads=2)
    with torch.no_grad():
        m.head.bias.uniform_(-0.5, 0.5)
    return m.eval()


@pytest.fixture(scope="module")
def noise():
    return torch.randn(N, 3, 16, 16, generator=torch.Generator().manual_seed(11))


def plain_loop(model, noise, k, second_order, dev=CPU):
    """The sampler written out in fp32 torch on images: ``forward_reference``, clamp, the formula
    with the floats of ``dpm2m_table``.  Returns the last x0-hat in [0, 1] on the host."""
    ts, tab = sch.dpm2m_table(model.total_steps, k)
    x = noise.to(dev).clone()
    x0p = None
    with torch.no_grad():
        for i, t in enumerate(ts):
            c0, c1, c2, c3, g = (float(v) for v in tab[i, :5])
            x0 = torch.clamp(model.forward_reference(x, torch.full((x.shape[0],), t, device=dev)), -1.0, 1.0)
            nxt = c2 * x0 + c3 * (x - c0 * x0) / c1
            if second_order and g != 0.0:
                nxt = nxt + g * (x0 - x0p)
            x, x0p = nxt, x0
    return ((x0p + 1) / 2).cpu()


def test_sampler_matches_the_plain_loop(model, noise):
    """Measured here: max deviation 1.2e-7 for solver="ddim" and 1.2e-7 for "dpmpp2m" (the bound
    being 4 x the former: the second-order term adds at most 2 |g| times the rounding of x0-hat)."""
    k = model.total_steps // 4
    dev = {}
    for solver in ("ddim", "dpmpp2m"):
        out = smp.DDIMSampler(model, CPU, k=k, solver=solver).sample(N, noise=noise)
        dev[solver] = float((out - plain_loop(model, noise, k, solver == "dpmpp2m")).abs().max())
    print(f"sampler against the plain loop: ddim {dev['ddim']:.3e}, dpmpp2m {dev['dpmpp2m']:.3e}")
    assert dev["dpmpp2m"] <= 4 * dev["ddim"]
    a = smp.DDIMSampler(model, CPU, k=k, solver="dpmpp2m").sample(N, noise=noise)
    b = smp.DDIMSampler(model, CPU, k=k).sample(N, noise=noise)
    assert not torch.equal(a, b)                                   # (the second-order term is there)


def test_sequence(model, noise):
    k = model.total_steps // 4
    s = smp.DDIMSampler(model, CPU, k=k, solver="dpmpp2m")
    seq = s.sequence(N, noise=noise)
    assert len(seq) == 4 + 1 and torch.equal(seq[0], (noise + 1) / 2)
    assert torch.equal(seq[-1], s.sample(N, noise=noise))
    ddim = smp.DDIMSampler(model, CPU, k=k).sequence(N, noise=noise)
    assert torch.equal(seq[1], ddim[1]) and not torch.equal(seq[2], ddim[2])   # the first step is DDIM's
    # an odd number of steps: the buffer written last is still the one returned
    k3 = 400
    s3 = smp.DDIMSampler(model, CPU, k=k3, solver="dpmpp2m")
    seq3 = s3.sequence(N, noise=noise)
    assert len(seq3) == 5 + 1 and torch.equal(seq3[-1], s3.sample(N, noise=noise))
    assert float((seq3[-1] - plain_loop(model, noise, k3, True)).abs().max()) < 1e-5


def test_model_api_takes_solver(model):
    gen = lambda: torch.Generator().manual_seed(1)  # noqa: E731
    a = model.sampler(CPU, k=500, N=2, generator=gen(), solver="dpmpp2m")
    b = model.sampler(CPU, k=500, N=2, generator=gen())
    assert a.shape == b.shape and not torch.equal(a, b)
    s1 = model.diffusion_sequence(CPU, k=500, N=2, generator=gen(), solver="dpmpp2m")
    assert len(s1) == 5 and torch.equal(s1[-1], a)


def test_from_starts_matches_per_sample_runs(model, noise):
    """Two samples joining one grid at their own starts, each = 1 rows: each equals the same
    sample run alone from its own start (the batch dimension only stacks them)."""
    starts, k = [1499, 999], 500
    both = smp.ddim_from_starts(model, noise, starts, k, CPU, solver="dpmpp2m")
    for b, s in enumerate(starts):
        alone = smp.ddim_from_starts(model, noise[b:b + 1], [s], k, CPU, solver="dpmpp2m")
        assert float((both[b:b + 1] - alone).abs().max()) < 1e-5
    ddim = smp.ddim_from_starts(model, noise, starts, k, CPU)
    assert not torch.equal(both[0], ddim[0])                       # three steps: a second-order one among them
    model.__dict__.pop("_sampler_graphs", None)


# ----------------------------------------------------------------------------- refusals, cache keys
def test_refusals(model, noise):
    with pytest.raises(ValueError):
        smp.DDIMSampler(model, CPU, k=500, solver="heun")
    with pytest.raises(ValueError):
        smp.DDIMSampler(model, CPU, k=500, solver="dpmpp2m", eta=0.5)
    with pytest.raises(ValueError):
        smp.ddim_from_starts(model, noise, [1499, 999], 500, CPU, solver="bogus")
    with pytest.raises(ValueError):
        smp.ddim_from_starts(model, noise, [1499, 999], 500, CPU, eta=1.0, solver="dpmpp2m")
    with pytest.raises(ValueError):
        smp.img2img(model, noise[0], [1499, 999], k=500, device=CPU, solver="dpm")
    with pytest.raises(ValueError):
        smp.img2img(model, noise[0], [1499, 999], k=500, device=CPU, eta=0.5, solver="dpmpp2m")
    assert smp.DDIMSampler(model, CPU, k=500, solver="ddim", eta=0.5).solver == "ddim"


def test_cache_keys(model, noise):
    model.__dict__.pop("_sampler_graphs", None)
    base = smp.DDIMSampler(model, CPU, k=500).sample(N, noise=noise)
    cache = smp._cache(model)
    assert list(cache) == [("ddim", N, 500, False, "cpu")]
    st = cache[("ddim", N, 500, False, "cpu")]
    smp.DDIMSampler(model, CPU, k=500, solver="dpmpp2m").sample(N, noise=noise)
    assert list(cache) == [("ddim", N, 500, False, "cpu"), ("ddim_dpm", N, 500, False, "cpu")]
    assert cache[("ddim", N, 500, False, "cpu")] is st
    assert torch.equal(smp.DDIMSampler(model, CPU, k=500).sample(N, noise=noise), base)
    model.__dict__.pop("_sampler_graphs", None)
    out = smp.img2img(model, noise[0], [1499, 999], k=500, device=CPU, generator=torch.Generator().manual_seed(2),
                      solver="dpmpp2m")
    assert out.shape == (2, 3, 16, 16)
    kinds = [key[0] for key in smp._cache(model)]
    assert kinds.count("img2img_dpm") == 1 and kinds.count("img2img") == 0
    smp.img2img(model, noise[0], [1499, 999], k=500, device=CPU, generator=torch.Generator().manual_seed(2))
    kinds = [key[0] for key in smp._cache(model)]
    assert kinds.count("img2img_dpm") == 1 and kinds.count("img2img") == 1
    ks = (1500, 750, 375, 300, 250, 150, 125, 100, 75, 60)        # more dpm loops than the limit: held to it,
    assert len(ks) > smp.IMG2IMG_GRAPHS
    for kk in ks:
        smp.img2img(model, noise[0], [1499], k=kk, device=CPU, solver="dpmpp2m")
    kinds = [key[0] for key in smp._cache(model)]
    assert kinds.count("img2img_dpm") == smp.IMG2IMG_GRAPHS and kinds.count("img2img") == 1   # the other kind kept
    model.__dict__.pop("_sampler_graphs", None)


# ----------------------------------------------------------------------------- CLI
def _cli(script, args):
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, script)] + args, capture_output=True, text=True, env=env,
                          timeout=600)


def test_cli_refuses_before_building_a_model(tmp_path):
    """``--model`` names no config: had a model been built first, that would be the error."""
    out = ["--out_dir", str(tmp_path)]
    r = _cli("ViT.py", ["--model", "no_such_model", "--solver", "bogus"] + out)
    assert r.returncode != 0 and "--solver" in r.stderr and "Traceback" not in r.stderr
    r = _cli("ViT.py", ["--model", "no_such_model", "--solver", "dpmpp2m", "--eta", "0.5"] + out)
    assert r.returncode != 0 and "--solver" in r.stderr and "Traceback" not in r.stderr
    r = _cli("ViT_draft2drawing.py", ["--solver", "bogus"] + out)
    assert r.returncode != 0 and "--solver" in r.stderr
    r = _cli("ViT_draft2drawing.py", ["--solver", "dpmpp2m", "--eta", "0.5"] + out)
    assert r.returncode != 0 and "--solver" in r.stderr
    assert os.listdir(str(tmp_path)) == []
