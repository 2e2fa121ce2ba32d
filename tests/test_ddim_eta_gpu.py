"""Stochastic DDIM (eta > 0) on the GPU: the head epilogue that draws its own noise
(``ops.head_step_rows_`` modes 5 / 6, EPI_HEADRS) under the checks of ops/eta_check.py -- the
noise probe against ``ops.randn_`` to the bit, fp64 truths with a-priori bounds, the exact cases
-- over every geometry and 4-wave tile; its argument checks; the seed read from device memory
by a captured graph; and the graph samplers against an eager fp32 loop fed the same noise.
The derivations are in the module's docstring; tests/test_ddim_eta_cpu.py shows the checks to
pass the reference and an fp32 emulation and to reject the mutants."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import build_model, ops
from ddim_cold_amd.diffusion import samplers as smp
from ddim_cold_amd.diffusion import schedule as sch
from ddim_cold_amd.ops import eta_check as tc
from ddim_cold_amd.ops import gemm_check as gc
from ddim_cold_amd.ops import reference as ref

DEV = "cuda"
SEED = 4242


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


def assert_tile(cfg, epi, M, N, K):
    """The launch under the tile override is the LDS-DMA kernel on config ``cfg``'s tile."""
    got = tuple(int(v) for v in torch.ops.ddim_cold.gemm_plan(epi, False, False, M, N, K, 1))
    assert got[:4] == (1, *gc.TILES[cfg]), f"plan {got} is not config {cfg} = {gc.TILES[cfg]}"


# ----------------------------------------------------------------------------- the epilogue
@pytest.mark.parametrize("cfg", tc.TILE_CFGS)
@pytest.mark.parametrize("geom", tc.GEOMS)
def test_eta_epilogue_values(geom, cfg):
    M, N, K = tc.plan_shape(geom)
    with ops.gemm_tile(cfg):
        assert_tile(cfg, tc.EPI_HEADRS, M, N, K)
        assert_tile(cfg, gc.EPI_HEADR, M, N, K)     # the same launch plan as the deterministic step
        worst = tc.run_all(DEV, geom)
    print(f"stochastic DDIM step {geom} cfg {cfg}: worst error / bound {worst:.4f}")


def test_automatic_plan_is_the_deterministic_one():
    for M, N, K in [tc.plan_shape(g) for g in tc.GEOMS] + [(8 * 65, 192, 192), (64 * 65, 192, 192)]:
        a = [int(v) for v in torch.ops.ddim_cold.gemm_plan(tc.EPI_HEADRS, False, False, M, N, K, 1)]
        b = [int(v) for v in torch.ops.ddim_cold.gemm_plan(gc.EPI_HEADR, False, False, M, N, K, 1)]
        assert a == b, (M, N, K, a, b)


def test_epilogue_noise_against_cpu_generator():
    """The generator's HIP-vs-CPU agreement (1e-4, tests/test_kernels_gpu.py::test_randn_stats) holds
    for the epilogue's draw as well."""
    geom = tc.GEOMS[3]
    case = tc.ddim_case(geom)
    B, NP, F = tc.dims(geom)
    z = tc.probe_noise(case, DEV, tc.rng_of(DEV), tc.step_site(2)).cpu()
    want = torch.empty(B * NP, F)
    ops.randn_(want, tc.rng_of("cpu"), tc.step_site(2))
    d = float((z - want).abs().max())
    print(f"epilogue z against the CPU randn_: max |d| {d:.3e}")
    assert d < 1e-4


def test_bad_calls_launch_nothing():
    geom = tc.GEOMS[0]
    c = tc.ddim_case(geom)
    B, NP, F = tc.dims(geom)
    a, w, bias = (t.to(DEV) for t in (c.a, c.w, c.bias))
    rng = tc.rng_of(DEV)
    row8 = tc.eta_rows((999,), 1.0)[0].to(DEV)
    bad = [
        dict(coef=row8, mode=5, rng=None),                                       # no rng
        dict(coef=row8[:4].contiguous(), mode=5, rng=rng),                       # a 4-float row
        dict(coef=row8, mode=6, rng=rng),                                        # mode 6: one row for B = 2
        dict(coef=tc.eta_rows((999,) * (B + 1), 1.0).to(DEV), mode=6, rng=rng),  # ... and B + 1 rows
        dict(coef=row8, mode=5, rng=rng.to(torch.int32)),                        # rng dtype
        dict(coef=row8, mode=5, rng=tc.rng_of("cpu")),                           # rng on the host
        dict(coef=row8, mode=7, rng=rng),                                        # no such mode
    ]
    for kw in bad:
        x = torch.full((B * NP, F), 3.0, device=DEV)
        x0 = torch.full((B * NP, F), 5.0, device=DEV)
        po = torch.full((B * NP, F), 7.0, dtype=torch.bfloat16, device=DEV)
        with pytest.raises(RuntimeError):
            torch.ops.ddim_cold.head_step_rows_(a, w, bias, x, x0, kw["coef"], B, kw["mode"], None, None, 1e-5, po,
                                                kw["rng"], tc.step_site(0))
        torch.cuda.synchronize()
        assert bool((x == 3.0).all()) and bool((x0 == 5.0).all()) and bool((po == 7.0).all()), kw["mode"]
    with pytest.raises(ValueError):
        ops.head_step_rows_(a, w, bias, torch.zeros(B * NP, F, device=DEV), torch.zeros(B * NP, F, device=DEV), row8, B, 5)


def test_seed_is_read_from_device_memory():
    geom = tc.GEOMS[2]
    c = tc.ddim_case(geom)
    B, NP, F = tc.dims(geom)
    a, w, bias = (t.to(DEV) for t in (c.a, c.w, c.bias))
    probe = torch.tensor(tc.PROBE_ROW, device=DEV)
    rng = tc.rng_of(DEV, 111)
    x = torch.zeros(B * NP, F, device=DEV)
    x0 = torch.zeros_like(x)

    def call(site):
        ops.head_step_rows_(a, w, bias, x, x0, probe, B, 5, noise=(rng, site))

    def randn(seed, site):
        z = torch.empty(B * NP, F, device=DEV)
        ops.randn_(z, tc.rng_of(DEV, seed), site)
        return z
    s0 = tc.step_site(0)
    call(s0)
    first = x.clone()
    call(s0)
    assert torch.equal(x, first) and torch.equal(first, randn(111, s0))    # same seed and site: the same bits
    call(s0 + 1)
    assert not torch.equal(x, first) and torch.equal(x, randn(111, s0 + 1))  # consecutive sites differ
    # one captured mode-5 step: the seed is a load from the buffer, not a captured constant
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(s0)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call(s0)
    for seed in (222, 111, 2 ** 40 + 5):
        rng.copy_(tc.rng_of(DEV, seed))
        x.zero_()
        g.replay()
        assert torch.equal(x, randn(seed, s0)), seed
    assert not torch.equal(randn(222, s0), randn(111, s0))


# ----------------------------------------------------------------------------- samplers
@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model("vit_tiny").to(DEV).eval()


def _step_noise(model, N, seed, i):
    """Step i's noise as an image batch, drawn on the device over the patch-row state."""
    p, (H, W), C = model.patch_size, model.img_size, model.in_chans
    z = torch.empty(N * (H // p) * (W // p), C * p * p, device=DEV)
    ops.randn_(z, torch.tensor([seed, 0], dtype=torch.int64, device=DEV), ops.SITE_STEP_NOISE + i)
    return ops.rows_to_image(z, N, C, H, W, p)


def _eager(model, x, ts, rows, seed):
    """fp32 eager loop: forward_reference + ref.ddim_step_eta with ``rows[i]`` ([8] or [N, 8]) per step."""
    x = x.to(DEV).clone()
    N = x.shape[0]
    with torch.no_grad():
        for i, t in enumerate(ts):
            raw = model.forward_reference(x, torch.full((N,), t, device=DEV))
            x, x0 = ref.ddim_step_eta(x, raw, rows[i].to(DEV), _step_noise(model, N, seed, i))
    return x0


def test_eta_sampler_matches_eager_reference(model):
    noise = torch.randn(8, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    model.__dict__.pop("_sampler_graphs", None)
    s = smp.DDIMSampler(model, DEV, k=400, eta=1.0)
    out = s.sample(8, noise=noise, noise_seed=SEED)
    ts, rows = sch.ddim_table_eta(model.total_steps, 400, 1.0)
    exp = (_eager(model, noise, ts, rows, SEED).cpu() + 1) / 2
    d = (out - exp).abs()
    print(f"eta=1 k=400 N=8: mean |d| {d.mean():.4f} max |d| {d.max():.4f}")
    assert d.mean() < 0.01 and d.max() < 0.2, (d.mean(), d.max())
    st = s._state(8, False)
    assert st.loop.graph is not None and st.loop.replays == 0
    out2 = smp.DDIMSampler(model, DEV, k=400, eta=1.0).sample(8, noise=noise, noise_seed=SEED)
    assert st.loop.replays == 1 and torch.equal(out, out2)        # a replay reproduces the capture run
    other = s.sample(8, noise=noise, noise_seed=SEED + 1)            # a new seed needs no new capture
    assert st.loop.replays == 2 and not torch.equal(other, out)
    seq = s.sequence(8, noise=noise, noise_seed=SEED)
    assert len(seq) == 6 and torch.equal(seq[-1], out)
    det = smp.DDIMSampler(model, DEV, k=400).sample(8, noise=noise)
    assert torch.equal(smp.DDIMSampler(model, DEV, k=400, eta=0.0).sample(8, noise=noise), det)
    assert not torch.equal(det, out)


def test_eta_from_starts_matches_eager_reference_and_fallback(model):
    starts, k = [1199, 1599, 1999], 400
    g = torch.Generator().manual_seed(9)
    draft = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).to(DEV)
    eps = torch.randn(len(starts), 3, 64, 64, generator=g).to(DEV)
    x = smp.img2img_noised(draft, eps, starts, model.total_steps)
    ts, rows = smp.starts_table_eta(model.total_steps, starts, k, 1.0)
    exp = _eager(model, x, ts, rows, SEED)
    outs = {}
    for rows_on in (True, False):
        smp.ROWS = rows_on
        model.__dict__.pop("_sampler_graphs", None)
        try:
            outs[rows_on] = smp.ddim_from_starts(model, x, starts, k, eta=1.0, noise_seed=SEED)
            again = smp.ddim_from_starts(model, x, starts, k, eta=1.0, noise_seed=SEED)   # replay
            assert torch.equal(outs[rows_on], again)
        finally:
            smp.ROWS = True
            model.__dict__.pop("_sampler_graphs", None)
    for b in range(len(starts)):
        d = (outs[True][b] - exp[b]).abs() / 2        # on the [0, 1] image scale
        print(f"eta=1 start {starts[b]}: mean |d| {d.mean():.4f} max |d| {d.max():.4f}")
        assert d.mean() < 0.01 and d.max() < 0.2, (b, d.mean(), d.max())
    d = (outs[True] - outs[False]).abs() / 2
    print(f"rows path against the fallback: mean |d| {d.mean():.5f} max |d| {d.max():.4f}")
    assert d.mean() < 2e-3 and d.max() < 0.05, (d.mean(), d.max())
