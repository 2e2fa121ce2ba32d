"""Weight EMA on the GPU: the fused AdamW + EMA kernel checked on raw bits (vector path,
scalar tail, unaligned fallback, second trip through the strided loop, partial gradient
zeroing, skipped step), the warm-up ramp computed on the device, the binding's errors,
and the engine: eager == graph replay, training untouched, the swap scope under the
model's forward / the samplers' cached graphs, and host snapshots."""
import pytest
import torch

from ddim_cold_amd import build_model, ops
from ddim_cold_amd.data.synthetic import ColdBatcher, synthetic_pool
from ddim_cold_amd.train.engine import EngineConfig, TrainEngine

pytestmark = pytest.mark.gpu
DEV = "cuda"
HYPER = [3e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 10.0, 0.0]
# scalar tail alone, one vector, vector + tail, several blocks, and > 2048 x 256 x 4
# elements: past the grid cap, so threads take a second trip through the strided loop
SIZES = [1, 3, 4, 5, 1027, 100_003, 2_098_181]


def _arenas(n, off=0, t=0, hyper=HYPER, seed=0):
    """Random p / e / g / m / v (+ bf16 shadow) of ``n`` elements starting ``off`` elements
    into their buffers (off = 1: no 16-byte alignment, the scalar fallback)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    a = {k: torch.randn(n + off, device=DEV, generator=g)[off:] for k in ("p", "e", "g")}
    a["m"] = (torch.randn(n + off, device=DEV, generator=g) * 0.01)[off:]
    a["v"] = (torch.rand(n + off, device=DEV, generator=g) * 1e-3)[off:]
    a["pb"] = torch.zeros(n + off, device=DEV, dtype=torch.bfloat16)[off:]
    a["sq"] = torch.zeros(ops.SQ_PARTS, device=DEV)
    ops.sqnorm(a["g"].clone(), a["sq"], 1.0)  # (a fresh, aligned copy: sqnorm reads 16-byte vectors)
    a["step"] = torch.tensor([t, t], dtype=torch.int64, device=DEV)
    a["hyper"] = torch.tensor(hyper, device=DEV)
    return a


def _clone(a, off=0):
    out = {}
    for k, v in a.items():
        if k in ("sq", "step", "hyper"):
            out[k] = v.clone()
        else:  # keep the (mis)alignment of the original view
            buf = torch.empty(v.numel() + off, device=DEV, dtype=v.dtype)
            buf[off:].copy_(v)
            out[k] = buf[off:]
    return out


def _step(a, **kw):
    ops.adamw_step(a["p"], a["g"], a["m"], a["v"], a["pb"], a["sq"], a["step"], a["hyper"], 1.0, **kw)
    torch.cuda.synchronize()


def _formula(e_before, p_after, d32):
    """e <- p + d (e - p) on the CPU: three separately rounded fp32 operations."""
    p = p_after.cpu()
    return p + d32 * (e_before.cpu() - p)


def _check_exact(n, off=0, zero_hi=None):
    a0 = _arenas(n, off)
    plain, a = _clone(a0, off), _clone(a0, off)
    kw = {} if zero_hi is None else dict(zero_hi=zero_hi)
    _step(plain, **kw)
    _step(a, ema=a["e"], ema_decay=0.9, ema_warmup=False, **kw)
    assert torch.equal(a["e"].cpu(), _formula(a0["e"], a["p"], torch.tensor(0.9)))
    assert not torch.equal(a["e"], a0["e"])
    for k in ("p", "m", "v", "pb", "g"):
        assert torch.equal(a[k], plain[k]), k
    assert not torch.equal(a["p"], a0["p"])
    return a0, a


@pytest.mark.parametrize("n", SIZES)
def test_kernel_exact(n):
    a0, a = _check_exact(n)
    assert torch.all(a["g"] == 0)


@pytest.mark.parametrize("n", [5, 1027, 100_003])
def test_kernel_exact_unaligned(n):
    a0, a = _check_exact(n, off=1)
    assert a["e"].data_ptr() % 16 == 4 and a["p"].data_ptr() % 16 == 4
    # only the EMA arena misaligned: it alone must switch the vector path off
    b0 = _arenas(n)
    b = _clone(b0)
    buf = torch.empty(n + 1, device=DEV)
    buf[1:].copy_(b0["e"])
    _step(b, ema=buf[1:], ema_decay=0.9, ema_warmup=False)
    assert torch.equal(buf[1:].cpu(), _formula(b0["e"], b["p"], torch.tensor(0.9)))


def test_kernel_partial_grad_zeroing():
    n, zh = 100_003, 40_962  # rounded up to whole 16-byte vectors: 40,964
    a0, a = _check_exact(n, zero_hi=zh)
    assert torch.all(a["g"][:40_964] == 0) and torch.equal(a["g"][40_964:], a0["g"][40_964:])


def test_kernel_skipped_step_leaves_ema_alone():
    a0 = _arenas(100_003)
    a0["sq"][17] = float("inf")
    a = _clone(a0)
    _step(a, ema=a["e"], ema_decay=0.9, ema_warmup=False)
    for k in ("p", "m", "v", "e"):
        assert torch.equal(a[k], a0[k]), k
    assert torch.all(a["g"] == 0)


@pytest.mark.parametrize("t", [0, 1, 90, 100_000])
def test_warmup_on_device(t):
    """d = min(decay, (1 + t) / (10 + t)) computed by the kernel from step[0].  Bound,
    elementwise: 2^-23 (|e_before - p_after| + |e_after|) -- a one-ulp difference in the
    quotient (d < 1: at most 2^-24 |e_before - p_after| in the product), the product's own
    rounding and the sum's; derived from the fp32 format, not from what the kernel gives."""
    decay = 0.9999
    a0 = _arenas(100_003, t=t)
    a = _clone(a0)
    _step(a, ema=a["e"], ema_decay=decay, ema_warmup=True)
    d32 = ops.weight_ema_decay(decay, t, True)
    ref = _formula(a0["e"], a["p"], d32)
    got = a["e"].cpu()
    bound = 2.0 ** -23 * ((a0["e"].cpu() - a["p"].cpu()).abs() + got.abs())
    assert torch.all((got - ref).abs() <= bound)
    # the ramp is really used: the constant decay would land elsewhere (t < 89,991)
    if t < 89_991:
        flat = _formula(a0["e"], a["p"], torch.tensor(decay, dtype=torch.float32))
        assert not torch.all((got - flat).abs() <= bound)
    if t == 0:  # d itself: e = 0, p = 1 (lr 0, so p stays) -> 1 + 0.1 (0 - 1) = 0.9
        h = list(HYPER)
        h[0] = 0.0
        b = _arenas(1027, hyper=h)
        b["p"].fill_(1.0)
        b["e"].zero_()
        _step(b, ema=b["e"], ema_decay=decay, ema_warmup=True)
        assert torch.all(b["p"] == 1.0)
        assert torch.all((b["e"] - 0.9).abs() <= 2.0 ** -23 * (1.0 + b["e"].abs()))


def test_binding_errors_launch_nothing():
    n = 1028
    a0 = _arenas(n)
    a = _clone(a0)

    def intact():
        torch.cuda.synchronize()
        return all(torch.equal(a[k], a0[k]) for k in ("p", "g", "m", "v", "e", "pb"))
    with pytest.raises(RuntimeError, match="lazy"):
        _step(a, ema=a["e"], ema_decay=0.9, lazy=(256, 512), lazy_decay=torch.ones(1, device=DEV))
    assert intact()
    with pytest.raises(RuntimeError):
        _step(a, ema=a["e"].double(), ema_decay=0.9)
    assert intact()
    with pytest.raises(RuntimeError):
        _step(a, ema=a["e"].to(torch.bfloat16), ema_decay=0.9)
    assert intact()
    with pytest.raises(RuntimeError, match="size"):
        _step(a, ema=a["e"][:-1], ema_decay=0.9)
    assert intact()
    with pytest.raises(RuntimeError, match="ema_decay"):
        _step(a, ema=a["e"], ema_decay=1.0)
    assert intact()
    _step(a, ema=a["e"], ema_decay=0.9)  # and the good call still runs
    assert not torch.equal(a["e"], a0["e"])


# ------------------------------------------------------------------ engine
def _engine(weight_ema=0.9, temb_rows=7, seed=0, **kw):
    """The model configuration of tests/test_engine_gpu.py: ViT-tiny, batch 8."""
    torch.manual_seed(seed)
    model = build_model("vit_tiny").cuda().train()
    cfg = dict(lr=1e-3, t_max=100, seed=3, use_graph=False, graph_warmup=1, temb_rows=temb_rows,
               weight_ema=weight_ema)
    cfg.update(kw)
    eng = TrainEngine(model, EngineConfig(**cfg))
    eng.set_batch_fn(ColdBatcher(synthetic_pool(64, seed=1, device="cuda"), 8, eng.rng))
    return eng


@pytest.fixture(scope="module")
def eager8():
    """8 eager steps with weight_ema = 0.9: the reference the other engine tests share."""
    eng = _engine()
    eng.train_steps(8)
    torch.cuda.synchronize()
    return eng.flat_p.clone(), eng.flat_e.clone()


def test_engine_graph_matches_eager(eager8):
    p_e, e_e = eager8
    eng = _engine(use_graph=True, graph_steps=4)
    eng.train_steps(8)
    torch.cuda.synchronize()
    assert eng._multi is not None and eng._multi[1] == 4 and int(eng.step_ctr[0]) == 8
    assert eng.lazy is None
    assert not torch.equal(eng.flat_e, eng.flat_p)
    assert torch.equal(eng.flat_p, p_e)
    assert torch.equal(eng.flat_e, e_e)


def test_engine_ema_does_not_perturb_training(eager8):
    p_e, _ = eager8
    off = _engine(weight_ema=0.0, temb_rows=None)
    off.train_steps(8)
    torch.cuda.synchronize()
    assert off.flat_e is None and off.lazy is None
    assert torch.equal(off.flat_p, p_e)


def _ema_twin(eng):
    """A fresh model loaded from ``eng.ema_state_dict()``, owned by an engine of its own
    so that the bf16 shadow, the LayerNorm fold and the transposed shadows are derived
    from the arena by the same code (a bare model folds from the fp32 weights instead of
    the bf16 shadow, which rounds differently whatever the weights are)."""
    twin = build_model("vit_tiny").cuda()
    twin.load_state_dict(eng.ema_state_dict(), strict=True)
    TrainEngine(twin, EngineConfig(use_graph=False, temb_rows=7))
    return twin.eval()


def test_scope_forward_and_training_after_it():
    eng, ctl = _engine(use_graph=True), _engine(use_graph=True)
    eng.train_steps(4)
    ctl.train_steps(4)
    model = eng.model
    g = torch.Generator().manual_seed(5)
    x = torch.randn(4, 3, 64, 64, generator=g).cuda()
    t = torch.tensor([1, 3, 5, 6], device=DEV)
    twin = _ema_twin(eng)
    p0, e0 = eng.flat_p.clone(), eng.flat_e.clone()
    model.eval()
    with torch.no_grad():
        raw = model(x, t)
        with eng.ema_weights():
            got = model(x, t)
        want = twin(x, t)
        again = model(x, t)
    model.train()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and not torch.equal(got, raw)
    assert torch.equal(again, raw)
    assert torch.equal(eng.flat_p, p0) and torch.equal(eng.flat_e, e0)
    # the captured step graph is still valid: one more replayed step == never swapped
    assert eng._graphs is not None
    eng.train_step()
    ctl.train_step()
    torch.cuda.synchronize()
    assert torch.equal(eng.flat_p, ctl.flat_p) and torch.equal(eng.flat_e, ctl.flat_e)


def test_scope_sampler_graph_replays_on_swapped_weights():
    from ddim_cold_amd.diffusion.samplers import DDIMSampler, _cache
    eng = _engine()
    eng.train_steps(3)
    model = eng.model.eval()
    noise = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(7))
    smp = DDIMSampler(model, DEV, k=500)  # 4 steps
    twin = _ema_twin(eng)
    first = smp.sample(2, noise=noise)
    loop = next(iter(_cache(model).values())).loop
    assert loop.graph is not None
    with eng.ema_weights():
        mid = smp.sample(2, noise=noise)
    last = smp.sample(2, noise=noise)
    assert loop.replays == 2 and len(_cache(model)) == 1  # the one cached graph, replayed
    want = DDIMSampler(twin, DEV, k=500).sample(2, noise=noise)
    assert torch.equal(first, last)
    assert torch.equal(mid, want) and not torch.equal(mid, first)


def test_snapshot_holds_the_ema():
    eng = _engine()
    eng.train_steps(2)
    snap = eng.snapshot_to_host()
    snap.wait()
    sd, want = snap.ema_state_dict(), eng.ema_state_dict()
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k].cpu()) for k in want)
    assert snap.ema.is_pinned()
    host, dev, _ = eng._snap
    ptrs = [t.data_ptr() for t in host + dev]
    snap2 = eng.snapshot_to_host()
    snap2.wait()
    assert [t.data_ptr() for t in eng._snap[0] + eng._snap[1]] == ptrs and snap2.ema is snap.ema
