"""DPM-Solver++(2M) on the GPU: ``dpm2m_rows_kernel`` (``ops.dpm2m_rows_``) bit for bit against
``reference.dpm2m_rows`` run on the same device tensors -- its fp32 state and its bf16 rows, one
row and one row per sample, below one wave, across workgroup boundaries and past one pass of the
grid -- the exact probe, rows with g = 0 over a NaN history, its argument checks, and the graph
sampler against the same steps issued one by one, against the image-layout path and against the
fp32 CPU loop of ``tests/test_dpm2m_cpu.py``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import build_model, ops
from ddim_cold_amd.diffusion import samplers as smp
from ddim_cold_amd.diffusion import schedule as sch
from ddim_cold_amd.ops import reference as ref

from test_dpm2m_cpu import check_exact_probe, plain_loop

DEV = "cuda"
T = 2000
# [rows, F], B: below one wave / 576 4-vectors = 2.25 workgroups, samples straddling them / 4096 * 256 + 5
# 4-vectors: past one pass of the 4096-workgroup grid
SHAPES = [((4, 16), 1), ((12, 192), 3), ((1048581, 4), 1)]
PAD = 64                                              # canary elements on either side of x / patches_out
X_CANARY = 0x4B3C614E                                 # fp32 bits (a finite value)
P_CANARY = 0x3E55                                     # bf16 bits
NAN = float("nan")


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


class _Case:
    """Operands of one shape (shared by its tests, never written): x, x0, x0_prev on the device."""
    _made = {}

    def __new__(cls, shape):
        if shape not in cls._made:
            c = cls._made[shape] = super().__new__(cls)
            g = torch.Generator().manual_seed(shape[0])
            c.shape = shape
            c.x = (torch.randn(shape, generator=g) * 1.5).to(DEV)
            c.x0 = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
            c.x0p = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
        return cls._made[shape]


def _rows(batch, each):
    """Table rows with g != 0 (k = 100): one, or one per sample."""
    tab = sch.dpm2m_table(T, 100)[1]
    return (tab[[3, 9, 17][:batch]] if each else tab[9]).contiguous().to(DEV)


def _canaried(shape, dtype, bits):
    n = shape[0] * shape[1]
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    whole = torch.full((n + 2 * PAD,), bits, dtype=ints, device=DEV)
    return whole, whole.view(dtype)[PAD:PAD + n].view(shape)


def _run(c, x0p, coef, batch, each, with_po=True):
    """One call on canaried buffers: (x, patches_out as int16 bits or None); the canaries are checked here."""
    xw, x = _canaried(c.shape, torch.float32, X_CANARY)
    pw, po = _canaried(c.shape, torch.bfloat16, P_CANARY)
    x.copy_(c.x)
    ops.dpm2m_rows_(x, c.x0, x0p, coef, batch, each, patches_out=po if with_po else None)
    torch.cuda.synchronize()
    n = x.numel()
    for w, bits in ((xw, X_CANARY), (pw, P_CANARY)):
        assert bool((w[:PAD] == bits).all()) and bool((w[PAD + n:] == bits).all()), "a write outside the buffer"
    if not with_po:
        assert bool((pw == P_CANARY).all())
        return x, None
    return x, po.view(torch.int16)


def _bits(v):
    return v.to(torch.bfloat16).view(torch.int16)


@pytest.mark.parametrize("with_po", [True, False], ids=["pout", "nopout"])
@pytest.mark.parametrize("each", [False, True], ids=["one_row", "each"])
@pytest.mark.parametrize("shape,batch", SHAPES, ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"B{v}")
def test_kernel_is_the_reference_bit_for_bit(shape, batch, each, with_po):
    c = _Case(shape)
    coef = _rows(batch, each)
    want = ref.dpm2m_rows(c.x, c.x0, c.x0p, coef, batch, each)
    assert want.device.type == "cuda"
    x, po = _run(c, c.x0p, coef, batch, each, with_po)
    assert torch.equal(x.view(torch.int32), want.view(torch.int32))
    assert not torch.equal(x, c.x)
    if with_po:
        assert torch.equal(po, _bits(want))


def test_exact_probe_on_the_gpu():
    check_exact_probe(DEV)


@pytest.mark.parametrize("shape,batch", SHAPES[:2], ids=lambda v: f"{v[0]}x{v[1]}" if isinstance(v, tuple) else f"B{v}")
def test_zero_g_rows_over_a_nan_history(shape, batch):
    c = _Case(shape)
    nan = torch.full(shape, NAN, device=DEV)
    for each in (False, True):
        coef = _rows(batch, each).clone()
        coef[..., 4] = 0.0
        want = ref.dpm2m_rows(c.x, c.x0, torch.zeros_like(c.x0p), coef, batch, each)
        x, po = _run(c, nan, coef, batch, each)
        assert bool(torch.isfinite(x).all()) and torch.equal(x.view(torch.int32), want.view(torch.int32))
        assert torch.equal(po, _bits(want))


def test_identity_row_sample_with_a_nan_history():
    """each = 1, three samples: the middle one has not started (identity row) and its history is
    NaN: its x comes back to the bit; its neighbours take their own second-order step."""
    shape, batch = SHAPES[1]
    c = _Case(shape)
    coef = _rows(batch, True).clone()
    coef[1] = torch.tensor(sch.ETA_IDENT_ROW, device=DEV)
    x0p = c.x0p.clone()
    x0p[4:8] = NAN
    x, po = _run(c, x0p, coef, batch, True)
    assert torch.equal(x[4:8].view(torch.int32), c.x[4:8].view(torch.int32))
    want = ref.dpm2m_rows(c.x, c.x0, c.x0p, coef, batch, True)
    assert torch.equal(x.view(torch.int32), want.view(torch.int32)) and torch.equal(po, _bits(want))
    assert not torch.equal(x[:4], c.x[:4]) and not torch.equal(x[8:], c.x[8:])


def test_bad_calls_launch_nothing():
    shape, batch = (12, 192), 3
    n = shape[0] * shape[1]
    good = dict(x0=torch.zeros(shape, device=DEV), x0p=torch.ones(shape, device=DEV),
                coef=torch.tensor([0.5, 0.5, 0.5, 0.5, 0.5, 0, 0, 0], device=DEV), batch=batch, each=False)
    xbuf = torch.full((n + 8,), 3.0, device=DEV)
    pbuf = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    obuf = torch.zeros(n + 8, device=DEV)
    x, po = xbuf[:n].view(shape), pbuf[:n].view(shape)
    bad = [
        dict(x=xbuf[:n].double().view(shape)), dict(x0=good["x0"].half()), dict(x0p=good["x0p"].double()),   # dtypes
        dict(coef=good["coef"].double()), dict(po=po.float()),
        dict(x0=good["x0"].cpu()), dict(x0p=good["x0p"].cpu()), dict(coef=good["coef"].cpu()), dict(po=po.cpu()),   # devices
        dict(x0=torch.zeros(192, 12, device=DEV)), dict(x0p=torch.zeros(n, device=DEV)),                 # shapes
        dict(po=torch.zeros(n, dtype=torch.bfloat16, device=DEV)),
        dict(x=xbuf[:n - 2].view(1, n - 2), x0=torch.zeros(1, n - 2, device=DEV),                        # numel % 4
             x0p=torch.zeros(1, n - 2, device=DEV), po=None, batch=1),
        dict(batch=5), dict(batch=0), dict(batch=-3),                                                   # numel % (4 batch)
        dict(coef=good["coef"][:4].contiguous()), dict(coef=torch.zeros(8 * batch, device=DEV)),         # coef size
        dict(coef=good["coef"], each=True), dict(coef=torch.zeros(8 * batch + 8, device=DEV), each=True),
        dict(x=xbuf[1:n + 1].view(shape)), dict(po=pbuf[1:n + 1].view(shape)),                           # alignment
        dict(x0=obuf[1:n + 1].view(shape)), dict(x0p=obuf[1:n + 1].view(shape)),
        dict(x0=x), dict(x0p=x), dict(x0=xbuf[4:n + 4].view(shape)), dict(x0p=xbuf[4:n + 4].view(shape)),   # aliasing
        dict(x0=torch.zeros(2 * shape[0], shape[1], device=DEV)[::2]),                                   # not contiguous
    ]
    for kw in bad:
        a = dict(good, x=x, po=po)
        a.update(kw)
        with pytest.raises(RuntimeError):
            torch.ops.ddim_cold.dpm2m_rows_(a["x"], a["x0"], a["x0p"], a["coef"], a["batch"], a["each"], a["po"])
        torch.cuda.synchronize()
        assert bool((xbuf == 3.0).all()) and bool((pbuf == 7.0).all()), sorted(kw)
    ops.dpm2m_rows_(x, good["x0"], good["x0p"], good["coef"], batch, False, patches_out=po)   # the good call runs
    assert not bool((x == 3.0).any()) and bool((xbuf[n:] == 3.0).all()) and bool((pbuf[n:] == 7.0).all())


# ----------------------------------------------------------------------------- the sampler
N = 4
K = 500                                               # 4 steps: DDIM, two second-order ones, the last onto a = 1


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    m = build_model("vit_tiny").to(DEV).eval()
    with torch.no_grad():
        m.head.bias.uniform_(-0.5, 0.5)
    return m


def _noise(seed):
    return torch.randn(N, 3, 64, 64, generator=torch.Generator().manual_seed(seed))


def _eager(model, noise, k):
    """The loop's steps issued one by one on the device, no graph: per step one forward with
    ``HEAD_CLAMP`` into the x0 rows (``_Rows.predict_x0``) and one ``ops.dpm2m_rows_``."""
    den = smp._Denoiser(model, torch.device(DEV))
    s = smp._Rows(model, N, DEV, den)
    ts, coef = sch.dpm2m_table(model.total_steps, k, device=DEV)
    bufs = [s.x0, torch.zeros_like(s.x0)]
    with torch.no_grad():
        s.begin(noise.to(DEV))
        for i, t in enumerate(ts):
            s.x0 = bufs[i % 2]
            s.predict_x0(torch.full((N,), t, dtype=torch.int64, device=DEV))
            ops.dpm2m_rows_(s.x, bufs[i % 2], bufs[1 - i % 2], coef[i], N, False, patches_out=s.pin)
        return ((s.image(bufs[(len(ts) - 1) % 2]) + 1) / 2).cpu()


def test_captured_loop_is_the_eager_steps_bit_for_bit(model):
    model.__dict__.pop("_sampler_graphs", None)
    sampler = smp.DDIMSampler(model, DEV, k=K, solver="dpmpp2m")
    n1, n2 = _noise(21), _noise(22)
    first = sampler.sample(N, noise=n1)                               # the warm-up run's result, then the capture
    st = smp._cache(model)[("ddim_dpm", N, K, False, DEV)]
    assert st.loop.graph is not None and st.loop.replays == 0
    assert torch.equal(first, _eager(model, n1, K))
    again = sampler.sample(N, noise=n1)                               # a replay
    assert st.loop.replays == 1 and torch.equal(again, first)
    other = sampler.sample(N, noise=n2)                               # a second replay, new noise
    assert st.loop.replays == 2 and not torch.equal(other, first)
    assert torch.equal(other, _eager(model, n2, K))
    ddim = smp.DDIMSampler(model, DEV, k=K).sample(N, noise=n1)
    assert not torch.equal(ddim, first)
    assert sorted(key[0] for key in smp._cache(model)) == ["ddim", "ddim_dpm"]
    seq = sampler.sequence(N, noise=n1)
    assert len(seq) == 5 and torch.equal(seq[-1], first)
    model.__dict__.pop("_sampler_graphs", None)


def test_from_starts_each_rows_on_the_gpu(model):
    """Per-sample rows (each = 1) in the captured loop: a sample joining later equals its own run."""
    model.__dict__.pop("_sampler_graphs", None)
    starts = [1499, 999, 1499, 499]
    x = _noise(23).to(DEV)
    both = smp.ddim_from_starts(model, x, starts, K, DEV, solver="dpmpp2m")
    again = smp.ddim_from_starts(model, x, starts, K, DEV, solver="dpmpp2m")
    assert torch.equal(both, again)
    kinds = [key[0] for key in smp._cache(model)]
    assert kinds.count("img2img_dpm") == 1 and kinds.count("img2img") == 0
    same = smp.ddim_from_starts(model, x, [1499] * 4, K, DEV, solver="dpmpp2m")
    assert torch.equal(both[0], same[0]) and torch.equal(both[2], same[2])   # (rows of the batch are independent)
    assert not torch.equal(both[1], same[1])
    model.__dict__.pop("_sampler_graphs", None)


def _rows_on_off(model, noise, solver):
    outs = {}
    for rows_on in (True, False):
        smp.ROWS = rows_on
        model.__dict__.pop("_sampler_graphs", None)
        try:
            outs[rows_on] = smp.DDIMSampler(model, DEV, k=K, solver=solver).sample(N, noise=noise)
        finally:
            smp.ROWS = True
            model.__dict__.pop("_sampler_graphs", None)
    return (outs[True] - outs[False]).abs()


def test_rows_path_against_the_image_layout(model):
    """The allowed difference is twice what the DDIM sampler's two paths show here, same model,
    noise and grid (the test prints both; no measured value is recorded here yet)."""
    noise = _noise(24)
    d_ddim, d_dpm = _rows_on_off(model, noise, "ddim"), _rows_on_off(model, noise, "dpmpp2m")
    print(f"rows on / off: ddim mean |d| {d_ddim.mean():.3e} max |d| {d_ddim.max():.3e}; "
          f"dpmpp2m mean |d| {d_dpm.mean():.3e} max |d| {d_dpm.max():.3e}")
    assert d_dpm.mean() <= 2 * d_ddim.mean() and d_dpm.max() <= 2 * d_ddim.max()


def test_against_the_fp32_cpu_loop(model):
    """The GPU sampler (bf16 GEMMs) against the fp32 CPU loop of the CPU test, same model and
    noise; the bound is 4 x the deviation ``solver="ddim"`` shows against its own CPU loop here
    (the test prints both; no measured value is recorded here yet)."""
    noise = _noise(25)
    model.__dict__.pop("_sampler_graphs", None)
    cpu = build_model("vit_tiny").eval()
    cpu.load_state_dict(model.state_dict())
    dev = {}
    for solver in ("ddim", "dpmpp2m"):
        out = smp.DDIMSampler(model, DEV, k=K, solver=solver).sample(N, noise=noise)
        dev[solver] = float((out - plain_loop(cpu, noise, K, solver == "dpmpp2m")).abs().max())
    print(f"GPU sampler against the fp32 CPU loop: ddim {dev['ddim']:.3e}, dpmpp2m {dev['dpmpp2m']:.3e}")
    assert dev["dpmpp2m"] <= 4 * dev["ddim"]
    model.__dict__.pop("_sampler_graphs", None)
