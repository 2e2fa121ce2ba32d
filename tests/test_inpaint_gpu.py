"""Inpainting on the GPU: ``repaint_rows_kernel`` (``ops.repaint_rows_``) against the device's own
``ops.randn_`` and an fp64 truth -- exact probes to the bit, the general case within a bound fixed
beforehand, its bf16 rows, what a paste-only call leaves alone, its argument checks, and the
seed / coefficients / mask read from device memory by a captured graph -- and the graph sampler
(``samplers.inpaint``) against an eager fp32 loop fed the same noise.

The bound: each stage is ``fma(b, z, fl(a v))``, two roundings of at most 2^-24 relative each on
quantities no larger than ``|a v| + |b z|``, so ``2 * 2^-24 * (|a v| + |b z|)``; the tests allow
twice that, ``4 * 2^-24 * (|ka known| + |kb z1|)`` for the paste and ``+ 4 * 2^-24 * (|ra y| +
|rb z2|)`` for the jump (``ra <= 1`` carries the paste's error over undiminished at most)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import build_model, ops
from ddim_cold_amd.diffusion import samplers as smp
from ddim_cold_amd.diffusion import schedule as sch
from ddim_cold_amd.ops import reference as ref

DEV = "cuda"
SEED = 4242
SHAPES = [(1, 4), (15, 48), (64, 192), (8200, 512)]   # one vector / ragged B = 3 / ViT-tiny rows / a 2nd grid trip
MASKS = ["zero", "one", "alt", "alt4", "random"]
SP, SJ = ops.SITE_PASTE_NOISE + 5, ops.SITE_JUMP_NOISE + 5
PAD = 64                                              # canary elements on either side of x / patches_out
X_CANARY = 0x4B3C614E                                 # fp32 bits (a finite value)
P_CANARY = 0x4B3C                                     # bf16 bits: bf16(X_CANARY's value, 0x4B3C614E -> 0x4B3C)
P_OTHER = 0x3E55                                      # bf16 bits unrelated to it
U = 2.0 ** -24


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


def _rng(seed=SEED):
    return torch.tensor([seed, 0], dtype=torch.int64, device=DEV)


def _randn(shape, site, seed=SEED):
    z = torch.empty(shape, device=DEV)
    ops.randn_(z, _rng(seed), site)
    return z


def _mask(name, shape, seed=0):
    n = shape[0] * shape[1]
    e = torch.arange(n, device=DEV)
    if name == "zero":
        m = torch.zeros(n, dtype=torch.bool, device=DEV)
    elif name == "one":
        m = torch.ones(n, dtype=torch.bool, device=DEV)
    elif name == "alt":
        m = e % 2 == 1                                 # mixed inside every 4-vector
    elif name == "alt4":
        m = (e // 4) % 2 == 1                          # whole 4-vectors
    else:
        m = (torch.rand(n, generator=torch.Generator().manual_seed(seed)) < 0.3).to(DEV)
    return (m.to(torch.uint8) * 255 if name == "random" else m.to(torch.uint8)).view(shape)


class _Case:
    """Operands of one shape (shared by its tests, never written): x, known, the two draws."""
    _made = {}

    def __new__(cls, shape):
        if shape not in cls._made:
            c = cls._made[shape] = super().__new__(cls)
            g = torch.Generator().manual_seed(shape[0])
            c.shape = shape
            c.x = (torch.randn(shape, generator=g) * 1.5).to(DEV)
            c.known = (torch.rand(shape, generator=g) * 2 - 1).to(DEV)
            c.z1, c.z2 = _randn(shape, SP), _randn(shape, SJ)
        return cls._made[shape]


def _canaried(shape, dtype, bits):
    """(whole buffer as ints, the [shape] slice in its middle as ``dtype``), every element ``bits``."""
    n = shape[0] * shape[1]
    ints = torch.int32 if dtype == torch.float32 else torch.int16
    whole = torch.full((n + 2 * PAD,), bits, dtype=ints, device=DEV)
    return whole, whole.view(dtype)[PAD:PAD + n].view(shape)


def _run(c, mask, coef, x_init=None, p_bits=P_OTHER):
    """One call on canaried buffers: (x, patches_out as int16 bits); the canaries are checked here."""
    xw, x = _canaried(c.shape, torch.float32, X_CANARY)
    pw, po = _canaried(c.shape, torch.bfloat16, p_bits)
    if x_init is not None:
        x.copy_(x_init)
    ops.repaint_rows_(x, c.known, mask, torch.tensor(coef, dtype=torch.float32, device=DEV), _rng(), SP, SJ, po)
    torch.cuda.synchronize()
    n = x.numel()
    for w, bits in ((xw, X_CANARY), (pw, p_bits)):
        assert bool((w[:PAD] == bits).all()) and bool((w[PAD + n:] == bits).all()), "a write outside the buffer"
    return x, po.view(torch.int16)


def _bits(v):
    return v.to(torch.bfloat16).view(torch.int16)


def _vec_any(keep):
    return keep.reshape(-1, 4).any(1, keepdim=True).expand(-1, 4).reshape(keep.shape)


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_probes(shape, mask_name):
    c = _Case(shape)
    mask = _mask(mask_name, shape)
    keep, wrote = mask != 0, _vec_any(mask != 0)

    def check_paste(x, po, want_kept):
        assert torch.equal(x[keep].view(torch.int32), want_kept[keep].view(torch.int32))
        assert torch.equal(x[~keep].view(torch.int32), c.x[~keep].view(torch.int32))       # the rest untouched
        assert torch.equal(po[wrote], _bits(x)[wrote]) and bool((po[~wrote] == P_OTHER).all())

    check_paste(*_run(c, mask, [1.0, 0.0, 1.0, 0.0], c.x), c.known)                        # known itself
    check_paste(*_run(c, mask, [0.0, 1.0, 1.0, 0.0], c.x), c.z1)                           # randn_ at the paste site
    ka = 0.8125 + 2.0 ** -20
    check_paste(*_run(c, mask, [ka, 0.0, 1.0, 0.0], c.x), c.known * ka)                    # fl(ka known)
    x, po = _run(c, torch.zeros_like(mask), [0.3, 0.4, 0.0, 1.0], c.x)                     # randn_ at the jump site
    assert torch.equal(x.view(torch.int32), c.z2.view(torch.int32)) and torch.equal(po, _bits(c.z2))


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_general_case_within_the_bound(shape, mask_name):
    c = _Case(shape)
    mask = _mask(mask_name, shape)
    keep = mask != 0
    ka, kb, ra, rb = (float(v) for v in torch.tensor(sch.repaint_row(2000, 999, 20, True), dtype=torch.float32))
    known, z1, z2, x0 = (v.double() for v in (c.known, c.z1, c.z2, c.x))
    y = torch.where(keep, ka * known + kb * z1, x0)
    b_paste = torch.where(keep, 4 * U * ((ka * known).abs() + (kb * z1).abs()), torch.zeros_like(y))
    # paste only: masked elements within the bound, the others to the bit
    x, po = _run(c, mask, [ka, kb, 1.0, 0.0], c.x)
    err = (x.double() - y).abs()
    print(f"{shape} {mask_name}: paste worst error / bound "
          f"{float((err[keep] / b_paste[keep]).max()) if bool(keep.any()) else 0.0:.3f}")
    assert bool((err <= b_paste).all())
    assert torch.equal(x[~keep].view(torch.int32), c.x[~keep].view(torch.int32))
    wrote = _vec_any(keep)
    assert torch.equal(po[wrote], _bits(x)[wrote]) and bool((po[~wrote] == P_OTHER).all())
    # paste + jump: every element written
    x, po = _run(c, mask, [ka, kb, ra, rb], c.x)
    want = ra * y + rb * z2
    bound = b_paste + 4 * U * ((ra * y).abs() + (rb * z2).abs())
    err = (x.double() - want).abs()
    print(f"{shape} {mask_name}: paste + jump worst error / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    assert torch.equal(po, _bits(x))


@pytest.mark.parametrize("mask_name", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_paste_only_leaves_the_rest_alone(shape, mask_name):
    """x starts as one bit pattern everywhere.  With patches_out holding that value's bf16 (what the
    head epilogue leaves there in the sampler) every unmasked element of both keeps its pattern; with
    an unrelated pattern in patches_out, every 4-vector without a mask byte keeps that one: no store
    happened there at all."""
    c = _Case(shape)
    mask = _mask(mask_name, shape)
    keep = mask != 0
    coef = [0.6, 0.8, 1.0, 0.0]
    x, po = _run(c, mask, coef, p_bits=P_CANARY)
    assert bool((x[~keep].view(torch.int32) == X_CANARY).all()) and bool((po[~keep] == P_CANARY).all())
    assert torch.equal(po[keep], _bits(x)[keep])
    x2, po2 = _run(c, mask, coef, p_bits=P_OTHER)
    assert torch.equal(x2.view(torch.int32), x.view(torch.int32))
    assert bool((po2[~_vec_any(keep)] == P_OTHER).all()) and torch.equal(po2[_vec_any(keep)], _bits(x)[_vec_any(keep)])
    if bool(keep.any()):
        assert not bool((x[keep].view(torch.int32) == X_CANARY).any())


def test_bad_calls_launch_nothing():
    shape = (15, 48)
    n = shape[0] * shape[1]
    good = dict(known=torch.zeros(shape, device=DEV), mask=torch.ones(shape, dtype=torch.uint8, device=DEV),
                coef=torch.tensor([0.5, 0.5, 0.5, 0.5], device=DEV), rng=_rng(), sp=SP, sj=SJ)
    xbuf = torch.full((n + 8,), 3.0, device=DEV)
    pbuf = torch.full((n + 8,), 7.0, dtype=torch.bfloat16, device=DEV)
    mbuf = torch.ones(n + 8, dtype=torch.uint8, device=DEV)
    x, po = xbuf[:n].view(shape), pbuf[:n].view(shape)
    bad = [
        dict(x=xbuf[:n].double().view(shape)),                                   # dtypes
        dict(known=good["known"].half()), dict(mask=good["mask"].bool()), dict(mask=good["mask"].to(torch.int8)),
        dict(coef=good["coef"].double()), dict(rng=_rng().to(torch.int32)), dict(po=po.float()),
        dict(known=good["known"].cpu()), dict(mask=good["mask"].cpu()), dict(coef=good["coef"].cpu()),   # devices
        dict(rng=_rng().cpu()), dict(po=po.cpu()),
        dict(known=torch.zeros(48, 15, device=DEV)), dict(mask=torch.ones(n, dtype=torch.uint8, device=DEV)),   # shapes
        dict(po=torch.zeros(n, dtype=torch.bfloat16, device=DEV)),
        dict(x=xbuf[:n - 2].view(1, n - 2), known=torch.zeros(1, n - 2, device=DEV),                          # numel % 4
             mask=torch.ones(1, n - 2, dtype=torch.uint8, device=DEV), po=None),
        dict(x=xbuf[1:n + 1].view(shape)), dict(po=pbuf[1:n + 1].view(shape)), dict(mask=mbuf[1:n + 1].view(shape)),   # alignment
        dict(known=x), dict(known=xbuf[4:n + 4].view(shape)),                    # x aliases / overlaps known
        dict(coef=good["coef"][:3].contiguous()), dict(coef=torch.zeros(8, device=DEV)),
        dict(rng=torch.zeros(3, dtype=torch.int64, device=DEV)), dict(rng=torch.zeros(1, dtype=torch.int64, device=DEV)),
        dict(sp=-1), dict(sj=-1),
        dict(known=torch.zeros(2 * shape[0], shape[1], device=DEV)[::2]),        # not contiguous
    ]
    for kw in bad:
        a = dict(good, x=x, po=po)
        a.update(kw)
        with pytest.raises(RuntimeError):
            torch.ops.ddim_cold.repaint_rows_(a["x"], a["known"], a["mask"], a["coef"], a["rng"], a["sp"], a["sj"], a["po"])
        torch.cuda.synchronize()
        assert bool((xbuf == 3.0).all()) and bool((pbuf == 7.0).all()), sorted(kw)
    ops.repaint_rows_(x, good["known"], good["mask"], good["coef"], good["rng"], SP, SJ, po)   # the good call runs
    assert not bool((x == 3.0).any()) and bool((xbuf[n:] == 3.0).all()) and bool((pbuf[n:] == 7.0).all())


def test_graph_reads_seed_coefficients_and_mask_from_memory():
    shape = (64, 192)
    c = _Case(shape)
    x = torch.empty(shape, device=DEV)
    po = torch.empty(shape, dtype=torch.bfloat16, device=DEV)
    rng, coef, mask = _rng(111), torch.tensor([0.6, 0.8, 1.0, 0.0], device=DEV), _mask("alt4", shape)

    def call():
        ops.repaint_rows_(x, c.known, mask, coef, rng, SP, SJ, po)

    def fresh(seed, cf, m):
        y = c.x.clone()
        ops.repaint_rows_(y, c.known, m, torch.tensor(cf, device=DEV), _rng(seed), SP, SJ)
        return y
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        call()
    seen = []
    for seed, cf, name in ((111, [0.6, 0.8, 1.0, 0.0], "alt4"), (222, [0.6, 0.8, 1.0, 0.0], "alt4"),
                           (222, [0.8, 0.6, 0.9, 0.5], "alt4"), (222, [0.8, 0.6, 0.9, 0.5], "random"),
                           (2 ** 40 + 5, [0.6, 0.8, 1.0, 0.0], "alt")):
        rng.copy_(_rng(seed))
        coef.copy_(torch.tensor(cf, device=DEV))
        mask.copy_(_mask(name, shape))
        x.copy_(c.x)
        g.replay()
        assert torch.equal(x, fresh(seed, cf, _mask(name, shape))), (seed, cf, name)
        seen.append(x.clone())
    assert all(not torch.equal(seen[i], seen[i + 1]) for i in range(len(seen) - 1))


# ----------------------------------------------------------------------------- the sampler
N = 4


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return build_model("vit_tiny").to(DEV).eval()


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(1)
    image = torch.rand(N, 3, 64, 64, generator=g) * 2 - 1
    noise = torch.randn(N, 3, 64, 64, generator=g)
    keep = torch.ones(64, 64, dtype=torch.bool)
    keep[16:48, 16:48] = False                         # a centred 32x32 hole
    return image, noise, keep


def _site_noise(model, seed, site):
    """The draw of ``site`` over the patch-row state, on the device, as an image batch."""
    p, (H, W), C = model.patch_size, model.img_size, model.in_chans
    z = torch.empty(N * (H // p) * (W // p), C * p * p, device=DEV)
    ops.randn_(z, torch.tensor([seed, 0], dtype=torch.int64, device=DEV), site)
    return ops.rows_to_image(z, N, C, H, W, p)


def _eager(model, image, keep, noise, k, eta, resample, seed):
    """fp32 eager loop (tests/test_ddim_eta_gpu.py's ``_eager`` with the mask step written out):
    forward_reference + ref.ddim_step_eta, then paste and jump in plain fp32 torch."""
    T = model.total_steps
    x, known, keep = noise.to(DEV).clone(), image.to(DEV), keep.to(DEV)
    n = 0
    with torch.no_grad():
        for t in sch.ddim_timesteps(T, k):
            for j in range(resample):
                raw = model.forward_reference(x, torch.full((N,), t, device=DEV))
                row = torch.tensor(sch.eta_row(T, t, k, eta), dtype=torch.float32, device=DEV)
                x, _ = ref.ddim_step_eta(x, raw, row, _site_noise(model, seed, ops.SITE_STEP_NOISE + n))
                ka, kb, ra, rb = sch.repaint_row(T, t, k, j < resample - 1)
                x = torch.where(keep, ka * known + kb * _site_noise(model, seed, ops.SITE_PASTE_NOISE + n), x)
                if j < resample - 1:
                    x = ra * x + rb * _site_noise(model, seed, ops.SITE_JUMP_NOISE + n)
                n += 1
    return ((x + 1) / 2).cpu(), n


@pytest.mark.parametrize("k,resample,eta,forwards", [(400, 1, 1.0, 5), (1000, 2, 0.0, 4)])
def test_sampler_matches_eager_reference(model, case, k, resample, eta, forwards):
    image, noise, keep = case
    model.__dict__.pop("_sampler_graphs", None)
    kw = dict(k=k, eta=eta, resample=resample, device=DEV, noise=noise, noise_seed=SEED)
    out = smp.inpaint(model, image, keep, **kw)
    exp, n = _eager(model, image, keep, noise, k, eta, resample, SEED)
    assert n == forwards
    d = (out - exp).abs()
    print(f"inpaint k={k} resample={resample} eta={eta}: mean |d| {d.mean():.4f} max |d| {d.max():.4f}")
    assert d.mean() < 0.01 and d.max() < 0.2, (d.mean(), d.max())
    unit = (image + 1) / 2
    assert torch.equal(out[:, :, keep], unit[:, :, keep])                 # kept pixels: the image to the bit
    st = smp._cache(model)[("inpaint", N, k, eta, resample, DEV)]
    assert st.loop.graph is not None and st.loop.replays == 0
    again = smp.inpaint(model, image, keep, **kw)
    assert st.loop.replays == 1 and torch.equal(out, again)               # a replay reproduces the capture run
    keep2 = keep.clone()
    keep2[:, 32:] = True                                                  # a new mask, then a new image: replays
    out2 = smp.inpaint(model, image, keep2, **kw)
    assert st.loop.replays == 2 and not torch.equal(out2, out) and torch.equal(out2[:, :, keep2], unit[:, :, keep2])
    out3 = smp.inpaint(model, image.flip(0), keep2, **kw)
    assert st.loop.replays == 3 and not torch.equal(out3, out2)
    assert torch.equal(out3[:, :, keep2], unit.flip(0)[:, :, keep2])
    other = smp.inpaint(model, image, keep, **dict(kw, noise_seed=SEED + 1))     # a new seed: a replay too
    assert st.loop.replays == 4 and not torch.equal(other, out)
    assert smp._cache(model)[("inpaint", N, k, eta, resample, DEV)] is st
    # nothing kept: the DDIM sampler's images
    free = smp.inpaint(model, image, torch.zeros(64, 64), **kw)
    ddim = smp.DDIMSampler(model, DEV, k=k, eta=eta).sample(N, noise=noise, noise_seed=SEED) if resample == 1 else None
    assert ddim is None or torch.equal(free, ddim)
    model.__dict__.pop("_sampler_graphs", None)


def test_all_zero_mask_is_the_ddim_sampler(model, case):
    image, noise, _ = case
    for eta in (0.0, 1.0):
        free = smp.inpaint(model, image, torch.zeros(64, 64), k=400, eta=eta, device=DEV, noise=noise, noise_seed=SEED)
        ddim = smp.DDIMSampler(model, DEV, k=400, eta=eta).sample(N, noise=noise, noise_seed=SEED)
        assert torch.equal(free, ddim), eta
    model.__dict__.pop("_sampler_graphs", None)


@pytest.mark.parametrize("k,resample,eta", [(400, 1, 1.0), (1000, 2, 0.0)])
def test_rows_path_against_the_fallback(model, case, k, resample, eta):
    image, noise, keep = case
    outs = {}
    for rows_on in (True, False):
        smp.ROWS = rows_on
        model.__dict__.pop("_sampler_graphs", None)
        try:
            outs[rows_on] = smp.inpaint(model, image, keep, k=k, eta=eta, resample=resample, device=DEV, noise=noise,
                                        noise_seed=SEED)
            again = smp.inpaint(model, image, keep, k=k, eta=eta, resample=resample, device=DEV, noise=noise,
                                noise_seed=SEED)
            assert torch.equal(outs[rows_on], again)
        finally:
            smp.ROWS = True
            model.__dict__.pop("_sampler_graphs", None)
    d = (outs[True] - outs[False]).abs()
    print(f"inpaint k={k} resample={resample} eta={eta}: rows path against the fallback, mean |d| {d.mean():.5f} "
          f"max |d| {d.max():.4f}")
    assert d.mean() < 2e-3 and d.max() < 0.05, (d.mean(), d.max())
    unit = (image + 1) / 2
    assert torch.equal(outs[False][:, :, keep], unit[:, :, keep])
