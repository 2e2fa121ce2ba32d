"""The epilogue-arithmetic checks (ops/epi_check.py) on the CPU: the reference passes every
runner of tests/test_epi_values_gpu.py, the fp32 emulation of the kernels' arithmetic passes
the same bounds, each arithmetic mutant is rejected, and a probe that breaks the exactness
condition fails before anything is compared."""
import pytest
import torch

from ddim_cold_amd.ops import epi_check as ec
from ddim_cold_amd.ops import reference as ref

CPU = "cpu"


def rejected(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


# ----------------------------------------------------------------------------- the device
def test_all_bf16_patterns():
    x = ec.all_bf16()
    bits = x.view(torch.int16).int() & 0xFFFF
    finite = (torch.arange(65536) & 0x7F80) != 0x7F80
    assert int(finite.sum()) == 65536 - 256
    assert torch.equal(bits[finite], torch.arange(65536, dtype=torch.int32)[finite])
    assert int(torch.count_nonzero(bits[~finite])) == 0
    assert int(torch.signbit(x.float()).sum()) == 32640


def test_exactness_condition_is_asserted():
    c = ec.gelu_case()
    assert torch.equal(ec.onehot_truth(c.a, c.w), c.w.float().t())
    two = c.a.clone()
    two[3, 5] = 1                                   # a second product in row 3
    rejected(ec.onehot_truth, two, c.w)
    half = c.a.clone()
    half[7, 7] = 0.5
    rejected(ec.onehot_truth, half, c.w)
    inf = c.w.clone()
    inf[0, 0] = float("inf")                        # 0 x inf
    rejected(ec.onehot_truth, c.a, inf)
    l1 = ec.l1_case(ec.GEOMS[0], 0.5)
    assert torch.equal(ec.bias_truth(l1.a, l1.w, l1.bias), l1.bias)
    dirty = l1.a.clone()
    dirty[1, 2] = 1
    rejected(ec.bias_truth, dirty, l1.w, l1.bias)
    rejected(ec.bias_truth, l1.a, l1.w, torch.full_like(l1.bias, float("nan")))
    assert float(ec.exact_difference(torch.tensor([0.5]), torch.tensor([0.25]))) == 0.25
    rejected(ec.exact_difference, torch.tensor([1.0]), torch.tensor([2.0 ** -30]))


def test_ulp_bf16():
    a = torch.tensor([1.0, 1.99, 2.0, 0.0, 2.0 ** -130, 3.0e38, float("inf")], dtype=torch.float64)
    want = [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** 120, 2.0 ** 120]
    assert ec.ulp_bf16(a).tolist() == want


# ----------------------------------------------------------------------------- 1. GELU
@pytest.mark.parametrize("p", ec.DROPOUT_PS)
def test_gelu_reference_and_emulation_pass(p):
    assert ec.run_gelu(CPU, p) <= 1.0
    c = ec.gelu_case()
    keep = ec._keep(c.v.numel(), ec.GELU_SITE, p, c.v.shape)
    worst = ec.check_gelu_h(ec.gelu_f32(c.v, p, keep), p, "fp32 emulation of gelu_f")
    assert 0.9 < worst <= 1.0                       # the half ulp dominates: the bound is tight


def test_norm_cdf_emulation_accuracy():
    """What csrc/common.h says of ``norm_cdf``: 8.6e-7 at worst over every bf16 input."""
    x = ec.gelu_case().v
    err = (ec.norm_cdf_f32(x).double() - ec.phi64(x)).abs()
    assert 5e-7 < float(err.max()) < 1e-6 < ec.PHI_TOL
    assert abs(float(x.flatten()[err.argmax()])) < 0.2


@pytest.mark.parametrize("p", ec.DROPOUT_PS)
def test_gelu_rejects_dropped_leading_coefficient(p):
    c = ec.gelu_case()
    keep = ec._keep(c.v.numel(), ec.GELU_SITE, p, c.v.shape)
    mutant = ec.gelu_f32(c.v, p, keep, coef=(0.0,) + ec.AS_COEF[1:])
    # ... which the suite's older tolerance accepts at every input
    good = ec.gelu_f32(c.v, p, keep).float()
    fin = torch.isfinite(good)
    assert bool(((mutant.float() - good).abs()[fin] <= 2e-2 + 1e-2 * good.abs()[fin]).all())
    rejected(ec.check_gelu_h, mutant, p)


def test_gelu_rejects_sign_and_mask_faults():
    c = ec.gelu_case()
    h = ec.gelu_f32(c.v)
    pos = h.clone()
    pos[c.v == -8.0] = 2.0 ** -30                   # a positive GELU at a negative input, inside the bound
    rejected(ec.check_gelu_h, pos, 0.0)
    keep = ec._keep(c.v.numel(), ec.GELU_SITE, 0.1, c.v.shape)
    other = ref.keep_mask(c.v.numel(), ec._rng(CPU), ec.GELU_SITE + 1, 0.1).view(c.v.shape)
    rejected(ec.check_gelu_h, ec.gelu_f32(c.v, 0.1, other), 0.1)
    u = c.v.to(torch.bfloat16)
    assert ec.check_gelu_u(u) == (254, 0)
    flushed = torch.where(c.v.abs() < ec.TINY, torch.zeros(()), c.v).to(torch.bfloat16)
    assert ec.check_gelu_u(flushed) == (0, 254)
    off = u.clone()
    off[5, 500] = off[5, 500] * 1.0078125           # one bf16 ulp
    rejected(ec.check_gelu_u, off)
    ec.check_gelu_h(ec.gelu_f32(c.v, 0.1, keep), 0.1)


# ----------------------------------------------------------------------------- 2. GELU'
@pytest.mark.parametrize("p", ec.DROPOUT_PS)
def test_dgelu_reference_and_emulation_pass(p):
    assert ec.run_dgelu(CPU, p) <= 1.0
    c = ec.dgelu_case()
    keep = ec._keep(c.dh.numel(), ec.DGELU_SITE, p, c.dh.shape)
    assert ec.check_dgelu(ec.dgelu_f32(c.dh, c.u, p, keep), p, "fp32 emulation of gelu_grad_f") <= 1.0


@pytest.mark.parametrize("p", ec.DROPOUT_PS)
def test_dgelu_rejects_forgotten_log2e(p):
    c = ec.dgelu_case()
    keep = ec._keep(c.dh.numel(), ec.DGELU_SITE, p, c.dh.shape)
    rejected(ec.check_dgelu, ec.dgelu_f32(c.dh, c.u, p, keep, log2e=False), p)


def test_dgelu_case_condition():
    c = ec.dgelu_case()
    assert set(c.dh.unique().tolist()) == set(ec.DGELU_S)
    rejected(ec.onehot_truth, c.dy.float() * 2, c.w.t())


# ----------------------------------------------------------------------------- 3. smooth-L1
@pytest.mark.parametrize("beta", ec.BETAS)
@pytest.mark.parametrize("geom", ec.GEOMS)
def test_smooth_l1_reference_and_emulation_pass(geom, beta):
    r_loss, r_grad = ec.run_smooth_l1(CPU, geom, beta)
    assert r_loss <= 1.0 and r_grad <= 1.0
    c = ec.l1_case(geom, beta)
    ec.check_l1(*ec.smooth_l1_f32(c.d, beta, geom), c, "fp32 emulation")


@pytest.mark.parametrize("mutant", ["dd*beta", "d*beta", "ad-0.5"])
@pytest.mark.parametrize("beta", [b for b in ec.BETAS if b != 1.0])
@pytest.mark.parametrize("geom", ec.GEOMS)
def test_smooth_l1_rejects_beta_mixups(geom, beta, mutant):
    c = ec.l1_case(geom, beta)
    rejected(ec.check_l1, *ec.smooth_l1_f32(c.d, beta, geom, mutant), c, mutant)


def test_smooth_l1_mixups_are_invisible_at_beta_one():
    """Why the cases leave beta = 1: there every mutant is the same arithmetic."""
    geom = ec.GEOMS[0]
    c = ec.l1_case(geom, 1.0)
    for mutant in ("dd*beta", "d*beta", "ad-0.5"):
        ec.check_l1(*ec.smooth_l1_f32(c.d, 1.0, geom, mutant), c, mutant)


def test_smooth_l1_rejects_gradient_faults():
    geom = ec.GEOMS[0]
    c = ec.l1_case(geom, 0.5)
    loss, dtok = ec.smooth_l1_f32(c.d, 0.5, geom)
    cls = dtok.clone()
    cls[0, 0] = 1e-8
    rejected(ec.check_l1, loss, cls, c, "cls row written")
    rejected(ec.check_l1, loss, -dtok, c, "sign of the gradient")
    rejected(ec.check_l1, loss * (1 + 2e-4), dtok, c, "loss off by 2e-4")


# ----------------------------------------------------------------------------- 4. DDIM update
@pytest.mark.parametrize("geom", ec.GEOMS)
def test_ddim_reference_passes(geom):
    assert ec.run_ddim(CPU, geom) <= 1.0
    assert ec.run_q_sample(CPU, geom) <= 1.0


def test_ddim_coefficient_rows():
    rows = ec.ddim_rows(ec.DDIM_TS)
    assert float(rows[2, 3]) == 0.0 and float(rows[2, 2]) == 1.0   # the last step: sqrt(1 - a_{t-k}) = 0
    assert float(rows[0, 0]) < 0.004                               # the first: a_t = 1e-5
    assert ec.ddim_rows((None,)).tolist() == [list(ec.IDENT_ROW)]
    sp = ec.ddim_specials().tolist()
    assert len(sp) == 11 and 1.0 + 2.0 ** -23 in sp and -(1.0 - 2.0 ** -24) in sp


@pytest.mark.parametrize("t", ec.DDIM_TS)
@pytest.mark.parametrize("geom", ec.GEOMS)
def test_ddim_rejects_swapped_coefficients(geom, t):
    c = ec.ddim_case(geom)
    rows = ec.ddim_rows((t,))
    ec.check_ddim(*ec.ddim_f32(c.x_t, c.raw, rows), c, rows, (t,), "fp32 emulation")
    rejected(ec.check_ddim, *ec.ddim_f32(c.x_t, c.raw, rows, swap02=True), c, rows, (t,), "c0 and c2 swapped")


def test_ddim_rejects_clamp_and_last_step_faults():
    c = ec.ddim_case(ec.GEOMS[0])
    rows = ec.ddim_rows((19,))
    xn, x0 = ec.ddim_f32(c.x_t, c.raw, rows)
    open_clamp = torch.where(c.raw == torch.nextafter(torch.tensor(1.0), torch.tensor(2.0)), c.raw, x0)
    rejected(ec.check_ddim, xn, open_clamp, c, rows, (19,), "clamp misses nextafter(1, 2)")
    ulp = xn.clone()
    ulp[0, 0, 0, 1] = torch.nextafter(ulp[0, 0, 0, 1], torch.tensor(4.0))   # inside the bound, not c2 x0
    rejected(ec.check_ddim, ulp, x0, c, rows, (19,), "last step one ulp off")
