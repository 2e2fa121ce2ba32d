"""fp64 truths and a-priori bounds for the per-element arithmetic of the epilogues: GELU and
GELU' (csrc/common.h ``norm_cdf`` / ``gelu_grad_f``), smooth-L1 (``tokgrad_kernel`` in
csrc/embed.hip, ``EPI_HEAD`` mode 3, ``EPI_HEADL``) and the DDIM update (``ddim_step_kernel``,
``EPI_HEAD`` / ``EPI_HEADR`` modes 1 and 4, ``q_sample_kernel``).

**The device.**  Every case sets the fp32 value that enters the epilogue to a chosen number,
bit for bit, so the GEMM in front of it contributes no error and the whole tolerance belongs to
the arithmetic under test.  Two ways, each asserting its *exactness condition* on the tensors
it is given (a probe that breaks it fails on the CPU):

* :func:`onehot_truth` -- one operand has one-hot rows (a single 1, zeros elsewhere), the other
  is finite: every sum has one non-zero product, exact in any order.
* :func:`bias_truth` -- a zero operand, so the accumulator is 0 and the value is ``bias[n]``,
  an arbitrary fp32 number (the head epilogues).

**GELU** (:func:`run_gelu`): ``W`` holds all 65,536 bf16 bit patterns (the 256 non-finite ones
replaced by 0) against a 64 x 64 identity.  ``u`` must be the input pattern to the bit; a
pattern below 2^-126 (zero or denormal) may also come back as a zero of either sign.  The
kernels keep denormals (MFMA products and the bf16 conversion do not flush; measured, see
tests/test_epi_values_gpu.py); a -0 may come back as +0 (the accumulator starts at +0).
``h`` is compared with ``x Phi(x) / (1 - p)``, ``Phi(x) = erfc(-x / sqrt 2) / 2`` in fp64 (no
cancellation in the lower tail), per element within

    ``1/2 ulp_bf16(max(|h|, |truth|)) + PHI_TOL |x| / (1 - p) + 2^-126``.

The first term is the one bf16 rounding of the stored value, the last lets either denormal
behaviour pass.  ``PHI_TOL = 4e-6`` is a derived worst case for ``norm_cdf``: Abramowitz &
Stegun 7.1.28 has |error| <= 3e-7 on erf, 1.5e-7 on Phi.  Its fp32 evaluation computes the
lower tail ``Phi(-|x|) = t^-16 / 2``, ``t = 1 + a1 z + .. + a6 z^6`` by Horner: six FMAs, each
rounding ``t`` by <= 2^-24 relative (every partial result is positive and the later steps
only shrink the earlier errors), so <= 6 x 2^-24 on ``t``, times 16 through the four
squarings = 96 x 2^-24; the squarings' own roundings reach the result with weights 8 + 4 + 2 +
1 = 15; the hardware reciprocal is good to 1 ulp = 2 x 2^-24.  Together <= 113 x 2^-24 = 6.7e-6
relative on a tail of at most 1/2: 3.4e-6, plus 1.5e-7 from the formula, rounded up to 4e-6.
(The upper half ``1 - tail`` adds one rounding of a number below 1: 6e-8, inside the margin.)
An fp32 emulation over every bf16 input (:func:`norm_cdf_f32`) shows 8.6e-7 at worst and
``h`` within 0.9985 of the bound: the half ulp dominates, the 4e-6 hides nothing.  A value
whose truth exceeds the largest bf16 by half an ulp must come back infinite (x / 0.9 at the
top of the range); the comparison treats an infinity as 2^128.  At negative inputs ``h <= 0``.

**GELU'** (:func:`run_dgelu`): ``u`` holds every pattern, the incoming gradient is exactly
``s`` in {1, -2, 0.5, 4} (one-hot ``dy`` rows against constant rows of ``W``); truth
``s (Phi(x) + x phi(x)) / (1 - p)``, bound as above with ``DPHI_TOL |s| / (1 - p)`` in the
middle: ``DPHI_TOL = 5e-6`` = Phi's 4e-6 plus the density path.  That path is
``x exp2(c x^2) / sqrt(2 pi)``: the product ``c x^2`` carries <= 1.5 x 2^-24 relative (two
roundings and the folded constant), which the exponential turns into ``1.5 x 2^-24 x^2 / 2``
relative on phi, i.e. ``x phi`` is off by at most ``0.75 x 2^-24 max|x^3 phi(x)| = 2.5e-8``,
the 1-ulp exponential and two more multiplies add 3 x 2^-24 max|x phi| = 4.3e-8: below 1e-7.
The transposed-operand path (``wt``) must agree with the plain one bit for bit.

**Smooth-L1** (:func:`run_smooth_l1`): the difference ``d`` is set exactly (``pred = 0`` or
the bias against a target chosen so that the fp32 subtraction is exact) to 0, +-2^-20, +-beta/2,
+-beta (1 -+ 2^-10), +-beta, +-2 beta, +-100 and a seeded fill in [-3 beta, 3 beta], for beta
away from 1 (at 1 ``d d / beta``, ``d d beta``, ``d / beta``, ``d beta`` coincide, as do
``|d| - beta / 2`` and ``|d| - 1/2``).  Loss: within ``n 2^-24`` relative of the fp64 sum
(every term is >= 0: the standard bound of an fp32 sum in any order).  Gradient: bit-equal to
``+-bf16(fp32(1 / n))`` where ``|d| >= beta``, within ``1/2 ulp_bf16 + 2^-22`` relative of
``d / (beta n)`` elsewhere (a 2.5-ulp fast division and the rounded ``1 / n``), zero in the cls
rows; for dyadic beta every operation before the bf16 rounding is exact and the three
implementations must agree bit for bit.

**DDIM update** (:func:`run_ddim`): raw predictions 0, +-1, +-nextafter(1, 2), +-nextafter(1,
0), +-3, +-2^-30 and a seeded fill in [-2, 2] through the bias, ``x_t`` seeded normal,
coefficient rows of the first step (t = T - 1), a middle one and the last (``sqrt(1 -
a_{t-k}) = 0``).  ``x0_out`` is ``clamp(raw, -1, 1)`` to the bit; ``x_next`` is within
``8 x 2^-24 (|c2 x0| + |c3 / c1| (|x_t| + |c0 x0|))`` of the fp64 value from the fp32
coefficients (five roundings and a 2.5-ulp fast division, each relative to an intermediate no
larger than that sum); at the last step it is ``fp32(c2) x0`` to the bit, under the identity
row {0, 1, 0, 1} of mode 4 it is ``x_t`` to the bit; ``patches_out`` is the bf16 rounding of
the stored ``x``.  :func:`run_q_sample`: at t = T - 1 (a = 0) the result is ``eps`` to the
bit, at t = 0 within ``4 x 2^-24 (|x0| + |eps|)`` of fp64.

Out of scope: non-finite predictions.  The kernels' ``fminf(fmaxf(v, -1), 1)`` maps NaN to -1
where ``torch.clamp`` keeps NaN; nothing here tests either.

Every runner calls the op through :mod:`ddim_cold_amd.ops` (HIP kernels on a GPU,
:mod:`.reference` on the CPU) and returns the worst observed error / bound ratio; verdicts
are appended to the file named by ``DDIM_COLD_EPI_ERROR_LOG``.  The ``*_f32`` functions
emulate the kernels' fp32 arithmetic on the CPU, with switches for the mutants
tests/test_epi_check_cpu.py shows the bounds to reject.
"""
from __future__ import annotations

import functools
import math
import os
from typing import NamedTuple, Optional, Sequence, Tuple

import torch

from . import reference as ref
from .gemm_check import _bits, assert_exact

LOG_ENV = "DDIM_COLD_EPI_ERROR_LOG"
U32 = 2.0 ** -24          # fp32 unit roundoff
TINY = 2.0 ** -126        # smallest normal fp32 / bf16
PHI_TOL = 4e-6            # norm_cdf in fp32 (derivation above)
DPHI_TOL = 5e-6           # PHI_TOL + the density path of gelu_grad_f
BF16_TOP = 2.0 ** 128     # what an infinite bf16 stands for in a comparison

DROPOUT_PS = (0.0, 0.1)
GELU_SITE, DGELU_SITE = 9, 11
GELU_M, GELU_K, GELU_N = 64, 64, 1024
DGELU_M, DGELU_K, DGELU_NOUT = 256, 256, 64
DGELU_S = (1.0, -2.0, 0.5, 4.0)
GEOMS = ((2, 3, 16, 16, 4), (2, 3, 16, 16, 8))   # (B, C, H, W, patch); D = 64
HEAD_D = 64
BETAS = (0.5, 2.0, 0.3, 1.0)
DDIM_T, DDIM_K = 2000, 20
DDIM_TS = (1999, 999, 19)                         # first step, a middle one, the last
DDIM_MODE4 = ((1999, None), (None, 999), (19, 1999))  # per-sample rows (None: the identity row)
IDENT_ROW = (0.0, 1.0, 0.0, 1.0)

# Abramowitz & Stegun 7.1.28, a6 .. a1 as csrc/common.h writes them
AS_COEF = (4.30638e-5, 2.765672e-4, 1.520143e-4, 9.2705272e-3, 4.22820123e-2, 7.05230784e-2)


def _log(line: str):
    path = os.environ.get(LOG_ENV)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def _ops():
    import ddim_cold_amd.ops as ops
    return ops


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _rng(device, seed: int = 1234, step: int = 5):
    return torch.tensor([seed, step], dtype=torch.int64, device=device)


def _c64(t) -> torch.Tensor:
    return t.detach().double().cpu()


# ----------------------------------------------------------------------------- exactness
def onehot_truth(a, w) -> torch.Tensor:
    """``a @ w.T`` ([M, N] fp32) for ``a`` [M, K] with one-hot rows and finite ``w`` [N, K]:
    output (m, n) is ``w[n][k_m]``, one non-zero product per sum, exact in any order.
    Asserts that condition (every element of ``a`` is 0 or 1, one 1 per row, ``w`` finite)."""
    af = a.detach().float().cpu()
    assert bool(((af == 0) | (af == 1)).all()) and bool((af.sum(1) == 1).all()), \
        "exactness condition violated: every row of the selecting operand must be one-hot"
    assert bool(torch.isfinite(w.float()).all()), "exactness condition violated: non-finite operand (0 x inf)"
    return w.detach().float().cpu()[:, af.argmax(1)].t().contiguous()


def bias_truth(a, w, bias) -> torch.Tensor:
    """The fp32 value entering the epilogue of ``a @ w.T + bias`` with ``a = 0``: ``bias[n]``.
    Asserts the condition (``a`` all zero, ``w`` and ``bias`` finite)."""
    assert int(torch.count_nonzero(a)) == 0, "exactness condition violated: the zero operand has a non-zero element"
    assert bool(torch.isfinite(w.float()).all()) and bool(torch.isfinite(bias).all()), \
        "exactness condition violated: non-finite operand (0 x inf)"
    return bias.detach().float().cpu()


def exact_difference(v, target) -> torch.Tensor:
    """``v - target`` (fp32 tensors) as fp32, asserting the fp32 subtraction is exact."""
    d = _c64(v) - _c64(target)
    assert bool((d.float().double() == d).all()), "exactness condition violated: v - target rounds in fp32"
    return d.float()


# ----------------------------------------------------------------------------- bounds
def all_bf16() -> torch.Tensor:
    """[65536] bf16: element i has bit pattern i; the 256 non-finite patterns are +0."""
    i = torch.arange(65536, dtype=torch.int32)
    x = (i - ((i >= 32768).int() << 16)).to(torch.int16).view(torch.bfloat16).clone()
    x[(i & 0x7F80) == 0x7F80] = 0.0
    assert int(torch.isfinite(x.float()).sum()) == 65536 and int((x.float() == 0).sum()) == 258
    return x


def _edge(t) -> torch.Tensor:
    """fp64 copy with +-inf standing for +-2^128 (the value an overflowing bf16 rounds from)."""
    return torch.nan_to_num(_c64(t), nan=float("nan"), posinf=BF16_TOP, neginf=-BF16_TOP)


def ulp_bf16(a: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 (8 significant bits) at magnitude ``a`` (fp64), 2^-133 below 2^-126
    and that of the top binade from 2^127 up."""
    a = a.abs().clamp(min=TINY, max=BF16_TOP)
    e = (torch.frexp(a)[1] - 1).clamp(max=127)
    return torch.ldexp(torch.ones_like(a), e - 7)


def half_ulp_bf16(got: torch.Tensor, truth: torch.Tensor) -> torch.Tensor:
    return 0.5 * ulp_bf16(torch.maximum(got.abs(), truth.abs()))


def assert_within(got, truth, tol, name: str, mask=None, first: int = 6) -> float:
    """``|got - truth| <= tol`` per element (fp64 ``truth`` / ``tol``; NaN fails; an infinite
    ``got`` counts as +-2^128, and so does a truth beyond it) where ``mask``; returns the
    worst error / tol."""
    g, t = _edge(got).reshape(truth.shape), truth.clamp(-BF16_TOP, BF16_TOP)
    err = (g - t).abs()
    ok = err <= tol
    m = torch.ones_like(ok) if mask is None else mask.reshape(ok.shape).cpu()
    ratio = torch.where(err == 0, torch.zeros_like(err), (err / tol).nan_to_num(nan=float("inf")))
    ratio = torch.where(m, ratio, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = (m & ~ok).nonzero()
    line = f"{name}: {bad.shape[0]} of {int(m.sum())} outside the bound, worst error / bound {worst:.4f}"
    _log(line + ("" if bad.shape[0] == 0 else "  FAILED"))
    if bad.shape[0]:
        lines = [line]
        for idx in bad[:first].tolist():
            i = tuple(idx)
            lines.append(f"  {list(i)} got {float(g[i])!r} want {float(t[i])!r} tol {float(tol[i]):.3e}")
        raise AssertionError("\n".join(lines))
    return worst


def phi64(x: torch.Tensor) -> torch.Tensor:
    """Standard normal CDF in fp64 through erfc: no cancellation in the lower tail."""
    return 0.5 * torch.special.erfc(-x.double() / math.sqrt(2.0))


def pdf64(x: torch.Tensor) -> torch.Tensor:
    x = x.double()
    return torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def _keep(numel: int, site: int, p: float, shape) -> torch.Tensor:
    if p <= 0:
        return torch.ones(shape, dtype=torch.bool)
    return ref.keep_mask(numel, _rng("cpu"), site, p).view(shape)


# ----------------------------------------------------------------------------- fp32 emulation (GELU)
def _f32(v: float) -> torch.Tensor:
    return torch.tensor(v, dtype=torch.float32)


def _fma(a, b, c):
    """fp32 fused multiply-add: the product is exact in fp64."""
    return (a.double() * b.double() + c.double()).float()


def norm_cdf_f32(x: torch.Tensor, coef: Sequence[float] = AS_COEF) -> torch.Tensor:
    """csrc/common.h ``norm_cdf`` operation by operation in fp32 (the reciprocal correctly
    rounded); ``coef`` = (a6, .., a1)."""
    x = x.float()
    z = x.abs() * _f32(0.70710678118654752)
    t = _fma(z, _f32(coef[0]).expand_as(z), _f32(coef[1]))
    for c in tuple(coef[2:]) + (1.0,):
        t = _fma(z, t, _f32(c))
    for _ in range(4):
        t = t * t
    tail = _f32(0.5) / t
    return torch.where(x >= 0, _f32(1.0) - tail, tail)


def _scale_f32(p: float) -> torch.Tensor:
    return _f32(1.0) / (_f32(1.0) - _f32(p)) if p > 0 else _f32(1.0)


def gelu_f32(x: torch.Tensor, p: float = 0.0, keep=None, coef: Sequence[float] = AS_COEF) -> torch.Tensor:
    """The GELU epilogue's ``h`` (bf16) from the fp32 pre-activation ``x``."""
    h = x.float() * norm_cdf_f32(x, coef)
    if p > 0:
        h = torch.where(keep, h * _scale_f32(p), torch.zeros(()))
    return h.to(torch.bfloat16)


def gelu_grad_f32(x: torch.Tensor, log2e: bool = True) -> torch.Tensor:
    """csrc/common.h ``gelu_grad_f`` in fp32; ``log2e=False``: the mutant ``exp2(-x^2 / 2)``."""
    x = x.float()
    c = _f32(-0.72134752044448170 if log2e else -0.5)
    pdf = torch.exp2(c * x * x) * _f32(0.39894228040143268)
    return norm_cdf_f32(x) + x * pdf


def dgelu_f32(dh: torch.Tensor, x: torch.Tensor, p: float = 0.0, keep=None, log2e: bool = True) -> torch.Tensor:
    """The DGELU epilogue's output (bf16) from the fp32 incoming gradient ``dh`` and ``u = x``."""
    v = dh.float()
    if p > 0:
        v = torch.where(keep, v * _scale_f32(p), torch.zeros(()))
    return (v * gelu_grad_f32(x, log2e)).to(torch.bfloat16)


# ----------------------------------------------------------------------------- 1. GELU
class GeluCase(NamedTuple):
    a: torch.Tensor      # [64, 64] bf16 identity
    w: torch.Tensor      # [1024, 64] bf16: every bit pattern
    bias: torch.Tensor   # [1024] fp32 zeros
    v: torch.Tensor      # [64, 1024] fp32: the value entering the epilogue (cpu)


@functools.lru_cache(maxsize=None)
def gelu_case() -> GeluCase:
    w = all_bf16().view(GELU_N, GELU_K)
    a = torch.eye(GELU_M, GELU_K).to(torch.bfloat16)
    return GeluCase(a, w, torch.zeros(GELU_N), onehot_truth(a, w))


@functools.lru_cache(maxsize=None)
def _gelu_truth(p: float):
    x = gelu_case().v.double()
    return x * phi64(x) / (1.0 - p)


def check_gelu_u(u, name: str = "linear_gelu_fwd u") -> Tuple[int, int]:
    """``u`` is the input pattern to the bit; a pattern below 2^-126 may come back as a zero of
    either sign.  Returns (denormal patterns kept, denormal patterns flushed)."""
    v = gelu_case().v
    ub, vb = _bits(u.detach().cpu()), _bits(v.to(torch.bfloat16))
    small = v.abs() < TINY
    same = ub == vb
    ok = same | (small & (u.detach().float().cpu() == 0))
    bad = (~ok).nonzero()
    assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} elements are not the input pattern; first {bad[:4].tolist()}"
    den = small & (v != 0)
    kept, flushed = int((den & same).sum()), int((den & ~same).sum())
    _log(f"{name}: exact; denormal inputs kept {kept}, flushed to zero {flushed}")
    return kept, flushed


def check_gelu_h(h, p: float, name: str = "linear_gelu_fwd h") -> float:
    """``h`` ([64, 1024] bf16) of the all-patterns case against the fp64 truth; the drop set
    against ``keep_mask``; ``h <= 0`` at the 32,640 negative finite inputs."""
    v = gelu_case().v
    x, truth = v.double(), _gelu_truth(p)
    hc = h.detach().cpu().reshape(v.shape)
    keep = _keep(v.numel(), GELU_SITE, p, v.shape)
    assert 0 < int((~keep).sum()) < keep.numel() or p == 0, name + ": degenerate mask"
    nz = int(torch.count_nonzero(hc[~keep]))
    assert nz == 0, f"{name}: {nz} dropped elements are not exactly 0"
    clear = keep & (x.abs() >= 2.0 ** -100) & (x.abs() <= 5.0)   # |truth| far above the bound
    assert int((hc[clear] == 0).sum()) == 0, f"{name}: kept elements read 0 (drop set differs from keep_mask)"
    hd = _edge(hc)
    tol = half_ulp_bf16(hd, truth) + PHI_TOL * x.abs() / (1.0 - p) + TINY
    worst = assert_within(hc, truth, tol, f"{name} p={p}", keep)
    neg = torch.signbit(v)
    assert int(neg.sum()) == 32640
    pos = int((hc.float()[neg] > 0).sum())
    assert pos == 0, f"{name}: positive GELU at {pos} negative inputs"
    return worst


def run_gelu(device, p: float) -> float:
    """``linear_gelu_fwd`` over every finite bf16 input; returns the worst error / bound of ``h``."""
    ops, c = _ops(), gelu_case()
    u, h = ops.linear_gelu_fwd(c.a.to(device), c.w.to(device), c.bias.to(device), _rng(device), GELU_SITE, p)
    check_gelu_u(u)
    return check_gelu_h(h, p)


# ----------------------------------------------------------------------------- 2. GELU'
class DgeluCase(NamedTuple):
    dy: torch.Tensor     # [256, 64] bf16 one-hot rows
    w: torch.Tensor      # [64, 256] bf16: row j is the constant s_j
    u: torch.Tensor      # [256, 256] bf16: every bit pattern
    dh: torch.Tensor     # [256, 256] fp32: the incoming gradient entering the epilogue (cpu)


@functools.lru_cache(maxsize=None)
def dgelu_case() -> DgeluCase:
    m = torch.arange(DGELU_M)
    dy = torch.zeros(DGELU_M, DGELU_NOUT)
    dy[m, m % DGELU_NOUT] = 1.0
    s = torch.tensor(DGELU_S)[torch.arange(DGELU_NOUT) % len(DGELU_S)]
    w = s.unsqueeze(1).expand(DGELU_NOUT, DGELU_K).contiguous().to(torch.bfloat16)
    dy = dy.to(torch.bfloat16)
    dh = onehot_truth(dy, w.t())
    assert torch.equal(dh, s[m % DGELU_NOUT].unsqueeze(1).expand(DGELU_M, DGELU_K))
    return DgeluCase(dy, w, all_bf16().view(DGELU_M, DGELU_K), dh)


def check_dgelu(out, p: float, name: str = "linear_dgrad_gelu") -> float:
    c = dgelu_case()
    x, s = c.u.double(), c.dh.double()
    truth = s * (phi64(x) + x * pdf64(x)) / (1.0 - p)
    oc = out.detach().cpu().reshape(x.shape)
    keep = _keep(x.numel(), DGELU_SITE, p, x.shape)
    assert 0 < int((~keep).sum()) < keep.numel() or p == 0, name + ": degenerate mask"
    nz = int(torch.count_nonzero(oc[~keep]))
    assert nz == 0, f"{name}: {nz} dropped elements are not exactly 0"
    clear = keep & (x > -3.0) & ((x + 0.75).abs() > 0.05)        # |gelu'| >= 2e-3 there
    assert int((oc[clear] == 0).sum()) == 0, f"{name}: kept elements read 0 (drop set differs from keep_mask)"
    tol = half_ulp_bf16(_edge(oc), truth) + DPHI_TOL * s.abs() / (1.0 - p) + TINY
    return assert_within(oc, truth, tol, f"{name} p={p}", keep)


def run_dgelu(device, p: float) -> float:
    """``linear_dgrad_gelu`` from ``W`` and from ``wt = W^T``: both within the bound and
    bit-identical; returns the worst error / bound."""
    ops, c = _ops(), dgelu_case()
    dy, w, u = c.dy.to(device), c.w.to(device), c.u.to(device)
    plain = ops.linear_dgrad_gelu(dy, w, u, _rng(device), DGELU_SITE, p)
    trans = ops.linear_dgrad_gelu(dy, w, u, _rng(device), DGELU_SITE, p, wt=w.t().contiguous())
    worst = max(check_dgelu(plain, p, "linear_dgrad_gelu (W)"), check_dgelu(trans, p, "linear_dgrad_gelu (wt)"))
    assert_exact(trans, plain, f"linear_dgrad_gelu p={p}: wt path against the W path")
    return worst


# ----------------------------------------------------------------------------- 3. smooth-L1
def _head_bias(F: int) -> torch.Tensor:
    """The head bias of the loss cases: multiples of 1/4, zero on every other column (where the
    special differences land exactly)."""
    return torch.tensor([0.0, 0.5, 0.0, -0.25])[torch.arange(F) % 4].contiguous()


def l1_specials(beta: float) -> torch.Tensor:
    """0, +-2^-20, +-beta/2, +-beta(1 - 2^-10), +-beta, +-beta(1 + 2^-10), +-2 beta, +-100 in fp32
    (``beta`` as the fp32 the kernels take)."""
    b = _f32(beta)
    pos = torch.stack([_f32(2.0 ** -20), b * 0.5, b * _f32(1 - 2.0 ** -10), b, b * _f32(1 + 2.0 ** -10), b * 2.0,
                       _f32(100.0)])
    return torch.cat((torch.zeros(1), torch.stack((pos, -pos), 1).reshape(-1)))


class L1Case(NamedTuple):
    geom: Tuple[int, int, int, int, int]
    beta: float
    a: torch.Tensor        # [B*N, 64] bf16 zeros
    w: torch.Tensor        # [F, 64] bf16 (finite, arbitrary: multiplied by zero)
    bias: torch.Tensor     # [F] fp32
    target: torch.Tensor   # [B, C, H, W] fp32: the head's target image
    d: torch.Tensor        # [B, C, H, W] fp32: prediction - target, exact


@functools.lru_cache(maxsize=None)
def l1_case(geom, beta: float) -> L1Case:
    B, C, H, W, p = geom
    g = _gen(100 + p)
    N, F = (H // p) * (W // p) + 1, C * p * p
    n = B * C * H * W
    b32 = float(_f32(beta))
    # the fill: multiples of 2^-12 in [-3 beta, 3 beta] (with biases in quarters every subtraction is exact)
    top = int(3 * b32 * 4096)
    d = torch.randint(-top, top + 1, (n,), generator=g).float() / 4096.0
    sp = l1_specials(beta)
    d[::2] = sp[torch.arange(n // 2) % sp.numel()]
    d = d.view(B, C, H, W)
    a = torch.zeros(B * N, HEAD_D, dtype=torch.bfloat16)
    w = torch.randn(F, HEAD_D, generator=g).to(torch.bfloat16)
    bias = _head_bias(F)
    pred = _ops().rows_to_image(bias_truth(a, w, bias).unsqueeze(0).expand(B * (N - 1), F), B, C, H, W, p)
    target = (pred - d).contiguous()               # rounds where the bias is not 0 ...
    d = exact_difference(pred, target)             # ... so d is what the subtraction gives, exactly
    zero_cols = _ops().rows_to_image((bias == 0).unsqueeze(0).expand(B * (N - 1), F), B, C, H, W, p)
    for v in sp.tolist():                          # every special value survives on a zero-bias column
        assert bool(((d == v) & zero_cols).any()), f"special difference {v!r} is not in the case"
    return L1Case(geom, beta, a, w, bias, target, d)


def l1_truth(d: torch.Tensor, beta: float):
    """(fp64 mean loss, linear-region mask, fp64 gradient d / (beta n)) with ``beta`` as fp32."""
    b = float(_f32(beta))
    dd = d.double()
    ad = dd.abs()
    lin = ad >= b
    loss = torch.where(lin, ad - 0.5 * b, 0.5 * dd * dd / b).sum() / d.numel()
    return float(loss), lin, dd / (b * d.numel())


def check_l1(loss, dtok, case: L1Case, name: str) -> Tuple[float, float]:
    """Loss (a tensor whose fp64 sum is the loss: the scalar or the partials) and the
    token-layout gradient against the truth; returns the worst error / bound of each."""
    B, C, H, W, p = case.geom
    n, N, F = case.d.numel(), (H // p) * (W // p) + 1, C * p * p
    want, lin, gtruth = l1_truth(case.d, case.beta)
    got = float(_c64(loss).sum())
    r_loss = abs(got - want) / (n * U32 * want)
    line = f"{name}: loss {got!r}, fp64 {want!r}, error / bound {r_loss:.4f}"
    _log(line + ("" if r_loss <= 1 else "  FAILED"))
    assert r_loss <= 1, line                       # (NaN fails)
    g = dtok.detach().cpu().view(B, N, F)
    assert int(torch.count_nonzero(g[:, 0])) == 0, f"{name}: cls rows of the gradient are not exactly zero"
    rows = lambda t: _ops().image_to_rows(t, p).reshape(B, N - 1, F)  # noqa: E731
    gp, lin_r, gt_r = g[:, 1:], rows(lin), rows(gtruth)
    edge = torch.where(rows(case.d) > 0, 1.0, -1.0) * (_f32(1.0) / _f32(float(n)))
    bad = ((_bits(gp) != _bits(edge.to(torch.bfloat16))) & lin_r).nonzero()
    assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} gradients with |d| >= beta are not +-bf16(fp32(1/n)); " \
                              f"first {bad[:4].tolist()}"
    tol = half_ulp_bf16(gp.double(), gt_r) + 2.0 ** -22 * gt_r.abs()
    r_grad = assert_within(gp, gt_r, tol, f"{name} gradient, |d| < beta", ~lin_r)
    return r_loss, r_grad


def smooth_l1_f32(d: torch.Tensor, beta: float, geom, mutant: Optional[str] = None):
    """The kernels' smooth-L1 arithmetic in fp32 on the difference ``d`` [B, C, H, W]:
    ``(loss [1], dtok)``.  ``mutant``: ``"dd*beta"``, ``"d*beta"`` or ``"ad-0.5"``."""
    assert mutant in (None, "dd*beta", "d*beta", "ad-0.5")
    B, C, H, W, p = geom
    b, inv_n = _f32(beta), _f32(1.0) / _f32(float(d.numel()))
    ad = d.abs()
    quad = 0.5 * d * d * b if mutant == "dd*beta" else 0.5 * d * d / b
    lin = ad - (_f32(0.5) if mutant == "ad-0.5" else 0.5 * b)
    loss = (torch.where(ad < b, quad, lin).sum() * inv_n).reshape(1)
    gr = torch.clamp(d * b if mutant == "d*beta" else d / b, -1.0, 1.0) * inv_n
    return loss, ref.img_to_tokgrad(gr, (H // p) * (W // p) + 1, p)


def run_smooth_l1(device, geom, beta: float) -> Tuple[float, float]:
    """``smooth_l1_fwd_bwd`` (finished and as partials), ``head_loss`` on an image target and on
    target rows at the same differences; returns the worst error / bound (loss, gradient)."""
    ops, c = _ops(), l1_case(geom, beta)
    B, C, H, W, p = geom
    N = (H // p) * (W // p) + 1
    a, w, bias, target = (t.to(device) for t in (c.a, c.w, c.bias, c.target))
    zero = torch.zeros(B, C, H, W, device=device)
    tag = f"B={B} C={C} {H}x{W} p={p} beta={beta}"
    outs = {}
    loss, outs["smooth_l1_fwd_bwd"] = ops.smooth_l1_fwd_bwd(zero, (-c.d).to(device), N, p, beta)
    worst = [check_l1(loss, outs["smooth_l1_fwd_bwd"], c, f"smooth_l1_fwd_bwd {tag}")]
    parts, dtok = ops.smooth_l1_fwd_bwd(zero, (-c.d).to(device), N, p, beta, finish=False)
    worst.append(check_l1(parts, dtok, c, f"smooth_l1_fwd_bwd partials {tag}"))
    assert_exact(dtok, outs["smooth_l1_fwd_bwd"], f"smooth_l1_fwd_bwd {tag}: gradient with and without finish")
    parts, outs["head_loss"] = ops.head_loss(a, w, bias, target, p, beta)
    worst.append(check_l1(parts, outs["head_loss"], c, f"head_loss {tag}"))
    trows = ops.image_to_rows(target, p).reshape(target.shape).contiguous()
    parts, outs["head_loss rows"] = ops.head_loss(a, w, bias, trows, p, beta, target_rows=True)
    worst.append(check_l1(parts, outs["head_loss rows"], c, f"head_loss target_rows {tag}"))
    if math.frexp(beta)[0] == 0.5:  # dyadic: every operation before the bf16 rounding is exact
        for k in ("head_loss", "head_loss rows"):
            assert_exact(outs[k], outs["smooth_l1_fwd_bwd"], f"{k} against smooth_l1_fwd_bwd, {tag}")
    return max(r[0] for r in worst), max(r[1] for r in worst)


# ----------------------------------------------------------------------------- 4. DDIM update
def ddim_rows(ts: Sequence[Optional[int]]) -> torch.Tensor:
    """fp32 coefficient rows [len(ts), 4] of ``ddim_coefficients(T, t, k)`` (None: the identity row)."""
    from ..diffusion.schedule import ddim_coefficients
    return torch.tensor([IDENT_ROW if t is None else ddim_coefficients(DDIM_T, t, DDIM_K) for t in ts],
                        dtype=torch.float32)


def ddim_specials() -> torch.Tensor:
    one = _f32(1.0)
    pos = torch.stack([one, torch.nextafter(one, _f32(2.0)), torch.nextafter(one, _f32(0.0)), _f32(3.0),
                       _f32(2.0 ** -30)])
    return torch.cat((torch.zeros(1), torch.stack((pos, -pos), 1).reshape(-1)))


class DdimCase(NamedTuple):
    geom: Tuple[int, int, int, int, int]
    a: torch.Tensor      # [B*N, 64] bf16 zeros
    w: torch.Tensor      # [F, 64] bf16
    bias: torch.Tensor   # [F] fp32: the raw prediction of each output column
    raw: torch.Tensor    # [B, C, H, W] fp32: the raw prediction as an image
    x_t: torch.Tensor    # [B, C, H, W] fp32


@functools.lru_cache(maxsize=None)
def ddim_case(geom) -> DdimCase:
    B, C, H, W, p = geom
    g = _gen(200 + p)
    N, F = (H // p) * (W // p) + 1, C * p * p
    sp = ddim_specials()
    bias = torch.rand(F, generator=g) * 4.0 - 2.0
    bias[::2] = sp[torch.arange((F + 1) // 2) % sp.numel()]
    assert F // 2 >= sp.numel()
    a = torch.zeros(B * N, HEAD_D, dtype=torch.bfloat16)
    w = torch.randn(F, HEAD_D, generator=g).to(torch.bfloat16)
    raw = _ops().rows_to_image(bias_truth(a, w, bias).unsqueeze(0).expand(B * (N - 1), F), B, C, H, W, p).contiguous()
    return DdimCase(geom, a, w, bias, raw, torch.randn(B, C, H, W, generator=g))


def check_ddim(x_next, x0_out, case: DdimCase, rows: torch.Tensor, ts: Sequence[Optional[int]], name: str) -> float:
    """``x_next`` / ``x0_out`` [B, C, H, W] of one update with the fp32 coefficient ``rows``
    ([1, 4] or one per sample; ``ts`` names them) against the truth; returns the worst error / bound."""
    B = case.raw.shape[0]
    x0 = case.raw.clamp(-1.0, 1.0)
    assert_exact(x0_out.detach().cpu().reshape(x0.shape), x0, f"{name} x0_out against clamp(raw, -1, 1)")
    cf = rows.double().expand(B, 4) if rows.shape[0] == 1 else rows.double()
    c0, c1, c2, c3 = (cf[:, i].reshape(B, 1, 1, 1) for i in range(4))
    x0d, xtd = x0.double(), case.x_t.double()
    truth = c2 * x0d + c3 * (xtd - c0 * x0d) / c1
    tol = 8 * U32 * ((c2 * x0d).abs() + (c3 / c1).abs() * (xtd.abs() + (c0 * x0d).abs()))
    xn = x_next.detach().cpu().reshape(x0.shape)
    worst = assert_within(xn, truth, tol, f"{name} x_next")
    for b, t in enumerate(ts if len(ts) == B else list(ts) * B):
        if t is None:
            assert_exact(xn[b], case.x_t[b], f"{name} sample {b}: x_next under the identity row against x_t")
        elif t + 1 == DDIM_K:
            assert float(cf[b, 3]) == 0.0
            assert_exact(xn[b], cf[b, 2].float() * x0[b], f"{name} sample {b}: x_next at the last step against c2 x0")
    return worst


def ddim_f32(x_t, raw, rows: torch.Tensor, swap02: bool = False):
    """The kernels' update in fp32 (``rows`` [1 or B, 4]); ``swap02``: the mutant with c0 and c2 swapped."""
    cf = [rows[:, i].reshape(-1, 1, 1, 1) for i in ((2, 1, 0, 3) if swap02 else (0, 1, 2, 3))]
    x0 = raw.clamp(-1.0, 1.0)
    return cf[2] * x0 + cf[3] * ((x_t - cf[0] * x0) / cf[1]), x0


def run_ddim(device, geom) -> float:
    """``ddim_step``, ``head_step_`` and ``head_step_rows_`` modes 1 and 4 on one case; returns
    the worst error / bound of ``x_next``."""
    ops, c = _ops(), ddim_case(geom)
    B, C, H, W, p = geom
    NP, F = (H // p) * (W // p), C * p * p
    a, w, bias, raw, x_t = (t.to(device) for t in (c.a, c.w, c.bias, c.raw, c.x_t))
    tag = f"B={B} C={C} {H}x{W} p={p}"
    worst = 0.0
    runs = [(ops.HEAD_DDIM, (t,)) for t in DDIM_TS] + [(ops.HEAD_DDIM_EACH, ts) for ts in DDIM_MODE4]
    for mode, ts in runs:
        rows = ddim_rows(ts)
        coef = (rows[0] if mode == ops.HEAD_DDIM else rows).contiguous().to(device)
        nm = f"mode {mode} t={ts} {tag}"
        if mode == ops.HEAD_DDIM:
            xn, x0 = ops.ddim_step(x_t, raw, coef)
            worst = max(worst, check_ddim(xn, x0, c, rows, ts, "ddim_step " + nm))
        x, x0o = x_t.clone(), torch.full_like(x_t, float("nan"))
        po = torch.full((B * NP, F), float("nan"), dtype=torch.bfloat16, device=device)
        ops.head_step_(a, w, bias, x, x0o, coef, p, mode, patches_out=po)
        worst = max(worst, check_ddim(x, x0o, c, rows, ts, "head_step_ " + nm))
        assert_exact(po, ref.patchify_bf16(x, p), f"head_step_ {nm} patches_out against bf16(x)")
        xr, x0r = ops.image_to_rows(x_t, p).contiguous(), torch.full((B * NP, F), float("nan"), device=device)
        po = torch.full((B * NP, F), float("nan"), dtype=torch.bfloat16, device=device)
        ops.head_step_rows_(a, w, bias, xr, x0r, coef, B, mode, patches_out=po)
        worst = max(worst, check_ddim(ops.rows_to_image(xr, B, C, H, W, p), ops.rows_to_image(x0r, B, C, H, W, p), c,
                                      rows, ts, "head_step_rows_ " + nm))
        assert_exact(po, xr.to(torch.bfloat16), f"head_step_rows_ {nm} patches_out against bf16(x)")
    return worst


def run_q_sample(device, geom) -> float:
    """``q_sample`` at t = T - 1 (a = 0: the result is ``eps`` to the bit) and at t = 0."""
    ops = _ops()
    B, C, H, W, _ = geom
    g = _gen(300)
    x0, eps = torch.rand(B, C, H, W, generator=g) * 2.0 - 1.0, torch.randn(B, C, H, W, generator=g)
    worst = 0.0
    for ts in ([DDIM_T - 1] * B, [0] * B, [DDIM_T - 1] + [0] * (B - 1)):
        t = torch.tensor(ts, dtype=torch.int64)
        out = ops.q_sample(x0.to(device), t.to(device), eps.to(device), DDIM_T).detach().cpu()
        al = (1.0 - torch.sqrt((t.double() + 1.0) / DDIM_T)).reshape(B, 1, 1, 1)
        truth = al.sqrt() * x0.double() + (1.0 - al).sqrt() * eps.double()
        tol = 4 * U32 * (x0.double().abs() + eps.double().abs())
        worst = max(worst, assert_within(out, truth, tol, f"q_sample t={ts}"))
        for b, tb in enumerate(ts):
            if tb == DDIM_T - 1:
                assert_exact(out[b], eps[b], f"q_sample t=T-1 sample {b} against eps")
    return worst
