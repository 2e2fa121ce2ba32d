"""fp64 truths, a-priori bounds and exact probes for the end of the training step:
``sqnorm_kernel``, ``adamw_kernel``, ``advance_kernel`` (csrc/optim.hip), the embedding-gradient
reductions of csrc/embed_parts.h (behind ``embed_bwd_kernel`` and as extra workgroups of the
weight-gradient launch) and the bf16 gradient wire (``wire_pack`` / ``wire_unpack``,
csrc/comm_wire.hip).

Every runner calls the op through :mod:`ddim_cold_amd.ops` (HIP kernels on a GPU, the fallbacks
and :mod:`.reference` on the CPU) and returns the worst observed error / bound ratio (0.0 for a
comparison on raw bits); verdicts are appended to the file named by ``DDIM_COLD_OPT_ERROR_LOG``.
No bound below is taken from what a kernel returns: each is counted from the roundings of the
arithmetic as written in the kernel, or it is an exact comparison whose exactness condition is
asserted on the inputs (a probe that breaks it fails on the CPU).

**1. AdamW** (:func:`run_adamw`).  The truth (:func:`adamw_truth`) is one step in fp64 from the
fp32 inputs, the fp32 ``hyper`` values as stored, ``grad_scale``, ``step`` and the fp64 sum of
the partials, written as the kernel writes it: ``coef = grad_scale min(1, max_norm / (sqrt(sq) +
1e-6f))``, ``t = step[0] + 1``, decoupled decay before the update, ``eps`` outside the bias
correction, the cosine rate from ``step[1]`` (as ``eta_min + (base_lr - eta_min) cos^2(pi s / 2
tmax)``, which does not cancel in fp64).  *Exactness condition* (:func:`exact_partials`): the
partial buffer holds at most four non-zero slots, each a power of two, within 2^20 of each
other, so every partial sum of any order is an fp32 number and the norm adds no error.

With u = 2^-24, a correctly rounded fp32 operation is off by <= u relative; a division or a
square root is taken as <= 2.5 ulp = 5 u (the fast forms; the correctly rounded ones do
better), ``cosf`` as <= 2 ulp = 4 u of a value <= 1.  The scalar prefactors multiply into every
element, so their errors are counted first (relative, in u):

* ``coef`` (``max_norm > 0``): sqrt 5, the sum with 1e-6f 1, the division 5, the product with
  ``grad_scale`` 1: **e_coef = 12** (0 without a clip: ``grad_scale`` itself).
* ``bc1``, ``bc2``: computed in fp64 and rounded once: 1 each.
  ``inv_sbc2 = 1 / sqrtf(bc2)``: 1/2 + 5 + 5: **e_isb = 11**.
* ``lr`` (``tmax > 0``): the angle ``a = pi_f s / tmax`` carries the rounded constant 1, the
  product 1 and the division 5: 7 u relative, which the cosine turns into ``7 u a |sin a|``;
  ``cosf`` adds 4 u, the sum ``1 + cos`` another ``u (1 + cos)``.  With ``w = (1 + cos a) / 2``
  the weight's *absolute* error is ``A_w = (7 a |sin a| + 4 + (1 + cos a)) u / 2``; the
  amplitude ``base_lr - eta_min`` and the product carry 2, the final sum 1 of ``lr``:

      ``E_lr = |base_lr - eta_min| (A_w + 2 u w) + u lr``        (absolute)

  and **e_lr = E_lr / lr**.  Near the end of the schedule ``w -> 0`` and ``1 + cosf`` cancels:
  ``E_lr`` stays at about ``2 u base_lr`` while ``lr -> eta_min``, so with ``eta_min > 0`` the
  *relative* error of the rate, and of the update, is hundreds of u (600 u at the late row
  below).  That is a property of forming the weight in fp32, and the bound gives it this term of
  its own instead of a larger global multiple: at every other row e_lr is below 30 (28 in the
  middle of a schedule, where ``a |sin a|`` peaks).
  Without a schedule (``tmax = 0``) ``lr = base_lr`` and e_lr = 0.
* ``step_size = lr / bc1``: **e_ss = e_lr + 1 + 5**.
* ``decay = 1 - lr wd``: the product 1 + e_lr relative to ``lr wd``, the difference 1:
  **e_decay = (u + lr wd (e_lr + u)) / decay**.

Per element, with ``S = |b1 m| + |(1 - b1) g coef|`` (the terms of ``m'``, which may cancel):

* ``gi = g coef``: e_coef + 1.
* ``m' = b1 m + (1 - b1) gi``: first term 1, second ``1 - b1`` 1, its product 1, ``gi``, and the
  sum 1 of ``|m'| <= S``: ``|dm| <= (e_coef + 4) u S``: **M_m = e_coef + 4**  (16, or 4).
* ``v' = b2 v + ((1 - b2) gi) gi``: every term is >= 0, so the scale is the true ``v'``: second
  term 1 + 1 + 1 + 2 (e_coef + 1), first term 1, the sum 1: **M_v = 2 e_coef + 6**  (30, or 6).
* ``denom = sqrtf(v') inv_sbc2 + eps`` (all >= 0): M_v / 2 + 5, e_isb + 1, the sum 1:
  **e_den = M_v / 2 + 18**.
* ``upd = step_size m' / denom``: ``U = step_size S / denom`` bounds it; its error is
  ``U (M_m + e_ss + 1 + 5 + e_den)``.
* ``p' = p decay - upd``: ``|p| (e_decay + 1)``, the above, and the difference 1 of
  ``|p'| <= |p| + U``:

      ``|dp| <= u [ (e_decay / u + 2) |p| + (M_m + M_v / 2 + 31 + e_lr / u) U ]``

  (``e_ss + 6 + e_den + 1 = e_lr + M_v / 2 + 31``: 62 + e_lr with a clip, 38 + e_lr without).
  FMA contraction only removes roundings.  The bounds are first order; a factor 1 + 2^-10 covers the products of two errors (the largest,
  e_lr, is 4e-5) and 2^-126 lets a flushed denormal pass.

The project's own CPU step stays within 2.0 u (``m``), 3.1 u (``v``) and 2.6 u (``p``) of the truth
against these scales, so the derived multiples (16, 30, 62 and more) sit above the reference,
and three orders of magnitude under the mutants: :func:`adamw_f32` emulates the kernel in fp32 on
the CPU with switches for ``eps`` inside the bias correction, ``step[0]`` and ``step[1]``
swapped, the cosine amplitude ``base_lr``, ``grad_scale`` applied twice, the decay applied after
the update, and coupled (L2) decay.  Each is rejected at the hard row; the first five pass
``rtol=1e-5, atol=1e-6`` at the suite's only row (tests/test_opt_check_cpu.py), which is why the
other rows exist.

``pb`` is ``bf16(p)`` of the kernel's own ``p`` to the bit (round to nearest even);
``lazy_decay`` is within ``(e_decay + u)`` relative of ``lazy_decay (1 - lr wd)`` (``decay`` and
one product).  The lazy range itself is filled with NaN (``g``, ``m``, ``v``) and must come back
bit-identical: the contract is no loads and no stores.  (On pointers that are not 16-byte
aligned the kernel has no lazy range -- ``adamw_launch`` drops it with the vector path -- so
the lazy mode runs on aligned views only.)

**2. Partials** (:func:`run_partials`, :func:`run_skip`, :func:`run_advance`): the only
non-zero slot is the *last* one of the buffer, a power of two: a sum that stops early sees
``sq = 0`` and leaves the clip coefficient at ``grad_scale``, far outside the bounds above.  An
``inf`` or a NaN there must skip the step: ``p``, ``m``, ``v``, ``lazy_decay`` to the bit, ``g``
zeroed below ``zero_hi`` only, ``step[0]`` held while ``step[1]`` and ``rng[1]`` advance.

**3. sqnorm** (:func:`run_sqnorm`, :func:`run_sqnorm_positions`): gradients in {0, +-1, +-2,
+-3}, ``scale`` 3 or 1/2 (``scale^2`` exact), with ``max(1, scale^2) sum g^2 < 2^24`` asserted:
every partial of any grouping is then an integer (or a multiple of 1/4) below 2^24, exact in
fp32, and the fp64 sum of the partials must *equal* the int64 truth.  The partial buffer starts
as NaN, so a slot left unwritten fails too.  The lazy range of ``g`` is NaN: no loads.

**4. embed_bwd** (:func:`run_embed`, :func:`run_embed_wgrad`): ``g`` integer in [-4, 4],
dropout 0 or 1/2 (threshold 32768 and a rescale of exactly 2, both asserted), integer prefill,
every sum below 2^24 (asserted on the truth): all fp32 sums are exact in any order and the
three gradients must equal the int64 truth bit for bit; ``gpatch`` is the exact bf16 of the
masked, doubled values.  In the weight-gradient launch each part workgroup writes the sum of
squares of what it wrote: non-negative terms, so the fp64 sum of those slots is within ``count
2^-24`` relative of the squares of the written values (the standard bound of an fp32 sum in any
order).  That launch takes ``B <= 256`` (one part-B pass) and ``owners <= B``: the shapes with
257 and 300 samples run through the stand-alone launch only.

**5. bf16 wire** (:func:`run_wire_pack`, :func:`run_wire_unpack`): every high half crossed with
the low halves 0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF (below, at and above every tie, both
parities), against ``src.to(torch.bfloat16)`` on the CPU, bit for bit wherever the input is not
NaN, NaN where it is; every bf16 pattern must unpack to ``bits << 16``.
"""
from __future__ import annotations

import math
import os
from typing import Dict, NamedTuple, Optional, Sequence, Tuple

import torch

from . import reference as ref
from .gemm_check import _bits, assert_exact, canary

LOG_ENV = "DDIM_COLD_OPT_ERROR_LOG"
U32 = 2.0 ** -24
TINY = 2.0 ** -126
SECOND_ORDER = 1.0 + 2.0 ** -10
DIV_U, SQRT_U, COS_U = 5.0, 5.0, 4.0   # 2.5 ulp, 2.5 ulp, 2 ulp in units of u

SUITE_HYPER = (3e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 10.0, 0.0)
ADAMW_SIZES = (4, 5, 1027, 100_003)
ADAMW_BIG = 2_098_181               # past the grid cap of 2048 x 256 vectors: a second trip
ADAMW_MODES = ("plain", "lazy", "ema")
MUTANTS = ("eps_in_bc", "swap_steps", "cos_amp", "scale_twice", "decay_after")
L2 = "l2"


class Row(NamedTuple):
    hyper: Tuple[float, ...]
    grad_scale: float
    step: Tuple[int, int]
    sq: float            # the squared norm the partials hold (a power of two)
    fresh: bool = False  # m = v = 0


ROWS: Dict[str, Row] = {
    # the only row the suite had: eta_min = 0, grad_scale = 1, step[0] == step[1]
    "suite": Row(SUITE_HYPER, 1.0, (3, 3), 4.0),
    # every hyper-parameter away from where two formulas coincide: large eps (its place
    # matters), eta_min > 0 (the amplitude), grad_scale != 1 (applied once), step[0] !=
    # step[1] (which counter feeds what), a strong decay (its order), norm 2 > max_norm
    "hard": Row((3e-3, 0.8, 0.99, 1e-3, 0.3, 0.5, 64.0, 1e-3), 0.25, (7, 10), 4.0),
    # the two branches the suite never took: no clip, no schedule
    "noclip_nosched": Row((3e-3, 0.9, 0.999, 1e-8, 0.05, 0.0, 0.0, 0.0), 0.5, (5, 9), 4.0),
    # norm 1/2 below max_norm = 1: the clip is min(1, .) = 1 and coef is grad_scale alone
    "below_max_norm": Row(SUITE_HYPER, 0.25, (3, 6), 0.25),
    # seven steps before the end of a 1e5-step schedule: 1 + cosf cancels, lr ~ eta_min
    "late": Row((3e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 1e5, 1e-5), 1.0, (99_993, 99_993), 4.0),
    # the first step: t = 1, bias corrections 1 - b, zero moments
    "first": Row(SUITE_HYPER, 1.0, (0, 0), 4.0, fresh=True),
}


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


def offset_view(t: torch.Tensor, off: int, device) -> torch.Tensor:
    """A copy of the 1-D ``t`` on ``device`` that starts ``off`` elements into its buffer
    (off = 1: no 16-byte alignment)."""
    buf = torch.empty(t.numel() + off, dtype=t.dtype, device=device)
    buf[off:].copy_(t)
    return buf[off:]


def within(got, truth, tol, name: str, mask=None, first: int = 4) -> float:
    """``|got - truth| <= tol`` per element (fp64 truth / tol; NaN fails) where ``mask``;
    returns the worst error / tol and logs the verdict."""
    g = _c64(got).reshape(truth.shape)
    err = (g - truth).abs()
    m = torch.ones_like(err, dtype=torch.bool) if mask is None else mask.reshape(err.shape)
    ratio = torch.where(err == 0, torch.zeros_like(err), (err / tol).nan_to_num(nan=float("inf")))
    ratio = torch.where(m, ratio, torch.zeros_like(err))
    worst = float(ratio.max()) if ratio.numel() else 0.0
    bad = (m & ~(err <= tol)).nonzero()
    line = f"{name}: {bad.shape[0]} of {int(m.sum())} outside the bound, worst error / bound {worst:.4f}"
    _log(line + ("" if bad.shape[0] == 0 else "  FAILED"))
    if bad.shape[0]:
        lines = [line]
        for idx in bad[:first].tolist():
            i = tuple(idx)
            lines.append(f"  {list(i)} got {float(g[i])!r} want {float(truth[i])!r} tol {float(tol[i]):.3e}")
        raise AssertionError("\n".join(lines))
    return worst


def exact(got, truth, name: str):
    assert_exact(got.detach().cpu(), truth.detach().cpu(), name)
    _log(f"{name}: exact")


# ----------------------------------------------------------------------------- 1. AdamW
def exact_partials(sq: torch.Tensor) -> float:
    """The fp64 sum of the partial buffer, asserting that its fp32 sum is exact in any order:
    at most four non-zero slots, powers of two, within 2^20 of each other."""
    s = _c64(sq)
    nz = s[s != 0]
    assert nz.numel() <= 4 and bool((nz > 0).all()) and bool(torch.isfinite(nz).all()), \
        "exactness condition violated: more than four non-zero partials, or a negative / non-finite one"
    if nz.numel():
        assert bool((torch.frexp(nz)[0] == 0.5).all()), "exactness condition violated: a partial is no power of two"
        assert float(nz.max() / nz.min()) <= 2.0 ** 20, "exactness condition violated: partials too far apart"
    return float(s.sum())


class Scalars(NamedTuple):
    coef: float
    lr: float
    bc1: float
    bc2: float
    decay: float
    # relative error bounds of the fp32 prefactors, in units of u
    e_coef: float
    e_lr: float
    e_decay: float


def adamw_scalars(hyper: torch.Tensor, step: Sequence[int], sq: float, grad_scale: float) -> Scalars:
    """The step's scalar prefactors in fp64 from the fp32 ``hyper`` as stored, with the error
    bounds of their fp32 evaluation (docstring above)."""
    base_lr, b1, b2, eps, wd, max_norm, tmax, eta_min = (float(x) for x in _c64(hyper.float())[:8])
    coef, e_coef = float(grad_scale), 0.0
    if max_norm > 0:
        coef *= min(1.0, max_norm / (math.sqrt(sq) + float(torch.tensor(1e-6, dtype=torch.float32))))
        e_coef = SQRT_U + 1 + DIV_U + 1
    t = int(step[0]) + 1
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    lr, e_lr = base_lr, 0.0
    if tmax > 0:
        a = math.pi * int(step[1]) / tmax
        w = math.cos(0.5 * a) ** 2                   # (1 + cos a) / 2 without the cancellation
        lr = eta_min + (base_lr - eta_min) * w
        a_w = 0.5 * ((1 + 1 + DIV_U) * a * abs(math.sin(a)) + COS_U + 2.0 * w)
        e_lr = (abs(base_lr - eta_min) * (a_w + 2.0 * w) + lr) / lr
    decay = 1.0 - lr * wd
    assert lr > 0 and 0.5 < decay <= 1.0 and 0 < bc1 <= 1 and 0 < bc2 <= 1
    e_decay = (1.0 + lr * wd * (e_lr + 1.0)) / decay
    return Scalars(coef, lr, bc1, bc2, decay, e_coef, e_lr, e_decay)


class Truth(NamedTuple):
    p: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    tol_p: torch.Tensor
    tol_m: torch.Tensor
    tol_v: torch.Tensor
    sc: Scalars


def adamw_truth(p, g, m, v, hyper, step, sq: float, grad_scale: float) -> Truth:
    """One AdamW step in fp64 as csrc/optim.hip writes it, with the per-element bounds."""
    sc = adamw_scalars(hyper, step, sq, grad_scale)
    _, b1, b2, eps = (float(x) for x in _c64(hyper.float())[:4])
    p, g, m, v = _c64(p), _c64(g), _c64(m), _c64(v)
    gi = g * sc.coef
    t_m1, t_m2 = b1 * m, (1.0 - b1) * gi
    m2 = t_m1 + t_m2
    v2 = b2 * v + (1.0 - b2) * gi * gi
    denom = v2.sqrt() / math.sqrt(sc.bc2) + eps
    step_size = sc.lr / sc.bc1
    p2 = p * sc.decay - step_size * m2 / denom
    S = t_m1.abs() + t_m2.abs()
    U = step_size * S / denom
    M_m, M_v = sc.e_coef + 4.0, 2.0 * sc.e_coef + 6.0
    K_p = M_m + 0.5 * M_v + 31.0 + sc.e_lr
    k = U32 * SECOND_ORDER
    return Truth(p2, m2, v2,
                 k * ((sc.e_decay + 2.0) * p.abs() + K_p * U) + TINY,
                 k * M_m * S + TINY, k * M_v * v2 + TINY, sc)


def _f(x) -> torch.Tensor:
    return torch.as_tensor(x, dtype=torch.float32)


def adamw_f32(p, g, m, v, hyper, step, sq: float, grad_scale: float, mutant: Optional[str] = None):
    """The kernel's step operation by operation in fp32 on the CPU: ``(p', m', v')``.
    ``mutant``: one of :data:`MUTANTS` or :data:`L2` (coupled weight decay)."""
    assert mutant is None or mutant in MUTANTS or mutant == L2
    h = hyper.detach().float().cpu()
    base_lr, b1, b2, eps, wd, max_norm, tmax, eta_min = (h[i] for i in range(8))
    p, g, m, v = (x.detach().float().cpu().clone() for x in (p, g, m, v))
    one = _f(1.0)
    coef = _f(grad_scale)
    if mutant == "scale_twice":
        coef = coef * _f(grad_scale)
    if float(max_norm) > 0:
        coef = coef * torch.minimum(one, max_norm / (torch.sqrt(_f(sq)) + _f(1e-6)))
    s_adam, s_sched = (step[1], step[0]) if mutant == "swap_steps" else (step[0], step[1])
    t = float(int(s_adam) + 1)
    bc1 = _f(1.0 - float(b1.double()) ** t)
    bc2 = _f(1.0 - float(b2.double()) ** t)
    lr = base_lr
    if float(tmax) > 0:
        amp = base_lr if mutant == "cos_amp" else base_lr - eta_min
        lr = eta_min + amp * _f(0.5) * (one + torch.cos(_f(3.14159265358979) * _f(float(int(s_sched))) / tmax))
    step_size = lr / bc1
    inv_sbc2 = one / torch.sqrt(bc2)
    decay = one - lr * wd
    gi = g * coef
    if mutant == L2:
        gi = gi + wd * p
    elif mutant != "decay_after":
        p = p * decay
    m = b1 * m + (one - b1) * gi
    v = b2 * v + (one - b2) * gi * gi
    den = (torch.sqrt(v) + eps) * inv_sbc2 if mutant == "eps_in_bc" else torch.sqrt(v) * inv_sbc2 + eps
    p = p - step_size * m / den
    if mutant == "decay_after":
        p = p * decay
    return p, m, v


class Arenas(NamedTuple):
    p: torch.Tensor
    g: torch.Tensor
    m: torch.Tensor
    v: torch.Tensor
    e: torch.Tensor


def arenas(n: int, fresh: bool = False, seed: int = 0) -> Arenas:
    """Random p / g / m / v / ema on the CPU, drawn as the suite's optimizer tests draw them:
    p, g, e ~ N(0, 1), m ~ 0.01 N(0, 1), v ~ 1e-3 U(0, 1); ``fresh``: m = v = 0."""
    gen = _gen(seed)
    p, e, g = (torch.randn(n, generator=gen) for _ in range(3))
    m = torch.randn(n, generator=gen) * 0.01
    v = torch.rand(n, generator=gen) * 1e-3
    if fresh:
        m, v = torch.zeros(n), torch.zeros(n)
    return Arenas(p, g, m, v, e)


def partials(device, nparts: int, slots: Dict[int, float]) -> torch.Tensor:
    sq = torch.zeros(nparts)
    for i, val in slots.items():
        sq[i] = val
    return sq.to(device)


def lazy_range(n: int) -> Tuple[int, int]:
    """A whole-vector range inside the arena: a third of the way in, a quarter long (the one
    vector there is at n < 8)."""
    n4 = n // 4
    lo = n4 // 3
    return 4 * lo, 4 * (lo + max(1, min(n4 // 4, n4 - lo)))


def check_adamw(got: Dict[str, torch.Tensor], tr: Truth, name: str, mask=None) -> Tuple[float, float, float]:
    """``got`` = {p, m, v} against the truth; returns the worst error / bound of (m, v, p)."""
    return (within(got["m"], tr.m, tr.tol_m, name + " m", mask), within(got["v"], tr.v, tr.tol_v, name + " v", mask),
            within(got["p"], tr.p, tr.tol_p, name + " p", mask))


def run_adamw(device, row: str, mode: str, n: int, off: int = 0, sq_slots: Optional[Dict[int, float]] = None,
              nparts: Optional[int] = None) -> Tuple[float, float, float]:
    """One step of ``ops.adamw_step`` at hyper-parameter row ``row`` over ``n`` elements that
    start ``off`` elements into their buffers, in ``mode`` plain / lazy / ema; returns the
    worst error / bound of (m, v, p)."""
    ops, r = _ops(), ROWS[row]
    assert mode in ADAMW_MODES and not (mode == "lazy" and off)
    a = arenas(n, r.fresh, seed=n)
    lo, hi = lazy_range(n) if mode == "lazy" else (0, 0)
    if hi > lo:  # no loads: whatever lies there must not matter
        for t in (a.g, a.m, a.v):
            t[lo:hi] = float("nan")
    nparts = ops.SQ_PARTS if nparts is None else nparts
    sq = partials(device, nparts, {17: r.sq} if sq_slots is None else sq_slots)
    sqv = exact_partials(sq)
    hyper = torch.tensor(r.hyper, dtype=torch.float32)
    step = torch.tensor(r.step, dtype=torch.int64)
    d = {k: offset_view(getattr(a, k), off, device) for k in ("p", "g", "m", "v", "e")}
    pb = offset_view(torch.zeros(n, dtype=torch.bfloat16), off, device)
    ld = torch.tensor([0.75], device=device)
    kw = {}
    if mode == "lazy":
        kw = dict(lazy=(lo, hi), lazy_decay=ld)
    elif mode == "ema":
        kw = dict(ema=d["e"], ema_decay=0.9, ema_warmup=False)
    ops.adamw_step(d["p"], d["g"], d["m"], d["v"], pb, sq, step.to(device), hyper.to(device), r.grad_scale, **kw)
    tr = adamw_truth(a.p, a.g, a.m, a.v, hyper, r.step, sqv, r.grad_scale)
    name = f"adamw_step [{torch.device(device).type}] row={row} mode={mode} n={n} off={off}"
    live = torch.ones(n, dtype=torch.bool)
    live[lo:hi] = False
    worst = check_adamw(d, tr, name, live)
    exact(pb[live.to(pb.device)], d["p"][live.to(pb.device)].to(torch.bfloat16), name + " pb against bf16(p)")
    gz = d["g"].detach().cpu()
    assert int(torch.count_nonzero(gz[live])) == 0, name + ": gradients not zeroed"
    if mode == "lazy":
        for k in ("p", "g", "m", "v"):
            exact(d[k][lo:hi], getattr(a, k)[lo:hi], f"{name} {k} inside the lazy range")
        assert int(pb[lo:hi].float().abs().sum()) == 0, name + ": bf16 shadow written inside the lazy range"
        want = torch.tensor([0.75], dtype=torch.float64) * tr.sc.decay
        within(ld, want, U32 * SECOND_ORDER * (tr.sc.e_decay + 1.0) * want, name + " lazy_decay")
    else:
        exact(ld, torch.tensor([0.75]), name + " lazy_decay untouched")
    return worst


# ----------------------------------------------------------------------------- 2. partials
def run_partials(device, nparts: int, n: int = 1027) -> Tuple[float, float, float]:
    """The only non-zero partial in the last slot of a buffer of ``nparts``: the hard row's
    step must match the truth (a sum that stops early leaves the clip at ``grad_scale``)."""
    return run_adamw(device, "hard", "plain", n, 0, sq_slots={nparts - 1: 4.0}, nparts=nparts)


def run_skip(device, nparts: int, bad: float, n: int = 100_003, zero_hi: int = 40_964):
    """A non-finite value in the last slot only: the step is skipped.  ``p``, ``m``, ``v`` and
    ``lazy_decay`` come back to the bit, ``g`` is zeroed below ``zero_hi`` and untouched above
    and inside the lazy range; then the counters: ``step[0]`` held, ``step[1]`` and ``rng[1]``
    advanced, ``rng[0]`` untouched."""
    ops = _ops()
    assert not math.isfinite(bad) and zero_hi % 4 == 0
    a = arenas(n, seed=7)
    lo, hi = 1024, 2048
    sq = partials(device, nparts, {nparts - 1: bad})
    hyper = torch.tensor(ROWS["hard"].hyper, dtype=torch.float32, device=device)
    step = torch.tensor([7, 10], dtype=torch.int64, device=device)
    rng = _rng(device)
    d = {k: getattr(a, k).to(device) for k in ("p", "g", "m", "v")}
    ld = torch.tensor([0.75], device=device)
    ops.adamw_step(d["p"], d["g"], d["m"], d["v"], None, sq, step, hyper, 0.25, zero_hi=zero_hi, lazy=(lo, hi),
                   lazy_decay=ld)
    name = f"adamw_step [{torch.device(device).type}] skipped step ({bad} in slot {nparts - 1} of {nparts})"
    for k in ("p", "m", "v"):
        exact(d[k], getattr(a, k), f"{name} {k}")
    exact(ld, torch.tensor([0.75]), name + " lazy_decay")
    want_g = a.g.clone()
    want_g[:lo] = 0.0
    want_g[hi:zero_hi] = 0.0
    exact(d["g"], want_g, name + " g zeroed below zero_hi only")
    ops.advance_counters(step, rng, sq)
    assert step.tolist() == [7, 11] and rng.tolist() == [1234, 6], f"{name}: counters {step.tolist()} {rng.tolist()}"
    _log(f"{name}: counters exact")


def run_advance(device, nparts: int):
    """Finite partials, and no partials at all: all three counters advance."""
    ops = _ops()
    for sq in (partials(device, nparts, {nparts - 1: 4.0}), None):
        step = torch.tensor([7, 10], dtype=torch.int64, device=device)
        rng = _rng(device)
        ops.advance_counters(step, rng, sq)
        assert step.tolist() == [8, 11] and rng.tolist() == [1234, 6], f"advance_counters: {step.tolist()} {rng.tolist()}"
    _log(f"advance_counters [{torch.device(device).type}] nparts={nparts}: exact")


# ----------------------------------------------------------------------------- 3. sqnorm
SQNORM_SCALES = (3.0, 0.5)
SQNORM_SMALL = (1, 3, 4, 7, 1027)


def sqnorm_sizes(nparts_min: int) -> Tuple[int, ...]:
    """The small sizes, one between ``nparts 256 4`` and four times that (one trip through
    the plain loop with a ragged end) and one above ``4 nparts 256 4 + 3`` (the unrolled loop,
    the remainder loop and the scalar tail), for the smallest partial buffer."""
    trip = nparts_min * 256 * 4
    return SQNORM_SMALL + (2 * trip + 4 * 333 + 2, 4 * trip + 4 * 1000 + 3)


def int_gradient(n: int, seed: int = 0) -> torch.Tensor:
    """fp32 values in {0, +-1, +-2, +-3}, thinned so that 9 sum g^2 stays below 2^24."""
    gen = _gen(seed)
    g = torch.randint(-3, 4, (n,), generator=gen)
    if n > 2 ** 18:
        g = g * (torch.rand(n, generator=gen) < 2.0 ** 18 / n)
    return g.float()


def sqnorm_truth(g: torch.Tensor, scale: float, lazy: Optional[Tuple[int, int]] = None) -> float:
    """``scale^2 sum g^2`` outside the lazy range from int64, asserting the exactness condition."""
    lo, hi = lazy if lazy is not None else (0, 0)
    live = torch.ones(g.numel(), dtype=torch.bool)
    live[lo:hi] = False
    gl = g.detach().cpu()[live]
    gi = gl.to(torch.int64)
    assert bool((gi.float() == gl).all()) and int(gi.abs().max() if gi.numel() else 0) <= 3, \
        "exactness condition violated: gradients must be integers in [-3, 3]"
    s2 = scale * scale
    assert s2 in (0.25, 1.0, 9.0), "exactness condition violated: scale^2 must be exact"
    total = int((gi * gi).sum())
    assert total * max(1.0, s2) < 2 ** 24, "exactness condition violated: scale^2 sum g^2 >= 2^24"
    return total * s2


def sqnorm_lazy_ranges(n: int, nparts: int) -> Dict[str, Tuple[int, int]]:
    """Ranges at element 0, ending at ``n // 4 * 4``, straddling the first trip boundary of the
    strided loop (or the middle of a short arena), and one vector long."""
    n4 = n // 4
    if n4 < 8:
        return {}
    st = nparts * 256
    mid = st if n4 > st + 64 else n4 // 2
    half = min(24, mid - 1, n4 - mid - 1)
    return {"at 0": (0, 4 * min(37, n4 // 2)), "to the end": (4 * (n4 - min(37, n4 // 2)), 4 * n4),
            "across a trip": (4 * (mid - half), 4 * (mid + half)), "one vector": (4 * mid, 4 * mid + 4)}


def _sqnorm_once(device, g_dev, nparts: int, scale: float, lazy, want: float, name: str):
    out = torch.full((nparts,), float("nan"), device=device)
    _ops().sqnorm(g_dev, out, scale, lazy=lazy)
    got = float(_c64(out).sum())
    ok = got == want
    _log(f"{name}: {'exact' if ok else f'got {got!r} want {want!r}  FAILED'}")
    assert ok, f"{name}: sum of the partials {got!r}, int64 truth {want!r}"


def run_sqnorm(device, n: int, nparts: int, off: int = 0) -> float:
    """``ops.sqnorm`` on an integer gradient of ``n`` elements (``off`` elements into its
    buffer) into ``nparts`` partials, at both scales, plain and with every lazy range (NaN
    inside): the fp64 sum of the partials equals the int64 truth."""
    g = int_gradient(n, seed=n)
    dev = torch.device(device).type
    for scale in SQNORM_SCALES:
        _sqnorm_once(device, offset_view(g, off, device), nparts, scale, None, sqnorm_truth(g, scale),
                     f"sqnorm [{dev}] n={n} parts={nparts} off={off} scale={scale}")
    for what, (lo, hi) in sqnorm_lazy_ranges(n, nparts).items():
        gl = g.clone()
        gl[lo:hi] = float("nan")
        _sqnorm_once(device, offset_view(gl, off, device), nparts, 3.0, (lo, hi), sqnorm_truth(gl, 3.0, (lo, hi)),
                     f"sqnorm [{dev}] n={n} parts={nparts} off={off} lazy {what} [{lo}, {hi})")
    return 0.0


def sqnorm_positions(n: int, nparts: int, lazy: Optional[Tuple[int, int]]) -> Tuple[int, ...]:
    """Element positions at the seams: both ends of the vector before the lazy range and of
    the one after it, the last vector of the first trip and the first of the second (through
    the lazy map), the first and the last vector, and every tail element."""
    n4 = n // 4
    lo4, len4 = (lazy[0] // 4, (lazy[1] - lazy[0]) // 4) if lazy is not None else (0, 0)
    vecs = {0, n4 - 1}
    if lazy is not None:
        vecs |= {lo4 - 1, lo4 + len4}
    for j in (nparts * 256 - 1, nparts * 256, 4 * nparts * 256 - 1, 4 * nparts * 256):
        if 0 <= j < n4 - len4:
            vecs.add(j if j < lo4 else j + len4)
    pos = set(range(n4 * 4, n))
    for vq in vecs:
        if 0 <= vq < n4 and not (lo4 <= vq < lo4 + len4):
            pos |= {4 * vq, 4 * vq + 3}
    return tuple(sorted(pos))


def run_sqnorm_positions(device, n: int, nparts: int, off: int = 0, with_lazy: bool = True) -> float:
    """A single +-1 in an otherwise zero gradient at each seam position: the sum is ``scale^2``."""
    lazy = sqnorm_lazy_ranges(n, nparts).get("across a trip") if with_lazy else None
    g = torch.zeros(n)
    if lazy is not None:
        g[lazy[0]:lazy[1]] = float("nan")
    gd = offset_view(g, off, device)
    dev = torch.device(device).type
    for k, i in enumerate(sqnorm_positions(n, nparts, lazy)):
        gd[i] = 1.0 if k % 2 == 0 else -1.0
        _sqnorm_once(device, gd, nparts, 3.0, lazy, 9.0, f"sqnorm [{dev}] n={n} parts={nparts} off={off} lazy={lazy} "
                                                         f"single {'+' if k % 2 == 0 else '-'}1 at {i}")
        gd[i] = 0.0
    return 0.0


def run_sqnorm_refusals(device, n: int = 1027):
    """A lazy range that is not whole vectors or leaves the arena raises; ``out`` is as it was."""
    g = int_gradient(n).to(device)
    out = torch.full((_ops().SQ_PARTS,), 7.0, device=device)
    for lazy in ((2, 8), (4, 10), (0, n // 4 * 4 + 4), (-4, 4), (n, n + 8)):
        try:
            _ops().sqnorm(g, out, 1.0, lazy=lazy)
        except RuntimeError:
            pass
        else:
            raise AssertionError(f"sqnorm accepted the lazy range {lazy} of an arena of {n}")
        exact(out, torch.full((out.numel(),), 7.0), f"sqnorm [{torch.device(device).type}] refused lazy={lazy}: out")


# ----------------------------------------------------------------------------- 4. embed_bwd
EMBED_SHAPES = ((1, 2, 4), (7, 5, 36), (9, 17, 64), (256, 3, 16), (257, 3, 16), (300, 17, 48))
EMBED_TSETS = ("equal", "distinct", "mix6", "ends", "passes")
EMBED_PS = (0.0, 0.5)
EMBED_SITE = 3
TEMB_ROWS = 2000
EMBED_MUTANTS = ("neighbour_site", "drop_last_sample", "merge_timesteps")


def embed_timesteps(B: int, tset: str) -> torch.Tensor:
    """[B] int64 in [0, TEMB_ROWS).  ``passes`` (B > 256): timestep 5 occurs in both passes of
    256 samples, 9 (from B = 259) only in the second, the rest are distinct and, past sample
    255, second-pass only as well."""
    if tset == "equal":
        return torch.full((B,), 77, dtype=torch.int64)
    if tset == "distinct":
        return (torch.arange(B) * 5 + 3) % TEMB_ROWS
    if tset == "mix6":
        return torch.tensor([0, 3, 4, 100, 1000, 1999])[torch.randint(0, 6, (B,), generator=_gen(B))]
    if tset == "ends":
        return torch.where(torch.arange(B) % 3 == 1, 0, TEMB_ROWS - 1)
    assert tset == "passes" and B > 256
    t = torch.arange(B) + 20
    t[[1, 200, 256]] = 5
    if B > 258:
        t[[257, B - 1]] = 9
    return t


class EmbedCase(NamedTuple):
    g: torch.Tensor        # [B, N, D] fp32 integers in [-4, 4]
    t: torch.Tensor        # [B] int64
    p: float
    dcls: torch.Tensor     # prefills (fp32 integers in [-3, 3])
    dpos: torch.Tensor
    dtemb: torch.Tensor    # [TEMB_ROWS, D]


def embed_case(B: int, N: int, D: int, tset: str, p: float) -> EmbedCase:
    gen = _gen(1000 * B + N + D)
    mk = lambda shape, a: torch.randint(-a, a + 1, shape, generator=gen).float()  # noqa: E731
    return EmbedCase(mk((B, N, D), 4), embed_timesteps(B, tset), p, mk((D,), 3), mk((N * D,), 3), mk((TEMB_ROWS, D), 3))


class EmbedTruth(NamedTuple):
    dcls: torch.Tensor
    dpos: torch.Tensor
    dtemb: torch.Tensor
    gpatch: torch.Tensor   # bf16 [B (N - 1), D]
    named: torch.Tensor    # [TEMB_ROWS] bool: rows some sample names


def embed_truth(c: EmbedCase, mutant: Optional[str] = None) -> EmbedTruth:
    """The three gradients from int64 sums and the patch-row gradient, the keep mask from
    ``reference.keep_mask`` on the flat index.  Asserts the exactness conditions.  ``mutant``
    (one of :data:`EMBED_MUTANTS`): a wrong truth the reference must not match."""
    assert mutant is None or mutant in EMBED_MUTANTS
    B, N, D = c.g.shape
    gi = c.g.to(torch.int64)
    assert bool((gi.float() == c.g).all()) and int(gi.abs().max()) <= 4, "exactness condition violated: g"
    for pre in (c.dcls, c.dpos, c.dtemb):
        assert bool((pre.to(torch.int64).float() == pre).all()), "exactness condition violated: prefill"
    assert c.p in EMBED_PS
    if c.p > 0:
        assert ref.drop_threshold(c.p) == 32768, "exactness condition violated: threshold"
        assert float(_f(1.0) / (_f(1.0) - _f(c.p))) == 2.0, "exactness condition violated: rescale"
        site = EMBED_SITE + 1 if mutant == "neighbour_site" else EMBED_SITE
        keep = ref.keep_mask(B * N * D, _rng("cpu"), site, c.p).view(B, N, D)
        assert 0 < int(keep.sum()) < keep.numel() or keep.numel() < 16
        gi = gi * 2 * keep
    elif mutant == "neighbour_site":
        gi = gi.roll(1, 2)
    gsum = gi[:-1] if mutant == "drop_last_sample" else gi
    t = c.t.clone()
    if mutant == "merge_timesteps":
        t[t == t.max()] = t.min() if int(t.min()) != int(t.max()) else (int(t[0]) + 1) % TEMB_ROWS
    dcls = c.dcls.to(torch.int64) + gsum[:, 0].sum(0)
    dpos = c.dpos.to(torch.int64) + gsum.sum(0).reshape(-1)
    dtemb = c.dtemb.to(torch.int64).index_add(0, t[:gsum.shape[0]], gsum.sum(1))
    assert max(int(x.abs().max()) for x in (dcls, dpos, dtemb)) < 2 ** 24, "exactness condition violated: a sum >= 2^24"
    # (every partial sum is bounded by 8 B N + 3 = 40,803 at the largest shape: far below 2^24)
    assert 8 * B * N + 3 < 2 ** 24
    named = torch.zeros(TEMB_ROWS, dtype=torch.bool)
    named[t] = True
    return EmbedTruth(dcls.float(), dpos.float(), dtemb.float(), gi[:, 1:].reshape(B * (N - 1), D).to(torch.bfloat16),
                      named)


def check_embed(dcls, dpos, dtemb, gpatch, c: EmbedCase, tr: EmbedTruth, name: str):
    """Bit equality with the truth; the rows of ``dtemb`` no sample names keep the prefill."""
    exact(dcls.reshape(-1), tr.dcls, name + " dcls")
    exact(dpos.reshape(-1), tr.dpos, name + " dpos")
    exact(dtemb, tr.dtemb, name + " dtemb")
    exact(dtemb.detach().cpu()[~tr.named], c.dtemb[~tr.named], name + " dtemb rows no sample names")
    if gpatch is not None:
        exact(gpatch, tr.gpatch, name + " gpatch")


def embed_outputs(device, c: EmbedCase):
    """``ops.embed_bwd`` on the case: (dcls, dpos, dtemb, gpatch)."""
    dcls, dpos, dtemb = (x.clone().to(device) for x in (c.dcls, c.dpos, c.dtemb))
    gpatch = _ops().embed_bwd(c.g.to(device), c.t.to(device), _rng(device), EMBED_SITE, c.p, dcls, dpos, dtemb)
    return dcls, dpos, dtemb, gpatch


def run_embed(device, B: int, N: int, D: int, tset: str, p: float) -> float:
    c = embed_case(B, N, D, tset, p)
    name = f"embed_bwd [{torch.device(device).type}] B={B} N={N} D={D} t={tset} p={p}"
    check_embed(*embed_outputs(device, c), c, embed_truth(c), name)
    return 0.0


WGRAD_JOB = (8, 8)   # (Nout, K) of the small job beside the embedding parts


def run_embed_wgrad(device, B: int, N: int, D: int, tset: str, p: float, tokens: int) -> float:
    """The same probe through ``ops.linear_wgrad_multi(..., embed=...)`` with one small job
    beside it, every output a view of one arena and the grad-norm partials on.  Returns the
    worst error / bound of the embedding workgroups' partial slots (GPU; 0.0 on the CPU, whose
    fallback writes one partial for the whole arena)."""
    ops = _ops()
    assert B <= 256, "the weight-gradient launch takes one part-B pass: B <= 256"
    c = embed_case(B, N, D, tset, p)
    tr = embed_truth(c)
    gen = _gen(tokens)
    n_out, k = WGRAD_JOB
    dy = torch.randint(1, 4, (tokens, n_out), generator=gen).to(torch.bfloat16).to(device)
    x = torch.randint(1, 4, (tokens, k), generator=gen).to(torch.bfloat16).to(device)
    assert 9 * tokens < 2 ** 24
    sizes = (n_out * k, n_out, D, N * D, TEMB_ROWS * D)
    arena = torch.zeros(sum(sizes), device=device)
    dw, db, dcls, dpos, dtemb = (v.view(s) if isinstance(s, tuple) else v for v, s in zip(
        arena.split(sizes), ((n_out, k), None, None, None, (TEMB_ROWS, D))))
    dcls.copy_(c.dcls), dpos.copy_(c.dpos), dtemb.copy_(c.dtemb)
    parts = torch.full((ops.sq_parts_size(1),), float("nan"), device=device)
    owners = int(tr.named.sum())
    ops.linear_wgrad_multi([(dy, x, dw, db)], store=True, sq=(parts, arena, None),
                           embed=(c.g.to(device), c.t.to(device), _rng(device), EMBED_SITE, c.p, dcls, dpos, dtemb,
                                  owners, None))
    name = f"linear_wgrad_multi embed [{torch.device(device).type}] B={B} N={N} D={D} t={tset} p={p} tokens={tokens}"
    check_embed(dcls, dpos, dtemb, None, c, tr, name)
    exact(dw, (dy.double().cpu().t() @ x.double().cpu()).float(), name + " dw")
    exact(db, dy.double().cpu().sum(0).float(), name + " db")
    if not ops.native_available() or torch.device(device).type != "cuda":
        return 0.0
    tiles = int(torch.ops.ddim_cold.wgrad_multi_plan([n_out], [k], [tokens])[4])
    slots = ops.wgrad_embed_slots(B, N, D, owners, 0, 0, tokens)
    got = float(_c64(parts)[tiles:].sum())             # (the tail has no range: its slots and the rest are 0)
    assert int(torch.count_nonzero(_c64(parts)[tiles:]) ) <= slots, name + ": more non-zero slots than workgroups"
    written = torch.cat((tr.dcls, tr.dpos, tr.dtemb[tr.named].reshape(-1))).double()
    want = float((written * written).sum())
    bound = written.numel() * U32 * want
    ratio = abs(got - want) / bound if got == got else float("inf")
    line = f"{name} grad-norm slots: {got!r}, fp64 {want!r}, error / bound {ratio:.4f}"
    _log(line + ("" if ratio <= 1 else "  FAILED"))
    assert ratio <= 1, line
    return ratio


# ----------------------------------------------------------------------------- 5. bf16 wire
WIRE_LOWS = (0x0000, 0x7FFF, 0x8000, 0x8001, 0xFFFF)
WIRE_N = 655_365          # 2 x 65536 x 5 + 5: a second grid-stride trip (256 x 256 x 8 per trip) and a tail of 5
WIRE_SMALL = (1, 7, 8, 9)


def wire_source(n: int = WIRE_N) -> torch.Tensor:
    """[n] fp32: every high half crossed with :data:`WIRE_LOWS`, repeated to ``n``."""
    hi = torch.arange(65536, dtype=torch.int64).repeat_interleave(len(WIRE_LOWS))
    lo = torch.tensor(WIRE_LOWS, dtype=torch.int64).repeat(65536)
    bits = (hi << 16) | lo
    bits = bits.repeat(-(-n // bits.numel()))[:n]
    return (bits - ((bits >= 2 ** 31).to(torch.int64) << 32)).to(torch.int32).view(torch.float32).clone()


def run_wire_pack(device, n: int = WIRE_N, off: int = 0) -> float:
    """``ops.wire_pack`` into a canaried destination ``off`` elements in: bit-equal to the CPU
    conversion wherever the input is not NaN, NaN where it is."""
    src = wire_source(n)
    view, check = canary((n + off,), 64, torch.bfloat16, device)
    before = view[:off].clone()
    _ops().wire_pack(offset_view(src, off, device), view[off:])
    name = f"wire_pack [{torch.device(device).type}] n={n} off={off}"
    got, want, nan = view[off:].detach().cpu(), src.to(torch.bfloat16), torch.isnan(src)
    assert bool(torch.isnan(got[nan].float()).all()), name + ": a NaN came out as a number"
    exact(got[~nan], want[~nan], name)
    check(name)
    exact(view[:off], before, name + " elements before the view")
    return 0.0


def run_wire_unpack(device, n: int = 65536, off: int = 0) -> float:
    """``ops.wire_unpack`` of every bf16 pattern (the first ``n``, or repeated to ``n``): ``bits << 16``."""
    pat = torch.arange(65536, dtype=torch.int64).repeat(-(-n // 65536))[:n]
    src = (pat - ((pat >= 32768).to(torch.int64) << 16)).to(torch.int16).view(torch.bfloat16).clone()
    view, check = canary((n + off,), 64, torch.float32, device)
    before = view[:off].clone()
    _ops().wire_unpack(offset_view(src, off, device), view[off:])
    name = f"wire_unpack [{torch.device(device).type}] n={n} off={off}"
    got = view[off:].detach().cpu()
    want = ((pat << 16) - ((pat >= 32768).to(torch.int64) << 32)).to(torch.int32).view(torch.float32)
    nan = torch.isnan(want)
    assert bool(torch.isnan(got[nan]).all()), name + ": a NaN came out as a number"
    exact(got[~nan], want[~nan], name)
    check(name)
    exact(view[:off], before, name + " elements before the view")
    return 0.0


def run_wire_refusals(device):
    """A size mismatch raises and writes nothing."""
    ops = _ops()
    for fn, sdt, ddt in ((ops.wire_pack, torch.float32, torch.bfloat16), (ops.wire_unpack, torch.bfloat16, torch.float32)):
        src = torch.ones(16, dtype=sdt, device=device)
        view, check = canary((15,), 64, ddt, device)
        before = view.clone()
        try:
            fn(src, view)
        except RuntimeError:
            pass
        else:
            raise AssertionError(f"{fn.__name__} accepted 16 elements into 15")
        exact(view, before, f"{fn.__name__} [{torch.device(device).type}] refused: destination")
        check(fn.__name__)
