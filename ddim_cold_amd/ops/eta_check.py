"""fp64 truths and a-priori bounds for the stochastic DDIM step (eta > 0) of the patch-row head
epilogue: ``ops.head_step_rows_`` modes 5 and 6 (csrc/gemm_epi.h ``EPI_HEADRS``), whose noise is
drawn inside the epilogue.  The companion of :mod:`.epi_check`, from which the cases
(:func:`epi_check.ddim_case`: a zero operand plus the bias sets the raw prediction to the bit)
and the comparison helpers come.

**The update.**  With a coefficient row of 8 floats ``{c0, c1, c2, dir, sigma, 0, 0, 0}``
(``schedule.eta_row``), per element of the fp32 patch-row state ``x`` [B*P, F]:

    ``x0 = clamp(raw, -1, 1)``,  ``x_next = c2 x0 + dir (x_t - c0 x0) / c1 + sigma z``.

``z`` is element (row, column) of ``ops.randn_`` over a buffer of ``x``'s shape at ``rng =
[seed, 0]`` and the step's site: flat index ``row F + column``.

**The noise probe** (:func:`probe_noise`).  The row ``{0, 1, 0, 0, 1, 0, 0, 0}`` makes the update
``0 x0 + 0 (x_t / 1) + 1 z``: every product with 0 is a zero, ``1 z`` is exact and adding zeros
changes nothing, so ``x_next`` IS the implementation's own ``z``, bit for bit (``x_t`` and ``raw``
finite).  :func:`run_noise_probe` compares it with ``ops.randn_`` on the same device at the
same ``rng``, site and shape and demands equality to the bit, at two sites: that pins the index
convention (row-major over the destination), the halves of each Box-Muller pair (cosine at the
even index) and the site.  The epilogue's helper (csrc/common.h ``gauss_pair``) performs
``randn_kernel``'s operations in its order for exactly this reason.

**Arithmetic** (:func:`check_eta`).  Truth in fp64 from the fp32 row, the exact raw prediction
and the probe's ``z``.  ``x0_out`` is the clamp to the bit; ``patches_out`` is the bf16 rounding
of the stored ``x`` to the bit; ``x_next`` is within

    ``10 x 2^-24 (|c2 x0| + |dir / c1| (|x_t| + |c0 x0|) + |sigma z|)``:

:mod:`.epi_check` derives 8 x 2^-24 for the deterministic part (five roundings and a 2.5-ulp
division, each relative to an intermediate no larger than the sum in brackets); the product
``sigma z`` and the final addition contribute one rounding each.

**Exact cases** (:func:`run_exact`).  A row with ``sigma = 0`` (eta = 0) gives, on the same
inputs, the bits of mode 1 (one row) / mode 4 (per-sample rows) in ``x``, ``x0_out`` and
``patches_out``: ``sigma z`` is a zero.  The identity row ``{0, 1, 0, 1, 0, ..}`` of mode 6
leaves ``x`` exactly ``x_t``.  At the last step of a k >= 2 grid ``dir = sigma = 0`` and
``x_next`` is ``fp32(c2) x0`` to the bit (checked inside :func:`check_eta`).

**Cases.**  Rows at t = T - 1, a middle step and the last of the k = 20 grid at eta = 0.3 and
eta = 1, in mode 5 and as mixed per-sample rows in mode 6 (started / not started / last).
Geometries ``(B, C, H, W, p)`` at D = 64: the two of :mod:`.epi_check`; ``(5, 3, 16, 16, 4)``
-- 85 token rows cross the 32- and 64-row tiles with a ragged last tile, F = 48 < 64; ``(3, 3,
24, 24, 8)`` -- P = 9, so sample boundaries fall inside 16-row fragments (per-sample rows
differ within a fragment), F = 192 = three column tiles.

Every runner takes ``step`` -- the implementation under test with the signature of
:func:`ops_step` (default: ``ops.head_step_rows_``, HIP on a GPU, the reference on the CPU) -- so
the same checks run on :func:`ddim_eta_f32`, an fp32 emulation of the kernel, and on its
mutants (``MUTANTS``), which tests/test_ddim_eta_cpu.py shows them to reject.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence, Tuple

import torch

from .epi_check import DDIM_K, DDIM_T, U32, DdimCase, _c64, _ops, assert_exact, assert_within, ddim_case, ddim_rows

EPI_HEADRS = 12            # csrc/kernels.h (the ``epi`` of ``torch.ops.ddim_cold.gemm_plan``)
HEAD_D = 64
GEOMS = ((2, 3, 16, 16, 4), (2, 3, 16, 16, 8), (5, 3, 16, 16, 4), (3, 3, 24, 24, 8))
TILE_CFGS = (0, 1, 2, 3)   # the 4-wave tiles (8-wave tiles are not built for the head epilogues)
ETAS = (0.3, 1.0)
ETA_TS = (1999, 999, 19)                    # first step, a middle one, the last (k = 20)
MODE6_CYCLE = (999, None, 19, 1999)         # started / not started / last / first ...
MODE6_SHIFTS = (0, 2)                       # ... sample b takes entry (b + shift) % 4
PROBE_ROW = (0.0, 1.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0)
IDENT_ROW8 = (0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
SEED = 20240229
STEPS = (0, 3)                              # the sampling steps whose sites the probe visits
MUTANTS = ("swap_halves", "column_noise", "sigma_squared", "dir_deterministic", "same_site", "neighbour_sigma")


def step_site(i: int) -> int:
    return _ops().SITE_STEP_NOISE + i


def rng_of(device, seed: int = SEED) -> torch.Tensor:
    return torch.tensor([seed, 0], dtype=torch.int64, device=device)


def eta_rows(ts: Sequence[Optional[int]], eta: float) -> torch.Tensor:
    """fp32 rows [len(ts), 8] of ``schedule.eta_row(T, t, k, eta)`` (None: the identity row)."""
    from ..diffusion.schedule import eta_row
    return torch.tensor([IDENT_ROW8 if t is None else eta_row(DDIM_T, t, DDIM_K, eta) for t in ts],
                        dtype=torch.float32)


def mode6_ts(B: int, shift: int):
    return tuple(MODE6_CYCLE[(b + shift) % len(MODE6_CYCLE)] for b in range(B))


def dims(geom):
    B, C, H, W, p = geom
    return B, (H // p) * (W // p), C * p * p


def case_rows(case: DdimCase):
    """(x_t rows, raw rows) [B*P, F] fp32 of a :func:`epi_check.ddim_case`."""
    p = case.geom[4]
    ops = _ops()
    return ops.image_to_rows(case.x_t, p).contiguous(), ops.image_to_rows(case.raw, p).contiguous()


# ----------------------------------------------------------------------------- implementations
def ops_step(case: DdimCase, device, x_t, coef, mode: int, rng=None, site: int = 0):
    """``ops.head_step_rows_`` on the case's zero operand + bias from the state ``x_t`` [B*P, F];
    returns ``(x, x0_out, patches_out)``; the outputs start as NaN canaries."""
    ops = _ops()
    B, NP, F = dims(case.geom)
    a, w, bias = (t.to(device) for t in (case.a, case.w, case.bias))
    x = x_t.to(device).clone()
    x0 = torch.full((B * NP, F), float("nan"), device=device)
    po = torch.full((B * NP, F), float("nan"), dtype=torch.bfloat16, device=device)
    noise = (rng.to(device), site) if mode in (ops.HEAD_ETA, ops.HEAD_ETA_EACH) else None
    ops.head_step_rows_(a, w, bias, x, x0, coef.contiguous().to(device), B, mode, patches_out=po, noise=noise)
    return x, x0, po


def ddim_eta_f32(case: DdimCase, device, x_t, coef, mode: int, rng=None, site: int = 0,
                 mutant: Optional[str] = None):
    """The kernel's arithmetic in fp32 on the CPU, operation by operation (the fused
    multiply-adds the compiler forms are at least as accurate), with the signature of
    :func:`ops_step`.  ``mutant``: one of ``MUTANTS`` --

    * ``swap_halves``: sine at the even index of each Box-Muller pair, cosine at the odd;
    * ``column_noise``: the noise indexed by the column alone (every row the same draw);
    * ``sigma_squared``: ``sigma^2 z`` added;
    * ``dir_deterministic``: ``sqrt(1 - a_tk)`` = ``sqrt(dir^2 + sigma^2)`` kept for ``dir``
      (wherever the row has a direction term);
    * ``same_site``: the first step's site at every step;
    * ``neighbour_sigma``: mode 6 takes ``sigma`` from the next sample's row."""
    assert mutant is None or mutant in MUTANTS
    ops = _ops()
    B, NP, F = dims(case.geom)
    x_t = x_t.detach().float().cpu()
    raw = case.bias.unsqueeze(0).expand(B * NP, F)
    x0 = raw.clamp(-1.0, 1.0)
    if mode in (ops.HEAD_DDIM, ops.HEAD_DDIM_EACH):
        cf = coef.detach().float().cpu().reshape(-1, 4)
        cf = cf.repeat_interleave(NP, 0) if mode == ops.HEAD_DDIM_EACH else cf.expand(B * NP, 4)
        c0, c1, c2, cd = (cf[:, i:i + 1] for i in range(4))
        xn = c2 * x0 + cd * ((x_t - c0 * x0) / c1)
        return xn, x0.clone(), xn.to(torch.bfloat16)
    cf = coef.detach().float().cpu().reshape(-1, 8)
    if mode == ops.HEAD_ETA_EACH and mutant == "neighbour_sigma":
        cf = torch.cat((cf[:, :4], cf.roll(-1, 0)[:, 4:]), 1)
    cf = cf.repeat_interleave(NP, 0) if mode == ops.HEAD_ETA_EACH else cf.expand(B * NP, 8)
    c0, c1, c2, cd, sg = (cf[:, i:i + 1] for i in range(5))
    z = torch.empty(B * NP, F)
    if mutant == "column_noise":
        zc = torch.empty(F)
        ops.randn_(zc, rng.cpu(), site)
        z.copy_(zc.unsqueeze(0).expand(B * NP, F))
    else:
        ops.randn_(z, rng.cpu(), step_site(0) if mutant == "same_site" else site)
    if mutant == "swap_halves":
        z = z.reshape(-1, 2).flip(1).reshape(B * NP, F)
    if mutant == "sigma_squared":
        sg = sg * sg
    if mutant == "dir_deterministic":
        cd = torch.where(cd != 0, torch.sqrt(cd * cd + sg * sg), cd)  # (the probe row has no direction term)
    xn = (c2 * x0 + cd * ((x_t - c0 * x0) / c1)) + sg * z
    return xn, x0.clone(), xn.to(torch.bfloat16)


def mutant_step(mutant: str) -> Callable:
    def step(case, device, x_t, coef, mode, rng=None, site=0):
        return ddim_eta_f32(case, device, x_t, coef, mode, rng, site, mutant=mutant)
    return step


# ----------------------------------------------------------------------------- noise probe
def probe_noise(case: DdimCase, device, rng, site: int, step: Callable = ops_step) -> torch.Tensor:
    """The implementation's own ``z`` [B*P, F] (on ``device``) at (rng, site): mode 5 with the probe row."""
    x_t, _ = case_rows(case)
    x, _, _ = step(case, device, x_t, torch.tensor(PROBE_ROW), _ops().HEAD_ETA, rng, site)
    return x


def run_noise_probe(device, geom, step: Callable = ops_step) -> None:
    """The probe's ``z`` against ``ops.randn_`` on the same device, to the bit, at the sites of
    two different sampling steps; the two draws differ from each other."""
    ops, case = _ops(), ddim_case(geom)
    B, NP, F = dims(geom)
    rng = rng_of(device)
    got = []
    for i in STEPS:
        z = probe_noise(case, device, rng, step_site(i), step)
        want = torch.empty(B * NP, F, device=device)
        ops.randn_(want, rng, step_site(i))
        assert_exact(z, want, f"noise probe {geom} step {i}: the epilogue's z against randn_ at the same rng / site")
        got.append(z)
    assert not torch.equal(got[0].cpu(), got[1].cpu()), "two steps drew the same noise"


# ----------------------------------------------------------------------------- arithmetic
def check_eta(x, x0_out, po, case: DdimCase, rows: torch.Tensor, z, ts: Sequence[Optional[int]], name: str) -> float:
    """``x`` / ``x0_out`` / ``patches_out`` [B*P, F] of one step with the fp32 ``rows`` ([1, 8], or
    [B, 8] per sample; ``ts`` names them) and the noise ``z`` against the truth; returns the
    worst error / bound of ``x_next``."""
    B, NP, F = dims(case.geom)
    x_t, raw = case_rows(case)
    x0 = raw.clamp(-1.0, 1.0)
    assert_exact(x0_out.detach().cpu(), x0, f"{name} x0_out against clamp(raw, -1, 1)")
    cf = (rows.double().expand(B, 8) if rows.shape[0] == 1 else rows.double()).repeat_interleave(NP, 0)
    c0, c1, c2, cd, sg = (cf[:, i:i + 1] for i in range(5))
    x0d, xtd, zd = x0.double(), x_t.double(), _c64(z)
    truth = c2 * x0d + cd * (xtd - c0 * x0d) / c1 + sg * zd
    tol = 10 * U32 * ((c2 * x0d).abs() + (cd / c1).abs() * (xtd.abs() + (c0 * x0d).abs()) + (sg * zd).abs())
    xn = x.detach().cpu()
    worst = assert_within(xn, truth, tol, f"{name} x_next")
    assert_exact(po.detach().cpu(), xn.to(torch.bfloat16), f"{name} patches_out against bf16(x)")
    tsb = list(ts) if len(ts) == B else list(ts) * B
    xb, x0b, xtb = (v.reshape(B, NP, F) for v in (xn, x0, x_t))
    for b, t in enumerate(tsb):
        if t is None:
            assert_exact(xb[b], xtb[b], f"{name} sample {b}: x_next under the identity row against x_t")
        elif t + 1 == DDIM_K:
            row = rows[b if rows.shape[0] > 1 else 0]
            assert float(row[3]) == 0.0 and float(row[4]) == 0.0, "last step: dir = sigma = 0"
            assert_exact(xb[b], row[2] * x0b[b], f"{name} sample {b}: x_next at the last step against c2 x0")
    return worst


def run_eta(device, geom, step: Callable = ops_step) -> float:
    """Modes 5 and 6 at eta in ``ETAS``: rows of the first, a middle and the last step, then mixed
    per-sample rows; the noise of each step is the implementation's own (the probe's) at that
    rng / site.  Returns the worst error / bound of ``x_next``."""
    case = ddim_case(geom)
    B, NP, F = dims(geom)
    x_t, _ = case_rows(case)
    rng = rng_of(device)
    zs = {i: probe_noise(case, device, rng, step_site(i), step) for i in STEPS}
    worst = 0.0
    for eta in ETAS:
        for n, t in enumerate(ETA_TS):
            i = STEPS[n % len(STEPS)]
            rows = eta_rows((t,), eta)
            x, x0, po = step(case, device, x_t, rows[0], _ops().HEAD_ETA, rng, step_site(i))
            worst = max(worst, check_eta(x, x0, po, case, rows, zs[i], (t,), f"mode 5 eta={eta} t={t} {geom}"))
        for n, shift in enumerate(MODE6_SHIFTS):
            i = STEPS[n % len(STEPS)]
            ts = mode6_ts(B, shift)
            rows = eta_rows(ts, eta)
            x, x0, po = step(case, device, x_t, rows, _ops().HEAD_ETA_EACH, rng, step_site(i))
            worst = max(worst, check_eta(x, x0, po, case, rows, zs[i], ts, f"mode 6 eta={eta} t={ts} {geom}"))
    return worst


# ----------------------------------------------------------------------------- exact cases
def run_exact(device, geom, step: Callable = ops_step) -> None:
    """sigma = 0 rows against modes 1 / 4 on the same inputs (x, x0_out, patches_out to the bit),
    and the identity row of mode 6 (x stays x_t to the bit)."""
    ops, case = _ops(), ddim_case(geom)
    B, NP, F = dims(geom)
    x_t, _ = case_rows(case)
    rng = rng_of(device)
    site = step_site(1)
    for t in ETA_TS:
        rows8, rows4 = eta_rows((t,), 0.0), ddim_rows((t,))
        assert torch.equal(rows8[:, :4], rows4) and float(rows8[0, 4]) == 0.0
        got = step(case, device, x_t, rows8[0], ops.HEAD_ETA, rng, site)
        want = step(case, device, x_t, rows4[0], ops.HEAD_DDIM)
        for g, w_, nm in zip(got, want, ("x", "x0_out", "patches_out")):
            assert_exact(g, w_, f"mode 5 with sigma = 0 against mode 1, t={t} {geom}: {nm}")
    for shift in MODE6_SHIFTS:
        ts = mode6_ts(B, shift)
        rows8, rows4 = eta_rows(ts, 0.0), ddim_rows(ts)
        got = step(case, device, x_t, rows8, ops.HEAD_ETA_EACH, rng, site)
        want = step(case, device, x_t, rows4, ops.HEAD_DDIM_EACH)
        for g, w_, nm in zip(got, want, ("x", "x0_out", "patches_out")):
            assert_exact(g, w_, f"mode 6 with sigma = 0 against mode 4, t={ts} {geom}: {nm}")
    x, _, _ = step(case, device, x_t, eta_rows((None,) * B, 1.0), ops.HEAD_ETA_EACH, rng, site)
    assert_exact(x, x_t, f"mode 6 identity rows {geom}: x against x_t")


def run_all(device, geom, step: Callable = ops_step) -> float:
    run_noise_probe(device, geom, step)
    run_exact(device, geom, step)
    return run_eta(device, geom, step)


def plan_shape(geom) -> Tuple[int, int, int]:
    """(M, N, K) of the head GEMM of a geometry (for ``gemm_plan``)."""
    B, NP, F = dims(geom)
    return B * (NP + 1), F, HEAD_D
