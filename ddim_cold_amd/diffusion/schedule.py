"""The "sqrt" noise schedule of the reference and DDIM step tables.

* training / q_sample:  abar(t) = 1 - sqrt((t+1)/T)          (diffusion_loader.py:52)
* DDIM update:          abar_t  = 1 - sqrt((t+1)/T) + 1e-5    (ViT.py:232)
                        abar_tk = 1 - sqrt((t+1-k)/T)          (ViT.py:231, no epsilon)
* img2img start noise:  alpha   = 1 - sqrt(t_start/T)          (ViT_draft2drawing.py:395)

The DDIM jump ``k`` must be such that t+1-k >= 0 at the last visited step
(the reference raises ``math domain error`` otherwise); we raise
a clear ``ValueError`` instead.
"""
from __future__ import annotations

import math
from typing import List

import torch


def alpha_bar_train(t, total_steps: int):
    if isinstance(t, torch.Tensor):
        return 1.0 - torch.sqrt((t.double() + 1.0) / total_steps)
    return 1.0 - math.sqrt((t + 1) / total_steps)


def ddim_timesteps(total_steps: int, k: int, start: int | None = None) -> List[int]:
    if k <= 0:
        raise ValueError("DDIM step jump k must be positive")
    start = total_steps - 1 if start is None else start
    ts = list(range(start, 0, -k))
    if not ts:
        raise ValueError("empty DDIM schedule")
    if ts[-1] + 1 - k < 0:
        raise ValueError(
            f"DDIM step jump k={k} incompatible with start={start}, total_steps={total_steps}: the last step "
            f"t={ts[-1]} would need alpha_bar at t+1-k={ts[-1] + 1 - k} < 0 (use k dividing {start + 1})")
    return ts


def ddim_coefficients(total_steps: int, t: int, k: int):
    """(sqrt(a_t), sqrt(1-a_t), sqrt(a_{t-k}), sqrt(1-a_{t-k})) for one DDIM jump."""
    a_t = 1.0 - math.sqrt((t + 1) / total_steps) + 1e-5
    a_tk = 1.0 - math.sqrt((t + 1 - k) / total_steps)
    if a_tk < 0:
        raise ValueError(f"invalid DDIM jump t={t}, k={k}")
    return math.sqrt(a_t), math.sqrt(1.0 - a_t), math.sqrt(a_tk), math.sqrt(1.0 - a_tk)


def ddim_table(total_steps: int, k: int, start: int | None = None, device="cpu"):
    ts = ddim_timesteps(total_steps, k, start)
    coef = torch.tensor([ddim_coefficients(total_steps, t, k) for t in ts], dtype=torch.float32, device=device)
    return ts, coef


def ddim_coefficients_eta(total_steps: int, t: int, k: int, eta: float):
    """``(c0, c1, c2, dir, sigma)`` of one jump of the DDIM family (Song et al. 2021, eq. 12
    and 16): ``x_{t-k} = c2 x0 + dir (x_t - c0 x0) / c1 + sigma z`` with the ``a_t`` /
    ``a_{t-k}`` of :func:`ddim_coefficients`,

        ``sigma = eta sqrt((1 - a_{t-k}) / (1 - a_t) (1 - a_t / a_{t-k}))``,
        ``dir = sqrt(1 - a_{t-k} - sigma^2)``.

    ``eta`` = 0 is the deterministic sampler (the very floats of :func:`ddim_coefficients`,
    ``sigma`` = 0.0), ``eta`` = 1 DDPM ancestral sampling.  At a last step onto ``a_{t-k}``
    = 1 (k >= 2 dividing T) both ``sigma`` and ``dir`` are exactly 0."""
    eta = float(eta)
    if not 0.0 <= eta <= 1.0:  # (NaN fails too)
        raise ValueError(f"eta must be in [0, 1], got {eta!r}")
    c0, c1, c2, c3 = ddim_coefficients(total_steps, t, k)
    if eta == 0.0:
        return c0, c1, c2, c3, 0.0
    a_t = 1.0 - math.sqrt((t + 1) / total_steps) + 1e-5
    a_tk = 1.0 - math.sqrt((t + 1 - k) / total_steps)
    rad = (1.0 - a_tk) / (1.0 - a_t) * (1.0 - a_t / a_tk)
    if rad < 0.0:
        raise ValueError(f"invalid DDIM jump t={t}, k={k}: a_t > a_(t-k)")
    sigma = eta * math.sqrt(rad)
    rdir = 1.0 - a_tk - sigma * sigma
    if rdir < 0.0:
        raise ValueError(f"invalid DDIM jump t={t}, k={k}, eta={eta}: 1 - a_(t-k) < sigma^2")
    return c0, c1, c2, math.sqrt(rdir), sigma


ETA_IDENT_ROW = (0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)  # x_next = x_t: a sample that has not started


def eta_row(total_steps: int, t: int, k: int, eta: float):
    """The 8-float coefficient row ``{c0, c1, c2, dir, sigma, 0, 0, 0}`` of one jump."""
    return ddim_coefficients_eta(total_steps, t, k, eta) + (0.0, 0.0, 0.0)


def ddim_table_eta(total_steps: int, k: int, eta: float, start: int | None = None, device="cpu"):
    """:func:`ddim_table` for the DDIM family: rows of 8 fp32 values (:func:`eta_row`)."""
    ts = ddim_timesteps(total_steps, k, start)
    coef = torch.tensor([eta_row(total_steps, t, k, eta) for t in ts], dtype=torch.float32, device=device)
    return ts, coef


def dpm2m_step_h(total_steps: int, t: int, k: int) -> float:
    """The step ``h = lambda_{t-k} - lambda_t`` of one jump in half-log-SNR ``lambda = ln(alpha /
    sigma)``, from the floats of :func:`ddim_coefficients`: ``ln(c2 / c3) - ln(c0 / c1)``;
    ``inf`` for the last jump onto a_{t-k} = 1 (``c3`` = 0)."""
    c0, c1, c2, c3 = ddim_coefficients(total_steps, t, k)
    if c3 == 0.0:
        return math.inf
    return math.log(c2 / c3) - math.log(c0 / c1)


def dpm2m_row(total_steps: int, t: int, k: int, h_prev):
    """The 8-float coefficient row ``{c0, c1, c2, c3, g, 0, 0, 0}`` of one DPM-Solver++(2M) jump
    t -> t-k (Lu et al. 2022, Algorithm 2) of an x0-predicting model; the update it describes is

        ``x_next = c2 x0 + c3 (x_t - c0 x0) / c1 + g (x0 - x0_prev)``     (``ops.dpm2m_rows_``)

    with ``c0..c3`` the very floats of :func:`ddim_coefficients`, ``x0`` this step's clamped
    prediction and ``x0_prev`` the previous step's.

    Derivation.  With alpha = sqrt(a), sigma = sqrt(1 - a), lambda = ln(alpha / sigma) and
    ``h = lambda_{t-k} - lambda_t`` the multistep solver steps

        ``x_next = (sigma_next / sigma_t) x_t - alpha_next (e^{-h} - 1) D``,
        ``D = (1 + 1 / (2 r)) x0 - (1 / (2 r)) x0_prev``,   ``r = h_prev / h``.

    ``e^{-h} = (sigma_next / alpha_next) (alpha_t / sigma_t) = c3 c0 / (c2 c1)``, so ``-alpha_next
    (e^{-h} - 1) = c2 - c3 c0 / c1``, and with D = x0 the step is ``(c3 / c1) x_t + (c2 - c3 c0 /
    c1) x0 = c2 x0 + c3 (x_t - c0 x0) / c1``: DDIM, the solver's first-order member.  The rest of
    D contributes ``(c2 - c3 c0 / c1) (1 / (2 r)) (x0 - x0_prev)``, hence

        ``g = (c2 - c3 c0 / c1) h / (2 h_prev)``,   ``h = ln(c2 / c3) - ln(c0 / c1)``.

    ``g`` is exactly 0.0, and the step DDIM's, when ``h_prev`` is None (a sample's first step:
    no history) and when ``c3 == 0`` (the last jump onto a = 1: h is infinite, the solver's
    final step is first-order).  Computed in Python floats, stored as fp32 by the tables."""
    c0, c1, c2, c3 = ddim_coefficients(total_steps, t, k)
    g = 0.0
    if h_prev is not None and c3 != 0.0:
        h = math.log(c2 / c3) - math.log(c0 / c1)
        g = (c2 - c3 * c0 / c1) * h / (2.0 * h_prev)
    return c0, c1, c2, c3, g, 0.0, 0.0, 0.0


def dpm2m_table(total_steps: int, k: int, start: int | None = None, device="cpu"):
    """``(ts, [steps, 8] fp32 rows of :func:`dpm2m_row`)`` over :func:`ddim_timesteps`: the first
    row has no history (g = 0), every later one the ``h`` of the row before it."""
    ts = ddim_timesteps(total_steps, k, start)
    rows, h_prev = [], None
    for t in ts:
        rows.append(dpm2m_row(total_steps, t, k, h_prev))
        h_prev = dpm2m_step_h(total_steps, t, k)
    return ts, torch.tensor(rows, dtype=torch.float32, device=device)


def repaint_row(total_steps: int, t: int, k: int, jump: bool):
    """``(ka, kb, ra, rb)`` of the inpainting mask step after the DDIM jump t -> t-k
    (``ops.repaint_rows_``; Lugmayr et al. 2022).  The known region is pasted at the level the
    jump landed on, ``ka known + kb z1`` with ``ka, kb = sqrt(a_{t-k}), sqrt(1 - a_{t-k})``: the
    very floats :func:`ddim_coefficients` returns last (exactly 1.0, 0.0 when the jump lands on
    a_{t-k} = 1).  ``jump``: the state is then diffused forward to level t again, ``ra x + rb
    z2`` with ``ra, rb = sqrt(a_t / a_{t-k}), sqrt(1 - a_t / a_{t-k})`` and the ``a_t`` of
    :func:`ddim_coefficients` (its 1e-5 included); otherwise ``ra, rb = 1.0, 0.0``."""
    _, _, ka, kb = ddim_coefficients(total_steps, t, k)
    a_t = 1.0 - math.sqrt((t + 1) / total_steps) + 1e-5
    a_tk = 1.0 - math.sqrt((t + 1 - k) / total_steps)
    if a_t > a_tk:
        raise ValueError(f"invalid DDIM jump t={t}, k={k}: a_t > a_(t-k)")
    if not jump:
        return ka, kb, 1.0, 0.0
    r = a_t / a_tk
    return ka, kb, math.sqrt(r), math.sqrt(1.0 - r)


def repaint_table(total_steps: int, k: int, resample: int = 1, device="cpu"):
    """``(ts, [forwards, 4] fp32 rows of :func:`repaint_row`)`` of an inpainting loop: each
    step of the ``ddim_timesteps(total_steps, k)`` grid runs ``resample`` times, jumping back to
    its own level after every run but the last; ``ts`` lists the timestep of every forward."""
    if isinstance(resample, bool) or not isinstance(resample, int) or resample < 1:
        raise ValueError(f"resample must be an int >= 1, got {resample!r}")
    ts, rows = [], []
    for t in ddim_timesteps(total_steps, k):
        for j in range(resample):
            ts.append(t)
            rows.append(repaint_row(total_steps, t, k, jump=j < resample - 1))
    return ts, torch.tensor(rows, dtype=torch.float32, device=device)


def img2img_alpha(t_start: int, total_steps: int) -> float:
    return 1.0 - math.sqrt(t_start / total_steps)


def cold_steps(img_size: int) -> int:
    """Number of cold (de-pixelation) steps = log2(image size) (6 for 64x64, ViT_draft2drawing.py:271)."""
    return int(math.log2(img_size))
