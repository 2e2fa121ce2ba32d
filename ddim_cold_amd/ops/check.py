"""Scale-aware comparison of the attention kernels with an fp64 truth.

Softmax outputs and their gradients shrink like ``sqrt(e/N)``, so an absolute
tolerance that is tight at N=65 is most of the signal at N=2,501.  The checks
here are relative to the size of the truth, and their bounds are not constants:
they are multiples of the distance the bf16-mirroring reference
(:func:`reference.attn_fwd` / :func:`reference.attn_bwd`) itself keeps from the
truth at the same inputs.

The kernel and the mirror round at the same points (P to bf16, dS to bf16,
outputs to bf16); what differs is fp32-level (MFMA summation order, hardware
exp2/log2, the lazy running max), so a right kernel sits at about 1x the
mirror's distance.  ``frob`` averages thousands of elements (margin 2x),
``maxn`` is an extreme-value statistic (3x), and the mirror's ``scale`` can be
zero by accident (3x plus a 5e-4 floor, 100x under a 5 % scale error).
"""
from __future__ import annotations

import math
import os
from typing import List, NamedTuple, Optional

import torch

from . import reference as ref

FROB_MARGIN = 2.0
MAXN_MARGIN = 3.0
SCALE_MARGIN = 3.0
SCALE_FLOOR = 5e-4
LSE_PAD_SHARE = 0.25          # of the smallest shift one extra zero-score key causes
LSE_ULPS = 8.0 * 2.0 ** -23   # of max|lse|: fp32 evaluation of the logarithm

# when set, every verdict is appended to this file as one line (profiles/attn_error.txt)
LOG_ENV = "DDIM_COLD_ATTN_ERROR_LOG"


# ----------------------------------------------------------------------------- truth
def attn_truth(qkv, do, scale: float, rng, site: int, p: float, bh0: int = 0):
    """fp64 attention forward and backward with the keep masks of
    :func:`reference.attn_keep_mask`: no bf16 rounding anywhere, delta from its own
    ``o``.  ``qkv`` [3,B,H,N,hd], ``do`` [B,N,H*hd] token-major (None: forward only).
    Returns ``o, lse, dq, dk, dv``, each [B,H,N,hd] (lse [B,H,N]) in fp64."""
    _, B, H, N, hd = qkv.shape
    q, k, v = qkv[0].double(), qkv[1].double(), qkv[2].double()
    s = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    pr = torch.exp(s - lse.unsqueeze(-1))
    del s
    if p > 0.0:
        m = ref.attn_keep_mask(B, H, N, rng, site, p, pr.device, bh0).double() / (1.0 - p)
        pd = pr * m
    else:
        m, pd = None, pr
    o = pd @ v
    if do is None:
        return o, lse, None, None, None
    dof = do.double().view(B, N, H, hd).transpose(1, 2)
    dv = pd.transpose(-1, -2) @ dof
    dp = dof @ v.transpose(-1, -2)
    if m is not None:
        dp = dp * m
    delta = (dof * o).sum(-1, keepdim=True)
    ds = pr * (dp - delta)
    dq = (ds @ k) * scale
    dk = (ds.transpose(-1, -2) @ q) * scale
    return o, lse, dq, dk, dv


def split_o(o: torch.Tensor, B: int, H: int, N: int, hd: int) -> torch.Tensor:
    """Token-major attention output [B,N,H*hd] -> [B,H,N,hd]."""
    return o.reshape(B, N, H, hd).transpose(1, 2)


def split_dqkv(dqkv: torch.Tensor, B: int, H: int, N: int, hd: int):
    """The ``dq, dk, dv`` blocks, each [B,H,N,hd], of the token-major [B*N, 3D] gradient."""
    d = dqkv.reshape(B, N, 3, H, hd).permute(2, 0, 3, 1, 4)
    return d[0], d[1], d[2]


# ----------------------------------------------------------------------------- metrics
class Metrics(NamedTuple):
    frob: float   # ||a-t|| / ||t||
    maxn: float   # max|a-t| / rms(t)
    scale: float  # <a,t>/<t,t> - 1
    err2: float   # ||a-t||      (un-normalised: the bounds compare these, so a zero
    errmax: float  # max|a-t|      truth leaves them defined)
    rms: float    # rms(t)


def metrics(a: torch.Tensor, truth: torch.Tensor) -> Metrics:
    """``frob``, ``maxn`` and ``scale`` of ``a`` against ``truth``, all in fp64."""
    a, t = a.double(), truth.double()
    assert a.shape == t.shape, (a.shape, t.shape)
    e = a - t
    tt = (t * t).sum().item()
    err2 = e.norm().item()
    errmax = e.abs().max().item()
    if not (math.isfinite(err2) and math.isfinite(errmax)):
        err2 = errmax = float("inf")  # NaN never passes a bound
    rms = math.sqrt(tt / max(t.numel(), 1))
    if tt > 0.0:
        return Metrics(err2 / math.sqrt(tt), errmax / rms, (a * t).sum().item() / tt - 1.0, err2, errmax, rms)
    z = 0.0 if err2 == 0.0 else float("inf")
    return Metrics(z, z, 0.0, err2, errmax, rms)


class Verdict(NamedTuple):
    name: str
    kernel: Metrics
    mirror: Metrics
    r_frob: float    # kernel / mirror
    r_maxn: float
    scale_bound: Optional[float]  # None: not judged (rms(truth) under the floor)
    failed: List[str]  # of "frob", "maxn", "scale"

    def line(self) -> str:
        return (f"{self.name}: frob {self.kernel.frob:.3e} ({self.r_frob:.2f}x mirror, <= {FROB_MARGIN:g}x)  "
                f"maxn {self.kernel.maxn:.3e} ({self.r_maxn:.2f}x, <= {MAXN_MARGIN:g}x)  "
                + (f"scale {self.kernel.scale:+.2e} (mirror {self.mirror.scale:+.2e}, bound {self.scale_bound:.2e})"
                   if self.scale_bound is not None else "scale not judged (zero truth)")
                + (f"  FAILED {','.join(self.failed)}" if self.failed else ""))


def _ratio(a: float, b: float) -> float:
    return a / b if b > 0.0 else (0.0 if a == 0.0 else float("inf"))


def _log(line: str):
    path = os.environ.get(LOG_ENV)
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def judge(kernel, mirror, truth, name: str = "", floor: float = 0.0) -> Verdict:
    """The verdict :func:`assert_within` asserts on, without raising.

    ``floor``: an absolute error every element is allowed on top of the mirror's.  It
    is zero except where the truth is identically zero and the outputs are the fp32
    cancellation residue of the inputs (dQ / dK at N=1), where the caller derives it
    from the operands; ``scale`` is not judged when rms(truth) is below it."""
    k, m = metrics(kernel, truth), metrics(mirror, truth)
    n = max(truth.numel(), 1)
    failed = []
    if not k.err2 <= FROB_MARGIN * m.err2 + floor * math.sqrt(n):
        failed.append("frob")
    if not k.errmax <= MAXN_MARGIN * m.errmax + floor:
        failed.append("maxn")
    bound = SCALE_MARGIN * abs(m.scale) + SCALE_FLOOR if k.rms > floor else None
    if bound is not None and not abs(k.scale) <= bound:
        failed.append("scale")
    v = Verdict(name, k, m, _ratio(k.err2, m.err2), _ratio(k.errmax, m.errmax), bound, failed)
    _log(v.line())
    return v


def assert_within(kernel, mirror, truth, name: str = "", floor: float = 0.0) -> Verdict:
    """``kernel`` against ``truth``, bounded by what ``mirror`` achieves against the same
    truth: frob <= 2x, maxn <= 3x, |scale| <= 3x |scale(mirror)| + 5e-4."""
    v = judge(kernel, mirror, truth, name, floor)
    assert not v.failed, v.line()
    return v


# ----------------------------------------------------------------------------- lse
def lse_bound(lse_truth: torch.Tensor) -> float:
    """max(a quarter of the smallest shift one extra zero-score key would cause in any
    row, log(1 + exp(-lse)), 8 fp32 ulps of the largest |lse|)."""
    t = lse_truth.double()
    pad = torch.log1p(torch.exp(-t)).min().item()
    return max(LSE_PAD_SHARE * pad, LSE_ULPS * t.abs().max().item())


def lse_verdict(lse, lse_truth, name: str = "lse"):
    err = (lse.double() - lse_truth.double()).abs().max().item()
    if not math.isfinite(err):
        err = float("inf")
    bound = lse_bound(lse_truth)
    line = f"{name}: max err {err:.3e} bound {bound:.3e} ({_ratio(err, bound):.3f} of it)"
    _log(line + ("" if err <= bound else "  FAILED lse"))
    return err, bound, line


def assert_lse(lse, lse_truth, name: str = "lse"):
    err, bound, line = lse_verdict(lse, lse_truth, name)
    assert err <= bound, line
    return err, bound
