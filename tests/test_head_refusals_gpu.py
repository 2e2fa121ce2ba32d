"""The argument checks of the four head ops (``head_fwd``, ``head_step_``, ``head_step_rows_``,
``head_loss``; csrc/bindings.cpp): every mis-shaped call is refused on the host and launches
nothing -- the outputs, filled with canaries, are intact after a synchronize.  The ops are called
directly (``torch.ops.ddim_cold``), past the Python wrappers' own checks.  The stochastic modes
of ``head_step_rows_`` have theirs in tests/test_ddim_eta_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
B, C, HW, P, D = 2, 3, 16, 4, 64
NP, F = (HW // P) ** 2, C * P * P  # patches per sample, head columns
M = B * (NP + 1)


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


@pytest.fixture(scope="module")
def operands():
    g = torch.Generator().manual_seed(7)
    a = (0.1 * torch.randn(M, D, generator=g)).to(torch.bfloat16).to(DEV)
    w = (0.1 * torch.randn(F, D, generator=g)).to(torch.bfloat16).to(DEV)
    return a, w, torch.zeros(F, device=DEV)


class Outputs:
    """x, x0_out and patches_out of a step in the image (``rows=False``) or patch-row layout."""

    def __init__(self, rows):
        shape = (B * NP, F) if rows else (B, C, HW, HW)
        self.x = torch.full(shape, 3.0, device=DEV)
        self.x0 = torch.full(shape, 5.0, device=DEV)
        self.po = torch.full((B * NP, F), 7.0, dtype=torch.bfloat16, device=DEV)

    def intact(self):
        torch.cuda.synchronize()
        return bool((self.x == 3.0).all()) and bool((self.x0 == 5.0).all()) and bool((self.po == 7.0).all())


def coef(n):
    return torch.tensor([0.6, 0.8, 0.8, 0.6] * B, device=DEV)[:n].contiguous()


def step(operands, o, mode, **kw):
    a, w, b = operands
    torch.ops.ddim_cold.head_step_(kw.get("a", a), w, b, kw.get("x", o.x), kw.get("x0", o.x0),
                                   kw.get("coef", coef(4 * B)), P, mode, None, None, 1e-5, kw.get("po", o.po))


def step_rows(operands, o, mode, **kw):
    a, w, b = operands
    torch.ops.ddim_cold.head_step_rows_(a, w, b, kw.get("x", o.x), o.x0, kw.get("coef", coef(4 * B)), B, mode, None,
                                        None, 1e-5, o.po, None, 0)


# case -> the faulty arguments (built on the GPU: when the test runs)
STEP_BAD = {
    "mode 0": lambda: dict(mode=0),
    "mode 3": lambda: dict(mode=3),
    "mode 7": lambda: dict(mode=7),
    "mode 1 without x0_out": lambda: dict(mode=1, x0=None),
    "mode 4 with fewer than 4*B coefficients": lambda: dict(mode=4, coef=coef(4 * B - 1)),
    "x0_out of another shape": lambda: dict(mode=1, x0=torch.full((B, C, HW * HW), 5.0, device=DEV)),
    "patches_out of the wrong numel": lambda: dict(
        mode=1, po=torch.full((B * NP - 1, F), 7.0, dtype=torch.bfloat16, device=DEV)),
    "a with one row too few": lambda: dict(mode=1, a=torch.zeros(M - 1, D, dtype=torch.bfloat16, device=DEV)),
}
ROWS_BAD = {
    "mode 1 with a short coef": lambda: dict(mode=1, coef=coef(3)),
    "mode 4 with a short coef": lambda: dict(mode=4, coef=coef(4 * B - 1)),
    "x whose rows are no multiple of batch": lambda: dict(mode=2, x=torch.full((B * NP - 1, F), 3.0, device=DEV)),
}


@pytest.mark.parametrize("case", STEP_BAD)
def test_head_step_refuses(operands, case):
    o, kw = Outputs(rows=False), STEP_BAD[case]()
    with pytest.raises(RuntimeError):
        step(operands, o, kw.pop("mode"), **kw)
    assert o.intact(), case
    for t, v in ((kw.get("x0"), 5.0), (kw.get("po"), 7.0)):  # the mis-shaped output itself
        assert t is None or bool((t == v).all()), case


@pytest.mark.parametrize("case", ROWS_BAD)
def test_head_step_rows_refuses(operands, case):
    o, kw = Outputs(rows=True), ROWS_BAD[case]()
    with pytest.raises(RuntimeError):
        step_rows(operands, o, kw.pop("mode"), **kw)
    assert o.intact(), case
    assert "x" not in kw or bool((kw["x"] == 3.0).all()), case


def test_head_fwd_and_head_loss_refuse(operands):
    a, w, b = operands
    target = torch.zeros(B, C, HW, HW, device=DEV)
    with pytest.raises(RuntimeError):  # w with the wrong row count
        torch.ops.ddim_cold.head_fwd(a, w[:F - 8].contiguous(), b, B, C, HW, HW, P)
    with pytest.raises(RuntimeError):  # beta = 0
        torch.ops.ddim_cold.head_loss(a, w, b, target, P, 0.0)
    with pytest.raises(RuntimeError):  # a 3-D target
        torch.ops.ddim_cold.head_loss(a, w, b, target.view(B * C, HW, HW), P, 1.0)
    torch.cuda.synchronize()


def test_the_unbroken_calls_are_accepted(operands):
    """The calls above fail for the fault they name: without it each op runs and writes its outputs."""
    a, w, b = operands
    for mode in (1, 2, 4):
        for fn, rows in ((step, False), (step_rows, True)):
            o = Outputs(rows)
            fn(operands, o, mode)
            torch.cuda.synchronize()
            assert float(o.x.abs().max()) <= 3.0 and not bool((o.x == 3.0).all()) and not bool((o.po == 7.0).all())
            assert bool((o.x0 == 5.0).all()) == (mode == 2)
    target = torch.zeros(B, C, HW, HW, device=DEV)
    assert torch.ops.ddim_cold.head_fwd(a, w, b, B, C, HW, HW, P).shape == target.shape
    parts, dtok = torch.ops.ddim_cold.head_loss(a, w, b, target, P, 1.0)
    assert dtok.shape == (M, F) and bool(torch.isfinite(parts).all())
