"""Per-element arithmetic of the epilogues against fp64 truths (ops/epi_check.py): GELU over
every finite bf16 input under every GEMM tile, GELU' in the DGELU epilogue on both operand
paths, the three smooth-L1 implementations at beta != 1 and the three DDIM updates at the
first, a middle and the last step, plus ``q_sample`` at both ends of the schedule.

The fp32 value entering each epilogue is set to the bit (a one-hot operand, or a zero operand
plus the bias), so the bounds are those of the arithmetic alone: half a bf16 ulp plus a derived
term for bf16 outputs, a few fp32 roundings for fp32 ones, bit equality wherever the result is
unique (``u``, drop sets, the clamp, the saturated gradient, the last DDIM step, the identity
row, ``q_sample`` at a = 0).  The derivations are in the module's docstring; the reference and
an fp32 emulation of the kernels pass the same checks, and arithmetic mutants fail them, in
tests/test_epi_check_cpu.py.  Each test prints its worst observed error / bound.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import ops
from ddim_cold_amd.ops import epi_check as ec
from ddim_cold_amd.ops import gemm_check as gc

DEV = "cuda"


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


def assert_tile(cfg, epi, M, N, K):
    """The launch under the tile override is the LDS-DMA kernel on config ``cfg``'s tile."""
    got = tuple(int(v) for v in torch.ops.ddim_cold.gemm_plan(epi, False, False, M, N, K, 1))
    assert got[:4] == (1, *gc.TILES[cfg]), f"plan {got} is not config {cfg} = {gc.TILES[cfg]}"


@pytest.mark.parametrize("p", ec.DROPOUT_PS)
@pytest.mark.parametrize("cfg", sorted(gc.TILES))
def test_gelu_every_bf16_input(cfg, p):
    with ops.gemm_tile(cfg):
        assert_tile(cfg, gc.EPI_GELU, ec.GELU_M, ec.GELU_N, ec.GELU_K)
        worst = ec.run_gelu(DEV, p)
    print(f"GELU cfg {cfg} p={p}: worst error / bound {worst:.4f}")


def test_gelu_keeps_denormals():
    """What the module's docstring states: a denormal pre-activation comes back as itself."""
    c = ec.gelu_case()
    u, _ = ops.linear_gelu_fwd(c.a.to(DEV), c.w.to(DEV), c.bias.to(DEV), ec._rng(DEV), ec.GELU_SITE, 0.0)
    kept, flushed = ec.check_gelu_u(u)
    print(f"GELU u: denormal inputs kept {kept}, flushed {flushed}")
    assert (kept, flushed) == (254, 0)


@pytest.mark.parametrize("p", ec.DROPOUT_PS)
def test_dgelu_every_bf16_input(p):
    worst = ec.run_dgelu(DEV, p)
    print(f"GELU' p={p}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("beta", ec.BETAS)
@pytest.mark.parametrize("geom", ec.GEOMS)
def test_smooth_l1_values(geom, beta):
    r_loss, r_grad = ec.run_smooth_l1(DEV, geom, beta)
    print(f"smooth-L1 {geom} beta={beta}: worst error / bound, loss {r_loss:.4f}, gradient {r_grad:.4f}")


@pytest.mark.parametrize("geom", ec.GEOMS)
def test_ddim_update_values(geom):
    worst = ec.run_ddim(DEV, geom)
    print(f"DDIM update {geom}: worst error / bound {worst:.4f}")


def test_q_sample_schedule_ends():
    worst = ec.run_q_sample(DEV, ec.GEOMS[0])
    print(f"q_sample: worst error / bound {worst:.4f}")
