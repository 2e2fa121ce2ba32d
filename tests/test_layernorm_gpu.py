"""``layernorm_fwd`` / ``layernorm_bwd`` (csrc/layernorm.hip) against an fp64 truth
(ops/ln_check.py) at every dispatched width, around the rows-per-workgroup groups, through
the workgroup-strided second pass with a ragged last group, and with every fused extra
(K-split partials, bf16 ``dy`` / ``x``, ``g_res``, the three dropouts, ``y_out``, ``gp_out``,
workspace slots or accumulation).

bf16-valued outputs (``y``, ``gy``, ``gp``, ``y_out``) are judged against the truth relative to
what the reference achieves (frob 2x, maxn 3x) with exact drop sets; fp32-valued ones
(``mean``, ``rstd``, ``g_out``, ``dgamma``, ``dbeta``) at the a-priori ``16 * 2^-24 * sum |terms|``
of ``ln_check.term_bound``.  tests/test_ln_check_cpu.py runs the reference through the same
grid at a quarter of those bounds and shows each comparator rejecting its mutants."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import ops
from ddim_cold_amd.ops import ln_check as lc

DEV = "cuda"


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


@pytest.mark.parametrize("r", [0.0, 16.0])
@pytest.mark.parametrize("D", lc.LN_DS)
def test_layernorm_fwd_widths(D, r):
    lc.run_ln_fwd(37, D, r, DEV)


@pytest.mark.parametrize("r", [0.0, 16.0])
@pytest.mark.parametrize("M", lc.LN_FWD_MS)
def test_layernorm_fwd_row_groups(M, r):
    """Around the 4 rows of a forward workgroup."""
    lc.run_ln_fwd(M, 128, r, DEV)


def test_layernorm_fwd_rejects_undispatched_width():
    x = torch.randn(8, 640, device=DEV)
    with pytest.raises(RuntimeError):
        ops.layernorm_fwd(x, torch.ones(640, device=DEV), torch.zeros(640, device=DEV))
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", lc.ln_bwd_cases(), ids=lambda c: "-".join(str(v) for v in c))
def test_layernorm_bwd(case):
    if case.M == lc.LN_BWD_STRIDED_M:
        assert ops.ln_ws_rows(case.M) == 512 and case.M > 8 * 512 and case.M % 8  # second pass, ragged group
    lc.run_ln_bwd(case, DEV)


def test_layernorm_bwd_after_folded_qkv():
    lc.run_ln_chain(DEV)
