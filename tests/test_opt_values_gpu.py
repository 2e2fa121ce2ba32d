"""The end of the training step against fp64 truths and exact probes (ops/opt_check.py):
``adamw_step`` at six hyper-parameter rows in its three modes within bounds counted from the
kernel's roundings, the partial sum and the skipped step on raw bits, ``sqnorm`` on integer
gradients over every loop, lazy-range seam and alignment (the fp64 sum of the partials equals
the int64 truth), ``embed_bwd`` on integer gradients at the smallest shape of each mechanism,
alone and inside the weight-gradient launch, and the bf16 wire over every tie.

The derivations are in the module's docstring; the CPU reference and an fp32 emulation pass the
same runners, and arithmetic mutants fail them, in tests/test_opt_check_cpu.py.  Each AdamW test
prints the kernel's worst error / bound next to the CPU reference's at the same row.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from ddim_cold_amd import ops
from ddim_cold_amd.ops import opt_check as oc

DEV = "cuda"
CPU = "cpu"
PARTS = [ops.SQ_PARTS, ops.sq_parts_size(3000)]


@pytest.fixture(autouse=True)
def _native():
    from ddim_cold_amd.ops import _ext
    _ext.load(raise_on_error=True)


def _both(row, mode, n, off, worst):
    for k, dev in enumerate((DEV, CPU)):
        worst[k] = [max(w, r) for w, r in zip(worst[k], oc.run_adamw(dev, row, mode, n, off))]


def _report(what, worst):
    (km, kv, kp), (rm, rv, rp) = worst
    line = (f"{what}: worst error / bound, kernel m {km:.4f} v {kv:.4f} p {kp:.4f} | reference m {rm:.4f} v {rv:.4f} "
            f"p {rp:.4f}")
    print(line)
    oc._log("SUMMARY " + line)


# ----------------------------------------------------------------------------- 1. AdamW
@pytest.mark.parametrize("mode", oc.ADAMW_MODES)
@pytest.mark.parametrize("row", sorted(oc.ROWS))
def test_adamw_values(row, mode):
    worst = [[0.0] * 3, [0.0] * 3]
    for n in oc.ADAMW_SIZES:
        for off in ((0,) if mode == "lazy" else (0, 1)):
            _both(row, mode, n, off, worst)
    _report(f"adamw_step row={row} mode={mode}", worst)


def test_adamw_values_past_the_grid_cap():
    worst = [[0.0] * 3, [0.0] * 3]
    _both("hard", "plain", oc.ADAMW_BIG, 0, worst)
    _report(f"adamw_step row=hard mode=plain n={oc.ADAMW_BIG}", worst)


# ----------------------------------------------------------------------------- 2. partials
@pytest.mark.parametrize("nparts", PARTS)
def test_partials_last_slot(nparts):
    worst = oc.run_partials(DEV, nparts)
    print(f"sum_parts, only slot {nparts - 1} non-zero: worst error / bound (m, v, p) {worst}")


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
@pytest.mark.parametrize("nparts", PARTS)
def test_partials_non_finite_last_slot_skips(nparts, bad):
    oc.run_skip(DEV, nparts, bad)


@pytest.mark.parametrize("nparts", PARTS)
def test_advance_counters(nparts):
    oc.run_advance(DEV, nparts)


# ----------------------------------------------------------------------------- 3. sqnorm
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("nparts", PARTS)
@pytest.mark.parametrize("n", oc.sqnorm_sizes(ops.SQ_PARTS))
def test_sqnorm_exact(n, nparts, off):
    oc.run_sqnorm(DEV, n, nparts, off)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("nparts", PARTS)
def test_sqnorm_positions(nparts, off):
    big = oc.sqnorm_sizes(ops.SQ_PARTS)[-1]
    oc.run_sqnorm_positions(DEV, big, nparts, off)
    oc.run_sqnorm_positions(DEV, 1027, nparts, off)
    oc.run_sqnorm_positions(DEV, 7, nparts, off, with_lazy=False)


def test_sqnorm_refuses_bad_ranges():
    oc.run_sqnorm_refusals(DEV)


# ----------------------------------------------------------------------------- 4. embed_bwd
@pytest.mark.parametrize("p", oc.EMBED_PS)
@pytest.mark.parametrize("shape", oc.EMBED_SHAPES)
def test_embed_bwd_exact(shape, p):
    for tset in oc.EMBED_TSETS:
        if tset != "passes" or shape[0] > 256:
            oc.run_embed(DEV, *shape, tset, p)


@pytest.mark.parametrize("tokens", [64, ops.WGRAD_WIDE_TOKENS])
@pytest.mark.parametrize("p", oc.EMBED_PS)
def test_embed_through_the_wgrad_launch(p, tokens):
    """The shapes the binding takes (B <= 256: one part-B pass) under the 256-thread and the
    512-thread form of the parts: the same bits, and the grad-norm slots of the part
    workgroups against the squares of what they wrote."""
    nt = 512 if tokens >= ops.WGRAD_WIDE_TOKENS else 256
    assert int(torch.ops.ddim_cold.wgrad_multi_plan([oc.WGRAD_JOB[0]], [oc.WGRAD_JOB[1]], [tokens])[0]) == nt // 4
    worst = 0.0
    for shape in [s for s in oc.EMBED_SHAPES if s[0] <= 256]:
        for tset in ("equal", "distinct", "mix6", "ends"):
            worst = max(worst, oc.run_embed_wgrad(DEV, *shape, tset, p, tokens))
    print(f"embedding parts in the weight-gradient launch, tokens={tokens} p={p}: grad-norm slots worst error / bound "
          f"{worst:.4f}")


# ----------------------------------------------------------------------------- 5. bf16 wire
@pytest.mark.parametrize("off", [0, 1])
def test_wire_pack_every_tie(off):
    oc.run_wire_pack(DEV, off=off)
    for n in oc.WIRE_SMALL:
        oc.run_wire_pack(DEV, n, off)


@pytest.mark.parametrize("off", [0, 1])
def test_wire_unpack_every_pattern(off):
    oc.run_wire_unpack(DEV, off=off)
    oc.run_wire_unpack(DEV, 3 * 65536 * 8 + 5, off)   # a second grid-stride trip and a tail of five
    for n in oc.WIRE_SMALL:
        oc.run_wire_unpack(DEV, n, off)


def test_wire_refuses_a_size_mismatch():
    oc.run_wire_refusals(DEV)
