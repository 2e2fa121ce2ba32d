"""The optimizer-side checks (ops/opt_check.py) on the CPU: the reference passes every runner
of tests/test_opt_values_gpu.py, the fp32 emulation of ``adamw_kernel`` passes the same bounds,
every arithmetic mutant is rejected at the hard row -- and accepted by the tolerance the suite
had at the only row it had, which is why the other rows exist -- wrong embedding truths are
rejected, and a probe that breaks an exactness condition fails before anything is compared."""
import pytest
import torch

from ddim_cold_amd import ops
from ddim_cold_amd.ops import opt_check as oc

CPU = "cpu"
N = 100_003


def rejected(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def _case(row, n=N):
    r = oc.ROWS[row]
    a = oc.arenas(n, r.fresh, seed=n)
    hyper = torch.tensor(r.hyper, dtype=torch.float32)
    return r, a, hyper, oc.adamw_truth(a.p, a.g, a.m, a.v, hyper, r.step, r.sq, r.grad_scale)


# ----------------------------------------------------------------------------- 1. AdamW
@pytest.mark.parametrize("mode", oc.ADAMW_MODES)
@pytest.mark.parametrize("row", sorted(oc.ROWS))
def test_adamw_reference_passes(row, mode):
    worst = [0.0, 0.0, 0.0]
    for n in oc.ADAMW_SIZES:
        for off in ((0,) if mode == "lazy" else (0, 1)):
            worst = [max(w, r) for w, r in zip(worst, oc.run_adamw(CPU, row, mode, n, off))]
    print(f"reference adamw_step row={row} mode={mode}: worst error / bound m {worst[0]:.4f} v {worst[1]:.4f} "
          f"p {worst[2]:.4f}")
    assert max(worst) <= 1.0


@pytest.mark.parametrize("row", sorted(oc.ROWS))
def test_adamw_emulation_passes(row):
    r, a, hyper, tr = _case(row)
    p, m, v = oc.adamw_f32(a.p, a.g, a.m, a.v, hyper, r.step, r.sq, r.grad_scale)
    worst = oc.check_adamw(dict(p=p, m=m, v=v), tr, f"fp32 emulation row={row}")
    print(f"fp32 emulation row={row}: worst error / bound (m, v, p) {worst}")
    assert max(worst) <= 1.0


def test_adamw_bounds_sit_above_the_reference_and_far_below_the_mutants():
    """The derived multiples: at least the 2.0 u / 3.1 u / 2.6 u the reference reaches, and no
    more than a few hundred u anywhere (the mutants are 1e4 u and more away)."""
    for row in oc.ROWS:
        _, a, _, tr = _case(row, 1027)
        assert tr.sc.e_coef in (0.0, 12.0)
        m_m, m_v = tr.sc.e_coef + 4.0, 2.0 * tr.sc.e_coef + 6.0
        assert 4.0 <= m_m <= 16.0 and 6.0 <= m_v <= 30.0
        k_p = m_m + 0.5 * m_v + 31.0 + tr.sc.e_lr
        assert 38.0 <= k_p <= (700.0 if row == "late" else 100.0), (row, k_p)
    late = _case("late", 1027)[3].sc
    rest = [oc.adamw_scalars(torch.tensor(r.hyper), r.step, r.sq, r.grad_scale).e_lr for k, r in oc.ROWS.items()
            if k != "late"]
    assert 300.0 < late.e_lr < 700.0 and max(rest) < 30.0   # the cancellation shows at the late row only


def test_adamw_late_row_needs_the_lr_term():
    """At the late row an fp32 evaluation of the schedule is off by tens of u of the rate (the
    absolute error of ``1 + cosf`` against ``lr ~ eta_min``), an order of magnitude above what
    every other rounding of the update adds up to in the reference: the rate's own term in
    the bound is what covers it, and it does."""
    r, a, hyper, tr = _case("late")
    p, m, v = oc.adamw_f32(a.p, a.g, a.m, a.v, hyper, r.step, r.sq, r.grad_scale)
    lr32 = float(hyper[7] + (hyper[0] - hyper[7]) * 0.5 * (1.0 + torch.cos(
        torch.tensor(3.14159265358979, dtype=torch.float32) * 99_993.0 / hyper[6])))
    rel = abs(lr32 - tr.sc.lr) / tr.sc.lr / oc.U32
    print(f"late row: fp32 rate off by {rel:.1f} u of the true rate; bound {tr.sc.e_lr:.1f} u")
    assert 30.0 < rel <= tr.sc.e_lr


@pytest.mark.parametrize("mutant", oc.MUTANTS + (oc.L2,))
def test_adamw_mutant_rejected_at_the_hard_row(mutant):
    r, a, hyper, tr = _case("hard")
    p, m, v = oc.adamw_f32(a.p, a.g, a.m, a.v, hyper, r.step, r.sq, r.grad_scale, mutant)
    rejected(oc.check_adamw, dict(p=p, m=m, v=v), tr, f"mutant {mutant}")


@pytest.mark.parametrize("mutant", oc.MUTANTS)
def test_adamw_mutant_passes_the_old_tolerance_at_the_suites_row(mutant):
    """Why the rows exist: at the suite's row (its hyper-parameters, ``grad_scale = 1``,
    ``step[0] == step[1]``, inputs drawn as its optimizer tests draw them, the norm the
    gradient's own), ``rtol=1e-5, atol=1e-6`` accepts each of the five on p, m and v.  Three
    of them compute the same bits there at any step.  ``eps`` inside the bias correction and
    the decay after the update differ by up to 60 u and 1.8e3 u of the scales, inside that
    tolerance from step 6 of the 10-step schedule on (shown here); in the first steps, where
    1 / bc1 blows the update up, it catches them on the few elements with the smallest v.  The
    derived bounds reject both at this very row and step."""
    a = oc.arenas(N, seed=0)
    hyper = torch.tensor(oc.SUITE_HYPER, dtype=torch.float32)
    sq = float((a.g.double() ** 2).sum())
    good = oc.adamw_f32(a.p, a.g, a.m, a.v, hyper, (6, 6), sq, 1.0)
    bad = oc.adamw_f32(a.p, a.g, a.m, a.v, hyper, (6, 6), sq, 1.0, mutant)
    for x, y in zip(bad, good):
        assert torch.allclose(x, y, rtol=1e-5, atol=1e-6)
    if mutant in ("eps_in_bc", "decay_after"):
        tr = oc.adamw_truth(a.p, a.g, a.m, a.v, hyper, (6, 6), sq, 1.0)
        oc.check_adamw(dict(zip("pmv", good)), tr, "fp32 emulation at the suite's row")
        rejected(oc.check_adamw, dict(zip("pmv", bad)), tr, f"mutant {mutant} at the suite's row")
    else:
        assert all(torch.equal(x, y) for x, y in zip(bad, good))


def test_partials_exactness_condition_is_asserted():
    assert oc.exact_partials(oc.partials(CPU, 1024, {3: 4.0, 1023: 0.25})) == 4.25
    rejected(oc.exact_partials, oc.partials(CPU, 1024, {3: 3.0}))                    # no power of two
    rejected(oc.exact_partials, oc.partials(CPU, 1024, {3: 1.0, 4: 2.0 ** -30}))     # too far apart
    rejected(oc.exact_partials, oc.partials(CPU, 1024, {i: 1.0 for i in range(5)}))  # too many
    rejected(oc.exact_partials, oc.partials(CPU, 1024, {3: float("inf")}))


# ----------------------------------------------------------------------------- 2. partials
@pytest.mark.parametrize("nparts", [ops.SQ_PARTS, ops.sq_parts_size(3000)])
def test_partials_reference_passes(nparts):
    assert max(oc.run_partials(CPU, nparts)) <= 1.0
    for bad in (float("inf"), float("nan")):
        oc.run_skip(CPU, nparts, bad)
    oc.run_advance(CPU, nparts)


def test_partials_early_stop_is_rejected():
    """What a sum that stops before the last slot computes (sq = 0: coef = grad_scale)."""
    r, a, hyper, tr = _case("hard", 1027)
    p, m, v = oc.adamw_f32(a.p, a.g, a.m, a.v, hyper, r.step, 0.0, r.grad_scale)
    rejected(oc.check_adamw, dict(p=p, m=m, v=v), tr, "sum_parts stops early")


# ----------------------------------------------------------------------------- 3. sqnorm
def test_sqnorm_sizes_reach_every_loop():
    small = ops.SQ_PARTS * 256 * 4
    a, b = oc.sqnorm_sizes(ops.SQ_PARTS)[-2:]
    assert small < a < 4 * small and a % 4 and (a // 4) % 256
    assert b > 4 * small + 3 and b % 4 == 3 and b * 4 < 17_000_000


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("nparts", [ops.SQ_PARTS, ops.sq_parts_size(3000)])
def test_sqnorm_reference_passes(nparts, off):
    for n in oc.SQNORM_SMALL + (300_001,):
        oc.run_sqnorm(CPU, n, nparts, off)
    oc.run_sqnorm_positions(CPU, 300_001, ops.SQ_PARTS, off)
    oc.run_sqnorm_positions(CPU, 7, ops.SQ_PARTS, off, with_lazy=False)


def test_sqnorm_refusals_and_conditions():
    oc.run_sqnorm_refusals(CPU)
    rejected(oc.sqnorm_truth, torch.full((8,), 4.0), 1.0)               # outside [-3, 3]
    rejected(oc.sqnorm_truth, torch.full((8,), 0.5), 1.0)               # no integer
    rejected(oc.sqnorm_truth, torch.ones(8), 1.5)                       # scale^2 rounds
    rejected(oc.sqnorm_truth, torch.full((2 ** 21,), 3.0), 3.0)         # 9 * 9 * 2^21 >= 2^24


def test_sqnorm_positions_cover_the_seams():
    n, parts = oc.sqnorm_sizes(ops.SQ_PARTS)[-1], ops.SQ_PARTS
    lazy = oc.sqnorm_lazy_ranges(n, parts)["across a trip"]
    pos = oc.sqnorm_positions(n, parts, lazy)
    st = parts * 256
    assert lazy[0] < 4 * st < lazy[1]
    for want in (lazy[0] - 4, lazy[0] - 1, lazy[1], lazy[1] + 3, n - 1, n - 2, n - 3, n - 4, 0,
                 4 * (4 * st - 1 + (lazy[1] - lazy[0]) // 4), 4 * (4 * st + (lazy[1] - lazy[0]) // 4)):
        assert want in pos, want
    assert not any(lazy[0] <= i < lazy[1] for i in pos)


def test_sqnorm_dropped_vector_is_rejected():
    """A sum that misses one vector at a seam differs from the truth by an integer: caught by
    equality, where 1e-5 relative on random data was blind to it."""
    g = oc.int_gradient(300_001, seed=1)
    g[1024:1028] = 1.0
    want = oc.sqnorm_truth(g, 3.0)
    miss = g.clone()
    miss[1024:1028] = 0.0
    got = oc.sqnorm_truth(miss, 3.0)
    assert got != want and abs(got - want) / want < 1e-5


# ----------------------------------------------------------------------------- 4. embed_bwd
def _tsets(B):
    return [t for t in oc.EMBED_TSETS if t != "passes" or B > 256]


@pytest.mark.parametrize("p", oc.EMBED_PS)
@pytest.mark.parametrize("shape", oc.EMBED_SHAPES)
def test_embed_reference_passes(shape, p):
    for tset in _tsets(shape[0]):
        oc.run_embed(CPU, *shape, tset, p)


@pytest.mark.parametrize("mutant", oc.EMBED_MUTANTS)
@pytest.mark.parametrize("p", oc.EMBED_PS)
def test_embed_wrong_truth_rejected(p, mutant):
    c = oc.embed_case(9, 17, 64, "mix6", p)
    out = oc.embed_outputs(CPU, c)
    oc.check_embed(*out, c, oc.embed_truth(c), "reference")
    rejected(oc.check_embed, *out, c, oc.embed_truth(c, mutant), f"wrong truth {mutant}")


def test_embed_timestep_sets():
    t = oc.embed_timesteps(300, "passes")
    assert 5 in t[:256].tolist() and 5 in t[256:].tolist()
    assert 9 not in t[:256].tolist() and 9 in t[256:].tolist()
    assert sorted(set(oc.embed_timesteps(300, "ends").tolist())) == [0, oc.TEMB_ROWS - 1]
    assert len(set(oc.embed_timesteps(300, "distinct").tolist())) == 300
    assert len(set(oc.embed_timesteps(300, "mix6").tolist())) == 6
    assert len(set(oc.embed_timesteps(300, "equal").tolist())) == 1


def test_embed_exactness_condition_is_asserted():
    c = oc.embed_case(7, 5, 36, "mix6", 0.5)
    rejected(oc.embed_truth, c._replace(g=c.g + 0.5))
    rejected(oc.embed_truth, c._replace(g=c.g * 2))
    rejected(oc.embed_truth, c._replace(p=0.1))
    rejected(oc.embed_truth, c._replace(dcls=c.dcls + 0.25))


@pytest.mark.parametrize("tokens", [64, ops.WGRAD_WIDE_TOKENS])
def test_embed_through_the_wgrad_launch_reference_passes(tokens):
    oc.run_embed_wgrad(CPU, 9, 17, 64, "mix6", 0.5, tokens)
    oc.run_embed_wgrad(CPU, 7, 5, 36, "equal", 0.0, tokens)


# ----------------------------------------------------------------------------- 5. bf16 wire
def test_wire_source_covers_every_tie():
    src = oc.wire_source()
    bits = src.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    assert src.numel() == oc.WIRE_N == 2 * 65536 * 5 + 5
    assert oc.WIRE_N // 8 > 256 * 256 and oc.WIRE_N % 8 == 5          # a second trip, a tail of five
    first = bits[:65536 * 5].view(65536, 5)
    assert torch.equal(first >> 16, torch.arange(65536).unsqueeze(1).expand(65536, 5))
    assert (first & 0xFFFF)[12345].tolist() == list(oc.WIRE_LOWS)
    want = src.to(torch.bfloat16)
    assert bool(torch.isinf(want[(bits == 0x7F7F8000) | (bits == 0x7F7FFFFF)].float()).all())  # overflow
    tie_even, tie_odd = bits == 0x3F808000, bits == 0x3F818000
    assert (want[tie_even].view(torch.int16) == 0x3F80).all() and (want[tie_odd].view(torch.int16) == 0x3F82).all()


@pytest.mark.parametrize("off", [0, 1])
def test_wire_fallbacks_pass(off):
    oc.run_wire_pack(CPU, off=off)
    oc.run_wire_unpack(CPU, off=off)
    for n in oc.WIRE_SMALL:
        oc.run_wire_pack(CPU, n, off)
        oc.run_wire_unpack(CPU, n, off)
    oc.run_wire_refusals(CPU)


def test_wire_truncation_is_rejected():
    """Round toward zero instead of to nearest even: caught at the first tie."""
    src = oc.wire_source(4096 * 5)
    trunc = (src.view(torch.int32) >> 16).to(torch.int16).view(torch.bfloat16)
    nan = torch.isnan(src)
    rejected(oc.exact, trunc[~nan], src.to(torch.bfloat16)[~nan], "truncating pack")
