"""The exact GEMM probes (ops/gemm_check.py) on the CPU: the reference passes every probe
at every shape of tests/test_gemm_exact_gpu.py (which proves the exactness condition
holds for the chosen ranges), and each kernel-shaped mutant of a reference output is
rejected by the probe documented to catch it."""
import pytest
import torch

from ddim_cold_amd.ops import gemm_check as gc
from ddim_cold_amd.ops import reference as ref

CPU = "cpu"
PAIRED = ((False, True), (True, False))


# ----------------------------------------------------------------------------- the reference passes
def _linear_shapes():
    s = set()
    for bm, bn, _ in gc.TILES.values():
        s |= {(M, N, K) for M in gc.edge_ms(bm) for N in gc.edge_ns(bn) for K in gc.EDGE_KS}
    return sorted(s)


def test_reference_passes_tile_edge_grid():
    for M, N, K in _linear_shapes():
        gc.run_linear(M, N, K, CPU)


@pytest.mark.parametrize("cfg", gc.TWO_DEPTH_TILES)
def test_reference_passes_ring_depth_shapes(cfg):
    M, N = gc.depth_shape(cfg)
    assert -(-M // gc.TILES[cfg][0]) * -(-N // gc.TILES[cfg][1]) > 256 * ((160 * 1024) // (512 * sum(gc.TILES[cfg][:2])))
    for K in gc.DEPTH_KS + gc.SHORT_KS:
        gc.run_linear(M, N, K, CPU, combos=PAIRED)
    bm, bn, _ = gc.TILES[cfg]
    for K in gc.SHORT_KS:
        gc.run_linear(bm + 1, bn + 4, K, CPU, combos=PAIRED)


def test_reference_passes_fixed_depth_and_plain_shapes():
    assert gc.TWO_DEPTH_TILES == [0, 1, 2, 3, 5] and gc.FIXED_DEPTH_TILES == [(4, 3), (6, 2)]
    for cfg, _ in gc.FIXED_DEPTH_TILES:
        bm, bn, _ = gc.TILES[cfg]
        for K in gc.FIXED_DEPTH_KS:
            gc.run_linear(2 * bm + 17, bn + 4, K, CPU, combos=((False, True), (False, False)))
    for M, N in gc.PLAIN_SHAPES:
        for K in gc.PLAIN_KS:
            gc.run_linear(M, N, K, CPU, combos=PAIRED)
            gc.run_linear(M, N, K, CPU, combos=PAIRED, seed=12)


def test_reference_passes_epilogue_probes():
    for s in gc.QKV_SHAPES + (gc.QKV_SHAPE_HD16,):
        gc.run_qkv(*s, CPU)
    for s in gc.RESID_SHAPES:
        gc.run_residual(*s, CPU)
    for s in gc.GELU_SHAPES:
        gc.run_gelu(*s, CPU)
    for s in gc.HEAD_GEOMS:
        gc.run_head(*s, CPU)
    for s in gc.EMBED_GEOMS:
        gc.run_patch_embed(*s, CPU)
    for s in gc.EMBED_STAT_GEOMS:
        gc.run_patch_embed(*s, CPU, stats=True)


@pytest.mark.parametrize("p", gc.DROPOUT_PS)
def test_reference_passes_dropout_placement(p):
    for cfg, (bm, bn, _) in gc.TILES.items():
        M, N = 2 * bm + 17, bn + 4
        tokens = gc.small_prime_factor(M)
        assert 1 < tokens < M
        for kind in ("resid_drop", "resid_dp", "gelu"):
            gc.run_dropout(kind, M, N, p, CPU, tokens=tokens)
        B, H, W, pp = gc.embed_dropout_geom(M)
        gc.run_dropout_embed(B, H, W, pp, N, p, CPU)
        gc.run_dropout("dgelu", M, gc.dgrad_width(cfg) if cfg < 6 else bn + 8, p, CPU)


def test_reference_passes_dgrad_probes():
    for K in (gc.dgrad_width(0), gc.dgrad_width(5)):
        for Nout in gc.DGRAD_NOUT:
            splits = gc.dgrad_splits(Nout)
            assert all(2 <= s <= 4 for s in splits)
            for M in gc.DGRAD_MS:
                gc.run_dgrad(M, Nout, K, CPU, splits=[1] + splits)
        for M, Nout in gc.DGELU_SHAPES:
            for wt in (False, True):
                gc.run_dgrad_gelu(M, Nout, K, CPU, with_wt=wt)
    assert gc.dgrad_splits(64) == [] and gc.dgrad_splits(200) == [2, 4] and gc.dgrad_splits(320) == [2, 3]
    assert gc.dgrad_splits(1152) == [2, 3, 4]
    for case in gc.DGRAD_LN_CASES:
        gc.run_dgrad_ln(*case, CPU)


def test_reference_passes_wgrad_probes():
    for T in gc.WGRAD_TOKENS:
        for Nout, K, db in gc.wgrad_shapes():
            gc.run_wgrad(T, Nout, K, CPU, db)
            gc.run_wgrad(T, Nout, K, CPU, not db)
        for store in (False, True):
            gc.run_wgrad_multi(T, gc.wgrad_shapes(), CPU, store)
    for store in (False, True):
        gc.run_wgrad_multi(gc.WGRAD_BIG_TOKENS, gc.WGRAD_BIG_SHAPES, CPU, store, lo=-2, hi=2, repeats=2)
        gc.run_wgrad_sq(200, gc.wgrad_shapes(), CPU, store)
        gc.run_wgrad_sq(gc.WGRAD_BIG_TOKENS, gc.WGRAD_BIG_SHAPES, CPU, store)


def test_reference_passes_fold_consumer_probes():
    """The constructed-statistics probe of the LayerNorm-fold consumers over the grid of
    tests/test_gemm_exact_gpu.py section (h): mean, rstd and output exact for K a power of two
    (which proves the exactness condition holds for the chosen codes), within the operand
    bound at K = 192 / 384."""
    shapes = set()
    for bm, bn, _ in gc.TILES.values():
        shapes |= {(M, N) for M in gc.edge_ms(bm) for N in gc.edge_ns(bn)}
    for K in gc.FOLD_EXACT_KS + gc.FOLD_BOUNDED_KS:
        for M, N in sorted(shapes):
            for kind in ("linear", "gelu"):
                gc.run_fold_consumer(kind, M, N, K, CPU)
    for B, T, H, D in gc.FOLD_QKV_SHAPES + gc.FOLD_QKV_BOUNDED:
        gc.run_fold_consumer("qkv", B * T, 3 * D, D, CPU, geom=(B, T, H))
    for B, C, H, W, p, D in gc.HEAD_GEOMS:
        gc.run_fold_consumer("head", B * ((H // p) * (W // p) + 1), C * p * p, D, CPU, geom=(B, C, H, W, p))


def _fold_probe(M=145, N=136, K=256, seed=13):
    g = torch.Generator().manual_seed(seed)
    a, w = gc.int_operands((M, K), -2, 2, g), gc.int_operands((N, K), -2, 2, g)
    b = gc.int_operands((N,), -8, 8, g, torch.float32)
    mu, sigma, c = gc.fold_codes(M, N, K)
    y, acc = gc.fold_truth_exact(a, w, b, mu, sigma, c)
    return a, w, b, mu, sigma, c, gc.fold_stats(mu, sigma, K), y, acc


def _fold_run(a, w, b, st, c, pure=False):
    M = a.shape[0]
    mean, rstd = torch.empty(M), torch.empty(M)
    y = ref._lin(torch.zeros_like(a) if pure else a, w, b, st, c.float(), 0.0, mean, rstd)
    return y, mean, rstd


def test_fold_probe_exactness_condition_is_enforced():
    a, w, b, mu, sigma, c, st, y, acc = _fold_probe()
    out, mean, rstd = _fold_run(a, w, b, st, c)
    gc.assert_fold(out, y, acc, mu, sigma, c, b, 256, "clean", TILE)
    gc.assert_fold_stats(mean, rstd, mu, sigma, 256, "clean")
    with pytest.raises(AssertionError, match="exactness"):  # codes too wide for fp32
        gc.fold_truth_exact(a, w, b, mu * 4096, sigma, c * 4096)
    with pytest.raises(AssertionError, match="integers"):
        gc.fold_truth_exact(a, w, b, mu + 0.3, sigma, c)
    with pytest.raises(AssertionError, match="integers / scale"):
        gc.fold_truth_exact(a, w * 0.3, b, mu, sigma, c)
    with pytest.raises(AssertionError):  # a total no fp32 slot sum holds exactly
        gc.fold_stats(mu * 4096, sigma, 256)


def test_mutant_fold_statistics_slot_dropped():
    a, w, b, mu, sigma, c, st, y, acc = _fold_probe()
    bad = st.clone()
    bad[:, 5, 0] = 0  # slot 5 of the 8 sums never added (a butterfly step short)
    out, mean, rstd = _fold_run(a, w, b, bad, c)
    _rejects(lambda: gc.assert_fold_stats(mean, rstd, mu, sigma, 256, "m"))
    _rejects(lambda: gc.assert_fold(out, y, acc, mu, sigma, c, b, 256, "m", TILE), "elements differ")
    dup = st.clone()
    dup[:, 5] = dup[:, 4]  # slot 4 read twice
    _rejects(lambda: gc.assert_fold_stats(*_fold_run(a, w, b, dup, c)[1:], mu, sigma, 256, "m"))


def test_mutant_fold_statistics_of_the_next_row():
    a, w, b, mu, sigma, c, st, y, acc = _fold_probe()
    nxt = torch.cat((st[1:], st[-1:]))  # row m reads the slots of row m + 1
    out, mean, rstd = _fold_run(a, w, b, nxt, c, pure=True)
    _rejects(lambda: gc.assert_fold_stats(mean, rstd, mu, sigma, 256, "m"), "ln_rstd")
    y0, acc0 = gc.fold_truth_exact(torch.zeros_like(a), w, b, mu, sigma, c)
    # sigma repeats every 4 rows: among rows of one sigma the pure-statistic probe names the row read
    one = st.clone()
    one[8] = st[12]
    out = _fold_run(a, w, b, one, c, pure=True)[0]
    _rejects(lambda: gc.assert_fold(out, y0, acc0, mu, sigma, c, b, 256, "m", TILE),
             rf"\[8, \d+\] .* with this column's c the mean code {float(mu[12]):g} \(rows \[[\d, ]*\b12\b")
    # a single slot of the next row in place of the row's own changes a total too
    one = st.clone()
    one[8, 3] = st[9, 3]
    _rejects(lambda: gc.assert_fold_stats(*_fold_run(a, w, b, one, c)[1:], mu, sigma, 256, "m"))


def test_mutant_fold_column_sums_shifted_16():
    a, w, b, mu, sigma, c, st, y, acc = _fold_probe()
    shifted = torch.roll(c, -16)  # c[n + 16] for c[n]
    out, mean, rstd = _fold_run(a, w, b, st, shifted)
    gc.assert_fold_stats(mean, rstd, mu, sigma, 256, "the statistics are right")
    _rejects(lambda: gc.assert_fold(out, y, acc, mu, sigma, c, b, 256, "m", TILE),
             rf"with this row's mean the column code {float(c[16]):g} \(columns \[[\d, ]*\b16\b")


def test_fold_bound_separates_neighbouring_codes():
    """K = 384: the operand bound is far below the change a mean code one off causes."""
    a, w, b, mu, sigma, c, st, y, acc = _fold_probe(K=384)
    assert float(mu.abs().max()) <= 4
    out, mean, rstd = _fold_run(a, w, b, st, c)
    gc.assert_fold(out, y, acc, mu, sigma, c, b, 384, "clean", TILE)
    gc.assert_fold(out.bfloat16(), y, acc, mu, sigma, c, b, 384, "clean bf16", TILE)
    gc.assert_fold_stats(mean, rstd, mu, sigma, 384, "clean")
    step = (c.abs().unsqueeze(0) / sigma.unsqueeze(1))  # a mean code one off moves the output by |c| / sigma
    bnd = gc.fold_bound(acc, mu, sigma, c)
    assert float((bnd / step.clamp_min(1e-9))[:, c != 0].max()) < 1e-2
    off = gc.fold_stats(mu + (torch.arange(mu.shape[0]) == 7), sigma, 384)
    out = _fold_run(a, w, b, off, c)[0]
    _rejects(lambda: gc.assert_fold(out, y, acc, mu, sigma, c, b, 384, "m", TILE), r"\[7, ")
    _rejects(lambda: gc.assert_fold(out.bfloat16(), y, acc, mu, sigma, c, b, 384, "m", TILE), r"\[7, ")


def test_exactness_condition_is_enforced():
    g = torch.Generator().manual_seed(0)
    a, w = gc.int_operands((4, 1152), -4, 4, g), gc.int_operands((8, 1152), -4, 4, g)
    gc.exact_truth(a, w)                                    # [-4, 4] holds to K = 1,152 ...
    with pytest.raises(AssertionError, match="exactness"):  # ... a bias of 2^24 does not
        gc.exact_truth(a, w, torch.full((8,), 2.0 ** 24))
    with pytest.raises(AssertionError, match="integers"):
        gc.exact_truth(a * 0.3, w)
    dy, x = gc.int_operands((20032, 8), -2, 2, g), gc.int_operands((20032, 8), -2, 2, g)
    gc.exact_truth(dy.t(), x.t())                           # [-2, 2] over 20,032 tokens
    a1, w1 = gc.int_operands((4, 128), -1, 1, g), gc.int_operands((32, 128), -1, 1, g)
    gc.exact_truth(a1, w1, stats=True)                      # [-1, 1], K <= 128: squares summed
    with pytest.raises(AssertionError, match="sum of squares"):
        gc.exact_truth(a[:, :128] * 16, w[:, :128].repeat(4, 1) * 16, stats=True)
    with pytest.raises(AssertionError):
        gc.int_operands((2, 2), -300, 300, g)


# ----------------------------------------------------------------------------- mutants
M_, N_, K_ = 145, 136, 320  # 64x64 tiles: 3 x 3 with ragged edges, 5 k-tiles
TILE = (64, 64)


def _random(seed=0):
    g = torch.Generator().manual_seed(seed)
    return gc.int_operands((M_, K_), -4, 4, g), gc.int_operands((N_, K_), -4, 4, g)


def _mm(a, w, dt=torch.float32):
    return (a.double() @ w.double().t()).to(dt)


def _probes():
    (a, w), (pa, pw) = _random(), gc.position_probe(M_, N_, K_)
    return a, w, pa, pw


def _rejects(fn, match=None):
    with pytest.raises(AssertionError, match=match):
        fn()


def _zero_cols(t, lo, hi):
    t = t.clone()
    t[:, lo:hi] = 0
    return t


def test_clean_output_is_accepted():
    a, w, pa, pw = _probes()
    gc.assert_exact(_mm(a, w), gc.exact_truth(a, w), "clean", TILE)
    for pr in (pa, pw):
        gc.assert_position(_mm(pr.a, pr.w), pr, "clean", TILE)
        gc.assert_position(_mm(pr.a, pr.w, torch.bfloat16), pr, "clean", TILE)


def test_mutant_last_ktile_dropped():
    a, w, pa, pw = _probes()
    _rejects(lambda: gc.assert_exact(_mm(_zero_cols(a, K_ - 64, K_), w), gc.exact_truth(a, w), "m", TILE))
    # the position probe names the rows that lost their source: row m reads k = (37 m + 11) mod K
    _rejects(lambda: gc.assert_position(_mm(_zero_cols(pa.a, K_ - 64, K_), pa.w), pa, "m", TILE),
             r"expected source k = (2[5-9]\d|3[01]\d)")


@pytest.mark.parametrize("S", [2, 3, 4])
def test_mutant_stale_ring_stage(S):
    """k-tile j read from the ring slot that still holds k-tile j - S."""
    a, w, pa, pw = _probes()
    j = 4

    def stale(t):
        t = t.clone()
        t[:, 64 * j:64 * (j + 1)] = t[:, 64 * (j - S):64 * (j - S + 1)]
        return t
    _rejects(lambda: gc.assert_exact(_mm(stale(a), stale(w)), gc.exact_truth(a, w), "m", TILE))
    # one-hot A: a row whose source lies in k-tile j - S is now read twice (no code value); one whose
    # source lies in k-tile j is lost
    _rejects(lambda: gc.assert_position(_mm(stale(pa.a), stale(pa.w)), pa, "m", TILE), "decodes to")


def test_mutant_8_element_chunk_dropped():
    a, w, pa, pw = _probes()
    lo = 64 * 2 + 8 * 3
    _rejects(lambda: gc.assert_exact(_mm(_zero_cols(a, lo, lo + 8), w), gc.exact_truth(a, w), "m", TILE))
    with pytest.raises(AssertionError) as e:
        gc.assert_position(_mm(_zero_cols(pa.a, lo, lo + 8), pa.w), pa, "m", TILE)
    # exactly the rows whose source k lies in the chunk, and the message says which k was expected
    rows = [m for m in range(M_) if lo <= (37 * m + 11) % K_ < lo + 8]
    assert rows and f"{len(rows) * N_ - sum(1 for m in rows for n in range(N_) if (7 * n + 13 * ((37 * m + 11) % K_)) % 251 == 0)} of" in str(e.value)
    assert f"expected source k = {(37 * rows[0] + 11) % K_}" in str(e.value)


def test_mutant_rows_swapped_within_a_tile():
    a, w, pa, pw = _probes()

    def swap(y, r=64 + 5):
        y = y.clone()
        y[[r, r + 16]] = y[[r + 16, r]]
        return y
    _rejects(lambda: gc.assert_exact(swap(_mm(a, w)), gc.exact_truth(a, w), "m", TILE), r"tiles \(1, 0\)..\(1, 2\), in-tile rows 5..21")
    # the value at row 69 names k = (37 * 85 + 11) mod 320 = 276, the source of row 85 (codes repeat mod 251)
    _rejects(lambda: gc.assert_position(swap(_mm(pa.a, pa.w)), pa, "m", TILE),
             rf"\[69, 0\] expected source k = {(37 * 69 + 11) % K_} .* decodes to W\[0\]\[k = 25 or 276\] \(the source of row 85\)")
    _rejects(lambda: gc.assert_position(swap(_mm(pw.a, pw.w)), pw, "m", TILE), r"in-tile rows 5..21")


def test_mutant_column_group_shifted():
    a, w, pa, pw = _probes()

    def shift(y, c=64 + 8):
        y = y.clone()
        y[:, c:c + 4] = y[:, c + 4:c + 8]
        return y
    _rejects(lambda: gc.assert_exact(shift(_mm(a, w)), gc.exact_truth(a, w), "m", TILE), r"cols 72..75")
    _rejects(lambda: gc.assert_position(shift(_mm(pa.a, pa.w)), pa, "m", TILE), r"in-tile cols 8..11")
    # the mirror probe decodes it: column 72 shows the k that column 76 selects
    _rejects(lambda: gc.assert_position(shift(_mm(pw.a, pw.w)), pw, "m", TILE),
             rf"\[0, 72\] expected source k = {(37 * 72 + 11) % K_} .*k = 12 or {(37 * 76 + 11) % K_}\] \(the source of column 76\)")


def test_mutant_last_partial_row_tile_unwritten():
    a, w, _, _ = _probes()
    out, ok = gc.canary((M_, N_), 4 * N_, torch.float32)
    out[:128] = _mm(a, w)[:128]  # rows 128..144 (the partial third row tile) never written
    _rejects(lambda: gc.assert_exact(out, gc.exact_truth(a, w), "m", TILE), r"17 \* 136|2312 of")
    ok("padding")  # nothing written outside


def test_mutant_out_of_bounds_writes():
    a, w, _, _ = _probes()
    y = _mm(a, w)
    out, ok = gc.canary((M_, N_), 2 * N_, torch.float32)
    out.copy_(y)
    ok("clean")
    flat = out.view(-1)
    # row M: lands in the padding after the buffer
    base = torch.as_strided(flat, (M_ * N_ + N_,), (1,))
    base[M_ * N_ + 3] = 7.0
    _rejects(lambda: ok("row M"), "past its end")
    # column N of the last row is the same place; of any other row it is the next row's
    # column 0, which the comparison of the valid region sees
    out2, ok2 = gc.canary((M_, N_), 2 * N_, torch.float32)
    out2.copy_(y)
    out2.view(-1)[5 * N_ + N_] = y[5, N_ - 1] + 1  # "column N" of row 5
    ok2("padding intact")
    _rejects(lambda: gc.assert_exact(out2, gc.exact_truth(a, w), "m", TILE), r"\[6, 0\]")
    # a read-add-write (not a store) into the padding before the buffer
    out3, ok3 = gc.canary((M_, N_), 2 * N_, torch.float32)
    before = torch.as_strided(out3, (4,), (1,), out3.storage_offset() - 4)
    before += 1.0
    _rejects(lambda: ok3("before"), "before the buffer")
    # bf16 buffers likewise
    o16, ok16 = gc.canary((M_, N_), N_, torch.bfloat16)
    torch.as_strided(o16, (1,), (1,), o16.storage_offset() + M_ * N_)[0] = 1.0
    _rejects(lambda: ok16("bf16 row M"), "past its end")


def test_mutant_one_bf16_ulp():
    a, w, _, _ = _probes()
    truth = gc.exact_truth(a, w, None, None, torch.bfloat16)
    y = truth.clone()
    y.view(torch.int16)[77, 100] += 1
    _rejects(lambda: gc.assert_exact(y, truth, "m", TILE), r"1 of .*\n\s+\[77, 100\]")
    # ... and a NaN is a mismatch, not a skipped comparison
    y = truth.clone()
    y[3, 3] = float("nan")
    _rejects(lambda: gc.assert_exact(y, truth, "m", TILE), r"\[3, 3\] got nan")


def test_mutant_dgrad_slices_swapped():
    g = torch.Generator().manual_seed(3)
    dy, w = gc.int_operands((65, 320), -4, 4, g), gc.int_operands((320, 72), -4, 4, g)
    parts = ref.linear_dgrad(dy, w, True, 3)  # slices of 128, 128, 64
    wt = w.t().contiguous()
    truths = [gc.exact_truth(dy[:, s], wt[:, s]) for s in (slice(0, 128), slice(128, 256), slice(256, 320))]
    for z in range(3):
        gc.assert_exact(parts[z], truths[z], f"slice {z}")
    swapped = parts[[1, 0, 2]]
    assert torch.equal(swapped.sum(0), parts.sum(0))  # the sum (what a tolerance test of dx sees) is blind
    _rejects(lambda: gc.assert_exact(swapped[0], truths[0], "slice 0"))


def test_mutant_bias_added_in_every_k_slice():
    a, w = _random()
    g = torch.Generator().manual_seed(4)
    b = gc.int_operands((N_,), -64, 64, g, torch.float32)
    truth = gc.exact_truth(a, w, b)
    y = sum(_mm(a[:, s], w[:, s]) + b for s in (slice(0, 192), slice(192, 320)))
    _rejects(lambda: gc.assert_exact(y, truth, "m", TILE))


def test_mutant_db_from_every_column_tile():
    g = torch.Generator().manual_seed(5)
    dy, db0 = gc.int_operands((72, 64), -4, 4, g), gc.int_operands((64,), -8, 8, g, torch.float32)
    ones = torch.ones(1, 72, dtype=torch.bfloat16)
    truth = gc.exact_truth(dy.t(), ones, None, db0.unsqueeze(1)).squeeze(1)
    col_tiles = -(-192 // 64)  # K = 192: three column tiles each add the column sum
    _rejects(lambda: gc.assert_exact(db0 + col_tiles * dy.float().sum(0), truth, "db"))
    # K <= 64 has one column tile: the grid must (and does) hold wider K to see this
    assert any(k > 64 for k in gc.WGRAD_DIMS)


def test_old_tolerance_is_blind_to_small_faults():
    """Why the exact probes exist.  The suite's ``close(..., 2e-2, 1e-2)`` on randn inputs
    (weights scaled 0.05, as in tests/test_gemm_tiles_gpu.py) is an absolute bound on O(1)
    outputs:

    * a bf16 output one ulp off on *every* element is accepted;
    * a dropped 8-element k-chunk is seen at that operand scale (measured here: 1,794 of
      the 2,137 changed elements leave the bound), but one in six of the changed elements
      stays inside it -- a fault of that size on a few elements can pass -- and
    * the same dropped chunk is accepted entirely once the operand has std 0.02 (the size
      of the gradients the backward GEMMs read in training): the verdict depends on the
      scale of the data.

    The exact probes reject all of these whatever the scale (tests above)."""
    torch.manual_seed(0)
    M, N, K = 145, 136, 384
    w = (torch.randn(N, K) * 0.05).to(torch.bfloat16)

    def old_close_bad(got, want, atol=2e-2, rtol=1e-2):
        err = (got.float() - want.float()).abs()
        return int((~(err <= atol + rtol * want.float().abs())).sum())

    def chunk_mutant(a):  # one 8-element chunk dropped for one 16-row fragment
        am = a.clone()
        am[64:80, 136:144] = 0
        y, ym = ref.linear_fwd(a, w, None, False), ref.linear_fwd(am, w, None, False)
        changed = int((ym != y).sum())
        return changed, old_close_bad(ym, y)

    a = torch.randn(M, K).to(torch.bfloat16)
    y = ref.linear_fwd(a, w, None, False)
    ulp = y.clone()
    ulp.view(torch.int16).add_(1)
    assert not torch.equal(ulp, y) and old_close_bad(ulp, y) == 0
    changed, bad = chunk_mutant(a)
    assert changed > 1000 and 0 < bad < 0.9 * changed, (changed, bad)
    changed_s, bad_s = chunk_mutant((torch.randn(M, K) * 0.02).to(torch.bfloat16))
    assert changed_s > 1000 and bad_s == 0, (changed_s, bad_s)
    print(f"old tolerance: one-ulp mutant 0 of {y.numel()} out of bound; chunk mutant {bad} of {changed} changed "
          f"elements out of bound; at std 0.02 {bad_s} of {changed_s}")
