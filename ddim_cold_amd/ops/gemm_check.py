"""Exact integer probes for the GEMMs (csrc/gemm.hip).

With small-integer bf16 operands every product and every partial sum of a GEMM
is an integer below 2^24, which fp32 holds exactly -- in any summation order,
K split or ring depth.  The right answer is therefore unique to the bit: the
fp32 output is that integer, a bf16 output its round-to-nearest-even, and the
comparison is on raw bits with no tolerance.  :func:`exact_truth` asserts this
*exactness condition* on the very tensors it is given, so a probe whose range is
too wide for its shape fails on the CPU, not silently on the GPU.

Ranges that satisfy the condition: ``[-4, 4]`` for K <= 1,152 (with biases and
residuals to a few hundred), ``[-2, 2]`` for weight gradients over 20,032 tokens,
``[-1, 1]`` with K <= 128 where squares are summed (``st_out`` row statistics).

Two probes, one comparison, one guard:

* :func:`int_operands` -- uniform random integers.  Any value-level fault (a
  dropped or stale k-tile, a dropped 8-element chunk, a bias added twice, a
  stale accumulate) changes some output by at least 1, with probability ~1.
* :func:`position_probe` -- one-hot rows of one operand against a coded other:
  every output *names* the operand element it was read from, so a mismatch
  decodes to "row r, col c should have read k = 75 and read k = 11": swapped
  rows, shifted column groups and dropped chunks are located, not only seen.
* :func:`assert_exact` -- bit comparison; on failure the count, the first few
  (row, col, got, want) and the bounding box of the mismatches in tile
  coordinates of the tile that ran.
* :func:`canary` -- a caller-provided output inside a buffer of sentinel bits;
  its checker proves nothing was written past the valid region.

Pure PyTorch and device-agnostic.  The shape grids of ``tests/test_gemm_exact_gpu.py``
live here too, so ``tests/test_gemm_check_cpu.py`` runs the reference through
the same shapes (which proves the chosen ranges satisfy the condition).
"""
from __future__ import annotations

from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple

import torch

EXACT_LIMIT = float(1 << 24)  # fp32 holds every integer of magnitude <= 2^24

# csrc/kernels.h GemmEpi (the ``epi`` of ``torch.ops.ddim_cold.gemm_plan``)
EPI_BF16, EPI_F32, EPI_QKV, EPI_RESID, EPI_GELU, EPI_HEAD, EPI_EMBED, EPI_DGELU, EPI_ATOMIC = range(9)
EPI_HEADR = 10

# csrc/gemm_plan.h tile configs (GEMM_TILES): cfg -> (BM, BN, waves)
TILES = {0: (32, 64, 4), 1: (64, 64, 4), 2: (128, 64, 4), 3: (128, 128, 4),
         4: (256, 128, 8), 5: (128, 128, 8), 6: (256, 192, 8)}


# ----------------------------------------------------------------------------- shape grids
def edge_ms(bm: int) -> List[int]:
    """Row counts around a BM-row tile: one row, one short, full, one over, two tiles and a ragged third."""
    return sorted({1, bm - 1, bm, bm + 1, 2 * bm + 17})


def edge_ns(bn: int) -> List[int]:
    """Column counts (multiples of 4: the vector epilogue) around a BN-column tile."""
    return sorted({4, bn - 4, bn, bn + 4})


EDGE_KS = (64, 192, 320)            # 1, 3 and 5 k-tiles (odd, prime to every ring depth)
SHORT_KS = (64, 128)                # fewer k-tiles than the prologue of a 3- / 4-stage ring issues
DEPTH_KS = (512, 576)               # 8 k-tiles (depth 3 over the threshold) and 9 (depth 4)
FIXED_DEPTH_KS = (64, 128, 448)     # 256x128 (always 3 stages) and 256x192 (always 2)
PLAIN_KS = (8, 40, 72, 136)         # K % 64 != 0: the non-DMA kernel
DGRAD_NOUT = (64, 200, 320, 1152)   # dgrad reduction lengths (200: non-DMA)
DGRAD_MS = (1, 65, 300)
WGRAD_TOKENS = (8, 56, 72, 136, 200)
WGRAD_DIMS = (8, 64, 72, 192)
WGRAD_BIG_TOKENS = 16392            # >= 16,384: the 128x128 weight-gradient tiles
QKV_SHAPES = ((3, 17, 2, 64), (2, 5, 4, 128), (2, 17, 3, 192))  # (B, N, H, D): hd = 32, 32, 64
QKV_SHAPE_HD16 = (2, 5, 4, 64)      # hd = 16
HEAD_GEOMS = tuple((3, 3, s, s, p, 64) for s in (16, 24) for p in (4, 8))  # (B, C, H, W, p, D)


def small_prime_factor(n: int) -> int:
    return next(d for d in range(2, n + 1) if n % d == 0)


RESID_SHAPES = ((81, 27, 96, 64), (285, 57, 160, 128))   # (M, tokens, Dout, K): tokens never divide a row tile
GELU_SHAPES = ((81, 68, 64), (285, 196, 192))            # (M, N, K)
EMBED_GEOMS = tuple((3, 3, s, s, p, 68) for s in (16, 24) for p in (8, 4))  # p = 8: K = 192; p = 4: K = 48
EMBED_STAT_GEOMS = ((3, 3, 16, 16, 8, 96), (3, 3, 24, 24, 8, 160))  # D % 32 == 0 but not a multiple of 64 / 128
PLAIN_SHAPES = ((81, 68), (961, 1024))                   # under / over 240 64x64 tiles
DGELU_SHAPES = ((65, 64), (300, 320))                    # (M, Nout); the output width comes from the tile
DGRAD_LN_CASES = ((300, 320, 128, 3), (65, 1152, 128, 4))  # (M, Nout, K, splits)
WGRAD_BIG_SHAPES = ((192, 192, True), (192, 136, False), (72, 192, True))  # 10 128x128 tiles: all in the split tail
DROPOUT_PS = (0.1, 0.3)


def dgrad_width(cfg: int) -> int:
    """A ragged output width (multiple of 8) for the transposed-B tiles: BN = 64 (4 waves) or 128."""
    return (64 if cfg <= 3 else 128) + 8


def wgrad_shapes():
    """Every (Nout, K) of the weight-gradient grid, ``db`` on alternate problems."""
    return [(n, k, (i + j) % 2 == 0) for i, n in enumerate(WGRAD_DIMS) for j, k in enumerate(WGRAD_DIMS)]


def embed_dropout_geom(rows: int):
    """(B, H, W, patch) whose B x 81 patch rows cover ``rows`` GEMM rows."""
    return -(-rows // 81), 72, 72, 8


def _stage_bytes(cfg: int) -> int:
    return (TILES[cfg][0] + TILES[cfg][1]) * 128  # one ring stage: BM + BN rows of 64 bf16


TWO_DEPTH_TILES = [c for c in TILES if 4 * _stage_bytes(c) <= 160 * 1024]  # 3 or 4 stages by grid size
FIXED_DEPTH_TILES = [(c, 2 if 3 * _stage_bytes(c) > 160 * 1024 else 3) for c in TILES if c not in TWO_DEPTH_TILES]


def depth_shape(cfg: int) -> Tuple[int, int]:
    """(M, N) just over the co-residency threshold of tile ``cfg`` (256 x per_cu4
    workgroups, csrc/gemm_plan.h gemm_ring_stages): N = 1,024 and one row more than
    fills the last whole row tile under the threshold."""
    bm, bn, _ = TILES[cfg]
    per_cu4 = (160 * 1024) // (4 * (bm * 128 + bn * 128))
    cols = 1024 // bn
    rows = (256 * per_cu4) // cols  # rows x cols == the threshold exactly
    assert rows * cols == 256 * per_cu4
    return bm * rows + 1, 1024


# ----------------------------------------------------------------------------- operands
def int_operands(shape, lo: int, hi: int, gen: torch.Generator, dtype=torch.bfloat16, device=None):
    """Uniform integers in ``[lo, hi]`` as a ``dtype`` tensor (bf16 operands; pass fp32
    for biases, residuals, ``pos`` / ``temb`` / ``cls`` and initial ``dw`` / ``db``).
    Drawn on the CPU from ``gen`` (the same values on every device)."""
    assert max(abs(lo), abs(hi)) <= 256, "bf16 holds integers exactly only to 256"
    t = torch.randint(lo, hi + 1, tuple(shape), generator=gen, dtype=torch.int32).to(dtype)
    return t if device is None else t.to(device)


def _amax(t) -> float:
    return 0.0 if t is None or t.numel() == 0 else float(t.detach().abs().max())


def _is_int(t) -> bool:
    return t is None or bool((t.double() == t.double().round()).all())


def exact_truth(a, w, bias=None, res=None, out_dtype=torch.float32, stats: bool = False, scale: int = 1):
    """``a @ w.T + bias + res`` in fp64 from the same tensors, cast to ``out_dtype``.

    ``a`` [M, K], ``w`` [N, K], ``bias`` [N], ``res`` [M, N].  Asserts the exactness
    condition ``K max|a| max|w| + max|bias| + max|res| < 2^24`` (operands that are
    integers, or integers / ``scale`` with ``scale`` a power of two: then the bound is on
    the scaled values) -- so any correct fp32 kernel gives this value to the bit.
    ``stats``: also the {sum, sum^2} per 32-column slot of the fp32 result
    ([M, N/32, 2] fp32), asserting every slot's sum of squares is below 2^24 too."""
    assert scale >= 1 and scale & (scale - 1) == 0, "scale must be a power of two"
    K = a.shape[-1]
    for t in (a, w, bias, res):
        assert _is_int(None if t is None else t.double() * scale), "exact_truth: operands must be integers / scale"
    bound = K * _amax(a) * _amax(w) * scale * scale + (_amax(bias) + _amax(res)) * scale * scale
    assert bound < EXACT_LIMIT, f"exactness condition violated: {bound:.0f} >= 2^24 (K = {K})"
    y = a.double() @ w.double().t()
    if bias is not None:
        y = y + bias.double()
    if res is not None:
        y = y + res.double().reshape(y.shape)
    out = y.to(out_dtype)
    if not stats:
        return out
    assert scale == 1
    return out, exact_row_stats(y)


def exact_row_stats(y):
    """{sum, sum^2} per 32-column slot of integer rows ``y`` ([..., N] fp64) as fp32
    [..., N/32, 2]; asserts every slot's sum of squares is below 2^24 (then exact in any order)."""
    ys = y.double().reshape(*y.shape[:-1], y.shape[-1] // 32, 32)
    sq = (ys * ys).sum(-1)
    assert float(sq.max()) < EXACT_LIMIT, "exactness condition violated in a slot's sum of squares"
    return torch.stack((ys.sum(-1), sq), dim=-1).float()


# ----------------------------------------------------------------------------- comparison
def _bits(t: torch.Tensor) -> torch.Tensor:
    if t.dtype in (torch.float32,):
        return t.contiguous().view(torch.int32)
    if t.dtype in (torch.bfloat16, torch.float16):
        return t.contiguous().view(torch.int16)
    return t.contiguous()


def _as2d(t: torch.Tensor) -> torch.Tensor:
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(-1, t.shape[-1])


def mismatches(got, truth) -> torch.Tensor:
    """[n, 2] (row, col) of the elements whose raw bits differ (2-D view: all leading dims are rows)."""
    assert got.shape == truth.shape, f"shape {tuple(got.shape)} != {tuple(truth.shape)}"
    assert got.dtype == truth.dtype, f"dtype {got.dtype} != {truth.dtype}"
    return (_as2d(_bits(got)) != _as2d(_bits(truth.to(got.device)))).nonzero()


def assert_exact(got, truth, name: str = "", tile: Optional[Sequence[int]] = None, first: int = 6):
    """Bit equality (NaN payloads and the sign of zero included).  ``tile`` = (BM, BN) of
    the tile that ran: the mismatches' bounding box is reported in tile coordinates."""
    bad = mismatches(got, truth)
    if bad.shape[0] == 0:
        return
    g2, t2 = _as2d(got), _as2d(truth.to(got.device))
    lines = [f"{name}: {bad.shape[0]} of {got.numel()} elements differ (shape {tuple(got.shape)}, {got.dtype})"]
    for r, c in bad[:first].tolist():
        lines.append(f"  [{r}, {c}] got {float(g2[r, c])!r} want {float(t2[r, c])!r}")
    r0, c0 = (int(v) for v in bad.min(0).values)
    r1, c1 = (int(v) for v in bad.max(0).values)
    box = f"  bounding box rows {r0}..{r1}, cols {c0}..{c1}"
    if tile is not None:
        bm, bn = int(tile[0]), int(tile[1])
        box += f" = {bm}x{bn} tiles ({r0 // bm}, {c0 // bn})..({r1 // bm}, {c1 // bn})"
        if r0 // bm == r1 // bm:  # offsets inside the tile, where the box stays in one
            box += f", in-tile rows {r0 % bm}..{r1 % bm}"
        if c0 // bn == c1 // bn:
            box += f", in-tile cols {c0 % bn}..{c1 % bn}"
    lines.append(box)
    raise AssertionError("\n".join(lines))


# ----------------------------------------------------------------------------- position probe
CODE_MOD = 251  # prime, < 256: every code value is an exact bf16 integer
_INV13 = pow(13, -1, CODE_MOD)


def _code(i, k):
    return (7 * i + 13 * k) % CODE_MOD


class PositionProbe(NamedTuple):
    a: torch.Tensor      # [M, K] bf16
    w: torch.Tensor      # [N, K] bf16
    want: torch.Tensor   # [M, N] fp64: the exact product
    onehot: str          # "a": rows of A select k against a coded W; "w": the mirror image
    src: torch.Tensor    # the k each row (of A) / column (= row of W) selects
    row_ids: torch.Tensor  # the probe's row number of each row of ``a`` (see :meth:`rows`)

    def rows(self, idx) -> "PositionProbe":
        """The probe restricted to output rows ``idx`` (an op that skips rows: the head's cls rows)."""
        idx = idx.cpu()
        return PositionProbe(self.a[idx.to(self.a.device)], self.w, self.want[idx], self.onehot,
                             self.src[idx] if self.onehot == "a" else self.src, self.row_ids[idx])

    def truth(self, out_dtype=torch.float32, bias=None):
        return exact_truth(self.a, self.w, bias, None, out_dtype)

    def decode(self, row: int, col: int, value: float) -> str:
        """The source index an observed value names at output (row, col)."""
        if value != value or value != round(value) or not 0 <= value < CODE_MOD:
            return f"{value!r} is no code value (a sum of several sources, or none)"
        i = col if self.onehot == "a" else int(self.row_ids[row])  # the coded operand's row index
        k = ((int(value) - 7 * i) * _INV13) % CODE_MOD
        K = self.a.shape[1]
        ks = list(range(k, K, CODE_MOD))
        who, what = ("W", "row") if self.onehot == "a" else ("A", "column")
        # whose source that is: the one-hot operand's row that selects this k
        owners = [int(j) for j in (self.src.unsqueeze(1) == torch.tensor(ks).unsqueeze(0)).any(1).nonzero().flatten()[:4]] \
            if ks else []
        if self.onehot == "a":
            owners = [int(self.row_ids[j]) for j in owners]
        return f"{who}[{i}][k = {' or '.join(map(str, ks)) if ks else f'{k} (>= K)'}]" + \
               (f" (the source of {what} {' / '.join(map(str, owners))})" if owners else "") + \
               (" or a zero (nothing read)" if value == 0 else "")


def position_probe(M: int, N: int, K: int, device=None) -> Tuple[PositionProbe, PositionProbe]:
    """The diagnostic pair: one-hot rows of A (row m selects ``k = (37 m + 11) mod K``)
    against ``W[n][k] = (7 n + 13 k) mod 251``, and the mirror image (one-hot rows of W,
    coded A).  Each output equals exactly one coded element, so it names the (row, k)
    that was read.  The first decodes row faults (the k an output shows is the source of
    the row it was computed from), the mirror column faults."""
    k_idx = torch.arange(K, dtype=torch.int64)
    out = []
    for onehot, R, Cn in (("a", M, N), ("w", N, M)):
        src = (37 * torch.arange(R, dtype=torch.int64) + 11) % K
        hot = torch.zeros(R, K)
        hot[torch.arange(R), src] = 1.0
        coded = _code(torch.arange(Cn, dtype=torch.int64).unsqueeze(1), k_idx.unsqueeze(0)).float()
        a, w = (hot, coded) if onehot == "a" else (coded, hot)
        a, w = a.to(torch.bfloat16), w.to(torch.bfloat16)
        want = a.double() @ w.double().t()
        if device is not None:
            a, w = a.to(device), w.to(device)
        out.append(PositionProbe(a, w, want, onehot, src, torch.arange(M)))
    return out[0], out[1]


def assert_position(got, probe: PositionProbe, name: str = "", tile: Optional[Sequence[int]] = None,
                    bias=None, first: int = 6):
    """:func:`assert_exact` against the probe's truth; a mismatch also says which source
    index was expected and which one the observed value decodes to."""
    truth = probe.truth(got.dtype, bias)
    bad = mismatches(got.reshape(truth.shape), truth)
    if bad.shape[0] == 0:
        return
    g2 = got.reshape(truth.shape).double().cpu()
    if bias is not None:
        g2 = g2 - bias.double().cpu()
    lines = []
    for r, c in bad[:first].tolist():
        k = int(probe.src[r if probe.onehot == "a" else c])
        lines.append(f"  [{r}, {c}] expected source k = {k} (value {float(probe.want[r, c]):.0f}); "
                     f"observed {float(g2[r, c])!r} decodes to {probe.decode(r, c, float(g2[r, c]))}")
    try:
        assert_exact(got.reshape(truth.shape), truth, f"{name} position probe (one-hot {probe.onehot})", tile, 0)
    except AssertionError as e:
        raise AssertionError(str(e) + "\n" + "\n".join(lines)) from None


# ----------------------------------------------------------------------------- canary
_SENTINEL = {torch.float32: -12345677.0, torch.bfloat16: -123.5, torch.int32: -1234567, torch.int64: -1234567}


def canary(shape_valid, pad: int, dtype=torch.float32, device=None) -> Tuple[torch.Tensor, Callable[[str], None]]:
    """``(view, check)``: a contiguous view of ``shape_valid`` inside a flat buffer with
    ``pad`` elements (rounded up to 64: the view keeps a 128-byte alignment) of sentinel
    before and after it; the view starts out as sentinel too, so an element the kernel
    leaves unwritten fails the exact comparison.  ``check(name)`` asserts that the padding
    is bit-identical afterwards (a write to row M lands there; a write to column N lands in
    the next row, where the comparison of the valid region sees it).  The sentinel is a
    finite odd value: a read-add-write into the padding changes it as surely as a store."""
    n = 1
    for s in shape_valid:
        n *= int(s)
    pad = (int(pad) + 63) // 64 * 64
    buf = torch.full((pad + n + pad,), _SENTINEL[dtype], dtype=dtype, device=device)
    before = buf.clone()
    view = buf[pad:pad + n].view(tuple(shape_valid))

    def check(name: str = ""):
        lo = (_bits(buf[:pad]) != _bits(before[:pad])).nonzero().flatten()
        hi = (_bits(buf[pad + n:]) != _bits(before[pad + n:])).nonzero().flatten()
        if lo.numel() or hi.numel():
            where = [f"{lo.numel()} elements before the buffer (nearest: {pad - int(lo.max())} before the start)"] \
                if lo.numel() else []
            if hi.numel():
                where.append(f"{hi.numel()} elements past its end (flat offsets {int(hi.min())}..{int(hi.max())} "
                             f"past the last valid element)")
            raise AssertionError(f"{name}: out-of-bounds write, " + "; ".join(where))

    return view, check


# ----------------------------------------------------------------------------- probe runs
# One function per op family: builds the integer operands on ``device``, calls the op
# through :mod:`ddim_cold_amd.ops` (HIP kernels on a GPU, :mod:`.reference` on the CPU)
# and compares bit for bit.  ``tile`` = (BM, BN) only labels the mismatch report.
def _ops():
    import ddim_cold_amd.ops as ops
    return ops


def _gen(seed: int) -> torch.Generator:
    g = torch.Generator()
    g.manual_seed(seed)
    return g


def _rng(device, seed: int = 1234, step: int = 5):
    return torch.tensor([seed, step], dtype=torch.int64, device=device)


def close(a, b, atol: float, rtol: float = 0.0, name: str = ""):
    """The suite's tolerance check (for the few non-integer outputs: GELU's ``h``, LayerNorm)."""
    a, b = a.float().cpu(), b.float().cpu()
    err = (a - b).abs()
    bad = (~(err <= atol + rtol * b.abs())).sum().item()  # NaN counts as a mismatch
    assert bad == 0, f"{name}: {bad} mismatches, max err {err.max().item():.3e}"


LINEAR_COMBOS = ((False, False), (False, True), (True, False), (True, True))  # (out_fp32, bias)


def run_linear(M: int, N: int, K: int, device, tile=None, combos=LINEAR_COMBOS, seed: int = 0):
    """``linear_fwd`` (EPI_BF16 / EPI_F32): random integers in [-4, 4] and both position
    probes.  ``tile``: (BM, BN), or a function of ``out_fp32`` returning it."""
    ops, g = _ops(), _gen(seed)
    a, w = int_operands((M, K), -4, 4, g, device=device), int_operands((N, K), -4, 4, g, device=device)
    b = int_operands((N,), -64, 64, g, torch.float32, device)
    y0 = exact_truth(a, w, None, None, torch.float64)
    y1 = exact_truth(a, w, b, None, torch.float64)
    probes = position_probe(M, N, K, device)
    for f32, bias in combos:
        bb, dt = (b if bias else None), (torch.float32 if f32 else torch.bfloat16)
        tl = tile(f32) if callable(tile) else tile
        name = f"linear_fwd M={M} N={N} K={K} {'f32' if f32 else 'bf16'}{' +bias' if bias else ''}"
        assert_exact(ops.linear_fwd(a, w, bb, f32), (y1 if bias else y0).to(dt), name, tl)
        for pr in probes:
            assert_position(ops.linear_fwd(pr.a, pr.w, bb, f32), pr, name, tl, bias=bb)


def _qkv_rows(out):
    """[3, B, H, N, hd] head-major -> the GEMM's [B*N, 3D] rows."""
    _, B, H, N, hd = out.shape
    return out.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * hd)


def run_qkv(B: int, N: int, H: int, D: int, device, tile=None, seed: int = 1):
    ops, g = _ops(), _gen(seed)
    M = B * N
    a, w = int_operands((M, D), -4, 4, g, device=device), int_operands((3 * D, D), -4, 4, g, device=device)
    b = int_operands((3 * D,), -64, 64, g, torch.float32, device)
    name = f"qkv_fwd B={B} N={N} H={H} D={D}"
    out = ops.qkv_fwd(a, w, b, B, N, H)
    assert out.shape == (3, B, H, N, D // H)
    assert_exact(_qkv_rows(out), exact_truth(a, w, b, None, torch.bfloat16), name, tile)
    for pr in position_probe(M, 3 * D, D, device):
        assert_position(_qkv_rows(ops.qkv_fwd(pr.a, pr.w, b, B, N, H)), pr, name, tile, bias=b)


def run_residual(M: int, tokens: int, Dout: int, K: int, device, tile=None, seed: int = 2):
    """``linear_residual_fwd`` without dropout: output, bf16 copy and the row statistics
    (sums of squares: operands in [-1, 1], K <= 128), ``st_out`` / ``xb_out`` in canaries."""
    ops, g = _ops(), _gen(seed)
    assert K <= 128 and M % tokens == 0 and Dout % 32 == 0
    a, w = int_operands((M, K), -1, 1, g, device=device), int_operands((Dout, K), -1, 1, g, device=device)
    b = int_operands((Dout,), -2, 2, g, torch.float32, device)
    x = int_operands((M, Dout), -3, 3, g, torch.float32, device)
    st, st_ok = canary((M, Dout // 32, 2), 4 * Dout, torch.float32, device)
    xb, xb_ok = canary((M, Dout), 4 * Dout, torch.bfloat16, device)
    name = f"linear_residual_fwd M={M} tokens={tokens} Dout={Dout} K={K}"
    y = ops.linear_residual_fwd(a, w, b, x, tokens, _rng(device), 3, 0.0, 4, 0.0, st_out=st, xb_out=xb)
    truth, st_truth = exact_truth(a, w, b, x, torch.float32, stats=True)
    assert_exact(y, truth, name, tile)
    assert_exact(xb, truth.to(torch.bfloat16), name + " xb_out", tile)
    assert_exact(st, st_truth, name + " st_out (row, slot*2 + {sum, sum^2})")
    st_ok(name + " st_out")
    xb_ok(name + " xb_out")
    zb, zx = torch.zeros_like(b), torch.zeros_like(x)
    for pr in position_probe(M, Dout, K, device):
        assert_position(ops.linear_residual_fwd(pr.a, pr.w, zb, zx, tokens, _rng(device), 3, 0.0, 4, 0.0), pr, name,
                        tile)


def run_gelu(M: int, N: int, K: int, device, tile=None, seed: int = 3):
    """``linear_gelu_fwd``: ``u`` exact; ``h`` (erf) at the suite's tolerance against the reference."""
    from . import reference as ref
    ops, g = _ops(), _gen(seed)
    a, w = int_operands((M, K), -2, 2, g, device=device), int_operands((N, K), -2, 2, g, device=device)
    b = int_operands((N,), -4, 4, g, torch.float32, device)
    name = f"linear_gelu_fwd M={M} N={N} K={K}"
    u, h = ops.linear_gelu_fwd(a, w, b, _rng(device), 9, 0.0)
    assert_exact(u, exact_truth(a, w, b, None, torch.bfloat16), name + " u", tile)
    _, hr = ref.linear_gelu_fwd(a.cpu(), w.cpu(), b.cpu(), _rng("cpu"), 9, 0.0)
    close(h, hr, 2e-2, 1e-2, name + " h")
    for pr in position_probe(M, N, K, device):
        assert_position(ops.linear_gelu_fwd(pr.a, pr.w, b, _rng(device), 9, 0.0)[0], pr, name + " u", tile, bias=b)


def _rows_to_head_image(rows, B, C, H, W, p):
    """[B*N, C*p*p] head rows (cls rows first of each sample) -> [B, C, H, W] (reference.head_fwd)."""
    y = rows.view(B, -1, rows.shape[-1])[:, 1:, :]
    return y.reshape(B, H // p, W // p, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W).contiguous()


def run_head(B: int, C: int, H: int, W: int, p: int, D: int, device, tile=None, seed: int = 4):
    """``head_fwd`` and ``head_step_`` mode 2 (clamp): weights and bias are multiples of
    1/8, so the clamp to [-1, 1] is exercised and every value still exact; cls rows are
    skipped; ``x`` / ``x0_out`` / ``patches_out`` in canaries (mode 2 must not touch ``x0_out``)."""
    from . import reference as ref
    ops, g = _ops(), _gen(seed)
    N, F = (H // p) * (W // p) + 1, C * p * p
    M = B * N
    a = int_operands((M, D), -1, 1, g, device=device)
    w = (int_operands((F, D), -8, 8, g, torch.float32, device) / 8).to(torch.bfloat16)
    b = int_operands((F,), -8, 8, g, torch.float32, device) / 8
    name = f"head B={B} C={C} {H}x{W} p={p} D={D}"
    img_truth = _rows_to_head_image(exact_truth(a, w, b, None, torch.float32, scale=8), B, C, H, W, p)
    assert_exact(ops.head_fwd(a, w, b, B, C, H, W, p), img_truth, name + " head_fwd")
    x, x_ok = canary((B, C, H, W), 4 * W, torch.float32, device)
    x0, x0_ok = canary((B, C, H, W), 4 * W, torch.float32, device)
    po, po_ok = canary((B * (N - 1), F), 4 * F, torch.bfloat16, device)
    x0_before = x0.clone()
    ops.head_step_(a, w, b, x, x0, None, p, 2, patches_out=po)
    clamped = img_truth.clamp(-1.0, 1.0)
    inside = ((img_truth > -1) & (img_truth < 1)).float().mean().item()
    assert 0.02 < inside < 0.98, f"{name}: the probe does not exercise both sides of the clamp ({inside:.2f} inside)"
    assert_exact(x, clamped, name + " head_step_ x")
    assert_exact(po, ref.patchify_bf16(clamped, p), name + " head_step_ patches_out")
    assert_exact(x0, x0_before, name + " head_step_ mode 2 wrote x0_out")
    for ok, what in ((x_ok, "x"), (x0_ok, "x0_out"), (po_ok, "patches_out")):
        ok(f"{name} head_step_ {what}")
    keep = (torch.arange(M) % N != 0).nonzero().flatten()  # the patch rows
    for pr in position_probe(M, F, D, device):
        rows = ops.image_to_rows(ops.head_fwd(pr.a, pr.w, torch.zeros_like(b), B, C, H, W, p), p)
        assert_position(rows, pr.rows(keep), name + " head_fwd", tile)


def run_patch_embed(B: int, C: int, H: int, W: int, p: int, D: int, device, tile=None, seed: int = 5,
                    stats: bool = False):
    """``patch_embed_fwd`` without dropout: integer image, bias, ``pos``, ``temb`` and ``cls``;
    on a GPU also with ``patches_in`` (the GEMM epilogue then writes the cls rows itself).
    ``stats``: the LayerNorm-fold producer outputs ``ln_st`` / ``xb_out`` in canaries, exact
    (operands in [-1, 1] so the slots' sums of squares stay below 2^24; D % 32 == 0)."""
    from . import reference as ref
    ops, g = _ops(), _gen(seed)
    NP, T = (H // p) * (W // p), 10
    N = NP + 1
    r, e = (1, 2) if stats else (4, 8)
    img = int_operands((B, C, H, W), -r, r, g, torch.float32, device)
    t = torch.randint(0, T, (B,), generator=g).to(device)
    w = int_operands((D, C * p * p), -r, r, g, device=device)
    b, cls = (int_operands((D,), -e, e, g, torch.float32, device) for _ in range(2))
    pos, temb = int_operands((N, D), -e, e, g, torch.float32, device), int_operands((T, D), -e, e, g, torch.float32, device)
    name = f"patch_embed_fwd B={B} C={C} {H}x{W} p={p} D={D}"
    rows = ref.patchify_bf16(img, p)  # a permutation: exact
    res = (pos[1:].unsqueeze(0) + temb[t].unsqueeze(1)).reshape(B * NP, D)
    tok_rows = exact_truth(rows, w, b, res, torch.float32).view(B, NP, D)
    cls_rows = ((cls + pos[0]).unsqueeze(0) + temb[t]).unsqueeze(1)  # [B, 1, D]: small integers, exact
    truth = torch.cat((cls_rows, tok_rows), dim=1)
    on_gpu = torch.device(device).type != "cpu"
    for patches_in in ((None, rows) if on_gpu else (None,)):
        what = name + (" (patches_in: cls rows from the epilogue)" if patches_in is not None else "")
        kw = {} if patches_in is None else {"patches_in": patches_in}
        st = xb = None
        if stats:
            st, st_ok = canary((B * N, D // 32, 2), 4 * D, torch.float32, device)
            xb, xb_ok = canary((B * N, D), 4 * D, torch.bfloat16, device)
        tok, patches = ops.patch_embed_fwd(img, t, w, b, cls, pos, temb, _rng(device), 1, 0.0, p, st, xb, **kw)
        assert_exact(patches.reshape(rows.shape), rows, what + " patches")
        assert_exact(tok, truth, what + " tokens", tile)
        if stats:
            assert_exact(xb.view(B, N, D), truth.to(torch.bfloat16), what + " xb_out", tile)
            # patch rows: slot by slot; cls rows: the slots' total (all a consumer reads -- the
            # patchify launch writes a cls row's whole {sum, sum^2} into slot 0, the epilogue per slot)
            st4, want = st.view(B, N, D // 32, 2), exact_row_stats(truth)
            assert_exact(st4[:, 1:], want[:, 1:], what + " ln_st (patch row, slot*2 + {sum, sum^2})")
            assert float((truth[:, 0].double() ** 2).sum(-1).max()) < EXACT_LIMIT
            assert_exact(st4[:, 0].sum(1), want[:, 0].sum(1), what + " ln_st (cls rows, slots summed)")
            st_ok(what + " ln_st")
            xb_ok(what + " xb_out")


def _cpu(*ts):
    return tuple(None if t is None else t.cpu() for t in ts)


def run_dropout(kind: str, M: int, N: int, p: float, device, tile=None, tokens: int = 1):
    """Dropout placement: constant inputs (A = 0, bias = 1, residual = 0), so the output
    *is* the mask: ``out == 0`` must equal the reference's drop set at the same site and
    the survivors its value, bit for bit.  ``kind``: ``resid_drop`` / ``resid_dp``
    (``tokens`` rows per sample), ``gelu`` (``h`` = dropout(gelu(1)): erf is not exact, so
    the survivors keep the suite's tolerance), ``dgelu`` (dh = 1, gelu'(0) = 1/2)."""
    from . import reference as ref
    ops = _ops()
    K = 64
    r = _rng(device)
    name = f"dropout placement {kind} M={M} N={N} p={p}"
    za, zw = torch.zeros(M, K, dtype=torch.bfloat16, device=device), torch.zeros(N, K, dtype=torch.bfloat16, device=device)
    one = torch.ones(N, device=device)
    if kind in ("resid_drop", "resid_dp"):
        pd, pdp = (p, 0.0) if kind == "resid_drop" else (0.0, p)
        x = torch.zeros(M, N, device=device)
        got = ops.linear_residual_fwd(za, zw, one, x, tokens, r, 3, pd, 4, pdp)
        want = ref.linear_residual_fwd(*_cpu(za, zw, one, x), tokens, _rng("cpu"), 3, pd, 4, pdp)
        if kind == "resid_drop":
            keep = ref.keep_mask(M * N, _rng("cpu"), 3, p).view(M, N)
        else:
            keep = (ref._sample_scale(M // tokens, _rng("cpu"), 4, p, "cpu") != 0).repeat_interleave(tokens)
            keep = keep.unsqueeze(1).expand(M, N)
    elif kind == "gelu":
        _, got = ops.linear_gelu_fwd(za, zw, one, r, 9, p)
        _, want = ref.linear_gelu_fwd(*_cpu(za, zw, one), _rng("cpu"), 9, p)
        keep = ref.keep_mask(M * N, _rng("cpu"), 9, p).view(M, N)
        assert torch.equal(got.cpu() == 0, ~keep), name + ": drop set differs from keep_mask"
        close(got, want, 2e-2, 1e-2, name + " survivors")
        return
    elif kind == "dgelu":
        dy, w = za.clone(), torch.zeros(K, N, dtype=torch.bfloat16, device=device)
        dy[:, 0] = 1
        w[0, :] = 1
        u = torch.zeros(M, N, dtype=torch.bfloat16, device=device)
        got = ops.linear_dgrad_gelu(dy, w, u, r, 11, p)
        want = ref.linear_dgrad_gelu(*_cpu(dy, w, u), _rng("cpu"), 11, p)
        keep = ref.keep_mask(M * N, _rng("cpu"), 11, p).view(M, N)
    else:
        raise ValueError(kind)
    assert 0 < int((~keep).sum()) < keep.numel() or kind == "resid_dp", name + ": degenerate mask"
    assert torch.equal(got.cpu() == 0, ~keep), name + ": drop set differs from the reference's mask"
    assert_exact(got.cpu(), want, name + " survivors", tile)


def run_dropout_embed(B: int, H: int, W: int, p_patch: int, D: int, p: float, device, tile=None):
    """EMBED dropout placement: zero image and weights, bias = cls = 1, pos = temb = 0."""
    from . import reference as ref
    ops = _ops()
    C, T = 3, 4
    N = (H // p_patch) * (W // p_patch) + 1
    img = torch.zeros(B, C, H, W, device=device)
    t = torch.zeros(B, dtype=torch.int64, device=device)
    w = torch.zeros(D, C * p_patch * p_patch, dtype=torch.bfloat16, device=device)
    b, cls = torch.ones(D, device=device), torch.ones(D, device=device)
    pos, temb = torch.zeros(N, D, device=device), torch.zeros(T, D, device=device)
    name = f"dropout placement embed B={B} {H}x{W} p={p_patch} D={D} p_drop={p}"
    got, _ = ops.patch_embed_fwd(img, t, w, b, cls, pos, temb, _rng(device), 1, p, p_patch)
    want, _ = ref.patch_embed_fwd(*_cpu(img, t, w, b, cls, pos, temb), _rng("cpu"), 1, p, p_patch)
    keep = ref.keep_mask(B * N * D, _rng("cpu"), 1, p).view(B, N, D)
    assert torch.equal(got.cpu() == 0, ~keep), name + ": drop set differs from keep_mask"
    assert_exact(got.cpu(), want, name + " survivors", tile)


def dgrad_splits(nout: int) -> List[int]:
    """The K splits in {2, 3, 4} the dgrad binding accepts for a reduction of ``nout``
    (every slice non-empty); the last is the largest."""
    kt = (nout + 63) // 64
    return [s for s in (2, 3, 4) if s <= kt and (kt + s - 1) // s * (s - 1) < kt]


def run_dgrad(M: int, Nout: int, K: int, device, tile=None, splits=(1,), seed: int = 6):
    """``linear_dgrad`` (transposed B), fp32 and bf16; with ``splits`` > 1 every slice is
    exact and three launches are bit-identical."""
    ops, g = _ops(), _gen(seed)
    dy, w = int_operands((M, Nout), -4, 4, g, device=device), int_operands((Nout, K), -4, 4, g, device=device)
    wt = w.t().contiguous()
    probes = position_probe(M, K, Nout, device)
    for f32 in (True, False):
        dt = torch.float32 if f32 else torch.bfloat16
        for s in splits:
            name = f"linear_dgrad M={M} Nout={Nout} K={K} {'f32' if f32 else 'bf16'} splits={s}"
            got = ops.linear_dgrad(dy, w, f32, s)
            if s == 1:
                assert_exact(got, exact_truth(dy, wt, None, None, dt), name, tile)
                for pr in probes:
                    assert_position(ops.linear_dgrad(pr.a, pr.w.t().contiguous(), f32, 1), pr, name, tile)
                continue
            step = ((Nout + 63) // 64 + s - 1) // s * 64
            assert got.shape == (s, M, K)
            for z in range(s):
                sl = slice(z * step, min((z + 1) * step, Nout))
                assert_exact(got[z], exact_truth(dy[:, sl], wt[:, sl], None, None, dt), f"{name} slice {z}", tile)
            for _ in range(2):
                assert torch.equal(_bits(ops.linear_dgrad(dy, w, f32, s)), _bits(got)), name + ": launches differ"


def run_dgrad_ln(M: int, Nout: int, K: int, s: int, device, seed: int = 7):
    """``layernorm_bwd`` summing fp32 dgrad slices on load (suite tolerance: its arithmetic
    is not integer), ``dgamma`` / ``dbeta`` in canaries."""
    from . import reference as ref
    ops, g = _ops(), _gen(seed)
    dy, w = int_operands((M, Nout), -2, 2, g, device=device), int_operands((Nout, K), -2, 2, g, device=device)
    dx = ops.linear_dgrad(dy, w, True, s)
    x = torch.randn(M, K, generator=g).to(device)
    gam, bet = torch.randn(K, generator=g).to(device), torch.randn(K, generator=g).to(device)
    _, mu, rs = ref.layernorm_fwd(x, gam, bet)
    dg, dg_ok = canary((K,), 64, torch.float32, device)
    db, db_ok = canary((K,), 64, torch.float32, device)
    dg.zero_()
    db.zero_()
    go, _ = ops.layernorm_bwd(dx, x, mu, rs, gam, None, dg, db, M, _rng(device), 0, 0.0, 0, 0.0, False)
    dg2, db2 = torch.zeros(K), torch.zeros(K)
    total = exact_truth(dy, w.t().contiguous(), None, None, torch.float32).cpu()
    gor, _ = ref.layernorm_bwd(total, *_cpu(x, mu, rs, gam), None, dg2, db2, M, _rng("cpu"), 0, 0.0, 0, 0.0, False)
    scale = float(total.abs().max())
    close(go, gor, 1e-4 * scale, 1e-4, "ln g_out (summed slices)")
    close(dg, dg2, 1e-2 * scale, 1e-4, "ln dgamma (summed slices)")
    close(db, db2, 1e-2 * scale, 1e-4, "ln dbeta (summed slices)")
    dg_ok("layernorm_bwd dgamma")
    db_ok("layernorm_bwd dbeta")


def run_dgrad_gelu(M: int, Nout: int, K: int, device, tile=None, with_wt: bool = False, seed: int = 8):
    """``linear_dgrad_gelu``: at u = 0 (gelu' = 1/2 exactly) and p = 0 the output is
    bf16(dh / 2), exact; with u != 0 and p = 0.1 the drop set is exact (dh > 0 everywhere)
    and the values keep the suite's tolerance."""
    from . import reference as ref
    ops, g = _ops(), _gen(seed)
    dy, w = int_operands((M, Nout), -4, 4, g, device=device), int_operands((Nout, K), -4, 4, g, device=device)
    wt = w.t().contiguous()
    kw = {"wt": wt} if with_wt else {}
    name = f"linear_dgrad_gelu M={M} Nout={Nout} K={K}{' wt' if with_wt else ''}"
    u0 = torch.zeros(M, K, dtype=torch.bfloat16, device=device)
    got = ops.linear_dgrad_gelu(dy, w, u0, _rng(device), 11, 0.0, **kw)
    assert_exact(got, (exact_truth(dy, wt, None, None, torch.float32) * 0.5).to(torch.bfloat16), name + " u=0", tile)
    dy, w = int_operands((M, Nout), 1, 3, g, device=device), int_operands((Nout, K), 1, 3, g, device=device)
    kw = {"wt": w.t().contiguous()} if with_wt else {}
    u = int_operands((M, K), -2, 2, g, device=device)
    got = ops.linear_dgrad_gelu(dy, w, u, _rng(device), 11, 0.1, **kw)
    want = ref.linear_dgrad_gelu(*_cpu(dy, w, u), _rng("cpu"), 11, 0.1)
    keep = ref.keep_mask(M * K, _rng("cpu"), 11, 0.1).view(M, K)
    assert torch.equal(got.cpu() == 0, ~keep), name + ": drop set differs from keep_mask"
    close(got, want, 2e-2, 1e-2, name + " values")


def _wgrad_job(T, Nout, K, with_db, store, g, device, lo=-4, hi=4):
    dy, x = int_operands((T, Nout), lo, hi, g, device=device), int_operands((T, K), lo, hi, g, device=device)
    dw, dw_ok = canary((Nout, K), 4 * K, torch.float32, device)
    dw.copy_(torch.zeros(Nout, K) if store else int_operands((Nout, K), -8, 8, g, torch.float32))
    db = db_ok = db_truth = None
    dw_truth = exact_truth(dy.t(), x.t(), None, dw.clone(), torch.float32)
    if with_db:
        db, db_ok = canary((Nout,), 64, torch.float32, device)
        db.copy_(torch.zeros(Nout) if store else int_operands((Nout,), -8, 8, g, torch.float32))
        db_truth = exact_truth(dy.t(), torch.ones(1, T, dtype=dy.dtype, device=device), None,
                               db.clone().unsqueeze(1), torch.float32).squeeze(1)
    return (dy, x, dw, db), (dw_truth, db_truth), (dw_ok, db_ok)


def _wgrad_check(jobs, truths, oks, name):
    for i, ((dy, x, dw, db), (dwt, dbt), (dw_ok, db_ok)) in enumerate(zip(jobs, truths, oks)):
        nm = f"{name} problem {i} (tokens={dy.shape[0]} Nout={dy.shape[1]} K={x.shape[1]})"
        assert_exact(dw, dwt, nm + " dw", (64, 64))
        dw_ok(nm + " dw")
        if db is not None:
            assert_exact(db, dbt, nm + " db")
            db_ok(nm + " db")


def run_wgrad(T: int, Nout: int, K: int, device, with_db: bool, seed: int = 9):
    """``linear_wgrad`` (transposed A, read-add-write): integer initial ``dw`` / ``db`` in canaries."""
    ops, g = _ops(), _gen(seed)
    job, truth, ok = _wgrad_job(T, Nout, K, with_db, False, g, device)
    ops.linear_wgrad(*job)
    _wgrad_check([job], [truth], [ok], "linear_wgrad")
    for pr in position_probe(Nout, K, T, device):  # dW = dy^T x: the probe's A is dy^T, its W is x^T
        dw = torch.zeros(Nout, K, device=device)
        ops.linear_wgrad(pr.a.t().contiguous(), pr.w.t().contiguous(), dw, None)
        assert_position(dw, pr, f"linear_wgrad tokens={T} Nout={Nout} K={K}", (64, 64))


def run_wgrad_multi(T: int, shapes, device, store: bool, seed: int = 10, lo: int = -4, hi: int = 4, repeats: int = 1):
    """``linear_wgrad_multi``: every (Nout, K, with_db) of ``shapes`` in one launch over ``T``
    tokens; ``repeats`` > 1: the launches are bit-identical."""
    ops = _ops()
    outs = []
    for _ in range(repeats):
        g = _gen(seed)
        built = [_wgrad_job(T, n, k, hb, store, g, device, lo, hi) for n, k, hb in shapes]
        jobs, truths, oks = (list(z) for z in zip(*built))
        ops.linear_wgrad_multi(jobs, store=store)
        _wgrad_check(jobs, truths, oks, f"linear_wgrad_multi store={store}")
        outs.append(jobs)
    for jobs in outs[1:]:
        for (_, _, dw, db), (_, _, dw0, db0) in zip(jobs, outs[0]):
            assert torch.equal(_bits(dw), _bits(dw0)) and (db is None or torch.equal(_bits(db), _bits(db0))), \
                "weight gradients differ between launches"


def run_wgrad_sq(T: int, shapes, device, store: bool, seed: int = 11, lo: int = -2, hi: int = 2):
    """``sq=`` grad-norm partials of ``linear_wgrad_multi``: dw / db are views of one arena
    with integer gaps; dw / db exact, and the fp64 sum of the partials equals the exact
    integer sum of squares of the arena to 1e-6 relative (the squares exceed 2^24)."""
    ops, g = _ops(), _gen(seed)
    gap = 320
    n_el = sum(n * k + (n if hb else 0) + gap for n, k, hb in shapes) + gap
    arena = int_operands((n_el,), -8, 8, g, torch.float32, device)
    off, jobs, truths, tiles = gap, [], [], 0
    for n, k, hb in shapes:
        dy, x = int_operands((T, n), lo, hi, g, device=device), int_operands((T, k), lo, hi, g, device=device)
        dw = arena[off:off + n * k].view(n, k)
        off += n * k
        db = None
        if hb:
            db = arena[off:off + n]
            off += n
        if len(jobs) < 5:  # gaps no tile writes (the launch takes at most 16 such ranges)
            off += gap
        if store:
            dw.zero_()
            if db is not None:
                db.zero_()
        dwt = exact_truth(dy.t(), x.t(), None, dw.clone(), torch.float32)
        dbt = None if db is None else exact_truth(dy.t(), torch.ones(1, T, dtype=dy.dtype, device=device), None,
                                                  db.clone().unsqueeze(1), torch.float32).squeeze(1)
        jobs.append((dy, x, dw, db))
        truths.append((dwt, dbt))
        tiles += -(-n // 64) * -(-k // 64)
    parts = torch.full((ops.sq_parts_size(tiles),), float("nan"), device=device)
    ops.linear_wgrad_multi(jobs, store=store, sq=(parts, arena, None))
    for (dy, x, dw, db), (dwt, dbt) in zip(jobs, truths):
        assert_exact(dw, dwt, f"wgrad_multi sq= dw tokens={T}", (64, 64))
        if db is not None:
            assert_exact(db, dbt, f"wgrad_multi sq= db tokens={T}")
    assert torch.isfinite(parts).all(), "every partial slot is written"
    expect = int((arena.double() ** 2).sum().item())
    got = parts.double().sum().item()
    assert abs(got - expect) <= 1e-6 * expect, f"grad-norm partials sum {got!r}, exact {expect}"


# ----------------------------------------------------------------------------- LayerNorm-fold consumers
# The fold epilogue computes rstd * (acc - mean * c) + b with (mean, rstd) from the row
# statistics st[m][K/32] = {sum x, sum x^2}.  ``st`` and ``c`` are inputs of the op, so the
# probe *constructs* them instead of deriving them from ``a``: row m gets an integer mean code
# mu_m and a standard deviation sigma_m in {1/2, 1, 2, 4}, i.e. totals sum x = K mu_m and
# sum x^2 = K (sigma_m^2 + mu_m^2), split over the slots as distinct integers; column n gets an
# integer code c_n; eps = 0.  For K a power of two 1/K is exact, so mean = mu_m, var = sigma_m^2,
# rstd = 1 / sigma_m in {2, 1, 1/2, 1/4} and every later operation are exact in fp32 in any
# order, with or without FMA contraction: the output is unique to the bit.  (This rests on the
# hardware reciprocal square root being exact at 1/4, 1, 4 and 16; the returned ``ln_rstd`` is
# asserted first -- see tests/test_gemm_exact_gpu.py for what was measured.)  For K = 192 / 384
# the host's 1/K is rounded and the same probe is compared within a bound derived from the
# operands (:func:`fold_bound`).
FOLD_SIGMAS = (0.5, 1.0, 2.0, 4.0)
FOLD_EXACT_KS = (64, 128, 256, 512)   # 2, 4, 8 and 16 statistics slots
FOLD_BOUNDED_KS = (384,)              # the model's K: 12 slots, 1/K rounded
FOLD_QKV_SHAPES = ((3, 17, 2, 64), (2, 5, 4, 128), (2, 17, 4, 256), (1, 9, 8, 512))  # (B, N, H, D): D a power of two
FOLD_QKV_BOUNDED = ((2, 17, 3, 192), (2, 5, 6, 384))
FOLD_KINDS = ("linear", "qkv", "gelu", "head")


def _pow2(k: int) -> bool:
    return k & (k - 1) == 0


def fold_codes(M: int, N: int, K: int):
    """(mu [M], sigma [M], c [N]) fp64: neighbouring rows and columns 16 apart differ in code.
    |mu| <= 11 for K a power of two, <= 4 otherwise (codes one apart then stay separated by
    far more than :func:`fold_bound`); |c| <= 6."""
    mod = 23 if _pow2(K) else 9
    m, n = torch.arange(M, dtype=torch.float64), torch.arange(N, dtype=torch.float64)
    mu = (5 * m) % mod - mod // 2
    sigma = torch.tensor(FOLD_SIGMAS, dtype=torch.float64)[torch.arange(M) % 4]
    return mu, sigma, (7 * n) % 13 - 6


def fold_stats(mu, sigma, K: int) -> torch.Tensor:
    """Row statistics [M, K/32, 2] fp32 with totals ``K mu`` and ``K (sigma^2 + mu^2)``, every
    slot a distinct non-zero integer that also differs from the same slot of the next row: a
    dropped, duplicated or neighbouring-row slot changes a total (asserted here)."""
    M, NP = mu.shape[0], K // 32
    assert K % 32 == 0 and 2 <= NP <= 16
    tot = torch.stack((K * mu, K * (sigma * sigma + mu * mu)), dim=-1).tolist()  # [M, 2]
    rows = []
    for m in range(M):
        comps = []
        for k, (step, rstep, rmod) in enumerate(((3, 5, 7), (4, 7, 5))):
            free = [step * j + rstep * (m % rmod) + 1 + k for j in range(NP - 1)]
            prev = rows[-1][k] if rows else None
            while True:  # the last slot closes the total; bump slot 0 until no two coincide
                s = free + [tot[m][k] - sum(free)]
                if len(set(s)) == NP and 0 not in s and (prev is None or all(x != y for x, y in zip(s, prev))):
                    break
                free[0] += 1
            comps.append(s)
        rows.append(comps)
    st = torch.tensor(rows, dtype=torch.float64).transpose(1, 2).contiguous()   # [M, NP, 2]
    assert bool((st == st.round()).all()) and float(st.abs().sum(1).max()) < EXACT_LIMIT and bool((st != 0).all())
    want = torch.tensor(tot, dtype=torch.float64)
    assert torch.equal(st.sum(1), want)
    for k in range(2):
        s = st[..., k]
        srt = s.sort(dim=1).values
        assert bool((srt[:, 1:] != srt[:, :-1]).all()), "fold_stats: two slots of a row coincide"
        assert M == 1 or bool((s[1:] != s[:-1]).all()), "fold_stats: a slot equals the next row's"
    return st.float()


def fold_truth_exact(a, w, bias, mu, sigma, c, scale: int = 1):
    """fp64 ``(a @ w.T - mu c) / sigma + bias`` of the probe, after asserting the exactness
    condition on its own tensors: every value an integer / ``scale`` (a power of two), and
    ``(K max|a| max|w| + max|mu c|) / min sigma + max|bias|``, on the scaled values, below 2^24."""
    assert scale >= 1 and _pow2(scale)
    K = a.shape[-1]
    for t in (a, w, bias):
        assert _is_int(t.double() * scale), "fold probe: operands must be integers / scale"
    assert _is_int(mu) and _is_int(c) and _is_int(sigma * 2), "fold probe: codes must be integers, sigma dyadic"
    bound = (K * _amax(a) * _amax(w) + _amax(mu) * _amax(c)) / float(sigma.min()) * scale * 2 + _amax(bias) * scale
    assert bound < EXACT_LIMIT, f"exactness condition violated: {bound:.0f} >= 2^24 (K = {K})"
    acc = a.double().cpu() @ w.double().cpu().t()
    y = (acc - mu.unsqueeze(1) * c.unsqueeze(0)) / sigma.unsqueeze(1) + bias.double().cpu()
    return y, acc


def fold_bound(acc, mu, sigma, c):
    """K not a power of two: the host's 1/K, hence mean and var, carry an fp32 rounding:
    ``2^-22 (1 + mu^2/sigma^2) |acc - mu c| / sigma + 2^-22 |mu c| / sigma`` per element."""
    mc = mu.unsqueeze(1) * c.unsqueeze(0)
    s = sigma.unsqueeze(1)
    return 2.0 ** -22 * ((1 + (mu / sigma).pow(2)).unsqueeze(1) * (acc - mc).abs() + mc.abs()) / s


def _fold_report(got, want, acc, mu, sigma, c, bias, bad, first: int = 4) -> str:
    """Which (row code, column code) the observed values decode to."""
    lines = []
    g = got.double().cpu()
    for r, col in bad[:first].tolist():
        if not bool(torch.isfinite(g[r, col])):
            lines.append(f"  [{r}, {col}] got {float(g[r, col])!r} want {float(want[r, col])!r}")
            continue
        t = float(acc[r, col] - (g[r, col] - float(bias[col])) * sigma[r])  # the mean * c the value shows
        line = f"  [{r}, {col}] got {float(g[r, col])!r} want {float(want[r, col])!r}: shows mean * c = {t:g}, " \
               f"expected {float(mu[r]):g} * {float(c[col]):g}"
        if c[col] != 0 and t / float(c[col]) == round(t / float(c[col])):
            rows = (mu == t / float(c[col])).nonzero().flatten()[:4].tolist()
            line += f"; with this column's c the mean code {t / float(c[col]):g} (rows {rows})"
        if mu[r] != 0 and t / float(mu[r]) == round(t / float(mu[r])):
            cols = (c == t / float(mu[r])).nonzero().flatten()[:4].tolist()
            line += f"; with this row's mean the column code {t / float(mu[r]):g} (columns {cols})"
        lines.append(line)
    return "\n".join(lines)


def assert_fold(got, y, acc, mu, sigma, c, bias, K: int, name: str = "", tile=None):
    """``got`` ([M, N] GEMM rows) against the probe's truth ``y``: bit for bit for K a power of
    two; otherwise between the roundings (to the output type: rounding is monotonic) of
    ``y -/+`` :func:`fold_bound`.  A mismatch is decoded (:func:`_fold_report`)."""
    got = got.cpu()
    if _pow2(K):
        truth = y.to(got.dtype)
        bad = mismatches(got, truth)
        if bad.shape[0] == 0:
            return
        try:
            assert_exact(got, truth, name, tile, 0)
        except AssertionError as e:
            raise AssertionError(str(e) + "\n" + _fold_report(got, y, acc, mu, sigma, c, bias, bad)) from None
    bnd = fold_bound(acc, mu, sigma, c)
    lo, hi = (y - bnd).to(got.dtype).double(), (y + bnd).to(got.dtype).double()
    g = got.double()
    bad = (~((g >= lo) & (g <= hi))).nonzero()  # NaN counts as a mismatch
    assert bad.shape[0] == 0, f"{name}: {bad.shape[0]} of {got.numel()} elements outside the operand bound\n" + \
        _fold_report(got, y, acc, mu, sigma, c, bias, bad)


def assert_fold_stats(mean, rstd, mu, sigma, K: int, name: str = ""):
    """The returned ``ln_mean`` / ``ln_rstd``: bit for bit (K a power of two), else within
    2^-22 |mu| and 2^-22 (1 + mu^2 / sigma^2) / sigma."""
    if _pow2(K):
        assert_exact(rstd.cpu(), (1.0 / sigma).float(), name + " ln_rstd (the reciprocal square root at 1/4, 1, 4, 16)")
        assert_exact(mean.cpu(), mu.float(), name + " ln_mean")
        return
    em, er = (mean.double().cpu() - mu).abs(), (rstd.double().cpu() - 1.0 / sigma).abs()
    assert bool((em <= 2.0 ** -22 * mu.abs()).all()), f"{name} ln_mean: max err {float(em.max()):.3e}"
    assert bool((er <= 2.0 ** -22 * (1 + (mu / sigma).pow(2)) / sigma).all()), f"{name} ln_rstd: max err {float(er.max()):.3e}"


def run_fold_consumer(kind: str, M: int, N: int, K: int, device, tile=None, geom=None, seed: int = 13):
    """A LayerNorm-fold consumer on the constructed-statistics probe, once with random
    integer ``a`` and once with ``a = 0`` (the output ``-mu_m c_n / sigma_m + b_n`` then names
    both indices).  ``kind``: ``linear`` (bf16 and f32), ``qkv`` (``geom`` = (B, tokens, H);
    N = 3 K), ``gelu`` (``u``), ``head`` (``geom`` = (B, C, H, W, p); ``head_fwd`` and
    ``head_step_`` mode 2, weights and bias / 8).  Returned statistics and ``head_step_``'s ``x``
    sit in canaries; ``ln_rstd`` is asserted before any output."""
    ops, g = _ops(), _gen(seed)
    head = kind == "head"
    scale = 8 if head else 1
    w = int_operands((N, K), -2 * scale, 2 * scale, g, torch.float32) / scale
    b = int_operands((N,), -8 * scale, 8 * scale, g, torch.float32) / scale
    mu, sigma, c = fold_codes(M, N, K)
    st, cd = fold_stats(mu, sigma, K).to(device), c.float().to(device)
    wd, bd = w.to(torch.bfloat16).to(device), b.to(device)
    for pure in (False, True):
        a = torch.zeros(M, K, dtype=torch.bfloat16) if pure else int_operands((M, K), -2, 2, g)
        y, acc = fold_truth_exact(a, w, b, mu, sigma, c, scale)
        ad = a.to(device)
        name = f"fold {kind} M={M} N={N} K={K}{' a=0' if pure else ''}"
        mean, mean_ok = canary((M,), 64, torch.float32, device)
        rstd, rstd_ok = canary((M,), 64, torch.float32, device)
        fold = (st, cd, 0.0, mean, rstd)
        outs = []
        if kind == "linear":
            for f32 in (False, True):
                outs.append((f"{name} {'f32' if f32 else 'bf16'}", ops.linear_fwd(ad, wd, bd, f32, fold=fold[:3])))
            mean = None  # linear_fwd returns no statistics
        elif kind == "qkv":
            B, tokens, H = geom
            assert B * tokens == M and N == 3 * K
            outs.append((name, _qkv_rows(ops.qkv_fwd(ad, wd, bd, B, tokens, H, fold=fold))))
        elif kind == "gelu":
            outs.append((name + " u", ops.linear_gelu_fwd(ad, wd, bd, _rng(device), 9, 0.0, fold=fold)[0]))
        elif head:
            B, C, H, W, p = geom
            assert B * ((H // p) * (W // p) + 1) == M and N == C * p * p
            img = ops.head_fwd(ad, wd, bd, B, C, H, W, p, fold=fold)
            x, x_ok = canary((B, C, H, W), 4 * W, torch.float32, device)
            ops.head_step_(ad, wd, bd, x, None, None, p, 2, fold=fold[:3])
        else:
            raise ValueError(kind)
        if mean is not None:
            assert_fold_stats(mean, rstd, mu, sigma, K, name)
            mean_ok(name + " ln_mean")
            rstd_ok(name + " ln_rstd")
        if head:
            keep = (torch.arange(M) % (M // B) != 0).nonzero().flatten()  # cls rows are skipped
            args = (y[keep], acc[keep], mu[keep], sigma[keep], c, b, K)
            assert_fold(ops.image_to_rows(img, p), *args, name + " head_fwd", tile)
            # clamp (monotonic, exact) applied to both sides of the comparison
            rows = ops.image_to_rows(x, p).cpu()
            inside = ((y[keep] > -1) & (y[keep] < 1)).double().mean().item()
            assert pure or 0.01 < inside < 0.99, f"{name}: the probe does not exercise both sides of the clamp"
            if _pow2(K):
                assert_exact(rows, y[keep].clamp(-1.0, 1.0).float(), name + " head_step_ x", tile)
            else:
                unclamped = (rows.abs() < 1)
                assert_fold(torch.where(unclamped, rows, y[keep].float()), *args, name + " head_step_ x", tile)
            x_ok(name + " head_step_ x")
        for nm, out in outs:
            assert_fold(out, y, acc, mu, sigma, c, b, K, nm, tile)
