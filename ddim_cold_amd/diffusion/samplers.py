"""Samplers: DDIM k-step (+ trajectory), cold de-pixelation, draft->drawing img2img, inpainting.

Reference behaviour: ``ViT.py:220-256`` (DDIM sampler / sequence),
``ViT_draft2drawing.py:259-309`` (cold sampler / sequence),
``ViT_draft2drawing.py:378-419`` (img2img).

MI355X design: the reference issues one H2D timestep copy, ~150 forward
kernels and ~8 elementwise DDIM kernels per step from Python and syncs with a
D2H copy per recorded step.  Here the *whole* sampling loop is captured once
as a hipGraph (static noise buffer, device-resident timestep and coefficient
tables, the fused ``ddim_step_`` kernel doing clamp + eps-hat + update in one
fp32 pass, trajectory written to a device buffer and copied back once), so a
replay is a single host call.  Graphs are cached per (N, k) and re-captured
if the weights they read were reallocated.

Sampling always runs the denoiser in eval mode (no dropout); the reference's
``ViT.py`` CLI forgot ``model.eval()``.

Every step is ONE forward whose head-GEMM epilogue applies the step (DDIM
update, cold clamp, or img2img's DDIM update with per-sample coefficients) and
hands the next step its bf16 patch rows; the cold sampler of an x0-predicting model
(``ColdSampler(predict="x0")``) instead follows each forward with one
:func:`ops.cold_step_` launch, and inpainting (:func:`inpaint`) each forward with one
:func:`ops.repaint_rows_` launch that pastes the kept region back, and the DPM-Solver++(2M)
solver (``DDIMSampler(solver="dpmpp2m")``) each forward with one :func:`ops.dpm2m_rows_` launch
that applies the second-order multistep update.  (Splitting a batch into concurrent
chains on separate streams measured slower on MI355X -- ViT-tiny N=64 k=20:
46.9 / 56.2 / 76.2 ms for 1 / 2 / 4 chains -- and was removed.)
"""
from __future__ import annotations

import time
from typing import List, Optional, Sequence

import torch

from .. import ops
from ..models.program import HeadStep, fold_width_ok, model_tensors
from .schedule import (ETA_IDENT_ROW, cold_steps, ddim_coefficients, ddim_coefficients_eta, ddim_table,
                       ddim_table_eta, dpm2m_row, dpm2m_step_h, dpm2m_table, eta_row, img2img_alpha, repaint_table)


def _use_fused(model, device) -> bool:
    from ..models.vit import _fused_allowed
    probe = torch.empty(0, device=device)
    return _fused_allowed(probe)


class _Denoiser:
    """x0-prediction f(x, t) in eval mode via the fused program (GPU) or the reference (CPU)."""

    def __init__(self, model, device):
        self.model = model
        self.device = torch.device(device)
        self.fused = _use_fused(model, self.device)
        if self.fused:
            self.prog = model.program()
            self.P = model_tensors(model)
            self.rng = torch.zeros(2, dtype=torch.int64, device=self.device)

    def key(self):
        return self.key_of(self.model)

    @staticmethod
    def key_of(model):
        """What a captured loop depends on: the engine whose arenas it reads, or the
        parameters' storage + version (checked per call before any denoiser is built:
        building one costs ~0.25 ms of host time)."""
        eng = getattr(model, "_engine", None)
        if eng is not None:
            return ("engine", id(eng))
        return tuple((p.data_ptr(), p._version) for p in model.parameters())

    def step_(self, x, t, hs: HeadStep):
        """In-place sampler step on ``x`` with the update fused into the head GEMM
        (``ops.HEAD_DDIM``: DDIM with ``hs.coef``, x0-hat into ``hs.x0_out``; ``ops.HEAD_CLAMP``:
        clamp).  ``hs.patches_in`` / ``hs.patches_out``: bf16 patch rows of ``x`` handed from
        one step's head epilogue to the next step's patch embedding (no patchify
        launch per step; ``patches_in`` None on the first step)."""
        if self.fused:
            self.prog.forward(self.P, x, t, self.rng, False, save=False, head_step=hs)
            return
        x0_raw = self(x, t)
        if hs.mode == ops.HEAD_CLAMP:
            torch.clamp(x0_raw, -1.0, 1.0, out=x)
        else:
            ops.ddim_step_(x, x0_raw, hs.x0_out, hs.coef)

    def x0_(self, x, t, hs: HeadStep):
        """Clamped x0-hat of f(x, t) into ``hs.x0_out``; ``x`` is left exactly as it is (the
        cold x0 sampler's forward: its update is :func:`ops.cold_step_`).  Fused: ``hs`` is
        ``ops.HEAD_DDIM`` with the coefficient row {0, 1, 0, 1} (x_next = x_t)."""
        if self.fused:
            self.step_(x, t, hs)
            return
        torch.clamp(self(x, t), -1.0, 1.0, out=hs.x0_out)

    def __call__(self, x, t):
        if self.fused:
            out, _ = self.prog.forward(self.P, x, t, self.rng, False, save=False)
            return out
        was = self.model.training
        self.model.eval()
        try:
            return self.model.forward_reference(x, t)
        finally:
            self.model.train(was)


# module constants, read when a loop is built: tests switch them to compare the paths.
# The head epilogue of each step also writes the new x_t as the next step's bf16
# patch rows, so every step after the first skips the patchify launch
PATCH_CHAIN = True


def _patch_rows(model, N: int, device, den) -> Optional[torch.Tensor]:
    """bf16 [N*P, C*p*p] hand-off buffer for the patch-row chain (None: not used)."""
    if not (PATCH_CHAIN and den.fused):
        return None
    p = model.patch_size
    H, W = model.img_size
    return torch.empty(N * (H // p) * (W // p), model.in_chans * p * p, dtype=torch.bfloat16, device=device)


# the sampler state as fp32 patch rows in the head's output column order
# (ops.image_to_rows): the head epilogue's x_t / x0 / x_next / bf16 patch-row accesses
# are contiguous 16-byte vectors (ops.head_step_rows_) instead of scattered pixels,
# and the first step needs no patchify launch either (head GEMM at N=64: 12.2 -> 7.0
# us, k=20 N=64 sampler 33.40 -> 32.90 ms per batch; profiles/sampler_rows_ab.txt)
ROWS = True


class _History:
    """The x0-hat history of a multistep loop (DPM-Solver++(2M)): ``x0`` is the buffer the
    step's forward writes, ``x0_prev`` the one the step before wrote, and the two trade places
    between steps.  The loop is unrolled at capture, so the swap renames two buffers: no copy,
    no store."""

    def history(self, steps: int):
        """Start a loop of ``steps`` steps: the last one writes the state's own ``x0``."""
        if getattr(self, "_x0_pair", None) is None:
            self._x0_pair = (self.x0, torch.zeros_like(self.x0))
        a, b = self._x0_pair
        self.x0, self.x0_prev = (a, b) if steps % 2 else (b, a)

    def swap_x0(self):
        self.x0, self.x0_prev = self.x0_prev, self.x0


class _Rows(_History):
    """Patch-row state of one captured sampling loop (GPU fused path only).

    Inside the loop: :meth:`begin` converts the [N, C, H, W] start image once and
    permutes the patch-embedding weight's columns into the head's order (so a
    replay after training uses the current weights); :meth:`step` is one forward
    with the update in the head epilogue; :meth:`image` converts rows back and
    :meth:`write_back` copies the state / x0-hat to the loop's image buffers."""
    rows = True

    def __init__(self, model, N: int, device, den):
        p = model.patch_size
        H, W = model.img_size
        C = model.in_chans
        NP, F = (H // p) * (W // p), C * p * p
        self.den, self.p, self.shape = den, p, (N, C, H, W)
        self.x = torch.zeros(N * NP, F, device=device)
        self.x0 = torch.zeros_like(self.x)
        self.pin = torch.empty(N * NP, F, dtype=torch.bfloat16, device=device)
        self.w = torch.empty_like(den.P.pe_w)

    def begin(self, x_img):
        self.w.copy_(ops.embed_weight_rows(self.den.P.pe_w, self.shape[1], self.p))
        self.x.copy_(ops.image_to_rows(x_img, self.p))
        self.pin.copy_(self.x)

    def step(self, t, mode: int, coef=None, noise=None):
        """``noise = (rng, site)`` (``ops.HEAD_ETA`` / ``HEAD_ETA_EACH``): the step's noise, drawn
        in the head epilogue."""
        x0 = None if mode == ops.HEAD_CLAMP else self.x0.view(self.shape)
        self.den.step_(self.x.view(self.shape), t, HeadStep(mode, x0, coef, self.pin, self.pin, self.w, noise))

    def predict_x0(self, t):
        """One forward from the bf16 rows in ``pin`` with the clamp aimed at the ``x0``
        rows: ``x`` and ``pin`` stay as they are (the embedding reads only ``pin``)."""
        self.den.step_(self.x0.view(self.shape), t, HeadStep(ops.HEAD_CLAMP, patches_in=self.pin, rows_w=self.w))

    def cold_step(self, t, algorithm: int):
        """``x`` <- cold step from ``x0`` (per-sample ``t``), and its bf16 rows into ``pin``."""
        N, C, H, W = self.shape
        ops.cold_step_rows_(self.x, self.x0, t, N, C, H, W, self.p, algorithm, patches_out=self.pin)

    def repaint(self, known, mask, coef, rng, site_paste: int, site_jump: int):
        """Inpainting mask step on ``x`` (``known`` / ``mask`` as patch rows), its bf16 rows into ``pin``."""
        ops.repaint_rows_(self.x, known, mask, coef, rng, site_paste, site_jump, patches_out=self.pin)

    def dpm_step(self, coef, each: bool):
        """``x`` <- DPM-Solver++(2M) step from ``x0`` / ``x0_prev`` (``coef``: one row of 8, or
        ``each``: one per sample), and its bf16 rows into ``pin``."""
        ops.dpm2m_rows_(self.x, self.x0, self.x0_prev, coef, self.shape[0], each, patches_out=self.pin)

    def image(self, xr):
        return ops.rows_to_image(xr, *self.shape, self.p)

    def write_back(self, x=None, x0=None):
        if x0 is not None:
            x0.copy_(self.image(self.x0))
        if x is not None:
            x.copy_(self.image(self.x))


class _Image(_History):
    """Image-layout state of one sampling loop, with the interface of :class:`_Rows` (the
    CPU, ``ROWS`` / ``PATCH_CHAIN`` off, a stochastic loop of the unfolded program): ``x`` and
    ``x0`` are the loop's own [N, C, H, W] buffers (``x0`` None: one of its own), so nothing
    is converted or copied back.  ``chain``: each step's head also writes the next step's
    bf16 patch rows (:func:`_patch_rows`)."""
    rows = False

    def __init__(self, model, N: int, device, den, x, x0=None, chain: bool = True):
        self.den, self.x = den, x
        self.p = model.patch_size
        self.x0 = torch.zeros_like(x) if x0 is None else x0
        self.pbuf = _patch_rows(model, N, device, den) if chain else None
        self.ident = torch.tensor([0.0, 1.0, 0.0, 1.0], device=device)

    def begin(self, x_img):
        self.first = True  # (x_img is x)

    def _head(self, mode: int, x0, coef) -> HeadStep:
        pin, self.first = (None if self.first else self.pbuf), False  # the first step patchifies x itself
        return HeadStep(mode, x0, coef, pin, self.pbuf)

    def step(self, t, mode: int, coef=None):
        self.den.step_(self.x, t, self._head(mode, None if mode == ops.HEAD_CLAMP else self.x0, coef))

    def predict_x0(self, t):
        """x0-hat into ``x0`` (:meth:`_Denoiser.x0_` with the identity row): ``x`` stays as it is."""
        self.den.x0_(self.x, t, self._head(ops.HEAD_DDIM, self.x0, self.ident))

    def cold_step(self, t, algorithm: int):
        ops.cold_step_(self.x, self.x0, t, algorithm, patches_out=self.pbuf)

    def repaint(self, known, mask, coef, rng, site_paste: int, site_jump: int):
        """Inpainting mask step (``known`` / ``mask`` as patch rows): ``x`` goes through the row
        layout around the op, as :meth:`_StepNoise.add_`'s noise does (a loop without a chain)."""
        xr = ops.image_to_rows(self.x, self.p).contiguous()
        ops.repaint_rows_(xr, known, mask, coef, rng, site_paste, site_jump)
        self.x.copy_(ops.rows_to_image(xr, *self.x.shape, self.p))

    def dpm_step(self, coef, each: bool):
        """DPM-Solver++(2M) step: ``x`` / ``x0`` / ``x0_prev`` go through the row layout around
        the op, as in :meth:`repaint` (a loop without a chain)."""
        xr, x0, x0p = (ops.image_to_rows(v, self.p).contiguous() for v in (self.x, self.x0, self.x0_prev))
        ops.dpm2m_rows_(xr, x0, x0p, coef, self.x.shape[0], each)
        self.x.copy_(ops.rows_to_image(xr, *self.x.shape, self.p))

    def image(self, xr):
        return xr

    def write_back(self, x=None, x0=None):
        pass


def _loop_state(model, N: int, device, den, x, x0=None, eta: bool = False, chain: bool = True):
    """The state a loop steps: patch rows on the GPU's fused path, else the image layout on
    the loop's buffers ``x`` / ``x0``.  ``eta``: a stochastic loop, whose step is a head mode
    of the patch-row epilogue of the LayerNorm-folded program only; on the image layout its
    noise changes ``x`` after the head wrote the bf16 rows, so there is no patch-row chain
    (``chain`` False: nor for any other loop that changes ``x`` between forwards there)."""
    rows = ROWS and PATCH_CHAIN and den.fused and torch.device(device).type == "cuda"
    if rows and (not eta or (den.P.folded and fold_width_ok(model.embed_dim))):
        return _Rows(model, N, device, den)
    return _Image(model, N, device, den, x, x0, chain=chain and not eta)


def _ddim_step(s, coef, each: bool, nz):
    """``step(i, t)`` of the DDIM family on the state ``s``: one forward with the update of
    table row ``coef[i]`` in the head epilogue (``each``: one row per sample).  ``nz`` (eta > 0,
    rows of 8): on patch rows still one forward, the noise drawn in the epilogue; on the image
    layout the deterministic step on ``{c0, c1, c2, dir}`` followed by :meth:`_StepNoise.add_`."""
    mode = ops.HEAD_DDIM_EACH if each else ops.HEAD_DDIM
    if nz is None:
        return lambda i, t: s.step(t, mode, coef[i])
    if s.rows:
        mode = ops.HEAD_ETA_EACH if each else ops.HEAD_ETA
        return lambda i, t: s.step(t, mode, coef[i], noise=nz.site(i))
    coef4 = coef[..., :4].contiguous()
    sigma = coef[..., 4]  # per step a float, or [N, 1, 1, 1]
    sigma = sigma.reshape(*sigma.shape, 1, 1, 1).contiguous() if each else [float(v) for v in sigma.tolist()]

    def step(i, t):
        s.step(t, mode, coef4[i])
        nz.add_(s.x, i, sigma[i])
    return step


def _dpm_step(s, coef, each: bool):
    """``step(i, t)`` of DPM-Solver++(2M) on the state ``s`` (after ``s.history(steps)``): one
    forward that writes the clamped x0-hat (``x`` untouched), then one :func:`ops.dpm2m_rows_`
    launch with table row ``coef[i]`` (rows of 8; ``each``: one per sample) that reads it and the
    x0-hat of the step before; the two x0 buffers trade places from step to step."""
    def step(i, t):
        if i:
            s.swap_x0()
        s.predict_x0(t)
        s.dpm_step(coef[i], each)
    return step


SOLVERS = ("ddim", "dpmpp2m")


def _check_solver(solver, eta: float):
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver == "dpmpp2m" and float(eta) > 0:
        raise ValueError("solver='dpmpp2m' is the deterministic ODE solver: eta must be 0 (no SDE variant)")


def _step_times(ts, N: int, device) -> torch.Tensor:
    """[len(ts), N] int64: row i is step i's timestep for every sample."""
    return torch.tensor(ts, dtype=torch.int64, device=device).unsqueeze(1).expand(-1, N).contiguous()


class _StepNoise:
    """Noise of the stochastic samplers: step i adds ``sigma z_i`` with ``z_i`` = ``ops.randn_``
    over the fp32 patch-row state [N*P, F] at ``rng = [seed, 0]``, site ``SITE_STEP_NOISE + i``
    (so sample b's noise does not depend on the batch size).  ``rng`` is a static device
    buffer the host writes before each run: a captured loop reads the seed from memory."""

    def __init__(self, model, N: int, device):
        p = model.patch_size
        H, W = model.img_size
        self.shape, self.p = (N, model.in_chans, H, W), p
        self.rng = torch.zeros(2, dtype=torch.int64, device=device)
        self.rows = (N * (H // p) * (W // p), model.in_chans * p * p)
        self.z = None  # the fallback's rows-shaped draw (allocated on first use)

    def site(self, i: int):
        return (self.rng, ops.SITE_STEP_NOISE + i)

    def repaint_sites(self, n: int):
        """(paste site, jump site) of an inpainting loop's forward ``n``."""
        return ops.SITE_PASTE_NOISE + n, ops.SITE_JUMP_NOISE + n

    def set_seed(self, seed: int):
        self.rng.copy_(torch.tensor([int(seed), 0], dtype=torch.int64))

    def add_(self, x, i: int, sigma):
        """Fallback (no fused epilogue): ``x += sigma z_i`` on the image-layout state; ``sigma``
        a float or [N, 1, 1, 1]."""
        if self.z is None:
            self.z = torch.empty(self.rows, device=x.device)
        ops.randn_(self.z, *self.site(i))
        x.add_(ops.rows_to_image(self.z, *self.shape, self.p) * sigma)


def draw_noise_seed(generator: Optional[torch.Generator] = None) -> int:
    """One seed for a stochastic sampling run from ``generator`` (None: the global one)."""
    dev = generator.device if generator is not None else "cpu"
    return int(torch.randint(0, 2 ** 62, (1,), generator=generator, device=dev).item())


def _unit_host(x: torch.Tensor) -> torch.Tensor:
    """(x + 1) / 2 as a host tensor -- the reference's return convention (ViT.py:236)
    -- with the affine done on the device before the copy: on the host it cost ~3 ms
    per 64-image batch (tools/ub_d2h.py; 9 % of a k=20 sampler call), on the GPU
    ~0.02 ms.  Same fp32 operations, same values."""
    if x.device.type == "cpu":
        return (x + 1) / 2
    return x.add(1.0).div_(2.0).cpu()


def _cache(model) -> dict:
    return model.__dict__.setdefault("_sampler_graphs", {})


class _LoopState:
    """One cached loop: its static buffers (``x`` in, ``x0`` / ``traj`` / ``x`` out), the
    :class:`_StepNoise` of a stochastic one, the :class:`_GraphLoop`, and ``key`` = what the
    capture depends on (:meth:`_Denoiser.key_of` when it was built)."""
    __slots__ = ("key", "x", "x0", "traj", "noise", "loop", "known", "mask")

    def __init__(self, key, x, loop, x0=None, traj=None, noise=None, known=None, mask=None):
        self.key, self.x, self.x0, self.traj, self.noise, self.loop = key, x, x0, traj, noise, loop
        self.known, self.mask = known, mask  # an inpainting loop's patch rows to keep / their uint8 mask


def _cached_loop(model, key, build, limit: Optional[int] = None) -> _LoopState:
    """The model's loop under ``key`` (a tuple; ``key[0]`` names its kind), from ``build()`` if
    there is none or the weights it captured were reallocated.  ``limit``: at most that many
    loops of the kind stay cached, least recently used evicted."""
    cache = _cache(model)
    if limit is None:
        st = cache.get(key)
    else:
        st = cache.pop(key, None)
        if st is not None:
            cache[key] = st  # most recently used last
    if st is not None and st.key == _Denoiser.key_of(model):
        return st
    if limit is not None:
        cached = [c for c in cache if isinstance(c, tuple) and c[0] == key[0] and c != key]
        for old in cached[:max(0, len(cached) - limit + 1)]:
            del cache[old]
    st = cache[key] = build()
    return st


class _GraphLoop:
    """Capture ``body()`` (a full sampling loop on static buffers) into one hipGraph.

    The first :meth:`run` executes the body eagerly on a side stream (allocator and
    kernel warm-up; its result is this call's result) and captures the graph;
    every later run is one replay.  Loops are cached per model and shape
    (:func:`_cache`), so a repeated call replays."""

    def __init__(self, body, device):
        self.body = body
        self.device = device
        self.graph = None

    def run(self, use_graph: bool):
        if not use_graph or self.device.type != "cuda":
            self.body()
            return
        if self.graph is None:
            s = torch.cuda.Stream(device=self.device)
            s.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(s):
                self.body()  # warm-up (allocator, kernels); also produces this call's result
            torch.cuda.current_stream(self.device).wait_stream(s)
            from ..utils.observe import no_gc
            # (a capture records the body without running it: the warm-up's
            # outputs stay this call's result)
            g = torch.cuda.CUDAGraph()
            with no_gc(), torch.cuda.graph(g, capture_error_mode="thread_local"):
                self.body()
            self.graph = g
            self.replays = 0
            return
        self.graph.replay()
        self.replays += 1


class DDIMSampler:
    """DDIM sampler, jump ``k``.  ``eta`` in [0, 1] selects the member of the DDIM family
    (Song et al. 2021): 0 the deterministic map from x_T (the default), 1 DDPM ancestral
    sampling; ``eta`` > 0 adds ``sigma z`` per step (:func:`schedule.ddim_coefficients_eta`;
    noise: :class:`_StepNoise`).  On the GPU's patch-row path a stochastic step is still ONE
    forward: the head epilogue draws z in registers (``ops.head_step_rows_`` mode 5).  Elsewhere
    (CPU, ``ROWS`` / ``PATCH_CHAIN`` off, the unfolded program) the
    deterministic step is followed by ``ops.randn_`` and ``x += sigma z``: the same values up
    to rounding, two more launches per step, no patch-row chain.

    The seed of a run's noise is one ``torch.randint`` from ``generator`` after x_T is drawn
    (``noise_seed=`` overrides it); with ``eta`` = 0 nothing extra is drawn.

    ``solver="dpmpp2m"``: DPM-Solver++(2M) (Lu et al. 2022) on the same timestep grid, the
    second-order multistep solver for x0-predicting models whose first-order member is DDIM
    (``schedule.dpm2m_row``).  A step is one forward that leaves the clamped x0-hat in its own
    buffer plus one :func:`ops.dpm2m_rows_` launch, which adds ``g (x0 - x0_prev)`` to the DDIM
    update and writes the next step's bf16 patch rows; it needs ``eta`` = 0.  The loops of the
    two solvers are cached under keys of different kinds."""

    def __init__(self, model, device, k: int = 10, use_graph: bool = True, eta: float = 0.0, solver: str = "ddim"):
        _check_solver(solver, eta)
        self.solver = solver
        self.model = model
        self.device = torch.device(device)
        self.k = k
        self.T = model.total_steps
        self.eta = float(eta)
        ddim_coefficients_eta(self.T, self.T - 1, k, self.eta)  # (ValueError for eta outside [0, 1])
        self.ts, coef = ddim_table(self.T, k, device=self.device)
        self.coef = coef
        self.coef8 = ddim_table_eta(self.T, k, self.eta, device=self.device)[1] if self.eta > 0 else None
        if solver == "dpmpp2m":
            self.coef8 = dpm2m_table(self.T, k, device=self.device)[1]
        self.use_graph = use_graph and self.device.type == "cuda"
        self.H, self.W = model.img_size
        self.C = model.in_chans

    def _state(self, N: int, record: bool):
        """The cached buffers + loop (the stochastic sampler: its own kind of key, eta included)."""
        key = ("ddim", N, self.k, record, str(self.device))
        if self.eta > 0:
            key = ("ddim_eta", N, self.k, record, str(self.device), self.eta)
        if self.solver == "dpmpp2m":
            key = ("ddim_dpm", N, self.k, record, str(self.device))
        return _cached_loop(self.model, key, lambda: self._build(N, record))

    def _build(self, N: int, record: bool) -> _LoopState:
        den = _Denoiser(self.model, self.device)
        dev = self.device
        x = torch.zeros(N, self.C, self.H, self.W, device=dev)
        x0 = torch.zeros_like(x)
        tt = _step_times(self.ts, N, dev)
        traj = torch.zeros(len(self.ts), N, self.C, self.H, self.W, device=dev) if record else None
        nz = _StepNoise(self.model, N, dev) if self.eta > 0 else None
        dpm = self.solver == "dpmpp2m"
        s = _loop_state(self.model, N, dev, den, x, x0, eta=nz is not None, chain=not dpm)
        if dpm:
            step = _dpm_step(s, self.coef8, False)
        else:
            step = _ddim_step(s, self.coef if nz is None else self.coef8, False, nz)

        def loop():
            s.begin(x)
            if dpm:
                s.history(len(self.ts))
            for i in range(len(self.ts)):
                step(i, tt[i])  # forward + clamp + DDIM update, one head epilogue (2M: + one launch)
                if traj is not None:
                    traj[i].copy_(s.image(s.x0))
            s.write_back(x0=x0)  # (x_t itself is not returned)

        return _LoopState(den.key(), x, _GraphLoop(loop, dev), x0, traj, nz)

    def _seed(self, st, generator, noise_seed):
        if self.eta > 0:
            st.noise.set_seed(draw_noise_seed(generator) if noise_seed is None else noise_seed)

    @torch.no_grad()
    def sample(self, N: int, generator: Optional[torch.Generator] = None, verbose: bool = False,
               noise: Optional[torch.Tensor] = None, device_noise: bool = False,
               noise_seed: Optional[int] = None) -> torch.Tensor:
        """``device_noise``: draw x_T on the GPU (``generator`` then a device generator)
        instead of on the host as the reference does (ViT.py:224-225) -- same
        distribution, a different stream; saves the host draw + copy (~2.5 ms per
        N=64 batch)."""
        st = self._state(N, False)
        t0 = time.time()
        if noise is not None:
            st.x.copy_(noise)
        elif device_noise:
            st.x.normal_(0.0, 1.0, generator=generator)
        else:
            st.x.copy_(torch.normal(0.0, 1.0, (N, self.C, self.H, self.W), generator=generator))
        self._seed(st, generator, noise_seed)
        st.loop.run(self.use_graph)
        out = _unit_host(st.x0)
        if verbose:
            print(f"ddim k={self.k} N={N}: {len(self.ts)} steps in {time.time() - t0:.3f}s")
        return out

    @torch.no_grad()
    def sequence(self, N: int, generator: Optional[torch.Generator] = None,
                 noise: Optional[torch.Tensor] = None, noise_seed: Optional[int] = None) -> List[torch.Tensor]:
        st = self._state(N, True)
        if noise is None:
            noise = torch.normal(0.0, 1.0, (N, self.C, self.H, self.W), generator=generator)
        st.x.copy_(noise)
        self._seed(st, generator, noise_seed)
        first = _unit_host(noise)
        st.loop.run(self.use_graph)
        traj = _unit_host(st.traj)
        return [first] + [traj[i] for i in range(traj.shape[0])]


COLD_RESTORE_GRAPHS = 8  # cached restoration loops (graph + buffers) per model


class ColdSampler:
    """Cold de-pixelation sampler, t = S..1, from constant-colour images (:meth:`sample`,
    :meth:`sequence`) or from pixelated versions of given images (:meth:`restore`).

    ``predict="prev"`` (a ``dataset: cold`` model, which predicts x_{t-1}): ``x <-
    clamp(f(x, t))``, the reference's rule (`ViT_draft2drawing.py:259-288`).
    ``predict="x0"`` (a ``dataset: cold_x0`` model, which predicts the clean image): with
    x0-hat = clamp(f(x_t, t)) and D the training degradation, ``algorithm`` 1 is
    ``x_{t-1} = D(x0-hat, t-1)`` and ``algorithm`` 2 ``x_{t-1} = x_t - D(x0-hat, t) +
    D(x0-hat, t-1)`` (Bansal et al. 2022, Algorithms 1 and 2); each step is one forward
    that leaves x0-hat in its own buffer plus one :func:`ops.cold_step_` launch, which also
    writes the next step's bf16 patch rows.  The whole loop is one cached hipGraph."""

    def __init__(self, model, device, use_graph: bool = True, steps: Optional[int] = None, predict: str = "prev",
                 algorithm: int = 2):
        if predict not in ("prev", "x0"):
            raise ValueError(f"predict must be 'prev' or 'x0', got {predict!r}")
        if algorithm not in (1, 2):
            raise ValueError(f"algorithm must be 1 or 2, got {algorithm!r}")
        self.model = model
        self.device = torch.device(device)
        self.steps = steps or cold_steps(model.img_size[1])
        self.use_graph = use_graph and self.device.type == "cuda"
        self.H, self.W = model.img_size
        self.C = model.in_chans
        self.predict = predict
        self.algorithm = algorithm

    def _state(self, N: int):
        key = ("cold", N, self.steps, str(self.device))
        if self.predict == "x0":
            key += ("x0", self.algorithm)
        return _cached_loop(self.model, key, lambda: self._build(N, [[t] * N for t in range(self.steps, 0, -1)]))

    def _build(self, N: int, levels) -> _LoopState:
        """Buffers + loop for the step grid ``levels`` ([steps][N], descending): row i holds
        the model's t of step i, or 0 for a sample that has not joined the grid yet (x0
        prediction only: the step kernel skips it)."""
        den = _Denoiser(self.model, self.device)
        dev = self.device
        x = torch.zeros(N, self.C, self.H, self.W, device=dev)
        ts = [max(row) for row in levels]
        tt = _step_times(ts, N, dev)
        traj = torch.zeros(len(ts), N, self.C, self.H, self.W, device=dev)
        s = _loop_state(self.model, N, dev, den, x)
        if self.predict == "x0":
            loop = self._x0_loop(s, x, tt, torch.tensor(levels, dtype=torch.int64, device=dev), traj)
        else:
            loop = self._prev_loop(s, x, tt, traj)
        return _LoopState(den.key(), x, loop, traj=traj)

    def _prev_loop(self, s, x, tt, traj) -> _GraphLoop:
        def loop():
            s.begin(x)
            for i in range(tt.shape[0]):
                s.step(tt[i], ops.HEAD_CLAMP)  # forward + clamp in the head epilogue
                traj[i].copy_(s.image(s.x))
            s.write_back(x=x)

        return _GraphLoop(loop, self.device)

    def _x0_loop(self, s, x, tt, tk, traj) -> _GraphLoop:
        """The x0-prediction loop: per step one forward (x0-hat into its own buffer, x
        untouched) and one cold-step launch with the per-sample levels ``tk[i]``; the
        recorded states and the final ``x`` are clamped to [-1, 1]."""
        alg = self.algorithm

        def loop():
            s.begin(x)
            for i in range(tt.shape[0]):
                s.predict_x0(tt[i])
                s.cold_step(tk[i], alg)
                torch.clamp(s.image(s.x), -1.0, 1.0, out=traj[i])
            torch.clamp(s.image(s.x), -1.0, 1.0, out=x)

        return _GraphLoop(loop, self.device)

    def _init(self, N, generator):
        c = torch.normal(0.0, 1.0, (N, self.C), generator=generator)
        return c[:, :, None, None].expand(-1, -1, self.H, self.W).contiguous()

    @torch.no_grad()
    def sample(self, N: int, generator=None) -> torch.Tensor:
        st = self._state(N)
        st.x.copy_(self._init(N, generator))
        st.loop.run(self.use_graph)
        return _unit_host(st.x)

    @torch.no_grad()
    def sequence(self, N: int, generator=None) -> List[torch.Tensor]:
        st = self._state(N)
        init = self._init(N, generator)
        st.x.copy_(init)
        st.loop.run(self.use_graph)
        traj = _unit_host(st.traj)
        return [(init + 1) / 2] + [traj[i] for i in range(traj.shape[0])]

    @torch.no_grad()
    def restore(self, images: torch.Tensor, level, sequence: bool = False, unit: bool = True):
        """Restore images from their pixelated versions: sample b starts from
        ``pixelate(images[b], 2**level[b])`` and joins the shared step grid ``t =
        max(level)..1`` at its own level (the cold counterpart of :func:`img2img`).

        ``images`` [B,C,H,W] in [-1, 1]; ``level`` an int or one int per image, each in
        ``0..cold_steps(W)``.  With ``predict="x0"`` a sample whose level is below step t is
        skipped by the step kernel and stays exactly as it is (level 0: the clamped input
        comes back); ``predict="prev"`` has no per-sample skip, so unequal levels raise
        ``ValueError``.  The loop is one hipGraph cached per (B, levels, predict, algorithm),
        at most ``COLD_RESTORE_GRAPHS`` per model, least recently used evicted.

        Returns host images in [0, 1] (``unit=False``: in [-1, 1]); with ``sequence`` the
        list [start, state after each step] instead, whose last entry is the result."""
        from ..ops import reference as ref
        if images.dim() == 3:
            images = images.unsqueeze(0)
        B = images.shape[0]
        if tuple(images.shape[1:]) != (self.C, self.H, self.W):
            raise ValueError(f"images must be [B, {self.C}, {self.H}, {self.W}], got {tuple(images.shape)}")
        levels = [int(level)] * B if isinstance(level, int) else [int(v) for v in level]
        top_ok = cold_steps(self.W)
        if len(levels) != B or any(v < 0 or v > top_ok for v in levels):
            raise ValueError(f"level: one int per image in 0..{top_ok}, got {level!r}")
        if self.predict == "prev" and len(set(levels)) > 1:
            raise ValueError("predict='prev' has no per-sample skip: all levels of one call must be equal")
        images = images.detach().float().cpu()
        start = torch.cat([ref.pixelate(images[b:b + 1], 2 ** v) for b, v in enumerate(levels)])
        to_host = _unit_host if unit else (lambda v: v.cpu().clone())
        top = max(levels)
        if top == 0:  # nothing to step through
            out = torch.clamp(start, -1.0, 1.0)
            return [to_host(out)] if sequence else to_host(out)
        key = ("cold_restore", B, tuple(levels), self.predict, self.algorithm, str(self.device))
        st = _cached_loop(self.model, key, lambda: self._build(
            B, [[t if v >= t else 0 for v in levels] for t in range(top, 0, -1)]), COLD_RESTORE_GRAPHS)
        st.x.copy_(start)
        st.loop.run(self.use_graph)
        if not sequence:
            return to_host(st.x)
        traj = to_host(st.traj)
        return [to_host(start)] + [traj[i] for i in range(traj.shape[0])]


IMG2IMG_GRAPHS = 8  # cached img2img loops (graph + buffers) per model


def starts_table(total_steps: int, starts: Sequence[int], k: int):
    """(descending grid ts, [len(ts), B, 4] per-sample DDIM coefficients) for samples
    joining one k-grid at their own start steps; a sample whose start is below
    step t has the identity row {0, 1, 0, 1} there (x_next = x_t exactly)."""
    top = max(starts)
    if any((top - s) % k for s in starts):
        raise ValueError("all start steps must share one k-grid")
    ts = list(range(top, 0, -k))
    if ts[-1] + 1 - k < 0:
        raise ValueError(f"k={k} incompatible with t_start={top}")
    ident = (0.0, 1.0, 0.0, 1.0)
    rows = [[ddim_coefficients(total_steps, t, k) if s >= t else ident for s in starts] for t in ts]
    return ts, torch.tensor(rows, dtype=torch.float32)


def starts_table_eta(total_steps: int, starts: Sequence[int], k: int, eta: float):
    """:func:`starts_table` for the DDIM family: rows of 8 floats ``{c0, c1, c2, dir, sigma,
    0, 0, 0}`` ([len(ts), B, 8]); a sample that has not started has ``{0, 1, 0, 1, 0, 0, 0, 0}``
    (x_next = x_t, no noise)."""
    ts, _ = starts_table(total_steps, starts, k)
    rows = [[eta_row(total_steps, t, k, eta) if s >= t else ETA_IDENT_ROW for s in starts] for t in ts]
    return ts, torch.tensor(rows, dtype=torch.float32)


def starts_table_dpm(total_steps: int, starts: Sequence[int], k: int):
    """:func:`starts_table` for DPM-Solver++(2M): rows ``{c0, c1, c2, c3, g, 0, 0, 0}``
    (``schedule.dpm2m_row``; [len(ts), B, 8]).  A sample that has not started has
    ``ETA_IDENT_ROW``; the step at which it starts has no history, so g = 0 there (DDIM), and
    every later one takes the ``h`` of the sample's step before."""
    ts, _ = starts_table(total_steps, starts, k)

    def row(s, t):
        if s < t:
            return ETA_IDENT_ROW
        return dpm2m_row(total_steps, t, k, None if s == t else dpm2m_step_h(total_steps, t + k, k))

    return ts, torch.tensor([[row(s, t) for s in starts] for t in ts], dtype=torch.float32)


def _from_starts_state(model, B: int, starts, k: int, device, eta: float, solver: str = "ddim") -> _LoopState:
    """Buffers + loop of :func:`ddim_from_starts`."""
    den = _Denoiser(model, device)
    T = model.total_steps
    dpm = solver == "dpmpp2m"
    if dpm:
        ts, coef = starts_table_dpm(T, starts, k)
    else:
        ts, coef = starts_table_eta(T, starts, k, eta) if eta > 0 else starts_table(T, starts, k)
    coef = coef.to(device)
    xs = torch.zeros(B, model.in_chans, *model.img_size, device=device)
    x0 = torch.zeros_like(xs)
    tt = _step_times(ts, B, device)
    nz = _StepNoise(model, B, device) if eta > 0 else None
    s = _loop_state(model, B, device, den, xs, x0, eta=nz is not None, chain=not dpm)
    step = _dpm_step(s, coef, True) if dpm else _ddim_step(s, coef, True, nz)

    def loop():
        s.begin(xs)
        if dpm:
            s.history(len(ts))
        for i in range(len(ts)):
            step(i, tt[i])
        s.write_back(x=xs, x0=x0)

    return _LoopState(den.key(), xs, _GraphLoop(loop, device), x0, noise=nz)


@torch.no_grad()
def ddim_from_starts(model, x: torch.Tensor, starts: Sequence[int], k: int, device=None,
                     use_graph: bool = True, eta: float = 0.0, noise_seed: Optional[int] = None,
                     solver: str = "ddim") -> torch.Tensor:
    """DDIM (jump ``k``) from per-sample start steps, all samples in ONE batch.

    Sample i joins the shared descending grid at its own ``starts[i]``; all starts
    must lie on one k-grid (``(max - s) % k == 0``).  Every step is ONE forward
    whose head epilogue applies the update with per-sample coefficients
    (:func:`ops.head_step_` mode 4: not-yet-started samples get the identity row),
    and the whole loop is one hipGraph, cached per (B, starts, k): a repeated
    call is one replay (at most ``IMG2IMG_GRAPHS`` such loops stay cached per model,
    least recently used evicted).  Returns the final clamped x0-hat on the device,
    in [-1, 1], as a fresh tensor (not the graph's output buffer, which the next call
    with the same key overwrites).

    ``eta`` > 0: the stochastic member of the DDIM family (see :class:`DDIMSampler`), head
    mode 6 (per-sample rows of 8 coefficients, the noise drawn in the epilogue); a sample
    that has not started is left exactly as it is.  ``noise_seed``: the run's noise seed
    (None: one draw from the global generator).

    ``solver="dpmpp2m"`` (``eta`` = 0 only): DPM-Solver++(2M) steps as in :class:`DDIMSampler`,
    with per-sample rows (:func:`starts_table_dpm`): one forward plus one
    :func:`ops.dpm2m_rows_` launch per step; the step at which a sample joins is first-order.
    Its loops are cached under their own kind of key, held to ``IMG2IMG_GRAPHS`` as well.
    """
    _check_solver(solver, eta)
    device = torch.device(device) if device is not None else x.device
    T = model.total_steps
    B = x.shape[0]
    starts = [int(s) for s in starts]
    eta = float(eta)
    ddim_coefficients_eta(T, max(starts), k, eta)  # (ValueError for eta outside [0, 1])
    key = ("img2img", B, tuple(starts), k, str(device))
    if eta > 0:
        key = ("img2img_eta", B, tuple(starts), k, str(device), eta)
    if solver == "dpmpp2m":
        key = ("img2img_dpm", B, tuple(starts), k, str(device))
    st = _cached_loop(model, key, lambda: _from_starts_state(model, B, starts, k, device, eta, solver),
                      IMG2IMG_GRAPHS)
    st.x.copy_(x.to(device).float())
    if st.noise is not None:
        st.noise.set_seed(draw_noise_seed() if noise_seed is None else noise_seed)
    st.loop.run(use_graph and device.type == "cuda")
    return st.x0.clone()


@torch.no_grad()
def img2img(model, draft: torch.Tensor, t_starts: Sequence[int] = tuple(range(1599, 2000, 50)), k: int = 10,
            device=None, generator: Optional[torch.Generator] = None, use_graph: bool = True,
            eta: float = 0.0, solver: str = "ddim") -> torch.Tensor:
    """Zero-shot draft->drawing (SDEdit-style) for several noise levels at once.

    For each t_start: x = sqrt(1-a) eps + sqrt(a) draft, a = 1 - sqrt(t_start/T)
    (ViT_draft2drawing.py:395-396, note t_start/T not (t+1)/T), then DDIM with
    jump k down to the grid's last step; returns the final x0-hat per t_start
    as CPU images in [0, 1], shape [len(t_starts), C, H, W].

    All t_starts on one k-grid run as ONE batch, each sample joining the shared
    step grid at its own start (the reference loops them one at a time at batch
    1); the loop is one cached hipGraph (:func:`ddim_from_starts`).  ``eta`` > 0: stochastic
    DDIM steps (what SDEdit uses), their noise seed one more draw from ``generator``.
    ``solver="dpmpp2m"``: DPM-Solver++(2M) steps instead (``eta`` = 0 only; :func:`ddim_from_starts`).
    """
    _check_solver(solver, eta)
    device = torch.device(device) if device is not None else next(model.parameters()).device
    T = model.total_steps
    starts = list(t_starts)
    B = len(starts)
    C, H, W = model.in_chans, *model.img_size
    if draft.dim() == 3:
        draft = draft.unsqueeze(0)
    draft = draft.to(device).float()
    if draft.shape[0] == 1:
        draft = draft.expand(B, -1, -1, -1)
    top = max(starts)
    if any((top - s) % k for s in starts):
        # different grids: run them one by one
        return torch.cat([img2img(model, draft[i:i + 1], [s], k, device, generator, use_graph, eta, solver)
                          for i, s in enumerate(starts)])
    eps = torch.normal(0.0, 1.0, (B, C, H, W), generator=generator).to(device)
    x = img2img_noised(draft, eps, starts, T)
    seed = draw_noise_seed(generator) if float(eta) > 0 else None
    x0 = ddim_from_starts(model, x, starts, k, device, use_graph, eta, seed, solver)
    return _unit_host(x0)


def img2img_noised(draft: torch.Tensor, eps: torch.Tensor, starts: Sequence[int], total_steps: int) -> torch.Tensor:
    """x = sqrt(1-a) eps + sqrt(a) draft per start step, a = 1 - sqrt(t_start/T)
    (ViT_draft2drawing.py:395-396)."""
    alpha = torch.tensor([img2img_alpha(s, total_steps) for s in starts], device=draft.device).view(-1, 1, 1, 1)
    return torch.sqrt(1 - alpha) * eps + torch.sqrt(alpha) * draft


INPAINT_GRAPHS = 8  # cached inpainting loops (graph + buffers) per model


def _inpaint_mask(mask, B: int, C: int, H: int, W: int) -> torch.Tensor:
    """``mask`` (bool, or numeric binarised at > 0.5; 1 = keep) as a host bool [B, C, H, W]."""
    mask = torch.as_tensor(mask).detach().cpu()
    keep = mask if mask.dtype == torch.bool else mask.float() > 0.5
    if tuple(keep.shape) == (H, W):
        keep = keep.view(1, 1, H, W)
    elif tuple(keep.shape) not in ((B, 1, H, W), (B, C, H, W)):
        raise ValueError(f"mask must be [{H}, {W}], [{B}, 1, {H}, {W}] or [{B}, {C}, {H}, {W}], "
                         f"got {tuple(mask.shape)}")
    return keep.expand(B, C, H, W)


def _inpaint_state(model, B: int, k: int, eta: float, resample: int, device) -> _LoopState:
    """Buffers + loop of :func:`inpaint`: forward n is one head step with row ``n // resample``
    of the DDIM table (noise site ``n`` at eta > 0) and one mask step with row n of
    :func:`schedule.repaint_table`."""
    T = model.total_steps
    ts, rp = repaint_table(T, k, resample, device=device)
    if len(ts) >= ops.SITE_LOOP_FORWARDS:
        raise ValueError(f"inpaint: {len(ts)} forwards (k={k}, resample={resample}); a loop has noise sites for "
                         f"fewer than {ops.SITE_LOOP_FORWARDS}")
    den = _Denoiser(model, device)
    coef = ddim_table_eta(T, k, eta, device=device)[1] if eta > 0 else ddim_table(T, k, device=device)[1]
    coef = coef.repeat_interleave(resample, 0).contiguous()  # one row per forward
    x = torch.zeros(B, model.in_chans, *model.img_size, device=device)
    tt = _step_times(ts, B, device)
    nz = _StepNoise(model, B, device)  # (the paste draws noise at every eta)
    known = torch.zeros(nz.rows, device=device)
    mask = torch.zeros(nz.rows, dtype=torch.uint8, device=device)
    s = _loop_state(model, B, device, den, x, eta=eta > 0, chain=False)
    step = _ddim_step(s, coef, False, nz if eta > 0 else None)

    def loop():
        s.begin(x)
        for n in range(len(ts)):
            step(n, tt[n])  # the DDIM jump t -> t-k in the head epilogue
            s.repaint(known, mask, rp[n], nz.rng, *nz.repaint_sites(n))  # paste (+ jump back to t)
        s.write_back(x=x)

    return _LoopState(den.key(), x, _GraphLoop(loop, device), noise=nz, known=known, mask=mask)


@torch.no_grad()
def inpaint(model, image: torch.Tensor, mask, k: int = 10, eta: float = 0.0, resample: int = 1, device=None,
            generator: Optional[torch.Generator] = None, use_graph: bool = True,
            noise: Optional[torch.Tensor] = None, noise_seed: Optional[int] = None, unit: bool = True) -> torch.Tensor:
    """Mask-conditioned DDIM sampling: keep ``image`` where ``mask`` is 1, generate the rest
    (RePaint, Lugmayr et al. 2022; no retraining of an x0-predicting model).

    From x_T, every step t of the ``ddim_timesteps(T, k)`` grid is one forward with the usual
    head step (``eta`` as in :class:`DDIMSampler`) followed by one :func:`ops.repaint_rows_`
    launch, which replaces the kept elements by the image noised to the level t-k the step
    landed on.  ``resample`` > 1 (an int >= 1) runs each grid step that many times, the mask
    step diffusing the state forward to level t again after every run but the last, which lets
    the generated region harmonise with the kept one.

    ``image`` [B,C,H,W] or [C,H,W] in [-1, 1]; ``mask`` bool or numeric (binarised at > 0.5),
    [H,W], [B,1,H,W] or [B,C,H,W].  x_T is ``noise`` or one ``torch.normal`` draw from
    ``generator``; the seed of the paste / jump / step noise one :func:`draw_noise_seed` after
    it (``noise_seed=`` overrides it).  The loop is one hipGraph cached per (B, k, eta,
    resample), at most ``INPAINT_GRAPHS`` per model; image, mask, x_T and the seed are static
    buffers, so a new one of any of them is a replay.

    The steps are first-order DDIM only: the paste rewrites ``x`` between forwards, which breaks
    the x0-hat history a multistep solver (``DDIMSampler(solver="dpmpp2m")``) extrapolates from.

    Returns the final state -- at the last step x0-hat in the free region and ``image`` exactly
    in the kept one -- as host images in [0, 1] (``unit=False``: in [-1, 1])."""
    device = torch.device(device) if device is not None else next(model.parameters()).device
    T = model.total_steps
    C, (H, W), p = model.in_chans, model.img_size, model.patch_size
    if image.dim() == 3:
        image = image.unsqueeze(0)
    if image.dim() != 4 or tuple(image.shape[1:]) != (C, H, W):
        raise ValueError(f"image must be [B, {C}, {H}, {W}] or [{C}, {H}, {W}], got {tuple(image.shape)}")
    B = image.shape[0]
    if isinstance(resample, bool) or not isinstance(resample, int) or resample < 1:
        raise ValueError(f"resample must be an int >= 1, got {resample!r}")
    eta = float(eta)
    ddim_coefficients_eta(T, T - 1, k, eta)  # (ValueError for eta outside [0, 1])
    keep = _inpaint_mask(mask, B, C, H, W)
    key = ("inpaint", B, k, eta, resample, str(device))
    st = _cached_loop(model, key, lambda: _inpaint_state(model, B, k, eta, resample, device), INPAINT_GRAPHS)
    st.known.copy_(ops.image_to_rows(image.detach().float().cpu(), p))
    st.mask.copy_(ops.image_to_rows(keep.to(torch.uint8), p))
    if noise is not None:
        st.x.copy_(noise)
    else:
        st.x.copy_(torch.normal(0.0, 1.0, (B, C, H, W), generator=generator))
    st.noise.set_seed(draw_noise_seed(generator) if noise_seed is None else noise_seed)
    st.loop.run(use_graph and device.type == "cuda")
    return _unit_host(st.x) if unit else st.x.cpu().clone()
