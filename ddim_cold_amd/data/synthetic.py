"""Synthetic, Oxford-Flowers-shaped image pools generated on the device.

There is no network access for datasets, so benchmarks and smoke tests use a
deterministic pool of smooth random RGB images in [-1, 1] (low-frequency
fields: a coarse random grid bilinearly upsampled plus a few radial "petal"
patterns), resident in HBM.  Training batches are then drawn *on device*
inside the captured step (pool index + cold timestep t from the counter RNG,
pixelation of (x_t, x_{t-1}) in one kernel: ``ops.cold_batch``), replacing the
reference's CPU DataLoader workers (multi_gpu_trainer.py:63-64,
diffusion_loader.py:84-97).
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from .. import ops

SITE_DATA = 3
SITE_NOISE = 4


def synthetic_pool(n: int, size=(64, 64), channels: int = 3, seed: int = 0, device="cpu") -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    H, W = size
    coarse = torch.rand(n, channels, 6, 6, generator=g) * 2 - 1
    img = F.interpolate(coarse, size=(H, W), mode="bicubic", align_corners=False)
    yy, xx = torch.meshgrid(torch.linspace(-1, 1, H), torch.linspace(-1, 1, W), indexing="ij")
    r = torch.sqrt(xx ** 2 + yy ** 2)
    th = torch.atan2(yy, xx)
    petals = torch.randint(3, 9, (n, 1, 1, 1), generator=g).float()
    phase = torch.rand(n, 1, 1, 1, generator=g) * 2 * math.pi
    radius = 0.4 + 0.4 * torch.rand(n, 1, 1, 1, generator=g)
    flower = torch.sigmoid(12 * (radius * (0.6 + 0.4 * torch.cos(petals * th + phase)) - r))
    color = torch.rand(n, channels, 1, 1, generator=g) * 2 - 1
    img = 0.5 * img + flower * color
    return img.clamp(-1, 1).contiguous().to(device)


class _Batcher:
    """Device-side batch source (graph-capturable): static buffers (x_t, target, t; a subclass
    allocates and names the target) and the :class:`ops.BatchSource` (:meth:`source`) that
    says how a batch is drawn into them.

    Each call draws t (and, unless ``idx`` is given, B pool indices) from the engine's RNG
    state and writes the buffers.  With ``idx`` (a static device int64[B] the host fills
    each step from a shard table) the batch follows DistributedSampler order; with
    ``idx_step = (ctr, off)`` as well, ``idx`` is the whole epoch table and the batch reads
    its row ``ctr[0] % rows`` (:func:`ops.stepped_idx`) -- no host copy.
    """

    def __init__(self, pool: torch.Tensor, batch: int, rng: torch.Tensor, idx: torch.Tensor | None, idx_step):
        self.pool = pool
        B, (C, H, W) = batch, pool.shape[1:]
        dev = pool.device
        self.x_t = torch.empty(B, C, H, W, device=dev)
        self.t = torch.empty(B, dtype=torch.int64, device=dev)
        self.draw = idx is None
        self.idx = torch.empty(B, dtype=torch.int64, device=dev) if idx is None else idx
        self.rng = rng
        self.idx_step = idx_step

    def source(self) -> ops.BatchSource:
        raise NotImplementedError

    def fused_spec(self):
        """Deferred form for a consumer that fuses the draw into its patch embedding
        (:func:`ops.patch_embed_cold_fwd`): ``((x_t, target, t), source())`` without launching
        anything; x_t is not materialised (the patch rows come straight from the pool)."""
        src = self.source()
        return (self.x_t, src.target, self.t), src

    def __call__(self):
        src = self.source()
        ops.batch_draw(src, self.rng, self.x_t, self.t)
        return self.x_t, src.target, self.t


class ColdBatcher(_Batcher):
    """Cold-diffusion batches: t ~ U{1..max_t}, x_t the pool image pixelated by 2^t, target =
    x_{t-1} (``ColdDownSampleDataset``) or x0 (``target='x0'``, ``ColdDownSampleDataset_au``)."""

    def __init__(self, pool: torch.Tensor, batch: int, rng: torch.Tensor, max_t: int | None = None,
                 target: str = "prev", idx: torch.Tensor | None = None, idx_step=None):
        super().__init__(pool, batch, rng, idx, idx_step)
        self.max_t = max_t or int(math.log2(pool.shape[3]))
        self.x_tm1 = torch.empty_like(self.x_t)
        self.target = target

    def source(self):
        return ops.BatchSource.cold(self.pool, SITE_DATA, self.max_t, self.x_tm1, self.idx, draw_idx=self.draw,
                                    target_x0=self.target == "x0", idx_step=self.idx_step)


class GaussianBatcher(_Batcher):
    """Gaussian DDIM batches: (q_sample(x0, t, eps), x0, t), t ~ U{0..T-1} (``DiffusionDataset``,
    diffusion_loader.py:24-58).  One launch (:func:`ops.gauss_batch`: pool draw + noise +
    q_sample), or none at all when the engine fuses the draw into its patch-embedding launch
    (:meth:`fused_spec`, same values)."""

    def __init__(self, pool: torch.Tensor, batch: int, rng: torch.Tensor, total_steps: int = 2000,
                 idx: torch.Tensor | None = None, idx_step=None):
        super().__init__(pool, batch, rng, idx, idx_step)
        self.T = total_steps
        self.x0 = torch.empty_like(self.x_t)
        self.B = batch

    def source(self):
        return ops.BatchSource.gaussian(self.pool, SITE_DATA, SITE_NOISE, self.T, self.x0, self.idx,
                                        draw_idx=self.draw, idx_step=self.idx_step)


def make_batcher(kind: str, pool: torch.Tensor, batch: int, rng: torch.Tensor, total_steps: int = 2000,
                 idx: torch.Tensor | None = None, idx_step=None):
    """Batch source for a dataset kind: 'cold' | 'cold_x0' | 'gaussian' (config key ``dataset``)."""
    if kind == "cold":
        return ColdBatcher(pool, batch, rng, idx=idx, idx_step=idx_step)
    if kind == "cold_x0":
        return ColdBatcher(pool, batch, rng, target="x0", idx=idx, idx_step=idx_step)
    if kind == "gaussian":
        return GaussianBatcher(pool, batch, rng, total_steps, idx=idx, idx_step=idx_step)
    raise ValueError(kind)
