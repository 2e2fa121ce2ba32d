"""TrainEngine — the MI355X training step runtime.

One training step of the reference (multi_gpu_trainer.py:115-134:
autocast forward, smooth-L1, backward with DDP all-reduce, unscale, clip 1.0,
AdamW step, cosine LR step, zero_grad) re-designed for a latency-bound
7 M-parameter model on MI355X:

* **Flat arenas.**  All parameters live in one fp32 arena (``nn.Parameter.data``
  are views), gradients in a second (``param.grad`` are views), Adam moments
  in two more, plus a bf16 shadow of the parameters that the MFMA GEMMs read.
  Every param offset is 256-B aligned.  All-reduce buckets are contiguous arena
  ranges: no pack/unpack kernels.
* **Fused optimizer.**  One launch: AdamW + clip + cosine LR + bf16 shadow refresh +
  grad zeroing.  The grad-norm partials come from the weight-gradient launch's
  epilogues (data parallel: one pass over the reduced arena); the loss EMA and the
  counter bump ride in the LayerNorm-fold launch that follows.  The LR / Adam
  step / RNG step live in device memory so the step is graph-replayable.
* **Deferred weight gradients.**  Single process: every weight-gradient GEMM
  of the step is ONE launch after the backward (``ops.linear_wgrad_multi``,
  1,548 64x64 tiles, no token split, no atomics).  Data parallel: one such launch
  per gradient bucket, so each bucket's all-reduce can start while the remaining
  blocks run backward.  (On a side stream they measured slower: 28.2k vs 33.1k img/s.)
* **hipGraphs per step, bucketed RCCL all-reduce.**  Single process: the step is
  ONE graph.  Data parallel: gradient buckets are contiguous arena ranges closed
  at transformer-block boundaries of the backward; as soon as a bucket's
  gradients are final its ``all_reduce`` (RCCL over xGMI) runs on a communication
  stream, overlapping the backward of the remaining blocks, and the optimizer
  waits on that stream.  Default (``comm_events``), the event-split step: forward
  + backward is one linear graph that bumps a per-bucket counter at every bucket
  boundary (a 1-lane kernel node), the optimizer a second; the host issues each
  bucket's collective on the comm stream behind a bounded polling kernel for its
  counter, queued ahead of the compute replay.  Alternatives: collectives
  captured into the one step graph (``graph_comm``; a comm branch costs ~30 us
  per fork on MI355X) or ``n_buckets + 1`` graph segments with host-issued
  collectives in between.  ``autotune_comm()`` picks the bucket layout (or one
  inline all-reduce) by measuring on the job's own ranks.  Buckets default to
  ~2 blocks (~7 MB fp32 for ViT-tiny): few enough collectives for the per-call
  latency of 7-link point-to-point xGMI rings, large enough to overlap.  Inactive
  time-embedding rows are not reduced.
"""
from __future__ import annotations

import contextlib
import math
import copy
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import torch
import torch.distributed as dist

from .. import ops
from ..models import program as _program
from ..models.program import BackwardPlan, LnFold, ModelTensors, ViTProgram, collect, is_matrix_param
from .layout import ArenaLayout, BucketLayout, arena_layout, bucket_layout

# Step graphs are captured in thread-local mode: other threads' HIP calls during a
# capture (ProcessGroupNCCL's watchdog polling the events of eager collectives)
# neither invalidate the capture nor fail in that thread.  In the default global
# mode a watchdog poll inside the capture window was seen on MI355X to invalidate
# the capture (fallback to segments) and abort the process from the watchdog.
CAPTURE_MODE = "thread_local"
# how a captured step replays (TrainEngine._capture): ONE graph (single process, or
# the collectives captured in it; K-step graphs too), the event-split pair, or one
# graph segment per gradient bucket; the last two with host-issued collectives
SINGLE, EVENT_SPLIT, SEGMENTS = "single", "event-split", "segments"
# event-split data parallel with counter hand-offs: queue the comm stream's work
# ahead of the compute-graph replay (DDIM_COLD_PREISSUE=0: behind it)
PREISSUE = os.environ.get("DDIM_COLD_PREISSUE", "1") != "0"
# the LayerNorm dgamma/dbeta replica finalize rides in the embedding-backward launch
# (False: a separate replica_reduce_ launch; tests compare the two)
FUSE_LN_FINAL = True
# single process: the grad-norm partials come from the weight-gradient launch's
# epilogues (ops.linear_wgrad_multi sq=) instead of a separate sqnorm pass over the
# arena (False: the sqnorm kernel; tests compare the two)
FUSE_SQNORM = True
# with FUSE_SQNORM: no embedding-backward launch -- the last LayerNorm backward writes
# the patch-row gradient, and the cls / pos / time-embedding gradients and the
# LayerNorm finalize run as extra workgroups of the weight-gradient launch
# (csrc/embed_parts.h; False: embed_bwd as its own launch; tests compare the two)
FUSE_EMBED_WGRAD = True
# one micro-batch with the LayerNorm finalize in the embedding launch: everything above
# ``acc_hi`` in the gradient arena (LayerNorms, blocks, head) is written by exactly one
# producer per step, which then stores instead of adding -- the optimizer zeroes only the
# embeddings and the deferred launches read no gradients; the all-reduce sums the fresh
# values in place (False: accumulate + zero everything; tests compare the two)
GRAD_OVERWRITE = True
# models of at least this many tokens per sample (vit_small_200: 626) keep transposed bf16
# shadows of the QKV / proj / fc1 / fc2 weights, re-transposed after every optimizer step, so
# their input-gradient GEMMs run on the k-contiguous operand path
# (tools/ub_dgrad_layout.py: QKV 31.7 -> 25.5 us, K = 384 15.0 -> 13.5 us at M = 20,032;
# ViT-tiny's M = 2,080 gains ~0.5 us per GEMM, less than the transpose launch costs)
TRANSPOSED_DGRAD_MIN_TOKENS = 512


class TransposedShadows:
    """Transposed copies ([in][out], bf16) of the blocks' QKV, proj, fc1 and fc2 weight
    shadows in one arena; :meth:`refresh` re-transposes all of them in one launch (after
    every optimizer step, inside the step graph), :meth:`attach` sets ``qkv_wt`` /
    ``proj_wt`` / ``fc1_wt`` / ``fc2_wt`` on the program's block tensors (fc2: the
    input gradient through GELU)."""

    KINDS = ("qkv", "proj", "fc1", "fc2")

    def __init__(self, P: ModelTensors):
        self.src = []
        for bp in P.blocks:
            self.src += [getattr(bp, k + "_w") for k in self.KINDS]
        n = sum(w.numel() for w in self.src)
        self.arena = torch.empty(n, dtype=torch.bfloat16, device=self.src[0].device)
        self.dst, o = [], 0
        for w in self.src:
            self.dst.append(self.arena[o:o + w.numel()].view(w.shape[1], w.shape[0]))
            o += w.numel()

    def refresh(self):
        ops.transpose_bf16_(self.src, self.dst)

    def attach(self, P: ModelTensors) -> ModelTensors:
        for i, bp in enumerate(P.blocks):
            for j, k in enumerate(self.KINDS):
                setattr(bp, k + "_wt", self.dst[len(self.KINDS) * i + j])
        return P


@dataclass
class EngineConfig:
    lr: float = 3.125e-4
    weight_decay: float = 0.05
    betas: Tuple[float, float] = (0.9, 0.999)
    eps: float = 1e-8
    max_grad_norm: float = 1.0
    t_max: int = 0            # cosine annealing period in optimizer steps (0: constant LR)
    eta_min: float = 0.0
    use_graph: bool = True
    graph_warmup: int = 3     # eager steps before capture
    bucket_blocks: int = 2    # transformer blocks per all-reduce bucket
    # the embedding gradients (cls / pos / patch-embed / time-embed, final only
    # after the embedding backward) get their own small last bucket, so block 0's
    # all-reduce overlaps the embedding backward and only ~0.4 MB (ViT-tiny) is
    # exposed before the optimizer
    embed_bucket: bool = True
    seed: int = 42
    loss_beta: float = 1.0
    ema_decay: float = 0.99
    ema_init: float = 5.0     # multi_gpu_trainer.py:52 (loss_rec = 5.0)
    force_segments: bool = False  # segmented capture + collectives even at world size 1 (testing)
    # rows of time_embed that can receive gradient (t < temb_rows for every sample);
    # the rest are all-zero on every rank and are left out of the all-reduce.
    # Cold diffusion draws t in 1..log2(W) (7 rows), so for ViT-tiny this drops
    # 3.1 MB of the 28.7 MB gradient all-reduce.  None: all rows.
    temb_rows: Optional[int] = None
    # data parallel with t drawn from the whole table (Gaussian diffusion, temb_rows
    # None): only the <= world x batch rows indexed by this step's timesteps carry
    # gradient, so the time_embed gradient is exchanged as all-gathered (t, row)
    # pairs (49 KB per rank for ViT-tiny at batch 32) instead of all-reducing the
    # dense [2000, 384] table (3.1 MB).  SURVEY.md §5.8 option 4.
    temb_sparse: bool = True
    # data parallel without comm_events: capture the bucketed all-reduces INTO the
    # step's one hipGraph (RCCL kernels on a comm-stream branch joined before the
    # optimizer) instead of replaying one graph segment per bucket with host-issued
    # collectives in between.  Measured on one MI355X with a 1-rank RCCL group:
    # 0.998 ms/step captured vs 1.125 segmented (each extra graph launch + stream join
    # costs ~30 us).  Falls back to segments if the capture raises.
    graph_comm: bool = True
    # data parallel, the default capture (event-split): the step's compute as TWO linear
    # graphs (forward + backward, then optimizer); the collectives are issued by the
    # host (eager RCCL, nothing of it captured), on the comm stream each behind a
    # polling kernel for the per-bucket counter that a 1-lane kernel node of the compute
    # graph bumps at the bucket's boundary, or (comm_inline) on the compute stream
    # between the two graphs.  A graph with a comm-stream branch (graph_comm) costs
    # ~30-35 us per fork on MI355X -- measured on one GPU with a 1-element kernel on a
    # side stream at each of the 5 bucket boundaries: 0.818 -> 1.013 ms/step -- and with
    # one elementwise pass per bucket on the comm stream (standing in for the
    # collective) the event-split step runs at 0.937 vs 1.072 captured.  False:
    # graph_comm / segments.
    comm_events: bool = True
    # data parallel: issue the collectives on the compute stream (no comm stream, no
    # overlap; with comm_events, host-issued between the two step graphs).  With one
    # bucket this is the single-process step + one all-reduce of the whole arena;
    # autotune_comm() measures it against the overlapped layouts on the real ranks.
    comm_inline: bool = False
    # micro-batches per optimizer step (batch_fn is called grad_accum times per
    # step; gradients accumulate in the arena, averaged in the optimizer; the
    # all-reduce runs once, after the last micro-batch's backward)
    grad_accum: int = 1
    # gradient all-reduce wire format: "fp32" (reference DDP semantics) or "bf16"
    # (halves the xGMI bytes; the sum is accumulated in bf16 by RCCL)
    grad_wire: str = "fp32"
    # who issues the gradient collectives: "torch" (torch.distributed 'nccl' =
    # RCCL through ProcessGroupNCCL) or "native" (csrc/comm.cpp: our own
    # ncclComm_t, collectives enqueued directly on the comm stream, bf16 wire
    # pack/unpack as two fused kernels).  torch.distributed stays the control
    # plane (rendezvous, barriers, metrics) either way.
    # "auto" (default): native when it initialises and verifies on every rank of the
    # default group (GPU), else torch
    comm: str = "auto"
    # a batch source with ``fused_spec()`` (data.synthetic.ColdBatcher) has its draw
    # fused into the patch-embedding launch (ops.patch_embed_cold_fwd: the patch rows
    # pixelated straight from the pool, x_t never materialised): one launch fewer
    # per step, identical values.
    fuse_batch: bool = True
    # optimizer steps per hipGraph replay for train_steps(n) (one graph holding K
    # complete steps, every counter on the device): the inter-replay dispatch gap
    # (~8 us before each step's first kernel in the graph-mode trace) is paid once
    # per K steps.  train_step() keeps replaying the one-step graph.
    graph_steps: int = 1
    # exponential moving average of the WEIGHTS (not the loss: that is ema_decay above):
    # 0 = off, else the decay d of e <- p + d (e - p), kept in one more fp32 arena that the
    # optimizer launch updates in the same pass (no extra launch, no communication: data
    # parallel replicas are bit-identical and so are their EMAs).  Read it with
    # ema_state_dict(), evaluate / sample on it inside ``with engine.ema_weights():``.
    # With it on, the lazy time-embedding range is off: those rows go through the
    # optimizer pass every step, as torch.optim.AdamW would update them, so that their
    # EMA follows them (~11 % of the ViT-tiny arena back in the pass).
    weight_ema: float = 0.0
    # ramp the decay as min(weight_ema, (1 + t) / (10 + t)) over the Adam steps t done so
    # far (0.1 at the first update), so the average forgets the initial weights quickly;
    # a resume continues the ramp from the restored Adam step
    weight_ema_warmup: bool = True


@dataclass(frozen=True)
class Switches:
    """The module switches above, as read when a :class:`StepPlan` is built."""
    ln_final: bool = True
    sqnorm: bool = True
    embed_wgrad: bool = True
    overwrite: bool = True


def step_decisions(cfg: EngineConfig, sw: Switches, world: int, segmented: bool, is_cuda: bool, B: int,
                   has_temb_grad: bool) -> Dict[str, bool]:
    """The step's fusion decisions, from the configuration alone (no tensors):

    * ``merge``: without a separate embedding bucket (single process) the patch-embedding
      weight gradient joins block 0's grouped launch;
    * ``ln_final``: the LayerNorm replica finalize rides in the embedding-backward launch
      (data parallel too: every LayerNorm lives in the last bucket's arena range);
    * ``overwrite``: see ``GRAD_OVERWRITE``;
    * ``fuse_sq``: single process, one micro-batch -- the one deferred weight-gradient launch
      is the last writer of the gradient arena and writes the grad-norm partials too;
    * ``embed_fused``: see ``FUSE_EMBED_WGRAD`` (its workgroups index a batch of <= 256)."""
    merge = not (segmented and cfg.embed_bucket)
    ln_final = is_cuda and sw.ln_final
    overwrite = sw.overwrite and ln_final and max(1, int(cfg.grad_accum)) == 1
    fuse_sq = sw.sqnorm and overwrite and not segmented and world == 1
    embed_fused = fuse_sq and sw.embed_wgrad and merge and has_temb_grad and B <= 256
    return dict(merge=merge, ln_final=ln_final, overwrite=overwrite, fuse_sq=fuse_sq, embed_fused=embed_fused)


@dataclass(frozen=True)
class StepPlan:
    """Every decision of one optimizer step at one batch size (:meth:`TrainEngine._plan`),
    with the bundles built from them.  ``tail``: the loss bookkeeping and counter advance
    ride in the LayerNorm-fold launch after the optimizer; ``fused_loss``: the head GEMM's
    epilogue computes the loss partials and the token-layout gradient; ``fuse_batch``: a
    batch source with ``fused_spec()`` is drawn inside the patch-embedding launch;
    ``flush_at``: the blocks after which a gradient bucket's weight gradients are issued
    (None: single process, one launch after the backward); ``embed_owners``: the time
    embedding rows of ``embed_fused``, else None; the rest as in :func:`step_decisions`."""
    k_acc: int
    tail: bool
    fused_loss: bool
    fuse_batch: bool
    merge: bool
    flush_at: Optional[frozenset]
    overwrite: bool
    fuse_sq: bool
    embed_owners: Optional[int]
    ln_final: Optional[ops.LnFinal]
    backward: BackwardPlan


class TrainEngine:
    def __init__(self, model, cfg: EngineConfig = EngineConfig(), device=None, process_group=None):
        self.cfg = cfg
        self.model = model
        self.device = torch.device(device) if device is not None else next(model.parameters()).device
        model.to(self.device)
        self.prog = ViTProgram.from_model(model)
        self.pg = process_group
        self.dist_on = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(process_group) if self.dist_on else 1
        self.rank = dist.get_rank(process_group) if self.dist_on else 0
        self.segmented = self.world > 1 or cfg.force_segments
        self.is_cuda = self.device.type == "cuda"
        if not 0.0 <= float(cfg.weight_ema) < 1.0:
            raise ValueError(f"weight_ema must be in [0, 1), got {cfg.weight_ema!r}")
        self._build_arenas()
        dev = self.device
        self.rng = torch.tensor([cfg.seed, 0], dtype=torch.int64, device=dev)
        self.step_ctr = torch.zeros(2, dtype=torch.int64, device=dev)  # {adam step, scheduler step}
        b1, b2 = cfg.betas
        self.hyper = torch.tensor([cfg.lr, b1, b2, cfg.eps, cfg.weight_decay, cfg.max_grad_norm,
                                   float(cfg.t_max), cfg.eta_min], dtype=torch.float32, device=dev)
        # grad-norm partials (sqnorm, or the fused weight-gradient launch: one per 64x64
        # output tile + tail workgroups; the 2-D parameter count bounds the tiles)
        self.sqnorm = torch.zeros(ops.sq_parts_size(self.layout.sq_tiles), dtype=torch.float32, device=dev)
        # tickets of the weight-gradient launches' K-split tails: this engine's own, allocated
        # here (never inside a capture) and shared by its graphs, whose launches one stream orders
        self.wgrad_tickets = ops.wgrad_tickets(dev) if self.is_cuda else None
        self.loss_last = torch.zeros(1, dtype=torch.float32, device=dev)
        self.loss_ema = torch.full((1,), cfg.ema_init, dtype=torch.float32, device=dev)
        # the comm stream is created once and kept across set_comm_layout() (a stream
        # created later could land on a hardware queue another stream already holds)
        self._comm_obj = self._comm_stream() if (self.is_cuda and self.segmented) else None
        self.comm = None if cfg.comm_inline else self._comm_obj
        self.comm_choice: Optional[str] = None  # autotune_comm() winner
        self.comm_times: Dict[str, float] = {}
        if cfg.comm not in ("torch", "native", "auto"):
            raise ValueError(f"comm must be 'torch', 'native' or 'auto', got {cfg.comm!r}")
        self.ncomm = None
        self.native_error: Optional[str] = None  # why comm='auto' fell back to torch.distributed
        self.comm_fallback: Optional[str] = None  # autotune_comm: why no layout ran (eager inline fallback)
        default_pg = process_group is None or process_group is dist.group.WORLD
        if cfg.comm == "native" and self.dist_on and self.is_cuda:
            if not default_pg:
                raise ValueError("comm='native' spans the default process group only")
            from ..parallel.comm import NativeComm
            self.ncomm = NativeComm(dev)
        elif cfg.comm == "auto" and self.dist_on and self.is_cuda and default_pg:
            self.ncomm = self._try_native(dev)
        self.comm_backend = "native" if self.ncomm is not None else "torch"
        # the captured step: written by _capture(), cleared by _drop_capture() only
        self._graphs: Optional[List[torch.cuda.CUDAGraph]] = None
        self._mode: Optional[str] = None  # how _graphs replay: SINGLE / EVENT_SPLIT / SEGMENTS
        self._multi = None  # (K-step graph, K) for train_steps
        self._plans: Dict[int, StepPlan] = {}  # _plan(): by batch size
        self._signal = None  # event-split step with a comm stream: the buckets' FlagSignal
        # event-split step: "pre-issued" / "post-replay" (comm stream), "inline" (none)
        self.handoff_order: Optional[str] = None
        self._graph_comm_failed = False  # captured collectives refused -> per-bucket segments
        self._eager_steps = 0
        self.comm_fit = None  # probe_allreduce()'s fitted all-reduce model
        self._snap = None  # snapshot_to_host() buffers
        self._sched_template = None  # scheduler_state_dict() key layout
        self.batch_fn: Optional[Callable] = None
        self._static = None
        self.steps_done = 0
        if self.world > 1:
            if self.ncomm is not None:
                self.ncomm.broadcast_(self.flat_p, 0)
            else:
                dist.broadcast(self.flat_p, src=0, group=self.pg)
            self._refresh_shadow()
        # weight EMA arena: a copy of the final (loaded, broadcast) parameters; the frozen
        # tail past train_hi is never updated and just stays equal to them
        self.flat_e = self.opt_e = None
        self._ema_tmp = None      # ema_weights(): the swap's reusable temp arena
        self._ema_scope = False   # inside ema_weights(): flat_p holds the EMA
        if cfg.weight_ema > 0:
            self.flat_e = self.flat_p.clone()
            self.opt_e = self.flat_e[:self.layout.train_hi]
        model._engine = self

    def _comm_stream(self):
        """The collectives' stream, high priority.  HIP keeps a separate pool of hardware queues per priority, so a
        high-priority comm stream can never share an in-order hardware queue with the
        normal-priority compute stream -- with GPU_MAX_HW_QUEUES=4 normal-priority
        streams beyond four do share queues round-robin, and a comm-stream wait
        queued ahead of the compute graph on a SHARED queue would block that graph
        (see :meth:`_preissue_ok`)."""
        return torch.cuda.Stream(device=self.device, priority=-1)

    def _preissue_ok(self) -> bool:
        """Queue the comm stream's counter waits + collectives AHEAD of the compute
        graph replay only when that cannot deadlock-until-timeout: RCCL issue never
        blocks the host, and the comm stream has a different priority from the
        compute stream, i.e. its own hardware queue.  Otherwise the host issues them
        after the replay (same overlap, ~2-3 us later start per bucket)."""
        if not (PREISSUE and self.comm is not None and self._comm_host_async()):
            return False
        return self.comm.priority != torch.cuda.current_stream(self.device).priority

    def _try_native(self, dev):
        """comm='auto': our own RCCL communicator if it comes up and sums correctly on
        EVERY rank (agreed through the torch process group), else torch.distributed.
        Its collectives are enqueued straight on the issuing stream; ProcessGroupNCCL
        runs each on its internal stream behind an event round trip each way (1-rank
        inline step: 0.849 vs 0.866 ms)."""
        import warnings
        from ..parallel.watchdog import phase
        phase("native-comm:check")
        # every rank must be able to enter ncclCommInitRank before any does: the init
        # blocks until all ranks have joined, so a rank that fails BEFORE it (no
        # extension, no comm ops) would leave the others hanging there
        ready = 1
        try:
            from ..ops import _ext
            _ext.load(raise_on_error=True)
            ready = int(hasattr(torch.ops.ddim_cold, "comm_init"))
        except Exception as e:  # pragma: no cover - depends on the build
            warnings.warn(f"native RCCL communicator unavailable ({e!r})")
            ready = 0
        flag = torch.tensor([ready], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.pg)
        if int(flag.item()) != 1:
            return None
        nc, ok = None, 1
        phase("native-comm:init")
        try:
            from ..parallel.comm import NativeComm
            nc = NativeComm(dev)
            phase("native-comm:verify", ranks=nc.info()[0])
            x = torch.full((4 * self.world + 3,), float(self.rank + 1), device=dev)
            nc.all_reduce_(x)
            torch.cuda.synchronize(dev)
            ok = int(bool((x == self.world * (self.world + 1) / 2).all()))
            if not ok:
                self.native_error = "verification sum mismatch"
        except Exception as e:  # noqa: BLE001 - any failure falls back to torch.distributed
            warnings.warn(f"native RCCL communicator unavailable ({e!r}); using torch.distributed")
            self.native_error = repr(e)[:300]
            ok = 0
        flag = torch.tensor([ok], dtype=torch.int32, device=dev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.pg)
        if int(flag.item()) == 1:
            phase("native-comm:ready", ranks=self.world)
            return nc
        if self.native_error is None:
            self.native_error = "failed on another rank"
        if nc is not None and nc.handle is not None:
            nc.destroy()
        phase("native-comm:fallback-torch", error=self.native_error)
        return None

    def _comm_rccl(self) -> bool:
        """Are the gradient collectives RCCL's (our communicator, ProcessGroupNCCL) or the
        device loopback pair's?  Under either name below: issuing one never blocks the host
        on device progress, and it can be captured into a hipGraph.  gloo with CUDA tensors
        waits on the host for its device-to-host copy -- its collectives must not be queued
        ahead of the compute graph they wait for -- and aborts the process inside a capture."""
        if self.ncomm is not None:
            return True
        try:
            return dist.get_backend(self.pg) == "nccl"
        except Exception:  # pragma: no cover - no process group
            return False

    _comm_host_async = _comm_capturable = _comm_rccl

    def check_comm(self):
        """Raise ``RuntimeError`` if a comm-stream hand-off wait timed out (FlagSignal):
        that bucket's collective then ran on gradients that were not final yet, so the
        replicas may have diverged -- the run must stop (and resume from a checkpoint),
        not continue.  One host sync; call at log points, not every step."""
        if self._signal is not None:
            self._signal.check()

    def comm_error(self) -> bool:
        """True if a hand-off wait has timed out since the last :meth:`reset_comm_error`."""
        return self._signal is not None and self._signal.failed()

    def reset_comm_error(self):
        if self._signal is not None:
            self._signal.err.zero_()

    def attach_comm(self, comm, world: int):
        """Drive the gradient exchange through ``comm`` (the ``all_reduce_`` of a
        NativeComm-like object) as one of ``world`` data-parallel replicas without a
        process group -- e.g. two engines of one process on one device joined by a
        :class:`parallel.comm.LoopbackPair` (tests of the cross-rank hand-off).  Needs
        ``force_segments`` (the data-parallel step); the replicas must start from the
        same parameters (no broadcast here)."""
        if not (self.segmented and self.is_cuda):
            raise ValueError("attach_comm needs a GPU engine built with force_segments=True")
        if self.bucketing.temb_bucket is not None and not hasattr(comm, "all_gather_"):
            raise ValueError(f"{type(comm).__name__} has no all_gather_, which this engine's sparse time-embedding "
                             "gradient exchange needs (Gaussian diffusion: temb_rows=None); build the engine "
                             "with temb_rows or temb_sparse=False")
        self.ncomm = comm
        self.world = int(world)
        self.comm_backend = type(comm).__name__
        self._drop_capture(rewarm=False)

    def close(self):
        """Release the native communicator (before the process group is destroyed)."""
        self.materialize_lazy()
        if self.ncomm is not None:
            if self.is_cuda:
                torch.cuda.synchronize(self.device)
            self.ncomm.destroy()
            self.ncomm = None

    # ------------------------------------------------------------------ arenas
    def _build_arenas(self):
        """Allocate the arenas that :attr:`layout` (``train/layout.py``: the ordering policy
        and the alignment) describes and rebind the model's parameters and gradients as
        views of them; then everything else that holds arena views."""
        named = list(self.model.named_parameters())
        c, cfg, dev = self.prog.cfg, self.cfg, self.device
        self.layout: ArenaLayout = arena_layout([(n, tuple(p.shape), p.requires_grad) for n, p in named],
                                                c.depth, c.dim, c.total_steps, cfg.temb_rows, cfg.weight_ema)
        lay = self.layout
        self.flat_p = torch.zeros(lay.numel, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(lay.numel, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(lay.numel, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(lay.numel, dtype=torch.float32, device=dev)
        self.flat_pb = torch.zeros(lay.numel, dtype=torch.bfloat16, device=dev)
        if cfg.grad_wire not in ("fp32", "bf16"):
            raise ValueError(f"grad_wire must be 'fp32' or 'bf16', got {cfg.grad_wire!r}")
        self.flat_gw = torch.zeros(lay.numel, dtype=torch.bfloat16, device=dev) if cfg.grad_wire == "bf16" else None
        views_g = {}
        for n, p in named:
            o, k = lay.offsets[n]
            vp = self.flat_p[o:o + k].view_as(p)
            vp.copy_(p.data)
            p.data = vp
            views_g[n] = self.flat_g[o:o + k].view_as(p)
            p.grad = None if n in lay.frozen else views_g[n]
        # the optimizer's ranges (frozen tensors excluded)
        self.opt_p, self.opt_g, self.opt_m, self.opt_v, self.opt_pb = (
            t[:lay.train_hi] for t in (self.flat_p, self.flat_g, self.flat_m, self.flat_v, self.flat_pb))
        # the bf16 shadows the MFMA GEMMs read; every other parameter is read in fp32
        shadows = {n: self.flat_pb[o:o + k].view(p.shape)
                   for n, p in named for o, k in [lay.offsets[n]] if is_matrix_param(n)}
        # LayerNorm fold: gamma-scaled bf16 weights / row sums / folded biases of
        # the QKV, fc1 and head GEMMs, recomputed from the fp32 masters after
        # every optimizer step (inside the step graph)
        # (reads the bf16 shadow the optimizer just wrote: half the bytes of the fp32 masters)
        self.lnfold = LnFold({n: p.data for n, p in named}, c.depth, weights=shadows) if _program.FOLD_LN else None
        self.wt = None
        self._refresh_shadow()
        self.param_tensors: ModelTensors = collect({n: shadows.get(n, p.data) for n, p in named}, c.depth, c.dim)
        if self.lnfold is not None:
            self.lnfold.attach(self.param_tensors)
        if self.is_cuda and c.tokens >= TRANSPOSED_DGRAD_MIN_TOKENS:
            self.wt = TransposedShadows(self.param_tensors)
            self.wt.attach(self.param_tensors)
            self.wt.refresh()
        self.grad_tensors: ModelTensors = collect(views_g, c.depth, c.dim)
        if not c.learn_temb:
            self.grad_tensors.temb = None
        self._temb_t: List[torch.Tensor] = []
        # the optimizer skips the time_embed rows no sample can select (``layout.lazy``) and
        # accumulates their weight-decay factor on the device (lazy_decay); materialize_lazy()
        # applies it before anything reads them (end of train_steps, snapshots, state dicts).
        # Run state: a resume can turn it off (_check_lazy_moments)
        self.lazy = lay.lazy
        self.lazy_decay = torch.ones(1, dtype=torch.float32, device=dev)
        self._lazy_dirty = False
        # LayerNorm dgamma/dbeta replica destinations, in ``layout.ln_order``: the grad-arena
        # range of each one's weight + bias
        self.ln_dsts = [self.flat_g[o:o + 2 * c.dim] for o in lay.ln_offs]
        # workspace rows depend on the backward's row count (ops.ln_ws_rows): allocated by
        # _ensure_batch_buffers at the first step of a batch size (eager, never inside a capture)
        self.ln_ws = None
        self.ln_R = 0
        self.ln_ptrs = torch.tensor([t.data_ptr() for t in self.ln_dsts], dtype=torch.int64, device=dev) \
            if self.is_cuda else None
        self._build_buckets()

    def _build_buckets(self):
        """The gradient-exchange layout of ``cfg.bucket_blocks`` / ``cfg.embed_bucket``
        (re-run by :meth:`set_comm_layout`)."""
        sparse = self.cfg.temb_sparse and self.segmented and self.grad_tensors.temb is not None
        self.bucketing: BucketLayout = bucket_layout(self.layout, self.cfg.bucket_blocks, self.cfg.embed_bucket, sparse)

    def _ensure_batch_buffers(self, B: int):
        """Buffers sized by the batch: the LayerNorm dgamma/dbeta slot workspaces
        ([2L+1, ops.ln_ws_rows(B N), 2D]) and room in the grad-norm partials for the
        embedding workgroups of the weight-gradient launch (FUSE_EMBED_WGRAD)."""
        c, n_ln = self.prog.cfg, len(self.layout.ln_order)
        D, M = c.dim, B * c.tokens
        rows = ops.ln_ws_rows(M)
        nparts = ops.sq_parts_size(self.layout.sq_tiles + ops.wgrad_embed_slots(
            B, c.tokens, D, self._emb_owners(B), n_ln, 2 * D, M))
        if (self.ln_ws is not None and self.ln_ws.shape[1] == rows and self.sqnorm.numel() >= nparts):
            return
        if self.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the batch size changed inside a graph capture (LayerNorm workspace)")
        self._plans.clear()  # they hold views of the buffers replaced here
        self.ln_ws = torch.zeros(n_ln, rows, 2 * D, dtype=torch.float32, device=self.device)
        self.ln_R = rows
        if self.sqnorm.numel() < nparts:
            self.sqnorm = torch.zeros(nparts, dtype=torch.float32, device=self.device)

    def _emb_owners(self, B: int) -> int:
        """Distinct timesteps a batch of ``B`` can hold (time-embedding gradient rows)."""
        rows = self.cfg.temb_rows
        return max(1, min(B, rows if rows is not None else self.prog.cfg.total_steps))

    def _refresh_shadow(self):
        self.flat_pb.copy_(self.flat_p.to(torch.bfloat16))
        if self.lnfold is not None:
            self.lnfold.refresh()
        if self.wt is not None:
            self.wt.refresh()

    # ------------------------------------------------------------------ step program
    def set_batch_fn(self, fn: Callable):
        """``fn() -> (x_t, target, t)`` device tensors; called inside the captured region."""
        self.batch_fn = fn
        self._drop_capture(rewarm=False)

    @property
    def _fuse_batch(self) -> bool:
        return self.cfg.fuse_batch and self.lnfold is not None and self.prog.supports_fused_loss(self.param_tensors)

    def _plan(self, B: int) -> StepPlan:
        """The step's decisions at batch size ``B``, cached until the capture is dropped or
        the batch buffers (whose views the plan holds) are reallocated."""
        self._ensure_batch_buffers(B)
        plan = self._plans.get(B)
        if plan is None:
            c, cfg = self.prog.cfg, self.cfg
            sw = Switches(FUSE_LN_FINAL, FUSE_SQNORM, FUSE_EMBED_WGRAD, GRAD_OVERWRITE)
            d = step_decisions(cfg, sw, self.world, self.segmented, self.is_cuda, B,
                               self.grad_tensors.temb is not None)
            tail = self.lnfold is not None
            hi = self.bucketing.ln_done_at[-1]
            ln_final = ops.LnFinal(self.ln_ws[:hi], self.ln_ptrs[:hi], 2 * c.dim, self.ln_R, d["overwrite"],
                                   list(self.layout.ln_offs[:hi])) if d["ln_final"] else None
            flush_at = frozenset(k for k in self.bucketing.bucket_after if k >= 0) if self.segmented else None
            owners = self._emb_owners(B) if d["embed_fused"] else None
            bwd = BackwardPlan(ln_ws=self.ln_ws, embed_with_block0=d["merge"], ln_final=ln_final, flush_at=flush_at,
                               store=d["overwrite"], owners=owners, tickets=self.wgrad_tickets,
                               grad_norm=ops.GradNorm(self.sqnorm, self.opt_g, self.lazy) if d["fuse_sq"] else None)
            plan = self._plans[B] = StepPlan(
                k_acc=max(1, int(cfg.grad_accum)), tail=tail,
                fused_loss=tail and self.prog.supports_fused_loss(self.param_tensors), fuse_batch=self._fuse_batch,
                merge=d["merge"], flush_at=flush_at, overwrite=d["overwrite"], fuse_sq=d["fuse_sq"],
                embed_owners=owners, ln_final=ln_final, backward=bwd)
        return plan

    def _step_iter(self):
        """One optimizer step: yields ``("bucket", k)`` when gradient bucket ``k`` is final
        (last micro-batch) and ``("done", -1)`` after the optimizer."""
        self._temb_t = []
        k_acc = max(1, int(self.cfg.grad_accum))
        loss_parts = None
        for micro in range(k_acc):
            if micro > 0:
                self.rng[1:].add_(1)  # fresh dropout masks and batch draws per micro-batch
            spec = getattr(self.batch_fn, "fused_spec", None)
            # (a fused spec is drawn inside the patch-embedding launch)
            batch, cold = spec() if self._fuse_batch and spec is not None else (self.batch_fn(), None)
            plan = self._plan(int(batch[2].shape[0]))
            loss_parts = yield from self._micro_batch(plan, batch, cold, micro == k_acc - 1, loss_parts)
        self._optimizer_tail(plan, loss_parts)
        yield ("done", -1)

    def _micro_batch(self, plan: StepPlan, batch, cold, last: bool, loss_acc):
        """Forward, loss and backward of one micro-batch, yielding at the gradient bucket
        boundaries of the ``last`` one; returns the step's loss partials so far.  With
        grad_accum > 1 the micro-batch partials are averaged, so the loss EMA moves once
        per optimizer step (multi_gpu_trainer.py:126 semantics)."""
        c, cfg = self.prog.cfg, self.cfg
        img, tgt, t = batch
        self._temb_t.append(t)
        if plan.fused_loss:
            (loss_parts, dtok), S = self.prog.forward(self.param_tensors, img, t, self.rng, True,
                                                      loss=(tgt, cfg.loss_beta), cold=cold)
        else:
            out, S = self.prog.forward(self.param_tensors, img, t, self.rng, True)
            if plan.tail or plan.k_acc > 1:
                loss_parts, dtok = ops.smooth_l1_fwd_bwd(out, tgt, c.tokens, c.patch, cfg.loss_beta, finish=False)
            else:
                loss_parts = None  # finished here: loss_last and its EMA
                _, dtok = ops.smooth_l1_fwd_bwd(out, tgt, c.tokens, c.patch, cfg.loss_beta, self.loss_last,
                                                self.loss_ema, cfg.ema_decay)
            del out
        if plan.k_acc > 1:  # mean over micro-batches (partials sum to each micro-batch's loss)
            lp = loss_parts.float() * (1.0 / plan.k_acc)
            loss_parts = lp if loss_acc is None else loss_acc + lp
        ln_lo, bk = 0, self.bucketing
        for i in self.prog.backward_iter(self.param_tensors, self.grad_tensors, S, dtok, self.rng, True,
                                         plan=plan.backward):
            if i in bk.bucket_after and (self.segmented or i == -1):
                hi = bk.ln_done_at[i]
                if plan.ln_final is not None:
                    ln_lo = hi  # already finalized by the embedding backward
                if hi > ln_lo:
                    ops.replica_reduce_(self.ln_ws[ln_lo:hi], None if self.ln_ptrs is None else self.ln_ptrs[ln_lo:hi],
                                        2 * c.dim, self.ln_R, dsts=self.ln_dsts[ln_lo:hi])
                    ln_lo = hi
                if last:
                    yield ("bucket", bk.bucket_after[i])
        return loss_parts

    def _optimizer_tail(self, plan: StepPlan, loss_parts):
        """Grad norm (unless the weight-gradient launch wrote it), AdamW, the transposed
        shadows, then the LayerNorm fold carrying the loss bookkeeping and counter advance
        (:class:`ops.StepTail`) or those as launches of their own."""
        cfg = self.cfg
        # grads are SUM-reduced over ranks and summed over micro-batches -> average via grad_scale
        gs = 1.0 / (self.world * plan.k_acc)
        if not plan.fuse_sq:
            ops.sqnorm(self.opt_g, self.sqnorm, gs, lazy=self.lazy)
        ema = {} if self.opt_e is None else dict(ema=self.opt_e, ema_decay=cfg.weight_ema,
                                                 ema_warmup=cfg.weight_ema_warmup)
        ops.adamw_step(self.opt_p, self.opt_g, self.opt_m, self.opt_v, self.opt_pb, self.sqnorm,
                       self.step_ctr, self.hyper, gs, zero_hi=self.layout.acc_hi if plan.overwrite else None,
                       lazy=self.lazy, lazy_decay=self.lazy_decay, **ema)
        if self.wt is not None:  # the input-gradient GEMMs' transposed shadows of the new weights
            self.wt.refresh()
        if plan.tail:
            self.lnfold.refresh(tail=ops.StepTail(loss_parts, self.loss_last, self.loss_ema, cfg.ema_decay,
                                                  self.step_ctr, self.rng, self.sqnorm))
        else:
            if plan.k_acc > 1:  # one EMA update per optimizer step
                loss = loss_parts.sum().reshape(self.loss_last.shape)
                self.loss_last.copy_(loss)
                self.loss_ema.mul_(cfg.ema_decay).add_(loss, alpha=1.0 - cfg.ema_decay)
            ops.advance_counters(self.step_ctr, self.rng, self.sqnorm)
        self.prog._keep = None

    def _allreduce(self, k: int, wait_counter: bool = False):
        """Issue bucket ``k``'s collectives: on the comm stream, ordered after the
        current stream (``wait_counter``: after the bucket's counter instead, bumped at
        its boundary inside the replayed compute graph), or with no comm stream right
        here on the current stream."""
        if self.ncomm is None and (not self.dist_on or (self.world <= 1 and not self.cfg.force_segments)):
            return
        ranges = self.bucketing.ranges[k]

        fake = os.environ.get("DDIM_COLD_FAKE_COMM") == "1"

        def reduce():
            many = getattr(self.ncomm, "all_reduce_many_", None)
            if many is not None and self.flat_gw is None and not fake and len(ranges) > 1:
                # the bucket's ranges as one RCCL group: one launch
                many([self.flat_g[a:b] for a, b in ranges])
                todo = ()
            else:
                todo = ranges
            for a, b in todo:
                if fake:  # topology experiment at 1 rank: passes over the range stand in for the collective
                    self.flat_g[a:b].mul_(1.0)
                elif self.ncomm is not None:
                    if self.flat_gw is None:
                        self.ncomm.all_reduce_(self.flat_g[a:b])
                    else:
                        self.ncomm.all_reduce_bf16_wire_(self.flat_g[a:b], self.flat_gw[a:b])
                elif self.flat_gw is None:
                    dist.all_reduce(self.flat_g[a:b], group=self.pg)
                else:  # bf16 wire: fused pack, reduce, fused unpack (on the comm stream)
                    w = self.flat_gw[a:b]
                    ops.wire_pack(self.flat_g[a:b], w)
                    dist.all_reduce(w, group=self.pg)
                    ops.wire_unpack(w, self.flat_g[a:b])
            if k == self.bucketing.temb_bucket:
                self._temb_exchange()

        if self.comm is not None:
            if wait_counter:
                self._signal.wait(k, self.comm)
            else:
                self.comm.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.comm):
                reduce()
        else:
            reduce()

    def _temb_exchange(self):
        """Sum the time_embed gradient over ranks from its non-zero rows only.

        Each rank contributes (t, row) for the distinct timesteps of its micro-batches
        (a repeated t keeps its first row, which already holds every sample's
        contribution), all-gathered; every rank then forms each gathered row's total
        with one [W*n, W*n] 0/1 matrix product over the gathered rows -- the same
        inputs and the same kernel on every rank, so the replicas stay bit-identical
        (a scatter-add with atomics would round differently per rank) -- and writes it
        back to those rows.  Rows no rank touched are zero everywhere already."""
        g = self.grad_tensors.temb
        idx = torch.cat([t.reshape(-1) for t in self._temb_t]).to(torch.int64)
        n = idx.numel()
        rows = g.index_select(0, idx)
        first = ~(idx[:, None] == idx[None, :]).tril(-1).any(1)
        rows.mul_(first[:, None].to(rows.dtype))
        idx_all = idx.new_empty(self.world * n)
        rows_all = rows.new_empty(self.world * n, g.shape[1])
        if self.ncomm is not None:  # every per-step collective on the one gradient communicator
            self.ncomm.all_gather_(idx_all, idx)
            self.ncomm.all_gather_(rows_all, rows)
        else:
            dist.all_gather_into_tensor(idx_all, idx, group=self.pg)
            dist.all_gather_into_tensor(rows_all, rows, group=self.pg)
        same = (idx_all[:, None] == idx_all[None, :]).to(rows.dtype)
        g.index_copy_(0, idx_all, same @ rows_all)

    def _join_comm(self):
        if self.comm is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.comm)

    # ------------------------------------------------------------------ comm layout
    # candidate gradient-exchange layouts for autotune_comm(): (name, bucket_blocks,
    # embed_bucket, inline).  overlap-*: buckets of 2 / 4 blocks + the embeddings,
    # all-reduced on the comm stream while the backward goes on; inline-1: ONE
    # all-reduce of the whole arena on the compute stream after the backward (no
    # second queue: the single-process step + the collective).  These run
    # event-split: collectives host-issued between the step's two graphs.
    # graph-inline-1: the same single all-reduce CAPTURED on the compute stream
    # inside the step graph -- one linear graph, no second queue, no host hand-off,
    # so ``graph_steps`` K-step graphs work data parallel too (the event-split
    # layouts replay two graphs per step).  graph-<overlap>: the captured comm-stream
    # branch (a fork/join per bucket inside the graph, K-step graphs as well).
    COMM_LAYOUTS = (("graph-inline-1", 1 << 16, False, True), ("overlap-2", 2, True, False),
                    ("overlap-4", 4, True, False), ("inline-1", 1 << 16, False, True))

    @classmethod
    def layout_by_name(cls, name: str):
        """``(name, bucket_blocks, embed_bucket, inline)`` for ``[graph-]overlap-<blocks>``
        / ``[graph-]inline-1`` (``graph-``: collectives captured in the step graph)."""
        base = name[6:] if name.startswith("graph-") else name
        if base == "inline-1":
            return (name, 1 << 16, False, True)
        if base.startswith("overlap-") and base[8:].isdigit() and int(base[8:]) >= 1:
            return (name, int(base[8:]), True, False)
        raise ValueError(f"unknown gradient-exchange layout {name!r} ([graph-]overlap-<blocks> or "
                         "[graph-]inline-1)")

    def apply_layout(self, layout):
        """Switch to a layout given by name or ``(name, bucket_blocks, embed_bucket,
        inline[, ...])``; records it as :attr:`comm_choice`.  A captured (``graph-``)
        layout on a non-capturable backend (gloo) runs as its event-split form."""
        L = self.layout_by_name(layout) if isinstance(layout, str) else tuple(layout)
        captured = L[0].startswith("graph-")
        if captured and self.is_cuda and self.segmented and not self._comm_capturable():
            import warnings
            warnings.warn(f"layout {L[0]}: collectives of this backend cannot be captured in a hipGraph; "
                          f"running {L[0][6:]} (event-split)")
            L = (L[0][6:],) + tuple(L[1:])
            captured = False
        self.set_comm_layout(L[1], L[2], L[3], captured=captured)
        self.comm_choice = L[0]
        return L

    def step_profile(self):
        """Cost-model view of this engine's step (parallel.costmodel.StepProfile):
        gradient bytes per block and of the rest (embeddings, head, LayerNorms,
        active time_embed rows) on the wire, backward timing scaled from the
        measured ViT-tiny step by this batch's GEMM work."""
        from ..parallel import costmodel as cm
        c, lay = self.prog.cfg, self.layout
        wire = 2 if self.cfg.grad_wire == "bf16" else 4
        xb = getattr(self.batch_fn, "x_t", None)
        B = int(xb.shape[0]) if isinstance(xb, torch.Tensor) else 32
        prof = cm.vit_step_profile(c.depth, c.dim, c.hidden, B * c.tokens, 0, wire_bytes=wire)
        prof.head_bytes = float(lay.head_numel * wire)
        other = max(0, self.reduced_numel() - c.depth * lay.block_numel - lay.head_numel)
        prof.embed_bytes = float(other * wire)
        return prof

    def reduced_numel(self) -> int:
        """Elements all-reduced per step (inactive time_embed rows / frozen tensors skipped)."""
        return self.bucketing.reduced_numel

    def probe_allreduce(self, sizes_mb=(0.25, 1.0, 4.0, 16.0), reps: int = 10):
        """Measure the gradient all-reduce on THIS job's ranks (the engine's own comm
        path: native RCCL communicator or torch.distributed, fp32) at a few sizes and
        fit ``T = alpha + S / algbw`` (parallel.costmodel.fit_allreduce).  Max over
        ranks, HIP-event timed on the stream the collectives run on (host clock for
        gloo on the CPU).  Returns the fitted model and ``{bytes: us}``; ``(None, {})``
        when not data parallel."""
        if not (self.dist_on and self.world > 1):
            return None, {}
        import time
        from ..parallel import costmodel as cm
        from ..parallel.dist import all_reduce_max, barrier
        n_max = int(max(sizes_mb) * (1 << 20) // 4)
        buf = torch.zeros(n_max, dtype=torch.float32, device=self.device)
        out = {}

        def sync():
            if self.is_cuda:
                torch.cuda.synchronize(self.device)
        for mb in sizes_mb:
            n = int(mb * (1 << 20) // 4)
            x = buf[:n]

            def ar():
                if self.ncomm is not None:
                    self.ncomm.all_reduce_(x)
                else:
                    dist.all_reduce(x, group=self.pg)
            for _ in range(3):
                ar()
            sync()
            barrier()
            if self.is_cuda:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    ar()
                e1.record()
                sync()
                us = e0.elapsed_time(e1) * 1e3 / reps
            else:  # gloo on the CPU: host clock
                t0 = time.perf_counter()
                for _ in range(reps):
                    ar()
                us = (time.perf_counter() - t0) * 1e6 / reps
            out[4 * n] = all_reduce_max(us, self.device)
        del buf
        fit = cm.fit_allreduce(self.world, list(out), list(out.values()))
        self.comm_fit = fit
        return fit, out

    def model_layouts(self, model=None):
        """Layouts ordered by the cost model's predicted exposed comm time:
        ``[(name, bucket_blocks, embed_bucket, inline, exposed_us)]``; ``model`` =
        the fitted all-reduce model (:meth:`probe_allreduce`) or the a-priori xGMI
        ring model of this world size."""
        from ..parallel import costmodel as cm
        if model is None:
            model = self.comm_fit or cm.xgmi_ring_model(max(2, min(self.world, 8)))
        return cm.plan_buckets(self.step_profile(), model)

    def candidate_layouts(self):
        """autotune_comm()'s default candidates: :attr:`COMM_LAYOUTS` plus the cost
        model's predicted best (fitted model if :meth:`probe_allreduce` ran)."""
        cands = list(self.COMM_LAYOUTS)
        if self.is_cuda and self.segmented and not self._comm_capturable():
            cands = [L_ for L_ in cands if not L_[0].startswith("graph-")]
        best = self.model_layouts()[0]
        if best[0] not in [L_[0] for L_ in cands]:
            cands.insert(1, best[:4])  # right after graph-inline-1 (the time budget runs in order)
        return cands

    def set_comm_layout(self, bucket_blocks: Optional[int] = None, embed_bucket: Optional[bool] = None,
                        inline: Optional[bool] = None, captured: Optional[bool] = None):
        """Re-bucket the gradient all-reduce and choose where its collectives run (a
        comm-stream branch overlapping the backward, or inline on the compute
        stream) and how (``captured``: inside the step graph; else host-issued
        between the event-split graphs).  The step graphs are dropped and
        re-captured after ``graph_warmup`` eager steps of the new layout."""
        import dataclasses
        kw = {}
        if bucket_blocks is not None:
            kw["bucket_blocks"] = int(bucket_blocks)
        if embed_bucket is not None:
            kw["embed_bucket"] = bool(embed_bucket)
        if inline is not None:
            kw["comm_inline"] = bool(inline)
        if captured is not None:
            kw["comm_events"] = not captured
            kw["graph_comm"] = bool(captured)
        if self.is_cuda:
            torch.cuda.synchronize(self.device)
        self.cfg = dataclasses.replace(self.cfg, **kw)
        self._build_buckets()
        if self.is_cuda and self.segmented:
            self.comm = None if self.cfg.comm_inline else self._comm_obj
        self._drop_capture(rewarm=True)
        self._graph_comm_failed = False

    def _snapshot_state(self):
        self.materialize_lazy()
        keys = ("flat_p", "flat_g", "flat_m", "flat_v", "rng", "step_ctr", "loss_ema", "loss_last", "lazy_decay")
        if self.flat_e is not None:
            keys += ("flat_e",)
        return {k: getattr(self, k).clone() for k in keys}, self.steps_done

    def _restore_state(self, snap):
        tensors, steps = snap
        for k, v in tensors.items():
            getattr(self, k).copy_(v)
        self.steps_done = steps
        self._lazy_dirty = False  # snapshots are taken materialized
        self._refresh_shadow()

    def autotune_comm(self, steps: int = 100, warm: int = 10, layouts=None, budget_s: Optional[float] = None):
        """Pick the gradient-exchange layout by measuring it on THIS job's ranks.

        Every layout of ``layouts`` (default :meth:`candidate_layouts`) runs
        ``graph_warmup`` eager steps, its capture and ``warm`` replayed steps, is
        checked, then timed over ``steps`` optimizer steps; the time is the max over
        ranks (so every rank takes the same decision) and the fastest layout is kept.
        Fail-fast, so the tuning can never eat the job's time limit:

        * a layout whose warm-up raised (a capture the RCCL build refuses) or whose
          counter hand-off timed out on ANY rank is dropped right after the warm-up
          (the timed-out wait raises the error word; every later wait then returns
          at once, so a broken layout costs one timeout, not one per bucket and step);
        * ``budget_s`` (default ``DDIM_COLD_AUTOTUNE_BUDGET_S``, 30 s) bounds the whole
          tuning: once spent (max over ranks), the remaining candidates are skipped;
        * if NO layout ran, the engine does not raise: it falls back to
          :meth:`fallback_eager_inline` (no graphs, no hand-offs, one all-reduce on the
          compute stream; on torch.distributed's communicator if ours fails too) and
          records the reason in :attr:`comm_fallback`.

        Parameters, Adam moments, counters, RNG and loss EMA are restored afterwards:
        the tuning steps leave no trace in the training state.  Returns
        ``{name: ms_per_step}`` (``inf``: failed, ``nan``: skipped for time; empty
        when not data parallel on a GPU).  Testing: ``DDIM_COLD_TEST_FAIL_LAYOUTS=1``
        makes every candidate fail after its warm-up."""
        if not (self.segmented and self.is_cuda and self.dist_on):
            return {}
        import time
        import warnings
        from ..parallel.dist import all_reduce_max, barrier
        from ..parallel.watchdog import phase
        if budget_s is None:
            budget_s = float(os.environ.get("DDIM_COLD_AUTOTUNE_BUDGET_S", "30"))
        force_fail = os.environ.get("DDIM_COLD_TEST_FAIL_LAYOUTS") == "1"
        layouts = list(layouts or self.candidate_layouts())
        snap = self._snapshot_state()
        times: Dict[str, float] = {}
        self.autotune_errors: Dict[str, str] = {}
        t_begin = time.perf_counter()
        for L in layouts:
            name = L[0]
            if all_reduce_max(time.perf_counter() - t_begin, self.device) > budget_s:
                times[name] = math.nan
                continue
            phase(f"autotune:{name}")
            failed = 0.0
            try:
                self.apply_layout(L)
                self.train_steps(self.cfg.graph_warmup + warm)
                if force_fail:
                    raise RuntimeError("DDIM_COLD_TEST_FAIL_LAYOUTS=1 (test hook)")
                torch.cuda.synchronize(self.device)
                if self.comm_error():
                    failed = 1.0
                    self.autotune_errors[name] = "hand-off wait timed out"
            except Exception as e:  # noqa: BLE001 - a candidate that cannot run is dropped, not fatal
                failed = 1.0
                self.autotune_errors[name] = repr(e)[:300]
                torch.cuda.synchronize(self.device)
            # every rank drops the layout if it failed on ANY rank; its stale-gradient
            # steps are undone by the state restore below
            if all_reduce_max(failed, self.device) > 0:
                times[name] = math.inf
                self.reset_comm_error()
                continue
            barrier()
            t0 = time.perf_counter()
            self.train_steps(steps)
            torch.cuda.synchronize(self.device)
            dt = time.perf_counter() - t0
            if self.comm_error():
                dt = math.inf
            times[name] = all_reduce_max(dt, self.device) / steps * 1e3
            self.reset_comm_error()
        ok = [L_ for L_ in layouts if math.isfinite(times[L_[0]])]
        self._restore_state(snap)
        for name, err in self.autotune_errors.items():
            warnings.warn(f"autotune_comm: layout {name} dropped ({err})")
        self.comm_times = times
        if not ok:
            warnings.warn(f"autotune_comm: no gradient-exchange layout ran ({times}); falling back to the "
                          "eager inline all-reduce")
            self.fallback_eager_inline(f"no layout ran: {sorted(self.autotune_errors)}")
        else:
            best = min(ok, key=lambda L_: times[L_[0]])
            self.apply_layout(best)
            phase("autotune:chosen", layout=best[0], ms=round(times[best[0]], 4))
        self.autotune_s = time.perf_counter() - t_begin
        return times

    def fallback_eager_inline(self, reason: str, verify_steps: int = 2):
        """Last-resort data-parallel step: no hipGraphs, no comm stream, no counter
        hand-offs -- forward + backward eagerly, then ONE all-reduce of the whole
        gradient arena on the compute stream, then the optimizer (the reference's
        DDP step minus the bucket overlap).  ``verify_steps`` eager steps are run on
        every rank (state restored afterwards); if they fail on any rank while our
        own RCCL communicator is in use, it is dropped for torch.distributed's and
        the check repeats.  Sets :attr:`comm_choice` = ``"eager-inline"`` and
        :attr:`comm_fallback` = ``reason``."""
        import dataclasses
        import warnings
        from ..parallel.dist import all_reduce_max
        from ..parallel.watchdog import phase
        phase("comm-fallback:eager-inline", reason=reason)
        self.set_comm_layout(1 << 16, False, True, captured=False)
        self.cfg = dataclasses.replace(self.cfg, use_graph=False)
        self.comm_choice = "eager-inline"
        self.comm_fallback = reason
        for attempt in range(2):
            snap = self._snapshot_state()
            failed, err = 0.0, None
            try:
                self.train_steps(verify_steps)
                if self.is_cuda:
                    torch.cuda.synchronize(self.device)
                if not bool(torch.isfinite(self.loss_last).all()):
                    failed, err = 1.0, "non-finite loss"
            except Exception as e:  # noqa: BLE001
                failed, err = 1.0, repr(e)[:300]
                if self.is_cuda:
                    torch.cuda.synchronize(self.device)
            self._restore_state(snap)
            if all_reduce_max(failed, self.device) == 0:
                phase("comm-fallback:verified", comm=self.comm_backend)
                return
            if attempt == 0 and self.ncomm is not None and self.dist_on:
                warnings.warn(f"eager inline fallback failed on the native communicator ({err}); "
                              "switching to torch.distributed")
                self.ncomm.destroy()
                self.ncomm = None
                self.comm_backend = "torch"
                self.comm_fallback = reason + "; native communicator dropped"
                continue
            break
        raise RuntimeError(f"data parallel: even the eager inline all-reduce step failed ({err}); {reason}")

    def _run_step(self):
        """One whole step issued on the current stream: eagerly, or inside the capture
        of a single step graph (the collectives then become graph nodes)."""
        for kind, k in self._step_iter():
            if kind == "bucket":
                self._allreduce(k)
                if k == len(self.bucketing.bounds) - 1:
                    self._join_comm()

    def _drop_capture(self, rewarm: bool):
        """Forget the captured step: its graphs, the K-step graph, the hand-off
        counters (``check_comm`` / ``comm_error`` then see none), ``handoff_order`` and the
        cached step plans.
        The next ``train_step`` re-captures, after ``graph_warmup`` fresh eager steps
        if ``rewarm``.  Nothing else clears these fields."""
        self._graphs = None
        self._mode = None
        self._multi = None
        self._signal = None
        self.handoff_order = None
        self._plans.clear()
        if rewarm:
            self._eager_steps = 0

    def _capture(self):
        """Capture the step in the mode the configuration resolves to and record the
        mode with the graphs; :meth:`_replay` dispatches on that record.  Captured
        collectives (``graph_comm``) that the RCCL build refuses fall back to
        per-bucket segments, for this and every later capture of the layout."""
        if not self.segmented:
            mode = SINGLE
        elif self.cfg.comm_events:
            mode = EVENT_SPLIT
        elif self.cfg.graph_comm and not self._graph_comm_failed:
            mode = SINGLE
        else:
            mode = SEGMENTS
        try:
            self._capture_as(mode)
        except Exception as e:  # pragma: no cover - depends on the RCCL build
            # a captured layout that was asked for (autotune candidate or explicit): its
            # failure must reach autotune_comm / the caller, not be timed as segments
            if not (self.segmented and mode == SINGLE) or (self.comm_choice or "").startswith("graph-"):
                raise
            import warnings
            warnings.warn(f"capturing collectives in the step graph failed ({e!r}); "
                          "falling back to per-bucket graph segments")
            self._graph_comm_failed = True
            torch.cuda.synchronize(self.device)
            self._capture_as(SEGMENTS)

    def _capture_as(self, mode: str):
        from ..utils.observe import drain_before_capture, no_gc
        if self.dist_on and self.is_cuda:
            # the warm-up's eager collectives finished on every rank (and dropped by
            # the process-group watchdog) before the capture opens
            drain_before_capture(self.device)
        multi = sig = order = None
        with no_gc():
            if mode == SINGLE:
                graphs, multi = self._capture_single()
            elif mode == EVENT_SPLIT:
                graphs, sig = self._capture_event_split()
                order = "inline" if sig is None else "pre-issued" if self._preissue_ok() else "post-replay"
            else:
                graphs = self._capture_segments()
        self._graphs, self._mode, self._multi, self._signal, self.handoff_order = graphs, mode, multi, sig, order

    def _capture_event_split(self):
        """Compute graph (forward + backward) + optimizer graph; see
        ``EngineConfig.comm_events``.  With a comm stream the compute graph tells it a
        bucket is final by bumping a per-bucket counter (a 1-lane kernel node,
        system-scope release) that a bounded polling kernel on the comm stream waits
        for.  Inline layout (no comm stream): the boundaries leave nothing in the graph."""
        from ..parallel.comm import FlagSignal
        pool = torch.cuda.graph_pool_handle()
        nb = len(self.bucketing.bounds)
        sig = FlagSignal(nb, self.device) if self.comm is not None else None
        gen = self._step_iter()
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(g1, pool=pool, capture_error_mode=CAPTURE_MODE):
            for _ in range(nb):
                kind, k = next(gen)
                assert kind == "bucket", kind
                if sig is not None:
                    sig.bump(k)
        with torch.cuda.graph(g2, pool=pool, capture_error_mode=CAPTURE_MODE):
            kind, _ = next(gen)
            assert kind == "done", kind
        return [g1, g2], sig

    def _capture_single(self):
        """The whole step as one graph, plus ``graph_steps`` = K > 1 steps as another."""
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=torch.cuda.graph_pool_handle(), capture_error_mode=CAPTURE_MODE):
            self._run_step()
        multi = None
        K = max(1, int(self.cfg.graph_steps))
        if K > 1:  # K steps in one graph, own memory pool
            gm = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gm, pool=torch.cuda.graph_pool_handle(), capture_error_mode=CAPTURE_MODE):
                for _ in range(K):
                    self._run_step()
            multi = (gm, K)
        return [g], multi

    def _capture_segments(self):
        """One graph up to each bucket boundary and one for the optimizer."""
        pool = torch.cuda.graph_pool_handle()
        gen = self._step_iter()
        graphs = []
        for _ in range(len(self.bucketing.bounds) + 1):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, capture_error_mode=CAPTURE_MODE):
                next(gen)
            graphs.append(g)
        return graphs

    def _replay(self):
        gs, nb = self._graphs, len(self.bucketing.bounds)
        if self._mode == SINGLE:
            gs[0].replay()
        elif self._mode == EVENT_SPLIT:
            sig = self._signal
            if sig is not None:
                sig.expected += 1  # this replay's counter value
            # pre-issued: the comm stream's counter waits + collectives are queued BEFORE
            # the compute graph (each waits for its own counter), so the comm queue holds
            # them when the graph starts instead of receiving them behind it
            pre = self.handoff_order == "pre-issued"
            if not pre:
                gs[0].replay()
            for k in range(nb):  # comm stream: behind the bucket's counter; inline: after gs[0]
                self._allreduce(k, wait_counter=sig is not None)
            if pre:
                gs[0].replay()
            self._join_comm()
            gs[1].replay()
        else:
            for k in range(nb):
                gs[k].replay()
                self._allreduce(k)
            self._join_comm()
            gs[nb].replay()

    def train_steps(self, n: int, materialize: bool = True):
        """Run ``n`` optimizer steps (``batch_fn`` draws each step's batch on the device).
        With ``graph_steps = K > 1`` every run of K steps is ONE replay of a K-step
        graph; the remainder (and the eager warm-up) goes through :meth:`train_step`.
        ``materialize``: apply the lazily accumulated weight decay afterwards (see
        ``lazy``), so every parameter is current when the call returns.
        Returns the device loss tensor of the last step (no host sync)."""
        self._no_ema_scope("train_steps")
        done = 0
        while done < n:
            multi = self._multi
            if multi is not None and n - done >= multi[1]:
                multi[0].replay()
                self.steps_done += multi[1]
                self._lazy_dirty = True
                done += multi[1]
            else:
                self.train_step(materialize=False)
                done += 1
        if materialize:
            self.materialize_lazy()
        return self.loss_last

    def materialize_lazy(self):
        """Apply the weight decay accumulated for the ``lazy`` rows since the last call
        (p *= prod(1 - lr_s wd); their moments are zero) and refresh their bf16 shadow."""
        if self.lazy is None or not self._lazy_dirty:
            return
        lo, hi = self.lazy
        self.flat_p[lo:hi].mul_(self.lazy_decay)
        self.flat_pb[lo:hi].copy_(self.flat_p[lo:hi])
        self.lazy_decay.fill_(1.0)
        self._lazy_dirty = False

    def train_step(self, materialize: bool = True):
        """Run one optimizer step on the batch produced by ``batch_fn``
        (``materialize``: as in :meth:`train_steps`; the trainer defers it to the
        epoch end, where it evaluates and checkpoints).

        Returns the device loss tensor (no host sync)."""
        self._no_ema_scope("train_step")
        if self.batch_fn is None:
            raise RuntimeError("set_batch_fn() or use step(x, target, t)")
        use_graph = self.cfg.use_graph and self.is_cuda
        if use_graph and self._graphs is None and self._eager_steps >= self.cfg.graph_warmup:
            self._capture()
        if use_graph and self._graphs is not None:
            self._replay()
        else:
            self._run_step()
            self._eager_steps += 1
        self.steps_done += 1
        self._lazy_dirty = True
        if materialize:
            self.materialize_lazy()
        return self.loss_last

    def step(self, x_t: torch.Tensor, target: torch.Tensor, t: torch.Tensor):
        """Convenience: copy an externally produced batch into static buffers and step."""
        self._no_ema_scope("step")
        if self._static is None or self._static[0].shape != x_t.shape:
            self._static = (torch.empty_like(x_t, device=self.device), torch.empty_like(target, device=self.device),
                            torch.empty(t.shape, dtype=torch.int64, device=self.device))
            st = self._static
            self.set_batch_fn(lambda: st)
        sx, sy, st_ = self._static
        sx.copy_(x_t, non_blocking=True)
        sy.copy_(target, non_blocking=True)
        st_.copy_(t, non_blocking=True)
        return self.train_step()

    # ------------------------------------------------------------------ weight EMA
    def _no_ema_scope(self, what: str):
        if self._ema_scope:
            raise RuntimeError(f"{what}() inside ema_weights(): the parameter arena holds the EMA weights; "
                               "leave the scope before training")

    def _need_ema(self, what: str):
        if self.flat_e is None:
            raise RuntimeError(f"{what}: this engine keeps no weight EMA (EngineConfig.weight_ema is 0)")

    def _swap_ema(self):
        """Exchange the contents of the parameter and EMA arenas (no address changes, so
        every captured graph stays valid) and re-derive what the kernels read."""
        if self._ema_tmp is None:
            self._ema_tmp = torch.empty_like(self.flat_p)
        self._ema_tmp.copy_(self.flat_p)
        self.flat_p.copy_(self.flat_e)
        self.flat_e.copy_(self._ema_tmp)
        self._refresh_shadow()

    @contextlib.contextmanager
    def ema_weights(self):
        """Scope in which the model runs on its EMA weights: ``model``,
        ``param_tensors``, ``trainer.evaluate`` and every sampler see them (bf16 shadow,
        LayerNorm fold and transposed shadows re-derived); on exit the arenas are
        swapped back, bitwise what they were.  Training inside the scope raises; the
        scope is not re-entrant."""
        self._need_ema("ema_weights()")
        if self._ema_scope:
            raise RuntimeError("ema_weights() is not re-entrant")
        self._swap_ema()
        self._ema_scope = True
        try:
            yield self
        finally:
            self._swap_ema()
            self._ema_scope = False

    def _arena_state_dict(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        """The model's ``state_dict`` (keys, shapes, order) read from an arena."""
        lay = self.layout
        shapes = dict(zip(lay.names, lay.shapes))
        out = {}
        for n in self.model.state_dict().keys():
            if n not in lay.offsets:
                raise KeyError(f"{n}: not in the parameter arena (a buffer?)")
            o, k = lay.offsets[n]
            out[n] = flat[o:o + k].view(shapes[n]).clone()
        return out

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The EMA weights as the model's ``state_dict`` (keys, shapes, order)."""
        self._need_ema("ema_state_dict()")
        return self._arena_state_dict(self.flat_p if self._ema_scope else self.flat_e)

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]):
        """Restore the EMA arena from a ``state_dict`` of the model's keys (strict)."""
        self._need_ema("load_ema_state_dict()")
        self._no_ema_scope("load_ema_state_dict")
        have = set(self.layout.names)
        if set(sd) != have:
            raise KeyError(f"EMA state dict keys differ from the model's: missing "
                           f"{sorted(have - set(sd))}, unexpected {sorted(set(sd) - have)}")
        for n, (o, k) in self.layout.offsets.items():
            self.flat_e[o:o + k].copy_(sd[n].reshape(-1).to(self.device, torch.float32))

    # ------------------------------------------------------------------ state
    def current_lr(self) -> float:
        return self._lr_at(int(self.step_ctr[1].item()))

    def _param_list(self):
        return [p for _, p in self.model.named_parameters()]

    def optimizer_state_dict(self) -> dict:
        """torch.optim.AdamW-format state dict (interchangeable with the reference's lastepoch.pkl)."""
        self.materialize_lazy()
        ctr = self.step_ctr.detach().cpu()
        return self._optimizer_sd(self.flat_m, self.flat_v, int(ctr[0]), int(ctr[1]))

    def _lr_at(self, sched_step: int) -> float:
        c = self.cfg
        if c.t_max <= 0:
            return c.lr
        return c.eta_min + (c.lr - c.eta_min) * 0.5 * (1 + math.cos(math.pi * sched_step / c.t_max))

    def _optimizer_sd(self, flat_m: torch.Tensor, flat_v: torch.Tensor, adam_step: int, sched_step: int) -> dict:
        """AdamW state dict from moment arenas (the live device ones, or a host snapshot)."""
        params = self._param_list()
        opt = torch.optim.AdamW(params, lr=self._lr_at(sched_step), betas=self.cfg.betas, eps=self.cfg.eps,
                                weight_decay=self.cfg.weight_decay)
        lay = self.layout
        if adam_step > 0:
            for n, shape, p in zip(lay.names, lay.shapes, params):
                if n in lay.frozen:  # torch.optim keeps no state for a parameter without .grad
                    continue
                o, k = lay.offsets[n]
                opt.state[p] = {"step": torch.tensor(float(adam_step)),
                                "exp_avg": flat_m[o:o + k].view(shape).clone(),
                                "exp_avg_sq": flat_v[o:o + k].view(shape).clone()}
        sd = opt.state_dict()
        sd["param_groups"][0]["initial_lr"] = self.cfg.lr
        return sd

    def snapshot_to_host(self) -> "HostSnapshot":
        """Training state (parameters, Adam moments, counters) for an off-critical-path
        checkpoint write: device-to-device copies into snapshot buffers on the CURRENT
        stream (ordered after the last step, ~90 MB at HBM speed for ViT-tiny), then
        device-to-host copies into pinned buffers on a side stream that the training
        stream never waits for.  ``HostSnapshot.wait()`` (the writer thread) blocks
        until the host copy has landed.  The buffers are reused: finish (wait) one
        snapshot before taking the next."""
        self.materialize_lazy()
        cur = torch.cuda.current_stream(self.device) if self.is_cuda else None
        src = (self.flat_p, self.flat_m, self.flat_v, self.step_ctr, self.rng)
        if self.flat_e is not None:  # the weight EMA rides along as a sixth buffer
            self._no_ema_scope("snapshot_to_host")
            src += (self.flat_e,)
        if self._snap is None:
            host = [torch.empty(t.shape, dtype=t.dtype, pin_memory=self.is_cuda) for t in src]
            dev = [torch.empty_like(t) for t in src] if self.is_cuda else None
            side = torch.cuda.Stream(self.device) if self.is_cuda else None
            self._snap = (host, dev, side)
        host, dev, side = self._snap
        ev = None
        if self.is_cuda:
            for d, t in zip(dev, src):
                d.copy_(t)
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for h, d in zip(host, dev):
                    h.copy_(d, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
        else:
            for h, t in zip(host, src):
                h.copy_(t)
        return HostSnapshot(self, *host[:5], ev, int(self.steps_done), ema=host[5] if len(host) > 5 else None)

    def load_optimizer_state_dict(self, sd: dict):
        st = sd.get("state", {})
        lay = self.layout
        step = 0
        for i, n in enumerate(lay.names):
            s = st.get(i)
            if s is None or n in lay.frozen:
                continue
            o, k = lay.offsets[n]
            self.flat_m[o:o + k].copy_(s["exp_avg"].reshape(-1).to(self.device))
            self.flat_v[o:o + k].copy_(s["exp_avg_sq"].reshape(-1).to(self.device))
            step = int(float(s["step"]))
        self.step_ctr[0] = step
        self._check_lazy_moments()

    def _check_lazy_moments(self):
        """The lazy time_embed rows assume zero Adam moments for the whole run.  A
        resumed state whose moments are non-zero there (a Gaussian-diffusion run, a
        different image size / ``temb_rows``) turns the shortcut off, so those rows
        keep moving as torch.optim.AdamW would move them."""
        if self.lazy is None:
            return
        lo, hi = self.lazy
        if bool(self.flat_m[lo:hi].any()) or bool(self.flat_v[lo:hi].any()):
            import warnings
            warnings.warn("optimizer state has non-zero Adam moments on time_embed rows this run cannot "
                          "select; updating them every step (lazy weight decay off)")
            self.materialize_lazy()
            self.lazy = None
            self._drop_capture(rewarm=True)

    def scheduler_state_dict(self, sched_step: Optional[int] = None) -> dict:
        """torch CosineAnnealingLR-format state dict (at ``sched_step``, default: now).
        The key layout comes from a real scheduler built once and cached (building a
        torch optimizer costs ~1.5 s the first time in a process -- it imports the
        compiler stack -- which must not land in a background checkpoint write)."""
        if self._sched_template is None:
            opt = torch.optim.AdamW([torch.zeros(1, requires_grad=True)], lr=self.cfg.lr)
            sch = torch.optim.lr_scheduler.CosineAnnealingLR(opt, max(self.cfg.t_max, 1), self.cfg.eta_min)
            self._sched_template = sch.state_dict()
        sd = copy.deepcopy(self._sched_template)
        sd["base_lrs"] = [self.cfg.lr]
        last = int(self.step_ctr[1].item()) if sched_step is None else int(sched_step)
        sd["last_epoch"] = last
        sd["_step_count"] = last + 1
        sd["_last_lr"] = [self._lr_at(last)]
        return sd

    def load_scheduler_state_dict(self, sd: dict):
        self.step_ctr[1] = int(sd.get("last_epoch", 0))

    def sync_params_from_model(self):
        """Call after loading weights into ``model`` (its params are arena views)."""
        self.lazy_decay.fill_(1.0)  # the loaded values are current: no decay pending
        self._lazy_dirty = False
        if self.flat_e is not None:  # the EMA restarts from the loaded weights
            self._no_ema_scope("sync_params_from_model")
            self.flat_e.copy_(self.flat_p)
        self._refresh_shadow()

    def detach(self):
        """Release the model from the engine (params stay on the device, as plain tensors).
        The EMA arena stays readable (``ema_state_dict``); the swap's temp arena is freed."""
        self._no_ema_scope("detach")
        self._ema_tmp = None
        self.materialize_lazy()
        for n, p in self.model.named_parameters():
            p.data = p.data.clone()
            p.grad = None
        self.model._engine = None


class HostSnapshot:
    """Host copy of an engine's training state (:meth:`TrainEngine.snapshot_to_host`):
    fp32 parameter / moment arenas, counters and RNG state, plus what is needed to
    lay them out as the reference's checkpoint dicts without touching the device."""

    def __init__(self, engine: TrainEngine, p, m, v, step_ctr, rng, event, steps_done: int, ema=None):
        self.engine, self.p, self.m, self.v, self.step_ctr, self.rng = engine, p, m, v, step_ctr, rng
        self.ema = ema  # host copy of the weight EMA arena; None when the engine keeps none
        self.event = event
        self.steps_done = steps_done

    def wait(self):
        if self.event is not None:
            self.event.synchronize()

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The model's ``state_dict`` (parameter order and shapes) from the snapshot."""
        return self.engine._arena_state_dict(self.p)

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The EMA weights as the model's ``state_dict``, from the snapshot."""
        if self.ema is None:
            raise RuntimeError("this snapshot holds no weight EMA (EngineConfig.weight_ema is 0)")
        return self.engine._arena_state_dict(self.ema)

    def optimizer_state_dict(self) -> dict:
        return self.engine._optimizer_sd(self.m, self.v, int(self.step_ctr[0]), int(self.step_ctr[1]))

    def scheduler_state_dict(self) -> dict:
        return self.engine.scheduler_state_dict(int(self.step_ctr[1]))
