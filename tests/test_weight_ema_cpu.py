"""Weight EMA on the CPU: the optimizer op's three-operation update and warm-up ramp,
the engine's EMA arena / swap scope, checkpoints and resume, the trainer's files and
``ema_eval``, 2-rank gloo data parallel, and the sampling CLI's ``--ema``."""
import dataclasses
import os
import subprocess
import sys
import tempfile
from fractions import Fraction

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from ddim_cold_amd import ops
from ddim_cold_amd.config import ExperimentConfig, load_config
from ddim_cold_amd.models import DiffusionVisionTransformer
from ddim_cold_amd.parallel.dist import free_port
from ddim_cold_amd.train import checkpoint as ckpt
from ddim_cold_amd.train.engine import EngineConfig, TrainEngine
from ddim_cold_amd.train.trainer import Paths, evaluate, launch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = dict(img_size=[16, 16], patch_size=4, embed_dim=32, depth=2, num_heads=2)
HYPER = [3e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, 10.0, 0.0]


# ------------------------------------------------------------------ op
def _arenas(n, seed=0, t=0):
    g = torch.Generator().manual_seed(seed)
    p, e, gr = (torch.randn(n, generator=g) for _ in range(3))
    m = torch.randn(n, generator=g) * 0.01
    v = torch.rand(n, generator=g) * 1e-3
    sq = torch.zeros(ops.SQ_PARTS)
    sq[0] = gr.pow(2).sum()
    return dict(p=p, g=gr, m=m, v=v, e=e, pb=torch.zeros(n, dtype=torch.bfloat16), sq=sq,
                step=torch.tensor([t, t], dtype=torch.int64), hyper=torch.tensor(HYPER))


def _call(a, **kw):
    a = {k: v.clone() for k, v in a.items()}
    ops.adamw_step(a["p"], a["g"], a["m"], a["v"], a["pb"], a["sq"], a["step"], a["hyper"], 1.0, **kw)
    return a


def test_op_three_operation_update_and_untouched_adamw():
    a0 = _arenas(1027)
    plain = _call(a0)
    a = {k: v.clone() for k, v in a0.items()}
    ops.adamw_step(a["p"], a["g"], a["m"], a["v"], a["pb"], a["sq"], a["step"], a["hyper"], 1.0,
                   ema=a["e"], ema_decay=0.9, ema_warmup=False)
    d32 = torch.tensor(0.9, dtype=torch.float32)
    assert torch.equal(a["e"], a["p"] + d32 * (a0["e"] - a["p"]))
    assert not torch.equal(a["e"], a0["e"])
    for k in ("p", "m", "v", "g", "pb"):
        assert torch.equal(a[k], plain[k]), k


def test_op_skipped_step_and_lazy():
    a0 = _arenas(260)
    a0["sq"][3] = float("inf")
    a = {k: v.clone() for k, v in a0.items()}
    ops.adamw_step(a["p"], a["g"], a["m"], a["v"], None, a["sq"], a["step"], a["hyper"], 1.0,
                   ema=a["e"], ema_decay=0.9)
    assert torch.equal(a["e"], a0["e"]) and torch.equal(a["p"], a0["p"]) and torch.all(a["g"] == 0)
    a = _arenas(260)
    with pytest.raises(RuntimeError, match="lazy"):
        ops.adamw_step(a["p"], a["g"], a["m"], a["v"], None, a["sq"], a["step"], a["hyper"], 1.0,
                       lazy=(64, 128), lazy_decay=torch.ones(1), ema=a["e"], ema_decay=0.9)
    with pytest.raises(RuntimeError, match="ema_decay"):
        ops.adamw_step(a["p"], a["g"], a["m"], a["v"], None, a["sq"], a["step"], a["hyper"], 1.0,
                       ema=a["e"], ema_decay=1.0)


@pytest.mark.parametrize("t", [0, 1, 90, 10 ** 6])
def test_warmup_decay(t):
    decay = 0.9999
    want = torch.minimum(torch.tensor(decay, dtype=torch.float32),
                         torch.tensor(1.0 + t, dtype=torch.float32) / torch.tensor(10.0 + t, dtype=torch.float32))
    assert torch.equal(ops.weight_ema_decay(decay, t, True), want)
    assert float(want) == pytest.approx(min(decay, (1 + t) / (10 + t)), rel=1e-6)
    assert torch.equal(ops.weight_ema_decay(decay, t, False), torch.tensor(decay, dtype=torch.float32))
    # the op uses it: e <- p + d (e - p) with d read from step[0]
    a0 = _arenas(37, t=t)
    a = {k: v.clone() for k, v in a0.items()}
    ops.adamw_step(a["p"], a["g"], a["m"], a["v"], None, a["sq"], a["step"], a["hyper"], 1.0,
                   ema=a["e"], ema_decay=decay, ema_warmup=True)
    assert torch.equal(a["e"], a["p"] + want * (a0["e"] - a["p"]))


def test_warmup_hands_over_to_decay_at_89991():
    decay = Fraction(9999, 10000)
    ramp = lambda t: Fraction(1 + t, 10 + t)  # noqa: E731
    assert ramp(89_990) == decay and ramp(89_991) > decay and ramp(89_989) < decay
    d32 = torch.tensor(0.9999, dtype=torch.float32)
    assert float(ops.weight_ema_decay(0.9999, 0, True)) == pytest.approx(0.1)
    assert ops.weight_ema_decay(0.9999, 80_000, True) < d32
    for t in (89_991, 89_992, 100_000, 10 ** 7):
        assert torch.equal(ops.weight_ema_decay(0.9999, t, True), d32), t


# ------------------------------------------------------------------ engine
def _model(seed=0):
    torch.manual_seed(seed)
    return DiffusionVisionTransformer(**CFG, drop_rate=0.1, attn_drop_rate=0.1, drop_path_rate=0.1).train()


def _batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, 16, 16, generator=g)
    y = torch.randn(B, 3, 16, 16, generator=g).clamp(-1, 1)
    return x, y, torch.randint(1, 5, (B,), generator=g)


def _engine(weight_ema=0.9, temb_rows=7, seed=0, **kw):
    return TrainEngine(_model(seed), EngineConfig(lr=1e-3, t_max=20, seed=11, weight_ema=weight_ema,
                                                  temb_rows=temb_rows, **kw), device="cpu")


def test_engine_ema_follows_hand_loop_and_leaves_training_alone():
    eng = _engine(0.9)
    off = _engine(0.0, temb_rows=None)
    assert eng.lazy is None and off.lazy is None and off.flat_e is None
    assert _engine(0.0).lazy is not None  # the same rows ARE lazy without the EMA
    e = eng.flat_p.clone()
    assert torch.equal(eng.flat_e, e) and eng.flat_e.data_ptr() != eng.flat_p.data_ptr()
    th = eng.layout.train_hi
    for s in range(6):
        eng.step(*_batch(4, s))
        off.step(*_batch(4, s))
        d = ops.weight_ema_decay(0.9, s, True)
        e[:th] = eng.flat_p[:th] + d * (e[:th] - eng.flat_p[:th])
        assert torch.equal(eng.flat_e, e), s
        assert torch.equal(eng.flat_p, off.flat_p), s
    assert not torch.equal(eng.flat_e, eng.flat_p)
    # no warm-up: the constant decay from the first step
    eng2 = _engine(0.9, weight_ema_warmup=False)
    e = eng2.flat_p.clone()
    eng2.step(*_batch(4, 0))
    assert torch.equal(eng2.flat_e[:th], eng2.flat_p[:th] + torch.tensor(0.9) * (e[:th] - eng2.flat_p[:th]))
    with pytest.raises(ValueError, match="weight_ema"):
        _engine(1.0)


def test_ema_scope():
    eng = _engine(0.9)
    model = eng.model
    for s in range(3):
        eng.step(*_batch(4, s))
    p0, e0 = eng.flat_p.clone(), eng.flat_e.clone()
    pb0 = eng.flat_pb.clone()
    want = eng.ema_state_dict()
    assert list(want) == list(model.state_dict()) and all(want[k].shape == v.shape
                                                          for k, v in model.state_dict().items())
    with eng.ema_weights():
        sd = model.state_dict()
        assert all(torch.equal(sd[k], want[k]) for k in want)
        assert all(torch.equal(eng.ema_state_dict()[k], want[k]) for k in want)
        assert torch.equal(eng.flat_pb, e0.to(torch.bfloat16))  # derived tensors follow
        with pytest.raises(RuntimeError, match="ema_weights"):
            eng.train_step()
        with pytest.raises(RuntimeError, match="ema_weights"):
            eng.train_steps(2)
        with pytest.raises(RuntimeError, match="ema_weights"):
            eng.step(*_batch(4, 9))
        with pytest.raises(RuntimeError, match="re-entrant"):
            with eng.ema_weights():
                pass
    assert torch.equal(eng.flat_p, p0) and torch.equal(eng.flat_e, e0) and torch.equal(eng.flat_pb, pb0)
    tmp = eng._ema_tmp
    with eng.ema_weights():
        pass
    assert eng._ema_tmp is tmp  # one reusable temp arena
    eng.step(*_batch(4, 3))  # training goes on after the scope
    with pytest.raises(RuntimeError, match="weight_ema"):
        with _engine(0.0).ema_weights():
            pass
    with pytest.raises(RuntimeError, match="weight_ema"):
        _engine(0.0).ema_state_dict()
    # loading weights restarts the EMA from them; detach leaves the model on plain tensors
    model.load_state_dict({k: v + 1 for k, v in model.state_dict().items()})
    eng.sync_params_from_model()
    assert torch.equal(eng.flat_e, eng.flat_p)
    eng.detach()
    assert model._engine is None and eng._ema_tmp is None
    assert all(p.data_ptr() != eng.flat_p[o:].data_ptr() for (n, p), (o, _) in
               zip(model.named_parameters(), (eng.layout.offsets[n] for n, _ in model.named_parameters())))


def test_snapshot_and_autotune_state_hold_the_ema():
    eng = _engine(0.9)
    for s in range(2):
        eng.step(*_batch(4, s))
    snap = eng.snapshot_to_host()
    snap.wait()
    sd, want = snap.ema_state_dict(), eng.ema_state_dict()
    assert list(sd) == list(want) and all(torch.equal(sd[k], want[k]) for k in want)
    bufs = eng._snap[0]
    snap2 = eng.snapshot_to_host()
    assert snap2.ema is snap.ema and eng._snap[0] is bufs and len(bufs) == 6
    off = _engine(0.0)
    s_off = off.snapshot_to_host()
    assert s_off.ema is None and len(off._snap[0]) == 5
    with pytest.raises(RuntimeError, match="weight EMA"):
        s_off.ema_state_dict()
    st = eng._snapshot_state()
    e0 = eng.flat_e.clone()
    eng.step(*_batch(4, 5))
    assert not torch.equal(eng.flat_e, e0)
    eng._restore_state(st)
    assert torch.equal(eng.flat_e, e0)


# ------------------------------------------------------------------ checkpoints
LASTEPOCH_KEYS = {"epoch", "steps", "loss_rec", "metric", "state_dict", "scheduler", "optimizer", "rng",
                  "engine_steps", "scaler"}


def test_lastepoch_keys_and_bitwise_resume(tmp_path):
    path = str(tmp_path / "lastepoch.pkl")
    eng = _engine(0.9)
    for s in range(3):
        eng.step(*_batch(4, s))
    ckpt.save_lastepoch(path, eng.model, eng, 0, 3, 1.0, 1.0)
    d = torch.load(path, weights_only=True)
    assert set(d) == LASTEPOCH_KEYS | {"ema_state_dict", "ema"}
    assert list(d["ema_state_dict"]) == list(d["state_dict"])
    assert all(k.startswith("module.") for k in d["ema_state_dict"])
    assert d["ema"] == {"decay": 0.9, "warmup": True}
    want = eng.ema_state_dict()
    assert all(torch.equal(d["ema_state_dict"]["module." + k], want[k]) for k in want)
    for s in range(3, 6):
        eng.step(*_batch(4, s))
    res = _engine(0.9, seed=5)  # other initial weights: everything comes from the file
    ckpt.load_lastepoch(path, res.model, res)
    for s in range(3, 6):
        res.step(*_batch(4, s))
    assert torch.equal(res.flat_p, eng.flat_p) and torch.equal(res.flat_e, eng.flat_e)
    # an engine without EMA ignores the key
    off = _engine(0.0, seed=5)
    ckpt.load_lastepoch(path, off.model, off)
    assert off.flat_e is None
    # load_weights(ema=True): strict, the EMA weights
    m = _model(3)
    missing, unexpected = ckpt.load_weights(m, path, strict=True, ema=True)
    assert not missing and not unexpected
    assert all(torch.equal(v, d["ema_state_dict"]["module." + k]) for k, v in m.state_dict().items())


def test_old_file_without_ema_key(tmp_path):
    path = str(tmp_path / "lastepoch.pkl")
    old = _engine(0.0)
    for s in range(2):
        old.step(*_batch(4, s))
    ckpt.save_lastepoch(path, old.model, old, 0, 2, 1.0, 1.0)
    assert set(torch.load(path, weights_only=True)) == LASTEPOCH_KEYS  # exactly today's keys
    eng = _engine(0.9, seed=5)
    with pytest.warns(UserWarning, match="ema_state_dict") as rec:
        ckpt.load_lastepoch(path, eng.model, eng)
    assert len([w for w in rec if "ema_state_dict" in str(w.message)]) == 1
    old.materialize_lazy()
    assert torch.equal(eng.flat_p, old.flat_p) and torch.equal(eng.flat_e, eng.flat_p)
    with pytest.raises(KeyError, match="ema_state_dict"):
        ckpt.load_weights(_model(), path, strict=True, ema=True)


# ------------------------------------------------------------------ trainer
def _yaml_cfg(tmp, **kw):
    cfg = load_config(os.path.join(ROOT, "configs", "synthetic_tiny.yaml"))
    return dataclasses.replace(cfg, ckpt_dir=str(tmp / "Saved_Models"), synthetic_size=64, max_steps=2,
                               epoch=[0, 1], graph=False, **kw).validate()


@pytest.fixture(scope="module")
def ema_run(tmp_path_factory):
    """configs/synthetic_tiny.yaml plus ``weight_ema: 0.99``, cut to one 2-step epoch."""
    tmp = tmp_path_factory.mktemp("ema_run")
    cfg = _yaml_cfg(tmp, weight_ema=0.99)
    paths = Paths.make(cfg, "ema", root=str(tmp))
    launch(cfg, "ema", paths, backend="gloo")
    return paths.ckpt_dir


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("plain_run")
    cfg = _yaml_cfg(tmp)
    paths = Paths.make(cfg, "plain", root=str(tmp))
    launch(cfg, "plain", paths, backend="gloo")
    return paths.ckpt_dir


def test_trainer_writes_bestloss_ema(ema_run, plain_run):
    from ddim_cold_amd import build_model
    best = os.path.join(ema_run, "bestloss_ema.pkl")
    assert os.path.isfile(best) and os.path.isfile(os.path.join(ema_run, "bestloss.pkl"))
    m = build_model("vit_tiny")
    missing, unexpected = ckpt.load_weights(m, best, strict=True)
    assert not missing and not unexpected
    last = torch.load(os.path.join(ema_run, "lastepoch.pkl"), weights_only=True)
    sd = torch.load(best, weights_only=True)
    assert not any(k.startswith("module.") for k in sd)
    assert all(torch.equal(sd[k], last["ema_state_dict"]["module." + k]) for k in sd)
    assert any(not torch.equal(sd[k], last["state_dict"]["module." + k]) for k in sd)
    assert last["ema"] == {"decay": 0.99, "warmup": True}
    assert not any("ema" in f for f in os.listdir(plain_run))
    assert set(torch.load(os.path.join(plain_run, "lastepoch.pkl"), weights_only=True)) == LASTEPOCH_KEYS


def _small_cfg(tmp, **kw):
    base = dict(initializing="init.pkl", framework="_ema", num_gpus=1, batch_size=4, epoch=[0, 1],
                image_size=[16, 16], patch_size=4, embed_dim=32, depth=2, head=2, synthetic=True,
                synthetic_size=64, log_every=2, graph=False, ckpt_dir=str(tmp / "Saved_Models"))
    base.update(kw)
    return ExperimentConfig(**base).validate()


def test_ema_eval_logs_the_ema_weights_metric(tmp_path):
    from ddim_cold_amd.data.datasets import shard_indices
    from ddim_cold_amd.data.synthetic import synthetic_pool
    cfg = _small_cfg(tmp_path, weight_ema=0.9, ema_eval=True)
    paths = Paths.make(cfg, "ev", root=str(tmp_path))
    res = launch(cfg, "ev", paths, backend="gloo")
    (epoch, logged), = res["history"]
    # by hand: the run's final state into a fresh engine, evaluate inside / outside the scope
    model = DiffusionVisionTransformer(**cfg.model_kwargs())
    eng = TrainEngine(model, EngineConfig(weight_ema=0.9, temb_rows=5), device="cpu")
    ckpt.load_lastepoch(os.path.join(paths.ckpt_dir, "lastepoch.pkl"), model, eng)
    model.eval()
    val = synthetic_pool(64 // 8, (16, 16), seed=cfg.seed + 1, device="cpu")
    vidx = shard_indices(val.shape[0], 1, 0, epoch, cfg.seed, shuffle=False, drop_last=False)

    def ev():
        rng = torch.tensor([cfg.seed + 7919, epoch * 1], dtype=torch.int64)
        return evaluate(model, eng, val, vidx, cfg.per_gpu_batch, cfg.dataset, cfg.model_total_steps, rng)
    raw = ev()
    with eng.ema_weights():
        on_ema = ev()
    assert logged == on_ema and raw != on_ema
    assert res["best_loss"] == on_ema  # the bestloss decision refers to it too


def test_config_validation():
    with pytest.raises(ValueError, match="weight_ema"):
        ExperimentConfig(synthetic=True, weight_ema=1.0).validate()
    with pytest.raises(ValueError, match="weight_ema"):
        ExperimentConfig(synthetic=True, weight_ema=-0.1).validate()
    with pytest.raises(ValueError, match="ema_eval"):
        ExperimentConfig(synthetic=True, ema_eval=True).validate()
    c = ExperimentConfig(synthetic=True, weight_ema=0.999, ema_eval=True).validate()
    assert c.weight_ema_warmup is True
    d = ExperimentConfig(synthetic=True)
    assert (d.weight_ema, d.weight_ema_warmup, d.ema_eval) == (0.0, True, False)


# ------------------------------------------------------------------ data parallel
def _dp_worker(rank, world, port, out_path):
    import test_dp_world_cpu as dpw
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        eng = _dp_engine(dpw, seed=rank)  # different init per rank: rank 0's is broadcast
        assert torch.equal(eng.flat_e, eng.flat_p)  # taken after the broadcast
        b = dpw.GB // world
        x, y, t = dpw._batch(False)
        sl = slice(rank * b, (rank + 1) * b)
        for _ in range(2):
            eng.step(x[sl], y[sl], t[sl])
        es = [torch.zeros_like(eng.flat_e) for _ in range(world)]
        dist.all_gather(es, eng.flat_e.clone())
        if rank == 0:
            torch.save({"e": es, "p": eng.flat_p.clone()}, out_path)
    finally:
        dist.destroy_process_group()


def _dp_engine(dpw, seed):
    return TrainEngine(dpw._model(seed), EngineConfig(lr=1e-3, weight_decay=0.0, max_grad_norm=0.0, temb_rows=7,
                                                      weight_ema=0.9), device="cpu")


def test_data_parallel_two_ranks_share_one_ema():
    import test_dp_world_cpu as dpw
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "r.pt")
        mp.start_processes(_dp_worker, args=(2, free_port(), out), nprocs=2, join=True, start_method="spawn")
        res = torch.load(out, weights_only=True)
    assert torch.equal(res["e"][0], res["e"][1])
    assert not torch.equal(res["e"][0], res["p"])
    one = _dp_engine(dpw, seed=0)  # the single-process run on the concatenated batch
    for _ in range(2):
        one.step(*dpw._batch(False))
    # the parity tests' fp32 bound: the all-reduce sums the two halves in another order
    init = _dp_engine(dpw, seed=0).flat_p
    moved = (one.flat_e - init).abs().max().item()
    assert moved > 0 and (res["e"][0] - one.flat_e).abs().max().item() <= 1e-4 * max(moved, 1e-3) + 1e-7


# ------------------------------------------------------------------ CLI
def _vit_cli(args, out):
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    return subprocess.run([sys.executable, os.path.join(ROOT, "ViT.py"), "--model", "vit_tiny", "--sample_n", "1",
                           "--acc_k", "1000", "--seq_n", "1", "--seq_k", "1000", "--out_dir", str(out)] + args,
                          capture_output=True, text=True, env=env, timeout=300)


def test_cli_ema_flag(ema_run, plain_run, tmp_path):
    last = os.path.join(ema_run, "lastepoch.pkl")
    r = _vit_cli(["--ema", "--ckpt", last], tmp_path / "a")
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"loaded EMA weights from {last} ['ema_state_dict']" in r.stdout
    # the sibling rule: bestloss.pkl -> bestloss_ema.pkl, the same weights here (one epoch)
    r = _vit_cli(["--ema", "--ckpt", os.path.join(ema_run, "bestloss.pkl")], tmp_path / "b")
    assert r.returncode == 0, r.stderr[-2000:]
    assert f"loaded EMA weights from {os.path.join(ema_run, 'bestloss_ema.pkl')}" in r.stdout
    # without --ema the raw weights: another picture from the same seed
    r = _vit_cli(["--ckpt", os.path.join(ema_run, "bestloss.pkl")], tmp_path / "c")
    assert r.returncode == 0, r.stderr[-2000:]

    def png(d):
        with open(os.path.join(d, "samples.png"), "rb") as f:
            return f.read()
    assert png(tmp_path / "a") == png(tmp_path / "b") != png(tmp_path / "c")
    # no EMA anywhere: non-zero exit naming the path it looked for
    r = _vit_cli(["--ema", "--ckpt", os.path.join(plain_run, "bestloss.pkl")], tmp_path / "d")
    assert r.returncode != 0
    assert os.path.join(plain_run, "bestloss_ema.pkl") in r.stderr
    # the cold CLI shares the rule
    env = dict(os.environ, PYTHONPATH=ROOT, CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "ViT_draft2drawing.py"), "--ema", "--ckpt",
                        os.path.join(plain_run, "bestloss.pkl"), "--out_dir", str(tmp_path / "e")],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode != 0 and os.path.join(plain_run, "bestloss_ema.pkl") in r.stderr
