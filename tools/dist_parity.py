"""1-rank RCCL group on one GPU: the distributed engine paths (event-split graphs with
host-issued collectives, collectives captured in the step graph, graph segments) must
reproduce the single-process engine.

Not bit for bit: the grouped weight-gradient GEMM combines its two token slices
with fp32 atomics (order-dependent last bits), and AdamW turns a last-bit change
of a near-zero gradient into up to 2*lr of parameter change per step.  So the
check is: same losses to 1e-4 and every parameter within 2*lr*steps."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.distributed as dist
from ddim_cold_amd.models import build_model
from ddim_cold_amd.train.engine import EngineConfig, TrainEngine
from ddim_cold_amd.data.synthetic import ColdBatcher, GaussianBatcher, synthetic_pool


def run(dist_mode, comm="torch", wire="fp32", gauss=False, tune=False, layout=None, graph_steps=1):
    torch.manual_seed(0)
    model = build_model("vit_tiny").cuda().train()
    cfg = EngineConfig(lr=1e-3, t_max=100, seed=5, temb_rows=None if gauss else 7,
                       force_segments=dist_mode is not None,
                       graph_comm=dist_mode == "captured", comm_events=dist_mode == "events",
                       graph_warmup=2, comm=comm, grad_wire=wire, graph_steps=graph_steps)
    eng = TrainEngine(model, cfg)
    pool = synthetic_pool(64, seed=3, device="cuda")
    # Gaussian diffusion (t over the whole table): sparse time_embed row exchange
    eng.set_batch_fn(GaussianBatcher(pool, 16, eng.rng, 2000) if gauss else ColdBatcher(pool, 16, eng.rng))
    assert (eng.bucketing.temb_bucket is not None) == (gauss and dist_mode is not None)
    if layout is not None:
        eng.apply_layout(layout)
    if tune:  # measures every layout, then restores the training state
        times = eng.autotune_comm(steps=4, warm=1)
        assert set(times) >= {l[0] for l in eng.COMM_LAYOUTS} and eng.comm_choice in times, times
        assert eng.steps_done == 0 and int(eng.step_ctr[0]) == 0 and int(eng.rng[1]) == 0
    if graph_steps > 1:  # 2 eager + capture, then one replay of the K-step graph
        eng.train_steps(2)
        eng.train_steps(4)
        assert eng._multi is not None and eng._multi[1] == graph_steps == 4, "no K-step graph"
    else:
        for _ in range(6):
            eng.train_step()
    torch.cuda.synchronize()
    out = eng.flat_p.clone(), float(eng.loss_last), getattr(eng, "_graph_comm_failed", False), len(eng._graphs)
    if comm in ("native", "auto"):  # auto: the native communicator came up and verified
        assert eng.ncomm is not None and eng.comm_backend == "native"
    eng.close()
    return out


if __name__ == "__main__":
    from ddim_cold_amd.parallel.dist import free_port
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(free_port()))
    torch.cuda.set_device(0)
    ref, loss0, _, _ = run(None)
    from ddim_cold_amd.parallel.dist import graph_safe_nccl_env
    graph_safe_nccl_env()
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    from ddim_cold_amd.parallel.comm import NativeComm, MAX
    nc = NativeComm(torch.device("cuda", 0))
    x = torch.randn(1000003, device="cuda")  # odd length: exercises the wire kernels' tail
    y = x.clone()
    nc.all_reduce_bf16_wire_(y, torch.empty(x.numel(), dtype=torch.bfloat16, device="cuda"))
    assert torch.equal(y, x.bfloat16().float()), "bf16 wire round trip"
    z = x.clone()
    nc.all_reduce_(z)
    nc.all_reduce_(z, MAX)
    assert torch.equal(z, x)
    b = torch.arange(10, device="cuda")
    nc.broadcast_(b, 0)
    assert torch.equal(b, torch.arange(10, device="cuda"))
    for src in (torch.arange(7, device="cuda"), torch.randn(5, 384, device="cuda")):
        out = torch.empty_like(src)
        nc.all_gather_(out, src)
        assert torch.equal(out, src), "all_gather at 1 rank"
    parts = [torch.randn(1001, device="cuda"), torch.randn(77, 3, device="cuda")]
    want = [p.clone() for p in parts]
    nc.all_reduce_many_(parts)  # one RCCL group over both buffers
    assert all(torch.equal(p, w) for p, w in zip(parts, want)), "all_reduce_many at 1 rank"
    nc.destroy()
    cap, loss1, failed, ng1 = run("captured")
    seg, loss2, _, ng2 = run("segmented")
    # native RCCL communicator (csrc/comm.cpp): captured in the step graph, fp32 and bf16 wire
    nat, loss3, failed3, ng3 = run("captured", comm="native")
    natb, loss4, failed4, ng4 = run("captured", comm="native", wire="bf16")
    gref, gl0, _, _ = run(None, gauss=True)
    gcap, gl1, gfailed, gng = run("captured", gauss=True)
    # event-split: forward + backward graph, optimizer graph, collectives host-issued on the comm stream
    ev, loss5, _, ng5 = run("events")
    evn, loss6, _, ng6 = run("events", comm="native")
    gev, gl2, _, gng2 = run("events", gauss=True)
    # the sparse time_embed exchange through the native communicator's all-gather
    gevn, gl3, _, _ = run("events", comm="native", gauss=True)
    gcapn, gl4, gfailedn, gngn = run("captured", comm="native", gauss=True)
    # one inline all-reduce between the graphs; the autotuned layout after its tuning steps
    evi, loss7, _, ng7 = run("events", layout="inline-1")
    evt, loss8, _, ng8 = run("events", tune=True)
    eva, loss9, _, ng9 = run("events", comm="auto", tune=True)
    # the captured inline layout: ONE all-reduce on the compute stream inside the step
    # graph, and a 4-step graph replayed (data parallel with K-step graphs)
    gin, loss10, gfail10, ng10 = run("events", comm="native", layout="graph-inline-1", graph_steps=4)
    gint, loss11, gfail11, _ = run("events", comm="torch", layout="graph-inline-1", graph_steps=4)
    assert not (gfail10 or gfail11) and ng10 == 1, (gfail10, gfail11, ng10)
    dist.destroy_process_group()
    assert ng5 == 2 and ng6 == 2 and gng2 == 2, (ng5, ng6, gng2)
    assert (gref - gev).abs().max().item() <= 2 * 1e-3 * 6 and abs(gl2 - gl0) <= 1e-4 * abs(gl0), (gl0, gl2)
    assert not gfailed and gng == 1, "sparse time_embed exchange not captured"
    assert not gfailedn and gngn == 1, "native sparse time_embed exchange not captured"
    for other, gl in ((gevn, gl3), (gcapn, gl4)):
        assert (gref - other).abs().max().item() <= 2 * 1e-3 * 6 and abs(gl - gl0) <= 1e-4 * abs(gl0), (gl0, gl)
    assert (gref - gcap).abs().max().item() <= 2 * 1e-3 * 6 and abs(gl1 - gl0) <= 1e-4 * abs(gl0), (gl0, gl1)
    print(f"losses {loss0:.6f} {loss1:.6f} {loss2:.6f} native {loss3:.6f} native-bf16 {loss4:.6f}; "
          f"graphs captured={ng1} segmented={ng2} native={ng3}/{ng4}; fallback={failed} {failed3} {failed4}")
    assert not (failed or failed3 or failed4), "graph capture of collectives fell back"
    assert ng1 == 1 and ng2 > 1 and ng3 == 1 and ng4 == 1
    bound = 2 * 1e-3 * 6
    # bf16 wire: a 1-rank all-reduce of the packed gradient is the bf16 rounding of it;
    # Adam's normalisation keeps the update within the same per-step bound
    for name, other, loss in (("captured", cap, loss1), ("segmented", seg, loss2), ("native", nat, loss3),
                              ("native-bf16", natb, loss4), ("events", ev, loss5), ("events-native", evn, loss6),
                              ("events-inline", evi, loss7), ("events-autotuned", evt, loss8),
                              ("events-auto-comm-autotuned", eva, loss9), ("graph-inline-1-native-K4", gin, loss10),
                              ("graph-inline-1-torch-K4", gint, loss11)):
        d = (ref - other).abs().max().item()
        assert d <= bound, (name, d)
        tol = 1e-2 if name.endswith("bf16") else 1e-4
        assert abs(loss - loss0) <= tol * abs(loss0), (name, loss, loss0)
    print("dist-parity ok")
