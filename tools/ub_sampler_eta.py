"""DDIM sampler (ViT-tiny, N=64, k=20: 100 steps) ms per batch at eta = 0, eta = 1 with the noise
drawn in the head epilogue (one forward per step), and eta = 1 on the fallback (``ROWS`` off:
the deterministic step, then a randn_ launch and x += sigma z), interleaved in one process.
Graph replays between device events, medians over rounds; the cost of the in-epilogue
Box-Muller per step is (fused - eta 0) / steps.
python tools/ub_sampler_eta.py [N] [reps] [rounds] [--eta0]   (--eta0: the eta = 0 variant alone,
for an A/B of two builds with tools/gpu_lib_ab.sh SAMPLER=1)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ddim_cold_amd import build_model
from ddim_cold_amd.diffusion import samplers as smp

args = [a for a in sys.argv[1:] if not a.startswith("--")]
N = int(args[0]) if len(args) > 0 else 64
reps = int(args[1]) if len(args) > 1 else 20
rounds = int(args[2]) if len(args) > 2 else 5
K = 20
if not torch.cuda.is_available():
    sys.exit("ub_sampler_eta: needs a GPU")
torch.manual_seed(1234)
model = build_model("vit_tiny").cuda().eval()
with torch.no_grad():
    model.head.bias.uniform_(-0.5, 0.5)
variants = {"eta=0": (0.0, True)}
if "--eta0" not in sys.argv:
    variants.update({"eta=1 fused": (1.0, True), "eta=1 fallback": (1.0, False)})
loops = {}
for name, (eta, rows) in variants.items():  # build each loop under its ROWS setting: capture, then warm the replay
    smp.ROWS = rows
    model.__dict__.pop("_sampler_graphs", None)
    s = smp.DDIMSampler(model, "cuda", k=K, eta=eta)
    for _ in range(3):
        s.sample(N, generator=torch.Generator().manual_seed(0))
    loops[name] = (s, s._state(N, False).loop)
    smp.ROWS = True
steps = len(loops["eta=0"][0].ts)
res = {k: [] for k in variants}
for r in range(rounds):
    for name, (s, loop) in loops.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            loop.run(True)
        e1.record()
        torch.cuda.synchronize()
        res[name].append(e0.elapsed_time(e1) / reps)
        print(f"round {r} {name}: replay {res[name][-1]:.3f} ms", flush=True)
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
base = med(res["eta=0"])
for name, v in res.items():
    print(f"{name}: N={N} k={K} {reps} replays x {rounds} rounds: median replay {med(v):.3f} ms/batch "
          f"({med(v) / base:.3f}x eta=0, {(med(v) - base) / steps * 1e3:+.2f} us/step)")
