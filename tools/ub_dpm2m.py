"""DPM-Solver++(2M) sampler (ViT-tiny, N=64) ms per batch, interleaved in one process:
solver="dpmpp2m" at k=100 (20 steps), solver="ddim" at k=100 (the same 20 forwards: what the
extra launch per step and the update moved out of the head epilogue cost) and solver="ddim" at
k=20 (100 steps, the headline shape).  Graph replays between device events:
python tools/ub_dpm2m.py [N] [reps] [rounds]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ddim_cold_amd import build_model
from ddim_cold_amd.diffusion import samplers as smp

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
if not torch.cuda.is_available():
    sys.exit("ub_dpm2m: needs a GPU")
torch.manual_seed(1234)
model = build_model("vit_tiny").cuda().eval()
with torch.no_grad():
    model.head.bias.uniform_(-0.5, 0.5)
noise = torch.randn(N, 3, 64, 64, generator=torch.Generator().manual_seed(0))
loops, steps = {}, {}
for name, solver, k in (("dpmpp2m k=100", "dpmpp2m", 100), ("ddim k=100", "ddim", 100), ("ddim k=20", "ddim", 20)):
    s = smp.DDIMSampler(model, "cuda", k=k, solver=solver)
    for _ in range(3):  # capture, then warm the replay
        s.sample(N, noise=noise)
    loops[name], steps[name] = s._state(N, False).loop, len(s.ts)
    assert loops[name].graph is not None
res = {name: [] for name in loops}
for r in range(rounds):
    for name, loop in loops.items():
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
dpm, d100, d20 = (med(res[n]) for n in ("dpmpp2m k=100", "ddim k=100", "ddim k=20"))
print(f"N={N} {reps} replays x {rounds} rounds, median replay: dpmpp2m k=100 ({steps['dpmpp2m k=100']} steps) {dpm:.3f} "
      f"ms/batch, ddim k=100 ({steps['ddim k=100']} steps) {d100:.3f} ms/batch, ddim k=20 ({steps['ddim k=20']} steps) "
      f"{d20:.3f} ms/batch; dpmpp2m against ddim at k=100 {(dpm - d100) / steps['ddim k=100'] * 1e3:+.2f} us per step, "
      f"against ddim at k=20 {d20 / dpm:.2f}x fewer ms")
