"""Inpainting (ViT-tiny, N=64, k=20, resample=1) ms per batch at eta = 0 and eta = 1 against
DDIMSampler at the same k, N and eta, interleaved in one process: what the mask-step launch
after every forward costs.  Graph replays between device events:
python tools/ub_inpaint.py [N] [reps] [rounds] [k]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ddim_cold_amd import build_model
from ddim_cold_amd.diffusion import samplers as smp

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
k = int(sys.argv[4]) if len(sys.argv) > 4 else 20
if not torch.cuda.is_available():
    sys.exit("ub_inpaint: needs a GPU")
torch.manual_seed(1234)
model = build_model("vit_tiny").cuda().eval()
with torch.no_grad():
    model.head.bias.uniform_(-0.5, 0.5)
g = torch.Generator().manual_seed(0)
image = torch.rand(N, 3, 64, 64, generator=g) * 2 - 1
noise = torch.randn(N, 3, 64, 64, generator=g)
keep = torch.ones(64, 64, dtype=torch.bool)
keep[16:48, 16:48] = False  # a centred 32x32 hole
loops = {}
for eta in (0.0, 1.0):
    s = smp.DDIMSampler(model, "cuda", k=k, eta=eta)
    for _ in range(3):  # capture, then warm the replay
        s.sample(N, noise=noise, noise_seed=1)
        smp.inpaint(model, image, keep, k=k, eta=eta, device="cuda", noise=noise, noise_seed=1)
    loops[f"ddim eta={eta:g}"] = s._state(N, False).loop
    loops[f"inpaint eta={eta:g}"] = smp._cache(model)[("inpaint", N, k, eta, 1, "cuda")].loop
steps = len(s.ts)
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
for eta in ("0", "1"):
    base, inp = med(res[f"ddim eta={eta}"]), med(res[f"inpaint eta={eta}"])
    print(f"eta={eta}: N={N} k={k} ({steps} steps) {reps} replays x {rounds} rounds: median replay ddim {base:.3f} "
          f"ms/batch, inpaint {inp:.3f} ms/batch ({inp / base:.3f}x, {(inp - base) / steps * 1e3:+.2f} us per step)")
