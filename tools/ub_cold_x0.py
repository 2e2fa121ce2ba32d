"""Cold sampler (ViT-tiny, N=64, six steps) ms per batch: predict="x0" (algorithms 1, 2)
against predict="prev", interleaved in one process.  Graph replays between device
events, and whole sample() calls (host start image, copies, [0, 1] mapping) by the host
clock: python tools/ub_cold_x0.py [N] [reps] [rounds]"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ddim_cold_amd import build_model
from ddim_cold_amd.diffusion.samplers import ColdSampler

N = int(sys.argv[1]) if len(sys.argv) > 1 else 64
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 30
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 3
if not torch.cuda.is_available():
    sys.exit("ub_cold_x0: needs a GPU")
torch.manual_seed(1234)
model = build_model("vit_tiny").cuda().eval()
with torch.no_grad():
    model.head.bias.uniform_(-0.5, 0.5)
variants = {"prev": dict(predict="prev"), "x0 alg 1": dict(predict="x0", algorithm=1),
            "x0 alg 2": dict(predict="x0", algorithm=2)}
samplers = {k: ColdSampler(model, "cuda", **v) for k, v in variants.items()}
for s in samplers.values():  # capture, then warm the replay
    for _ in range(3):
        s.sample(N, generator=torch.Generator().manual_seed(0))
res = {k: ([], []) for k in variants}
for r in range(rounds):
    for name, s in samplers.items():
        loop = s._state(N).loop
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(reps):
            loop.run(True)
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / reps
        t0 = time.perf_counter()
        for _ in range(reps):
            s.sample(N, generator=torch.Generator().manual_seed(0))
        torch.cuda.synchronize()
        call_ms = (time.perf_counter() - t0) / reps * 1e3
        res[name][0].append(dev_ms)
        res[name][1].append(call_ms)
        print(f"round {r} {name}: replay {dev_ms:.3f} ms, sample() {call_ms:.3f} ms", flush=True)
med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
base = med(res["prev"][0])
for name, (dev, call) in res.items():
    print(f"{name}: N={N} {reps} replays x {rounds} rounds: median replay {med(dev):.3f} ms/batch "
          f"({med(dev) / base:.2f}x prev), median sample() {med(call):.3f} ms/batch")
