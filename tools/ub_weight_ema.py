"""Cost of the weight EMA in the training step, on one box: the ViT-tiny training
configuration of bench.py (cold diffusion, batch 32, synthetic pool, 4-step graphs)
through TrainEngine.train_steps with EngineConfig.weight_ema 0 and 0.9999, the two
variants interleaved ROUNDS times (an engine per variant, built once and warmed up).
The EMA variant also runs the time-embedding rows that are lazy without it.
usage: python tools/ub_weight_ema.py [steps=400] [rounds=3]"""
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from ddim_cold_amd.data.synthetic import ColdBatcher, synthetic_pool  # noqa: E402
from ddim_cold_amd.models import build_model  # noqa: E402
from ddim_cold_amd.train.engine import EngineConfig, TrainEngine  # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 400
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
BATCH, K, WARMUP = 32, 4, 24
dev = torch.device("cuda")


def engine(weight_ema):
    torch.manual_seed(1234)
    model = build_model("vit_tiny").to(dev).train()
    cfg = EngineConfig(lr=0.005 * BATCH / 512, t_max=512 * 100, seed=42, graph_steps=K,
                       temb_rows=int(math.log2(model.img_size[1])) + 1, weight_ema=weight_ema)
    eng = TrainEngine(model, cfg, device=dev)
    eng.set_batch_fn(ColdBatcher(synthetic_pool(1024, tuple(model.img_size), seed=7, device=dev), BATCH, eng.rng))
    eng.train_steps(WARMUP)  # eager warm-up, capture, a few replays
    torch.cuda.synchronize()
    return eng


variants = [(w, engine(w)) for w in (0.0, 0.9999)]
for _ in range(rounds):
    for w, eng in variants:
        eng.train_steps(K)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.train_steps(steps)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(f"weight_ema={w}: {1e3 * dt / steps:.4f} ms/step (lazy rows {'on' if eng.lazy else 'off'})", flush=True)
