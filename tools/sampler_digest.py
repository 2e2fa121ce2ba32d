"""One ``name sha256`` line per sampler case, through the public API alone: run on two trees
(same built extension) and diff the output to show a change of the sampling code kept every
result bit for bit.  On ``cuda`` each case runs twice (capture, then replay) under the default
switches, ``ROWS`` off, and ``ROWS`` + ``PATCH_CHAIN`` off; the eta > 0 cases once more on the
unfolded program.  python tools/sampler_digest.py cpu|cuda"""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ddim_cold_amd import build_model
from ddim_cold_amd.diffusion import samplers as smp
from ddim_cold_amd.models import program

dev = sys.argv[1] if len(sys.argv) > 1 else "cpu"
torch.manual_seed(0)
model = build_model("vit_tiny")
with torch.no_grad():
    model.head.bias.uniform_(-0.5, 0.5)  # loud head bias: at random init x0-hat would be ~ 0
model = model.to(dev).eval()
gen = lambda seed: torch.Generator().manual_seed(seed)  # noqa: E731
imgs = torch.rand(3, 3, 64, 64, generator=gen(5)) * 2.4 - 1.2
xs = torch.randn(3, 3, 64, 64, generator=gen(6))


def ddim(eta, seed):
    s = smp.DDIMSampler(model, dev, k=400, eta=eta)
    return [s.sample(4, generator=gen(1), noise_seed=seed)] + s.sequence(2, generator=gen(2), noise_seed=seed)


def starts(eta, seed):
    return smp.ddim_from_starts(model, xs.to(dev), [1999, 999, 1999], 1000, dev, eta=eta, noise_seed=seed).cpu()


ETA_CASES = {"ddim eta=0.5": lambda: ddim(0.5, 7), "from_starts eta=1": lambda: starts(1.0, 11)}
CASES = {
    "ddim eta=0": lambda: ddim(0.0, None),
    "cold prev": lambda: smp.ColdSampler(model, dev).sequence(3, generator=gen(3)),
    "cold x0 alg 1": lambda: smp.ColdSampler(model, dev, predict="x0", algorithm=1).sequence(3, generator=gen(3)),
    "cold x0 alg 2": lambda: smp.ColdSampler(model, dev, predict="x0", algorithm=2).sequence(3, generator=gen(3)),
    "cold restore": lambda: smp.ColdSampler(model, dev, predict="x0").restore(imgs, [2, 0, 5], sequence=True),
    "from_starts eta=0": lambda: starts(0.0, None),
    "img2img one grid": lambda: smp.img2img(model, imgs[0], [1599, 1799, 1999], k=100, device=dev, generator=gen(4)),
    "img2img two grids": lambda: smp.img2img(model, imgs[0], [1999, 1900], k=100, device=dev, generator=gen(4)),
    **ETA_CASES,
}


def digest(out) -> str:
    out = torch.cat([o.reshape(-1) for o in out]) if isinstance(out, (list, tuple)) else out
    return hashlib.sha256(out.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:32]


def run(setting: str, cases, rows=True, chain=True, fold=True):
    smp.ROWS, smp.PATCH_CHAIN, program.FOLD_LN = rows, chain, fold
    model.__dict__.pop("_sampler_graphs", None)
    for name, case in cases.items():
        for run_ in (("capture", "replay") if dev == "cuda" else ("eager",)):
            print(f"{setting} / {name} / {run_} {digest(case())}", flush=True)


run("default", CASES)
if dev == "cuda":
    run("ROWS off", CASES, rows=False)
    run("ROWS, PATCH_CHAIN off", CASES, rows=False, chain=False)
    run("unfolded", ETA_CASES, fold=False)
