#!/usr/bin/env python3
"""Compatibility demo: cold de-pixelation sequence + zero-shot draft -> drawing.

Reference behaviour (ViT_draft2drawing.py:331-419): load the ViT-tiny cold
model (``Saved_Models/20220822vit_tiny_diffusion/bestloss.pkl``), write a cold
de-pixelation trajectory grid (5 samples x 7 columns), then noise a draft
image to t_start in 1599..1999 (step 50), denoise each with DDIM k=10 and
write the 1 x 10 grid ``draft2img.png``.  Here the 9 noise levels run as one
batched, hipGraph-captured img2img call.  Without the draft / checkpoint
files (not shipped) a synthetic draft / random init is used, with a warning.

``--predict x0`` samples a model trained to predict the clean image (``dataset:
cold_x0``) with the Cold Diffusion update (``--algorithm`` 1 or 2).  ``--restore
IMAGE`` replaces the draft -> drawing stage: IMAGE is pixelated at every level
1..S and each version restored (x0 models: one batched call; prev models: one
call per level); ``restore.png`` shows the pixelated inputs over the results.
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import torch  # noqa: E402

from ddim_cold_amd.models.vit import (Attention, Block, DiffusionVisionTransformer, DropPath, Mlp,  # noqa: E402,F401
                                      PatchEmbed, drop_path, positionalencoding1d, trunc_normal_)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ckpt", default=os.path.join(HERE, "Saved_Models", "20220822vit_tiny_diffusion", "bestloss.pkl"))
    ap.add_argument("--ema", action="store_true",
                    help="use the EMA weights: 'ema_state_dict' of a lastepoch.pkl-style --ckpt, else the "
                         "<ckpt>_ema sibling file (bestloss.pkl -> bestloss_ema.pkl)")
    ap.add_argument("--draft", default=os.path.join(HERE, "Saved_Models", "draft.jpg"))
    ap.add_argument("--out_dir", default=os.path.join(HERE, "Saved_Models"))
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--eta", type=float, default=0.0,
                    help="DDIM noise scale of the draft -> drawing stage, in [0, 1]: 0 deterministic DDIM "
                         "(default), 1 DDPM ancestral sampling")
    ap.add_argument("--solver", choices=("ddim", "dpmpp2m"), default="ddim",
                    help="solver of the draft -> drawing stage: ddim (default), or dpmpp2m = DPM-Solver++(2M), "
                         "second-order multistep on the same grid (needs --eta 0)")
    ap.add_argument("--predict", choices=("prev", "x0"), default="prev",
                    help="what the cold model predicts: x_{t-1} (dataset: cold) or x0 (dataset: cold_x0)")
    ap.add_argument("--algorithm", type=int, choices=(1, 2), default=2,
                    help="cold x0 update: 1 = D(x0, t-1), 2 = x_t - D(x0, t) + D(x0, t-1)")
    ap.add_argument("--restore", metavar="IMAGE", default=None,
                    help="restore IMAGE from each pixelation level instead of the draft -> drawing stage")
    a = ap.parse_args(argv)
    if not 0.0 <= a.eta <= 1.0:
        ap.error(f"--eta must be in [0, 1], got {a.eta}")
    if a.solver == "dpmpp2m" and a.eta > 0:
        ap.error(f"--solver dpmpp2m needs --eta 0, got {a.eta}")
    from ddim_cold_amd.data.datasets import load_image
    from ddim_cold_amd.data.synthetic import synthetic_pool
    from ddim_cold_amd.diffusion.samplers import img2img
    from ddim_cold_amd.models import build_model
    from ddim_cold_amd.train.checkpoint import load_weights, resolve_ema_checkpoint
    from ddim_cold_amd.utils.images import get_next_path, save_grid, save_sequence_grid
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model = build_model("vit_tiny")
    if a.ema:
        try:
            path, key = resolve_ema_checkpoint(a.ckpt)
        except FileNotFoundError as e:
            sys.exit(f"error: {e}")
        load_weights(model, path, strict=True, ema=key)
        print(f"loaded EMA weights from {path}" + (" ['ema_state_dict']" if key else ""))
    elif os.path.isfile(a.ckpt):
        load_weights(model, a.ckpt, strict=True)
    else:
        print(f"warning: {a.ckpt} not found, using random-init weights", file=sys.stderr)
    model.to(device).eval()
    g = torch.Generator().manual_seed(a.seed)
    seq = model.cold_diffusion_sequence(device, N=5, generator=g, predict=a.predict, algorithm=a.algorithm)
    p1 = save_sequence_grid(seq, get_next_path(os.path.join(a.out_dir, "denoise_sequence.png")))
    if a.restore is not None:
        from ddim_cold_amd.diffusion.schedule import cold_steps
        from ddim_cold_amd.ops.reference import pixelate
        if os.path.isfile(a.restore):
            img = load_image(a.restore, model.img_size)
        else:
            print(f"warning: {a.restore} not found, using a synthetic picture", file=sys.stderr)
            img = synthetic_pool(1, tuple(model.img_size), seed=a.seed)[0]
        levels = list(range(1, cold_steps(model.img_size[1]) + 1))
        imgs = img.unsqueeze(0).expand(len(levels), -1, -1, -1)
        if a.predict == "x0":  # every level in one batch, each joining the grid at its own step
            out = model.cold_restore(imgs, levels, device, predict="x0", algorithm=a.algorithm)
        else:
            out = torch.cat([model.cold_restore(imgs[i:i + 1], v, device) for i, v in enumerate(levels)])
        pix = torch.cat([pixelate(imgs[i:i + 1], 2 ** v) for i, v in enumerate(levels)])
        p2 = save_grid(torch.cat([(pix + 1) / 2, out]), get_next_path(os.path.join(a.out_dir, "restore.png")),
                       nrow=len(levels))
        print(f"wrote {p1} and {p2}")
        return 0
    if os.path.isfile(a.draft):
        draft = load_image(a.draft, model.img_size)
    else:
        print(f"warning: {a.draft} not found, using a synthetic draft", file=sys.stderr)
        draft = synthetic_pool(1, tuple(model.img_size), seed=a.seed)[0]
    starts = list(range(1599, 2000, 50))
    out = img2img(model, draft, starts, k=a.k, device=device, generator=g, eta=a.eta, solver=a.solver)
    row = torch.cat([((draft + 1) / 2).unsqueeze(0), out], dim=0)
    p2 = save_grid(row, get_next_path(os.path.join(a.out_dir, "draft2img.png")), nrow=row.shape[0])
    print(f"wrote {p1} and {p2}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
