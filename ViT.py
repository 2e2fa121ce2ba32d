#!/usr/bin/env python3
"""Compatibility sampling CLI: ``python ViT.py [--sample_n 256] [--acc_k 1]``.

Reference behaviour (ViT.py:258-316): build the Oxford-Flowers model (64x64,
p=4, D=256, depth 6, 4 heads), load ``Saved_Models/OxfordFlower.pkl``, write a
DDIM trajectory grid (k=100, 6 samples) to ``denoise_sequence.png`` and a
``sample_n`` DDIM sample grid (jump ``acc_k``) to ``samples.png``.  ``--inpaint IMAGE --mask MASK
[--resample R]`` instead keeps IMAGE where MASK is white and generates the rest (``inpaint.png``).

Differences: the model runs in eval mode (the reference left
dropout on), samplers are hipGraph-captured on the GPU, ``get_next_path``
terminates, and a missing checkpoint falls back to random init with a warning
(pretrained blobs are not shipped).  Also re-exports the model API so
``from ViT import DiffusionVisionTransformer`` keeps working.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import click  # noqa: E402
import torch  # noqa: E402

from ddim_cold_amd.models.vit import (Attention, Block, DiffusionVisionTransformer, DropPath, Mlp,  # noqa: E402,F401
                                      PatchEmbed, drop_path, trunc_normal_)
from ddim_cold_amd.utils.images import get_next_path, save_grid, save_sequence_grid  # noqa: E402


def _inpaint(model, device, image_file, mask_file, k, eta, resample, seed, generator, out_dir):
    """``--inpaint``: the grid original | masked input | result as ``inpaint.png``; returns its path."""
    from ddim_cold_amd.data.datasets import load_image
    from ddim_cold_amd.data.synthetic import synthetic_pool
    H, W = model.img_size
    if os.path.isfile(image_file):
        img = load_image(image_file, model.img_size)
    else:
        print(f"warning: {image_file} not found, using a synthetic picture", file=sys.stderr)
        img = synthetic_pool(1, (H, W), seed=seed)[0]
    if mask_file is not None and os.path.isfile(mask_file):
        keep = load_image(mask_file, model.img_size).mean(0) > 0.0  # white = keep
    else:
        if mask_file is not None:
            print(f"warning: {mask_file} not found, using a centred square hole", file=sys.stderr)
        keep = torch.ones(H, W, dtype=torch.bool)
        keep[H // 4:H - H // 4, W // 4:W - W // 4] = False
    out = model.inpaint(img, keep, k=k, eta=eta, resample=resample, device=device, generator=generator)
    unit = (img + 1) / 2
    grid = torch.stack([unit, unit * keep, out[0]])
    return save_grid(grid, get_next_path(os.path.join(out_dir, "inpaint.png")), nrow=3)


@click.command()
@click.option("--sample_n", default=256, help="Number of samples you'll get.")
@click.option("--acc_k", default=1, help="Number of step jumped during sampling.")
@click.option("--ckpt", default=os.path.join(HERE, "Saved_Models", "OxfordFlower.pkl"), help="state_dict file")
@click.option("--model", "model_name", default="oxford_flower", help="named config (ddim_cold_amd.models.MODEL_CONFIGS)")
@click.option("--out_dir", default=os.path.join(HERE, "Saved_Models"))
@click.option("--seq_n", default=6)
@click.option("--seq_k", default=100)
@click.option("--seed", default=0)
@click.option("--ema", is_flag=True, help="sample from the EMA weights: 'ema_state_dict' of a lastepoch.pkl-style "
              "--ckpt, else the <ckpt>_ema sibling file (bestloss.pkl -> bestloss_ema.pkl)")
@click.option("--eta", default=0.0, type=float, help="DDIM noise scale in [0, 1]: 0 deterministic DDIM (default), "
              "1 DDPM ancestral sampling; applies to the trajectory grid and the samples")
@click.option("--solver", default="ddim", help="ddim (default), or dpmpp2m: DPM-Solver++(2M), the second-order "
              "multistep solver on the same --acc_k grid (needs --eta 0; not used by --inpaint)")
@click.option("--inpaint", "inpaint_image", default=None, metavar="IMAGE", help="inpaint IMAGE instead of sampling: "
              "keep it where --mask is white, generate the rest (jump --acc_k, noise --eta, --seed); writes "
              "inpaint.png = original | masked input | result")
@click.option("--mask", "mask_file", default=None, metavar="MASK", help="mask picture of --inpaint (white = keep); "
              "default: a centred square hole of half the image size")
@click.option("--resample", default=1, help="--inpaint: runs of every grid step (RePaint resampling), >= 1")
def main(sample_n, acc_k, ckpt, model_name, out_dir, seq_n, seq_k, seed, ema, eta, solver, inpaint_image, mask_file,
         resample):
    """DDIM sampling from a DiffusionVisionTransformer checkpoint."""
    from ddim_cold_amd.models import build_model
    from ddim_cold_amd.train.checkpoint import load_weights, resolve_ema_checkpoint
    if not 0.0 <= eta <= 1.0:
        sys.exit(f"error: --eta must be in [0, 1], got {eta}")
    if solver not in ("ddim", "dpmpp2m"):
        sys.exit(f"error: --solver must be ddim or dpmpp2m, got {solver}")
    if solver == "dpmpp2m" and eta > 0:
        sys.exit(f"error: --solver dpmpp2m needs --eta 0, got {eta}")
    if resample < 1:
        sys.exit(f"error: --resample must be >= 1, got {resample}")
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model = build_model(model_name, init_order="vit")  # ViT.py:184 draw order (weights are loaded anyway)
    if ema:
        try:
            path, key = resolve_ema_checkpoint(ckpt)
        except FileNotFoundError as e:
            sys.exit(f"error: {e}")
        load_weights(model, path, strict=True, ema=key)
        print(f"loaded EMA weights from {path}" + (" ['ema_state_dict']" if key else ""))
    elif os.path.isfile(ckpt):
        load_weights(model, ckpt, strict=True)
    else:
        print(f"warning: {ckpt} not found, sampling from random-init weights", file=sys.stderr)
    model.to(device).eval()
    g = torch.Generator().manual_seed(seed)
    if inpaint_image is not None:
        print(f"wrote {_inpaint(model, device, inpaint_image, mask_file, acc_k, eta, resample, seed, g, out_dir)}")
        return
    seq = model.diffusion_sequence(device, seq_k, N=seq_n, generator=g, eta=eta, solver=solver)
    p1 = save_sequence_grid(seq, get_next_path(os.path.join(out_dir, "denoise_sequence.png")))
    imgs = model.sampler(device, acc_k, sample_n, generator=g, eta=eta, solver=solver)
    p2 = save_grid(imgs, get_next_path(os.path.join(out_dir, "samples.png")), nrow=16)
    print(f"wrote {p1} and {p2}")


if __name__ == "__main__":
    main()
