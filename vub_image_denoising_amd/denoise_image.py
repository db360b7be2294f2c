"""Denoise one image file of any size (no reference counterpart: the reference's
evaluation feeds 256x256 blocks only).

    python -m vub_image_denoising_amd.denoise_image --checkpoint ckpt.pth --input noisy.png --output clean.png

The image goes through ``sampling.denoise_tiled``: overlapping tiles of one fixed shape
through one captured sampler, blended back.  Pixels are normalised as in the loaders
(``(x/255 - 0.5)/0.5``) and written back with ``denormalize``, clamp and round.  The
checkpoint is either form the trainers write -- the per-epoch dict with
``model_state_dict`` or the final bare ``state_dict`` -- read with ``weights_only=True``.
``--weights ema`` takes the averaged weights of a per-epoch checkpoint trained with
``--ema_decay`` (its ``ema_state_dict``); the ``*_final_ema.pth`` file is a bare
``state_dict`` and loads as it is.  ``--ensemble {2,4,8}`` averages every tile over its
flips (and transposes): the geometric self-ensemble of ``sampling.denoise_tiled``.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np
import torch


def build_parser():
    p = argparse.ArgumentParser(description="Denoise an image of any size with a trained diffusion RDUNet.")
    p.add_argument('--checkpoint', type=str, required=True)
    p.add_argument('--input', type=str, required=True)
    p.add_argument('--output', type=str, required=True)
    p.add_argument('--sampler', type=str, default='improved', choices=['improved', 'direct'])
    p.add_argument('--tile', type=int, default=512)
    p.add_argument('--overlap', type=int, default=32)
    p.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    p.add_argument('--base_filters', type=int, default=32)
    p.add_argument('--timesteps', type=int, default=20)
    p.add_argument('--weights', type=str, default='model', choices=['model', 'ema'],
                   help="ema: the averaged weights of a checkpoint trained with --ema_decay")
    p.add_argument('--ensemble', type=int, default=1, choices=[1, 2, 4, 8],
                   help="geometric self-ensemble: average over 2 (x-flip), 4 (flips) or 8 (flips and transposes) "
                        "transforms of every tile; 1: off")
    return p


def image_to_tensor(img) -> torch.Tensor:
    """PIL image -> [1,3,H,W] fp32 in [-1, 1] (ToTensor + Normalize(0.5, 0.5))."""
    a = np.array(img.convert("RGB"), dtype=np.uint8)     # a writable copy, HWC
    t = torch.from_numpy(a).permute(2, 0, 1).float().div_(255.0)
    return t.sub_(0.5).div_(0.5).unsqueeze(0)


def tensor_to_image(t: torch.Tensor):
    """[1,3,H,W] in [-1, 1] -> PIL RGB image: denormalize, clamp to [0, 1], round to uint8."""
    from PIL import Image
    a = (t[0].detach().float().cpu() * 0.5 + 0.5).clamp_(0.0, 1.0).mul_(255.0).round_().to(torch.uint8)
    return Image.fromarray(a.permute(1, 2, 0).contiguous().numpy())   # uint8 HWC: mode RGB


def load_model(checkpoint, base_filters=32, timesteps=20, dtype="fp32", device="cuda", weights="model"):
    from .diffusion_RDUnet import DiffusionModel, ema_weights
    from .Unet_model import RDUNet_T
    if weights not in ("model", "ema"):
        raise ValueError(f"weights must be 'model' or 'ema', got {weights!r}")
    unet = RDUNet_T(base_filters=base_filters)
    unet.set_compute_dtype(dtype)
    model = DiffusionModel(unet, timesteps=timesteps)
    ckpt = torch.load(checkpoint, map_location="cpu", weights_only=True)
    if weights == "ema":
        ckpt = ema_weights(ckpt, checkpoint)
    elif isinstance(ckpt, dict) and "model_state_dict" in ckpt:
        ckpt = ckpt["model_state_dict"]
    model.load_state_dict(ckpt)
    return model.to(device).eval()


def main(argv=None):
    from PIL import Image
    args = build_parser().parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("denoise_image runs on the ROCm GPU only (HIP kernels); no device found")
    model = load_model(args.checkpoint, args.base_filters, args.timesteps, args.dtype, weights=args.weights)
    with Image.open(args.input) as img:
        noisy = image_to_tensor(img).cuda()
    out = model.denoise_image(noisy, tile=args.tile, overlap=args.overlap, sampler=args.sampler, ensemble=args.ensemble)
    tensor_to_image(out).save(args.output)
    print(f"{args.input}: {noisy.size(3)}x{noisy.size(2)} -> {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
