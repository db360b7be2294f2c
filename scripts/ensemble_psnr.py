"""What the geometric self-ensemble is worth in PSNR (report only, no threshold).

Trains the GPU leg of ``scripts/psnr_parity.py``'s protocol (procedural textures, sigma =
25, identical seeded init, data and t draws, Adam every step, fp32) and denoises the
held-out set from the same weights with ``DiffusionModel.denoise_image`` at ``ensemble`` 1,
2, 4 and 8 (improved sampler; a 64 x 64 image is one tile).  PSNR by the protocol's
convention; one line of JSON per run, the per-seed gains over ``ensemble=1`` and their mean.
The self-ensemble usually gains on networks trained without augmentation; whatever comes
out is the result, no gain included.

  python scripts/ensemble_psnr.py [--steps 150] [--seeds 3] [--out profiles/x.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

import psnr_parity as P  # noqa: E402


def one_seed(args, seed):
    import vub_image_denoising_amd as vm
    from oracle import rdunet_ref as R
    from oracle.weights import make_params
    a = argparse.Namespace(**vars(args))
    a.seed = seed
    data = P.make_data(a)
    trained = P.run_gpu(a, make_params(R.param_shapes(a.base_filters), seed), data, "fp32")
    model = vm.DiffusionModel(vm.RDUNet_T(base_filters=a.base_filters), timesteps=a.timesteps)
    model.load_state_dict(trained.pop("_state"))
    model = model.cuda().eval()
    ev_noisy, ev_clean = data[2].cuda(), data[3]
    r = {"seed": seed, "psnr_noisy_input": P.psnr_per_image(data[2], data[3]),
         "psnr_improved_sampling": trained["psnr"], "loss_first": trained["loss_first"], "loss_last": trained["loss_last"]}
    for n in (1, 2, 4, 8):
        den = model.denoise_image(ev_noisy, ensemble=n).cpu()
        r[f"psnr_ensemble{n}"] = P.psnr_per_image(den, ev_clean)
    print(f"seed {seed}: " + ", ".join(f"x{n} {r[f'psnr_ensemble{n}']:.4f}" for n in (1, 2, 4, 8)), flush=True)
    return r


def main(argv=None):
    ap = P.parser()
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("ensemble_psnr trains and denoises on the GPU; no device found")
    runs = [one_seed(args, args.seed + 100 * i) for i in range(args.seeds)]
    res = {"protocol": "scripts/psnr_parity.py GPU leg (fp32), held-out PSNR of denoise_image at ensemble 1/2/4/8 "
                       "from the same weights",
           "config": {k: getattr(args, k) for k in ("steps", "batch", "size", "n_train", "n_eval", "base_filters",
                                                    "timesteps", "sigma", "lr", "seed", "seeds")}}
    for n in (1, 2, 4, 8):
        res[f"psnr_ensemble{n}"] = float(np.mean([r[f"psnr_ensemble{n}"] for r in runs]))
    for n in (2, 4, 8):
        g = [r[f"psnr_ensemble{n}"] - r["psnr_ensemble1"] for r in runs]
        res[f"gain_ensemble{n}_db"] = {"mean": float(np.mean(g)), "per_seed": [float(v) for v in g]}
    res["runs"] = runs
    s = json.dumps(res)
    print(s, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(s + "\n")
    return res


if __name__ == "__main__":
    main()
