#!/usr/bin/env python3
"""What the weight EMA costs in the captured train step (optim.EMA).

The captured 'step' graph of RDUNet_T(base_filters=32) in bf16 at ``--batch`` x 3 x
``--size`` x ``--size`` with optim.FusedAdamW, three variants, each with its own model,
optimizer and graph:

  none      no EMA                                   (the launches of the step as it was)
  fused     EMA attached: updated inside rdn_adam_step_ema  (+8 bytes per parameter)
  separate  EMA as its own rdn_ema_update launch behind rdn_adam_step, inside the graph
            (+12 bytes per parameter, one launch more)

``--ema-warmup`` adds the device update counter (one rdn_counter_inc node) to the two EMA
variants.  A pass times ``--steps`` replays between two device synchronisations; the
passes alternate none, fused, separate, none, ... in one process after a warm-up pass of
each, and the median, minimum and maximum pass of every variant are written, with the
spread (max - min) / median as the run-to-run noise to judge differences by.

    python scripts/ema_bench.py --out profiles/ema_step_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

VARIANTS = ("none", "fused", "separate")


def make_variant(name, args):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd import _hip as H
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    from vub_image_denoising_amd.optim import EMA, FusedAdamW
    from vub_image_denoising_amd.train_graph import TrainStepGraph

    class SeparateEmaAdamW(FusedAdamW):
        """The attached EMA updated by its own launch behind the plain Adam entry."""

        def _update(self, fp, g, lib, st):
            ema, self.ema = self.ema, None
            try:
                super()._update(fp, g, lib, st)
            finally:
                self.ema = ema
            shadow, *rest = ema._kernel_args()
            H.check(lib.rdn_ema_update(shadow, fp.flat.data_ptr(), fp.numel, *rest, st), "ema_update")
            ema._advance(lib, st)

    torch.manual_seed(0)
    unet = vm.RDUNet_T(base_filters=args.base_filters).cuda()
    unet.set_compute_dtype(args.dtype)
    model = DiffusionModel(unet, timesteps=20).cuda()
    opt = (SeparateEmaAdamW if name == "separate" else FusedAdamW)(model.parameters(), lr=1e-4, weight_decay=1e-4)
    ema = None
    if name != "none":
        ema = EMA(model, args.decay, warmup=args.ema_warmup)
        opt.attach_ema(ema)
    shape = (args.batch, 3, args.size, args.size)
    graph = TrainStepGraph(model, opt, shape, clip_value=1.0)
    return dict(name=name, model=model, opt=opt, ema=ema, graph=graph, ms=[])


def run_pass(v, clean, noisy, steps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        v["graph"](clean, noisy)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--base-filters", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--decay", type=float, default=0.9999)
    ap.add_argument("--ema-warmup", action="store_true")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "ema_step_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ema_bench.py measures on the GPU; none found")
    if args.passes < 3:
        sys.exit("--passes must be at least 3 (the median is reported)")
    g = torch.Generator(device="cuda").manual_seed(0)
    clean = torch.rand(args.batch, 3, args.size, args.size, generator=g, device="cuda") * 2 - 1
    noisy = clean + 0.1 * torch.randn(clean.shape, generator=g, device="cuda")
    variants = [make_variant(n, args) for n in VARIANTS]
    for v in variants:
        run_pass(v, clean, noisy, max(10, args.steps // 5))
    for _ in range(args.passes):
        for v in variants:
            v["ms"].append(run_pass(v, clean, noisy, args.steps))
    numel = variants[0]["opt"]._fp.numel
    rows = []
    for v in variants:
        med = statistics.median(v["ms"])
        row = dict(variant=v["name"], step_ms_median=med, step_ms_min=min(v["ms"]), step_ms_max=max(v["ms"]),
                   spread=(max(v["ms"]) - min(v["ms"])) / med, step_ms_passes=[round(x, 4) for x in v["ms"]],
                   graph_nodes=v["graph"].graph_nodes,
                   extra_bytes_algorithmic={"none": 0, "fused": 8, "separate": 12}[v["name"]] * numel)
        if v["ema"] is not None:
            row["ema_updates"] = v["ema"].num_updates
        rows.append(row)
        print(f"{v['name']:9s} {med:8.4f} ms/step  (min {row['step_ms_min']:.4f}, max {row['step_ms_max']:.4f}, "
              f"nodes {row['graph_nodes']})", flush=True)
    base = rows[0]["step_ms_median"]
    for r in rows:
        r["us_over_none"] = 1e3 * (r["step_ms_median"] - base)
    result = dict(what="captured 'step' replay (TrainStepGraph, FusedAdamW), ms per step between two device "
                       "synchronisations; median / min / max of interleaved passes",
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, batch=args.batch, size=args.size,
                  base_filters=args.base_filters, dtype=args.dtype, decay=args.decay, ema_warmup=args.ema_warmup,
                  steps_per_pass=args.steps, passes=args.passes, flat_parameters=numel, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
