#!/usr/bin/env python3
"""Time the trainers' epoch loop (diffusion_RDUnet.run_epochs) eager against captured.

One epoch of ``--batches`` in-memory device batches (a few distinct ones, cycled),
``val_loader=None``, RDUNet_T(base_filters=32) at 256x256 in bf16, for every
batch size in ``--batch-sizes`` and both accumulation modes.  Variants:

  a  torch.optim.AdamW, eager, log_every=1        (the trainers before captured steps)
  b  optim.FusedAdamW,  eager, log_every=1
  c  optim.FusedAdamW,  captured, log_every=1
  d  optim.FusedAdamW,  captured, log_every=50

Each variant keeps its own model and optimizer, is warmed up on a short epoch (which
also captures its graphs), and the timed passes alternate a, b, c, d, a, b, ... in one
process; the median pass is reported.  Two times per pass: ``loop`` from the first
batch handed to the loop until the device has finished the last one (what the batches
cost), and ``epoch`` for the whole call (adds the epoch's checkpoint write).  The
per-batch ``print`` of the loop goes to an in-memory sink.

``--model baseline`` times the plain RDUNet baseline's trainer instead
(RDUNet_model.train_model: L1 loss, its one accumulation rule, RDUNet(base_filters)),
the same variants.

    python scripts/trainer_bench.py --out profiles/trainer_graph_bench.json
    python scripts/trainer_bench.py --model baseline --base-filters 128 --dtype fp32 --batch-sizes 16 \
        --batches 16 --warmup-batches 8 --variants b c d --out profiles/baseline_trainer_bench_f128_fp32.json
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import tempfile
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

VARIANTS = {   # name: (fused optimizer, captured, log_every)
    "a_torch_adamw_eager_log1": (False, False, 1),
    "b_fused_adamw_eager_log1": (True, False, 1),
    "c_fused_adamw_graph_log1": (True, True, 1),
    "d_fused_adamw_graph_log50": (True, True, 50),
}


class DeviceBatches:
    """``n`` device batches per epoch out of ``distinct`` resident ones; records when the
    loop takes the first batch and when the device has finished after the last."""

    def __init__(self, n, batch, size, distinct=8, seed=0):
        g = torch.Generator(device="cuda").manual_seed(seed)
        self.data = []
        for _ in range(distinct):
            clean = torch.rand(batch, 3, size, size, generator=g, device="cuda") * 2 - 1
            self.data.append((clean + 0.1 * torch.randn(clean.shape, generator=g, device="cuda"), clean))
        self.n = n
        self.t0 = self.t1 = None

    def __len__(self):
        return self.n

    def __iter__(self):
        torch.cuda.synchronize()
        self.t0 = time.perf_counter()
        for k in range(self.n):
            yield self.data[k % len(self.data)]
        torch.cuda.synchronize()
        self.t1 = time.perf_counter()


def make_variant(name, args):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    from vub_image_denoising_amd.optim import FusedAdamW
    fused, captured, log_every = VARIANTS[name]
    torch.manual_seed(0)
    if args.model == "baseline":
        model = vm.RDUNet(base_filters=args.base_filters).cuda()
        model.set_compute_dtype(args.dtype)
    else:
        unet = vm.RDUNet_T(base_filters=args.base_filters).cuda()
        unet.set_compute_dtype(args.dtype)
        model = DiffusionModel(unet, timesteps=20).cuda()
    cls = FusedAdamW if fused else torch.optim.AdamW
    opt = cls(model.parameters(), lr=1e-4, weight_decay=1e-4)
    return dict(name=name, model=model, opt=opt, captured=captured, log_every=log_every, loop=[], epoch=[])


def run_pass(v, loader, mode, outdir):
    from vub_image_denoising_amd.diffusion_RDUnet import run_epochs
    from vub_image_denoising_amd.RDUNet_model import train_model
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        if mode == "baseline":
            train_model(v["model"], loader, None, v["opt"], None, None, outdir, 1, accumulation_steps=4,
                        clip_value=1.0, log_every=v["log_every"], captured=v["captured"])
        else:
            run_epochs(v["model"], loader, None, v["opt"], None, None, outdir, 'uniform', 1, 0, 4, 1.0, v["log_every"],
                       sample=None, accumulation=mode, captured=v["captured"])
    torch.cuda.synchronize()
    return loader.t1 - loader.t0, time.perf_counter() - t0


def bench_config(batch, mode, args, outdir):
    variants = [make_variant(n, args) for n in VARIANTS if n[0] in args.variants]
    warm = DeviceBatches(args.warmup_batches, batch, args.size)
    loader = DeviceBatches(args.batches, batch, args.size)
    for v in variants:
        run_pass(v, warm, mode, outdir)
    for _ in range(args.passes):
        for v in variants:
            loop, epoch = run_pass(v, loader, mode, outdir)
            v["loop"].append(loop)
            v["epoch"].append(epoch)
    rows = []
    for v in variants:
        loop, epoch = statistics.median(v["loop"]), statistics.median(v["epoch"])
        row = dict(batch=batch, accumulation=mode, variant=v["name"], log_every=v["log_every"],
                   loop_ms_per_batch=1e3 * loop / args.batches, img_per_s=batch * args.batches / loop,
                   loop_s_passes=[round(x, 4) for x in v["loop"]], epoch_s=epoch)
        if v["captured"]:
            (graphs,) = v["model"]._rdn_train_graphs.values()
            row["captures"] = graphs.captures
        rows.append(row)
        print(f"B{batch} {mode:9s} {v['name']:28s} {row['loop_ms_per_batch']:7.3f} ms/batch "
              f"{row['img_per_s']:7.1f} img/s  (passes {row['loop_s_passes']}, whole call {epoch:.3f} s)", flush=True)
    base = rows[0]["loop_ms_per_batch"]
    for r in rows:
        r["speedup_vs_" + rows[0]["variant"][0]] = base / r["loop_ms_per_batch"]
    del variants
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch-sizes", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--modes", nargs="+", default=["reference", "fixed"])
    ap.add_argument("--batches", type=int, default=200)
    ap.add_argument("--warmup-batches", type=int, default=52)   # log_every=50: a logged non-step batch occurs
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--base-filters", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--model", default="diffusion", choices=["diffusion", "baseline"],
                    help="baseline: RDUNet_model.train_model on a plain RDUNet (--modes is not used)")
    ap.add_argument("--variants", nargs="+", default=["a", "b", "c", "d"], choices=["a", "b", "c", "d"])
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trainer_graph_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("trainer_bench.py measures on the GPU; none found")
    if args.passes < 3:
        sys.exit("--passes must be at least 3 (the median is reported)")
    rows = []
    with tempfile.TemporaryDirectory() as outdir:
        for batch in args.batch_sizes:
            for mode in (["baseline"] if args.model == "baseline" else args.modes):
                rows += bench_config(batch, mode, args, outdir)
    what = "RDUNet_model.train_model" if args.model == "baseline" else "run_epochs"
    result = dict(what=what + ", one epoch, val_loader=None; median of interleaved passes", model=args.model,
                  device=torch.cuda.get_device_name(0), torch=torch.__version__, batches=args.batches,
                  passes=args.passes, size=args.size, base_filters=args.base_filters, dtype=args.dtype,
                  accumulation_steps=4, rows=rows)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
