"""Device time of the SSIM loss term: forward + backward at 16 x 3 x 256^2 through the
fused pair (rdn_ssim_fwd + rdn_ssim_bwd) and through the torch-op ``functional.ssim``
with autograd, and the captured B16 256^2 bf16 train step (train_graph.TrainStepGraph)
with the loss weights (0, 1, 0) and (0, 0.84, 0.16).  hipEvents, 10 warm-up then 50
timed calls each.

    python scripts/ssim_kbench.py [out.json]      (default profiles/ssim_kbench.json)
"""
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

WARMUP, TIMED = 10, 50
SHAPE = (16, 3, 256, 256)
MIXES = ((0.0, 1.0, 0.0), (0.0, 0.84, 0.16))


def timed_us(fn):
    """Mean and minimum device time of one call: per-call hipEvent pairs."""
    for _ in range(WARMUP):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(TIMED)]
    torch.cuda.synchronize()
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    t = [1e3 * s.elapsed_time(e) for s, e in ev]
    return {"mean_us": round(sum(t) / len(t), 2), "min_us": round(min(t), 2), "median_us": round(sorted(t)[len(t) // 2], 2)}


def loss_pair():
    from vub_image_denoising_amd import _hip as H
    from vub_image_denoising_amd import functional as Fn
    lib = H.lib()
    g = torch.Generator(device="cuda").manual_seed(0)
    clean = torch.rand(SHAPE, device="cuda", generator=g) * 2 - 1
    pred = clean + 0.2 * torch.randn(SHAPE, device="cuda", generator=g)
    n, c, h, w = SHAPE
    ws = torch.empty(lib.rdn_ssim_workspace_size(n, c, h, w) // 4, device="cuda")
    coef = torch.empty((3, n, c, h - 10, w - 10), device="cuda")
    out = torch.empty(1, device="cuda")
    gout = torch.ones(1, device="cuda")
    dx = torch.empty_like(pred)
    st = H.stream_ptr()

    def fwd():
        H.check(lib.rdn_ssim_fwd(pred.data_ptr(), clean.data_ptr(), n, c, h, w, 1.0, coef.data_ptr(), ws.data_ptr(),
                                 out.data_ptr(), st), "ssim_fwd")

    def bwd():
        H.check(lib.rdn_ssim_bwd(pred.data_ptr(), clean.data_ptr(), coef.data_ptr(), n, c, h, w, 1.0, gout.data_ptr(),
                                 dx.data_ptr(), 0, st), "ssim_bwd")

    def fused():
        fwd()
        bwd()

    def fused_autograd():      # the same two launches through ssim_fused (allocations and autograd included)
        x = pred.detach().requires_grad_(True)
        Fn.ssim_fused(x, clean).backward()

    def torch_ops():
        x = pred.detach().requires_grad_(True)
        Fn.ssim(x, clean, data_range=1.0).backward()

    r = {"shape": list(SHAPE)}
    for name, fn in (("fused_fwd", fwd), ("fused_bwd", bwd), ("fused_pair", fused), ("fused_autograd", fused_autograd),
                     ("torch_ops", torch_ops)):
        r[name] = timed_us(fn)
        print(json.dumps({name: r[name]}), flush=True)
    r["torch_over_fused"] = round(r["torch_ops"]["mean_us"] / r["fused_pair"]["mean_us"], 1)
    return r


def step(weights):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    from vub_image_denoising_amd.optim import FusedAdamW
    from vub_image_denoising_amd.train_graph import TrainStepGraph
    torch.manual_seed(0)
    unet = vm.RDUNet_T(base_filters=32).cuda().set_compute_dtype("bf16")
    model = DiffusionModel(unet, timesteps=20).cuda()
    opt = FusedAdamW(model.parameters(), lr=1e-4, weight_decay=1e-4)
    clean = torch.rand(SHAPE, device="cuda") * 2 - 1
    noisy = clean + 0.2 * torch.randn(SHAPE, device="cuda")
    g = TrainStepGraph(model, opt, SHAPE, 'uniform', 1.0, loss_weights=weights)
    r = timed_us(lambda: g(clean, noisy))
    r.update(loss_weights=list(weights), graph_nodes=g.graph_nodes, loss=round(g.loss.item(), 6))
    print(json.dumps({"step": r}), flush=True)
    return r


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "profiles", "ssim_kbench.json")
    res = {"device": torch.cuda.get_device_name(0), "warmup": WARMUP, "timed": TIMED, "loss": loss_pair(),
           "step_b16_256_bf16": [step(w) for w in MIXES]}
    a, b = (s["mean_us"] for s in res["step_b16_256_bf16"])
    res["step_delta_us"] = round(b - a, 1)
    print(json.dumps(res))
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
