"""The cases of tests/test_gpu_pointwise_bits.py and of the recorder of its goldens
(tests/golden/make_pointwise_golden.py): the loss, clip, optimizer, EMA, SSIM, metrics and
PReLU-backward entry points of the library, called through the C ABI on inputs that no random
generator made, each result reduced to its bits.

A scalar result is its integer bit pattern (int32 for fp32, int64 for float64, a list for
several), a bulk result the sha256 of its bytes.  ``GROUPS`` maps a group's name to a function
that runs its cases on the GPU and returns ``{case: bits}``.
"""
import hashlib

import torch

M1, M2, M3 = 2654435761, 2246822519, 3266489917
SIZES = (1, 255, 10007, 2098177)      # 2098177 = 1024 * 2048 + 1025: past the reduction's block cap, odd tail
N_OPT = 10007
STEPS = 3


def seq(n, mult=M1):
    """n fp32 values in [-0.5, 0.5) from integer arithmetic alone."""
    k = (torch.arange(n, dtype=torch.int64) * mult) % 65521
    return k.float() / 65521 - 0.5


def pair(n):
    """(pred, target): target equals pred at every 7th element (L1's sign sees exact zeros)."""
    pred, target = seq(n, M1), seq(n, M2)
    target[::7] = pred[::7]
    return pred, target


def dev(values, offset=0):
    """A GPU copy of `values` at element `offset` of its allocation (1: not 16-byte aligned)."""
    whole = torch.zeros(offset + values.numel(), dtype=values.dtype, device="cuda")
    view = whole[offset:]
    view.copy_(values)
    assert (view.data_ptr() % 16 == 0) == (offset * values.element_size() % 16 == 0)
    return view


def sha(t):
    t = t.detach().cpu().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return hashlib.sha256(t.numpy().tobytes()).hexdigest()


def bits(t):
    t = t.detach().cpu().contiguous()
    v = t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).flatten().tolist()
    return v[0] if len(v) == 1 else v


def _api():
    from vub_image_denoising_amd import _hip as H
    return H, H.lib(), H.stream_ptr()


def _red_ws(lib, n):
    return torch.zeros(lib.rdn_reduce_workspace_size(n) // 4, device="cuda")


def loss_cases():
    H, lib, st = _api()
    out = {}
    for n, offset in [(n, 0) for n in SIZES] + [(10007, 1)]:
        tag = f"n{n}" + ("_off1" if offset else "")
        p, t = (dev(v, offset) for v in pair(n))
        gout = torch.full((1,), 0.75, device="cuda")
        ws, res, dp = _red_ws(lib, n), torch.zeros(2, device="cuda"), dev(torch.zeros(n), offset)
        H.check(lib.rdn_l1_fwd(p.data_ptr(), t.data_ptr(), n, ws.data_ptr(), res.data_ptr(), st), "l1_fwd")
        out[f"l1_fwd_{tag}"] = bits(res[:1])
        H.check(lib.rdn_l1_bwd(p.data_ptr(), t.data_ptr(), n, gout.data_ptr(), dp.data_ptr(), st), "l1_bwd")
        out[f"l1_bwd_{tag}"] = sha(dp)
        if offset:
            continue
        H.check(lib.rdn_charbonnier_fwd(p.data_ptr(), t.data_ptr(), n, 1e-3, ws.data_ptr(), res.data_ptr(), st), "charb_fwd")
        out[f"charbonnier_fwd_{tag}"] = bits(res)
        H.check(lib.rdn_charbonnier_bwd(p.data_ptr(), t.data_ptr(), n, 1e-3, 0.7, 0.3, gout.data_ptr(), dp.data_ptr(), st),
                "charb_bwd")
        out[f"charbonnier_bwd_{tag}"] = sha(dp)
    return out


def clip_cases():
    """The norm of a gradient in [-0.5, 0.5) is at least 0.5 * pre_scale: max_norm 1e-3 lies
    below it (the gradient is scaled down), 1e6 above it (the coefficient is pre_scale)."""
    H, lib, st = _api()
    out = {}
    for n in SIZES:
        grad = seq(n, M2)
        for pre in (1.0, 0.125):
            for max_norm in (1e-3, 1e6):
                g, ws, res = dev(grad), _red_ws(lib, n), torch.zeros(2, device="cuda")
                H.check(lib.rdn_sqnorm_scaled(g.data_ptr(), n, max_norm, pre, ws.data_ptr(), res.data_ptr(), st), "sqnorm")
                H.check(lib.rdn_clip_scale(g.data_ptr(), n, res[1:].data_ptr(), st), "clip_scale")
                tag = f"n{n}_pre{pre}_max{max_norm:g}"
                out[f"sqnorm_{tag}"] = bits(res)
                out[f"clip_{tag}"] = sha(g)
    return out


def _optim_run(kind, ema, device_counts, offset=0, wd=1e-2):
    """3 steps of one optimizer entry; the hashes of p, both state buffers and the shadow."""
    H, lib, st = _api()
    n = N_OPT
    p, s1, s2, e = dev(seq(n, M1), offset), dev(torch.zeros(n), offset), dev(torch.zeros(n), offset), dev(seq(n, M3), offset)
    grads = [dev(seq(n, M2 + 2 * k) * 0.25, offset) for k in range(STEPS)]
    step_dev = torch.ones((), dtype=torch.int64, device="cuda") if device_counts and kind != "adadelta" else None
    n_dev = torch.zeros((), dtype=torch.int64, device="cuda") if device_counts and ema else None
    for k in range(STEPS):
        ema_args = (e.data_ptr(), 0.9, 1 if device_counts else 0, k, H.ptr(n_dev)) if ema else ()
        if kind == "adadelta":
            fn = lib.rdn_adadelta_step_ema if ema else lib.rdn_adadelta_step
            rc = fn(p.data_ptr(), grads[k].data_ptr(), s1.data_ptr(), s2.data_ptr(), n, 1.0, 0.9, 1e-6, wd, 0.5, *ema_args, st)
        else:
            fn = lib.rdn_adam_step_ema if ema else lib.rdn_adam_step
            rc = fn(p.data_ptr(), grads[k].data_ptr(), s1.data_ptr(), s2.data_ptr(), n, 1e-3, 0.9, 0.999, 1e-8, wd,
                    1 if kind == "adamw" else 0, 0 if step_dev is not None else k + 1, H.ptr(step_dev), 0.5, *ema_args, st)
        H.check(rc, kind)
        for counter in (step_dev, n_dev):
            if counter is not None:
                H.check(lib.rdn_counter_inc(counter.data_ptr(), st), "counter_inc")
    return [sha(p), sha(s1), sha(s2)] + ([sha(e)] if ema else [])


def optim_cases():
    out = {}
    for kind in ("adam", "adamw", "adadelta"):
        for ema in (False, True):
            for device_counts in (False, True):
                if kind == "adadelta" and not ema and device_counts:
                    continue          # the plain Adadelta entry takes no count at all
                out[f"{kind}{'_ema' if ema else ''}_{'device' if device_counts else 'host'}"] = _optim_run(kind, ema, device_counts)
    for ema in (False, True):
        out[f"adadelta{'_ema' if ema else ''}_off1"] = _optim_run("adadelta", ema, ema, offset=1, wd=0.0)
    return out


def ema_cases():
    H, lib, st = _api()
    out = {}
    for offset in (0, 1):
        for warmup in (0, 1):
            e, p = dev(seq(N_OPT, M3), offset), dev(seq(N_OPT, M1), offset)
            n_dev = torch.full((), 2, dtype=torch.int64, device="cuda") if warmup else None
            for k in range(STEPS):
                H.check(lib.rdn_ema_update(e.data_ptr(), p.data_ptr(), N_OPT, 0.9999, warmup, k, None, st), "ema_update")
                H.check(lib.rdn_ema_update(e.data_ptr(), p.data_ptr(), N_OPT, 0.9, warmup, k, H.ptr(n_dev), st),
                        "ema_update")
                if warmup:
                    H.check(lib.rdn_counter_inc(n_dev.data_ptr(), st), "counter_inc")
            out[f"ema_update_warmup{warmup}" + ("_off1" if offset else "")] = sha(e)
    return out


def ssim_cases():
    H, lib, st = _api()
    n, c, h, w = 2, 3, 42, 43
    count = n * c * (h - 10) * (w - 10)
    x, y = (dev(v) for v in pair(n * c * h * w))
    coef, res = torch.zeros(3 * count, device="cuda"), torch.zeros(1, device="cuda")
    ws = torch.zeros(lib.rdn_ssim_workspace_size(n, c, h, w) // 4, device="cuda")
    H.check(lib.rdn_ssim_fwd(x.data_ptr(), y.data_ptr(), n, c, h, w, 1.0, coef.data_ptr(), ws.data_ptr(), res.data_ptr(), st),
            "ssim_fwd")
    return {"ssim_fwd_mean": bits(res), "ssim_fwd_coef": sha(coef)}


def metrics_cases():
    H, lib, st = _api()
    n, c, h, w = 2, 3, 40, 50
    gt, x = (dev(v) for v in pair(n * c * h * w))
    ws = torch.zeros(lib.rdn_image_metrics_workspace_size(n, c, h, w) // 8, dtype=torch.float64, device="cuda")
    psnr, ssim = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    H.check(lib.rdn_image_metrics(gt.data_ptr(), x.data_ptr(), n, c, h, w, 1.0, ws.data_ptr(), psnr.data_ptr(), ssim.data_ptr(),
                                  st), "image_metrics")
    return {"image_metrics_psnr": bits(psnr), "image_metrics_ssim": bits(ssim)}


def prelu_cases():
    H, lib, st = _api()
    n, h, w, C = 2, 16, 16, 16
    P = n * h * w
    out = {}
    for dt in (torch.bfloat16, torch.float32):
        code = H.dtype_code(dt)
        dy, pre = dev(seq(P * C, M2).to(dt)), dev(seq(P * C, M1).to(dt))
        alpha = dev(seq(C, M3) + 0.5)
        dyp = torch.zeros(P * C, dtype=dt, device="cuda")
        da, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        ws = torch.zeros(lib.rdn_prelu_bwd_workspace_size(code, P, C, C) // 4, device="cuda")
        H.check(lib.rdn_prelu_bwd(code, P, n, h, w, C, C, dy.data_ptr(), C, 0, 0, None, pre.data_ptr(), C, alpha.data_ptr(),
                                  dyp.data_ptr(), da.data_ptr(), db.data_ptr(), ws.data_ptr(), st), "prelu_bwd")
        name = "bf16" if dt == torch.bfloat16 else "f32"
        out[f"prelu_bwd_{name}"] = {"dalpha": sha(da), "dbias": sha(db), "dyp": sha(dyp)}
    return out


GROUPS = {"loss": loss_cases, "clip": clip_cases, "optim": optim_cases, "ema": ema_cases, "ssim": ssim_cases,
          "metrics": metrics_cases, "prelu": prelu_cases}
