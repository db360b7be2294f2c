"""Whole-image tiled denoising, measured (no threshold): one 3000 x 4000 image in bf16,
improved sampler at T = 20, default tile and overlap (sampling.denoise_tiled).

    python scripts/tiled_bench.py [--height 3000 --width 4000 --repeats 5 --warmup 2]
    python scripts/tiled_bench.py --ensemble 8 [--block 256]

Prints one JSON line: Mpx/s of the whole call, the share of its time spent in
rdn_tile_gather + rdn_tile_blend, and the tile sampler's own time at the same batch shape.
Every time is a median of ``repeats`` device-event timings after ``warmup`` untimed runs.

``--ensemble N`` (2, 4, 8) measures the geometric self-ensemble instead: the whole call at
``ensemble=N`` and at ``ensemble=1`` timed in alternation, their ratio, and the share of the
ensemble call spent in rdn_tile_gather_d4 + rdn_tile_accum_d4 (all batches of all passes,
timed on their own).  ``--block S`` adds the single-block case (one S x S image is one tile):
one ``ensemble=N`` call, which packs the N transforms into one sampler batch, against N
``ensemble=1`` calls on explicitly transformed inputs (with and without the torch flips /
transposes and the mean around them), the three timed in alternation."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e)


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = [_timed(fn) for _ in range(repeats)]
    return statistics.median(times), min(times), max(times)


def interleaved_ms(fns, warmup, repeats):
    """``median_ms`` of several variants whose timed runs alternate (a, b, a, b, ...), so a
    drift of the machine falls on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            times[k].append(_timed(fn))
    return {k: (statistics.median(t), min(t), max(t)) for k, t in times.items()}


def _spread(t):
    return {"median": round(t[0], 2), "min": round(t[1], 2), "max": round(t[2], 2)}


def _d4(u, d):
    """T_d of include/rdunet_hip.h in torch: flips, then the transpose."""
    if d & 1:
        u = u.flip(-1)
    if d & 2:
        u = u.flip(-2)
    return u.transpose(-1, -2) if d & 4 else u


def _d4_inverse(v, d):
    if d & 4:
        v = v.transpose(-1, -2)
    if d & 2:
        v = v.flip(-2)
    return v.flip(-1) if d & 1 else v


def measure_ensemble(a, model, x):
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import (denoise_tiled, ensemble_passes, plan_tiles, tile_accum_d4, tile_blend,
                                                  tile_gather_d4)
    n = a.ensemble
    kw = dict(tile=a.tile, overlap=a.overlap, sampler=a.sampler)
    th, tw, ys, xs = plan_tiles(a.height, a.width, a.tile, a.overlap)
    n_tiles = len(ys) * len(xs)
    passes = ensemble_passes(n, th, tw)
    k = 2 if a.sampler == "improved" else 1
    tb = max(1, min(n_tiles * max(nd for _, nd in passes), E.FWD_CHUNK_PIXELS // (k * th * tw)))   # denoise_tiled's default
    whole = interleaved_ms({"ens1": lambda: denoise_tiled(model, x, **kw),
                            "ensN": lambda: denoise_tiled(model, x, ensemble=n, **kw)}, a.warmup, a.repeats)
    tout = torch.empty(n_tiles, 3, th, tw, device="cuda")
    out = torch.empty_like(x)
    bufs = {d0: (torch.empty((tb, 3, tw, th) if d0 >= 4 else (tb, 3, th, tw), device="cuda"),
                 torch.rand((tb, 3, tw, th) if d0 >= 4 else (tb, 3, th, tw), device="cuda")) for d0, _ in passes}

    def gather_all():
        for d0, nd in passes:
            for first in range(0, n_tiles * nd, tb):
                tile_gather_d4(x, a.tile, a.overlap, d0, nd, first, tb, out=bufs[d0][0])

    def accum_all():
        for d0, nd in passes:
            for first in range(0, n_tiles * nd, tb):
                tile_accum_d4(bufs[d0][1], tout, d0, nd, n, first, tb)

    gather = median_ms(gather_all, a.warmup, a.repeats)
    accum = median_ms(accum_all, a.warmup, a.repeats)
    blend = median_ms(lambda: tile_blend(tout, out, a.tile, a.overlap), a.warmup, a.repeats)
    px = a.height * a.width
    items = sum(n_tiles * nd for _, nd in passes)
    # gather read+write; accumulate: src read, acc written once per tile and batch (approx.: whole tiles per batch)
    moved = 4 * 3 * th * tw * (2 * items + items + n_tiles)
    res = {
        "image": [a.height, a.width], "dtype": a.dtype, "sampler": a.sampler, "timesteps": a.timesteps,
        "tile": [th, tw], "overlap": a.overlap, "tiles": n_tiles, "ensemble": n, "passes": passes,
        "tile_batch": tb, "batches": sum(-(-n_tiles * nd // tb) for _, nd in passes),
        "graphs": len(model.unet._rdn_tile_graphs),
        "whole_ms": _spread(whole["ensN"]), "whole_ms_ensemble1": _spread(whole["ens1"]),
        "ratio_to_ensemble1": round(whole["ensN"][0] / whole["ens1"][0], 4),
        "mpx_per_s": round(px / 1e6 / (whole["ensN"][0] / 1e3), 3),
        "gather_d4_all_ms": round(gather[0], 4), "accum_d4_all_ms": round(accum[0], 4), "blend_ms": round(blend[0], 4),
        "d4_share": round((gather[0] + accum[0]) / whole["ensN"][0], 6),
        "d4_gb_per_s": round(moved / 1e9 / ((gather[0] + accum[0]) / 1e3), 1),
        "repeats": a.repeats, "warmup": a.warmup,
    }
    if a.block:
        res["block"] = measure_block(a, model)
    return res


def measure_block(a, model):
    """One S x S block (one tile): the packed ensemble call against N plain calls."""
    from vub_image_denoising_amd.sampling import denoise_tiled
    n, s = a.ensemble, a.block
    kw = dict(tile=a.tile, overlap=a.overlap, sampler=a.sampler)
    xb = torch.rand(1, 3, s, s, device="cuda") * 2 - 1
    pre = [_d4(xb, d).contiguous() for d in range(n)]

    def calls():
        for t in pre:
            denoise_tiled(model, t, **kw)

    def loop():
        acc = None
        for d in range(n):
            v = _d4_inverse(denoise_tiled(model, _d4(xb, d).contiguous(), **kw), d)
            acc = v.clone() if acc is None else acc.add_(v)
        return acc.mul_(1.0 / n)

    t = interleaved_ms({"packed": lambda: denoise_tiled(model, xb, ensemble=n, **kw), "calls": calls, "loop": loop},
                       a.warmup, a.block_repeats)
    return {"size": s, "ensemble": n, "repeats": a.block_repeats,
            "one_call_ms": _spread(t["packed"]), "n_calls_ms": _spread(t["calls"]), "torch_loop_ms": _spread(t["loop"]),
            "gain_over_n_calls": round(t["calls"][0] / t["packed"][0], 3),
            "gain_over_torch_loop": round(t["loop"][0] / t["packed"][0], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=3000)
    ap.add_argument("--width", type=int, default=4000)
    ap.add_argument("--tile", type=int, default=512)
    ap.add_argument("--overlap", type=int, default=32)
    ap.add_argument("--timesteps", type=int, default=20)
    ap.add_argument("--base_filters", type=int, default=32)
    ap.add_argument("--dtype", default="bf16", choices=["fp32", "bf16"])
    ap.add_argument("--sampler", default="improved", choices=["improved", "direct"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--ensemble", type=int, default=1, choices=[1, 2, 4, 8])
    ap.add_argument("--block", type=int, default=0, help="with --ensemble: also time one block of this size (e.g. 256)")
    ap.add_argument("--block_repeats", type=int, default=11)
    a = ap.parse_args(argv)
    if a.block and a.ensemble == 1:
        ap.error("--block needs --ensemble 2, 4 or 8")
    if not torch.cuda.is_available():
        raise RuntimeError("tiled_bench measures on the GPU; no device found")
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import denoise_tiled, plan_tiles, tile_blend, tile_gather

    torch.manual_seed(7)
    unet = vm.RDUNet_T(base_filters=a.base_filters)
    unet.set_compute_dtype(a.dtype)
    model = vm.DiffusionModel(unet, timesteps=a.timesteps).cuda().eval()
    x = torch.rand(1, 3, a.height, a.width, device="cuda") * 2 - 1
    if a.ensemble > 1:
        res = measure_ensemble(a, model, x)
        print(json.dumps(res))
        return res
    th, tw, ys, xs = plan_tiles(a.height, a.width, a.tile, a.overlap)
    n_tiles = len(ys) * len(xs)
    k = 2 if a.sampler == "improved" else 1
    tb = max(1, min(n_tiles, E.FWD_CHUNK_PIXELS // (k * th * tw)))      # denoise_tiled's default
    batches = -(-n_tiles // tb)

    whole = median_ms(lambda: denoise_tiled(model, x, tile=a.tile, overlap=a.overlap, sampler=a.sampler),
                      a.warmup, a.repeats)

    tin = torch.empty(tb, 3, th, tw, device="cuda")
    tout = torch.rand(n_tiles, 3, th, tw, device="cuda")
    out = torch.empty_like(x)

    def gather_all():
        for first in range(0, n_tiles, tb):
            tile_gather(x, a.tile, a.overlap, first, tb, out=tin)

    gather = median_ms(gather_all, a.warmup, a.repeats)
    blend = median_ms(lambda: tile_blend(tout, out, a.tile, a.overlap), a.warmup, a.repeats)
    graphs = list(model.unet._rdn_tile_graphs.values())
    assert len(graphs) == 1, "one captured sampler serves the whole image"
    sg = graphs[0][1]
    sampler = median_ms(lambda: sg(tin), a.warmup, a.repeats)

    px = a.height * a.width
    moved = 4 * 3 * (2 * n_tiles * th * tw + px) + 4 * 3 * px      # gather read+write, blend read+write (approx.)
    res = {
        "image": [a.height, a.width], "dtype": a.dtype, "sampler": a.sampler, "timesteps": a.timesteps,
        "tile": [th, tw], "overlap": a.overlap, "tiles": n_tiles, "tile_batch": tb, "batches": batches,
        "whole_ms": {"median": round(whole[0], 2), "min": round(whole[1], 2), "max": round(whole[2], 2)},
        "mpx_per_s": round(px / 1e6 / (whole[0] / 1e3), 3),
        "gather_all_ms": round(gather[0], 4), "blend_ms": round(blend[0], 4),
        "gather_blend_share": round((gather[0] + blend[0]) / whole[0], 6),
        "gather_blend_gb_per_s": round(moved / 1e9 / ((gather[0] + blend[0]) / 1e3), 1),
        "tile_sampler_ms_per_batch": round(sampler[0], 2),
        "tile_sampler_ms_all_batches": round(sampler[0] * batches, 2),
        "tile_sampler_share": round(sampler[0] * batches / whole[0], 4),
        "repeats": a.repeats, "warmup": a.warmup,
    }
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
