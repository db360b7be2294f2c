"""Whole-image tiled denoising, measured (no threshold): one 3000 x 4000 image in bf16,
improved sampler at T = 20, default tile and overlap (sampling.denoise_tiled).

    python scripts/tiled_bench.py [--height 3000 --width 4000 --repeats 5 --warmup 2]

Prints one JSON line: Mpx/s of the whole call, the share of its time spent in
rdn_tile_gather + rdn_tile_blend, and the tile sampler's own time at the same batch shape.
Every time is a median of ``repeats`` device-event timings after ``warmup`` untimed runs."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e))
    return statistics.median(times), min(times), max(times)


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
    a = ap.parse_args(argv)
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
