"""Host side of whole-image tiling (no GPU): the tile grid of rdn_tile_grid against
sampling.plan_tiles and the restatement in tests/_tiles_ref.py, its coverage properties,
the argument checks of the three C entry points, and the CLI parser's defaults."""
import ctypes
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_ref as TR  # noqa: E402

TILES = (16, 32, 64)
SIZES = range(8, 141)


def _overlaps(tile):
    return (0, 8, tile // 2)


def _c_grid(lib, h, w, tile, overlap):
    out = (ctypes.c_int32 * 4)()
    rc = lib.rdn_tile_grid(h, w, tile, overlap, out)
    assert rc == 0, lib.rdn_last_error()
    return tuple(out)


def test_c_grid_equals_plan_tiles_on_a_sweep():
    from vub_image_denoising_amd import _hip as H
    from vub_image_denoising_amd.sampling import plan_tiles
    lib = H.load_library()
    n = 0
    for tile in TILES:
        for ov in _overlaps(tile):
            for h in SIZES:
                # every h against a spread of w, and the mirrored pair, so both axes see all of 8..140
                for w in list(range(8, 141, 11)) + [148 - h]:
                    for hh, ww in ((h, w), (w, h)):
                        th, tw, ys, xs = plan_tiles(hh, ww, tile, ov)
                        assert _c_grid(lib, hh, ww, tile, ov) == (th, tw, len(ys), len(xs)), (hh, ww, tile, ov)
                        n += 1
    assert n > 20000


def test_grid_properties_per_axis():
    """Every pixel covered; last origin npad - t; at most 3 tiles over a pixel; the same
    origins as the restatement written from the definition."""
    from vub_image_denoising_amd.sampling import plan_tiles
    worst = 0
    for tile in TILES:
        for ov in _overlaps(tile):
            for n in SIZES:
                th, tw, ys, xs = plan_tiles(n, 148 - n, tile, ov)
                for t, origins, ext in ((th, ys, n), (tw, xs, 148 - n)):
                    rt, npad, ro = TR.axis(ext, tile, ov)
                    assert (t, origins) == (rt, ro)
                    assert t % 8 == 0 and t <= tile and npad - ext <= 7
                    assert origins[0] == 0 and origins[-1] == npad - t
                    assert all(b > a for a, b in zip(origins, origins[1:]))
                    cover = [sum(o <= p < o + t for o in origins) for p in range(npad)]
                    assert min(cover) >= 1, (ext, tile, ov)
                    assert max(cover) <= 3, (ext, tile, ov)
                    worst = max(worst, max(cover))
    assert worst == 3       # the clamped last tile does overlap two predecessors somewhere in the sweep


def test_documented_grids():
    from vub_image_denoising_amd.sampling import plan_tiles
    assert plan_tiles(37, 61, 32, 8) == (32, 32, [0, 5], [0, 24, 29])
    assert plan_tiles(13, 100, 32, 16) == (16, 32, [0], [0, 16, 32, 48, 64, 68])
    assert plan_tiles(70, 45, 32, 16) == (32, 32, [0, 16, 32, 38], [0, 13])
    assert plan_tiles(9, 9, 32, 8) == (16, 16, [0], [0])
    assert plan_tiles(32, 95, 32, 0) == (32, 32, [0], [0, 32, 63])
    assert plan_tiles(3000, 4000, 512, 32)[:2] == (512, 512)


BAD = [  # (h, w, tile, overlap, c, name in the message)
    (64, 64, 20, 4, 3, b"tile="),
    (64, 64, 8, 0, 3, b"tile="),
    (64, 64, 0, 0, 3, b"tile="),
    (64, 64, 32, -1, 3, b"overlap="),
    (64, 64, 32, 17, 3, b"overlap="),
    (7, 64, 32, 8, 3, b"h="),
    (64, 7, 32, 8, 3, b"w="),
    (64, 64, 32, 8, 0, b"c="),
    (64, 64, 32, 8, 9, b"c="),
]


@pytest.mark.parametrize("h,w,tile,ov,c,name", BAD)
def test_invalid_arguments_fail_on_the_host(h, w, tile, ov, c, name):
    from vub_image_denoising_amd import _hip as H
    from vub_image_denoising_amd.sampling import plan_tiles
    lib = H.load_library()
    fake = 4096      # never dereferenced: the checks return before any launch
    out = (ctypes.c_int32 * 4)()
    if name != b"c=":
        assert lib.rdn_tile_grid(h, w, tile, ov, out) == -1
        assert name in lib.rdn_last_error() and b"rdn_tile_grid" in lib.rdn_last_error()
        with pytest.raises(ValueError):
            plan_tiles(h, w, tile, ov)
    assert lib.rdn_tile_gather(fake, 1, c, h, w, tile, ov, 0, 1, fake, None) == -1
    assert name in lib.rdn_last_error() and b"rdn_tile_gather" in lib.rdn_last_error()
    assert lib.rdn_tile_blend(fake, 1, c, h, w, tile, ov, fake, None) == -1
    assert name in lib.rdn_last_error() and b"rdn_tile_blend" in lib.rdn_last_error()


def test_null_pointers_and_counts_fail_on_the_host():
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    fake = 4096
    assert lib.rdn_tile_grid(64, 64, 32, 8, None) == -1 and b"out" in lib.rdn_last_error()
    assert lib.rdn_tile_gather(None, 1, 3, 64, 64, 32, 8, 0, 1, fake, None) == -1 and b"img" in lib.rdn_last_error()
    assert lib.rdn_tile_gather(fake, 1, 3, 64, 64, 32, 8, 0, 1, None, None) == -1 and b"tiles" in lib.rdn_last_error()
    assert lib.rdn_tile_blend(None, 1, 3, 64, 64, 32, 8, fake, None) == -1 and b"tiles" in lib.rdn_last_error()
    assert lib.rdn_tile_blend(fake, 1, 3, 64, 64, 32, 8, None, None) == -1 and b"out" in lib.rdn_last_error()
    assert lib.rdn_tile_gather(fake, 0, 3, 64, 64, 32, 8, 0, 1, fake, None) == -1 and b"n=" in lib.rdn_last_error()
    assert lib.rdn_tile_gather(fake, 1, 3, 64, 64, 32, 8, -1, 1, fake, None) == -1 and b"first=" in lib.rdn_last_error()
    assert lib.rdn_tile_gather(fake, 1, 3, 64, 64, 32, 8, 0, 0, fake, None) == -1 and b"count=" in lib.rdn_last_error()
    assert lib.rdn_tile_blend(fake, 0, 3, 64, 64, 32, 8, fake, None) == -1 and b"n=" in lib.rdn_last_error()


def test_denoise_tiled_needs_device_tensors():
    import torch
    import vub_image_denoising_amd as vm
    model = vm.DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=2)
    with pytest.raises(RuntimeError, match="GPU"):
        vm.denoise_tiled(model, torch.zeros(1, 3, 40, 40), tile=32, overlap=8)
    with pytest.raises(RuntimeError, match="GPU"):
        model.denoise_image(torch.zeros(1, 3, 40, 40))
    with pytest.raises(ValueError):
        vm.denoise_tiled(model, torch.zeros(1, 3, 40, 40), sampler="ddim")


def test_cli_parser_defaults():
    from vub_image_denoising_amd.denoise_image import build_parser
    a = build_parser().parse_args(["--checkpoint", "c.pth", "--input", "i.png", "--output", "o.png"])
    assert (a.checkpoint, a.input, a.output) == ("c.pth", "i.png", "o.png")
    assert (a.sampler, a.tile, a.overlap, a.dtype, a.base_filters, a.timesteps) == ("improved", 512, 32, "fp32", 32, 20)
    a = build_parser().parse_args(["--checkpoint", "c", "--input", "i", "--output", "o", "--sampler", "direct",
                                   "--dtype", "bf16", "--tile", "256", "--overlap", "16"])
    assert (a.sampler, a.dtype, a.tile, a.overlap) == ("direct", "bf16", 256, 16)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--input", "i", "--output", "o"])
