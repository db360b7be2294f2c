"""Whole images by overlapping tiles on the GPU: rdn_tile_gather / rdn_tile_blend against
the torch restatement (tests/_tiles_ref.py) and sampling.denoise_tiled against the
samplers and the CPU oracle.

Model: RDUNet_T(base_filters=16), T = 2, B = 2, C = 3.  Shapes (H, W, tile, overlap), the
smallest that reach each branch:
  (37, 61, 32, 8)    2 x 3 grid, last origins clamped to 5 and 29
  (13, 100, 32, 16)  H reflect-padded to 16; 6 tiles on W, triple cover
  (70, 45, 32, 16)   4 tiles on H, triple cover
  (9, 9, 32, 8)      both axes padded, one tile
  (32, 95, 32, 0)    zero overlap, one doubly covered column

Bounds: the gather is a copy (bit-equal).  The blend sums at most 9 terms, each with a
couple of fp32 roundings, then one division: about 10 * 2^-24 = 6e-7, bound 1e-6 absolute
for |v| <= 1 against the fp64 restatement.  Against the CPU oracle the fp32 sampler has the
budget of tests/test_gpu_network.py::test_sampling_golden (rel-L2 1e-3; the blend adds
<= 1e-6); bf16 has the bf16 bound of tests/test_gpu_splitk.py (1e-2) against the GPU fp32
result."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

B, C, T = 2, 3, 2
SHAPES = [(37, 61, 32, 8), (13, 100, 32, 16), (70, 45, 32, 16), (9, 9, 32, 8), (32, 95, 32, 0)]
DTYPES = ["fp32", "bf16"]


def _image(H, W, seed=3, b=B):
    g = torch.Generator().manual_seed(seed + 1000 * H + W)
    return torch.rand(b, C, H, W, generator=g) * 2 - 1


def _model(dtype="fp32", seed=3):
    import vub_image_denoising_amd as vm
    from oracle.weights import make_params
    model = vm.DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=T)
    sd = model.state_dict()
    p = make_params({k[5:]: tuple(v.shape) for k, v in sd.items()}, seed=seed)
    model.load_state_dict({"unet." + k: torch.from_numpy(v) for k, v in p.items()})
    model.unet.set_compute_dtype(dtype)
    return model.cuda().eval()


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("H,W,tile,ov", SHAPES)
def test_gather_bit_equal(H, W, tile, ov):
    from vub_image_denoising_amd.sampling import tile_gather
    x = _image(H, W)
    ref = TR.gather(x, tile, ov)
    n = ref.size(0)
    xd = x.cuda()
    got = tile_gather(xd, tile, ov, 0, n)
    assert got.shape == ref.shape and torch.equal(got.cpu(), ref)
    # batches of 4 running past the end: the surplus repeats the last tile; canary behind the buffer
    for first in range(0, n + 4, 4):
        buf = torch.full((5,) + tuple(ref.shape[1:]), 7.5, device="cuda")
        tile_gather(xd, tile, ov, first, 4, out=buf[:4])
        want = torch.stack([ref[min(first + j, n - 1)] for j in range(4)])
        assert torch.equal(buf[:4].cpu(), want), first
        assert (buf[4] == 7.5).all()


@pytest.mark.parametrize("H,W,tile,ov", SHAPES)
def test_blend_random_tiles(H, W, tile, ov):
    from vub_image_denoising_amd.sampling import plan_tiles, tile_blend
    th, tw, ys, xs = plan_tiles(H, W, tile, ov)
    n = B * len(ys) * len(xs)
    g = torch.Generator().manual_seed(17 + H)
    tiles = torch.rand(n, C, th, tw, generator=g) * 2 - 1     # random contents, not crops
    ref, cnt = TR.blend(tiles, B, C, H, W, tile, ov)
    # canary-filled output with room behind [B, C, H, W]
    buf = torch.full((B * C * H * W + 4096,), -77.0, device="cuda")
    out = buf[:B * C * H * W].view(B, C, H, W)
    tile_blend(tiles.cuda(), out, tile, ov)
    assert (buf[B * C * H * W:] == -77.0).all()
    got = out.cpu()
    err = (got.double() - ref).abs().max().item()
    print(f"blend {(H, W, tile, ov)}: max abs err vs fp64 {err:.3e}, max cover {int(cnt.max())}")
    assert err <= 1e-6
    single = (cnt == 1).expand(B, C, H, W)
    assert torch.equal(got[single], ref[single].float())      # pass-through: the tile's own bits
    if len(ys) * len(xs) > 1:
        assert (cnt > 1).any()


@pytest.mark.parametrize("H,W,tile,ov", SHAPES)
def test_blend_of_gather_is_identity(H, W, tile, ov):
    from vub_image_denoising_amd.sampling import plan_tiles, tile_blend, tile_gather
    x = _image(H, W).cuda()
    th, tw, ys, xs = plan_tiles(H, W, tile, ov)
    tiles = tile_gather(x, tile, ov, 0, B * len(ys) * len(xs))
    out = tile_blend(tiles, torch.full_like(x, 9.0), tile, ov)
    err = (out - x).abs().max().item()
    print(f"identity {(H, W, tile, ov)}: max abs err {err:.3e}")
    assert err <= 1e-6


# ------------------------------------------------------------------ denoise_tiled
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("graph", [True, False])
@pytest.mark.parametrize("sampler", ["improved", "direct"])
def test_one_tile_is_the_sampler(sampler, graph, dtype):
    from vub_image_denoising_amd.sampling import denoise_tiled
    x = _image(32, 32).cuda()
    model = _model(dtype)
    y = denoise_tiled(model, x, tile=32, overlap=8, tile_batch=2, sampler=sampler, graph=graph).clone()
    ref = _model(dtype)
    with torch.no_grad():
        want = ref.improved_sampling(x) if sampler == "improved" else ref.direct_sampling(x)
    assert y.shape == x.shape and y.dtype == torch.float32
    assert torch.equal(y, want)
    assert not torch.equal(y, x)


@pytest.mark.parametrize("sampler", ["improved", "direct"])
def test_no_overlap_places_quadrants(sampler):
    from vub_image_denoising_amd.sampling import denoise_tiled
    x = _image(64, 64).cuda()
    model = _model()
    y = model.denoise_image(x, tile=32, overlap=0, tile_batch=4, sampler=sampler).clone()
    ref = _model()
    for b in range(B):
        quads = torch.stack([x[b, :, oy:oy + 32, ox:ox + 32] for oy in (0, 32) for ox in (0, 32)]).contiguous()
        with torch.no_grad():
            q = ref.improved_sampling(quads) if sampler == "improved" else ref.direct_sampling(quads)
        i = 0
        for oy in (0, 32):
            for ox in (0, 32):
                assert torch.equal(y[b, :, oy:oy + 32, ox:ox + 32], q[i]), (b, oy, ox)
                i += 1


_ORACLE = {}


def _oracle_tiled(H, W, tile, ov, sampler):
    """Per-tile CPU oracle sampler + fp64 blend, computed once per case."""
    key = (H, W, tile, ov, sampler)
    if key not in _ORACLE:
        from oracle import rdunet_ref as R
        model = _model()
        params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
        unet = lambda xx, tt: R.rdunet_t_forward(params, xx, tt, prefix="unet.")   # noqa: E731
        tiles = TR.gather(_image(H, W), tile, ov)
        with torch.no_grad():
            yt = R.improved_sampling(unet, tiles, T) if sampler == "improved" else R.direct_sampling(unet, tiles)
        _ORACLE[key] = TR.blend(yt, B, C, H, W, tile, ov)[0]
    return _ORACLE[key]


@pytest.mark.parametrize("sampler", ["improved", "direct"])
@pytest.mark.parametrize("H,W,tile,ov", [(40, 56, 32, 8), (13, 100, 32, 16)])
def test_against_cpu_oracle(H, W, tile, ov, sampler):
    from vub_image_denoising_amd.sampling import denoise_tiled
    want = _oracle_tiled(H, W, tile, ov, sampler)
    x = _image(H, W).cuda()
    y32 = denoise_tiled(_model("fp32"), x, tile=tile, overlap=ov, sampler=sampler).clone()
    r32 = _rel(y32.cpu(), want)
    y16 = denoise_tiled(_model("bf16"), x, tile=tile, overlap=ov, sampler=sampler).clone()
    r16 = _rel(y16, y32)
    print(f"tiled {sampler} {(H, W, tile, ov)}: fp32 vs oracle rel-L2 {r32:.3e}; bf16 vs GPU fp32 rel-L2 {r16:.3e}")
    assert r32 < 1e-3
    assert r16 < 1e-2


@pytest.mark.parametrize("dtype", DTYPES)
def test_last_batch_padding_and_graph_cache(monkeypatch, dtype):
    """(70, 45, 32, 16) with B = 2 has 16 tiles: tile_batch 5 ends on a batch with one real
    tile.  Split-K off: the slice count of a layer depends on the engine's batch."""
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import SamplerGraph, denoise_tiled, plan_tiles
    monkeypatch.setattr(E, "SPLITK", False)
    th, tw, ys, xs = plan_tiles(70, 45, 32, 16)
    assert B * len(ys) * len(xs) == 16
    x = _image(70, 45).cuda()
    m5 = _model(dtype)
    y5 = denoise_tiled(m5, x, tile=32, overlap=16, tile_batch=5).clone()
    y1 = denoise_tiled(_model(dtype), x, tile=32, overlap=16, tile_batch=1).clone()
    assert torch.equal(y5, y1)
    assert torch.isfinite(y5).all() and not torch.equal(y5, x)
    # a second image of another size at the same tile shape reuses the one captured sampler
    graphs = m5.unet._rdn_tile_graphs
    assert len(graphs) == 1
    sg = next(iter(graphs.values()))[1]
    assert isinstance(sg, SamplerGraph)
    x2 = _image(37, 61).cuda()
    z = denoise_tiled(m5, x2, tile=32, overlap=8, tile_batch=5).clone()
    assert len(m5.unet._rdn_tile_graphs) == 1 and next(iter(m5.unet._rdn_tile_graphs.values()))[1] is sg
    assert z.shape == x2.shape
    # one forward-only engine: the tile batch shape (2 x 5 images for the improved sampler)
    assert sorted(k[:3] for k in m5.unet._rdn_engines) == [(10, 32, 32)]
    # identical calls are bit-equal (and the first image again after another one)
    assert torch.equal(denoise_tiled(m5, x2, tile=32, overlap=8, tile_batch=5), z)
    assert torch.equal(denoise_tiled(m5, x, tile=32, overlap=16, tile_batch=5), y5)


def test_default_tile_batch_stays_below_the_chunk_threshold():
    from vub_image_denoising_amd.sampling import denoise_tiled
    x = _image(37, 61).cuda()
    m = _model()
    y = denoise_tiled(m, x, tile=32, overlap=8).clone()          # 12 tiles, one batch of 12
    assert sorted(k[:3] for k in m.unet._rdn_engines) == [(24, 32, 32)]
    yd = denoise_tiled(m, x, tile=32, overlap=8, sampler="direct").clone()
    assert sorted(k[:3] for k in m.unet._rdn_engines) == [(12, 32, 32), (24, 32, 32)]
    assert len(m.unet._rdn_tile_graphs) == 2
    assert not torch.equal(y, yd)


@pytest.mark.parametrize("graph", [True, False])
def test_weights_changed_in_place(graph):
    from vub_image_denoising_amd.sampling import denoise_tiled
    x = _image(37, 61).cuda()
    model = _model()
    y0 = denoise_tiled(model, x, tile=32, overlap=8, graph=graph).clone()
    with torch.no_grad():
        for p in model.unet.parameters():
            p.data.mul_(0.5)                 # where torch's version counters do not see it
    model.unet.mark_weights_dirty()
    y1 = denoise_tiled(model, x, tile=32, overlap=8, graph=graph).clone()
    assert not torch.equal(y1, y0)
    fresh = _model()
    fresh.load_state_dict({k: v.detach().clone() for k, v in model.state_dict().items()})
    assert torch.equal(y1, denoise_tiled(fresh, x, tile=32, overlap=8, graph=graph))


# ------------------------------------------------------------------ CLI
@pytest.mark.parametrize("form", ["epoch_dict", "bare_state_dict"])
def test_cli_round_trip(tmp_path, form):
    from PIL import Image
    from vub_image_denoising_amd import denoise_image as D
    model = _model()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ckpt = tmp_path / "ckpt.pth"
    torch.save({"epoch": 3, "model_state_dict": sd, "optimizer_state_dict": {}, "scheduler_state_dict": None}
               if form == "epoch_dict" else sd, ckpt)
    rgb = np.random.default_rng(5).integers(0, 256, size=(70, 45, 3), dtype=np.uint8)    # H = 70, W = 45
    Image.fromarray(rgb).save(tmp_path / "noisy.png")
    rc = D.main(["--checkpoint", str(ckpt), "--input", str(tmp_path / "noisy.png"), "--output", str(tmp_path / "out.png"),
                 "--base_filters", "16", "--timesteps", str(T), "--tile", "32", "--overlap", "8"])
    assert rc == 0
    with Image.open(tmp_path / "out.png") as im:
        assert im.size == (45, 70) and im.mode == "RGB"
        got = np.asarray(im).copy()
    # the same run through the Python interface, quantised the same way
    x = torch.from_numpy(rgb).permute(2, 0, 1).float().div(255.0).sub(0.5).div(0.5).unsqueeze(0).cuda()
    y = model.denoise_image(x, tile=32, overlap=8)[0].cpu().numpy()
    q = np.rint(np.clip(y * np.float32(0.5) + np.float32(0.5), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(got, q.transpose(1, 2, 0))
    assert not np.array_equal(got, rgb)
