"""The geometric self-ensemble on the GPU: rdn_tile_gather_d4 / rdn_tile_accum_d4 against
the torch restatement (tests/_tiles_ens_ref.py over tests/_tiles_ref.py) and
sampling.denoise_tiled(ensemble=n) against the composition from public pieces.

Model: RDUNet_T(base_filters=16), T = 2, B = 2, C = 3, hash weights (tests/test_gpu_tiled.py).
Shapes (H, W, tile, overlap), the smallest that reach each branch of the 32 x 32-patch kernels:
  (37, 61, 32, 8)    32 x 32 tiles, 2 x 3 grid: square, one pass
  (13, 100, 32, 16)  16 x 32 tiles, 6 per image: non-square (two passes at 8), H reflect-padded
  (9, 9, 32, 8)      16 x 16, one tile: both axes padded, tile smaller than the patch
  (45, 70, 40, 8)    40 x 40: partial patches on both axes
  (24, 100, 40, 8)   24 x 40: non-square with partial patches

Bounds.  The gather is a copy and the accumulate a fixed-order fp32 sum: bit-equal.  The
whole call: pixels under one tile are bit-equal to the composition (the sampler is
deterministic and, split-K off, independent of the batch), elsewhere the blend's own bound
of tests/test_gpu_tiled.py, 1e-6 absolute against the fp64 blend.  Equivariance: the n
members of T_e(x) are the members of x in another order, so the two means differ by two
fp32 summation orders of n-1 adds each, every partial sum at most n*M, divided by n:
2*(n-1) * 2^-24 * M with M the largest member magnitude (n = 8: 14 * 2^-24 * M = 8.4e-7 * M;
n = 2: one commutative add, the bound 2 * 2^-24 * M is met with 0)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _tiles_ens_ref as ER  # noqa: E402
import _tiles_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

B, C, T = 2, 3, 2
SHAPES = [(37, 61, 32, 8), (13, 100, 32, 16), (9, 9, 32, 8), (45, 70, 40, 8), (24, 100, 40, 8)]
PASSES = [(0, 1), (0, 2), (0, 4), (1, 3), (4, 4)]
SQUARE_PASSES = [(0, 8), (3, 4)]


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


def _sample(model, x, sampler):
    with torch.no_grad():
        return (model.improved_sampling(x) if sampler == "improved" else model.direct_sampling(x)).clone()


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("H,W,tile,ov", SHAPES)
def test_gather_d4_bit_equal(H, W, tile, ov):
    from vub_image_denoising_amd.sampling import tile_gather_d4
    x = _image(H, W)
    tiles = TR.gather(x, tile, ov)
    n, th, tw = tiles.size(0), tiles.size(2), tiles.size(3)
    xd = x.cuda()
    for d0, nd in PASSES + (SQUARE_PASSES if th == tw else []):
        ref = ER.gather_items(tiles, d0, nd)
        shape = (C, tw, th) if d0 >= 4 else (C, th, tw)
        assert tuple(ref.shape) == (n * nd,) + shape
        got = tile_gather_d4(xd, tile, ov, d0, nd, 0, n * nd)
        assert got.shape == ref.shape and torch.equal(got.cpu(), ref), (d0, nd)
        # batches of 5 running past the end: the surplus repeats the last item; canary behind the buffer
        for first in range(0, n * nd + 5, 5):
            buf = torch.full((6,) + shape, 7.5, device="cuda")
            tile_gather_d4(xd, tile, ov, d0, nd, first, 5, out=buf[:5])
            want = torch.stack([ref[min(first + j, n * nd - 1)] for j in range(5)])
            assert torch.equal(buf[:5].cpu(), want), (d0, nd, first)
            assert (buf[5] == 7.5).all(), (d0, nd, first)


@pytest.mark.parametrize("H,W,tile,ov", SHAPES)
def test_accum_d4_bit_equal(H, W, tile, ov):
    from vub_image_denoising_amd.sampling import plan_tiles, tile_accum_d4
    th, tw, ys, xs = plan_tiles(H, W, tile, ov)
    n = B * len(ys) * len(xs)
    numel = n * C * th * tw
    g = torch.Generator().manual_seed(23 + H)
    for n_ens in (1, 2, 4, 8):
        passes = ER.passes(n_ens, th, tw)
        # random sampler outputs for every work item of every pass, in the pass's tile shape
        srcs = {(d0, nd): torch.rand((n * nd, C) + ((tw, th) if d0 >= 4 else (th, tw)), generator=g) * 2 - 1
                for d0, nd in passes}
        want = torch.full((n, C, th, tw), float("nan"))
        for (d0, nd), src in srcs.items():
            ER.accumulate(want, src, d0, nd, n_ens, 0, n * nd)
        assert torch.isfinite(want).all()
        for batch in (3, 1, n * 8):
            buf = torch.full((numel + 4096,), float("nan"), device="cuda")     # d = 0 must store without reading
            buf[numel:] = -77.0
            acc = buf[:numel].view(n, C, th, tw)
            for (d0, nd), src in srcs.items():                                 # non-square at 8: both passes in sequence
                sd = src.cuda()
                for first in range(0, n * nd, batch):
                    part = torch.full((batch,) + tuple(sd.shape[1:]), float("inf"), device="cuda")   # surplus: never read
                    m = min(batch, n * nd - first)
                    part[:m] = sd[first:first + m]
                    tile_accum_d4(part, acc, d0, nd, n_ens, first, batch)
            assert (buf[numel:] == -77.0).all(), (n_ens, batch)
            assert torch.equal(acc.cpu(), want), (n_ens, batch)


def test_accum_d4_partial_pass_and_items_past_the_end():
    """A pass that does not start at d = 0 reads the stored partial sum, one that does not
    end at n_ens-1 leaves it unscaled, and a batch wholly past the end changes nothing."""
    from vub_image_denoising_amd.sampling import tile_accum_d4
    n, th, tw = 3, 40, 40
    g = torch.Generator().manual_seed(4)
    start = torch.rand(n, C, th, tw, generator=g)
    src = torch.rand(n * 4, C, th, tw, generator=g) * 2 - 1
    want = ER.accumulate(start.clone(), src, 3, 4, 8, 0, n * 4)          # d = 3..6 of 8, across the transpose
    acc = start.clone().cuda()
    tile_accum_d4(src.cuda(), acc, 3, 4, 8, 0, n * 4)
    assert torch.equal(acc.cpu(), want)
    tile_accum_d4(src.cuda(), acc, 3, 4, 8, n * 4, 5)                    # first == n_tiles*nd: surplus only
    assert torch.equal(acc.cpu(), want)
    want = ER.accumulate(start.clone(), src[:n * 2], 1, 2, 4, 0, n * 2)  # d = 1, 2 of 4: read, add, no scaling
    acc = start.clone().cuda()
    tile_accum_d4(src[:n * 2].cuda(), acc, 1, 2, 4, 0, n * 2)
    assert torch.equal(acc.cpu(), want)
    assert not torch.equal(want, start)


# ------------------------------------------------------------------ denoise_tiled(ensemble=n)
_MEMBERS = {}


def _members(H, W, tile, ov, sampler, dtype):
    """v_d = T_d^-1(sampler(T_d(tiles))) for d = 0..7 from public pieces, [8, n_tiles, C, th, tw]
    on the CPU; computed once per case and left unchanged."""
    key = (H, W, tile, ov, sampler, dtype)
    if key not in _MEMBERS:
        model = _model(dtype)
        tiles = TR.gather(_image(H, W), tile, ov)
        _MEMBERS[key] = torch.stack([ER.inverse(_sample(model, ER.transform(tiles, d).cuda(), sampler).cpu(), d)
                                     for d in range(8)])
    return _MEMBERS[key]


def _check_against_composition(monkeypatch, H, W, tile, ov, sampler, dtype, n):
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import denoise_tiled
    monkeypatch.setattr(E, "SPLITK", False)
    members = _members(H, W, tile, ov, sampler, dtype)
    n_tiles = members.size(1)
    mean = torch.stack([ER.ensemble_mean(members[:n, t]) for t in range(n_tiles)])
    want, cnt = TR.blend(mean, B, C, H, W, tile, ov)
    x = _image(H, W).cuda()
    got = denoise_tiled(_model(dtype), x, tile=tile, overlap=ov, sampler=sampler, tile_batch=n_tiles, ensemble=n).cpu()
    assert got.shape == x.shape and got.dtype == torch.float32
    single = (cnt == 1).expand(B, C, H, W)
    err = (got.double() - want).abs().max().item()
    print(f"ensemble {n} {sampler} {dtype} {(H, W, tile, ov)}: max abs err vs composition {err:.3e}, "
          f"max |v| {mean.abs().max().item():.3f}, single-cover pixels {int(single.sum())}")
    assert single.any()
    assert torch.equal(got[single], want[single].float())      # the ensemble value of the one tile, bit for bit
    assert err <= 1e-6


@pytest.mark.parametrize("n", [2, 4, 8])
@pytest.mark.parametrize("sampler", ["improved", "direct"])
@pytest.mark.parametrize("H,W,tile,ov", [(37, 61, 32, 8), (13, 100, 32, 16)])
def test_ensemble_is_the_composition(monkeypatch, H, W, tile, ov, sampler, n):
    _check_against_composition(monkeypatch, H, W, tile, ov, sampler, "fp32", n)


def test_ensemble_is_the_composition_bf16(monkeypatch):
    _check_against_composition(monkeypatch, 13, 100, 32, 16, "improved", "bf16", 8)


@pytest.mark.parametrize("H,W,tile,ov,shapes", [
    (37, 61, 32, 8, [(32, 32)]),
    (13, 100, 32, 16, [(16, 32), (32, 16)]),
])
def test_tile_batch_and_graph_cache(monkeypatch, H, W, tile, ov, shapes):
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import SamplerGraph, denoise_tiled, ensemble_passes, plan_tiles
    monkeypatch.setattr(E, "SPLITK", False)
    th, tw, ys, xs = plan_tiles(H, W, tile, ov)
    n_tiles = B * len(ys) * len(xs)
    tb = n_tiles * max(nd for _, nd in ensemble_passes(8, th, tw))          # the default: the largest pass's item count
    x = _image(H, W).cuda()
    m = _model()
    y8 = denoise_tiled(m, x, tile=tile, overlap=ov, ensemble=8).clone()
    graphs = dict(m.unet._rdn_tile_graphs)
    assert sorted(k[:3] for k in graphs) == sorted((h, w, tb) for h, w in shapes)
    assert sorted(tuple(v[1].inp.shape) for v in graphs.values()) == sorted((tb, C, h, w) for h, w in shapes)
    assert all(isinstance(v[1], SamplerGraph) for v in graphs.values())
    # one forward-only engine per tile shape (2 x tb images for the improved sampler)
    assert sorted(k[:3] for k in m.unet._rdn_engines) == sorted((2 * tb, h, w) for h, w in shapes)
    # a second call reuses every captured graph and gives the same bits
    assert torch.equal(denoise_tiled(m, x, tile=tile, overlap=ov, ensemble=8), y8)
    again = m.unet._rdn_tile_graphs
    assert set(again) == set(graphs) and all(again[k][1] is graphs[k][1] for k in graphs)
    assert torch.isfinite(y8).all()
    # the result does not depend on how the batches cut the work items
    for batch in (1, 3):
        assert torch.equal(denoise_tiled(m, x, tile=tile, overlap=ov, ensemble=8, tile_batch=batch), y8), batch
    assert torch.equal(denoise_tiled(m, x, tile=tile, overlap=ov, ensemble=8, graph=False), y8)


def test_ensemble_1_is_the_plain_call(monkeypatch):
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import denoise_tiled
    monkeypatch.setattr(E, "SPLITK", False)
    x = _image(37, 61).cuda()
    m = _model()
    y1 = denoise_tiled(m, x, tile=32, overlap=8).clone()
    assert torch.equal(denoise_tiled(m, x, tile=32, overlap=8, ensemble=1), y1)
    assert len(m.unet._rdn_tile_graphs) == 1                # the same captured sampler, nothing new
    y2 = denoise_tiled(m, x, tile=32, overlap=8, ensemble=2).clone()
    y8 = denoise_tiled(m, x, tile=32, overlap=8, ensemble=8).clone()
    assert not torch.equal(y2, y1) and not torch.equal(y8, y1) and not torch.equal(y8, y2)


@pytest.mark.parametrize("n", [2, 4, 8])
def test_equivariance_on_one_square_tile(monkeypatch, n):
    from vub_image_denoising_amd import engine as E
    from vub_image_denoising_amd.sampling import denoise_tiled
    monkeypatch.setattr(E, "SPLITK", False)
    x = _image(32, 32)
    ref = _model()
    M = max(_sample(ref, ER.transform(x, d).cuda(), "improved").abs().max().item() for d in range(n))
    bound = 2 * (n - 1) * 2.0 ** -24 * M
    m = _model()
    base = denoise_tiled(m, x.cuda(), tile=32, overlap=8, ensemble=n).cpu()
    assert not torch.equal(base, _sample(ref, x.cuda(), "improved").cpu())
    for e in ([1] if n == 2 else range(n)):
        got = denoise_tiled(m, ER.transform(x, e).cuda(), tile=32, overlap=8, ensemble=n).cpu()
        err = (got.double() - ER.transform(base, e).double()).abs().max().item()
        print(f"equivariance n={n} e={e}: max abs err {err:.3e}, bound {bound:.3e} (M = {M:.3f})")
        assert err <= bound, (n, e)
    assert len(m.unet._rdn_tile_graphs) == 1


# ------------------------------------------------------------------ CLI
def test_cli_ensemble(tmp_path):
    from PIL import Image
    from vub_image_denoising_amd import denoise_image as D
    model = _model()
    ckpt = tmp_path / "ckpt.pth"
    torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, ckpt)
    rgb = np.random.default_rng(5).integers(0, 256, size=(70, 45, 3), dtype=np.uint8)    # H = 70, W = 45
    Image.fromarray(rgb).save(tmp_path / "noisy.png")
    outs = {}
    for n in (8, 1):
        rc = D.main(["--checkpoint", str(ckpt), "--input", str(tmp_path / "noisy.png"), "--output",
                     str(tmp_path / f"out{n}.png"), "--base_filters", "16", "--timesteps", str(T), "--tile", "32",
                     "--overlap", "8", "--ensemble", str(n)])
        assert rc == 0
        with Image.open(tmp_path / f"out{n}.png") as im:
            assert im.size == (45, 70) and im.mode == "RGB"
            outs[n] = np.asarray(im).copy()
    x = torch.from_numpy(rgb).permute(2, 0, 1).float().div(255.0).sub(0.5).div(0.5).unsqueeze(0).cuda()
    y = model.denoise_image(x, tile=32, overlap=8, ensemble=8)[0].cpu().numpy()
    q = np.rint(np.clip(y * np.float32(0.5) + np.float32(0.5), 0.0, 1.0) * np.float32(255.0)).astype(np.uint8)
    assert np.array_equal(outs[8], q.transpose(1, 2, 0))
    assert not np.array_equal(outs[8], outs[1])
