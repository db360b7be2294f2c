"""Reverse-diffusion samplers on the GPU.

``improved_sampling`` restates ``DiffusionModel.improved_sampling``
(diffusion_denoising/diffusion_RDUnet.py:38-50): for t = T..1 two UNet calls on
the same x_t at t/T and (t-1)/T, then
``x_t = x_t - ((1-a)*f1 + a*y) + ((1-a')*f2 + a'*y)`` — one fused
``rdn_sampling_combine`` launch per step.

MI355X-first changes, each bit-exact:

* the two calls of a step read the same x_t, so they run as ONE UNet call of
  batch 2B (x_t twice, t = [a]*B + [a']*B): images never interact in the
  network (no batch statistics) and every conv's per-pixel summation order is
  fixed, so each half equals the separate call bit for bit — and a batch-1
  sampler keeps twice the CUs busy;
* the t scalars live in small device tables (no per-step host->device copies),
  so the whole loop is a fixed launch sequence ``SamplerGraph`` captures into
  one hipGraph;
* optional ``skip_zero_weight``: at t = T the reference multiplies f1 by
  (1 - a) = 0 (:45); skipping that call changes nothing unless f1 is not finite.

``denoise_tiled`` (no reference counterpart) runs either sampler over whole images of
any size: overlapping tiles of one fixed shape through one captured SamplerGraph,
gathered and blended by ``rdn_tile_gather`` / ``rdn_tile_blend``.  With
``ensemble`` > 1 each tile is denoised under 2, 4 or 8 flips / transposes sharing sampler
batches, transformed and averaged by ``rdn_tile_gather_d4`` / ``rdn_tile_accum_d4``.
"""
from __future__ import annotations

import torch

from . import _hip as H
from . import engine as E
from . import functional as Fn


_TABLES = {}


def _t_table(T, dev):
    # t/T rounded from double exactly as torch.tensor([t / T]) does (:43,:46);
    # cached so a graph capture never issues a host->device copy
    key = (T, str(dev))
    tab = _TABLES.get(key)
    if tab is None:
        tab = _TABLES[key] = torch.tensor([t / T for t in range(T + 1)], dtype=torch.float32, device=dev)
    return tab


def _t_pairs(T, B, dev):
    """row t: [t/T]*B + [(t-1)/T]*B as a [2B, 1, 1, 1] per-image t tensor."""
    key = ("pairs", T, B, str(dev))
    tab = _TABLES.get(key)
    if tab is None:
        rows = [[t / T] * B + [(t - 1) / T] * B for t in range(1, T + 1)]
        tab = torch.tensor([[0.0] * 2 * B] + rows, dtype=torch.float32, device=dev).view(T + 1, 2 * B, 1, 1, 1)
        _TABLES[key] = tab
    return tab


def improved_sampling(model, noisy_image: torch.Tensor, batched: bool = True,
                      skip_zero_weight: bool = False) -> torch.Tensor:
    T = model.timesteps
    y = noisy_image.contiguous().float()
    B = y.size(0)
    tt = _t_table(T, y.device)
    if not batched:
        x_t = y.clone()
        for t in reversed(range(1, T + 1)):
            a, ap = t / T, (t - 1) / T
            f1 = model.unet(x_t, tt[t].view(1, 1, 1, 1))
            f2 = model.unet(x_t, tt[t - 1].view(1, 1, 1, 1))
            Fn.sampling_combine(x_t, f1, f2, y, a, ap)
        return x_t
    tp = _t_pairs(T, B, y.device)
    x2 = torch.empty((2 * B,) + tuple(y.shape[1:]), dtype=torch.float32, device=y.device)
    x_t = x2[:B]
    x_t.copy_(y)
    for t in reversed(range(1, T + 1)):
        a, ap = t / T, (t - 1) / T
        if skip_zero_weight and t == T:
            f2 = model.unet(x_t, tt[t - 1].view(1, 1, 1, 1))
            Fn.sampling_combine(x_t, f2, f2, y, a, ap)     # (1 - a) = 0 multiplies the skipped f1
            continue
        x2[B:].copy_(x_t)
        out = model.unet(x2, tp[t])
        Fn.sampling_combine(x_t, out[:B], out[B:], y, a, ap)
    return x_t


class SamplerGraph:
    """hipGraph capture of the full improved_sampling (or direct_sampling) loop
    for a fixed input shape: one host launch per call after capture."""

    def __init__(self, model, shape, direct=False, batched=True, skip_zero_weight=False):
        self.model = model
        self.direct = direct
        self.batched = batched
        self.skip = skip_zero_weight
        dev = next(model.parameters()).device
        self.inp = torch.zeros(shape, dtype=torch.float32, device=dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(s):
            for _ in range(2):  # warm up: engines, packs, workspaces allocated outside capture
                self._body()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = self._body()

    def _body(self):
        if self.direct:
            return self.model.unet(self.inp, _t_table(1, self.inp.device)[1].view(1, 1, 1, 1))
        return improved_sampling(self.model, self.inp, self.batched, self.skip)

    def __call__(self, noisy_image):
        self.inp.copy_(noisy_image)
        for packs in self.model.unet._rdn_packs.values():  # weights changed since capture -> repack first
            packs.refresh()
        self.graph.replay()
        return self.out


# ----------------------------------------------------------------- whole images by tiles
def _plan_axis(n, tile, overlap):
    """One axis of the tile grid (include/rdunet_hip.h, rdn_tile_grid): tile extent and origins."""
    t = min(tile, (n + 7) // 8 * 8)
    npad = max(n, t)
    if npad == t:
        return t, [0]
    s = t - overlap
    k = -((t - npad) // s)            # ceil((npad - t) / s)
    return t, [min(i * s, npad - t) for i in range(k + 1)]


def plan_tiles(H, W, tile, overlap):
    """The tile grid of an H x W image: ``th, tw, ys, xs`` -- the tile shape and the tiles'
    row / column origins in the image padded (reflect, bottom / right) to at least one tile.
    The same definition as ``rdn_tile_grid``; tile ``(ky, kx)`` of image ``b`` has the
    global index ``(b*len(ys) + ky)*len(xs) + kx``."""
    if tile % 8 or tile < 16:
        raise ValueError(f"tile must be a multiple of 8 and >= 16, got {tile}")
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f"overlap must be in [0, tile/2], got {overlap} for tile {tile}")
    if H < 8 or W < 8:
        raise ValueError(f"image must be at least 8x8, got {H}x{W}")
    th, ys = _plan_axis(H, tile, overlap)
    tw, xs = _plan_axis(W, tile, overlap)
    return th, tw, ys, xs


def tile_gather(img, tile, overlap, first, count, out=None):
    """Tiles ``first .. first+count-1`` of ``img`` [B,C,H,W] as [count,C,th,tw]; an index
    past the last tile repeats the last tile (``rdn_tile_gather``)."""
    H.require_device(img)
    B, C, Hh, Ww = img.shape
    th, tw, _, _ = plan_tiles(Hh, Ww, tile, overlap)
    if out is None:
        out = torch.empty((count, C, th, tw), dtype=torch.float32, device=img.device)
    H.check(H.lib().rdn_tile_gather(img.data_ptr(), B, C, Hh, Ww, tile, overlap, first, count, out.data_ptr(),
                                    H.stream_ptr()), "tile_gather")
    return out


def tile_blend(tiles, out, tile, overlap):
    """Blend all tiles [B*ny*nx,C,th,tw] of the grid of ``out`` [B,C,H,W] into ``out``
    (``rdn_tile_blend``)."""
    H.require_device(tiles, out)
    B, C, Hh, Ww = out.shape
    th, tw, ys, xs = plan_tiles(Hh, Ww, tile, overlap)
    if tuple(tiles.shape) != (B * len(ys) * len(xs), C, th, tw):
        raise RuntimeError(f"tile_blend: expected tiles {(B * len(ys) * len(xs), C, th, tw)}, got {tuple(tiles.shape)}")
    H.check(H.lib().rdn_tile_blend(tiles.data_ptr(), B, C, Hh, Ww, tile, overlap, out.data_ptr(), H.stream_ptr()),
            "tile_blend")
    return out


ENSEMBLES = (1, 2, 4, 8)


def ensemble_passes(ensemble, th, tw):
    """The passes ``(d0, nd)`` of a geometric self-ensemble on th x tw tiles: transforms
    ``d0 .. d0+nd-1`` share one tile shape (``include/rdunet_hip.h``, rdn_tile_gather_d4)."""
    if th == tw:
        return [(0, ensemble)]
    return [(0, min(ensemble, 4))] + ([(4, 4)] if ensemble == 8 else [])


def tile_gather_d4(img, tile, overlap, d0, nd, first, count, out=None):
    """Work items ``first .. first+count-1`` of the pass ``(d0, nd)`` over the tiles of
    ``img`` [B,C,H,W]: item ``g*nd + (d - d0)`` is tile ``g`` under transform ``d``, as
    [count,C,th,tw] ([count,C,tw,th] for ``d0 >= 4``); an item past the last repeats the
    last (``rdn_tile_gather_d4``)."""
    H.require_device(img)
    B, C, Hh, Ww = img.shape
    th, tw, _, _ = plan_tiles(Hh, Ww, tile, overlap)
    if out is None:
        shape = (count, C, tw, th) if d0 >= 4 else (count, C, th, tw)
        out = torch.empty(shape, dtype=torch.float32, device=img.device)
    H.check(H.lib().rdn_tile_gather_d4(img.data_ptr(), B, C, Hh, Ww, tile, overlap, d0, nd, first, count, out.data_ptr(),
                                       H.stream_ptr()), "tile_gather_d4")
    return out


def tile_accum_d4(src, acc, d0, nd, n_ens, first, count=None):
    """Map the sampler outputs ``src`` of work items ``first .. first+count-1`` of the pass
    ``(d0, nd)`` back and add them into the running ensemble mean ``acc`` [n_tiles,C,th,tw]
    in ascending ``d`` (``rdn_tile_accum_d4``).  ``count`` defaults to ``src.size(0)``."""
    H.require_device(src, acc)
    n_tiles, C, th, tw = acc.shape
    count = src.size(0) if count is None else count
    want = (C, tw, th) if d0 >= 4 else (C, th, tw)
    if src.dim() != 4 or tuple(src.shape[1:]) != want or src.size(0) < count:
        raise RuntimeError(f"tile_accum_d4: expected src [>= {count}, {want}], got {tuple(src.shape)}")
    if src.dtype != torch.float32 or acc.dtype != torch.float32 or not (src.is_contiguous() and acc.is_contiguous()):
        raise RuntimeError("tile_accum_d4: src and acc must be contiguous fp32")
    H.check(H.lib().rdn_tile_accum_d4(src.data_ptr(), acc.data_ptr(), n_tiles, C, th, tw, d0, nd, n_ens, first, count,
                                      H.stream_ptr()), "tile_accum_d4")
    return acc


def _tile_sampler(model, shape, sampler, graph):
    """The sampler for tile batches of ``shape``: eager, or the model's cached SamplerGraph."""
    direct = sampler == "direct"
    if not graph:
        return model.direct_sampling if direct else (lambda x: improved_sampling(model, x))
    unet = model.unet
    E.flat_params(unet, next(unet.parameters()).device)     # (re)creates the runtime state if it is stale
    cache = unet.__dict__.setdefault("_rdn_tile_graphs", {})
    # what a capture depends on besides the tile batch shape and the sampler
    key = (shape[2], shape[3], shape[0], sampler, shape[1], model.timesteps, unet.compute_dtype, unet.training)
    hit = cache.get(key)
    if hit is None or hit[0] is not unet._rdn_flat or hit[1].model is not model:
        hit = cache[key] = (unet._rdn_flat, SamplerGraph(model, shape, direct=direct))
    return hit[1]


def denoise_tiled(model, noisy, *, tile=512, overlap=32, sampler="improved", tile_batch=None, graph=True,
                  ensemble=1):
    """Denoise whole images of any size H, W >= 8: ``noisy`` [B,C,H,W] (device, fp32) is cut
    into overlapping tiles of one shape (``plan_tiles``), ``tile_batch`` tiles at a time go
    through the sampler (``improved_sampling`` or ``direct_sampling``), and the results are
    blended back with a linear ramp over the overlap.  One engine and -- with ``graph`` --
    one captured SamplerGraph, kept on the model, serve every image size; memory is bounded
    by the tile batch.  A region covered by one tile is that tile's sampler output bit for
    bit.  Tiling is not the untiled network: the receptive field is far wider than the
    overlap, so results differ from an untiled run wherever there is more than one tile.

    ``ensemble`` in {1, 2, 4, 8}: the geometric self-ensemble.  Every tile goes through the
    sampler under the first ``ensemble`` flips / transposes of the square (2: identity and
    x-flip, 4: the four flips, 8: all of D4) and the results, mapped back, are averaged in
    fp32 in a fixed order before the blend (``rdn_tile_gather_d4`` / ``rdn_tile_accum_d4``,
    DESIGN.md 3.2).  ``tile_batch`` then counts work items (tile, transform), the transforms
    of a tile being adjacent, and the result does not depend on it.  Non-square tiles at
    ``ensemble=8`` run a second pass on transposed tiles: one more engine and one more
    captured graph.  ``ensemble=1`` is the plain path, launch for launch."""
    if sampler not in ("improved", "direct"):
        raise ValueError(f"sampler must be 'improved' or 'direct', got {sampler!r}")
    if ensemble not in ENSEMBLES:
        raise ValueError(f"ensemble must be one of {ENSEMBLES}, got {ensemble!r}")
    if not isinstance(noisy, torch.Tensor) or noisy.dim() != 4:
        raise RuntimeError("denoise_tiled: expected a [B,C,H,W] tensor")
    H.require_device(noisy, next(model.parameters()))
    x = noisy.contiguous().float()
    B, C, Hh, Ww = x.shape
    th, tw, ys, xs = plan_tiles(Hh, Ww, tile, overlap)
    n_tiles = B * len(ys) * len(xs)
    passes = ensemble_passes(ensemble, th, tw)
    if tile_batch is None:
        # the batched improved sampler runs 2B images: stay below run_unet's chunking threshold
        k = 2 if sampler == "improved" else 1
        tile_batch = max(1, min(n_tiles * max(nd for _, nd in passes), E.FWD_CHUNK_PIXELS // (k * th * tw)))
    if tile_batch < 1:
        raise ValueError(f"tile_batch must be >= 1, got {tile_batch}")
    if ensemble > 1:
        with torch.no_grad():
            tout = torch.empty((n_tiles, C, th, tw), dtype=torch.float32, device=x.device)
            out = torch.empty_like(x)
            for d0, nd in passes:
                shape = (tile_batch, C, tw, th) if d0 >= 4 else (tile_batch, C, th, tw)
                run = _tile_sampler(model, shape, sampler, graph)
                tin = torch.empty(shape, dtype=torch.float32, device=x.device)
                for first in range(0, n_tiles * nd, tile_batch):
                    tile_gather_d4(x, tile, overlap, d0, nd, first, tile_batch, out=tin)
                    # the surplus of the last batch is ignored; the running mean lives in tout
                    tile_accum_d4(run(tin).contiguous(), tout, d0, nd, ensemble, first, tile_batch)
            tile_blend(tout, out, tile, overlap)
        return out
    with torch.no_grad():
        run = _tile_sampler(model, (tile_batch, C, th, tw), sampler, graph)
        tin = torch.empty((tile_batch, C, th, tw), dtype=torch.float32, device=x.device)
        tout = torch.empty((n_tiles, C, th, tw), dtype=torch.float32, device=x.device)
        out = torch.empty_like(x)
        for first in range(0, n_tiles, tile_batch):
            tile_gather(x, tile, overlap, first, tile_batch, out=tin)
            m = min(tile_batch, n_tiles - first)
            tout[first:first + m].copy_(run(tin)[:m])     # the surplus of the last batch is dropped
        tile_blend(tout, out, tile, overlap)
    return out


class ForwardGraph:
    """hipGraph capture of one network forward for a fixed input shape: the plain
    ``RDUNet`` (UNet/RDUNet_model.py:157-186) or ``RDUNet_T`` with a fixed t map --
    the ~70 conv launches of a forward as one host launch (a batch-1 forward at
    64x64 or 256x256 is launch-bound when issued eagerly)."""

    def __init__(self, net, shape, t=None):
        self.net = net
        dev = next(net.parameters()).device
        self.inp = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.t = None if t is None else t.to(dev)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.no_grad(), torch.cuda.stream(s):
            for _ in range(2):   # engines, packs and workspaces allocated outside the capture
                self._body()
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.no_grad(), torch.cuda.graph(self.graph):
            self.out = self._body()

    def _body(self):
        return self.net(self.inp) if self.t is None else self.net(self.inp, self.t)

    def __call__(self, x):
        self.inp.copy_(x)
        for packs in self.net._rdn_packs.values():   # weights changed since capture -> repack first
            packs.refresh()
        self.graph.replay()
        return self.out
