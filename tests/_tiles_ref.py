"""Torch restatement of the tile grid, gather and blend of include/rdunet_hip.h
(rdn_tile_grid / rdn_tile_gather / rdn_tile_blend), written from the definition and
independent of sampling.plan_tiles:

  t = min(tile, ceil8(n)); npad = max(n, t); s = t - overlap
  k = 0 if npad == t else ceil((npad - t) / s); o_i = min(i*s, npad - t), i = 0..k
  gather: F.pad(..., mode="reflect") to (Hp, Wp), then slices at the origins
  blend:  fp64 sum of wy*wx*v / sum of wy*wx, w(i) = min(1, min(i+1, t-i)/(overlap+1))
          rounded to fp32; a pixel under exactly one tile takes the tile's value.
"""
import math

import torch
import torch.nn.functional as F


def axis(n, tile, overlap):
    t = min(tile, 8 * math.ceil(n / 8))
    npad = max(n, t)
    if npad == t:
        return t, npad, [0]
    s = t - overlap
    k = math.ceil((npad - t) / s)
    return t, npad, [min(i * s, npad - t) for i in range(k + 1)]


def grid(H, W, tile, overlap):
    th, Hp, ys = axis(H, tile, overlap)
    tw, Wp, xs = axis(W, tile, overlap)
    return th, tw, Hp, Wp, ys, xs


def gather(x, tile, overlap):
    """All tiles of x [B,C,H,W] in global order, [B*ny*nx, C, th, tw]."""
    B, C, H, W = x.shape
    th, tw, Hp, Wp, ys, xs = grid(H, W, tile, overlap)
    xp = F.pad(x, (0, Wp - W, 0, Hp - H), mode="reflect") if (Hp > H or Wp > W) else x
    return torch.stack([xp[b, :, oy:oy + th, ox:ox + tw] for b in range(B) for oy in ys for ox in xs])


def window(t, overlap):
    i = torch.arange(t, dtype=torch.float32)
    m = torch.minimum(i + 1, t - i)
    return torch.clamp(m / torch.tensor(float(overlap + 1), dtype=torch.float32), max=1.0)   # fp32 division


def blend(tiles, B, C, H, W, tile, overlap):
    """fp64 blend of tiles [B*ny*nx, C, th, tw] -> (out [B,C,H,W] float64, cover count [H,W])."""
    th, tw, Hp, Wp, ys, xs = grid(H, W, tile, overlap)
    tiles = tiles.detach().cpu()
    assert tuple(tiles.shape) == (B * len(ys) * len(xs), C, th, tw)
    w2 = window(th, overlap).double()[:, None] * window(tw, overlap).double()[None, :]
    acc = torch.zeros(B, C, Hp, Wp, dtype=torch.float64)
    wsum = torch.zeros(Hp, Wp, dtype=torch.float64)
    cnt = torch.zeros(Hp, Wp, dtype=torch.int64)
    single = torch.zeros(B, C, Hp, Wp, dtype=torch.float64)
    g = 0
    for b in range(B):
        for oy in ys:
            for ox in xs:
                acc[b, :, oy:oy + th, ox:ox + tw] += w2 * tiles[g].double()
                single[b, :, oy:oy + th, ox:ox + tw] = tiles[g].double()
                if b == 0:
                    wsum[oy:oy + th, ox:ox + tw] += w2
                    cnt[oy:oy + th, ox:ox + tw] += 1
                g += 1
    assert wsum.min().item() > 0 and cnt.min().item() >= 1
    out = torch.where(cnt == 1, single, acc / wsum)
    return out[:, :, :H, :W], cnt[:H, :W]
