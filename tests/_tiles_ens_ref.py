"""Torch restatement of the geometric self-ensemble of include/rdunet_hip.h
(rdn_tile_gather_d4 / rdn_tile_accum_d4), written from the definition and independent of
sampling.py:

  transform d in 0..7: bit 0 flips x, bit 1 flips y, bit 2 transposes, after the flips:
      u.flip(-1) if d&1, then u.flip(-2) if d&2, then u.transpose(-1, -2) if d&4
  element form, u of th x tw:  T_d(u)[y', x'] = u[sy, sx]  with
      (y, x) = (x', y') if d&4 else (y', x');  sy = th-1-y if d&2 else y;  sx = tw-1-x if d&1 else x
  the inverse transposes first and then flips
  ensemble n in {1, 2, 4, 8} uses d = 0..n-1, per tile of the grid
  e_g = (((v_0 + v_1) + v_2) + ... + v_{n-1}) * (1/n), v_d = T_d^-1(sampler(T_d(tile g))), fp32
  passes (d0, nd): square tiles (0, n); otherwise (0, min(n, 4)) and for n == 8 also (4, 4)
  work item w = g*nd + (d - d0), 0 <= w < n_tiles*nd; a batch is `count` consecutive items,
  items past the end repeat the last item
"""
import torch


def transform(u, d):
    """T_d over the last two axes."""
    if d & 1:
        u = u.flip(-1)
    if d & 2:
        u = u.flip(-2)
    if d & 4:
        u = u.transpose(-1, -2)
    return u.contiguous()


def inverse(v, d):
    """T_d^-1 over the last two axes: the transpose first, then the flips."""
    if d & 4:
        v = v.transpose(-1, -2)
    if d & 2:
        v = v.flip(-2)
    if d & 1:
        v = v.flip(-1)
    return v.contiguous()


def transform_elementwise(u, d):
    """T_d of a 2-D tensor by the element formula (a Python loop: small tiles only)."""
    th, tw = u.shape
    oh, ow = (tw, th) if d & 4 else (th, tw)
    out = torch.empty(oh, ow, dtype=u.dtype)
    for yp in range(oh):
        for xp in range(ow):
            y, x = (xp, yp) if d & 4 else (yp, xp)
            sy = th - 1 - y if d & 2 else y
            sx = tw - 1 - x if d & 1 else x
            out[yp, xp] = u[sy, sx]
    return out


def passes(n, th, tw):
    if th == tw:
        return [(0, n)]
    return [(0, min(n, 4))] + ([(4, 4)] if n == 8 else [])


def work_item(w, d0, nd):
    """(tile g, transform d) of work item w of the pass (d0, nd)."""
    return w // nd, d0 + w % nd


def batch_items(first, count, n_tiles, d0, nd):
    """The (g, d) of the `count` items of a batch from `first`; past the end: the last item again."""
    last = n_tiles * nd - 1
    return [work_item(min(first + j, last), d0, nd) for j in range(count)]


def gather_items(tiles, d0, nd):
    """All work items of the pass (d0, nd) over `tiles` [n_tiles, C, th, tw] (e.g. of
    _tiles_ref.gather), in work-item order: [n_tiles*nd, C, th', tw']."""
    return torch.stack([transform(tiles[g], d) for g, d in
                        (work_item(w, d0, nd) for w in range(tiles.size(0) * nd))])


def accumulate(acc, src, d0, nd, n_ens, first, count):
    """One rdn_tile_accum_d4 call in fp32 on the CPU: `src` holds the outputs of work items
    first .. first+count-1 (surplus past the end ignored); `acc` [n_tiles, C, th, tw] is
    updated in place, item by item in ascending w (so ascending d inside a tile)."""
    n_tiles = acc.size(0)
    for j in range(count):
        w = first + j
        if w >= n_tiles * nd:
            break
        g, d = work_item(w, d0, nd)
        v = inverse(src[j].float(), d)
        acc[g] = v if d == 0 else acc[g] + v
        if d == n_ens - 1:
            acc[g] = acc[g] * torch.tensor(1.0 / n_ens, dtype=torch.float32)
    return acc


def ensemble_mean(members):
    """(((v_0 + v_1) + v_2) + ...) * (1/n) in fp32 for members [n, ...] already mapped back."""
    s = members[0].float().clone()
    for v in members[1:]:
        s = s + v.float()
    return s * torch.tensor(1.0 / len(members), dtype=torch.float32)
