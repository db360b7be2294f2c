"""The split-K reduce of the weight gradients through the C ABI, exact.

Slabs, partials and the gradients they are added to hold small integers (uniform in
[-8, 8], stored as fp32), so every partial sum is an integer far below 2^24 (at most
70 x 8 for the slabs, 333 x 8 for the partials) and exact in fp32 in any order: the
result has to ``torch.equal`` the integer sum torch computes on the CPU.  Every case
runs three ways -- through rdn_wgrad_reduce / rdn_wgrad_reduce_cols (whichever can
express it), as a one-job rdn_wgrad_reduce_batch, and as one job among eight different
ones in one launch -- and all three have to give that sum.

The cases walk every branch of the reduce's block: splits 1, 3, 5, 17 and 70 (below, at
and past the 4-way unrolled loop, 1 to 16 split lanes), mdim 16 and 24, padded columns
dropped (ndim 8, ndim_real 3) and ndim 32, 9 and 4 taps, store and accumulate onto a
non-zero gradient, a column part (columns 32..64 / 64..96 of 96), and dalpha/dbias
partials over as many rows as splits (given as 0 and explicitly) and over 300 / 333
rows (past one 256-thread stride), with dalpha or dbias null."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from vub_image_denoising_amd import _hip as H  # noqa: E402

# splits, mdim, ndim, ndim_real, taps, gstride, gci0, accumulate,
# partial rows in the buffer (0: no partials), part_splits argument, dalpha, dbias
CASES = [
    (1, 16, 8, 3, 9, 3, 0, 0, 0, 0, False, False),
    (3, 24, 32, 32, 4, 32, 0, 1, 3, 0, True, True),
    (5, 16, 32, 32, 9, 96, 32, 1, 5, 5, True, False),
    (17, 24, 8, 3, 4, 3, 0, 1, 300, 300, False, True),
    (70, 16, 32, 32, 9, 32, 0, 0, 70, 0, True, True),
    (70, 24, 8, 3, 9, 3, 0, 1, 0, 0, False, False),
    (17, 16, 32, 32, 4, 96, 32, 0, 333, 333, True, True),
    (5, 24, 32, 32, 9, 32, 0, 0, 0, 0, False, False),
    (3, 16, 8, 3, 4, 3, 0, 1, 3, 3, False, True),
    (1, 24, 32, 32, 9, 96, 64, 1, 1, 0, True, True),
]
_DATA = {}


def _ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


def _data(i):
    """Case i's inputs on the CPU and the device, and its expected outputs (built once)."""
    if i in _DATA:
        return _DATA[i]
    splits, mdim, ndim, ndim_real, taps, gstride, gci0, acc, prow, psplit, has_a, has_b = CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    ws = _ints(g, splits, mdim, taps, ndim)                 # ws[s][m][tap * ndim + nd]
    grad0 = _ints(g, mdim, gstride, taps)                   # grad[(m * gstride + gci0 + nd) * taps + tap]
    part = _ints(g, prow, 2, mdim) if prow else None        # part[z][dalpha | dbias][m]
    da0, db0 = _ints(g, mdim), _ints(g, mdim)
    s = ws.long().sum(0)[:, :, :ndim_real].permute(0, 2, 1)  # [m][nd][tap]
    grad = grad0.long().clone()
    cols = grad[:, gci0:gci0 + ndim_real]
    cols.copy_(cols + s if acc else s)
    exp = {"grad": grad.float()}
    if part is not None:
        ps = part.long()[:psplit or splits].sum(0)
        if has_a:
            exp["dalpha"] = (da0.long() + ps[0]).float()
        if has_b:
            exp["dbias"] = (db0.long() + ps[1]).float()
    dev = {"ws": ws.cuda(), "part": None if part is None else part.cuda()}
    init = {"grad": grad0, "dalpha": da0 if part is not None and has_a else None,
            "dbias": db0 if part is not None and has_b else None}
    _DATA[i] = (dev, init, exp)
    return _DATA[i]


def _outputs(i):
    """Fresh device copies of case i's gradient, dalpha and dbias (None where null)."""
    return {k: None if v is None else v.cuda() for k, v in _data(i)[1].items()}


def _job(i, out):
    splits, mdim, ndim, ndim_real, taps, gstride, gci0, acc, _, psplit, _, _ = CASES[i]
    dev = _data(i)[0]
    return H.ReduceJob(ws=dev["ws"].data_ptr(), grad=out["grad"].data_ptr(), part=H.ptr(dev["part"]),
                       dalpha=H.ptr(out["dalpha"]), dbias=H.ptr(out["dbias"]), splits=splits, mdim=mdim, ndim=ndim,
                       ndim_real=ndim_real, taps=taps, gstride=gstride, gci0=gci0, accumulate=acc, part_splits=psplit)


def _expect(i, out, how):
    for k, e in _data(i)[2].items():
        assert torch.equal(out[k].cpu(), e), f"case {i} {CASES[i]} {how}: {k}"


@pytest.mark.parametrize("i", range(len(CASES)))
def test_reduce_is_the_exact_integer_sum_three_ways(i):
    lib, st = H.lib(), H.stream_ptr()
    splits, mdim, ndim, ndim_real, taps, gstride, gci0, acc, _, psplit, _, _ = CASES[i]
    dev = _data(i)[0]

    out = _outputs(i)                                   # the single entries
    if gstride == ndim_real and gci0 == 0:
        H.check(lib.rdn_wgrad_reduce(dev["ws"].data_ptr(), splits, mdim, ndim, ndim_real, taps, out["grad"].data_ptr(),
                                     acc, H.ptr(dev["part"]), psplit, H.ptr(out["dalpha"]), H.ptr(out["dbias"]), st),
                "wgrad_reduce")
        how = "rdn_wgrad_reduce"
    else:
        assert ndim_real == ndim
        H.check(lib.rdn_wgrad_reduce_cols(dev["ws"].data_ptr(), splits, mdim, ndim, taps, out["grad"].data_ptr(), gstride,
                                          gci0, acc, H.ptr(dev["part"]), psplit, H.ptr(out["dalpha"]),
                                          H.ptr(out["dbias"]), st), "wgrad_reduce_cols")
        how = "rdn_wgrad_reduce_cols"
    _expect(i, out, how)

    out = _outputs(i)                                   # a one-job batch
    H.check(lib.rdn_wgrad_reduce_batch((H.ReduceJob * 1)(_job(i, out)), 1, st), "wgrad_reduce_batch")
    _expect(i, out, "one-job batch")

    n = H.REDUCE_BATCH_MAX                              # one of eight different jobs, at slot i % 8
    assert n == 8
    ids = [(i - i % n + k) % len(CASES) for k in range(n)]
    assert ids[i % n] == i and len(set(ids)) == n
    outs = [_outputs(k) for k in ids]
    jobs = [_job(k, o) for k, o in zip(ids, outs)]
    H.check(lib.rdn_wgrad_reduce_batch((H.ReduceJob * n)(*jobs), n, st), "wgrad_reduce_batch")
    for k, o in zip(ids, outs):
        _expect(k, o, f"job {ids.index(k)} of the eight-job batch of case {i}")
