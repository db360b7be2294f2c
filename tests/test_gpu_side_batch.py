"""Batched split-K reduces of the weight-gradient stream (engine.SIDE_BATCH, default 4):
up to SIDE_BATCH consecutive unfused layers' reduces go in one rdn_wgrad_reduce_batch
launch on the side stream, each layer's slabs in its own entry of a ring of SIDE_BATCH
slab buffers (``side_slab``); a layer the compute stream has to wait for while it is
still batched is flushed early (``wait_done``), which happens whenever the dYpre slot
ring (WGRAD_SLOTS) is shorter than the batch.

Scheduling only: the per-layer work and summation order are those of one reduce launch
per layer, so every parameter gradient is bit-identical to the SIDE_BATCH=1 run -- over
two forward/backward passes in a row on one engine (slabs reused across steps) and over
two live graphs on two pooled engines that share the pool's scratch (the second on the
mirrored input, whose gradients differ) -- with one slot per layer, with a 2-slot and
with a 6-slot ring.  (fp32, 2 slots: level 0's fused weight-gradient kernels write their
dalpha/dbias partials into the ring slot from the side stream without passing wait_done;
before the engine flushed the batch there, block_0_0.conv_0 / conv_1's bias and PReLU
gradients were reduced from the partials of the layer two places later.)  The launches are observed by wrapping the library entry: an early
flush shows as a side-stream launch before the last with fewer than SIDE_BATCH jobs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

B, S = 2, 64
_REF = {}


def _grads(monkeypatch, side_batch, slots, dtype):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd import _hip as H
    from vub_image_denoising_amd import engine as E
    lib = H.lib()
    orig = lib.rdn_wgrad_reduce_batch
    calls = []          # (jobs, stream) of every batched reduce launch
    marks = []          # len(calls) at the start of each backward

    def spy(jobs, n, stream):
        calls.append((int(n), int(stream or 0)))
        return orig(jobs, n, stream)

    with monkeypatch.context() as mp:
        mp.setattr(E, "SIDE_BATCH", side_batch)
        mp.setattr(E, "WGRAD_SLOTS", slots)
        mp.setattr(lib, "rdn_wgrad_reduce_batch", spy)
        torch.manual_seed(0)
        m = vm.RDUNet_T(base_filters=32).cuda()
        m.set_compute_dtype(dtype)
        g = torch.Generator().manual_seed(1)
        x = (torch.rand(B, 3, S, S, generator=g) * 2 - 1).cuda()
        t = torch.rand(B, 1, 1, 1, generator=g).cuda()
        w = torch.randn(B, 3, S, S, generator=g).cuda()

        def backward(y):
            m.zero_grad(set_to_none=True)
            marks.append(len(calls))
            (y * w).mean().backward()
            return {n: p.grad.detach().clone() for n, p in m.named_parameters()}

        grads = [backward(m(x, t)) for _ in range(2)]       # (a) one engine, two steps in a row
        y1, y2 = m(x, t), m(x.flip(-1), t)                  # (b) two live graphs, two pooled engines
        grads.append(backward(y1))
        grads.append(backward(y2))
        torch.cuda.synchronize()
    marks.append(len(calls))
    pools = [pool for pool in m._rdn_engines.values() if any(e.train for e in pool)]
    assert len(pools) == 1 and len(pools[0]) == 2, [len(p) for p in pools]
    engs = pools[0]
    assert all(e.scratch is engs[0].scratch for e in engs), "one scratch dict per pool"
    assert all(e.side is not None for e in engs), "the weight-gradient stream is on by default"
    side_streams = {e.side.cuda_stream for e in engs}
    per_bwd = [[n for n, s in calls[a:b] if s in side_streams] for a, b in zip(marks, marks[1:])]
    return grads, per_bwd, engs


def _structure(engs, side_batch, slots):
    """The slab ring: SIDE_BATCH distinct slab buffers, shared by the pool's engines; in
    backward order unfused layers SIDE_BATCH apart share a slab, closer ones do not."""
    n_side = None
    for e in engs:
        assert e.side_batch == side_batch and len(e.ws_side) == side_batch
        assert len({w.data_ptr() for w in e.ws_side}) == side_batch
        assert [w.data_ptr() for w in e.ws_side] == [w.data_ptr() for w in engs[0].ws_side]
        if slots:
            assert e.slots == slots
        side = [L for L in reversed(e.layers) if not L.extra["dw"]]
        n_side = len(side)
        assert n_side >= 2 * side_batch + 1, f"{n_side} unfused layers: the ring of {side_batch} does not wrap twice"
        ptrs = [L.wgrad_desc.ws for L in side]
        for k, L in enumerate(side):
            assert L.extra["side_slab"] == k % side_batch
            assert ptrs[k] == e.ws_side[k % side_batch].data_ptr()
            for d in range(1, side_batch):
                if k + d < n_side:
                    assert ptrs[k + d] != ptrs[k], (k, d)
            if k + side_batch < n_side:
                assert ptrs[k + side_batch] == ptrs[k], k
    return n_side


def _check(monkeypatch, side_batch, slots, dtype):
    if dtype not in _REF:    # SIDE_BATCH=1, one slot per layer: one reduce launch per layer
        _REF[dtype] = _grads(monkeypatch, 1, 0, dtype)[0]
    ref = _REF[dtype]
    grads, per_bwd, engs = _grads(monkeypatch, side_batch, slots, dtype)
    n_side = _structure(engs, side_batch, slots)
    print(f"{dtype} SIDE_BATCH={side_batch} WGRAD_SLOTS={slots}: slots {engs[0].slots}, {len(engs[0].layers)} layers, "
          f"{n_side} on the weight-gradient stream; side-stream batch launches per backward: {per_bwd}")
    assert len(grads) == len(ref) == 4 and len(per_bwd) == 4
    for i, (a, b) in enumerate(zip(grads, ref)):
        for n in b:
            assert torch.equal(a[n], b[n]), f"backward {i}: {n}"
    for n in grads[0]:       # the sequential repeat and the live-graph backward of x equal the first
        assert torch.equal(grads[1][n], grads[0][n]) and torch.equal(grads[2][n], grads[0][n]), n
    assert any(not torch.equal(grads[3][n], grads[2][n]) for n in grads[2]), "mirrored input: same gradients"
    for jobs in per_bwd:
        if side_batch == 1:
            assert jobs == [1] * n_side, f"SIDE_BATCH=1: not one reduce launch per layer on the side stream: {jobs}"
            continue
        assert sum(jobs) == n_side and all(1 <= j <= side_batch for j in jobs), jobs
        early = [j for j in jobs[:-1] if j < side_batch]
        if slots and slots < side_batch:
            # the ring is shorter than the batch: wait_done has to flush a batched layer
            assert early, f"no early flush with {slots} slots and SIDE_BATCH={side_batch}: {jobs}"


@pytest.mark.parametrize("slots", [0, 2, 6])
@pytest.mark.parametrize("side_batch", [1, 4, 8])
def test_side_batch_bit_identical_bf16(monkeypatch, side_batch, slots):
    _check(monkeypatch, side_batch, slots, "bf16")


def test_side_batch_bit_identical_fp32(monkeypatch):
    _check(monkeypatch, 4, 2, "fp32")
