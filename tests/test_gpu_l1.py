"""``functional.l1_loss`` (rdn_l1_fwd / rdn_l1_bwd): the forward against
torch.nn.functional.l1_loss in fp64 on the CPU, the backward bit for bit against
``sign(p - t) * (g / n)`` with exact ties planted, and repeated forwards giving the same
bits.  Shapes: fewer elements than one block, a count that is no multiple of 4 (the
scalar tail), many blocks with several grid-stride sweeps (786432 elements against
1024 blocks x 256 threads x 4), and a view one element into a larger buffer (pointers
not 16-byte aligned: the scalar path)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = {"one_block": (1, 3, 8, 8), "tail": (2, 3, 33, 17), "many_blocks": (4, 3, 256, 256)}
CASES = list(SHAPES) + ["unaligned"]


def _over_n(g, n):
    """g / n as one correctly rounded fp32 division on the device.  (A device tensor divided
    by a Python number is not that: torch multiplies by the rounded reciprocal 1 / n.)"""
    return g / torch.tensor(float(n), device=g.device)


def _pair(case):
    g = torch.Generator().manual_seed(len(case))
    if case == "unaligned":
        n = 2 * 3 * 33 * 17
        p, t = (torch.randn(n + 5, generator=g).cuda()[1:n + 1].view(2, 3, 33, 17) for _ in range(2))
        assert p.data_ptr() % 16 == 4 and t.data_ptr() % 16 == 4 and p.is_contiguous()
    else:
        p, t = (torch.randn(SHAPES[case], generator=g).cuda() for _ in range(2))
        assert p.data_ptr() % 16 == 0 and t.data_ptr() % 16 == 0
    # exact ties, spread over the vector body, the last unit and the tail; -0.0 against 0.0
    pf, tf = p.view(-1), t.view(-1)
    n = pf.numel()
    ties = [0, 5, n // 2, n - 1, n - 2]
    for i in ties:
        tf[i] = pf[i]
    pf[7], tf[7] = -0.0, 0.0
    pf[n - 3], tf[n - 3] = 0.0, -0.0
    return p, t, ties + [7, n - 3]


@pytest.mark.parametrize("case", CASES)
def test_l1_forward_vs_fp64(case):
    from vub_image_denoising_amd import functional as Fn
    p, t, _ = _pair(case)
    loss = Fn.l1_loss(p, t)
    assert loss.dim() == 0 and loss.is_cuda and loss.dtype == torch.float32
    ref = torch.nn.functional.l1_loss(p.cpu().double(), t.cpu().double()).item()
    rel = abs(loss.item() - ref) / ref
    print(f"{case}: l1 {loss.item():.8f} fp64 {ref:.8f} rel {rel:.2e}")
    assert rel < 1e-5


@pytest.mark.parametrize("case", CASES)
def test_l1_backward_bit_exact(case):
    from vub_image_denoising_amd import functional as Fn
    p, t, ties = _pair(case)
    p.requires_grad_(True)
    t.requires_grad_(True)
    g = torch.tensor(-2.75, device="cuda")
    Fn.l1_loss(p, t).backward(g)
    n = p.numel()
    with torch.no_grad():
        ref = torch.sign(p - t) * _over_n(g, n)
    bad = (p.grad != ref).view(-1).nonzero().view(-1)
    assert torch.equal(p.grad, ref), (bad.numel(), bad[:8].tolist(), p.grad.view(-1)[bad[:4]].tolist(),
                                      ref.view(-1)[bad[:4]].tolist())
    assert torch.equal(t.grad, -p.grad)
    flat = p.grad.view(-1)
    for i in ties:
        assert flat[i].item() == 0.0, i
    assert int((flat == 0).sum()) == len(ties) and int((flat != 0).sum()) == n - len(ties)
    assert set(flat[flat != 0].abs().unique().tolist()) == {abs(_over_n(g, n).item())}


def test_l1_backward_of_pred_only():
    """The trainer's use: the target needs no gradient, the loss is scaled downstream."""
    from vub_image_denoising_amd import functional as Fn
    p, t, _ = _pair("tail")
    p.requires_grad_(True)
    (Fn.l1_loss(p, t) * 3.0).backward()
    assert t.grad is None
    assert torch.equal(p.grad, torch.sign(p.detach() - t) * _over_n(torch.tensor(3.0, device="cuda"), p.numel()))


@pytest.mark.parametrize("case", ["tail", "many_blocks", "unaligned"])
def test_l1_forward_is_deterministic(case):
    from vub_image_denoising_amd import functional as Fn
    p, t, _ = _pair(case)
    a = Fn.l1_loss(p, t).clone()
    b = Fn.l1_loss(p, t).clone()
    assert torch.equal(a.view(1).view(torch.int32), b.view(1).view(torch.int32))


def test_l1_refuses_cpu_tensors_and_shape_mismatch():
    from vub_image_denoising_amd import functional as Fn
    with pytest.raises(RuntimeError):
        Fn.l1_loss(torch.zeros(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match="shapes differ"):
        Fn.l1_loss(torch.zeros(4, device="cuda"), torch.zeros(8, device="cuda"))
