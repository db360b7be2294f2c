"""The plain RDUNet baseline's trainer (RDUNet_model.train_step / train_model): one L1
step against the CPU oracle, train_model(captured=True) against the eager loop bit for
bit (parameters, optimizer state, logged losses, checkpoints; a second batch shape, a
validation batch between the epochs, an LR change), a DiffusionModel captured next to a
baseline in one process, and a step at the reference's width of 128."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rdunet_ref as R  # noqa: E402
from oracle.weights import make_params  # noqa: E402

B, S = 2, 32


def _rel(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


class _Writer:
    def __init__(self):
        self.loss, self.val = {}, {}

    def add_scalar(self, tag, v, step):
        {"Loss/train": self.loss, "Loss/validation": self.val}[tag][step] = float(v)


def _batches(n, seed=11, last_b=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        b = last_b if (last_b and k == n - 1) else B
        clean = torch.rand(b, 3, S, S, generator=g) * 2 - 1
        out.append((clean + 0.15 * torch.randn(b, 3, S, S, generator=g), clean))
    return out


def _model(seed=17):
    import vub_image_denoising_amd as vm
    m = vm.RDUNet(channels=3, base_filters=16)
    p = make_params({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    return m.cuda()


def _oracle_grads(params, noisy, dy, dtype):
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in params.items()}
    y = R.rdunet_forward(leaves, noisy.to(dtype))
    y.backward(dy.to(dtype))
    return {k: v.grad for k, v in leaves.items()}


def test_l1_step_vs_oracle():
    """The batch is seed 33: of the seeds 0..39 the one whose smallest PReLU pre-activation
    lies farthest from 0 in the fp64 oracle (7e-6 of its layer's mean magnitude).  The
    network itself is not smooth there: at seed 11 a level-2 pre-activation lies 7e-7 from
    0, torch's own fp32 CPU pass takes the other PReLU branch and its gradients differ from
    the fp64 ones by 7.7e-3 in block_2_1 (1e-6 on a batch without such an element), which
    says nothing about the kernels.  The test checks that property of its input first."""
    from vub_image_denoising_amd import functional as Fn
    model = _model().train()
    noisy, clean = _batches(1, seed=33)[0]
    y = model(noisy.cuda())
    y.retain_grad()
    loss = Fn.l1_loss(y, clean.cuda())
    loss.backward()
    n = y.numel()
    leaves = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    y_ref = R.rdunet_forward(leaves, noisy.double())
    loss_ref = torch.nn.functional.l1_loss(y_ref, clean.double())
    r_out, r_loss = _rel(y.detach().cpu().numpy(), y_ref.detach().numpy()), abs(loss.item() - loss_ref.item()) / loss_ref.item()
    print(f"output rel {r_out:.2e}; loss {loss.item():.7f} oracle {loss_ref.item():.7f} rel {r_loss:.2e}")
    assert r_out < 1e-3
    assert r_loss < 1e-4
    with torch.no_grad():
        dy = torch.sign(y - clean.cuda()) * (torch.tensor(1.0, device="cuda") / torch.tensor(float(n), device="cuda"))
    assert torch.equal(y.grad, dy)
    # the GPU's own dy through the oracle: L1 is not smooth, an element whose residual is
    # below the forward error may carry the other sign on the two sides, and the sign
    # itself is covered by test_gpu_l1
    y_ref.backward(y.grad.cpu().double())
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref32 = _oracle_grads(params, noisy, y.grad.cpu(), torch.float32)
    own = max(_rel(ref32[k].numpy(), leaves[k].grad.numpy()) for k in ref32)
    print(f"the oracle's own fp32 against fp64, worst per-tensor rel {own:.2e}")
    assert own < 1e-5, "the input has a PReLU pre-activation on the kink: not a usable case"
    worst = (0.0, "")
    for name, p in model.named_parameters():
        worst = max(worst, (_rel(p.grad.cpu().numpy(), leaves[name].grad.numpy()), name))
    print(f"parameter gradients: worst per-tensor rel {worst[0]:.2e} ({worst[1]})")
    assert worst[0] < 2e-3, worst


def _train(tmp, log_every, captured, epochs=2, data=None, val=True):
    from vub_image_denoising_amd.optim import FusedAdamW
    from vub_image_denoising_amd.RDUNet_model import train_model
    model = _model()
    opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    w = _Writer()
    data = data or _batches(6, last_b=1)   # a partial group of 2 per epoch; the last batch a second shape
    train_model(model, data, _batches(1, seed=5) if val else None, opt, sched, w, str(tmp), epochs,
                accumulation_steps=4, clip_value=1.0, log_every=log_every, captured=captured)
    return model, opt, w


@pytest.mark.parametrize("log_every", [1, 4])
def test_captured_equals_eager(log_every, tmp_path):
    from vub_image_denoising_amd.RDUNet_model import train_model
    mE, oE, wE = _train(tmp_path / "eager", log_every, False)
    mG, oG, wG = _train(tmp_path / "graph", log_every, True)
    for (n, a), b in zip(mE.named_parameters(), mG.parameters()):
        assert torch.equal(a, b), n
    sE, sG = oE.state_dict(), oG.state_dict()
    assert sE["state"].keys() == sG["state"].keys() and len(sE["state"]) > 0
    for k in sE["state"]:
        assert sE["state"][k].keys() == sG["state"][k].keys()
        for key, v in sE["state"][k].items():
            if key == "step":
                assert float(v) == float(sG["state"][k][key]) == 2.0   # one update per epoch
            else:
                assert torch.equal(v, sG["state"][k][key]), (k, key)
    assert oE._step == oG._step == 2
    assert sE["param_groups"][0]["lr"] == sG["param_groups"][0]["lr"] == 1e-3 / 4
    assert wE.loss == wG.loss and len(wE.loss) == 2 * len(range(0, 6, log_every))
    assert wE.val == wG.val and sorted(wE.val) == [1, 2] and all(np.isfinite(v) for v in wE.val.values())
    name = "RDUNet_model_epoch_2.pth"
    cE = torch.load(os.path.join(tmp_path / "eager", name), map_location="cuda", weights_only=True)
    cG = torch.load(os.path.join(tmp_path / "graph", name), map_location="cuda", weights_only=True)
    assert sorted(cE) == sorted(cG) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert cE["epoch"] == cG["epoch"] == 2 and cE["scheduler_state_dict"] == cG["scheduler_state_dict"]
    assert cE["model_state_dict"].keys() == cG["model_state_dict"].keys() == mE.state_dict().keys()
    assert not any(k.startswith("unet.") for k in cE["model_state_dict"])
    for k, v in cE["model_state_dict"].items():
        assert torch.equal(v, cG["model_state_dict"][k]), k
    for k, st in cE["optimizer_state_dict"]["state"].items():
        for key, v in st.items():
            assert torch.equal(torch.as_tensor(v), torch.as_tensor(cG["optimizer_state_dict"]["state"][k][key])), (k, key)
    (graphs,) = mG._rdn_train_graphs.values()
    print("log_every", log_every, "captures", graphs.captures, sorted(graphs.graphs, key=str))
    # (B2, accum), (B2, accum_step), (B1, accum); the LR change of epoch 2 re-captures in place
    assert graphs.captures == len(graphs.graphs) == 3
    assert set(graphs.graphs) == {((2, 3, S, S), 'accum'), ((2, 3, S, S), 'accum_step'), ((1, 3, S, S), 'accum')}
    assert not hasattr(mE, "_rdn_train_graphs")
    # a second call replays what the first captured
    before = dict(graphs.graphs)
    train_model(mG, _batches(6, last_b=1), None, oG, None, None, str(tmp_path / "graph"), 3, start_epoch=2,
                captured=True)
    (again,) = mG._rdn_train_graphs.values()
    assert again is graphs and graphs.captures == 3 and all(graphs.graphs[k] is before[k] for k in before)
    assert oG._step == 3


def test_step_and_loss_kinds_and_t_refused():
    """The kinds the trainer does not use: 'loss' is the forward loss of the batch without a
    gradient, 'step' the whole step of one batch (zero_grad, backward, clip, update), each
    the eager calls' bits; a bare RDUNet's graph has no t."""
    from vub_image_denoising_amd.optim import FusedAdamW
    from vub_image_denoising_amd.RDUNet_model import forward_loss_device, train_step_device
    from vub_image_denoising_amd.train_graph import TrainStepGraph, TrainStepGraphs
    (n1, c1), (n2, c2) = [(a.cuda(), b.cuda()) for a, b in _batches(2)]
    mE, mG = _model(), _model()
    oE, oG = (FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4) for m in (mE, mG))
    graphs = TrainStepGraphs(mG, oG, clip_value=1.0)
    mE.train()
    assert torch.equal(forward_loss_device(mE, n1, c1), graphs(c1, n1, kind='loss'))
    for noisy, clean in ((n1, c1), (n2, c2)):
        le = train_step_device(mE, noisy, clean, oE, 1.0, zero_grad=True, clip=True)
        oE.step()
        assert torch.equal(le, graphs(clean, noisy))
    for a, b in zip(mE.parameters(), mG.parameters()):
        assert torch.equal(a, b)
    assert oE._step == oG._step == 2 and graphs.captures == 2
    assert graphs.graphs[((B, 3, S, S), 'step')].t is None
    with pytest.raises(ValueError, match="no t"):
        graphs(c1, n1, t=torch.zeros(B, device="cuda"))
    with pytest.raises(ValueError, match="no t input"):
        TrainStepGraph(mG, oG, (B, 3, S, S), t_input=True)


def test_diffusion_model_captures_next_to_a_baseline(tmp_path):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel, train_step_device
    from vub_image_denoising_amd.optim import FusedAdamW
    from vub_image_denoising_amd.train_graph import trainer_graphs
    data = _batches(4)
    base, bopt, _ = _train(tmp_path, 1, True, epochs=1, data=data, val=False)

    def diffusion():
        m = DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=20)
        p = make_params({k[5:]: tuple(v.shape) for k, v in m.state_dict().items()}, 17)
        m.load_state_dict({"unet." + k: torch.from_numpy(v) for k, v in p.items()})
        m = m.cuda()
        return m, FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)

    (mE, oE), (mG, oG) = diffusion(), diffusion()
    graphs = trainer_graphs(mG, oG, 'uniform', 1.0)
    batches = [(n.cuda(), c.cuda()) for n, c in data[:2]]
    torch.manual_seed(9)
    got = [graphs(c, n, kind='step').clone() for n, c in batches]
    torch.manual_seed(9)
    want = []
    for n, c in batches:
        want.append(train_step_device(mE, c, n, oE, 'uniform', 1.0).clone())
        oE.step()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    for a, b in zip(mE.parameters(), mG.parameters()):
        assert torch.equal(a, b)
    assert list(mG._rdn_train_graphs) == [('uniform', 1.0, (0.0, 1.0, 0.0))] and list(graphs.graphs) == [((B, 3, S, S), 'step')]
    assert list(base._rdn_train_graphs) == [('l1', 1.0)]
    assert graphs.graphs[((B, 3, S, S), 'step')].t is None and oG._step == 2
    # the baseline's graphs still replay after the diffusion captures
    from vub_image_denoising_amd.RDUNet_model import train_model
    (bgraphs,) = base._rdn_train_graphs.values()
    train_model(base, data, None, bopt, None, None, str(tmp_path), 2, start_epoch=1, captured=True)
    assert bgraphs.captures == 2 and bopt._step == 2


def test_reference_width_step():
    """RDUNet(base_filters=128), the width the reference trains: one eager step."""
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.RDUNet_model import train_step_device
    torch.manual_seed(0)
    model = vm.RDUNet(channels=3, base_filters=128).cuda()
    g = torch.Generator().manual_seed(3)
    clean = torch.rand(1, 3, S, S, generator=g) * 2 - 1
    noisy = clean + 0.15 * torch.randn(1, 3, S, S, generator=g)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loss = train_step_device(model, noisy.cuda(), clean.cuda(), opt, zero_grad=True)
    params = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = torch.nn.functional.l1_loss(R.rdunet_forward(params, noisy).double(), clean.double()).item()
    rel = abs(loss.item() - ref) / ref
    print(f"base_filters 128: loss {loss.item():.7f} oracle {ref:.7f} rel {rel:.2e}")
    assert rel < 1e-4
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
