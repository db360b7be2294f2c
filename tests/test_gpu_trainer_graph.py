"""run_epochs(captured=True): every batch of the trainers replayed as one hipGraph
(train_graph kinds 'step', 'loss', 'accum', 'accum_step') leaves the parameters, the
optimizer state, the logged losses and the checkpoints of the eager loop bit for bit,
in both accumulation modes, with FusedAdamW and FusedAdadelta, across a second batch
shape, a validation sample between the epochs and an LR change (re-capture); and the
captured Adadelta training follows the fp64 oracle loop."""
import math
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rdunet_ref as R  # noqa: E402
from oracle.weights import make_params  # noqa: E402

T_STEPS, B, S = 20, 2, 32


class _Writer:
    def __init__(self):
        self.loss = {}

    def add_scalar(self, tag, v, step):
        if tag == "Loss/train":
            self.loss[step] = float(v)


def _batches(n, seed=11, last_b=None):
    g = torch.Generator().manual_seed(seed)
    out = []
    for k in range(n):
        b = last_b if (last_b and k == n - 1) else B
        clean = torch.rand(b, 3, S, S, generator=g) * 2 - 1
        out.append((clean + 0.15 * torch.randn(b, 3, S, S, generator=g), clean))
    return out


def _model():
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    m = DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=T_STEPS)
    sd = m.state_dict()
    p = make_params({k[5:]: tuple(v.shape) for k, v in sd.items()}, 17)
    m.load_state_dict({"unet." + k: torch.from_numpy(v) for k, v in p.items()})
    return m.cuda()


def _optimizer(name, model):
    from vub_image_denoising_amd.optim import FusedAdadelta, FusedAdamW
    if name == "adamw":
        return FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    return FusedAdadelta(model.parameters(), lr=1.0)


def _sample(m, x):
    return m.improved_sampling(x)


def _train(tmp, mode, optname, log_every, dist, captured, epochs=2, data=None, val=True):
    from vub_image_denoising_amd.diffusion_RDUnet import run_epochs
    model = _model()
    opt = _optimizer(optname, model)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    w = _Writer()
    data = data or _batches(6, last_b=1)   # a partial group of 2 per epoch; the last batch a second shape
    torch.manual_seed(123)
    run_epochs(model, data, _batches(1, seed=5) if val else None, opt, sched, w, str(tmp), dist, epochs, 0, 4, 1.0,
               log_every, sample=_sample, accumulation=mode, captured=captured)
    return model, opt, w.loss


# distinct (shape, kind) pairs of the schedule above (batches 0-4 have B = 2, batch 5 B = 1; the
# 4th batch steps; log_every = 1 logs every batch, log_every = 4 batches 0 and 4):
#   reference, log_every 1: (B2, loss), (B2, step), (B1, loss)
#   reference, log_every 4: (B2, loss), (B2, step)       -- batches 1, 2, 5 only draw t
#   fixed, any log_every:   (B2, accum), (B2, accum_step), (B1, accum)
CAPTURES = {("reference", 1): 3, ("reference", 4): 2, ("fixed", 1): 3, ("fixed", 4): 3}

CASES = [(m, o, le, "uniform") for m in ("reference", "fixed") for o in ("adamw", "adadelta") for le in (1, 4)]
CASES.append(("fixed", "adamw", 1, "biased"))


@pytest.mark.parametrize("mode,optname,log_every,dist", CASES)
def test_captured_equals_eager(mode, optname, log_every, dist, tmp_path):
    mE, oE, lE = _train(tmp_path / "eager", mode, optname, log_every, dist, False)
    mG, oG, lG = _train(tmp_path / "graph", mode, optname, log_every, dist, True)
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
    assert sE["param_groups"][0]["lr"] == sG["param_groups"][0]["lr"]
    assert lE == lG and len(lE) == 2 * len(range(0, 6, log_every))
    name = "diffusion_RDUNet_model_checkpointed_epoch_2.pth"
    cE = torch.load(os.path.join(tmp_path / "eager", name), map_location="cuda", weights_only=True)
    cG = torch.load(os.path.join(tmp_path / "graph", name), map_location="cuda", weights_only=True)
    assert cE["model_state_dict"].keys() == cG["model_state_dict"].keys()
    for k, v in cE["model_state_dict"].items():
        assert torch.equal(v, cG["model_state_dict"][k]), k
    (graphs,) = mG._rdn_train_graphs.values()
    print(mode, optname, log_every, dist, "captures", graphs.captures, sorted(graphs.graphs, key=str))
    assert graphs.captures == len(graphs.graphs) == CAPTURES[(mode, log_every)]
    assert not hasattr(mE, "_rdn_train_graphs")


def test_second_call_replays_the_first_calls_graphs(tmp_path):
    from vub_image_denoising_amd.diffusion_RDUnet import run_epochs
    data = _batches(4)
    model, opt, _ = _train(tmp_path, "fixed", "adadelta", 1, "uniform", True, epochs=1, data=data, val=False)
    (graphs,) = model._rdn_train_graphs.values()
    before = dict(graphs.graphs)
    assert graphs.captures == 2
    run_epochs(model, data, None, opt, None, None, str(tmp_path), "uniform", 2, 1, 4, 1.0, 1, sample=_sample,
               accumulation="fixed", captured=True)
    (again,) = model._rdn_train_graphs.values()
    assert again is graphs and graphs.captures == 2
    assert graphs.graphs.keys() == before.keys() and all(graphs.graphs[k] is before[k] for k in before)
    assert opt._step == 2


def test_default_kind_is_the_step_graph():
    from vub_image_denoising_amd.train_graph import TrainStepGraph
    model = _model()
    opt = _optimizer("adamw", model)
    a = TrainStepGraph(model, opt, (B, 3, S, S))
    b = TrainStepGraph(model, opt, (B, 3, S, S), kind='step')
    print("graph nodes", a.graph_nodes, b.graph_nodes)
    assert a.kind == 'step' and a.graph_nodes and a.graph_nodes == b.graph_nodes
    with pytest.raises(ValueError):
        TrainStepGraph(model, opt, (B, 3, S, S), kind='update')
    with pytest.raises(TypeError):
        TrainStepGraph(model, torch.optim.Adadelta(model.parameters()), (B, 3, S, S))


def test_accumulate_kinds_refuse_data_parallel():
    from vub_image_denoising_amd.train_graph import TrainStepGraph

    class _Sync:
        world = 2
    model = _model()
    opt = _optimizer("adamw", model)
    _train_once(model, opt)
    model.unet._rdn_flat.grad_sync = _Sync()
    try:
        for kind in ("loss", "accum", "accum_step"):
            with pytest.raises(NotImplementedError):
                TrainStepGraph(model, opt, (B, 3, S, S), kind=kind)
    finally:
        model.unet._rdn_flat.grad_sync = None


def _train_once(model, opt):
    from vub_image_denoising_amd.diffusion_RDUnet import train_step_device
    noisy, clean = _batches(1)[0]
    train_step_device(model, clean.cuda(), noisy.cuda(), opt, 'uniform', 1.0, t=torch.tensor([3., 11.]).cuda())


@pytest.mark.parametrize("choice", ["adam", "adamw", "adadelta"])
def test_train_entry_in_graph_mode(choice, tmp_path, monkeypatch):
    """``--step_mode graph``: train(args) builds the fused optimizer and trains captured."""
    from vub_image_denoising_amd import diffusion_RDUnet as D
    from vub_image_denoising_amd import optim as fo
    monkeypatch.chdir(tmp_path)
    seen = {}
    inner = D.train_model_checkpointed

    def spy(model, train_loader, val_loader, optimizer, *a, **kw):
        seen.update(model=model, optimizer=optimizer, captured=kw.get("captured"),
                    before=[p.detach().clone() for p in model.parameters()])
        return inner(model, train_loader, val_loader, optimizer, *a, **kw)

    monkeypatch.setattr(D, "train_model_checkpointed", spy)
    args = D.build_parser().parse_args(["--step_mode", "graph", "--optimizer_choice", choice, "--base_filters", "16",
                                        "--num_epochs", "1", "--output_dir", str(tmp_path / "ck"), "--lr", "1e-2"])
    D.train(args, _batches(4), _batches(1, seed=5))
    want = {"adam": fo.FusedAdam, "adamw": fo.FusedAdamW, "adadelta": fo.FusedAdadelta}[choice]
    assert type(seen["optimizer"]) is want and seen["captured"] is True
    (graphs,) = seen["model"]._rdn_train_graphs.values()
    assert graphs.captures == 2 and seen["optimizer"]._step == 1          # (B2, loss), (B2, step)
    assert any(not torch.equal(a, b) for a, b in zip(seen["before"], seen["model"].parameters()))
    assert os.path.isfile(tmp_path / "ck" / "diffusion_RDUNet_model_checkpointed_final.pth")


# ------------------------------------------------------------------ against the fp64 oracle
NB = 8


def _oracle(mode, ts, data):
    """The trainers' loop restated on the CPU oracle in fp64, with torch.optim.Adadelta."""
    p0 = {"unet." + k: torch.from_numpy(v).double() for k, v in make_params(
        {k: v for k, v in R.param_shapes(16).items()}, 17).items()}
    leaves = {k: v.clone().requires_grad_(False) for k, v in p0.items()}
    opt = torch.optim.Adadelta(list(leaves.values()), lr=1.0)
    losses, acc = [], None
    for k, (noisy, clean) in enumerate(data):
        step_now = (k + 1) % 4 == 0
        loss, _, g, _ = R.train_step(leaves, clean.double(), noisy.double(), ts[k], T_STEPS,
                                     clip_value=1.0 if mode == "reference" else math.inf, prefix="unet.")
        losses.append(loss.item())
        if mode == "fixed":
            acc = g if acc is None else {n: acc[n] + g[n] for n in g}
        if step_now:
            grads = g if mode == "reference" else dict(zip(acc, R.clip_grad_norm(list(acc.values()), 1.0)[1]))
            for n, t in leaves.items():
                t.grad = grads[n]
            opt.step()
            acc = None
    return p0, leaves, losses


@pytest.mark.parametrize("mode", ["reference", "fixed"])
def test_captured_adadelta_vs_oracle(mode, tmp_path):
    """lr = 1.0: with the command line's 1e-4 the updates fall below an fp32 ulp of the
    parameters and fp32 against fp64 alone differs by 2.4e-2."""
    data = _batches(NB)
    model, opt, logged = _train(tmp_path, mode, "adadelta", 1, "uniform", True, epochs=1, data=data, val=False)
    torch.manual_seed(123)   # the run's t draws, replayed (the only CUDA RNG use)
    ts = [torch.randint(0, T_STEPS + 1, (B,), device="cuda").cpu() for _ in range(NB)]
    p0, ref, ref_losses = _oracle(mode, ts, data)
    got = [logged[i] for i in range(NB)]
    print(mode, "losses", np.round(got, 6), "oracle", np.round(ref_losses, 6))
    assert np.allclose(got, ref_losses, rtol=2e-4), (got, ref_losses)
    num = den = 0.0
    for n, prm in model.named_parameters():
        d = prm.detach().cpu().double() - p0[n]
        dr = ref[n].detach() - p0[n]
        num += float(((d - dr) ** 2).sum())
        den += float((dr ** 2).sum())
    dist = math.sqrt(num / den)
    print(f"{mode}: parameter-delta rel-L2 vs the fp64 oracle {dist:.3e} after {opt._step} updates")
    assert opt._step == NB // 4 and dist < 5e-2
