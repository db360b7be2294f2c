"""Host-side pieces of the captured trainers (no GPU): make_optimizer(fused=True),
the new command-line flags and their defaults, run_epochs(captured=True)'s optimizer
check, rdn_adadelta_step's argument validation and load_data's dispatch on
``--data_pipeline``."""
import ctypes

import pytest
import torch


def _args(**kw):
    from vub_image_denoising_amd.diffusion_RDUnet import build_parser
    a = build_parser().parse_args([])
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _params():
    return [torch.nn.Parameter(torch.zeros(3))]


@pytest.mark.parametrize("choice", ["adam", "adamw", "adadelta"])
def test_make_optimizer_fused(choice):
    from vub_image_denoising_amd import optim as fo
    from vub_image_denoising_amd.diffusion_RDUnet import make_optimizer
    args = _args(optimizer_choice=choice, lr=3e-4, weight_decay=2e-3)
    plain, plain_s = make_optimizer(args, _params())
    same, _ = make_optimizer(args, _params(), fused=False)
    fused, fused_s = make_optimizer(args, _params(), fused=True)
    want = {"adam": (torch.optim.Adam, fo.FusedAdam), "adamw": (torch.optim.AdamW, fo.FusedAdamW),
            "adadelta": (torch.optim.Adadelta, fo.FusedAdadelta)}[choice]
    assert type(plain) is want[0] and type(same) is want[0] and type(fused) is want[1]
    assert type(fused_s) is type(plain_s)
    assert fused_s.state_dict().keys() == plain_s.state_dict().keys()
    for k in ("T_max", "step_size", "gamma"):
        assert getattr(fused_s, k, None) == getattr(plain_s, k, None)
    gp, gf = plain.param_groups[0], fused.param_groups[0]
    for k, v in gf.items():   # every hyperparameter the fused class carries is the unfused call's
        if k != "params":
            assert gp[k] == v, (k, gp[k], v)
    assert gf["lr"] == 3e-4
    if choice == "adamw":
        assert gf["weight_decay"] == 2e-3 and fused.decoupled
    if choice == "adam":
        assert gf["weight_decay"] == 0 and not fused.decoupled and tuple(gf["betas"]) == (0.9, 0.999)
    if choice == "adadelta":
        assert (gf["rho"], gf["eps"], gf["weight_decay"]) == (0.9, 1e-6, 0)


def test_parser_flags_and_unchanged_defaults():
    a = vars(_args())
    assert a.pop("step_mode") == "eager" and a.pop("data_pipeline") == "pil"
    assert a == dict(dataset_choice='SIDD', checkpoint_path=None, num_epochs=300, batch_size=8, num_workers=8,
                     validation_split=0.2, augment=True, dataset_percentage=0.1, base_filters=32, timesteps=20,
                     optimizer_choice='adamw', scheduler_choice='step', output_dir='checkpoints', lr=1e-4,
                     weight_decay=1e-4, distribution_choice='uniform', dtype='fp32', accumulation='reference',
                     mse_weight=0.0, charbonnier_weight=1.0, ssim_weight=0.0)
    from vub_image_denoising_amd.diffusion_RDUnet import build_parser
    b = build_parser().parse_args(["--step_mode", "graph", "--data_pipeline", "gpu"])
    assert (b.step_mode, b.data_pipeline) == ("graph", "gpu")
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--step_mode", "triton"])


def test_captured_needs_a_fused_optimizer(tmp_path):
    from vub_image_denoising_amd.diffusion_RDUnet import run_epochs
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.AdamW(model.parameters())
    with pytest.raises(TypeError, match=r"make_optimizer\(\.\.\., fused=True\)"):
        run_epochs(model, [], None, opt, None, None, str(tmp_path), 'uniform', 1, 0, 4, 1.0, 1,
                   sample=None, captured=True)
    assert not list(tmp_path.iterdir())   # refused before the first epoch


def test_trainers_take_captured_keyword_only():
    import inspect
    from vub_image_denoising_amd import diffusion_RDUnet as a, diffusion_RDUnet_direct as c, main_diffusion_RDUnet as b
    for mod in (a, b, c):
        p = inspect.signature(mod.train_model_checkpointed).parameters["captured"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False, mod.__name__
    assert inspect.signature(a.run_epochs).parameters["captured"].default is False
    for mod in (b, c):
        assert inspect.signature(mod.make_training_objects).parameters["fused"].default is False


def test_adadelta_step_validates_on_the_host():
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)   # never dereferenced: every call below is refused before a launch
    for bad in range(4):
        ptrs = [p, p, p, p]
        ptrs[bad] = None
        assert lib.rdn_adadelta_step(*ptrs, 4, 1.0, 0.9, 1e-6, 0.0, 1.0, None) == -1
        assert b"rdn_adadelta_step: null" in lib.rdn_last_error()
    assert lib.rdn_adadelta_step(p, p, p, p, -1, 1.0, 0.9, 1e-6, 0.0, 1.0, None) == -1
    assert b"rdn_adadelta_step: count" in lib.rdn_last_error()


@pytest.mark.parametrize("dataset", ["DIV2K", "SIDD"])
def test_load_data_gpu_pipeline_dispatch(dataset, monkeypatch):
    from vub_image_denoising_amd import data_loader, synth
    from vub_image_denoising_amd.diffusion_RDUnet import load_data
    calls = []

    def fake(name):
        def f(folder, **kw):
            calls.append((name, folder, kw))
            return name + "_train", name + "_val"
        return f

    def pil(*a, **k):
        raise AssertionError("the PIL loader was called")

    monkeypatch.setattr(synth, "load_data_gpu", fake("div2k"))
    monkeypatch.setattr(synth, "load_sidd_data_gpu", fake("sidd"))
    monkeypatch.setattr(data_loader, "load_data", pil)
    monkeypatch.setattr(data_loader, "load_sidd_data", pil)
    args = _args(dataset_choice=dataset, data_pipeline="gpu", batch_size=5, dataset_percentage=0.5,
                 validation_split=0.25)
    out = load_data(args)
    name, folder = {"DIV2K": ("div2k", 'dataset/DIV2K_train_HR.nosync'),
                    "SIDD": ("sidd", 'dataset/SIDD_dataset.nosync/SIDD_Medium_Srgb')}[dataset]
    assert out == (name + "_train", name + "_val")
    assert calls == [(name, folder, dict(batch_size=5, augment=args.augment, dataset_percentage=0.5,
                                         validation_split=0.25, use_rgb=True))]


# ------------------------------------------------------------------ the epoch loop's schedule
def _batches():
    return [(torch.tensor([float(k)]), torch.tensor([10.0 + k])) for k in range(1, 7)]   # (noisy, clean)


class _Writer:
    def __init__(self):
        self.logged = {}

    def add_scalar(self, tag, v, at):
        self.logged[(tag, at)] = v


@pytest.mark.parametrize("mode,skip", [("reference", True), ("reference", False), ("fixed", True)])
def test_run_epochs_schedule(mode, skip, tmp_path, monkeypatch):
    """The diffusion loop's counterpart of test_baseline_cpu.test_train_model_schedule: 6 batches,
    accumulation_steps=4, two epochs.  'reference': only batch 4 trains (zero_grad and clip inside
    the step) and is followed by the epoch's one optimizer step; the other batches only draw t,
    with the loss where it is logged -- or, ``skip_discarded=False``, train too.  'fixed': every
    batch adds its gradient (no zero_grad, no clip), batch 4 is followed by one clip_grad_norm_
    over the model's parameters, then the step.  Batches 5-6 leave a partial group that the next
    epoch's zero_grad drops."""
    from test_baseline_cpu import _Recorder
    from vub_image_denoising_amd import diffusion_RDUnet as D
    from vub_image_denoising_amd import functional as Fn
    log = []
    model = torch.nn.Linear(2, 2)
    opt = _Recorder(model.parameters(), log)

    def train(model_, clean, noisy, optimizer, distribution_choice='uniform', clip_value=0.1, t=None, zero_grad=True,
              clip=True, loss_weights=None):
        assert model_ is model and optimizer is opt and distribution_choice == 'biased' and clip_value == 0.5
        assert t is None and loss_weights == (0.25, 0.5, 0.25) and float(clean[0]) == 10 + float(noisy[0])
        log.append(("train", int(noisy[0]), zero_grad, clip))
        return torch.tensor(float(noisy[0]))

    def forward(model_, clean, noisy, distribution_choice='uniform', t=None, need_loss=True, loss_weights=None):
        assert model_ is model and distribution_choice == 'biased' and t is None
        assert float(clean[0]) == 10 + float(noisy[0])
        log.append(("forward", int(noisy[0]), need_loss))
        return torch.tensor(float(noisy[0])) if need_loss else None

    def clip_grad_norm_(parameters, max_norm, *a, **kw):
        assert [id(p) for p in parameters] == [id(p) for p in model.parameters()]
        log.append(("clip_grad_norm_", max_norm))

    monkeypatch.setattr(D, "train_step_device", train)
    monkeypatch.setattr(D, "forward_step_device", forward)
    monkeypatch.setattr(Fn, "clip_grad_norm_", clip_grad_norm_)
    w = _Writer()
    D.run_epochs(model, _batches(), None, opt, None, w, str(tmp_path), 'biased', 2, 0, 4, 0.5, 4, sample=None,
                 accumulation=mode, skip_discarded=skip, loss_weights=(0.25, 0.5, 0.25))
    if mode == "fixed":
        epoch = (["zero_grad"] + [("train", k, False, False) for k in (1, 2, 3, 4)]
                 + [("clip_grad_norm_", 0.5), "step", "zero_grad"] + [("train", k, False, False) for k in (5, 6)])
    elif skip:
        epoch = (["zero_grad", ("forward", 1, True), ("forward", 2, False), ("forward", 3, False),
                  ("train", 4, True, True), "step", "zero_grad", ("forward", 5, True), ("forward", 6, False)])
    else:
        epoch = (["zero_grad"] + [("train", k, True, True) for k in (1, 2, 3, 4)] + ["step", "zero_grad"]
                 + [("train", k, True, True) for k in (5, 6)])
    assert log == epoch + epoch
    train_tags = {k: v for k, v in w.logged.items() if k[0] == "Loss/train"}
    assert train_tags == {("Loss/train", 0): 1.0, ("Loss/train", 4): 5.0, ("Loss/train", 6): 1.0,
                          ("Loss/train", 10): 5.0}
    assert sorted(k[1] for k in w.logged if k[0] == "Loss/validation") == [1, 2]
    assert not any(k[0] == "Loss/validation_ema" for k in w.logged)
    assert sorted(p.name for p in tmp_path.iterdir()) == [
        f"diffusion_RDUNet_model_checkpointed_epoch_{e}.pth" for e in (1, 2)]
    ck = torch.load(tmp_path / "diffusion_RDUNet_model_checkpointed_epoch_2.pth", weights_only=True)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert ck["epoch"] == 2 and sorted(ck["model_state_dict"]) == ["bias", "weight"]


class _StubEMA:
    """What the loops use of an optim.EMA beside an optimizer that is not fused."""

    def __init__(self, log):
        self.log = log

    def use_names_of(self, model):
        return self

    def bind(self):
        self.log.append("bind")

    def update(self):
        self.log.append("update")

    def applied(self):
        import contextlib

        @contextlib.contextmanager
        def cm():
            self.log.append("applied")
            try:
                yield self
            finally:
                self.log.append("restored")
        return cm()

    def state_dict(self):
        return {"decay": 0.5, "warmup": False, "num_updates": self.log.count("update"), "shadow": {}}


@pytest.mark.parametrize("trainer", ["diffusion_reference", "diffusion_fixed", "baseline"])
def test_unfused_ema_order_in_both_loops(trainer, tmp_path, monkeypatch):
    """Beside a torch optimizer both loops keep the average themselves: ``bind, step, update,
    zero_grad`` after the stepping batch; the validation batch is evaluated with the raw weights
    and again inside ``ema.applied()`` (``Loss/validation_ema``), and the checkpoint gains
    ``ema_state_dict``."""
    from test_baseline_cpu import _Recorder
    from vub_image_denoising_amd import RDUNet_model as M
    from vub_image_denoising_amd import diffusion_RDUnet as D
    from vub_image_denoising_amd import functional as Fn
    log = []
    model = torch.nn.Linear(2, 2)
    opt = _Recorder(model.parameters(), log)
    ema = _StubEMA(log)

    def train(*a, **k):
        log.append("train")
        return torch.tensor(1.0)

    def forward(*a, need_loss=True, **k):
        log.append("forward")
        return torch.tensor(1.0) if need_loss else None

    def val_loss(*a, **k):   # one validation batch, on the CPU: 2.0 with the raw weights, 3.0 inside applied()
        log.append("val")
        return torch.tensor(3.0 if log[-2] == "applied" else 2.0)

    monkeypatch.setattr(D, "train_step_device", train)
    monkeypatch.setattr(D, "forward_step_device", forward)
    monkeypatch.setattr(M, "train_step_device", train)
    monkeypatch.setattr(Fn, "clip_grad_norm_", lambda *a, **k: log.append("clip_grad_norm_"))
    monkeypatch.setattr(D, "combined_loss", val_loss)
    monkeypatch.setattr(M, "forward_loss_device", val_loss)
    w = _Writer()
    data, val = _batches()[:4], _batches()[:1]
    if trainer == "baseline":
        M.train_model(model, data, val, opt, None, w, str(tmp_path), 1, accumulation_steps=4, clip_value=0.5, ema=ema)
        name = "RDUNet_model_epoch_1.pth"
        batches = ["train"] * 4
    else:
        mode = trainer.split("_")[1]
        D.run_epochs(model, data, val, opt, None, w, str(tmp_path), 'uniform', 1, 0, 4, 0.5, 1,
                     sample=lambda m, x: x, accumulation=mode, ema=ema)
        name = "diffusion_RDUNet_model_checkpointed_epoch_1.pth"
        batches = ["forward"] * 3 + ["train"] if mode == "reference" else ["train"] * 4 + ["clip_grad_norm_"]
    assert log == ["zero_grad"] + batches + ["bind", "step", "update", "zero_grad", "val", "applied", "val", "restored"]
    assert w.logged[("Loss/validation", 1)] == 2.0 and w.logged[("Loss/validation_ema", 1)] == 3.0
    ck = torch.load(tmp_path / name, weights_only=True)
    assert sorted(ck) == ["ema_state_dict", "epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert ck["ema_state_dict"]["num_updates"] == 1
