"""Host-side pieces of the plain RDUNet baseline's trainer (no GPU): the L1 symbols of
the C ABI and their argument validation, the baseline's own command line, the
captured trainer's optimizer check and the accumulate / clip / step schedule of
``RDUNet_model.train_model``."""
import ctypes
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_l1_symbols_declared_and_exported():
    from vub_image_denoising_amd import _hip as H
    src = open(os.path.join(REPO, "include", "rdunet_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = H.load_library()
    for name in ("rdn_l1_fwd", "rdn_l1_bwd"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), f"{name} is not declared in rdunet_hip.h"
        assert hasattr(lib, name), name
        assert name in H.SIGNATURES and len(H.SIGNATURES[name][1]) == 6


def test_l1_launchers_validate_on_the_host():
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    buf = (ctypes.c_float * 8)()
    p = ctypes.addressof(buf)   # never dereferenced: every call below is refused before a launch
    for fn, name, nptr in ((lib.rdn_l1_fwd, b"rdn_l1_fwd", (0, 1, 3, 4)), (lib.rdn_l1_bwd, b"rdn_l1_bwd", (0, 1, 3, 4))):
        for bad in nptr:
            a = [p, p, 4, p, p, None]
            a[bad] = None
            assert fn(*a) == -1, (name, bad)
            assert name in lib.rdn_last_error()
        for count in (0, -3):
            assert fn(p, p, count, p, p, None) == -1
            assert name in lib.rdn_last_error()


def test_baseline_parser_defaults():
    from vub_image_denoising_amd.RDUNet_model import build_parser
    a = vars(build_parser().parse_args([]))
    assert a == dict(dataset_choice='SIDD', checkpoint_path=None, num_epochs=300, batch_size=8, num_workers=8,
                     validation_split=0.2, augment=True, dataset_percentage=0.1, base_filters=128,
                     output_dir='checkpoints', lr=1e-4, weight_decay=1e-4, accumulation_steps=4, dtype='fp32',
                     step_mode='eager', data_pipeline='pil')
    b = build_parser().parse_args(["--step_mode", "graph", "--data_pipeline", "gpu", "--dtype", "bf16",
                                   "--base_filters", "64", "--accumulation_steps", "2"])
    assert (b.step_mode, b.data_pipeline, b.dtype, b.base_filters, b.accumulation_steps) == ("graph", "gpu", "bf16", 64, 2)
    for bad in (["--step_mode", "triton"], ["--dtype", "fp16"], ["--timesteps", "20"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)


def test_baseline_make_optimizer():
    from vub_image_denoising_amd import optim as fo
    from vub_image_denoising_amd.RDUNet_model import build_parser, make_optimizer
    args = build_parser().parse_args(["--lr", "3e-4", "--weight_decay", "2e-3"])
    for fused, cls in ((False, torch.optim.AdamW), (True, fo.FusedAdamW)):
        opt, sched = make_optimizer(args, [torch.nn.Parameter(torch.zeros(3))], fused=fused)
        assert type(opt) is cls and type(sched) is torch.optim.lr_scheduler.StepLR
        g = opt.param_groups[0]
        assert (g["lr"], g["weight_decay"]) == (3e-4, 2e-3) and (sched.step_size, sched.gamma) == (3, 0.5)


def test_captured_baseline_needs_a_fused_optimizer(tmp_path):
    from vub_image_denoising_amd.RDUNet_model import train_model
    model = torch.nn.Linear(2, 2)
    opt = torch.optim.AdamW(model.parameters())
    with pytest.raises(TypeError, match="fused optimizer"):
        train_model(model, [], None, opt, None, None, str(tmp_path), 1, captured=True)
    assert not list(tmp_path.iterdir())   # refused before the first epoch


class _Recorder(torch.optim.SGD):
    def __init__(self, params, log):
        super().__init__(params, lr=0.0)
        self.log = log

    def step(self, closure=None):
        self.log.append("step")

    def zero_grad(self, set_to_none=True):
        self.log.append("zero_grad")


def test_train_model_schedule(tmp_path, monkeypatch):
    """6 batches, accumulation_steps=4, two epochs: batches 1-3 accumulate, batch 4 clips and
    is followed by the only optimizer step of the epoch, batches 5-6 accumulate a partial
    group that the next epoch's zero_grad drops; no zero_grad between the batches of a
    group."""
    from vub_image_denoising_amd import RDUNet_model as M
    log = []
    model = torch.nn.Linear(2, 2)
    opt = _Recorder(model.parameters(), log)

    def step(model_, noisy, clean, optimizer, clip_value=1.0, zero_grad=False, clip=False):
        assert optimizer is opt and clip_value == 0.5 and not zero_grad
        log.append(("batch", int(noisy[0]), int(clean[0]), "clip" if clip else "accumulate"))
        return torch.tensor(float(noisy[0]))

    monkeypatch.setattr(M, "train_step_device", step)
    data = [(torch.tensor([k]), torch.tensor([10 + k])) for k in range(1, 7)]
    logged = {}

    class W:
        def add_scalar(self, tag, v, at):
            logged[(tag, at)] = v

    M.train_model(model, data, None, opt, None, W(), str(tmp_path), 2, accumulation_steps=4, clip_value=0.5,
                  log_every=4)
    epoch = (["zero_grad"] + [("batch", k, 10 + k, "accumulate") for k in (1, 2, 3)]
             + [("batch", 4, 14, "clip"), "step", "zero_grad"]
             + [("batch", k, 10 + k, "accumulate") for k in (5, 6)])
    assert log == epoch + epoch
    train = {k: v for k, v in logged.items() if k[0] == "Loss/train"}
    assert train == {("Loss/train", 0): 1.0, ("Loss/train", 4): 5.0, ("Loss/train", 6): 1.0, ("Loss/train", 10): 5.0}
    assert sorted(k[1] for k in logged if k[0] == "Loss/validation") == [1, 2]
    ck = torch.load(tmp_path / "RDUNet_model_epoch_2.pth", weights_only=True)
    assert sorted(ck) == ["epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"]
    assert ck["epoch"] == 2 and sorted(ck["model_state_dict"]) == ["bias", "weight"]


def test_load_checkpoint_takes_both_forms(tmp_path):
    from vub_image_denoising_amd.RDUNet_model import load_checkpoint
    from vub_image_denoising_amd.diffusion_RDUnet import save_epoch_checkpoint
    src = torch.nn.Linear(2, 2)
    opt = torch.optim.AdamW(src.parameters(), lr=0.25)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    opt.step()
    sched.step()
    save_epoch_checkpoint(src, opt, sched, 7, str(tmp_path / "epoch.pth"))
    torch.save(src.state_dict(), tmp_path / "bare.pth")
    for name, epoch, lr in (("epoch.pth", 7, 0.125), ("bare.pth", 0, 1.0)):
        dst = torch.nn.Linear(2, 2)
        o = torch.optim.AdamW(dst.parameters(), lr=1.0)
        s = torch.optim.lr_scheduler.StepLR(o, step_size=1, gamma=0.5)
        assert load_checkpoint(dst, o, s, str(tmp_path / name)) == epoch
        assert torch.equal(dst.weight, src.weight) and torch.equal(dst.bias, src.bias)
        assert o.param_groups[0]["lr"] == lr
    assert load_checkpoint(torch.nn.Linear(2, 2), None, None, str(tmp_path / "missing.pth")) == 0
