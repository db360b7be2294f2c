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
