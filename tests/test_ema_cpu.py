"""Host side of the weight EMA (no GPU): the decay schedule, the float64 reference of the
GPU tests against its closed form, the trainers' flags (no EMA by default), the names of
``EMA.state_dict()['shadow']``, the checkpoint keys, ``load_model(weights='ema')``, and
the C ABI's declarations, exports and argument checks."""
import ctypes
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_ref as ER  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rdn_ema_update", "rdn_adam_step_ema", "rdn_adadelta_step_ema")


@pytest.mark.parametrize("fn", ["optim", "ref"])
def test_decay_schedule(fn):
    from vub_image_denoising_amd.optim import ema_decay_at
    f = ema_decay_at if fn == "optim" else ER.decay_at
    assert f(0.9999, True, 0) == 0.1
    assert f(0.9999, True, 1) == 2.0 / 11.0
    assert f(0.5, True, 7) == 8.0 / 17.0 and f(0.5, True, 8) == 0.5 and f(0.5, True, 9) == 0.5   # 9/18 reaches the cap
    assert f(0.9999, True, 5000) == 5001.0 / 5010.0
    assert f(0.9999, True, 10 ** 6) == 0.9999
    assert f(0.0, True, 0) == 0.0
    for n in (0, 1, 5000):
        for d in (0.0, 0.5, 0.9999):
            assert f(d, False, n) == d


def test_reference_weight_is_rounded_once_from_double():
    assert ER.weight32(0.9999, False, 3) == np.float32(1.0 - 0.9999)
    assert ER.weight32(0.9999, True, 0) == np.float32(0.9)
    assert ER.weight32(0.9999, True, 1) == np.float32(1.0 - 2.0 / 11.0)


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9999])
def test_recurrence_against_closed_form(decay):
    rng = np.random.default_rng(3)
    e0 = rng.standard_normal(64).astype(np.float32)
    p = rng.standard_normal(64).astype(np.float32)
    w = ER.weight32(decay, False, 0)
    for steps in (1, 5, 200):
        rec, closed = ER.recurrence(e0, p, w, steps), ER.closed_form(e0, p, w, steps)
        # float64 rounding of `steps` updates, each of magnitude <= max(|e0|, |p|)
        tol = 4 * steps * np.finfo(np.float64).eps * np.maximum(np.abs(e0), np.abs(p)).astype(np.float64)
        assert np.all(np.abs(rec - closed) <= tol), (decay, steps, np.abs(rec - closed).max())
    if decay == 0.0:
        assert np.array_equal(ER.recurrence(e0, p, w, 1), p.astype(np.float64))   # w = 1: the average is p


def _parsers():
    from vub_image_denoising_amd import RDUNet_model, diffusion_RDUnet, diffusion_RDUnet_direct, main_diffusion_RDUnet
    return {"diffusion": diffusion_RDUnet.build_parser, "main": main_diffusion_RDUnet.build_parser,
            "direct": diffusion_RDUnet_direct.build_parser, "baseline": RDUNet_model.build_parser}


@pytest.mark.parametrize("trainer", ["diffusion", "main", "direct", "baseline"])
def test_parsers_default_to_no_ema(trainer):
    from vub_image_denoising_amd.diffusion_RDUnet import make_ema
    build = _parsers()[trainer]
    a = build().parse_args([])
    assert getattr(a, "ema_decay", 0.0) == 0.0 and getattr(a, "ema_warmup", False) is False
    assert make_ema(a, torch.nn.Linear(2, 2)) is None
    assert make_ema(build().parse_args(["--ema_decay", "0"]), torch.nn.Linear(2, 2)) is None
    assert make_ema(build().parse_args(["--ema_warmup"]), torch.nn.Linear(2, 2)) is None     # no decay: no EMA
    a = build().parse_args(["--ema_decay", "0.999", "--ema_warmup"])
    assert a.ema_decay == 0.999 and a.ema_warmup is True
    ema = make_ema(a, torch.nn.Linear(2, 2))
    assert (ema.decay, ema.warmup, ema.num_updates) == (0.999, True, 0)


def test_denoise_image_weights_flag():
    from vub_image_denoising_amd.denoise_image import build_parser
    base = ["--checkpoint", "c", "--input", "i", "--output", "o"]
    assert build_parser().parse_args(base).weights == "model"
    assert build_parser().parse_args(base + ["--weights", "ema"]).weights == "ema"


def _models():
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    from vub_image_denoising_amd.RDUNet_model import RDUNet
    torch.manual_seed(0)
    return {"diffusion": DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=20), "baseline": RDUNet(base_filters=16)}


@pytest.mark.parametrize("kind", ["diffusion", "baseline"])
@pytest.mark.parametrize("how", ["model", "params"])
def test_state_dict_names_are_the_models(kind, how):
    from vub_image_denoising_amd.optim import EMA, shadow_names
    model = _models()[kind]
    ema = EMA(model, 0.999) if how == "model" else EMA(model.parameters(), 0.999, warmup=True).use_names_of(model)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "num_updates", "shadow"}
    assert (sd["decay"], sd["warmup"], sd["num_updates"]) == (0.999, how == "params", 0)
    assert list(sd["shadow"]) == list(model.state_dict()) == shadow_names(model, list(model.parameters()))
    assert all(k.startswith("unet.") for k in sd["shadow"]) == (kind == "diffusion")
    assert any(k.startswith("unet.") for k in sd["shadow"]) == (kind == "diffusion")
    for k, v in model.state_dict().items():       # before any update the average is the weights
        assert torch.equal(sd["shadow"][k], v), k
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    back = torch.load(buf, weights_only=True)     # tensors and plain numbers only
    fresh = _models()[kind]
    fresh.load_state_dict(back["shadow"])
    other = EMA(fresh, 0.5)
    other.load_state_dict(back)                   # before the first bind: held, and saved again as loaded
    assert (other.decay, other.warmup, other.num_updates) == (0.999, how == "params", 0)
    assert list(other.state_dict()["shadow"]) == list(sd["shadow"])


def test_ema_refuses_foreign_parameters_and_bad_decay():
    from vub_image_denoising_amd.optim import EMA
    a, b = torch.nn.Linear(2, 2), torch.nn.Linear(2, 2)
    with pytest.raises(ValueError):
        EMA(a.parameters(), 0.9).use_names_of(b)
    for d in (-0.1, 1.5):
        with pytest.raises(ValueError):
            EMA(a, d)


def test_checkpoint_keys_and_ema_weight_loading(tmp_path, capsys):
    from vub_image_denoising_amd import denoise_image
    from vub_image_denoising_amd.diffusion_RDUnet import ema_weights, load_checkpoint, save_epoch_checkpoint
    from vub_image_denoising_amd.optim import EMA
    model = _models()["diffusion"]
    opt = torch.optim.AdamW(model.parameters(), lr=1e-3)
    plain, with_ema = str(tmp_path / "plain.pth"), str(tmp_path / "ema.pth")
    save_epoch_checkpoint(model, opt, None, 3, plain)
    ck = torch.load(plain, weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"}
    # an average that differs from the weights: loaded as a shadow before any bind
    ema = EMA(model, 0.99)
    sd = ema.state_dict()
    sd["num_updates"] = 7
    sd["shadow"] = {k: v + 1.0 for k, v in sd["shadow"].items()}
    ema.load_state_dict(sd)
    save_epoch_checkpoint(model, opt, None, 3, with_ema, ema=ema)
    ck = torch.load(with_ema, weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "ema_state_dict"}
    assert ck["ema_state_dict"]["num_updates"] == 7
    loaded = denoise_image.load_model(with_ema, base_filters=16, device="cpu", weights="ema")
    raw = denoise_image.load_model(with_ema, base_filters=16, device="cpu")
    for (k, a), b in zip(loaded.state_dict().items(), raw.state_dict().values()):
        assert torch.equal(a, b + 1.0) and torch.equal(b, model.state_dict()[k]), k
    with pytest.raises(KeyError, match="no EMA weights"):
        denoise_image.load_model(plain, base_filters=16, device="cpu", weights="ema")
    with pytest.raises(KeyError, match="no EMA weights"):
        ema_weights(model.state_dict(), "bare")
    with pytest.raises(ValueError):
        denoise_image.load_model(plain, base_filters=16, device="cpu", weights="shadow")
    # a wanted EMA and a checkpoint without one: restarted from the loaded weights, one line says so
    fresh = _models()["diffusion"]
    e2 = EMA(fresh, 0.99)
    e2.load_state_dict(sd)
    capsys.readouterr()
    assert load_checkpoint(fresh, torch.optim.AdamW(fresh.parameters(), lr=1e-3), None, plain, ema=e2) == 3
    assert capsys.readouterr().out.count("no EMA") == 1
    assert e2.num_updates == 0
    for k, v in e2.state_dict()["shadow"].items():
        assert torch.equal(v, model.state_dict()[k]), k
    e3 = EMA(fresh, 0.5)
    assert load_checkpoint(fresh, torch.optim.AdamW(fresh.parameters(), lr=1e-3), None, with_ema, ema=e3) == 3
    assert (e3.decay, e3.num_updates) == (0.99, 7)
    for k, v in e3.state_dict()["shadow"].items():
        assert torch.equal(v, model.state_dict()[k] + 1.0), k


def test_header_declares_and_library_exports_ema():
    from vub_image_denoising_amd import _hip as H
    with open(os.path.join(REPO, "include", "rdunet_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(H.LIB_PATH)
    for name in NAMES:
        assert name + "(" in header, name
        assert hasattr(lib, name), name
        assert name in H.SIGNATURES, name
    assert header.count("no reference counterpart") >= 3


def test_bad_arguments_fail_on_the_host():
    """RDN_E_ARG before any launch (the fake pointers are never dereferenced); count == 0 is
    a no-op that launches nothing either."""
    from vub_image_denoising_amd import _hip as H
    lib = H.load_library()
    fake = 4096
    ok = [fake, fake, 16, 0.5, 0, 0, None, None]   # ema, p, count, decay, warmup, n, n_dev, stream
    for i, bad in ((0, None), (1, None), (2, -1), (3, -0.1), (3, 1.5), (3, float("nan")), (5, -1)):
        args = list(ok)
        args[i] = bad
        assert lib.rdn_ema_update(*args) == -1, (i, bad)
        assert b"rdn_ema_update" in lib.rdn_last_error()
    assert lib.rdn_ema_update(fake, fake, 0, 0.5, 1, 3, None, None) == 0
    adam = [fake, fake, fake, fake, 16, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, None, 1.0]
    adadelta = [fake, fake, fake, fake, 16, 1.0, 0.9, 1e-6, 0.0, 1.0]
    for fn, head in ((lib.rdn_adam_step_ema, adam), (lib.rdn_adadelta_step_ema, adadelta)):
        for tail in ([None, 0.5, 0, 0, None], [fake, 1.5, 0, 0, None], [fake, -0.5, 1, 0, None], [fake, 0.5, 0, -2, None]):
            assert fn(*head, *tail, None) == -1, tail
        bad_head = list(head)
        bad_head[0] = None
        assert fn(*bad_head, fake, 0.5, 0, 0, None, None) == -1
    assert lib.rdn_adadelta_step_ema(fake, fake, fake, fake, 0, 1.0, 0.9, 1e-6, 0.0, 1.0, fake, 0.5, 0, 0, None, None) == 0
