"""Forward-only engines and the module's mode (engine._run, UNetEngine._plan_splitk).

A forward-only engine plans split-K once, at construction, from ``module.training``:
eval-mode engines (the samplers) split the small-grid convs, train-mode ones (the logged
loss of a step whose gradient is discarded, ``forward_step_device``) keep the train
engine's single-pass kernels so that loss is the train step's bit for bit.  The engine
cache key has no mode in it, so ``_run`` keeps one forward-only engine per mode under a
shape's key and serves each call from the one whose ``module_training`` matches; these
tests switch one module between ``.train()`` and ``.eval()`` in both orders.

Shape: RDUNet_T(32), fp32, 1 x 3 x 64 x 64 -- the forward-only engine has split layers
there (tests/test_gpu_splitk.py)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _model(seed=0):
    import vub_image_denoising_amd as vm
    torch.manual_seed(seed)
    return vm.RDUNet_T(base_filters=32).cuda()


def _inputs():
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).cuda()
    t = torch.rand(1, 1, 1, 1, generator=g).cuda()
    return x, t


def _nograd(m, x, t):
    """A no-grad forward and the engine that served it (found by wrapping the engines'
    forward, not by position in the pool)."""
    from vub_image_denoising_amd import engine as E
    served = []
    orig = E.UNetEngine.forward

    def spy(self, xs, tt):
        served.append(self)
        return orig(self, xs, tt)

    E.UNetEngine.forward = spy
    try:
        with torch.no_grad():
            y = m(x, t).clone()
    finally:
        E.UNetEngine.forward = orig
    assert len(served) == 1 and not served[0].train
    return y, served[0]


def _nsplit(eng):
    return sum("splitk" in L.extra for L in eng.layers)


def test_eval_then_train_forward_only():
    from vub_image_denoising_amd import engine as E
    assert E.SPLITK
    m = _model()
    x, t = _inputs()
    m.eval()
    y_eval, e_eval = _nograd(m, x, t)
    assert _nsplit(e_eval) >= 1, "eval-mode forward-only engine must split"
    m.train()
    y_train, e_train = _nograd(m, x, t)
    assert e_train.module_training and _nsplit(e_train) == 0, \
        f"train-mode no-grad call served by an engine with {_nsplit(e_train)} split layers"
    y_grad = m(x, t).detach()            # grad-enabled: the train engine
    assert torch.equal(y_train, y_grad), "train-mode no-grad forward differs from the train engine's"
    # non-vacuity: split-K changes the fp32 summation order, so the two modes differ somewhere
    assert not torch.equal(y_eval, y_train), "split and unsplit outputs identical: split-K not engaged"
    # the key is unchanged and the first engine built stays at [0]
    pool = m._rdn_engines[(1, 64, 64, torch.float32, False)]
    assert pool[0] is e_eval and len(pool) == 2
    m.eval()
    y_eval2, e_eval2 = _nograd(m, x, t)
    assert e_eval2 is e_eval and torch.equal(y_eval2, y_eval) and len(pool) == 2


def test_train_then_eval_forward_only():
    x, t = _inputs()
    m = _model()
    m.train()
    _, e_train = _nograd(m, x, t)
    assert _nsplit(e_train) == 0
    m.eval()
    y_eval, e_eval = _nograd(m, x, t)
    assert not e_eval.module_training and _nsplit(e_eval) >= 1, \
        "eval call after a train-mode call of the same shape got no split-K"
    ref = _model().eval()                # same seed, same weights, only ever in eval mode
    y_ref, e_ref = _nograd(ref, x, t)
    assert _nsplit(e_ref) == _nsplit(e_eval)
    assert torch.equal(y_eval, y_ref)


def test_logged_loss_equals_train_step_loss_after_sampling():
    """diffusion_RDUnet.forward_step_device's loss is train_step_device's bit for bit, also
    after an eval-mode sampler call of the same shape built the first forward-only engine."""
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel, forward_step_device, train_step_device
    torch.manual_seed(0)
    dm = DiffusionModel(vm.RDUNet_T(base_filters=32), timesteps=5).cuda()
    g = torch.Generator().manual_seed(4)
    clean = (torch.rand(1, 3, 64, 64, generator=g) * 2 - 1).cuda()
    noisy = (clean + 0.2 * torch.randn(1, 3, 64, 64, generator=g).cuda()).clamp(-1, 1)
    dm.eval()
    with torch.no_grad():
        dm.improved_sampling(noisy)
        dm.direct_sampling(noisy)
    # the samplers left a split forward-only engine under the very key the train-mode
    # forward_step_device call below looks up (else this test says nothing)
    pool = dm.unet._rdn_engines.get((1, 64, 64, torch.float32, False), [])
    assert len(pool) == 1 and not pool[0].module_training and _nsplit(pool[0]) >= 1, list(dm.unet._rdn_engines)
    opt = torch.optim.SGD(dm.parameters(), lr=0.0, weight_decay=0.0)   # the weights never change
    dm.train()
    from vub_image_denoising_amd import engine as E
    served = []
    orig = E.UNetEngine.forward

    def spy(self, xs, tt):
        y = orig(self, xs, tt)
        served.append((self, y.detach().clone()))
        return y

    E.UNetEngine.forward = spy
    try:
        for step in range(1, 6):
            t = torch.tensor([step]).cuda()
            l_fwd = forward_step_device(dm, clean, noisy, t=t)
            l_step = train_step_device(dm, clean, noisy, opt, t=t)
            assert torch.equal(l_fwd, l_step), (step, l_fwd.item(), l_step.item())
    finally:
        E.UNetEngine.forward = orig
    # the loss is a mean over 3 x 64^2 values and hides a 7th-digit difference of single
    # pixels: also the denoised images behind the two losses are bit-identical, and the
    # logged-loss forwards ran on an unsplit forward-only engine
    assert len(served) == 10
    for (e_fwd, y_fwd), (e_step, y_step) in zip(served[0::2], served[1::2]):
        assert not e_fwd.train and e_step.train
        assert e_fwd.module_training and _nsplit(e_fwd) == 0
        assert torch.equal(y_fwd, y_step)
