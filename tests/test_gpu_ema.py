"""The weight EMA on the GPU: rdn_ema_update against the float64 reference step by step,
the fused optimizer entries (rdn_adam_step_ema / rdn_adadelta_step_ema) bit for bit against
the plain entry followed by rdn_ema_update, optim.EMA on the network (attached to a fused
optimizer, beside torch.optim.AdamW), inside captured train steps (warm-up roll-back,
re-capture, accumulation, a bare RDUNet, node counts), swapped into the weights for
sampling, and through the trainers' checkpoints (resume continues bit for bit)."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _ema_ref as ER  # noqa: E402

STEPS = 5
GUARD = 8        # elements around each buffer that a kernel must not touch
SHAPE = (2, 3, 32, 32)


def _buf(count, offset, values=None):
    whole = torch.full((offset + count + GUARD,), 7.0, device="cuda")
    v = whole[offset:offset + count]
    if values is not None:
        v.copy_(values)
    return whole, v


def _untouched(whole, offset, count):
    return bool(torch.all(whole[:offset] == 7.0) and torch.all(whole[offset + count:] == 7.0))


# ----------------------------------------------------------------- the kernel alone
@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9999])
@pytest.mark.parametrize("count,offset", [(1, 0), (255, 0), (1027, 0), (255, 1)])
def test_ema_kernel_against_reference(count, offset, decay):
    """Warm-up off, and on with the device counter starting at 0, 1 and 5000.  Each of 5
    updates is compared with the float64 value of e + w (p - e) of the GPU's own fp32
    inputs, bound 2 ulp32(max(|e|, |p|)) (tests/_ema_ref.py::bound).  offset 1: buffers
    that are not 16-byte aligned (the scalar loop alone)."""
    from vub_image_denoising_amd import _hip as H
    lib = H.lib()
    for warmup, n0 in ((0, 0), (1, 0), (1, 1), (1, 5000)):
        g = torch.Generator(device="cuda").manual_seed(31 * count + n0)
        ew, e = _buf(count, offset, torch.randn(count, generator=g, device="cuda"))
        hw, e_host = _buf(count, offset, e)           # the same updates with the count passed from the host
        pw, p = _buf(count, offset)
        n_dev = torch.full((), n0, dtype=torch.int64, device="cuda") if warmup else None
        worst = 0.0
        for step in range(STEPS):
            p.copy_(torch.randn(count, generator=g, device="cuda") * (10.0 ** (step - 2)))
            e0, p0 = e.cpu().numpy(), p.cpu().numpy()
            H.check(lib.rdn_ema_update(e.data_ptr(), p.data_ptr(), count, decay, warmup, 0, H.ptr(n_dev),
                                       H.stream_ptr()), "ema_update")
            if warmup:
                H.check(lib.rdn_counter_inc(n_dev.data_ptr(), H.stream_ptr()), "counter_inc")
            H.check(lib.rdn_ema_update(e_host.data_ptr(), p.data_ptr(), count, decay, warmup, n0 + step, None,
                                       H.stream_ptr()), "ema_update")
            ref = ER.step(e0, p0, ER.weight32(decay, warmup, n0 + step))
            got = e.cpu().numpy().astype(np.float64)
            ratio = float((np.abs(got - ref) / ER.bound(e0, p0)).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, (warmup, n0, step, ratio)
            assert torch.equal(e, e_host), (warmup, n0, step)   # device-derived weight == host-derived weight
        print(f"count {count} offset {offset} decay {decay} warmup {warmup} n0 {n0}: worst |err| / bound {worst:.3f}")
        if warmup:
            assert int(n_dev) == n0 + STEPS
        assert _untouched(ew, offset, count) and _untouched(pw, offset, count) and _untouched(hw, offset, count)


def test_ema_kernel_count_zero_touches_nothing():
    from vub_image_denoising_amd import _hip as H
    ew, e = _buf(16, 0, torch.arange(16.0))
    pw, p = _buf(16, 0, torch.ones(16))
    before = ew.clone()
    n_dev = torch.full((), 3, dtype=torch.int64, device="cuda")
    assert H.lib().rdn_ema_update(e.data_ptr(), p.data_ptr(), 0, 0.5, 1, 0, n_dev.data_ptr(), H.stream_ptr()) == 0
    torch.cuda.synchronize()
    assert torch.equal(ew, before) and int(n_dev) == 3


# ----------------------------------------------------------------- the fused entries
def _optim_call(kind, lib, p, g, s1, s2, count, step, wd, gs, ema_args=None):
    from vub_image_denoising_amd import _hip as H
    st = H.stream_ptr()
    if kind == "adadelta":
        head = (p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), count, 1.0, 0.9, 1e-6, wd, gs)
        plain, fused = lib.rdn_adadelta_step, lib.rdn_adadelta_step_ema
    else:
        head = (p.data_ptr(), g.data_ptr(), s1.data_ptr(), s2.data_ptr(), count, 1e-3, 0.9, 0.999, 1e-8, wd,
                1 if kind == "adamw" else 0, step, None, gs)
        plain, fused = lib.rdn_adam_step, lib.rdn_adam_step_ema
    if ema_args is None:
        H.check(plain(*head, st), kind)
    else:
        H.check(fused(*head, *ema_args, st), kind + "_ema")


@pytest.mark.parametrize("warmup", [0, 1])
@pytest.mark.parametrize("weight_decay", [0.0, 1e-2])
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("count,offset", [(1027, 0), (255, 1)])
@pytest.mark.parametrize("kind", ["adam", "adamw", "adadelta"])
def test_fused_entries_equal_plain_entry_plus_ema_update(kind, count, offset, grad_scale, weight_decay, warmup):
    """p and both moment buffers get the plain entry's bits, the shadow the bits of
    rdn_ema_update run behind the plain entry; gradients include exact zeros."""
    from vub_image_denoising_amd import _hip as H
    lib = H.lib()
    g = torch.Generator(device="cuda").manual_seed(5 + count)
    init = torch.randn(count, generator=g, device="cuda")
    shadow0 = torch.randn(count, generator=g, device="cuda")
    sides = []
    for _ in range(2):   # 0: plain entry + rdn_ema_update, 1: the fused entry
        sides.append(dict(p=_buf(count, offset, init), s1=_buf(count, offset, torch.zeros(count)),
                          s2=_buf(count, offset, torch.zeros(count)), e=_buf(count, offset, shadow0),
                          n=torch.zeros((), dtype=torch.int64, device="cuda")))
    gw, grad = _buf(count, offset)
    for step in range(STEPS):
        grad.copy_(torch.randn(count, generator=g, device="cuda") * 1e-2)
        grad[step % count::3] = 0.0
        for k, s in enumerate(sides):
            n_dev = s["n"].data_ptr() if warmup else None
            ema_args = (s["e"][1].data_ptr(), 0.9, warmup, step, n_dev)
            _optim_call(kind, lib, s["p"][1], grad, s["s1"][1], s["s2"][1], count, step + 1, weight_decay, grad_scale,
                        ema_args if k == 1 else None)
            if k == 0:
                H.check(lib.rdn_ema_update(s["e"][1].data_ptr(), s["p"][1].data_ptr(), count, 0.9, warmup, step, n_dev,
                                           H.stream_ptr()), "ema_update")
            H.check(lib.rdn_counter_inc(s["n"].data_ptr(), H.stream_ptr()), "counter_inc")
    a, b = sides
    for key in ("p", "s1", "s2", "e"):
        assert torch.equal(a[key][0], b[key][0]), key         # whole buffers: the guards too
        assert _untouched(b[key][0], offset, count), key
    assert not torch.equal(b["e"][1], shadow0) and not torch.equal(b["p"][1], init)
    assert _untouched(gw, offset, count)


# ----------------------------------------------------------------- on the network
def _model_with_grads(seed=0, bf=16):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel, train_step_device
    torch.manual_seed(seed)
    model = DiffusionModel(vm.RDUNet_T(base_filters=bf), timesteps=4).cuda()
    g = torch.Generator().manual_seed(seed + 1)
    clean = (torch.rand(SHAPE, generator=g) * 2 - 1).cuda()
    noisy = clean + 0.1 * torch.randn(SHAPE, generator=g).cuda()

    class _Z:
        def zero_grad(self, set_to_none=True):
            for p in model.parameters():
                p.grad = None
    train_step_device(model, clean, noisy, _Z(), clip_value=1.0, t=torch.tensor([3, 1]).cuda())
    return model


def _set_grads(model, step):
    """Deterministic per-step gradients written into the flat gradient views."""
    g = torch.Generator(device="cuda").manual_seed(100 + step)
    for p in model.parameters():
        p.grad.copy_(torch.randn(p.shape, generator=g, device="cuda") * 1e-2)


def _gaps(fp):
    """Indices of the flat layout that belong to no parameter."""
    used = torch.zeros(fp.numel, dtype=torch.bool)
    for p, off in zip(fp.params, fp.offsets):
        used[off:off + p.numel()] = True
    return (~used).nonzero().flatten().cuda()


def _fused(kind, model, lr=None):
    from vub_image_denoising_amd.optim import FusedAdadelta, FusedAdam, FusedAdamW
    if kind == "adam":
        return FusedAdam(model.parameters(), lr=lr or 1e-3)
    if kind == "adamw":
        return FusedAdamW(model.parameters(), lr=lr or 1e-3, weight_decay=1e-2)
    return FusedAdadelta(model.parameters(), lr=lr or 1.0)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("kind", ["adam", "adamw", "adadelta"])
def test_attached_ema_equals_separate_update(kind, warmup):
    from vub_image_denoising_amd.optim import EMA
    mA, mB = _model_with_grads(), _model_with_grads()
    oA, oB = _fused(kind, mA), _fused(kind, mB)
    eA, eB = EMA(mA, 0.9, warmup=warmup), EMA(mB.parameters(), 0.9, warmup=warmup)
    oA.attach_ema(eA)
    eB.bind()                                  # the average starts as the weights before the first step
    start = eB._shadow.clone()
    assert torch.equal(start, eB._fp.flat)
    for step in range(STEPS):
        _set_grads(mA, step)
        _set_grads(mB, step)
        oA.step()
        oB.step()
        eB.update()
    assert torch.equal(eA._fp.flat, eB._fp.flat)
    assert torch.equal(eA._shadow, eB._shadow) and not torch.equal(eA._shadow, start)
    assert not torch.equal(eA._shadow, eA._fp.flat)
    gaps = _gaps(eA._fp)
    assert gaps.numel() > 0
    assert torch.all(eA._shadow[gaps] == 0) and torch.all(eA._fp.flat[gaps] == 0)
    assert eA.num_updates == eB.num_updates == STEPS
    if warmup:
        assert int(eA._n_dev) == int(eB._n_dev) == STEPS
    else:
        assert eA._n_dev is None and eB._n_dev is None
    assert len(oA.graph_buffers()) == len(oB.graph_buffers()) + (2 if warmup else 1)
    assert oA.graph_key() != oB.graph_key()
    # the names: the model's own for an EMA built from the model, the network's bare ones otherwise
    assert list(eA.state_dict()["shadow"]) == list(mA.state_dict())
    assert list(eB.state_dict()["shadow"]) == [k[5:] for k in mB.state_dict()]
    # reset_state leaves the average alone
    kept = eA._shadow.clone()
    oA.reset_state()
    assert torch.equal(eA._shadow, kept) and eA.num_updates == STEPS and oA._step == 0


def test_torch_adamw_with_separate_ema_update():
    """The eager trainers' path: torch.optim's in-place step writes through the parameter
    views into the flat buffer, ema.update() follows it; every update within the kernel's bound."""
    from vub_image_denoising_amd.optim import EMA
    model = _model_with_grads()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-2)
    ema = EMA(model, 0.9, warmup=True)
    ema.bind()
    for step in range(STEPS):
        _set_grads(model, step)
        opt.step()
        e0, p0 = ema._shadow.cpu().numpy(), ema._fp.flat.cpu().numpy()
        ema.update()
        ref = ER.step(e0, p0, ER.weight32(0.9, True, step))
        assert np.all(np.abs(ema._shadow.cpu().numpy().astype(np.float64) - ref) <= ER.bound(e0, p0))
        assert not np.array_equal(ema._shadow.cpu().numpy(), e0)
    assert ema.num_updates == int(ema._n_dev) == STEPS


# ----------------------------------------------------------------- captured
def _batches(n, shape=SHAPE, seed=11):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        clean = torch.rand(shape, generator=g) * 2 - 1
        noisy = clean + 0.2 * torch.randn(shape, generator=g)
        t = torch.randint(0, 5, (shape[0],), generator=g).float()
        out.append((clean.cuda(), noisy.cuda(), t.cuda()))
    return out


def _model(seed=0):
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.diffusion_RDUnet import DiffusionModel
    torch.manual_seed(seed)
    return DiffusionModel(vm.RDUNet_T(base_filters=16), timesteps=4).cuda()


def _eager_step(model, opt, clean, noisy, t):
    from vub_image_denoising_amd.diffusion_RDUnet import train_step_device
    loss = train_step_device(model, clean, noisy, opt, 'uniform', 1.0, t=t)
    opt.step()
    return loss


def _same(mA, oA, eA, mB, oB, eB, updates):
    for (n, a), b in zip(mA.named_parameters(), mB.parameters()):
        assert torch.equal(a, b), n
    for a, b in zip(oA.graph_buffers(), oB.graph_buffers()):   # moments, shadow, device counter
        assert torch.equal(a, b)
    assert oA._step == oB._step == updates
    assert torch.equal(eA._shadow, eB._shadow) and not torch.equal(eA._shadow, eA._fp.flat)
    assert eA.num_updates == eB.num_updates == updates
    if eA.warmup:
        assert int(eA._n_dev) == int(eB._n_dev) == updates


@pytest.mark.parametrize("kind,warmup", [("adamw", True), ("adamw", False), ("adadelta", True)])
def test_captured_step_equals_eager(kind, warmup):
    """Six 'step' replays, then an LR change (re-capture) and two more."""
    from vub_image_denoising_amd.optim import EMA
    from vub_image_denoising_amd.train_graph import TrainStepGraphs
    data = _batches(4)
    mA, mB = _model(), _model()
    oA, oB = _fused(kind, mA), _fused(kind, mB)
    eA, eB = EMA(mA, 0.99, warmup=warmup), EMA(mB, 0.99, warmup=warmup)
    oA.attach_ema(eA)
    oB.attach_ema(eB)
    graphs = TrainStepGraphs(mB, oB, t_input=True)
    for k in range(6):
        clean, noisy, t = data[k % 4]
        assert torch.equal(_eager_step(mA, oA, clean, noisy, t), graphs(clean, noisy, t))
    _same(mA, oA, eA, mB, oB, eB, 6)
    assert graphs.captures == 1
    for o in (oA, oB):
        o.param_groups[0]["lr"] *= 0.5
    for k in range(2):
        clean, noisy, t = data[k]
        assert torch.equal(_eager_step(mA, oA, clean, noisy, t), graphs(clean, noisy, t))
    _same(mA, oA, eA, mB, oB, eB, 8)


def test_capture_rolls_the_average_back():
    """After construction and capture, before the first replay: the shadow is the initial
    weights, the counter 0 (the warm-up steps were rolled back); a 'loss' replay leaves the
    average bitwise alone; a swapped average refuses to train."""
    from vub_image_denoising_amd.optim import EMA
    from vub_image_denoising_amd.train_graph import TrainStepGraph
    model = _model()
    initial = {k: v.clone() for k, v in model.state_dict().items()}
    opt = _fused("adamw", model)
    ema = EMA(model, 0.99, warmup=True)
    opt.attach_ema(ema)
    g = TrainStepGraph(model, opt, SHAPE, t_input=True)
    gl = TrainStepGraph(model, opt, SHAPE, t_input=True, kind='loss')
    for k, v in ema.state_dict()["shadow"].items():
        assert torch.equal(v, initial[k]) and torch.equal(model.state_dict()[k], initial[k]), k
    assert ema.num_updates == 0 and int(ema._n_dev) == 0 and opt._step == 0
    clean, noisy, t = _batches(1)[0]
    g(clean, noisy, t)
    assert ema.num_updates == 1 and int(ema._n_dev) == 1
    kept = ema._shadow.clone()
    gl(clean, noisy, t)
    assert torch.equal(ema._shadow, kept) and ema.num_updates == 1 and int(ema._n_dev) == 1
    with ema.applied():
        with pytest.raises(RuntimeError, match="swapped"):
            g(clean, noisy, t)
    assert ema.num_updates == 1 and int(ema._n_dev) == 1


def test_captured_fixed_accumulation_equals_eager():
    """accum x3 + accum_step, twice; the eager loop is run_epochs' fixed mode."""
    from vub_image_denoising_amd import functional as Fn
    from vub_image_denoising_amd.diffusion_RDUnet import train_step_device
    from vub_image_denoising_amd.optim import EMA
    from vub_image_denoising_amd.train_graph import TrainStepGraphs
    data = _batches(8)
    mA, mB = _model(), _model()
    oA, oB = _fused("adamw", mA), _fused("adamw", mB)
    eA, eB = EMA(mA, 0.99, warmup=True), EMA(mB, 0.99, warmup=True)
    oA.attach_ema(eA)
    oB.attach_ema(eB)
    graphs = TrainStepGraphs(mB, oB, t_input=True)
    oA.zero_grad()
    for k, (clean, noisy, t) in enumerate(data):
        last = (k + 1) % 4 == 0
        la = train_step_device(mA, clean, noisy, oA, 'uniform', 1.0, t=t, zero_grad=False, clip=False)
        if last:
            Fn.clip_grad_norm_(mA.parameters(), 1.0)
            oA.step()
            oA.zero_grad()
        before = None if eB._shadow is None else eB._shadow.clone()
        assert torch.equal(la, graphs(clean, noisy, t, kind='accum_step' if last else 'accum'))
        if before is None:                                       # bound by the first capture: still the weights
            assert not last and torch.equal(eB._shadow, eB._fp.flat) and eB.num_updates == 0
        else:
            assert torch.equal(before, eB._shadow) != last       # only the updating batch moves the average
    _same(mA, oA, eA, mB, oB, eB, 2)


def test_captured_bare_rdunet_equals_eager():
    import vub_image_denoising_amd as vm
    from vub_image_denoising_amd.optim import EMA, FusedAdamW
    from vub_image_denoising_amd.RDUNet_model import train_step_device
    from vub_image_denoising_amd.train_graph import TrainStepGraphs
    data = _batches(4)

    def make():
        torch.manual_seed(3)
        m = vm.RDUNet(channels=3, base_filters=16).cuda()
        o = FusedAdamW(m.parameters(), lr=1e-3, weight_decay=1e-4)
        e = EMA(m, 0.99, warmup=True)
        o.attach_ema(e)
        return m, o, e
    mA, oA, eA = make()
    mB, oB, eB = make()
    graphs = TrainStepGraphs(mB, oB, clip_value=1.0)
    oA.zero_grad()
    for k, (clean, noisy, _) in enumerate(data):
        last = (k + 1) % 2 == 0
        la = train_step_device(mA, noisy, clean, oA, 1.0, clip=last)
        if last:
            oA.step()
            oA.zero_grad()
        assert torch.equal(la, graphs(clean, noisy, kind='accum_step' if last else 'accum'))
    _same(mA, oA, eA, mB, oB, eB, 2)
    assert list(eB.state_dict()["shadow"]) == list(mB.state_dict())    # bare names


def test_step_graph_node_counts():
    """Without warm-up the averaged step has the nodes of the plain one (the update is
    inside the optimizer's launch); the warm-up counter costs at most one."""
    from vub_image_denoising_amd.optim import EMA
    from vub_image_denoising_amd.train_graph import TrainStepGraph
    counts = {}
    for name, warmup in (("plain", None), ("ema", False), ("ema_warmup", True)):
        model = _model()
        opt = _fused("adamw", model)
        if warmup is not None:
            opt.attach_ema(EMA(model, 0.99, warmup=warmup))
        counts[name] = TrainStepGraph(model, opt, SHAPE, t_input=True).graph_nodes
    print("step graph nodes", counts)
    if counts["plain"] is None:      # train_graph._node_count: not exposed by this build
        return
    assert counts["ema"] == counts["plain"]
    assert counts["plain"] <= counts["ema_warmup"] <= counts["plain"] + 1


# ----------------------------------------------------------------- using the average
def test_applied_average_samples_like_a_model_loaded_from_it():
    from vub_image_denoising_amd.optim import EMA
    from vub_image_denoising_amd.sampling import SamplerGraph
    data = _batches(3)
    model = _model()
    opt = _fused("adamw", model, lr=1e-2)
    ema = EMA(model, 0.9)
    opt.attach_ema(ema)
    for clean, noisy, t in data:
        _eager_step(model, opt, clean, noisy, t)
    model.eval()
    x = data[0][1]
    with torch.no_grad():
        sg = SamplerGraph(model, SHAPE)               # captured before the swap
        raw = model.improved_sampling(x).clone()
        assert torch.equal(sg(x), raw)
        fresh = _model(seed=9)
        fresh.load_state_dict(ema.state_dict()["shadow"])
        want = fresh.eval().improved_sampling(x).clone()
        assert not torch.equal(want, raw)
        flat, shadow = ema._fp.flat.clone(), ema._shadow.clone()
        ptrs = (ema._fp.flat.data_ptr(), ema._shadow.data_ptr())
        with ema.applied():
            assert ema.swapped and torch.equal(ema._fp.flat, shadow) and torch.equal(ema._shadow, flat)
            assert torch.equal(model.improved_sampling(x), want)
            assert torch.equal(sg(x), want)
            for k, v in ema.state_dict()["shadow"].items():     # still the average while swapped
                assert torch.equal(v, fresh.state_dict()[k]), k
            with pytest.raises(RuntimeError, match="swapped"):
                opt.step()
            with pytest.raises(RuntimeError, match="swapped"):
                ema.update()
        assert not ema.swapped and (ema._fp.flat.data_ptr(), ema._shadow.data_ptr()) == ptrs
        assert torch.equal(ema._fp.flat, flat) and torch.equal(ema._shadow, shadow)
        assert torch.equal(model.improved_sampling(x), raw)
        assert torch.equal(sg(x), raw)
    assert ema.num_updates == 3


# ----------------------------------------------------------------- trainers and checkpoints
class _Writer:
    def __init__(self):
        self.scalars = {}

    def add_scalar(self, tag, v, step):
        self.scalars.setdefault(tag, {})[step] = float(v)


class _Epochs(list):
    """Four tiny batches; every pass reseeds torch with the epoch's number, so a resumed
    run draws the timesteps of the uninterrupted one."""
    epoch = 0

    def __iter__(self):
        torch.manual_seed(1000 + self.epoch)
        self.epoch += 1
        return super().__iter__()


def _train(tmp, optname, captured, epochs, ema_decay=0.9, resume=None):
    from vub_image_denoising_amd.diffusion_RDUnet import load_checkpoint, run_epochs
    from vub_image_denoising_amd.optim import EMA, FusedAdamW
    model = _model(seed=2)
    if optname == "torch":
        opt = torch.optim.AdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    else:
        opt = FusedAdamW(model.parameters(), lr=1e-3, weight_decay=1e-4)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    ema = EMA(model, ema_decay, warmup=True) if ema_decay else None
    data = _Epochs((n.cpu(), c.cpu()) for c, n, _ in _batches(4))
    start = 0
    if resume is not None:
        start = load_checkpoint(model, opt, sched, resume, ema=ema)
        data.epoch = start
    w = _Writer()
    val = [(n.cpu(), c.cpu()) for c, n, _ in _batches(1, seed=5)]
    run_epochs(model, data, val, opt, sched, w, str(tmp), 'uniform', epochs, start, 2, 1.0, 1,
               sample=lambda m, x: m.improved_sampling(x), captured=captured, ema=ema)
    return model, opt, ema, w


CKPT = "diffusion_RDUNet_model_checkpointed_epoch_{}.pth"


@pytest.mark.parametrize("optname,captured", [("torch", False), ("fused", False), ("fused", True)])
def test_checkpoint_resume_continues_bit_for_bit(optname, captured, tmp_path):
    from vub_image_denoising_amd import denoise_image
    from vub_image_denoising_amd.diffusion_RDUnet import load_checkpoint
    from vub_image_denoising_amd.optim import EMA
    mU, oU, eU, wU = _train(tmp_path / "whole", optname, captured, 2)
    _train(tmp_path / "part", optname, captured, 1)
    mR, _, eR, wR = _train(tmp_path / "part", optname, captured, 2, resume=str(tmp_path / "part" / CKPT.format(1)))
    for (n, a), b in zip(mU.named_parameters(), mR.parameters()):
        assert torch.equal(a, b), n
    assert torch.equal(eU._shadow, eR._shadow) and not torch.equal(eU._shadow, eU._fp.flat)
    assert eU.num_updates == eR.num_updates == int(eU._n_dev) == int(eR._n_dev) == 4
    assert set(wU.scalars) == {"Loss/train", "Loss/validation", "Loss/validation_ema"}
    assert wU.scalars["Loss/validation_ema"][2] == wR.scalars["Loss/validation_ema"][2]
    assert wU.scalars["Loss/validation_ema"] != wU.scalars["Loss/validation"]
    # the checkpoint: the EMA key, weights-only loadable, the averaged weights usable as they are
    path = str(tmp_path / "whole" / CKPT.format(2))
    ck = torch.load(path, map_location="cuda", weights_only=True)
    assert set(ck) == {"epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict", "ema_state_dict"}
    assert ck["ema_state_dict"]["num_updates"] == 4 and ck["ema_state_dict"]["warmup"] is True
    for k, v in eU.state_dict()["shadow"].items():
        assert torch.equal(ck["ema_state_dict"]["shadow"][k], v), k
    loaded = denoise_image.load_model(path, base_filters=16, timesteps=4, weights="ema")
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, ck["ema_state_dict"]["shadow"][k]), k
    if optname == "torch":
        return
    # without an EMA: the same training, the same validation loss, today's four checkpoint keys
    mP, _, _, wP = _train(tmp_path / "plain", optname, captured, 2, ema_decay=0.0)
    for (n, a), b in zip(mU.named_parameters(), mP.parameters()):
        assert torch.equal(a, b), n
    assert wP.scalars["Loss/validation"] == wU.scalars["Loss/validation"]
    assert set(wP.scalars) == {"Loss/train", "Loss/validation"}
    plain = str(tmp_path / "plain" / CKPT.format(2))
    assert set(torch.load(plain, map_location="cuda", weights_only=True)) == {
        "epoch", "model_state_dict", "optimizer_state_dict", "scheduler_state_dict"}
    with pytest.raises(KeyError, match="no EMA weights"):
        denoise_image.load_model(plain, base_filters=16, timesteps=4, weights="ema")
    # an EMA wanted from that checkpoint, on a bound EMA: restarted from the loaded weights, in place
    ptr = eU._shadow.data_ptr()
    assert load_checkpoint(mU, oU, None, plain, ema=eU) == 2
    assert eU.num_updates == 0 and int(eU._n_dev) == 0 and eU._shadow.data_ptr() == ptr
    assert torch.equal(eU._shadow, eU._fp.flat)
    assert isinstance(eU, EMA)
