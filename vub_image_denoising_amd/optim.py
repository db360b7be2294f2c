"""Fused optimizers over the flat parameter buffer: one ``rdn_adam_step`` /
``rdn_adadelta_step`` launch per step instead of torch's per-tensor (foreach) kernels.

Same updates as ``torch.optim.Adam`` / ``AdamW`` / ``Adadelta`` (the optimizers of
diffusion_RDUnet.py:264-276 and main_diffusion_RDUnet.py:230), same
``param_groups`` (so LR schedulers work) and a ``state_dict`` in torch's
per-parameter format (``step`` plus ``exp_avg``, ``exp_avg_sq`` or ``square_avg``,
``acc_delta``), whose state tensors are views of flat state buffers.
``load_state_dict`` restores the state and the step count into those buffers, so a
resumed run continues bit-identically (diffusion_RDUnet.py:180-193 resume path).

What ``train_graph.TrainStepGraph`` needs from a fused optimizer is the surface
of ``FusedFlatOptimizer``: ``graph_buffers()`` (the flat state to snapshot and
restore around warm-up steps), ``graph_key()`` (the hyperparameters and buffer
addresses a capture bakes in), ``use_device_step()`` (which also binds),
``host_counts()`` / ``set_host_counts()`` (the step count and an attached EMA's update
count, which warm-up steps and the capture advance and must give back),
``check_ema_not_swapped()`` and ``_replayed()``.

``EMA`` (no reference counterpart) keeps an exponential moving average of the weights
in one more flat buffer.  Attached to a fused optimizer (``attach_ema``) it is updated
inside the optimizer's launch (``rdn_adam_step_ema`` / ``rdn_adadelta_step_ema``) and
its buffer and update counter join the optimizer's graph surface; beside a
``torch.optim`` optimizer ``EMA.update()`` is one ``rdn_ema_update`` launch.
"""
from __future__ import annotations

import contextlib

import torch

from . import _hip as H
from .engine import find_flat


class FusedFlatOptimizer(torch.optim.Optimizer):
    """One parameter group bound lazily to a network's FlatParams, ``len(STATE_KEYS)``
    flat fp32 state buffers of its layout, and a step count (host mirror, the
    ``step`` tensor of the state dict and, for updates that read it, a device
    counter).  Subclasses set ``STATE_KEYS`` / ``NEEDS_DEVICE_STEP`` and write ``_update``."""

    STATE_KEYS: tuple = ()
    NEEDS_DEVICE_STEP = False   # the update kernel reads the step count (replayed graphs: from device memory)

    def __init__(self, params, defaults, grad_scale=1.0):
        super().__init__(params, defaults)
        if len(self.param_groups) != 1:
            raise ValueError(f"{type(self).__name__} works on one parameter group (the fused network's flat buffer)")
        self.grad_scale = grad_scale
        self._fp = None
        self._bufs = None       # flat state buffers, in STATE_KEYS order
        self._step = 0
        self._step_dev = None   # device step counter (use_device_step)
        self.ema = None         # EMA updated inside the update launch (attach_ema)

    def attach_ema(self, ema):
        """Keep ``ema`` (an ``EMA`` over this optimizer's parameters) inside the update
        launch: every ``step()`` -- eager or replayed in a captured graph -- also updates
        the average, with no launch of its own.  ``None`` detaches."""
        if ema is not None:
            mine = self.param_groups[0]["params"]
            if len(ema.params) != len(mine) or any(a is not b for a, b in zip(ema.params, mine)):
                raise ValueError("attach_ema: the EMA must average exactly this optimizer's parameters, in order")
            if self._fp is not None:
                ema._bind_to(self._fp)
        self.ema = ema
        return self

    def _bind(self):
        params = self.param_groups[0]["params"]
        fp = find_flat(params)
        if fp is None:
            raise RuntimeError(f"{type(self).__name__} needs the parameters of one GPU RDUNet (run a forward/backward "
                               "first); use the torch.optim class otherwise")
        if self._fp is not fp:
            # state already in self.state (a load_state_dict before the first step,
            # or a previous flat buffer) is carried over into the new flat buffers
            self._fp = fp
            self._bufs = [torch.zeros_like(fp.flat) for _ in self.STATE_KEYS]
            self._steps = torch.zeros((), dtype=torch.float32)
            self._load_state()
        if self.ema is not None:
            self.ema._bind_to(fp)
        return fp

    def _load_state(self):
        """Copy the state / step count held in ``self.state`` (torch's per-parameter
        format) INTO the existing flat buffers and device step counter, then make the
        state entries views of them again.  In place, so a TrainStepGraph captured
        over these buffers keeps replaying on the loaded state."""
        fp = self._fp
        old = {p: self.state[p] for p in fp.params if p in self.state}
        steps = set()
        for b in self._bufs:
            b.zero_()
        first = self.STATE_KEYS[0]
        for p, off in zip(fp.params, fp.offsets):
            n = p.numel()
            st = old.get(p)
            if st and first in st:
                for b, key in zip(self._bufs, self.STATE_KEYS):
                    b[off:off + n].copy_(st[key].reshape(-1))
                steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise RuntimeError(f"{type(self).__name__}: parameters were saved at different step counts {sorted(steps)}")
        self.set_step(steps.pop() if steps else 0)
        self._views()

    def set_step(self, step, device=True):
        """Set the step count everywhere it is kept: host, state dict and (``device``)
        the device counter."""
        self._step = int(step)
        self._steps.fill_(self._step)
        if device and self._step_dev is not None:
            if self._step_dev.device == self._fp.device:
                self._step_dev.fill_(self._step)
            else:
                self._step_dev = torch.full((), self._step, dtype=torch.int64, device=self._fp.device)

    def host_counts(self):
        """The host counts a step advances: the step count and an attached EMA's update count (else None)."""
        return self._step, None if self.ema is None else self.ema.num_updates

    def set_host_counts(self, counts, device=True):
        """Roll the counts back to an earlier ``host_counts()``; ``device`` as in ``set_step``
        (an EMA's device counter is one of ``graph_buffers()`` and is restored with them)."""
        self.set_step(counts[0], device)
        if self.ema is not None:
            self.ema.num_updates = counts[1]

    def check_ema_not_swapped(self, who):
        """An update now would train the averaged weights: refuse inside ``EMA.applied()``."""
        if self.ema is not None and self.ema.swapped:
            raise RuntimeError(f"{who}: the attached EMA is swapped into the weights (inside EMA.applied()); "
                               "swap back first")

    def reset_state(self):
        """Forget the state and the step count, in place (the flat state buffers
        and device step counter keep their addresses, so a TrainStepGraph captured
        over them replays from a fresh optimizer: re-initialised training runs).
        An attached EMA is left alone: the average is not optimizer state."""
        self.state.clear()
        if self._fp is not None:
            self._load_state()
        else:
            self._step = 0

    def use_device_step(self):
        """Make the step replayable in a hipGraph (train_graph.TrainStepGraph): where
        the update reads the step count, keep it in device memory, incremented and
        read by the update kernels, so a captured step stays exact on every replay;
        the host count mirrors it."""
        fp = self._bind()
        if self.NEEDS_DEVICE_STEP and self._step_dev is None:
            self._step_dev = torch.full((), self._step, dtype=torch.int64, device=fp.device)
        return self

    def _replayed(self):
        """A captured step ran (host mirror of the step count)."""
        self._step += 1
        self._steps.fill_(self._step)
        self._fp.generation += 1
        if self.ema is not None:
            self.ema.num_updates += 1

    def graph_buffers(self):
        """The flat state buffers a step writes (bound optimizers only), an attached
        EMA's shadow and device counter included."""
        return list(self._bufs) + ([] if self.ema is None else self.ema.graph_buffers())

    def graph_key(self):
        """What a captured step bakes in: the group's hyperparameters, the gradient
        scale and the addresses of the buffers the update touches."""
        g = self.param_groups[0]
        hyper = tuple((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in sorted(g.items())
                      if k != "params" and isinstance(v, (int, float, bool, list, tuple, type(None))))
        bufs = (self._bufs or []) + [self._step_dev, None if self._fp is None else self._fp.flat]
        key = hyper, float(self.grad_scale), tuple(0 if b is None else b.data_ptr() for b in bufs)
        return key if self.ema is None else key + (self.ema.graph_key(),)

    def _views(self):
        fp = self._fp
        for p, off in zip(fp.params, fp.offsets):
            n = p.numel()
            st = {"step": self._steps}
            for b, key in zip(self._bufs, self.STATE_KEYS):
                st[key] = b[off:off + n].view_as(p)
            self.state[p] = st

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        if self._fp is None:
            return                        # state is taken over at the first bind
        fp = find_flat(self.param_groups[0]["params"])
        if fp is self._fp or fp is None:
            # same flat buffers (the usual resume): loaded into the existing state
            # buffers and step counter, whose addresses a captured graph holds
            self._load_state()
        else:
            self._fp = None
            self._bind()

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        self.check_ema_not_swapped(f"{type(self).__name__}.step()")
        fp = self._bind()
        self._step += 1
        self._steps.fill_(self._step)
        self._update(fp, self.param_groups[0], H.lib(), H.stream_ptr())
        fp.generation += 1  # weights changed behind torch's version counters: repack
        return loss

    def zero_grad(self, set_to_none: bool = True):
        fp = find_flat(self.param_groups[0]["params"])
        if fp is not None and not set_to_none:
            fp.gflat.zero_()
            return
        super().zero_grad(set_to_none=set_to_none)


class FusedAdam(FusedFlatOptimizer):
    STATE_KEYS = ("exp_avg", "exp_avg_sq")
    NEEDS_DEVICE_STEP = True

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False,
                 grad_scale=1.0):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay), grad_scale)
        self.decoupled = decoupled

    def _update(self, fp, g, lib, st):
        b1, b2 = g["betas"]
        m, v = self._bufs
        sd = None
        if self._step_dev is not None:
            H.check(lib.rdn_counter_inc(self._step_dev.data_ptr(), st), "counter_inc")
            sd = self._step_dev.data_ptr()
        args = (fp.flat.data_ptr(), fp.gflat.data_ptr(), m.data_ptr(), v.data_ptr(), fp.numel, float(g["lr"]),
                float(b1), float(b2), float(g["eps"]), float(g["weight_decay"]), 1 if self.decoupled else 0,
                self._step, sd, float(self.grad_scale))
        if self.ema is None:
            H.check(lib.rdn_adam_step(*args, st), "adam_step")
        else:
            H.check(lib.rdn_adam_step_ema(*args, *self.ema._kernel_args(), st), "adam_step_ema")
            self.ema._advance(lib, st)


class FusedAdamW(FusedAdam):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, grad_scale=1.0):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, decoupled=True,
                         grad_scale=grad_scale)


class FusedAdadelta(FusedFlatOptimizer):
    """``torch.optim.Adadelta`` (``--optimizer_choice adadelta``, diffusion_RDUnet.py:270-272)
    as one ``rdn_adadelta_step`` launch.  The update reads no step count, so the
    launch replays in a captured graph as it is."""
    STATE_KEYS = ("square_avg", "acc_delta")

    def __init__(self, params, lr=1.0, rho=0.9, eps=1e-6, weight_decay=0, grad_scale=1.0):
        super().__init__(params, dict(lr=lr, rho=rho, eps=eps, weight_decay=weight_decay), grad_scale)

    def _update(self, fp, g, lib, st):
        sq, acc = self._bufs
        args = (fp.flat.data_ptr(), fp.gflat.data_ptr(), sq.data_ptr(), acc.data_ptr(), fp.numel, float(g["lr"]),
                float(g["rho"]), float(g["eps"]), float(g["weight_decay"]), float(self.grad_scale))
        if self.ema is None:
            H.check(lib.rdn_adadelta_step(*args, st), "adadelta_step")
        else:
            H.check(lib.rdn_adadelta_step_ema(*args, *self.ema._kernel_args(), st), "adadelta_step_ema")
            self.ema._advance(lib, st)


def ema_decay_at(decay, warmup, n):
    """The decay of the update after ``n`` earlier ones: ``decay``, or with warm-up
    ``min(decay, (1 + n) / (10 + n))`` (0.1 for the first update, rising to the cap).
    In double, the expression the kernels evaluate (csrc/optim.hip, ema_weight)."""
    return min(float(decay), (1.0 + n) / (10.0 + n)) if warmup else float(decay)


def shadow_names(model, params):
    """The names under which ``model.state_dict()`` saves ``params`` (matched by identity):
    ``unet.``-prefixed for a DiffusionModel, bare for an RDUNet."""
    by_id = {id(p): n for n, p in model.named_parameters()}
    try:
        return [by_id[id(p)] for p in params]
    except KeyError:
        raise ValueError("EMA: the model does not own every averaged parameter") from None


class EMA:
    """Exponential moving average of a fused network's weights (no reference counterpart):
    ``e += w * (p - e)``, ``w = 1 - ema_decay_at(decay, warmup, num_updates)``, one flat
    fp32 shadow buffer in the layout of the network's flat parameter buffer.

    ``params``: the network's parameters, or the model itself (a DiffusionModel or an
    RDUNet), which also fixes the names ``state_dict()['shadow']`` uses to the model's
    own (``use_names_of``; the trainers call it).  Binds lazily to the network's
    FlatParams, like the fused optimizers; the shadow starts as a copy of the weights at
    bind time (``bind()`` before the first optimizer step).  With ``warmup`` the update
    count also lives in a device int64 the kernels read, so a captured step stays exact
    on every replay."""

    def __init__(self, params, decay, warmup=False):
        model = params if isinstance(params, torch.nn.Module) else None
        self.params = list(model.parameters() if model is not None else params)
        if not 0.0 <= float(decay) <= 1.0:
            raise ValueError(f"EMA: decay must be in [0, 1], got {decay}")
        self.decay, self.warmup = float(decay), bool(warmup)
        self.num_updates = 0
        self.swapped = False
        self._names = None
        self._fp = None
        self._shadow = None
        self._n_dev = None
        self._pending = None    # a shadow loaded before the first bind
        if model is not None:
            self.use_names_of(model)

    def use_names_of(self, model):
        self._names = shadow_names(model, self.params)
        return self

    # ------------------------------------------------------------------ binding
    def bind(self):
        fp = self._fp
        if fp is not None and fp.intact():
            return fp
        if self.swapped:
            raise RuntimeError("EMA: the network's flat parameters were rebuilt while the average was swapped in")
        fp = find_flat(self.params, need_grads=False)
        if fp is None:
            raise RuntimeError("EMA needs the parameters of one GPU RDUNet that has run (a forward builds its flat "
                               "parameter buffer)")
        return self._bind_to(fp)

    def _bind_to(self, fp):
        if self._fp is fp:
            return fp
        if len(fp.params) != len(self.params) or any(a is not b for a, b in zip(fp.params, self.params)):
            raise ValueError("EMA: bound to the flat parameters of another network")
        old = self._shadow
        self._fp = fp
        if old is not None and old.numel() == fp.numel:    # the network was re-flattened: the average moves along
            self._shadow = old.to(fp.device, copy=True)
        else:
            self._shadow = fp.flat.clone()
        self._n_dev = None
        self._set_count(self.num_updates)
        if self._pending is not None:
            pending, self._pending = self._pending, None
            self._load_shadow(pending)
        return fp

    def _set_count(self, n, device=True):
        self.num_updates = int(n)
        if not (device and self._fp is not None):
            return
        if not self.warmup:
            self._n_dev = None
        elif self._n_dev is None:
            self._n_dev = torch.full((), self.num_updates, dtype=torch.int64, device=self._fp.device)
        else:
            self._n_dev.fill_(self.num_updates)

    def _name_list(self):
        return self._names if self._names is not None else (None if self._fp is None else self._fp.names)

    # ------------------------------------------------------------------ update
    def _kernel_args(self):
        return (self._shadow.data_ptr(), self.decay, 1 if self.warmup else 0, self.num_updates, H.ptr(self._n_dev))

    def _advance(self, lib, st):
        """Behind an update launch: the device counter (stream-ordered) and its host mirror."""
        if self._n_dev is not None:
            H.check(lib.rdn_counter_inc(self._n_dev.data_ptr(), st), "counter_inc")
        self.num_updates += 1

    @torch.no_grad()
    def update(self):
        """The stand-alone launch (beside an optimizer that is not fused)."""
        if self.swapped:
            raise RuntimeError("EMA.update(): the average is swapped into the weights (inside applied()); "
                               "swap back first")
        fp = self.bind()
        lib, st = H.lib(), H.stream_ptr()
        shadow, *rest = self._kernel_args()
        H.check(lib.rdn_ema_update(shadow, fp.flat.data_ptr(), fp.numel, *rest, st), "ema_update")
        self._advance(lib, st)

    def graph_buffers(self):
        return [] if self._shadow is None else [self._shadow] + ([] if self._n_dev is None else [self._n_dev])

    def graph_key(self):
        return self.decay, self.warmup, 0 if self._shadow is None else self._shadow.data_ptr(), H.ptr(self._n_dev) or 0

    # ------------------------------------------------------------------ using the average
    @torch.no_grad()
    def swap(self):
        """Exchange the weights and the average in place (no address moves; weight packs
        and captured samplers pick the change up through ``packs.refresh()``)."""
        fp = self.bind()
        tmp = fp.flat.clone()
        fp.flat.copy_(self._shadow)
        self._shadow.copy_(tmp)
        self.swapped = not self.swapped
        fp.generation += 1

    @contextlib.contextmanager
    def applied(self):
        """The network computes with the averaged weights inside the block."""
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def reset_to_weights(self):
        """Restart the average from the current weights, count 0 (in place)."""
        if self.swapped:
            raise RuntimeError("EMA.reset_to_weights(): swapped")
        self._pending = None
        if self._fp is not None:
            self._shadow.copy_(self._fp.flat)
        self._set_count(0)

    # ------------------------------------------------------------------ state
    def _shadow_dict(self):
        if self._fp is None:
            try:
                self.bind()
            except RuntimeError:
                pass
        names = self._name_list()
        if self._fp is None:
            if self._pending is not None:
                return dict(self._pending)
            if names is None:
                raise RuntimeError("EMA.state_dict(): not bound and built from bare parameters (no names yet)")
            return {n: p.detach().clone() for n, p in zip(names, self.params)}   # the average starts as the weights
        fp = self._fp
        src = fp.flat if self.swapped else self._shadow
        return {n: src[off:off + p.numel()].view_as(p) for n, p, off in zip(names, fp.params, fp.offsets)}

    def state_dict(self):
        """Tensors and plain numbers only (loads under ``weights_only=True``).  ``shadow``
        maps the model's own parameter names to views of the flat average:
        ``model.load_state_dict(ema.state_dict()['shadow'])`` loads the averaged weights."""
        return {'decay': self.decay, 'warmup': self.warmup, 'num_updates': self.num_updates,
                'shadow': self._shadow_dict()}

    @torch.no_grad()
    def _load_shadow(self, shadow):
        names = self._name_list()
        if set(shadow) != set(names):
            odd = sorted(set(shadow) ^ set(names))
            raise KeyError(f"EMA.load_state_dict: shadow names do not match the model's ({odd[:4]} ...)")
        fp = self._fp
        for n, p, off in zip(names, fp.params, fp.offsets):
            self._shadow[off:off + p.numel()].view_as(p).copy_(shadow[n])

    def load_state_dict(self, sd):
        """Into the existing buffers (a captured graph keeps replaying on them); before the
        first bind the shadow is held until then."""
        if self.swapped:
            raise RuntimeError("EMA.load_state_dict(): the average is swapped into the weights")
        self.decay, warm = float(sd['decay']), bool(sd['warmup'])
        if warm != self.warmup:
            self.warmup, self._n_dev = warm, None
        self._set_count(int(sd['num_updates']))
        if self._fp is None:
            self._pending = {k: v.detach().clone() for k, v in sd['shadow'].items()}
        else:
            self._load_shadow(sd['shadow'])
