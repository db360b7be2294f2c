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
addresses a capture bakes in), ``use_device_step()``, ``set_step()`` and
``_replayed()``.
"""
from __future__ import annotations

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

    def reset_state(self):
        """Forget the state and the step count, in place (the flat state buffers
        and device step counter keep their addresses, so a TrainStepGraph captured
        over them replays from a fresh optimizer: re-initialised training runs)."""
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

    def graph_buffers(self):
        """The flat state buffers a step writes (bound optimizers only)."""
        return list(self._bufs)

    def graph_key(self):
        """What a captured step bakes in: the group's hyperparameters, the gradient
        scale and the addresses of the buffers the update touches."""
        g = self.param_groups[0]
        hyper = tuple((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in sorted(g.items())
                      if k != "params" and isinstance(v, (int, float, bool, list, tuple, type(None))))
        bufs = (self._bufs or []) + [self._step_dev, None if self._fp is None else self._fp.flat]
        return hyper, float(self.grad_scale), tuple(0 if b is None else b.data_ptr() for b in bufs)

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
        H.check(lib.rdn_adam_step(fp.flat.data_ptr(), fp.gflat.data_ptr(), m.data_ptr(), v.data_ptr(),
                                  fp.numel, float(g["lr"]), float(b1), float(b2), float(g["eps"]),
                                  float(g["weight_decay"]), 1 if self.decoupled else 0, self._step, sd,
                                  float(self.grad_scale), st), "adam_step")


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
        H.check(lib.rdn_adadelta_step(fp.flat.data_ptr(), fp.gflat.data_ptr(), sq.data_ptr(), acc.data_ptr(),
                                      fp.numel, float(g["lr"]), float(g["rho"]), float(g["eps"]),
                                      float(g["weight_decay"]), float(self.grad_scale), st), "adadelta_step")
