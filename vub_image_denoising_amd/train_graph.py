"""hipGraph capture of one whole train step: the t draw, the interpolation, the
fused RDUNet_T forward, the Charbonnier loss, the backward, clip_grad_norm_ and
the fused Adam(W) update (diffusion_RDUnet.py:76-115 + ``optimizer.step()``),
replayed with ONE host launch per step instead of ~700 kernel launches issued
from Python.

What makes the step capturable:

* every buffer the step touches exists before capture (engine activations and
  launch descriptors, the flat gradient buffer, clip and Adam workspaces):
  warm-up steps build them, then their effect on the weights, the Adam moments,
  the step count and the RNG is rolled back, so the first replay IS the model's
  next step;
* the Adam step count lives in device memory (FusedAdam.use_device_step), so
  bias corrections advance on every replay;
* an EMA attached to the optimizer (optim.EMA, FusedFlatOptimizer.attach_ema) is
  updated by the optimizer's own launch: its shadow buffer and, with warm-up, its
  device update counter are part of ``graph_buffers()`` (rolled back over the warm-up
  steps like the moments) and of ``graph_key()``; only ``step`` / ``accum_step``
  replays touch it;
* ``torch.randint`` t draws use torch's graph-safe Philox generator (every
  replay advances its offset exactly as an eager step does); the 'biased'
  distribution draws on the CPU in the reference (:71-73), so its t are drawn
  on the host per call and copied into the graph's t input;
* values baked into the graph — lr, betas, eps, weight decay, clip value,
  compute dtype — are compared on every call; a change (an LR scheduler step)
  re-captures.

The graph owns the parameters' ``.grad`` (views of the flat gradient buffer its
backward writes); an eager step in between is allowed and does not disturb it.

Besides the full step (``kind='step'``) a graph can capture the other batches the
trainers issue (trainer.train_epochs): ``'loss'`` (the t draw, forward and
loss of a batch whose gradient the reference discards, forward_step_device),
``'accum'`` (t draw, forward, loss, backward, the gradient added into the model's
flat accumulator) and ``'accum_step'`` (the same, then clip and update on the
accumulated gradient and the accumulator cleared): the fixed accumulation mode.
The accumulator is one flat fp32 buffer of the gradient layout per model
(``grad_accumulator``), shared by the graphs of every shape; each backward writes
its own flat buffer and ONE flat ``add_`` folds it in (eager accumulation is 207
per-tensor adds of the same elements: the same bits).  After an accumulate replay the
parameters' ``.grad`` are views of the accumulator, as after eager accumulation.

What a batch is comes from the model's *task* (``trainer``'s module docstring;
``model.train_task(distribution_choice, loss_weights)`` unless one is passed): a
DiffusionModel's is the step described above, a bare ``RDUNet``'s (the plain baseline)
``L1(model(noisy), clean)`` with no t and no loss weights, in the same four kinds.
"""
from __future__ import annotations

import os

import torch

from .engine import find_flat
from .functional import clip_grad_norm_

KINDS = ("step", "loss", "accum", "accum_step")
_FUSED_SURFACE = ("graph_buffers", "graph_key", "use_device_step", "host_counts", "set_host_counts",
                  "check_ema_not_swapped", "_replayed")


def is_fused(optimizer) -> bool:
    """The optimizer has what a captured step needs (optim.FusedFlatOptimizer's surface)."""
    return all(hasattr(optimizer, a) for a in _FUSED_SURFACE)


def grad_accumulator(fp):
    """The model's flat gradient accumulator (created on first use) and its
    per-parameter views.  It is a member of the gradient buffer pool, so ``.grad``
    tensors that are its views count as flat (clip and the fused update run on it as
    single launches); the views held here keep a backward from taking it as scratch."""
    acc = getattr(fp, "_accum", None)
    if acc is None:
        acc = fp._accum = torch.zeros(fp.numel, dtype=torch.float32, device=fp.device)
        fp._gpool.append(acc)
        fp._accum_views = fp.grad_views(acc)
    return acc, fp._accum_views


def clear_accumulator(network):
    """Discard a partial accumulation group of the fused ``network`` (the trainers'
    ``optimizer.zero_grad()`` at the start of an epoch)."""
    fp = getattr(network, "_rdn_flat", None)
    if fp is not None and getattr(fp, "_accum", None) is not None:
        fp._accum.zero_()


class GraphCaptureUnsafe(RuntimeError):
    """Capturing the data-parallel step is not safe on this torch build."""


def _drain_collectives(fp) -> None:
    """Before a capture: wait until ProcessGroupNCCL's watchdog has retired every
    eager collective (the warm-up steps' all-reduces).  Its loop queries each
    pending work's end event, recorded on the group's RCCL stream; once that stream
    is pulled into the capture, HIP refuses the query (hipErrorCapturedEvent) and the
    watchdog aborts the process -- seen in the world-1 graph test on MI355X, round 4,
    whenever the capture began before the watchdog's next sweep."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return
    sync = getattr(fp, "grad_sync", None) if fp is not None else None
    groups = [dist.group.WORLD] + ([sync.group] if sync is not None and sync.group is not None else [])
    for pg in groups:
        try:
            if dist.get_backend(pg) != "nccl":
                continue
        except (RuntimeError, ValueError):
            continue
        if os.environ.get("TORCH_NCCL_CUDA_EVENT_CACHE") != "0":
            # with the event cache on, an eager collective's cached event can be re-recorded
            # inside the capture and the watchdog's query of it aborts the process (ddp.capture_safe_env)
            raise GraphCaptureUnsafe("capturing an RCCL train step needs TORCH_NCCL_CUDA_EVENT_CACHE=0 set before "
                                     "init_process_group (call ddp.capture_safe_env() first)")
        wait = getattr(pg, "_wait_for_pending_works", None)
        if wait is None:   # (a private ProcessGroupNCCL method; a build without it cannot capture safely)
            raise GraphCaptureUnsafe(
                "torch.distributed's NCCL process group has no _wait_for_pending_works(): the watchdog may query "
                "a captured event and abort the process, so the RCCL train step is not captured (run eagerly)")
        wait()


def _node_count(g):
    """Kernel/memset/copy nodes of a captured graph (None if not exposed)."""
    try:
        import ctypes
        hip = ctypes.CDLL("libamdhip64.so")
        raw = g.raw_cuda_graph()
        n = ctypes.c_size_t(0)
        if hip.hipGraphGetNodes(ctypes.c_void_p(raw), None, ctypes.byref(n)) != 0:
            return None
        return n.value
    except Exception:
        return None


class TrainStepGraph:
    def __init__(self, model, optimizer, shape, distribution_choice='uniform', clip_value=1.0, t_input=False,
                 warmup=2, loss_weights=None, kind='step', *, task=None):
        if not is_fused(optimizer):
            raise TypeError("TrainStepGraph needs a fused optimizer (optim.FusedAdam / FusedAdamW / FusedAdadelta)")
        if kind not in KINDS:
            raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
        self.task = task = task or model.train_task(distribution_choice, loss_weights)
        if t_input and not task.takes_t:
            raise ValueError(f"the step of a {type(model).__name__} has no t input")
        self.net = task.network
        sync = getattr(getattr(self.net, "_rdn_flat", None), "grad_sync", None)
        if kind != 'step' and sync is not None and sync.world > 1:
            raise NotImplementedError(f"data-parallel capture of kind {kind!r} is not implemented (only 'step')")
        self.kind = kind
        self.model, self.opt = model, optimizer
        self.clip = clip_value
        dev = next(model.parameters()).device
        self.dev = dev
        self.clean = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.noisy = torch.zeros(shape, dtype=torch.float32, device=dev)
        self.t = torch.zeros(shape[0], dtype=torch.float32, device=dev) if (t_input or task.host_t) else None
        self.graph = None
        self._build(warmup)

    # ------------------------------------------------------------------
    def _hyper(self):
        """Everything baked into the captured graph: hyperparameters, the task's own
        (the loss and its weights), the compute dtype, and the addresses of the buffers
        the optimizer updates (a rebound optimizer or a re-flattened model re-captures
        instead of replaying onto freed memory)."""
        return self.opt.graph_key(), float(self.clip), self.net.compute_dtype, self.task.graph_key

    def _backward(self, clip=True):
        """Backward of this batch alone (gradients zeroed first), clipped or not."""
        return self.task.train_batch(self.clean, self.noisy, self.opt, self.clip, zero_grad=True, clip=clip, t=self.t)

    def _body(self):
        if self.kind == 'loss':
            return self.task.loss_batch(self.clean, self.noisy, need_loss=True, t=self.t)
        if self.kind == 'step':
            loss = self._backward()
            self.opt.step()
            return loss
        # 'accum' / 'accum_step': this backward's gradient lands in a flat buffer of its
        # own (the parameters' .grad are dropped first), one flat add folds it into the
        # accumulator, and .grad become the accumulator's views, which clip and the
        # update then see as the flat gradient
        loss = self._backward(clip=False)
        params = list(self.model.parameters())
        fp = find_flat(params)
        if fp is None:
            raise RuntimeError("TrainStepGraph: the backward did not leave flat gradient views")
        acc, views = grad_accumulator(fp)
        acc.add_(fp.gflat)
        for p, v in zip(fp.params, views):
            p.grad = v
        if self.kind == 'accum_step':
            clip_grad_norm_(params, self.clip, want_norm=False)
            self.opt.step()
            acc.zero_()
        return loss

    def _build(self, warmup):
        rng = torch.cuda.get_rng_state(self.dev)
        params, opt = list(self.model.parameters()), self.opt
        side = torch.cuda.Stream(device=self.dev)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            if find_flat(params) is None:
                # gradients as flat views, so the optimizer can bind (no update yet)
                self._backward()
            opt.use_device_step()    # (binds the optimizer to the flat parameters)
            fp = find_flat(params)
            state = [fp.flat] + opt.graph_buffers()
            if self.kind in ('accum', 'accum_step'):
                state.append(grad_accumulator(fp)[0])   # may hold a partial group: kept
            snap = [b.clone() for b in state]
            counts = opt.host_counts()
            for _ in range(max(1, warmup)):
                self._body()
            for b, s in zip(state, snap):
                b.copy_(s)
            opt.set_host_counts(counts)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize(self.dev)
        _drain_collectives(fp)
        fp.generation += 1
        for wp in self.net._rdn_packs.values():
            wp.key = None          # the weight repack is the graph's first launch
        self.graph = None
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.graph(g):
            self.loss = self._body().detach()
        self.graph_nodes = _node_count(g)
        g.instantiate()
        self.graph = g
        self._captured = self._hyper()
        # capture ran nothing: undo its host-side effects (step count, pack keys)
        opt.set_host_counts(counts, device=False)
        fp.generation += 1
        torch.cuda.set_rng_state(rng, self.dev)

    # ------------------------------------------------------------------
    def __call__(self, clean_images, noisy_images, t=None):
        """One train step on this batch; returns the loss (a device tensor, valid
        until the next call)."""
        self.opt.check_ema_not_swapped("TrainStepGraph")
        if self._hyper() != self._captured:
            self._build(1)
        self.clean.copy_(clean_images)
        self.noisy.copy_(noisy_images)
        if self.t is not None:
            if t is None:
                if not self.task.host_t:
                    raise ValueError("this graph was built with t_input=True: pass t")
                t = self.task.draw_t(self.clean.size(0))
            self.t.copy_(t)
        elif t is not None:
            raise ValueError("this graph has no t input: its step takes no t, or draws it itself (build it with "
                             "t_input=True to pass t)")
        self.graph.replay()
        if self.kind in ('step', 'accum_step'):
            self.opt._replayed()
        return self.loss


class TrainStepGraphs:
    """One captured train step per input shape and kind (config 5's mixed 128/256
    patch stream, synth.MixedPatchLoader; the trainers' step / loss / accumulate
    batches): a batch of a new (shape, kind) captures its own
    TrainStepGraph (its own engine, activations and graph); the graphs share the
    model's flat parameters, gradient buffer and accumulator and the optimizer's state
    (moments and the device step counter), and replays run one after another on the
    stream, so the alternation is the same sequence of steps as eager training."""

    def __init__(self, model, optimizer, distribution_choice='uniform', clip_value=1.0, t_input=False, warmup=2,
                 loss_weights=None, *, task=None):
        self.model, self.opt = model, optimizer
        self.kw = dict(clip_value=clip_value, t_input=t_input, warmup=warmup,
                       task=task or model.train_task(distribution_choice, loss_weights))
        self.graphs = {}
        self.captures = 0

    def __call__(self, clean_images, noisy_images, t=None, kind='step'):
        key = (tuple(clean_images.shape), kind)
        g = self.graphs.get(key)
        if g is None:
            g = self.graphs[key] = TrainStepGraph(self.model, self.opt, key[0], kind=kind, **self.kw)
            self.captures += 1
        return g(clean_images, noisy_images, t)


def trainer_graphs(model, optimizer, distribution_choice='uniform', clip_value=1.0, loss_weights=None, *, task=None):
    """The TrainStepGraphs of a trainer (trainer.train_epochs(captured=True)), kept on the
    model: a later call with the same optimizer and settings replays what an earlier one
    captured."""
    if not is_fused(optimizer):
        raise TypeError("captured training needs a fused optimizer: build it with make_optimizer(..., fused=True) "
                        f"(optim.FusedAdam / FusedAdamW / FusedAdadelta), got {type(optimizer).__name__}")
    task = task or model.train_task(distribution_choice, loss_weights)
    key = (task.graph_key[0], float(clip_value)) + task.graph_key[1:]
    table = model.__dict__.setdefault("_rdn_train_graphs", {})
    g = table.get(key)
    if g is None or g.opt is not optimizer:
        g = table[key] = TrainStepGraphs(model, optimizer, clip_value=clip_value, task=task)
    return g
