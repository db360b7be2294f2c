"""Fused RDUNet execution engine: the whole forward / backward of ``RDUNet_T`` or
``RDUNet`` as a fixed sequence of ``librdunet_hip`` launches over NHWC buffers.

Layout in HBM (per engine = per (batch, H, W, dtype, train) shape):

* level l (l = 0..3) has P_l = B*(H>>l)*(W>>l) pixels and F_l = base_filters*2^l
  channels.  Every dense block owns one buffer ``[P_l, F_l + 3*F_l/2]``: conv_k
  reads the channel prefix and writes its F_l/2 outputs behind it, so the
  reference's ``torch.cat`` calls (Unet_model.py:83,85,87) never copy.
* conv_3 (+PReLU + residual, :88-89) writes straight into the next consumer's
  buffer (the next block, or the skip/concat buffer ``CAT_l = [skip F_l | up
  F_{l+1}]`` read by ``down_l`` and ``up_l``), so ``torch.cat([concat, upsample])``
  (:43) is free as well.
* the PReLU input of every conv is kept (``PRE_*``) for the backward, as aten
  autograd keeps it; gradients of activations mirror the activation buffers.
* parameters and their gradients live in one flat fp32 buffer each (the
  nn.Parameters are views), so grad-norm clipping, the optimizer and the DDP
  all-reduce are single flat launches.

Ordering of the backward (what is stored vs accumulated) follows the
dependency order of the reference's autograd graph; see DESIGN.md.
"""
from __future__ import annotations

import ctypes as C
import os
import warnings
import weakref
from dataclasses import dataclass, field
from functools import partialmethod
from types import MappingProxyType

import torch

from . import _hip as H

_ALIGN = 64  # elements


def _ru(x, m):
    return (x + m - 1) // m * m


# ----------------------------------------------------------------- parameters
_GPOOL_MAX = 4


def _storage_refs(t: torch.Tensor) -> int:
    """Tensors sharing ``t``'s storage (``t`` itself included)."""
    return torch._C._storage_Use_Count(t.untyped_storage()._cdata) - 1


class ParamSet:
    """A module's parameters in a fixed order at aligned offsets of one flat fp32
    index space, and the flat buffers their gradients are produced into.

    The backward writes every weight gradient of one pass into ONE flat buffer
    and hands autograd a fresh view per parameter: ``AccumulateGrad`` adopts a
    view as ``p.grad`` when ``p.grad`` is None (the usual ``zero_grad()`` loop,
    so ``.grad`` tensors are views of one flat buffer and clipping / the fused
    optimizer / the DDP all-reduce stay single launches) and adds it into
    ``p.grad`` otherwise, exactly as it does for aten's gradients;
    ``torch.autograd.grad`` returns the views themselves.  A buffer is reused only
    when no tensor references its storage any more (``p.grad`` views, grads a
    caller kept), so a pass never overwrites a gradient anyone still holds."""

    def _layout(self, module: torch.nn.Module, device):
        self.params = list(module.parameters())
        self.names = [n for n, _ in module.named_parameters()]
        self.index = {n: i for i, n in enumerate(self.names)}
        offs, o = [], 0
        for p in self.params:
            offs.append(o)
            o = _ru(o + p.numel(), _ALIGN)
        self.numel = o
        self.offsets = offs
        self.device = device
        self._shapes = [tuple(p.shape) for p in self.params]
        self._strides = [torch.empty(s, device="meta").stride() for s in self._shapes]
        self._gpool = [torch.zeros(o, dtype=torch.float32, device=device)]
        self._gcur = self._gpool[0]
        self._gexpect = {}
        self.grad_sync = None   # ddp.GradSync attached by data-parallel training

    @property
    def gflat(self) -> torch.Tensor:
        """The flat buffer the ``.grad`` tensors are views of (after
        ``grads_are_views()``), else the last one a backward produced."""
        return self._gcur

    def grad_buffer(self) -> torch.Tensor:
        """A flat gradient buffer nothing references (the caller zero-fills it)."""
        for b in self._gpool:
            if _storage_refs(b) == 1:
                return b
        b = torch.empty(self.numel, dtype=torch.float32, device=self.device)
        if len(self._gpool) < _GPOOL_MAX:
            self._gpool.append(b)
        return b

    def grad_views(self, buf: torch.Tensor, which=None) -> list:
        """Fresh per-parameter views of a flat gradient buffer (None where
        ``which[i]`` is false)."""
        st = torch.as_strided
        if which is None:
            return [st(buf, s, r, o) for s, r, o in zip(self._shapes, self._strides, self.offsets)]
        return [st(buf, s, r, o) if w else None for s, r, o, w in zip(self._shapes, self._strides, self.offsets, which)]

    def grads_are_views(self) -> bool:
        """Every ``p.grad`` is its view of one pooled flat buffer; that buffer
        becomes ``gflat``."""
        ptrs = [0 if p.grad is None else p.grad.data_ptr() for p in self.params]
        for b in self._gpool:
            exp = self._gexpect.get(b.data_ptr())
            if exp is None:
                base = b.data_ptr()
                exp = self._gexpect[base] = [base + 4 * o for o in self.offsets]
            if ptrs == exp:
                self._gcur = b
                return True
        return False


class FlatParams(ParamSet):
    """Flat fp32 storage for a module's parameters (and gradients).

    The module's ``nn.Parameter`` objects keep their identity (optimizers and
    ``state_dict`` see the usual tensors) but their ``.data`` become views of
    ``self.flat``; ``.grad`` become views of a flat gradient buffer (ParamSet)."""

    def __init__(self, module: torch.nn.Module, device):
        self._layout(module, device)
        self.flat = torch.zeros(self.numel, dtype=torch.float32, device=device)
        self.views = []
        with torch.no_grad():
            for p, off in zip(self.params, self.offsets):
                v = self.flat[off:off + p.numel()].view_as(p)
                v.copy_(p.data.to(device=device, dtype=torch.float32))
                p.data = v
                self.views.append(v)
        self._ptrs = [v.data_ptr() for v in self.views]
        self.generation = 0
        _FLAT_REGISTRY[:] = [r for r in _FLAT_REGISTRY if r() is not None]
        _FLAT_REGISTRY.append(weakref.ref(self))

    def intact(self) -> bool:
        """Every parameter's storage is still its view of ``flat`` (host-cheap:
        one pointer list compare; runs several times per training step)."""
        f32 = torch.float32
        return [p.data_ptr() for p in self.params] == self._ptrs and all(p.dtype is f32 for p in self.params)

    def version_key(self):
        return (self.generation, sum(p._version for p in self.params))


class BlockParams(ParamSet):
    """The parameters of one block run on its own (``DenoisingBlock(...)(x)``):
    used in place (no flat copy, so a block that is also part of a fused
    network keeps sharing the network's storage); its GEMM packs are rebuilt
    on every forward, as nothing tracks raw-pointer writes into that storage."""

    def __init__(self, module: torch.nn.Module, device):
        for n, p in module.named_parameters():
            if p.device != device or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError(f"{type(module).__name__}: parameter {n} must be a contiguous fp32 tensor "
                                   f"on {device} (got {p.dtype} on {p.device})")
        self._layout(module, device)
        self._ptrs = [p.data_ptr() for p in self.params]
        self.generation = 0

    def intact(self) -> bool:
        return [p.data_ptr() for p in self.params] == self._ptrs

    def version_key(self):
        self.generation += 1
        return self.generation


_FLAT_REGISTRY: list = []

# Optional launch tracer (bench.py): an object with start(info) -> token|None and
# stop(token); info = (phase, layer, kernel key, algorithmic flops, algorithmic bytes).
TRACER = None

# PReLU backward is fused into a layer's dgrad/wgrad loaders when its weight-gradient
# kernel reads the gated operand in ONE input-channel chunk (re-gating it per chunk
# cost more than the separate pass it saves, r02 A/B)
FUSE_PRELU = os.environ.get("RDN_FUSE_PRELU", "1") != "0"
# weight gradients on a side stream (overlapped with the dgrad chain) and the depth
# of the dYpre ring that decouples the two chains
WGRAD_STREAM = os.environ.get("RDN_WGRAD_STREAM", "1") != "0"
# (a ring of 6 slots: 1690 / 1691 img/s against 1672 / 1673 with 4, 1681-1684 with 8,
# 1678-1682 with 12, profiles/r03_v9_slots_ab.txt; one slot per layer -- no dgrad-chain
# waits on the weight-gradient stream at all, each a ~6 us cross-queue gap in the
# replayed graph -- 1739 / 1742 against 1723 / 1724 with 6, profiles/r03_v11_slots_ab.txt;
# all interleaved on one box.  Memory: the dYpre / partial / slab buffers of every layer,
# ~1.5 GB at B16)
WGRAD_SLOTS = int(os.environ.get("RDN_WGRAD_SLOTS", "0"))   # 0: one slot per layer (within SLOT_BUDGET)
SLOT_BUDGET = float(os.environ.get("RDN_SLOT_BUDGET", "0.25"))   # fraction of free device memory
# With one slot per layer the captured graph has no edge from the weight-gradient branch
# back into the dgrad chain, and the replay enqueues the whole chain before the branch:
# harmless while the host enqueues a replay in ~1 ms, but under a profiler (slower
# enqueue) the branch then ran after the chain (10.3 vs 9.4 ms per step traced,
# profiles/r03_v13_prof_modes.txt).  Every ORDER_EVERY layers the chain therefore waits
# for the branch ORDER_EVERY layers back (a few cross-queue edges per step) to pin the
# replay order.
ORDER_EVERY = int(os.environ.get("RDN_ORDER_EVERY", "12"))
# bench.py's per-kernel profiling pass serialises the backward (isolated kernel times)
SERIAL_BWD = False
# channel-blocked ("planar") activation buffers: a level-l buffer is [C/cb, P, cb] with
# cb = F_l/2 (one plane per dense-block growth slice), so a conv reading or writing a
# channel slice touches only its planes (include/rdunet_hip.h, *_pl fields)
PLANAR = os.environ.get("RDN_PLANAR", "1") != "0"
# gated level-0 convs: input + weight gradient in one fused kernel on the compute
# stream (rdn_conv_dgrad_wgrad) instead of dgrad there and wgrad on the side stream
FUSE_DW = os.environ.get("RDN_DW", "1") != "0"
# PReLU backward of a layer fused into the input-gradient epilogue of its last
# consumer in backward order (rdn_conv_desc.gout: conv_k+1 finishes dense slice
# out_k, up_l.conv finishes up_l.conv_t's output), instead of a separate pass.
# Per launch it saves 0.5-6 us at levels 2/3 (scripts/gate_kbench.py,
# profiles/r03_v9_gate_kbench.json); with the r03 ring of dYpre slots the whole step
# measured 1666-1674 img/s with it against 1680-1691 without (profiles/r03_v9_slots_ab.txt:
# the longer finisher launches sat on the critical path beside the weight-gradient
# stream).  Round 4 (one slot per layer, column-half dw, conv3_big prefetch), interleaved:
# +0.2 % B16 / +0.2 % B32 on top of the prefetch (profiles/r04_v5_big_pf_gate_out_ab.txt):
# on by default.  Tested both ways (tests/test_gpu_gateout.py).
GATE_OUT = os.environ.get("RDN_GATE_OUT", "1") == "1"
# gate-out in the fused dgrad+wgrad kernel (conv3_dw ",go": up_0.conv finishing
# up_0.conv_t, the level-1 conv_0s finishing down_0 / the previous block's conv_3)
GATE_OUT_DW = os.environ.get("RDN_GATE_OUT_DW", "1") == "1"
# round 5: the level-1 conv_3 (160 input channels, 64 dY channels) as ONE fused dgrad +
# wgrad launch in five 32-channel parts (conv3_dw "h5") instead of conv3_big dgrad on
# the compute stream + wgrad3_glds on the side stream.  Pre-gated: the kernel reads the
# layer's dYpre, gated once by a gate-out finisher or the PReLU-backward pass (gated in
# each part's loader, the five parts gated the same tile five times: 143 vs 101 us per
# launch at B16, profiles/r05_*); RDN_DW_PREGATED=0 gates in the loaders instead
DW_PREGATED = os.environ.get("RDN_DW_PREGATED", "1") != "0"
# every split-K reduce is a rdn_wgrad_reduce_batch launch (_ReduceQueue): those of
# consecutive fused layers go in one launch on the compute stream
# (RDN_REDUCE_BATCH=0: one launch per layer, its column parts as its jobs)
REDUCE_BATCH = os.environ.get("RDN_REDUCE_BATCH", "1") != "0"
# conv_0..conv_2 of every level-0 DenoisingBlock (base_filters 32, bf16) as ONE
# launch that reads x once and keeps out_0 / out_1 on chip (rdn_dense3_fwd)
FUSE_DENSE = os.environ.get("RDN_DENSE", "1") != "0"
# round 6: the level-1 blocks' conv_0..2 as one launch too (conv3_dense1.hip); RDN_DENSE1=0
# keeps them on the three rdn_conv_fwd launches (A/B)
FUSE_DENSE1 = os.environ.get("RDN_DENSE1", "1") != "0"
# round 6: 3x3 forwards whose pixel grid covers under half of the CUs (a batch-1
# forward's deep levels) run split-K (rdn_conv_fwd_splitk; RDN_SPLITK=0: off)
SPLITK = os.environ.get("RDN_SPLITK", "1") != "0"
# round 6: the weight-gradient stream's split-K reduces of this many consecutive
# layers in one rdn_wgrad_reduce_batch launch (each layer its own slab of a ring;
# RDN_SIDE_BATCH=1: one one-job launch per layer, right behind its wgrad)
SIDE_BATCH = max(1, min(8, int(os.environ.get("RDN_SIDE_BATCH", "4"))))
# forward-only batches are run in chunks of at most this many pixels (run_unet)
FWD_CHUNK_PIXELS = 1 << 23


def find_flat(params, need_grads=True):
    """The FlatParams whose parameter list is exactly ``params`` (same objects,
    same order) with every gradient its view of one flat gradient buffer
    (which becomes its ``gflat``), else None.  ``need_grads=False`` drops the gradient
    condition (what only reads or writes the weights: optim.EMA)."""
    params = list(params)
    for ref in _FLAT_REGISTRY:
        fp = ref()
        if fp is None or len(fp.params) != len(params):
            continue
        if (all(a is b for a, b in zip(fp.params, params)) and fp.intact()
                and (not need_grads or fp.grads_are_views())):
            return fp
    return None


def flat_params(module: torch.nn.Module, device) -> FlatParams:
    fp = getattr(module, "_rdn_flat", None)
    if fp is None or fp.device != device or not fp.intact():
        fp = FlatParams(module, device)
        module._rdn_flat = fp
        module._rdn_packs = {}
        module._rdn_engines = {}
    return fp


def block_params(module: torch.nn.Module, device) -> BlockParams:
    bp = getattr(module, "_rdn_flat", None)
    if bp is None or bp.device != device or not bp.intact():
        bp = BlockParams(module, device)
        module._rdn_flat = bp
        module._rdn_packs = {}
        module._rdn_engines = {}
    return bp


# ----------------------------------------------------------------- layer plan
@dataclass
class Slice:
    """An NHWC channel slice: buffer name, channel offset."""
    buf: str
    c0: int = 0


# who produces a layer's dYpre (the gradient at its PReLU input)
GATE_LOADER = "loader"       # its own dgrad / wgrad loaders gate dY with the saved PReLU input
GATE_FINISHER = "finisher"   # the dgrad epilogue of its last consumer (gate-out, `gated_by`)
GATE_PRELU = "prelu"         # the separate rdn_prelu_bwd pass


@dataclass
class LayerBwd:
    """Backward launch state of one layer in a train engine.  ``gate`` and ``dw`` are
    the layer's path: who produces dYpre, and whether the gradients come from the
    fused dgrad+wgrad kernel on the compute stream (``dw``; ``pregated``: it reads
    dYpre, else it gates in its loader) or from dgrad there + wgrad on the side stream."""
    bidx: int                 # position in backward order
    slot: int                 # ring slot of its dYpre / partials / fused slabs (bidx % slots)
    dyp: int                  # dYpre pointer (the slot's buffer)
    olvl: int                 # level of the output grid
    pidx: list                # parameter indices: weight, bias, PReLU weight
    goff: list                # their byte offsets in a flat gradient buffer
    gate: str = GATE_PRELU
    dw: bool = False
    pregated: bool = False
    wgrad: tuple = ()         # (splits, mdim, ndim, ndim_real, taps) of the weight-gradient slabs
    dw_bytes: int = 0         # fused kernel's slabs (0: not dw)
    dw_cols: int = 0          # input channels per slab (< ndim: column parts)
    part_bytes: int = 0       # dalpha / dbias partials
    part_rows: int = 0        # partial rows the reduce sums besides the loaders' (0: GATE_LOADER)
    pws: int = 0              # partials pointer (the slot's buffer)
    side_slab: int | None = None   # side-stream layers: entry of the ws_side ring
    gates: ConvLayer | None = field(default=None, repr=False)      # layer whose dYpre this dgrad epilogue writes
    gated_by: ConvLayer | None = field(default=None, repr=False)   # ... and the reverse link
    ev_ready: object = None   # dYpre ready (compute stream)
    ev_done: object = None    # weight gradients reduced, slot free


@dataclass
class ConvLayer:
    name: str                 # module prefix, e.g. "block_0_0.conv_1"
    act: str                  # PReLU prefix, e.g. "block_0_0.actv_1"
    kind: str                 # "c3" | "down" | "up"
    level: int                # level of the GEMM rows in forward (c3/down: output; up: input)
    cin: int                  # real input channels
    cin_pad: int
    cout: int                 # real output channels
    cout_pad: int
    src: Slice                # forward input
    dst: Slice | None         # forward output (None -> NCHW image)
    pre: str                  # pre-activation buffer name
    resid: Slice | None = None  # residual added after PReLU (dense conv_3)
    resid_c: int = 0
    dsrc: Slice | None = None   # gradient of the input slice (None -> not needed)
    accum: bool = False         # dgrad accumulates (else stores)
    ddst: Slice | None = None   # gradient arriving at dst (None -> NCHW dy)
    fwd_desc: object = None
    dgrad_desc: object = None
    wgrad_desc: object = None
    pack_fwd: tuple = ()
    pack_dgrad: tuple = ()
    # bound by the engine that runs the layer
    splitk: int = 0             # forward runs split-K in this many slices (0: single pass)
    dense3: object = None       # conv_0 of a fused dense block: the conv_0..2 launch's descriptor
    dense3_skip: bool = False   # conv_1 / conv_2 of such a block: no launch of their own
    info: dict | None = None    # launch name -> (phase, layer, key, flops, bytes[, fused_min]) for the tracer
    bwd: LayerBwd | None = None  # backward launch state (None in forward-only engines)

    @property
    def extra(self):
        """Read-only view of the bound state for tests, bench.py and scripts; a key is
        present only where the layer has that state."""
        S = self.bwd
        v = {"info": self.info, "splitk": self.splitk or None, "dense3": self.dense3, "dw": S and S.dw,
             "gates": S and S.gates, "side_slab": S and S.side_slab}
        return MappingProxyType({k: x for k, x in v.items() if x is not None})


def reduce_jobs(S: LayerBwd, ws: int, gbase: int) -> list:
    """The split-K reduce of one layer's weight gradient (slabs at ``ws``) into the flat
    gradient buffer at ``gbase``, as rdn_wgrad_reduce_batch jobs: one, or one per column
    part of the fused kernel (each part's slabs hold ``dw_cols`` input channels; the
    dalpha/dbias partials are part 0's rows).  Plain integers in, ctypes structs out."""
    splits, mdim, ndim, ndim_real, taps = S.wgrad
    ow, ob, oa = S.goff
    cols = S.dw_cols
    nh = ndim // cols
    sh = splits // nh
    jn, jr = (cols, cols) if nh > 1 else (ndim, ndim_real)
    part_splits = sh if nh > 1 and S.gate == GATE_LOADER else S.part_rows
    return [H.ReduceJob(ws=ws + hh * sh * mdim * taps * cols * 4, grad=gbase + ow, part=S.pws if hh == 0 else None,
                        dalpha=gbase + oa, dbias=gbase + ob, splits=sh, mdim=mdim, ndim=jn, ndim_real=jr, taps=taps,
                        gstride=ndim_real, gci0=hh * cols, accumulate=1, part_splits=part_splits)
            for hh in range(nh)]


class _ReduceQueue:
    """Layers whose reduce jobs wait for one rdn_wgrad_reduce_batch launch on ``st``
    (``stream``: its torch stream when the pass has a side stream, else None); ``cap``
    layers fill it (None: flushed by the sweep only)."""
    __slots__ = ("st", "stream", "cap", "sync", "layers", "jobs")

    def __init__(self, st, stream, cap, sync):
        self.st, self.stream, self.cap, self.sync = st, stream, cap, sync
        self.layers, self.jobs = [], []

    def holds(self, L):
        return any(Lp is L for Lp in self.layers)

    def add(self, L, jobs):
        self.layers.append(L)
        self.jobs += jobs
        if self.cap is not None and len(self.layers) >= self.cap:
            self.flush()

    def flush(self):
        jl, fn = self.jobs, H.lib().rdn_wgrad_reduce_batch
        for i in range(0, len(jl), H.REDUCE_BATCH_MAX):
            n = min(H.REDUCE_BATCH_MAX, len(jl) - i)
            rc = fn((H.ReduceJob * n)(*jl[i:i + n]), n, self.st)
            if rc:
                H.check(rc, f"wgrad_reduce_batch[{self.layers[0].name}..{self.layers[-1].name}]")
        for L in self.layers:   # slot free / gradients complete, on the stream that reduced them
            if self.stream is not None:
                L.bwd.ev_done.record(self.stream)
            if self.sync is not None:
                self.sync.params_done(L.bwd.pidx, stream=self.stream)
        self.layers, self.jobs = [], []


@dataclass
class Program:
    """What one engine runs: forward-ordered convs over named NHWC buffers
    ``{name: (level, channels)}`` (level l = the input grid halved l times).

    ``inputs`` are the NCHW fp32 tensors of forward, each stored at channel 0 of
    its buffer ``(buffer, level, channels)``; ``image_input``: input 0 is the network's
    image, packed into 8-channel rows by ``rdn_pack_input``, with the broadcast t
    map as its next channel when ``time_input`` (RDUNet_T).  The last conv writes
    the NCHW fp32 output of level ``out_level``, adding ``inputs[0]`` when
    ``resid_input`` (the network's ``+ inputs``, Unet_model.py:166, or a dense
    block's ``out_3 + x``, :89).  ``cb``: level -> plane width of the
    channel-blocked buffers of that level (none: plain NHWC)."""
    layers: list
    bufs: dict
    inputs: list
    out_level: int
    out_channels: int
    resid_input: bool
    time_input: bool = False
    image_input: bool = False
    cb: dict = field(default_factory=dict)
    min_div: int = 1


def _plan(F0: int, cin_img: int, has_t: bool, cout_img: int) -> Program:
    """The whole network (Unet_model.py:92-166 / RDUNet_model.py)."""
    F = [F0 << l for l in range(4)]
    D = [f + 3 * (f // 2) for f in F]
    bufs = {"IN": (0, 8), "IB1": (0, F[0]), "O6": (0, F[0]), "OB1": (0, F[0]),
            "PRE_OUT": (0, 8)}
    for l in range(4):
        for k in range(4 if l < 3 else 2):
            bufs[f"B{l}{k}"] = (l, D[l])
        if l < 3:
            bufs[f"CAT{l}"] = (l, F[l] + F[l + 1])
        if l > 0:
            bufs[f"U{l}"] = (l, F[l])
    layers: list[ConvLayer] = []

    def c3(name, act, level, cin, cout, src, dst, pre_c, resid=None, resid_c=0, cin_pad=None, cout_pad=None):
        pre = f"PRE_{name}"
        bufs[pre] = (level, cout_pad or cout)
        layers.append(ConvLayer(name, act, "c3", level, cin, cin_pad or cin, cout, cout_pad or cout,
                                src, dst, pre, resid, resid_c))

    cin_in = cin_img + (1 if has_t else 0)
    c3("input_block.conv_1", "input_block.actv_1", 0, cin_in, F[0], Slice("IN"), Slice("IB1"), 0, cin_pad=8)
    c3("input_block.conv_2", "input_block.actv_2", 0, F[0], F[0], Slice("IB1"), Slice("B00"), 0)

    def dense(blk, l, buf, dst):
        C_, i = F[l], F[l] // 2
        for k in range(3):
            c3(f"{blk}.conv_{k}", f"{blk}.actv_{k}", l, C_ + k * i, i, Slice(buf), Slice(buf, C_ + k * i), 0)
        c3(f"{blk}.conv_3", f"{blk}.actv_3", l, C_ + 3 * i, C_, Slice(buf), dst, 0, resid=Slice(buf), resid_c=C_)

    def down(l):
        pre = f"PRE_down_{l}"
        bufs[pre] = (l + 1, F[l + 1])
        layers.append(ConvLayer(f"down_{l}.conv", f"down_{l}.actv", "down", l + 1, F[l], F[l], F[l + 1], F[l + 1],
                                Slice(f"CAT{l}"), Slice(f"B{l + 1}0"), pre))

    def up(l):
        # ConvTranspose2d(F[l+1] -> F[l+1]) then Conv2d(F[l] + F[l+1] -> F[l])
        pre = f"PRE_up_{l}_t"
        bufs[pre] = (l, F[l + 1])
        layers.append(ConvLayer(f"up_{l}.conv_t", f"up_{l}.actv_t", "up", l + 1, F[l + 1], F[l + 1], F[l + 1],
                                F[l + 1], Slice(f"U{l + 1}"), Slice(f"CAT{l}", F[l]), pre))
        c3(f"up_{l}.conv", f"up_{l}.actv", l, F[l] + F[l + 1], F[l], Slice(f"CAT{l}"), Slice(f"B{l}2"), 0)

    dense("block_0_0", 0, "B00", Slice("B01"))
    dense("block_0_1", 0, "B01", Slice("CAT0"))
    down(0)
    dense("block_1_0", 1, "B10", Slice("B11"))
    dense("block_1_1", 1, "B11", Slice("CAT1"))
    down(1)
    dense("block_2_0", 2, "B20", Slice("B21"))
    dense("block_2_1", 2, "B21", Slice("CAT2"))
    down(2)
    dense("block_3_0", 3, "B30", Slice("B31"))
    dense("block_3_1", 3, "B31", Slice("U3"))
    up(2)
    dense("block_2_2", 2, "B22", Slice("B23"))
    dense("block_2_3", 2, "B23", Slice("U2"))
    up(1)
    dense("block_1_2", 1, "B12", Slice("B13"))
    dense("block_1_3", 1, "B13", Slice("U1"))
    up(0)
    dense("block_0_2", 0, "B02", Slice("B03"))
    dense("block_0_3", 0, "B03", Slice("O6"))
    c3("output_block.conv_1", "output_block.actv_1", 0, F[0], F[0], Slice("O6"), Slice("OB1"), 0)
    layers.append(ConvLayer("output_block.conv_2", "output_block.actv_2", "c3", 0, F[0], F[0], cout_img, 8,
                            Slice("OB1"), None, "PRE_OUT"))
    return Program(layers, bufs, [("IN", 0, cin_img)], 0, cout_img, True, time_input=has_t, image_input=True,
                   cb={l: F[l] // 2 for l in range(4)}, min_div=8)


def block_program(block) -> Program:
    """One block of Unet_model.py:23-89 on its own: NCHW fp32 in and out, the
    same kernels and buffer conventions as inside the network.  Channel counts
    on a conv's input side must be multiples of 8 (the NHWC K chunks); the
    input block's image channels and the output block's image channels are
    padded to 8."""
    kind = type(block).__name__
    bufs: dict = {}
    layers: list[ConvLayer] = []

    def need8(*cs):
        for c in cs:
            if c % 8:
                raise ValueError(f"{kind}: the GPU kernels need channel counts that are multiples of 8; got {c}")

    def c3(name, act, cin, cout, src, dst, cout_pad=None):
        bufs[f"PRE_{name}"] = (0, cout_pad or cout)
        layers.append(ConvLayer(name, act, "c3", 0, cin, _ru(cin, 8), cout, cout_pad or cout, src, dst,
                                f"PRE_{name}"))

    if kind == "DenoisingBlock":       # :69-89
        C_, i, Co = block.conv_0.in_channels, block.conv_0.out_channels, block.conv_3.out_channels
        if Co != C_:
            raise ValueError(f"DenoisingBlock: out_3 + x needs out_channels == in_channels ({Co} != {C_})")
        need8(C_, i)
        bufs["X"] = (0, C_ + 3 * i)
        for k in range(3):
            c3(f"conv_{k}", f"actv_{k}", C_ + k * i, i, Slice("X"), Slice("X", C_ + k * i))
        c3("conv_3", "actv_3", C_ + 3 * i, Co, Slice("X"), None)
        return Program(layers, bufs, [("X", 0, C_)], 0, Co, True)
    if kind == "InputBlock":           # :45-55
        cin, F = block.conv_1.in_channels, block.conv_1.out_channels
        need8(F)
        bufs["X"], bufs["Y1"] = (0, _ru(cin, 8)), (0, F)
        c3("conv_1", "actv_1", cin, F, Slice("X"), Slice("Y1"))
        c3("conv_2", "actv_2", F, F, Slice("Y1"), None)
        return Program(layers, bufs, [("X", 0, cin)], 0, F, False)
    if kind == "OutputBlock":          # :57-67
        F, co = block.conv_1.in_channels, block.conv_2.out_channels
        need8(F)
        bufs["X"], bufs["Y1"] = (0, F), (0, F)
        c3("conv_1", "actv_1", F, F, Slice("X"), Slice("Y1"))
        c3("conv_2", "actv_2", F, co, Slice("Y1"), None, cout_pad=_ru(co, 8))
        return Program(layers, bufs, [("X", 0, F)], 0, co, False)
    if kind == "DownsampleBlock":      # :23-30
        cin, co = block.conv.in_channels, block.conv.out_channels
        need8(cin, co)
        bufs["X"], bufs["PRE_conv"] = (0, cin), (1, co)
        layers.append(ConvLayer("conv", "actv", "down", 1, cin, cin, co, co, Slice("X"), None, "PRE_conv"))
        return Program(layers, bufs, [("X", 0, cin)], 1, co, False, min_div=2)
    if kind == "UpsampleBlock":        # :32-43, forward((upsample, concat))
        cu, co = block.conv_t.in_channels, block.conv.out_channels
        cc = block.conv.in_channels - cu
        need8(cu, cc, co)
        bufs["U"], bufs["CAT"], bufs["PRE_conv_t"] = (1, cu), (0, cc + cu), (0, cu)
        layers.append(ConvLayer("conv_t", "actv_t", "up", 1, cu, cu, cu, cu, Slice("U"), Slice("CAT", cc),
                                "PRE_conv_t"))
        c3("conv", "actv", cc + cu, co, Slice("CAT"), None)
        return Program(layers, bufs, [("U", 1, cu), ("CAT", 0, cc)], 0, co, False)
    raise TypeError(f"no GPU program for {kind}")


def _assign_backward(layers):
    """Gradient routing: which slice receives each layer's input gradient and
    whether it is the first (store) or a later (accumulate) contribution, in
    backward (reverse) execution order."""
    written = set()
    # gradient arriving at a layer's output = gradient slice of its dst
    for L in layers:
        L.ddst = None if L.dst is None else Slice("d" + L.dst.buf, L.dst.c0)
    for L in reversed(layers):
        L.dsrc = Slice("d" + L.src.buf, L.src.c0)
        L.accum = L.dsrc.buf in written
        written.add(L.dsrc.buf)


# ----------------------------------------------------------------- weight packing
class WeightPacks:
    """Packed (GEMM-operand) copies of the conv weights for one dtype, rebuilt
    when the parameters change (optimizer step, load_state_dict).  Shared by
    every engine (input shape) of the module."""

    def __init__(self, module, fp: FlatParams, layers, dtype):
        self.dtype = dtype
        self.code = H.dtype_code(dtype)
        self.fp = fp
        self.key = None
        self.fwd, self.dgrad = {}, {}
        named = dict(module.named_parameters())
        dev = fp.device

        lib = H.lib()

        def mk(mode, w, d0, d1, kh, kw, pad0, pad1, rows, kp, ck=0):
            out = torch.zeros(_ru(rows, 128), _ru(kp, 64), dtype=dtype, device=dev)
            return (mode, w, d0, d1, kh, kw, pad0, pad1, out, out.shape[0], out.shape[1], ck)

        def chunk(c):
            ck, kp = lib.rdn_conv3_chunk(c, self.code), lib.rdn_conv3_packed_k(c, self.code)
            if ck <= 0 or kp <= 0:
                raise RuntimeError(f"conv3 K side of {c} channels unsupported")
            return ck, kp

        for L in layers:
            w = named[L.name + ".weight"]
            if L.kind == "c3":       # Conv2d 3x3 W[co][ci][3][3], chunked K for the halo kernel
                ck, kp = chunk(L.cin_pad)
                self.fwd[L.name] = mk(H.PACK_CONV_FWD, w, L.cout, L.cin, 3, 3, 0, L.cin_pad, L.cout, kp, ck)
                ck, kp = chunk(L.cout_pad)
                self.dgrad[L.name] = mk(H.PACK_CONV_DGRAD, w, L.cout, L.cin, 3, 3, L.cout_pad, 0, L.cin, kp, ck)
            elif L.kind == "down":   # Conv2d 2x2 s2 W[co][ci][2][2]
                self.fwd[L.name] = mk(H.PACK_CONV_FWD, w, L.cout, L.cin, 2, 2, 0, L.cin, L.cout, 4 * L.cin)
                self.dgrad[L.name] = mk(H.PACK_GEMM_T, w, L.cout, L.cin, 2, 2, L.cout, 0, 4 * L.cin, L.cout)
            else:                    # ConvTranspose2d 2x2 s2 W[ci][co][2][2]
                self.fwd[L.name] = mk(H.PACK_GEMM_T, w, L.cin, L.cout, 2, 2, L.cin, 0, 4 * L.cout, L.cin)
                self.dgrad[L.name] = mk(H.PACK_CONV_FWD, w, L.cin, L.cout, 2, 2, 0, L.cout, L.cin, 4 * L.cout)
        self.items = list(self.fwd.values()) + list(self.dgrad.values())
        arr = (H.PackItem * len(self.items))()
        for i, (mode, w, d0, d1, kh, kw, pad0, pad1, out, rows, kp, ck) in enumerate(self.items):
            arr[i] = H.PackItem(w.data_ptr(), out.data_ptr(), mode, d0, d1, kh, kw, pad0, pad1, rows, kp, ck)
        raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
        self.items_dev = raw.to(dev)   # device copy of the descriptors: one launch packs all

    def attach(self, layers):
        for L in layers:
            L.pack_fwd = self.fwd[L.name]
            L.pack_dgrad = self.dgrad[L.name]

    def refresh(self):
        key = self.fp.version_key()
        if key == self.key:
            return
        H.check(H.lib().rdn_pack_weights_batched(self.items_dev.data_ptr(), len(self.items), self.code,
                                                 H.stream_ptr()), "pack_weights_batched")
        self.key = key


def weight_packs(module, fp, layers, dtype) -> WeightPacks:
    wp = module._rdn_packs.get(dtype)
    if wp is None:
        wp = WeightPacks(module, fp, layers, dtype)
        module._rdn_packs[dtype] = wp
    return wp


# ----------------------------------------------------------------- engine
# descriptor pointers that select a kernel variant (kept as they are by the probes)
_SELECT = {H.ConvDesc: ("gate", "gate_alpha", "gout", "gout_pre", "gout_alpha", "gout_part"),
           H.WgradDesc: ("a_gate", "a_gate_alpha", "part")}


class UNetEngine:
    """Buffers and prebuilt launch descriptors of one Program (the network, or
    one block) for one input shape (B, H, W of level 0)."""

    def __init__(self, module, B, Hh, Ww, dtype, train: bool, prog: Program | None = None, params=None,
                 scratch: dict | None = None):
        if prog is None:
            F0 = module.base_filters
            if F0 % 16:
                raise RuntimeError(f"base_filters must be a multiple of 16 for the NHWC/MFMA layout; got {F0}")
            prog = _plan(F0, module.image_channels, module.time_conditioned, module.out_channels)
        if Hh % prog.min_div or Ww % prog.min_div:
            raise RuntimeError(f"{type(module).__name__} needs H and W divisible by {prog.min_div}; got {Hh}x{Ww}")
        self.module = module
        self.prog = prog
        # backward-only buffers (activation gradients, dYpre / partial / slab slots,
        # workspaces), shared by every grad-enabled engine of one (shape, dtype) pool:
        # backwards run one after another on the compute stream (each ends by waiting
        # for its weight-gradient stream), so one set serves all of them and a pooled
        # engine costs only its forward activations and PReLU inputs
        self.scratch = {} if scratch is None else scratch
        self.B, self.H, self.W = B, Hh, Ww
        self.dtype = dtype
        self.code = H.dtype_code(dtype)
        self.train = train
        self.module_training = bool(getattr(module, "training", False))
        dev = next(module.parameters()).device
        self.device = dev
        self.fp = params if params is not None else flat_params(module, dev)
        layers, bufspec = prog.layers, prog.bufs
        _assign_backward(layers)
        self.layers = layers
        self.packs = weight_packs(module, self.fp, layers, dtype)
        self.packs.attach(layers)
        self.P = [B * (Hh >> l) * (Ww >> l) for l in range(4)]
        self.grid = [(B, Hh >> l, Ww >> l) for l in range(4)]
        self.bufs = {}
        self.geo = {}   # buffer name -> (pixel stride ps, plane stride pl); pl = 0: plain NHWC
        in_bufs = {b for b, _, _ in prog.inputs}
        # buffers no layer writes in forward (pure inputs): their layers' input
        # gradients are only computed when that input needs a gradient
        self.pure_inputs = in_bufs - {L.dst.buf for L in layers if L.dst is not None}

        def alloc(name, lvl, ch, shared=False):
            cb = prog.cb.get(lvl, 0)
            if (PLANAR and cb and name not in in_bufs and name[1:] not in in_bufs and not name.startswith("PRE_")
                    and ch % cb == 0 and ch > cb):
                pl = self.P[lvl] * cb
                shape = (ch // cb, pl)
                self.geo[name] = (cb, pl)
            else:
                shape = (self.P[lvl], ch)
                self.geo[name] = (ch, 0)
            if shared:
                t = self._shared(("buf", name), lambda: torch.zeros(shape, dtype=dtype, device=dev))
            else:
                t = torch.zeros(shape, dtype=dtype, device=dev)
            self.bufs[name] = t

        for name, (lvl, ch) in bufspec.items():
            if not train and name.startswith("PRE_"):
                continue
            alloc(name, lvl, ch)
        self.named = dict(module.named_parameters())
        self._build_fwd()
        self._plan_dense3()
        if train:
            for name, (lvl, ch) in bufspec.items():
                if name.startswith("PRE_"):
                    continue
                alloc("d" + name, lvl, ch, shared=True)
            # weight gradients (wgrad + reduce) run on a side stream, overlapped with
            # the dgrad chain; the dYpre / PReLU-partial / slab buffers they read live in
            # SLOTS slots (layer b of the backward order uses slot b % SLOTS), each sized
            # for the largest layer that uses it; the dgrad chain waits for the side
            # stream only where it reuses a slot (default: one slot per layer, no waits)
            # (a high-priority side stream measured 1215 vs 1892 img/s B16, r06: not kept)
            self.side = torch.cuda.Stream(device=dev) if (dev.type == "cuda" and WGRAD_STREAM) else None
            if self.side is None:
                self.slots = 1
            elif WGRAD_SLOTS > 0:
                self.slots = min(WGRAD_SLOTS, len(layers))
            else:
                # one slot per layer while its dYpre buffers stay within a quarter of the
                # free device memory (1.5 GB at B16 256^2, 6 GB at B64 or 512^2 crops;
                # RDN_SLOT_BUDGET), else the 6-slot ring of round 3 (-1 % step)
                # (decided once per pool: its engines share the slot buffers)
                def pick():
                    need = sum(self.P[self._out_level(L)] * L.cout_pad for L in layers) * (2 if dtype == torch.bfloat16 else 4)
                    free = torch.cuda.mem_get_info(dev)[0]
                    return len(layers) if need <= SLOT_BUDGET * free else min(6, len(layers))
                self.slots = self._shared("slots", pick)
            sizes = [0] * self.slots
            for b, L in enumerate(reversed(layers)):
                sizes[b % self.slots] = max(sizes[b % self.slots], self.P[self._out_level(L)] * L.cout_pad)
            self.dyp = [self._shared(("dyp", i), lambda n=n: torch.zeros(n, dtype=dtype, device=dev))
                        for i, n in enumerate(sizes)]
            self._build_bwd()
        self._build_info()
        self.lease = None   # weakref to the autograd graph's lease while it owns the activations
        self.lease_seq = 0

    # ------------------------------------------------------------------
    def _shared(self, key, make):
        """A backward scratch buffer of this engine's pool (made on first use)."""
        t = self.scratch.get(key)
        if t is None:
            t = self.scratch[key] = make()
        return t

    def _out_level(self, L):
        return L.level - 1 if L.kind == "up" else L.level

    def _buf(self, name):
        return self.bufs[name]

    def _slice(self, sl):
        """(pointer, ps, c0, pl) of a channel slice of a buffer."""
        ps, pl = self.geo[sl.buf]
        return self.bufs[sl.buf].data_ptr(), ps, sl.c0, pl

    def _build_fwd(self):
        lib = H.lib()
        for L in self.layers:
            d = H.ConvDesc()
            d.dtype = self.code
            n, h, w = self.grid[L.level]
            d.n, d.h, d.w = n, h, w
            d.x, d.x_ps, d.x_c0, d.x_pl = self._slice(L.src)
            packed = L.pack_fwd[8]
            d.wp, d.kp = packed.data_ptr(), packed.shape[1]
            d.bias = self.named[L.name + ".bias"].data_ptr()
            d.alpha = self.named[L.act + ".weight"].data_ptr()
            flags = H.EPI_BIAS | H.EPI_PRELU
            pre = self.bufs.get(L.pre)
            if self.train:
                flags |= H.EPI_STORE_PRE
                d.pre, d.pre_ps = pre.data_ptr(), pre.shape[1]
            if L.kind == "c3":
                d.gather = H.RDN_G_CONV3
                d.hin, d.win = h, w
                d.cin = L.cin_pad
                d.ncols, d.cout = L.cout, L.cout
            elif L.kind == "down":
                d.gather = H.RDN_G_S2
                d.hin, d.win = 2 * h, 2 * w
                d.cin = L.cin
                d.ncols, d.cout = L.cout, L.cout
            else:
                d.gather = H.RDN_G_PIX
                d.hin, d.win = h, w
                d.cin = L.cin
                d.ncols, d.cout = 4 * L.cout, L.cout
                flags |= H.EPI_SCATTER2
            if L.dst is None:
                flags |= H.EPI_OUT_NCHW
                if self.prog.resid_input:   # + inputs (Unet_model.py:166) / out_3 + x (:89)
                    flags |= H.EPI_RESID
            else:
                d.out, d.out_ps, d.out_c0, d.out_pl = self._slice(L.dst)
                if L.resid is not None:
                    flags |= H.EPI_RESID
                    d.res, d.res_ps, d.res_c0, d.res_pl = self._slice(L.resid)
                    d.res_climit = L.resid_c
            d.flags = flags
            L.fwd_desc = d
        self._plan_splitk()

    def _plan_splitk(self):
        """Split-K slices of the forwards whose tile grid leaves most CUs idle
        (rdn_conv_fwd_splits > 0: a batch-1 forward's level-2/3 convs, 256 / 64 pixels
        at 64^2) and one workspace for their fp32 slices; forward-only engines (the
        samplers, config 1's RDUNet forward)."""
        if not SPLITK or self.train or self.module_training:
            # (forward-only engines of a module in eval mode: the samplers, inference.  A
            # train step's gradients at batch 1 are sums over a few thousand pixels, so the
            # fp32 reordering can flip a PReLU gate whose input is within noise of 0 and
            # move a whole gradient by ~1/sqrt(pixels): train engines keep the single-pass
            # launches; and a train-mode forward-only call -- the logged loss of a step whose
            # gradient the reference discards, diffusion_RDUnet.forward_step_device -- keeps
            # the train engine's kernels, so its loss is the train step's bit for bit.  The
            # mode is the module's when the engine is built, so _run keeps one forward-only
            # engine per mode under a shape's key and serves a call from the one whose
            # module_training equals module.training: an eval call never decides for a
            # later train-mode call of the same shape, nor the other way round)
            return
        lib = H.lib()
        need = 0
        for L in self.layers:
            s = lib.rdn_conv_fwd_splits(C.byref(L.fwd_desc))
            if s > 0:
                L.splitk = s
                need = max(need, lib.rdn_conv_fwd_splitk_workspace_size(C.byref(L.fwd_desc), s))
        if need:
            self.ws_fwd = torch.empty(need // 4 + 4, dtype=torch.float32, device=self.device)

    def _plan_dense3(self):
        """Dense blocks whose conv_0..conv_2 forward runs as one rdn_dense3_fwd launch
        (Unet_model.py:81-87): level 0 (x = 32 channels, growth 16, 16-channel planes)
        and, round 6, level 1 (x = 64 channels, growth 32, 32-channel planes; the
        level-1 grid a multiple of 16).  The three layers read the block buffer's
        channel prefix and write its next planes; the launch goes at conv_0, the other
        two are skipped."""
        if not FUSE_DENSE or self.code != H.RDN_BF16:
            return
        by_name = {L.name: L for L in self.layers}
        for L0 in self.layers:
            if not L0.name.endswith(".conv_0") or L0.kind != "c3" or L0.level not in (0, 1):
                continue
            lvl = L0.level
            if lvl == 1 and not FUSE_DENSE1:
                continue
            n, h, w = self.grid[lvl]
            if (lvl == 0 and (h % 8 or w % 16)) or (lvl == 1 and (h % 16 or w % 16)):
                continue
            g, x_c = (16, 32) if lvl == 0 else (32, 64)
            blk = L0.name[:-len(".conv_0")]
            Ls = [by_name.get(f"{blk}.conv_{k}") for k in range(3)]
            if any(L is None or L.kind != "c3" or L.level != lvl for L in Ls):
                continue
            buf = L0.src.buf
            ps, pl = self.geo[buf]
            if (ps != g or not pl or any(L.src.buf != buf or L.src.c0 != 0 or L.dst is None or L.dst.buf != buf
                                           or L.cout != g or L.cout_pad != g or L.resid is not None for L in Ls)
                    or [L.cin for L in Ls] != [x_c, x_c + g, x_c + 2 * g]
                    or [L.dst.c0 for L in Ls] != [x_c, x_c + g, x_c + 2 * g]):
                continue
            d = H.Dense3Desc()
            d.n, d.h, d.w = n, h, w
            d.x_c = x_c
            d.x, d.x_pl = self.bufs[buf].data_ptr(), pl
            for k, L in enumerate(Ls):
                ptr, _, c0, _ = self._slice(L.dst)
                d.out[k] = ptr + 2 * (c0 // ps) * pl
                pre = self.bufs.get(L.pre)
                d.pre[k] = pre.data_ptr() if pre is not None else None   # (forward-only: none kept)
                packed = L.pack_fwd[8]
                d.wp[k], d.kp[k] = packed.data_ptr(), packed.shape[1]
                d.bias[k] = self.named[L.name + ".bias"].data_ptr()
                d.alpha[k] = self.named[L.act + ".weight"].data_ptr()
            L0.dense3 = d
            for L in Ls[1:]:
                L.dense3_skip = True

    def _gate_operands(self, L):
        """(pointer, pixel stride, alpha pointer) of the saved PReLU input that gates dY."""
        pre = self.bufs[L.pre]
        return pre.data_ptr(), pre.shape[1], self.named[L.act + ".weight"].data_ptr()

    def _dgrad_desc(self, L, gated):
        """Input gradient as a forward-shaped conv over dYpre (``gated``: over dY,
        gated by the saved PReLU input in the loader)."""
        d = H.ConvDesc(dtype=self.code)
        packed = L.pack_dgrad[8]
        d.wp, d.kp = packed.data_ptr(), packed.shape[1]
        d.x, d.x_c0 = L.bwd.dyp, 0
        n, h, w = self.grid[L.level]
        flags = 0
        if L.kind == "c3":
            d.gather, d.hin, d.win = H.RDN_G_CONV3, h, w
            d.x_ps, d.cin = L.cout_pad, L.cout_pad
            d.ncols = d.cout = L.cin
            if gated:
                d.x, d.x_ps, d.x_c0, d.x_pl = self._slice(L.ddst)
                d.gate, d.gate_ps, d.gate_alpha = self._gate_operands(L)
        elif L.kind == "down":       # per-pixel GEMM on the low-res grid, scattered to 2x2
            d.gather, d.hin, d.win = H.RDN_G_PIX, h, w
            d.x_ps, d.cin = L.cout, L.cout
            d.ncols, d.cout = 4 * L.cin, L.cin
            flags |= H.EPI_SCATTER2
        else:                        # conv-s2 gather of the hi-res dYpre
            d.gather, d.hin, d.win = H.RDN_G_S2, 2 * h, 2 * w
            d.x_ps, d.cin = L.cout, L.cout
            d.ncols = d.cout = L.cin
        d.n, d.h, d.w = n, h, w
        d.out, d.out_ps, d.out_c0, d.out_pl = self._slice(L.dsrc)
        if L.accum:
            flags |= H.EPI_ACCUM
        if L.resid is not None:      # d(x) += dOut through "out_3 + x" (Unet_model.py:89)
            flags |= H.EPI_RESID
            d.res, d.res_ps, d.res_c0, d.res_pl = self._slice(L.ddst)
            d.res_climit = L.resid_c
        d.flags = flags
        return d

    def _wgrad_desc(self, L, gated):
        """Weight gradient dYpre^T x (gathered input); ``splits`` left 0 (automatic)."""
        n, h, w = self.grid[L.level]
        wg = H.WgradDesc(dtype=self.code, n=n, h=h, w=w)
        dyp = L.bwd.dyp
        if L.kind == "c3":
            wg.gather, wg.hin, wg.win = H.RDN_G_CONV3, h, w
            wg.a, wg.a_ps, wg.a_c0, wg.mdim = dyp, L.cout_pad, 0, L.cout
            wg.b, wg.b_ps, wg.b_c0, wg.b_pl = self._slice(L.src)
            wg.ndim = L.cin_pad
            if gated:
                wg.a, wg.a_ps, wg.a_c0, wg.a_pl = self._slice(L.ddst)
                wg.a_gate, wg.a_gate_ps, wg.a_gate_alpha = self._gate_operands(L)
        elif L.kind == "down":
            wg.gather, wg.hin, wg.win = H.RDN_G_S2, 2 * h, 2 * w
            wg.a, wg.a_ps, wg.a_c0, wg.mdim = dyp, L.cout, 0, L.cout
            wg.b, wg.b_ps, wg.b_c0, wg.b_pl = self._slice(L.src)
            wg.ndim = L.cin
        else:
            wg.gather, wg.hin, wg.win = H.RDN_G_S2, 2 * h, 2 * w
            wg.a, wg.a_ps, wg.a_c0, wg.a_pl = self._slice(L.src)
            wg.mdim = L.cin
            wg.b, wg.b_ps, wg.b_c0, wg.ndim = dyp, L.cout, 0, L.cout
        return wg

    def _plan_path(self, L):
        """A layer's backward path: (gated in the loaders, split count of the fused
        dgrad+wgrad kernel or 0, dgrad and wgrad descriptors).  In priority order: the
        pre-gated fused kernel (multi-chunk layers), the fused kernel gating in its own
        loader (also multi-chunk: column parts), the separate kernels gating in their
        loaders when the weight gradient reads the gated operand in ONE input-channel
        chunk, else the separate kernels over dYpre (always: NCHW dy, the 2x2 convs)."""
        lib = H.lib()
        gate_ok = L.kind == "c3" and L.ddst is not None and FUSE_PRELU
        single = False
        if gate_ok:
            n, h, w = self.grid[L.level]
            probe = H.WgradDesc(dtype=self.code, gather=H.RDN_G_CONV3, n=n, h=h, w=w, hin=h, win=w,
                                mdim=L.cout, ndim=L.cin_pad)
            single = lib.rdn_wgrad_chunks(C.byref(probe)) == 1
        dw_ok = gate_ok and FUSE_DW and L.src.buf not in self.pure_inputs
        fused_kernel = [False, True] if not single and DW_PREGATED else [True]
        for gated in fused_kernel if dw_ok else []:
            d, wg = self._dgrad_desc(L, gated), self._wgrad_desc(L, gated)
            dw = lib.rdn_conv_dgrad_wgrad_splits(C.byref(d), C.byref(wg))
            if dw > 0:
                return gated, dw, d, wg
        return single, 0, self._dgrad_desc(L, single), self._wgrad_desc(L, single)

    def _build_bwd(self):
        lib = H.lib()
        ws_need = 0
        for b, L in enumerate(reversed(self.layers)):   # backward order -> ring slot
            olvl, slot = self._out_level(L), b % self.slots
            pidx = [self.fp.index[n] for n in (L.name + ".weight", L.name + ".bias", L.act + ".weight")]
            L.bwd = S = LayerBwd(b, slot, self.dyp[slot].data_ptr(), olvl, pidx, [4 * self.fp.offsets[i] for i in pidx])
            fused, dw, d, wg = self._plan_path(L)
            S.gate, S.dw, S.pregated = GATE_LOADER if fused else GATE_PRELU, dw > 0, dw > 0 and not fused
            L.dgrad_desc, L.wgrad_desc = d, wg
            S.dw_cols = wg.ndim
            if dw > 0:   # the fused kernel's slabs: one per block of its persistent grid
                wg.splits = dw
                S.dw_bytes = dw * wg.mdim * 9 * wg.ndim * 4
                S.dw_cols = lib.rdn_conv_dgrad_wgrad_cols(C.byref(d), C.byref(wg))
            else:
                wg.splits = lib.rdn_wgrad_splits(C.byref(wg))
                ws_need = max(ws_need, lib.rdn_wgrad_workspace_size(C.byref(wg)))
            # dalpha / dbias partials: the fused loaders' per-split rows, else the
            # separate PReLU-backward pass's per-block rows
            if fused:
                S.part_bytes = wg.splits * 2 * wg.mdim * 4
            else:
                S.part_rows = lib.rdn_prelu_bwd_blocks(self.code, self.P[olvl], L.cout_pad)
                S.part_bytes = lib.rdn_prelu_bwd_workspace_size(self.code, self.P[olvl], L.cout, L.cout_pad)
            S.wgrad = (wg.splits, wg.mdim, wg.ndim, L.cout if L.kind == "up" else L.cin, 9 if L.kind == "c3" else 4)
        self._plan_gate_out()
        self._bind_bwd_buffers(ws_need)

    def _bind_bwd_buffers(self, ws_need):
        """Sizes the pool's shared workspaces from the planned layers and binds each
        layer's slab / partials pointers and events."""
        self.ws = self._shared("ws", lambda: torch.zeros(max(ws_need // 4, 4), dtype=torch.float32,
                                                          device=self.device))
        # per slot: fused layers' slabs (written from the compute stream while the side
        # stream may still reduce an earlier layer's) and the dalpha/dbias partials
        dwb, pwb = [0] * self.slots, [16] * self.slots
        for S in (L.bwd for L in self.layers):
            dwb[S.slot] = max(dwb[S.slot], S.dw_bytes)
            pwb[S.slot] = max(pwb[S.slot], S.part_bytes)
        f32 = dict(dtype=torch.float32, device=self.device)
        self.ws_dw = [self._shared(("ws_dw", i), lambda n=n: torch.zeros((n // 4 + 3) // 4 * 4, **f32)) if n else None
                      for i, n in enumerate(dwb)]
        self.pws = [self._shared(("pws", i), lambda n=n: torch.zeros((n // 4 + 3) // 4 * 4, **f32))
                    for i, n in enumerate(pwb)]
        # the weight-gradient stream's layers (not fused): a ring of SIDE_BATCH slabs in
        # backward order, so SIDE_BATCH consecutive layers' reduces can go in one launch
        self.side_batch = SIDE_BATCH if self.side is not None else 1
        self.ws_side = [self.ws] + [self._shared(("ws_side", i), lambda: torch.zeros(max(ws_need // 4, 4), **f32))
                                    for i in range(1, self.side_batch)]
        k = 0
        for L in reversed(self.layers):
            S, wg = L.bwd, L.wgrad_desc
            S.pws = self.pws[S.slot].data_ptr()
            if S.dw:
                wg.ws = self.ws_dw[S.slot].data_ptr()
            else:
                S.side_slab = k % self.side_batch
                wg.ws = self.ws_side[S.side_slab].data_ptr()
                k += 1
            if S.gate == GATE_LOADER:
                wg.part = S.pws
            if S.gated_by is not None:   # the finisher's epilogue writes this layer's partials
                S.gated_by.dgrad_desc.gout_part = S.pws
        if self.side is not None:   # per layer: dYpre ready (compute stream) / slot free (side stream)
            for L in self.layers:
                L.bwd.ev_ready, L.bwd.ev_done = torch.cuda.Event(), torch.cuda.Event()
            self.ev_begin = torch.cuda.Event()
            self.ev_end = torch.cuda.Event()

    def _plan_gate_out(self) -> None:
        """Pair every layer that still needs a separate PReLU-backward pass with the
        last consumer of its output in backward order when that consumer's input
        gradient has the layer's output as the tail of its columns (dense conv_k+1
        for slice out_k, Unet_model.py:81-87; up_l.conv for up_l.conv_t's output,
        :43), and let that epilogue write the layer's dYpre and dalpha/dbias
        partials (rdn_conv_desc.gout).  The partials' bytes go into the gated layer's
        ``part_bytes`` (sized into its slot's pws buffer)."""
        if not GATE_OUT:
            return
        lib = H.lib()
        index = {id(L): i for i, L in enumerate(self.layers)}
        for K in self.layers:
            if K.bwd.gate == GATE_LOADER or K.dst is None or K.kind == "down" or K.cout != K.cout_pad:
                continue
            lo, hi = K.dst.c0, K.dst.c0 + K.cout
            cons = [L for L in self.layers if index[id(L)] > index[id(K)] and L.src.buf == K.dst.buf
                    and L.src.c0 < hi and L.src.c0 + L.cin > lo]
            if not cons:
                continue
            J = min(cons, key=lambda L: index[id(L)])   # last in backward order
            dwj = J.bwd.dw
            # a residual reader of the slice adds its gradient in its own dgrad epilogue;
            # the fused dgrad+wgrad finisher runs after every such reader in backward
            # order (the next block's conv_3 before its conv_0), the others never do
            resid = [L for L in self.layers if L.resid is not None and L.resid.buf == K.dst.buf and
                     L.resid.c0 < hi and L.resid.c0 + L.resid_c > lo]
            if resid and not (dwj and all(index[id(L)] > index[id(J)] for L in resid)):
                continue
            # (level 0 with a conv3_big / conv3_halo finisher: its 8-byte-per-lane epilogue
            # streamed the extra PReLU input slower than the separate pass -- up_0: +13 us
            # per step; the fused dgrad+wgrad finisher prefetches it with the dX operand)
            if self._out_level(K) == 0 and not dwj:
                continue
            if (J.kind != "c3" or J.bwd.gates is not None or J.src.buf in self.pure_inputs
                    or J.cin != J.cin_pad or J.src.c0 + J.cin != hi or J.src.c0 > lo):
                continue
            pre = self.bufs[K.pre]
            d = J.dgrad_desc
            d.gout, d.gout_ps = K.bwd.dyp, K.cout_pad
            d.gout_pre, d.gout_pre_ps = pre.data_ptr(), pre.shape[1]
            d.gout_alpha = self.named[K.act + ".weight"].data_ptr()
            d.gout_part = 4096   # stand-in until the workspace exists (rows probe)
            d.gout_c0 = lo - J.src.c0
            if dwj:   # one partial row per block of the fused kernel's persistent grid
                if K.resid is not None:   # K's own dgrad reads its dY again (residual operand)
                    d.flags |= H.EPI_GOUT_KEEP
                wq = self._probe_copy(J.wgrad_desc, keep=("a_gate", "a_gate_alpha"))   # (part: stand-in)
                rows = lib.rdn_conv_dgrad_wgrad_gate_rows(C.byref(d), C.byref(wq)) if GATE_OUT_DW else 0
            else:
                rows = lib.rdn_conv_gate_rows(C.byref(d))
            if rows <= 0:
                d.flags &= ~H.EPI_GOUT_KEEP
                d.gout = d.gout_pre = d.gout_alpha = d.gout_part = None
                d.gout_ps = d.gout_pre_ps = d.gout_c0 = 0
                continue
            J.bwd.gates, K.bwd.gated_by, K.bwd.gate = K, J, GATE_FINISHER
            K.bwd.part_rows = rows
            K.bwd.part_bytes = max(K.bwd.part_bytes, rows * 2 * K.cout * 4)

    @staticmethod
    def _probe_copy(desc, keep=None):
        """Copy of a descriptor whose per-call pointers (bound at launch time) are
        stand-ins, for the dispatch probe; pointers that select a kernel variant
        (`keep`, default: the descriptor type's) stay as they are."""
        cls = type(desc)
        keep = _SELECT[cls] if keep is None else keep
        d = cls.from_buffer_copy(desc)
        for name, typ in cls._fields_:
            if name not in keep and issubclass(typ, (C.c_void_p, C._Pointer)) and not getattr(d, name):
                setattr(d, name, C.cast(C.c_void_p(4096), typ) if typ is not C.c_void_p else 4096)
        return d

    def _probe_key(self, probe, *descs):
        """Name of the kernel instantiation the library's own dispatch picks for the
        descriptor(s): ``probe`` is one of its rdn_*_kernel_name functions."""
        args = [C.byref(self._probe_copy(d) if type(d) in _SELECT else d) for d in descs]
        buf = C.create_string_buffer(128)
        H.check(getattr(H.lib(), probe)(*args, buf, 128), probe)
        return buf.value.decode()

    _kernel_key = partialmethod(_probe_key, "rdn_conv_kernel_name")
    _wgrad_key = partialmethod(_probe_key, "rdn_wgrad_kernel_name")
    _dense3_key = partialmethod(_probe_key, "rdn_dense3_kernel_name")   # (its pointers are bound at build time)
    _dw_key = partialmethod(_probe_key, "rdn_conv_dgrad_wgrad_kernel_name")   # (dgrad, wgrad)

    def _build_info(self):
        """Per launch: kernel instantiation key + algorithmic FLOPs and bytes
        (each operand read once, each output written once)."""
        es = 2 if self.code == H.RDN_BF16 else 4
        for L in self.layers:
            olvl = self._out_level(L)
            Pout, Pin = self.P[olvl], self.P[L.level if L.kind == "up" else (L.level - 1 if L.kind == "down" else L.level)]
            taps = 9 if L.kind == "c3" else 4
            if L.kind == "up":
                macs = self.P[L.level] * 4 * L.cout * L.cin
            else:
                macs = Pout * L.cout * taps * L.cin
            fwd_bytes = es * (Pin * L.cin + Pout * L.cout * (2 if self.train else 1) +
                              (Pout * L.cout if L.resid is not None else 0))
            fkey = self._kernel_key(L.fwd_desc) + (f",splitk{L.splitk}" if L.splitk else "")
            info = {"fwd": ("fwd", L.name, fkey, 2 * macs, fwd_bytes)}
            if L.dense3 is not None:   # conv_0..2 in one launch: their algorithmic work summed below
                info["dense3"] = None
            S = L.bwd
            if S is not None:
                # a fused PReLU backward (gate in the loader) also reads the saved
                # PReLU input of the output slice
                gate = Pout * L.cout if S.gate == GATE_LOADER else 0
                gout = Pin * S.gates.cout if S.gates is not None else 0
                if L.dgrad_desc.flags & H.EPI_GOUT_KEEP:   # (dY stored beside its dYpre)
                    gout *= 2
                dg_bytes = es * (Pout * L.cout + gate + Pin * L.cin * (2 if L.accum else 1) + gout +
                                 (Pin * L.resid_c if L.resid is not None else 0))
                # (a fused layer's dgrad descriptor is the fused kernel's: no separate key)
                dkey = "conv3_dw_kernel" if S.dw else self._kernel_key(L.dgrad_desc)
                info["dgrad"] = ("dgrad", L.name, dkey, 2 * macs, dg_bytes)
                info["wgrad"] = ("wgrad", L.name, self._wgrad_key(L.wgrad_desc), 2 * macs,
                                 es * (Pout * L.cout + gate + Pin * L.cin))
                if S.gate == GATE_PRELU:
                    # the separate PReLU-backward pass: dY + PReLU input read, dYpre written
                    info["prelu"] = ("prelu", L.name, "prelu_bwd_kernel", 0, 3 * es * Pout * L.cout)
                if S.dw:   # one pass: dY + gate + X read once, dX written
                    info["dw"] = ("dwgrad", L.name, self._dw_key(L.dgrad_desc, L.wgrad_desc), 4 * macs,
                                  dg_bytes + es * Pin * L.cin)
            L.info = info
        # the fused conv_0..2 launch: the three convs' algorithmic FLOPs and bytes (each
        # conv's input read once, output + PReLU input written once), as unfused
        by_name = {L.name: L for L in self.layers}
        for L in self.layers:
            if L.dense3 is not None:
                blk = L.name[:-len(".conv_0")]
                parts = [by_name[f"{blk}.conv_{k}"].info["fwd"] for k in range(3)]
                # 6th entry: the fused launch's own minimal bytes (x read once, each
                # conv's output and PReLU input written once: 32 + 3 x 32 channels)
                Ls = [by_name[f"{blk}.conv_{k}"] for k in range(3)]
                fused_min = es * self.P[L.level] * (Ls[0].cin + sum(2 * x.cout for x in Ls))
                L.info["dense3"] = ("fwd", f"{blk}.conv_0-2", self._dense3_key(L.dense3),
                                    sum(p[3] for p in parts), sum(p[4] for p in parts), fused_min)

    # ------------------------------------------------------------------
    @staticmethod
    def _launch(info, what, L, fn, *args, on=()):
        """One library launch of layer ``L`` between TRACER.start(info, *on) (``on``: the
        stream, where it is not the current one) and .stop; a non-zero return code
        raises as ``what[layer]``."""
        tr = TRACER
        tok = tr.start(info, *on) if tr is not None else None
        rc = fn(*args)
        if tok is not None:
            tr.stop(tok)
        if rc:
            H.check(rc, f"{what}[{L.name}]")

    def forward(self, xs, t: torch.Tensor | None = None) -> torch.Tensor:
        """``xs``: the Program's NCHW fp32 inputs (contiguous, on the device)."""
        lib, st = H.lib(), H.stream_ptr()
        prog = self.prog
        if len(xs) != len(prog.inputs):
            raise RuntimeError(f"expected {len(prog.inputs)} inputs, got {len(xs)}")
        for (bname, lvl, ch), x in zip(prog.inputs, xs):
            n, h, w = self.grid[lvl]
            if tuple(x.shape) != (n, ch, h, w):
                raise RuntimeError(f"input for {bname}: expected {(n, ch, h, w)}, got {tuple(x.shape)}")
        self.packs.refresh()
        x0 = xs[0]
        if prog.image_input:
            # network image input (+ the broadcast t map as channel cin_img), 8-channel rows
            B, Hh, Ww = self.B, self.H, self.W
            IN, cin = self.bufs["IN"], prog.inputs[0][2]
            if prog.time_input:
                te = t.to(device=x0.device, dtype=torch.float32).expand(B, 1, Hh, Ww)
                rc = lib.rdn_pack_input(self.code, x0.data_ptr(), B, cin, Hh, Ww, te.data_ptr(), te.stride(0),
                                        te.stride(2), te.stride(3), 1, IN.data_ptr(), 8, st)
            else:
                rc = lib.rdn_pack_input(self.code, x0.data_ptr(), B, cin, Hh, Ww, None, 0, 0, 0, 0,
                                        IN.data_ptr(), 8, st)
            H.check(rc, "pack_input")
        else:
            for (bname, lvl, ch), x in zip(prog.inputs, xs):
                ptr, ps, c0, pl = self._slice(Slice(bname))
                n, h, w = self.grid[lvl]
                H.check(lib.rdn_nchw_to_nhwc(self.code, x.data_ptr(), n, ch, h, w, ptr, ps, c0, pl, 0, st),
                        "nchw_to_nhwc")
        n, h, w = self.grid[prog.out_level]
        y = torch.empty(n, prog.out_channels, h, w, dtype=torch.float32, device=x0.device)
        last = self.layers[-1].fwd_desc
        last.out_nchw = y.data_ptr()
        last.res_nchw = x0.data_ptr() if prog.resid_input else None
        launch = self._launch
        for L in self.layers:
            if L.dense3_skip:
                continue
            if L.dense3 is not None:
                launch(L.info["dense3"], "conv_fwd", L, lib.rdn_dense3_fwd, C.byref(L.dense3), st)
            elif L.splitk:
                launch(L.info["fwd"], "conv_fwd", L, lib.rdn_conv_fwd_splitk, C.byref(L.fwd_desc), L.splitk,
                       self.ws_fwd.data_ptr(), st)
            else:
                launch(L.info["fwd"], "conv_fwd", L, lib.rdn_conv_fwd, C.byref(L.fwd_desc), st)
        return y

    def backward(self, dy: torch.Tensor, need_dx):
        """Reverse sweep; returns (input gradients (None where ``need_dx[i]`` is
        false), the flat buffer holding every weight gradient of this pass).

        Compute stream: PReLU backward (unfused layers) and the dgrad chain.  Side
        stream (when enabled): each layer's wgrad + reduce, which only wait for
        that layer's dYpre (event ``ev_ready``); a layer's unfused PReLU backward
        waits for the side stream to release its ring slot (the ``ev_done`` of
        the layer SLOTS earlier in backward order).  Gradient buffers are never
        aliased (one per activation buffer) and a slice's gradient is complete
        before its producer layer is reached, so the two chains share nothing
        else but these slots."""
        if not self.train:
            raise RuntimeError("engine was built without saved activations (no_grad forward)")
        lib, st = H.lib(), H.stream_ptr()
        prog = self.prog
        need_buf = {b: bool(nd) for (b, _, _), nd in zip(prog.inputs, need_dx)}
        gbuf = self.fp.grad_buffer()
        gbuf.zero_()
        gbase = gbuf.data_ptr()
        sync = self.fp.grad_sync
        if sync is not None:
            sync.begin(gbuf)
        dy = dy.contiguous()
        side = None if SERIAL_BWD else self.side
        if side is not None:
            main = torch.cuda.current_stream()
            sst = side.cuda_stream
            self.ev_begin.record(main)
            side.wait_event(self.ev_begin)   # gradient buffer zeroed
        else:
            main, sst = None, st
        launch = self._launch
        rev = list(reversed(self.layers))
        # split-K reduces waiting for a batched launch: the fused layers' on the compute
        # stream (consecutive ones: flushed before the next unfused layer), the others'
        # on the weight-gradient stream (this pass's: none under SERIAL_BWD)
        batch_side = side is not None and self.side_batch > 1
        cq = _ReduceQueue(st, main, None if REDUCE_BATCH else 1, sync)
        sq = _ReduceQueue(sst, side, min(self.side_batch, H.REDUCE_BATCH_MAX) if batch_side else 1, sync)

        def wait_done(Lw):
            """The compute stream waits for layer Lw's weight-gradient work (its slot
            free / an ordering edge); a still-batched layer is flushed first, so its
            event is recorded in this pass before the wait."""
            for q in (cq, sq):
                if q.holds(Lw):
                    q.flush()
            main.wait_event(Lw.bwd.ev_done)

        def wait_slot(bi):
            """Before the compute stream writes the ring slot of backward index ``bi``:
            wait for the layer that used the slot before (none in the first round)."""
            if side is not None and bi >= self.slots:
                wait_done(rev[bi - self.slots])

        for b, L in enumerate(rev):
            S, info = L.bwd, L.info
            dw, fused = S.dw, S.gate == GATE_LOADER
            if cq.layers and not dw:
                cq.flush()
            if side is not None and ORDER_EVERY and b >= ORDER_EVERY and b % ORDER_EVERY == 0 and b < self.slots:
                # ordering edge only (no buffer is reused): see ORDER_EVERY
                wait_done(rev[b - ORDER_EVERY])
            pws = S.pws
            # unfused: the PReLU-backward pass leaves its dalpha/dbias partials in
            # pws for this layer's rdn_wgrad_reduce to sum (no finalize launch);
            # gated-out: the previous layer's dgrad epilogue already did (below)
            if S.gate == GATE_PRELU:
                wait_slot(b)
                n, h, w = self.grid[S.olvl]
                pre = self.bufs[L.pre]
                dy_src = (None, 0, 0, 0, dy.data_ptr()) if L.ddst is None else (*self._slice(L.ddst), None)
                launch(info["prelu"], "prelu_bwd", L, lib.rdn_prelu_bwd, self.code, self.P[S.olvl], n, h, w, L.cout,
                       L.cout_pad, *dy_src, pre.data_ptr(), pre.shape[1], self.named[L.act + ".weight"].data_ptr(),
                       S.dyp, None, None, pws, st)
            K = S.gates   # (gate-out) this layer's dgrad epilogue writes K's dYpre / partials into K's ring slot
            if dw:
                # fused input + weight gradient on the compute stream; its slabs and
                # partials go to this ring slot's buffers, free once the side stream
                # reduced the layer that used the slot before
                wait_slot(b)
                if K is not None:
                    wait_slot(K.bwd.bidx)
                launch(info["dw"], "dgrad_wgrad", L, lib.rdn_conv_dgrad_wgrad, C.byref(L.dgrad_desc),
                       C.byref(L.wgrad_desc), st)
                if side is not None:
                    S.ev_ready.record(main)
            else:
                if side is not None:
                    S.ev_ready.record(main)
                if K is not None:
                    wait_slot(K.bwd.bidx)
                if L.src.buf not in self.pure_inputs or need_buf[L.src.buf]:
                    launch(info["dgrad"], "dgrad", L, lib.rdn_conv_fwd, C.byref(L.dgrad_desc), st)
            if not dw:
                if side is not None:
                    side.wait_event(S.ev_ready)
                if fused and batch_side and b >= self.slots and sq.holds(rev[b - self.slots]):
                    # a fused wgrad writes its dalpha/dbias partials into this ring slot from
                    # the side stream and never passes wait_done: the slot's previous layer
                    # must not still sit in the batch (its reduce reads those partials);
                    # launched first, the side stream's order does the rest
                    sq.flush()
                launch(info["wgrad"], "wgrad", L, lib.rdn_conv_wgrad, C.byref(L.wgrad_desc), sst, on=(side,))
            # stream of this layer's reduce: a fused layer's right behind its kernel on
            # the main stream (interleaved step A/B 1652 vs 1636 img/s on the side
            # stream -- at level 0 the side stream has nothing else to overlap)
            (cq if dw else sq).add(L, reduce_jobs(S, L.wgrad_desc.ws, gbase))
        cq.flush()
        sq.flush()
        if side is not None:
            self.ev_end.record(side)
            main.wait_event(self.ev_end)
        if sync is not None:
            sync.finish()
        dxs = []
        for i, ((bname, lvl, ch), nd) in enumerate(zip(prog.inputs, need_dx)):
            if not nd:
                dxs.append(None)
                continue
            n, h, w = self.grid[lvl]
            if i == 0 and prog.resid_input:   # the residual's share: d(y)/d(input 0) = 1
                dx, acc = dy.clone(), 1
            else:
                dx, acc = torch.empty(n, ch, h, w, dtype=torch.float32, device=dy.device), 0
            ptr, ps, c0, pl = self._slice(Slice("d" + bname))
            H.check(lib.rdn_nhwc_to_nchw(self.code, ptr, ps, c0, pl, n, ch, h, w, dx.data_ptr(), acc, st),
                    "nhwc_to_nchw")
            dxs.append(dx)
        return dxs, gbuf


class _Lease:
    """Held by one autograd graph while its engine's saved activations are its own."""
    __slots__ = ("__weakref__",)


def _engine_free(eng) -> bool:
    return eng.lease is None or eng.lease() is None


# engines per (shape, dtype) that grad-enabled forwards may hold at once (each holds
# its forward activations and PReLU inputs; the backward scratch is one per pool).
# Past the cap the least recently leased engine is taken over, and backward through
# the graph that held it raises (RDN_MAX_TRAIN_ENGINES; 0 = no cap)
MAX_TRAIN_ENGINES = int(os.environ.get("RDN_MAX_TRAIN_ENGINES", "16"))
_LEASE_SEQ = [0]
_WARNED_POOL: list = []


class _EngineFunction(torch.autograd.Function):
    """One engine forward as one autograd node.  Inputs: the Program's input
    tensors, then every parameter of the module, so ``torch.autograd.grad``,
    ``requires_grad_(False)``, hooks and AccumulateGrad see the weights as the
    reference's graph has them."""

    @staticmethod
    def forward(ctx, engine, lease, t, n_in, *tensors):
        ctx.engine, ctx.lease, ctx.n_in = engine, lease, n_in
        return engine.forward(tensors[:n_in], t)

    @staticmethod
    def backward(ctx, dy):
        eng, n = ctx.engine, ctx.n_in
        if eng.lease is None or eng.lease() is not ctx.lease:
            raise RuntimeError("this graph's saved RDUNet activations were released by an earlier backward "
                               "(use retain_graph=True to backward through it twice)")
        needs = ctx.needs_input_grad
        dxs, gbuf = eng.backward(dy, needs[4:4 + n])
        if not torch._C._autograd._get_current_graph_task_keep_graph():
            eng.lease = None          # activations free for the next forward
        return (None, None, None, None, *dxs, *eng.fp.grad_views(gbuf, needs[4 + n:]))


def _run(module, key_shape, xs, t, params, make_engine):
    need_grad = torch.is_grad_enabled() and (any(x.requires_grad for x in xs) or
                                             any(p.requires_grad for p in params.params))
    key = key_shape + (module.compute_dtype, bool(need_grad))
    pool = module._rdn_engines.setdefault(key, [])
    if not need_grad:
        # at most one forward-only engine per module mode (the engine plans split-K from
        # module.training at construction, _plan_splitk); the first one built stays at [0]
        training = bool(getattr(module, "training", False))
        eng = next((e for e in pool if e.module_training == training), None)
        if eng is None:
            eng = make_engine(False, None)
            pool.append(eng)
        with torch.no_grad():
            return eng.forward(xs, t)
    # a graph owns its engine's activations until its backward (or until it is
    # freed): a second forward before that backward gets a second engine, up to
    # MAX_TRAIN_ENGINES per shape; past that the least recently leased engine is
    # taken over and the graph that held it raises if it is ever backwarded
    eng = next((e for e in pool if _engine_free(e)), None)
    if eng is None:
        if MAX_TRAIN_ENGINES <= 0 or len(pool) < MAX_TRAIN_ENGINES:
            eng = make_engine(True, pool[0].scratch if pool else None)
            pool.append(eng)
        else:
            eng = min(pool, key=lambda e: e.lease_seq)
            if not _WARNED_POOL:
                _WARNED_POOL.append(True)
                warnings.warn(f"{type(module).__name__}: {MAX_TRAIN_ENGINES} grad-enabled forwards of one shape are "
                              "alive without a backward; reusing the oldest one's saved activations, so a backward "
                              "through that forward will raise (raise the cap with RDN_MAX_TRAIN_ENGINES, or run "
                              "evaluation under torch.no_grad()).", RuntimeWarning, stacklevel=3)
    lease = _Lease()
    eng.lease = weakref.ref(lease)
    _LEASE_SEQ[0] += 1
    eng.lease_seq = _LEASE_SEQ[0]
    return _EngineFunction.apply(eng, lease, t, len(xs), *xs, *params.params)


def _f32_input(x, what):
    if not isinstance(x, torch.Tensor) or x.dim() != 4:
        raise RuntimeError(f"{what}: expected a [B,C,H,W] tensor")
    return x.contiguous() if x.dtype == torch.float32 else x.float().contiguous()


def run_unet(module, x: torch.Tensor, t: torch.Tensor | None) -> torch.Tensor:
    """Entry used by ``RDUNet_T.forward`` / ``RDUNet.forward``."""
    H.require_device(x, *(p for p in [next(module.parameters())]))
    if t is not None:
        H.require_device(t)
    if x.dim() != 4 or x.size(1) != module.image_channels:
        raise RuntimeError(f"expected input [B,{module.image_channels},H,W], got {tuple(x.shape)}")
    x = _f32_input(x, type(module).__name__)
    fp = flat_params(module, x.device)
    B, Hh, Ww = x.size(0), x.size(2), x.size(3)
    need_grad = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in fp.params))
    if not need_grad and B > 1 and B * Hh * Ww > FWD_CHUNK_PIXELS:
        # a forward-only batch past 2^23 pixels (config 4: 64 x 512^2) runs as chunks of
        # images: its channel-blocked level-0 buffers would otherwise put byte offsets
        # past the 32-bit buffer-descriptor range of the fast conv kernels (conv3_ws /
        # conv3_big / conv3_dense*, which then decline the launch), and the images are
        # independent (no batch statistics), so the result is the same
        bc = max(1, FWD_CHUNK_PIXELS // (Hh * Ww))
        ys = []
        for i in range(0, B, bc):
            tc = t[i:i + bc] if (t is not None and t.dim() > 0 and t.size(0) == B) else t
            ys.append(run_unet(module, x[i:i + bc], tc))
        return torch.cat(ys, 0)
    return _run(module, (B, Hh, Ww), [x], t, fp,
                lambda train, scratch: UNetEngine(module, B, Hh, Ww, module.compute_dtype, train, scratch=scratch))


def run_block(block, xs) -> torch.Tensor:
    """Entry of the blocks' standalone ``forward`` (Unet_model.py:23-89)."""
    xs = [_f32_input(x, type(block).__name__) for x in xs]
    H.require_device(*xs, next(block.parameters()))
    bp = block_params(block, xs[0].device)
    prog = getattr(block, "_rdn_prog", None)
    if prog is None:
        prog = block._rdn_prog = block_program(block)
    lvl0 = prog.inputs[0][1]
    B, Hh, Ww = xs[0].size(0), xs[0].size(2) << lvl0, xs[0].size(3) << lvl0
    return _run(block, (B, Hh, Ww), xs, None, bp,
                lambda train, scratch: UNetEngine(block, B, Hh, Ww, block.compute_dtype, train,
                                                  prog=block_program(block), params=bp, scratch=scratch))
