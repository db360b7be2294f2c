"""MI355X-native drop-in for ``UNet/RDUNet_model.py``: the plain RDUNet baseline
the reference compares its diffusion model against, network and trainer.

``RDUNet(channels=3, base_filters=64)`` (RDUNet_model.py:117-186): the same
residual-dense UNet without the timestep channel; ``forward(inputs)`` returns
``output_block(...) + inputs``.

The trainer (RDUNet_model.py:189-261): ``train_step`` / ``train_model`` with the
reference's rule -- ``loss = L1(model(noisy), clean)`` (mean, not divided by
``accumulation_steps``), gradients accumulated over ``accumulation_steps`` batches, and
on the last of them ``clip_grad_norm_(clip_value)``, ``optimizer.step()``,
``zero_grad()`` -- AdamW with StepLR, and ``python -m vub_image_denoising_amd.RDUNet_model``
as the command line.  The loss is ``functional.l1_loss`` (two launches), the backward
the fused one of ``engine``, and ``captured=True`` replays every batch as one hipGraph
(``train_graph``, kinds ``'accum'`` / ``'accum_step'``).  The reference module builds
``RDUNet(128)``, AdamW and StepLR when it is imported; here nothing happens at import,
``train(args)`` builds them.

Decided here, because the survey of the reference does not record
them: the checkpoint file names (``RDUNet_model_epoch_{n}.pth``,
``RDUNet_model_final.pth``), StepLR's ``step_size=3, gamma=0.5`` and the ``--lr`` /
``--weight_decay`` defaults (those of the diffusion command line's AdamW choice), the
validation rule (the L1 loss of the first validation batch, in eval mode under
``no_grad``), the ``Loss/train`` / ``Loss/validation`` tags and the checkpoint dict (those
of the diffusion trainers), and ``train_step``'s ``zero_grad`` / ``clip`` switches.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch

from . import functional as Fn
from . import trainer
from .engine import run_unet
from .trainer import (add_data_arguments, add_ema_arguments, load_data, make_ema, restore_ema,  # noqa: F401
                      save_epoch_checkpoint, save_final_ema, train_epochs, use_ema)
from .Unet_model import (DenoisingBlock, DownsampleBlock, InputBlock, OutputBlock,  # noqa: F401
                         UpsampleBlock, _RDUNetBase, init_weights)


class RDUNet(_RDUNetBase):
    def __init__(self, channels=3, base_filters=64):
        super().__init__()
        if not 1 <= channels <= 8:
            raise ValueError("RDUNet supports 1..8 image channels")
        self._build(channels, base_filters, channels)
        self.time_conditioned = False
        self.image_channels = channels

    def forward(self, inputs):
        return run_unet(self, inputs, None)

    def train_task(self, distribution_choice='uniform', loss_weights=None):
        """What a train batch of this model is, for ``trainer`` and ``train_graph``: L1, no t
        (``distribution_choice`` has nothing to choose)."""
        if loss_weights is not None:
            raise ValueError("a bare RDUNet trains on L1: no loss weights")
        return L1Task(self)


def denormalize(tensor):
    """RDUNet_model.py:197-198."""
    return tensor * 0.5 + 0.5


def train_step_device(model, noisy, clean, optimizer, clip_value=1.0, zero_grad=False, clip=False):
    """One batch of the baseline's training loop (RDUNet_model.py:201-215) without the
    host sync: ``L1(model(noisy), clean).backward()``, the loss returned as a device
    tensor.  The gradients add onto the existing ones unless ``zero_grad``;
    ``clip=True`` (the last batch of an accumulation group) clips their global norm to
    ``clip_value`` afterwards.  ``optimizer.step()`` is the caller's."""
    model.train()
    if zero_grad:
        optimizer.zero_grad()
    loss = Fn.l1_loss(model(noisy), clean)
    loss.backward()
    if clip:
        Fn.clip_grad_norm_(list(model.parameters()), clip_value, want_norm=False)
    return loss


def train_step(model, noisy, clean, optimizer, clip_value=1.0, zero_grad=False, clip=False):
    """``train_step_device`` returning ``loss.item()`` as the reference's step does."""
    return train_step_device(model, noisy, clean, optimizer, clip_value, zero_grad, clip).item()


def forward_loss_device(model, noisy, clean):
    """``L1(model(noisy), clean)`` under ``no_grad`` (the validation loss; the
    ``'loss'`` kind of a captured baseline step), in the model's current mode."""
    with torch.no_grad():
        return Fn.l1_loss(model(noisy), clean)


CHECKPOINT_NAME = "RDUNet_model_epoch_{epoch}.pth"
FINAL_NAME = "RDUNet_model_final.pth"
FINAL_EMA_NAME = "RDUNet_model_final_ema.pth"


class L1Task:
    """What a batch of the baseline's trainer is (see ``trainer``): ``L1(model(noisy), clean)``,
    no t; the steps are this module's ``train_step_device`` / ``forward_loss_device``."""
    takes_t = host_t = False
    graph_key = ('l1',)

    def __init__(self, model):
        self.model = self.network = model

    def train_batch(self, clean, noisy, optimizer, clip_value, zero_grad=True, clip=True, t=None):
        return train_step_device(self.model, noisy, clean, optimizer, clip_value, zero_grad=zero_grad, clip=clip)

    def loss_batch(self, clean, noisy, need_loss=True, t=None):
        self.model.train()
        return forward_loss_device(self.model, noisy, clean)

    def validation_loss(self, clean, noisy):
        return forward_loss_device(self.model, noisy, clean)


def train_model(model, train_loader, val_loader, optimizer, scheduler, writer, output_dir, num_epochs,
                start_epoch=0, accumulation_steps=4, clip_value=1.0, log_every=1, captured=False, ema=None):
    """RDUNet_model.py:201-261: ``trainer.train_epochs`` on an ``L1Task`` with the fixed
    accumulation rule (see there for ``log_every``, ``captured`` and ``ema``) -- each batch adds
    its L1 gradient, every ``accumulation_steps``-th batch clips, steps and zeroes.  The
    checkpoint dicts' parameter names are the network's own, without a ``unet.`` prefix; a
    captured run replays the ``'accum'`` / ``'accum_step'`` kinds of ``train_graph`` and needs
    ``optim.FusedAdamW``."""
    train_epochs(L1Task(model), train_loader, val_loader, optimizer, scheduler, writer,
                 os.path.join(output_dir, CHECKPOINT_NAME), num_epochs, start_epoch, accumulation_steps, clip_value,
                 log_every, accumulation='fixed', captured=captured, ema=ema)


def load_checkpoint(model, optimizer, scheduler, checkpoint_path, *, ema=None):
    """Resume from a per-epoch checkpoint dict of ``train_model`` (returns its epoch), or
    load the bare ``state_dict`` that ``train`` writes at the end (weights only: the
    optimizer and scheduler stay as built, returns 0); the optimizer may be None.  ``ema``
    (optim.EMA) is restored from the checkpoint's ``ema_state_dict``, or restarted from the
    loaded weights where there is none (trainer.restore_ema)."""
    return trainer.load_checkpoint(model, optimizer, scheduler, checkpoint_path, ema=ema, bare_weights=True)


def make_optimizer(args, params, fused=False):
    """AdamW + StepLR, the pair the reference builds at module level; ``fused=True``:
    ``optim.FusedAdamW`` with the same hyperparameters (what a captured step needs)."""
    if fused:
        from .optim import FusedAdamW as adamw
    else:
        adamw = torch.optim.AdamW
    optimizer = adamw(params, lr=args.lr, weight_decay=args.weight_decay)
    return optimizer, torch.optim.lr_scheduler.StepLR(optimizer, step_size=3, gamma=0.5)


def train(args, train_loader=None, val_loader=None):
    """Build ``RDUNet(base_filters=args.base_filters)``, AdamW and StepLR, resume from
    ``args.checkpoint_path`` and run ``train_model`` (TensorBoard if importable)."""
    try:
        from torch.utils.tensorboard import SummaryWriter
        writer = SummaryWriter(log_dir=os.path.join("runs", "RDUNet", os.path.basename(args.output_dir)))
    except Exception:  # tensorboard is optional
        writer = None
    if train_loader is None or val_loader is None:
        train_loader, val_loader = load_data(args)
    dev = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    model = RDUNet(base_filters=args.base_filters).to(dev)
    model.set_compute_dtype(args.dtype)
    model.apply(init_weights())
    captured = args.step_mode == 'graph'
    optimizer, scheduler = make_optimizer(args, model.parameters(), fused=captured)
    ema = make_ema(args, model)
    start_epoch = load_checkpoint(model, optimizer, scheduler, args.checkpoint_path, ema=ema)
    train_model(model, train_loader, val_loader, optimizer, scheduler, writer, args.output_dir, args.num_epochs,
                start_epoch=start_epoch, accumulation_steps=args.accumulation_steps, captured=captured, ema=ema)
    final_model_path = os.path.join(args.output_dir, FINAL_NAME)
    os.makedirs(args.output_dir, exist_ok=True)
    torch.save(model.state_dict(), final_model_path)
    print(f"Final model saved at {final_model_path}")
    if ema is not None:
        save_final_ema(model, ema, os.path.join(args.output_dir, FINAL_EMA_NAME))
    if writer is not None:
        writer.close()


def build_parser():
    """The baseline's own command line: the dataset flags of the diffusion one, the
    reference's width of 128, AdamW's ``--lr`` / ``--weight_decay`` and the
    accumulation group size."""
    parser = argparse.ArgumentParser(description="Train the plain RDUNet baseline (L1 loss, AdamW, StepLR).")
    add_data_arguments(parser)
    parser.add_argument('--base_filters', type=int, default=128)
    parser.add_argument('--lr', type=float, default=1e-4)
    parser.add_argument('--weight_decay', type=float, default=1e-4)
    parser.add_argument('--accumulation_steps', type=int, default=4)
    add_ema_arguments(parser)
    return parser


if __name__ == "__main__":
    train(build_parser().parse_args())
    sys.exit(0)
