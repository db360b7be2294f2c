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
from .engine import run_unet
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


def train_model(model, train_loader, val_loader, optimizer, scheduler, writer, output_dir, num_epochs,
                start_epoch=0, accumulation_steps=4, clip_value=1.0, log_every=1, captured=False, ema=None):
    """RDUNet_model.py:201-261: every epoch starts with ``zero_grad`` (a partial
    accumulation group left by the previous epoch is dropped), each batch adds its L1
    gradient, every ``accumulation_steps``-th batch clips, steps and zeroes; then one
    validation batch (``Loss/validation``), ``scheduler.step()`` and a checkpoint dict
    (``epoch``, ``model_state_dict``, ``optimizer_state_dict``, ``scheduler_state_dict``;
    the parameter names are the network's own, without a ``unet.`` prefix).
    ``log_every`` > 1 rate-limits the per-batch ``loss.item()`` host sync.
    ``captured=True`` replays each batch as one hipGraph (the ``'accum'`` and
    ``'accum_step'`` kinds of ``train_graph``, kept on the model) and needs a fused
    optimizer (``optim.FusedAdamW``): parameters, optimizer state and logged losses are
    the eager loop's bit for bit.  ``ema`` (optim.EMA): an average of the weights kept with
    every update, as in diffusion_RDUnet.run_epochs -- ``Loss/validation_ema`` is the same
    validation batch under the averaged weights, the checkpoints gain ``ema_state_dict``."""
    from .diffusion_RDUnet import save_epoch_checkpoint, use_ema
    graphs = None
    if captured:
        from . import train_graph
        graphs = train_graph.trainer_graphs(model, optimizer, clip_value=clip_value)
    ema_update = use_ema(model, optimizer, ema)
    dev = next(model.parameters()).device
    for epoch in range(start_epoch, num_epochs):
        model.train()
        optimizer.zero_grad()
        if captured:
            train_graph.clear_accumulator(model)
        n_batches = len(train_loader) if hasattr(train_loader, "__len__") else 0
        for batch_idx, (noisy, clean) in enumerate(train_loader):
            noisy, clean = noisy.to(dev), clean.to(dev)
            step_now = (batch_idx + 1) % accumulation_steps == 0
            if captured:
                loss_t = graphs(clean, noisy, kind='accum_step' if step_now else 'accum')
            else:
                loss_t = train_step_device(model, noisy, clean, optimizer, clip_value, clip=step_now)
                if step_now:
                    if ema_update:
                        ema.bind()      # (first step: the average starts as the weights before it)
                    optimizer.step()
                    if ema_update:
                        ema.update()
                    optimizer.zero_grad()
            if batch_idx % log_every == 0:
                loss = loss_t.item()
                print(f"Epoch [{epoch + 1}/{num_epochs}], Batch [{batch_idx + 1}/{n_batches}], Loss: {loss:.4f}")
                if writer is not None:
                    writer.add_scalar('Loss/train', loss, epoch * n_batches + batch_idx)
        model.eval()
        validation_loss = ema_loss = float("nan")
        if val_loader is not None:
            val_noisy, val_clean = next(iter(val_loader))
            val_noisy, val_clean = val_noisy.to(dev), val_clean.to(dev)
            validation_loss = forward_loss_device(model, val_noisy, val_clean).item()
            if ema is not None:
                with ema.applied():
                    ema_loss = forward_loss_device(model, val_noisy, val_clean).item()
        print(f"Epoch [{epoch + 1}/{num_epochs}], Validation Loss: {validation_loss:.4f}")
        if ema is not None:
            print(f"Epoch [{epoch + 1}/{num_epochs}], Validation Loss (EMA weights): {ema_loss:.4f}")
        if writer is not None:
            writer.add_scalar('Loss/validation', validation_loss, epoch + 1)
            if ema is not None:
                writer.add_scalar('Loss/validation_ema', ema_loss, epoch + 1)
            if hasattr(writer, "flush"):
                writer.flush()
        if scheduler is not None:
            scheduler.step()
        save_epoch_checkpoint(model, optimizer, scheduler, epoch + 1,
                              os.path.join(output_dir, CHECKPOINT_NAME.format(epoch=epoch + 1)), ema=ema)


def load_checkpoint(model, optimizer, scheduler, checkpoint_path, *, ema=None):
    """Resume from a per-epoch checkpoint dict of ``train_model`` (returns its epoch), or
    load the bare ``state_dict`` that ``train`` writes at the end (weights only: the
    optimizer and scheduler stay as built, returns 0).  ``ema`` (optim.EMA) is restored
    from the checkpoint's ``ema_state_dict``, or restarted from the loaded weights where
    there is none (diffusion_RDUnet.restore_ema)."""
    from .diffusion_RDUnet import restore_ema
    if (checkpoint_path is not None) and os.path.isfile(checkpoint_path):
        print(f"Loading checkpoint '{checkpoint_path}'")
        dev = next(model.parameters()).device
        checkpoint = torch.load(checkpoint_path, map_location=dev, weights_only=True)
        if 'model_state_dict' not in checkpoint:
            model.load_state_dict(checkpoint)
            restore_ema(ema, None, model)
            print(f"Loaded weights '{checkpoint_path}'")
            return 0
        model.load_state_dict(checkpoint['model_state_dict'])
        if optimizer is not None:
            optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
        if scheduler is not None and checkpoint.get('scheduler_state_dict') is not None:
            scheduler.load_state_dict(checkpoint['scheduler_state_dict'])
        restore_ema(ema, checkpoint, model)
        start_epoch = checkpoint['epoch']
        print(f"Loaded checkpoint '{checkpoint_path}' (epoch {start_epoch})")
        return start_epoch
    print(f"No checkpoint found at '{checkpoint_path}'")
    return 0


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
    from .diffusion_RDUnet import load_data, make_ema, save_final_ema
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
    parser.add_argument('--dataset_choice', type=str, default='SIDD', choices=['DIV2K', 'SIDD'])
    parser.add_argument('--checkpoint_path', type=str, default=None)
    parser.add_argument('--num_epochs', type=int, default=300)
    parser.add_argument('--batch_size', type=int, default=8)
    parser.add_argument('--num_workers', type=int, default=8)
    parser.add_argument('--validation_split', type=float, default=0.2)
    parser.add_argument('--augment', action='store_false')
    parser.add_argument('--dataset_percentage', type=float, default=0.1)
    parser.add_argument('--base_filters', type=int, default=128)
    parser.add_argument('--output_dir', type=str, default='checkpoints')
    parser.add_argument('--lr', type=float, default=1e-4)
    parser.add_argument('--weight_decay', type=float, default=1e-4)
    parser.add_argument('--accumulation_steps', type=int, default=4)
    parser.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--step_mode', type=str, default='eager', choices=['eager', 'graph'],
                        help="graph: fused AdamW, every batch replayed as one captured hipGraph")
    parser.add_argument('--data_pipeline', type=str, default='pil', choices=['pil', 'gpu'],
                        help="gpu: patches cut and augmented on the device (synth loaders), no worker processes")
    from .diffusion_RDUnet import add_ema_arguments
    add_ema_arguments(parser)
    return parser


if __name__ == "__main__":
    train(build_parser().parse_args())
    sys.exit(0)
