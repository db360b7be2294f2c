"""Drop-in for the definitions ``diffusion_denoising/main_diffusion_RDUnet.py``
declares inline (:24-352): the network classes, ``DiffusionModel``, the losses,
``denormalize``, and this script's own trainer signatures, which differ from
``diffusion_RDUnet.py``'s:

* ``train_step_checkpointed(model, clean, noisy, optimizer, accumulation_steps,
  clip_value=0.1)`` — uniform t only (:237-273);
* ``train_model_checkpointed(model, train_loader, val_loader, optimizer, scheduler,
  writer, num_epochs=10, start_epoch=0, accumulation_steps=4, clip_value=1.0)`` —
  improved_sampling validation, checkpoints under ``checkpoints/`` (:275-336);
* ``load_checkpoint(model, optimizer, scheduler, checkpoint_path)`` (:339-352) — the
  one loader of ``trainer``: unlike the reference's it also takes a path of None (no
  checkpoint: epoch 0) and a scheduler, or a checkpoint's scheduler state, of None.

The script's module-level model / Adam(2e-4) / CosineAnnealingLR(T_max=10)
(:228-231) stay in the user's script; ``make_training_objects`` builds the same
four objects for callers that want them.
"""
from __future__ import annotations

import torch.optim as optim
from torch.optim.lr_scheduler import CosineAnnealingLR

from .diffusion_RDUnet import (DiffusionModel, add_ema_arguments, charbonnier_loss, combined_loss,  # noqa: F401
                               denormalize, device, load_checkpoint, make_ema, restore_ema, run_epochs,
                               train_step_device)
from .Unet_model import (DenoisingBlock, DownsampleBlock, InputBlock, OutputBlock, RDUNet_T,  # noqa: F401
                         UpsampleBlock, init_weights)

CHECKPOINT_DIR = "checkpoints"


def make_training_objects(base_filters=32, lr=2e-4, dev=None, model_cls=None, fused=False):
    """main_diffusion_RDUnet.py:228-231: RDUNet_T(32), DiffusionModel, Adam(lr, (0.9, 0.999)),
    CosineAnnealingLR(T_max=10).  ``fused=True``: optim.FusedAdam with the same
    hyperparameters (for ``train_model_checkpointed(..., captured=True)``)."""
    dev = dev or device
    unet = RDUNet_T(base_filters=base_filters).to(dev)
    model = (model_cls or DiffusionModel)(unet).to(dev)
    if fused:
        from .optim import FusedAdam
        optimizer = FusedAdam(model.parameters(), lr=lr, betas=(0.9, 0.999))
    else:
        optimizer = optim.Adam(model.parameters(), lr=lr, betas=(0.9, 0.999))
    scheduler = CosineAnnealingLR(optimizer, T_max=10)
    return unet, model, optimizer, scheduler


def build_parser():
    """The reference script takes no flags (its settings are module-level constants); the
    only ones here are this package's own: ``--ema_decay`` / ``--ema_warmup``, which
    ``make_ema(args, model)`` turns into the ``ema`` of ``train_model_checkpointed``."""
    import argparse
    return add_ema_arguments(argparse.ArgumentParser(description="EMA options of the main_diffusion_RDUnet trainer."))


def train_step_checkpointed(model, clean_images, noisy_images, optimizer, accumulation_steps, clip_value=0.1, *,
                            loss_weights=None):
    """main_diffusion_RDUnet.py:237-273 (uniform t; returns ``loss.item()``)."""
    return train_step_device(model, clean_images, noisy_images, optimizer, 'uniform', clip_value,
                             loss_weights=loss_weights).item()


def _sample(model, x):
    return model.improved_sampling(x)


def train_model_checkpointed(model, train_loader, val_loader, optimizer, scheduler, writer, num_epochs=10,
                             start_epoch=0, accumulation_steps=4, clip_value=1.0, *, accumulation='reference',
                             loss_weights=None, captured=False, ema=None):
    """main_diffusion_RDUnet.py:275-336 (``captured``, ``ema``: see trainer.train_epochs)."""
    run_epochs(model, train_loader, val_loader, optimizer, scheduler, writer, CHECKPOINT_DIR, 'uniform', num_epochs,
               start_epoch, accumulation_steps, clip_value, 1, sample=_sample, accumulation=accumulation,
               loss_weights=loss_weights, captured=captured, ema=ema)
