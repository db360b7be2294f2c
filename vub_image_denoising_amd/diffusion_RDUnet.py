"""MI355X-native drop-in for ``diffusion_denoising/diffusion_RDUnet.py``
(and the identical definitions inlined in ``main_diffusion_RDUnet.py`` /
``diffusion_RDUnet_direct.py``).

Same names and signatures: ``DiffusionModel`` (forward_diffusion,
improved_sampling, direct_sampling, forward), ``charbonnier_loss``,
``combined_loss``, ``denormalize``, ``sample_biased``,
``train_step_checkpointed``, ``train_model_checkpointed``, ``load_checkpoint``,
``load_data(args)``, ``train(args, train_loader, val_loader)`` and the argparse
CLI (``python -m vub_image_denoising_amd.diffusion_RDUnet``).

Numerics follow the reference, including its two quirks:
``train_step_checkpointed`` zeroes gradients at its top, so with
``accumulation_steps=4`` only every 4th batch's (clipped) gradient reaches
``optimizer.step()`` (:78, :126-128); and the UNet's residual adds the
3-channel input after the output PReLU.
"""
from __future__ import annotations

import argparse
import os
import sys

import torch
import torch.distributions as dist
import torch.nn as nn
import torch.optim as optim
from torch.optim.lr_scheduler import CosineAnnealingLR

from . import functional as Fn
from .trainer import (ACCUMULATION_MODES, add_data_arguments, add_ema_arguments, ema_weights,  # noqa: F401
                      load_checkpoint, load_data, make_ema, restore_ema, save_epoch_checkpoint, save_final_ema,
                      train_epochs, use_ema)
from .Unet_model import RDUNet_T, init_weights  # noqa: F401

device = torch.device("cuda" if torch.cuda.is_available() else "cpu")


class DiffusionModel(nn.Module):
    """diffusion_RDUnet.py:27-55 (+ direct_sampling, diffusion_RDUnet_direct.py:198-201)."""

    def __init__(self, unet, timesteps=20):
        super(DiffusionModel, self).__init__()
        self.unet = unet
        self.timesteps = timesteps

    def forward_diffusion(self, clean_image, noisy_image, t):
        alpha = t / self.timesteps
        if isinstance(alpha, torch.Tensor) and alpha.numel() == clean_image.size(0) and clean_image.is_cuda:
            return Fn.interpolate(clean_image, noisy_image, alpha.reshape(-1))
        return alpha * noisy_image + (1 - alpha) * clean_image

    def improved_sampling(self, noisy_image):
        """2T UNet forwards (t = T..1): x_t <- x_t - x~(t) + x~(t-1), :38-50."""
        from .sampling import improved_sampling
        return improved_sampling(self, noisy_image)

    def direct_sampling(self, noisy_image):
        t = torch.tensor([1.0], device=noisy_image.device).unsqueeze(0).unsqueeze(2).unsqueeze(3)
        return self.unet(noisy_image, t)

    def denoise_image(self, noisy_image, **kw):
        """Whole images of any size by overlapping tiles (sampling.denoise_tiled)."""
        from .sampling import denoise_tiled
        return denoise_tiled(self, noisy_image, **kw)

    def forward(self, clean_image, noisy_image, t):
        noisy_step_image = self.forward_diffusion(clean_image, noisy_image, t)
        return self.improved_sampling(noisy_step_image)

    def train_task(self, distribution_choice='uniform', loss_weights=None):
        """What a train batch of this model is, for ``trainer`` and ``train_graph``."""
        return DiffusionTask(self, distribution_choice, loss_weights)


charbonnier_loss = Fn.charbonnier_loss
combined_loss = Fn.combined_loss


def denormalize(tensor):
    return tensor * 0.5 + 0.5


def sample_biased(num_samples, timesteps, alpha=2.0):
    """Beta(alpha, 1) * timesteps, drawn on the CPU as the reference does (:71-73)."""
    beta_dist = dist.Beta(alpha, 1.0)
    return beta_dist.sample((num_samples,)) * timesteps


def _draw_t(batch_size, timesteps, distribution_choice, dev):
    if distribution_choice == 'biased':
        return sample_biased(batch_size, timesteps).to(dev)
    return torch.randint(0, timesteps + 1, (batch_size,), device=dev).float()


def _forward_loss(model, clean_images, noisy_images, distribution_choice, t, loss_weights=None):
    B = clean_images.size(0)
    T = model.timesteps
    if t is None:
        t = _draw_t(B, T, distribution_choice, clean_images.device)
    t_normalized = t.to(device=clean_images.device, dtype=torch.float32) / T           # :90
    interpolated = Fn.interpolate(clean_images, noisy_images, t_normalized)            # :99-100
    t_tensor = t_normalized.view(B, 1, 1, 1).expand(-1, 1, clean_images.size(2), clean_images.size(3))  # :93
    denoised = model.unet(interpolated, t_tensor)                                      # :106
    return combined_loss(denoised, clean_images, *Fn.loss_weights_or_default(loss_weights))   # :109


def train_step_device(model, clean_images, noisy_images, optimizer, distribution_choice='uniform',
                      clip_value=0.1, t=None, zero_grad=True, clip=True, loss_weights=None):
    """The body of train_step_checkpointed without the host sync: returns the
    loss as a device tensor.  ``t`` (integer steps, [B]) overrides the draw.
    ``zero_grad=False, clip=False`` accumulates into the existing gradients
    (the fixed accumulation mode of trainer.train_epochs).  ``loss_weights``: the
    ``(mse, charbonnier, ssim)`` weights of ``combined_loss``, None for the
    reference's (0, 1, 0)."""
    model.train()
    if zero_grad:
        optimizer.zero_grad()
    loss = _forward_loss(model, clean_images, noisy_images, distribution_choice, t, loss_weights)
    # data-parallel: the clip right after the backward also applies the 1/world
    # average of the all-reduced gradient (one pass instead of two, ddp.py)
    # -- only when the gradients are this backward's alone (zero_grad): accumulated
    # ones already hold averaged sums from earlier calls, which must not be scaled again
    fp = getattr(model.unet, "_rdn_flat", None)
    sync = getattr(fp, "grad_sync", None) if clip else None
    fold = sync is not None and sync.world > 1 and zero_grad
    if fold:
        sync.defer_average = True
    try:
        loss.backward()                                                                # :110
    finally:
        if fold:
            sync.defer_average = False
    if clip:
        pre = sync.take_pending() if fold else None
        params = list(model.parameters())
        flat = Fn.find_flat(params) if pre is not None else None
        if pre is not None and flat is None:
            sync._average()   # gradients not the flat views: average them first
            pre = None
        if pre is not None:
            Fn.clip_grad_norm_flat(flat, clip_value, pre_scale=pre, want_norm=False)   # :113
        else:
            Fn.clip_grad_norm_(params, clip_value, want_norm=False)                    # :113
    return loss


def forward_step_device(model, clean_images, noisy_images, distribution_choice='uniform', t=None, need_loss=True,
                        loss_weights=None):
    """A train step whose gradient the reference throws away (diffusion_RDUnet.py:78:
    the next step's zero_grad): the same timestep draw (so the RNG streams stay the
    reference's) and, when the loss is logged, the same forward + loss without
    saved activations; no backward, no clip, no gradient all-reduce."""
    if not need_loss:
        if t is None:
            _draw_t(clean_images.size(0), model.timesteps, distribution_choice, clean_images.device)
        return None
    model.train()
    with torch.no_grad():
        return _forward_loss(model, clean_images, noisy_images, distribution_choice, t, loss_weights)


def train_step_checkpointed(model, clean_images, noisy_images, optimizer, accumulation_steps,
                            distribution_choice='uniform', clip_value=0.1, *, t=None, loss_weights=None):
    """diffusion_RDUnet.py:76-115 (returns ``loss.item()`` like the reference).
    ``main_diffusion_RDUnet.py``'s variant has no ``distribution_choice``; passing
    the clip value positionally there works the same (a float is taken as the
    clip value)."""
    if isinstance(distribution_choice, (int, float)) and not isinstance(distribution_choice, bool):
        clip_value, distribution_choice = float(distribution_choice), 'uniform'
    loss = train_step_device(model, clean_images, noisy_images, optimizer, distribution_choice, clip_value, t=t,
                             loss_weights=loss_weights)
    return loss.item()


def train_model_checkpointed(model, train_loader, val_loader, optimizer, scheduler, writer, output_dir,
                             distribution_choice='uniform', num_epochs=10, start_epoch=0, accumulation_steps=4,
                             clip_value=1.0, log_every=1, accumulation='reference', loss_weights=None, *,
                             captured=False, ema=None):
    """diffusion_RDUnet.py:117-178: ``run_epochs`` with the one-batch improved_sampling
    validation (``log_every``, ``accumulation``, ``captured`` and ``ema``: see
    trainer.train_epochs; ``loss_weights``: the loss mix of the train steps and the validation)."""
    run_epochs(model, train_loader, val_loader, optimizer, scheduler, writer, output_dir, distribution_choice,
               num_epochs, start_epoch, accumulation_steps, clip_value, log_every,
               sample=lambda m, x: m.improved_sampling(x), accumulation=accumulation, loss_weights=loss_weights,
               captured=captured, ema=ema)


CHECKPOINT_NAME = "diffusion_RDUNet_model_checkpointed_epoch_{epoch}.pth"


class DiffusionTask:
    """What a batch of the diffusion trainers is (see ``trainer``): this module's
    ``train_step_device`` / ``forward_step_device`` with ``distribution_choice`` and
    ``loss_weights``; validation samples one batch with ``sample(model, noisy)``."""
    takes_t = True

    def __init__(self, model, distribution_choice='uniform', loss_weights=None, sample=None):
        self.model, self.sample = model, sample
        self.distribution_choice, self.loss_weights = distribution_choice, loss_weights
        self.host_t = distribution_choice == 'biased'   # drawn on the CPU, as the reference does (:71-73)
        self.graph_key = (distribution_choice, Fn.loss_weights_or_default(loss_weights))

    @property
    def network(self):
        return self.model.unet

    def draw_t(self, batch_size):
        return sample_biased(batch_size, self.model.timesteps)

    def train_batch(self, clean_images, noisy_images, optimizer, clip_value, zero_grad=True, clip=True, t=None):
        # the step's own clip is for this backward's gradient alone (it folds the data-parallel
        # average in); gradients accumulated over batches are clipped as a whole afterwards
        loss = train_step_device(self.model, clean_images, noisy_images, optimizer, self.distribution_choice,
                                 clip_value, t=t, zero_grad=zero_grad, clip=clip and zero_grad,
                                 loss_weights=self.loss_weights)
        if clip and not zero_grad:
            Fn.clip_grad_norm_(self.model.parameters(), clip_value)
        return loss

    def loss_batch(self, clean_images, noisy_images, need_loss=True, t=None):
        return forward_step_device(self.model, clean_images, noisy_images, self.distribution_choice, t=t,
                                   need_loss=need_loss, loss_weights=self.loss_weights)

    def validation_loss(self, clean_images, noisy_images):
        with torch.no_grad():
            return combined_loss(self.sample(self.model, noisy_images), clean_images,
                                 *Fn.loss_weights_or_default(self.loss_weights))


def run_epochs(model, train_loader, val_loader, optimizer, scheduler, writer, output_dir, distribution_choice,
               num_epochs, start_epoch, accumulation_steps, clip_value, log_every, sample, accumulation='reference',
               skip_discarded=True, loss_weights=None, captured=False, ema=None):
    """The epoch loop shared by the three reference trainers (diffusion_RDUnet.py:117-178,
    main_diffusion_RDUnet.py:275-336, diffusion_RDUnet_direct.py:266-327), which differ only in
    the validation sampler ``sample`` and the checkpoint directory: ``trainer.train_epochs`` on
    a ``DiffusionTask`` (see there for ``accumulation``, ``skip_discarded``, ``captured`` and
    ``ema``).  ``loss_weights``: the ``(mse, charbonnier, ssim)`` weights of the train and
    validation loss, None for the reference's (0, 1, 0)."""
    train_epochs(DiffusionTask(model, distribution_choice, loss_weights, sample), train_loader, val_loader, optimizer,
                 scheduler, writer, os.path.join(output_dir, CHECKPOINT_NAME), num_epochs, start_epoch,
                 accumulation_steps, clip_value, log_every, accumulation, skip_discarded, captured, ema)


def make_optimizer(args, params, fused=False):
    """diffusion_RDUnet.py:264-276 choices; ``fused=True``: the one-launch optimizers of
    ``optim`` with the same hyperparameters (what ``captured=True`` training needs)."""
    if fused:
        from . import optim as fused_optim
        adam, adamw, adadelta = fused_optim.FusedAdam, fused_optim.FusedAdamW, fused_optim.FusedAdadelta
    else:
        adam, adamw, adadelta = optim.Adam, optim.AdamW, optim.Adadelta
    if args.optimizer_choice == 'adam':
        optimizer = adam(params, lr=args.lr, betas=(0.9, 0.999))
        scheduler = CosineAnnealingLR(optimizer, T_max=10)
    elif args.optimizer_choice == 'adamw':
        optimizer = adamw(params, lr=args.lr, weight_decay=args.weight_decay)
        scheduler = optim.lr_scheduler.StepLR(optimizer, step_size=3, gamma=0.5)
    else:
        optimizer = adadelta(params, lr=args.lr)
        scheduler = optim.lr_scheduler.StepLR(optimizer, step_size=3, gamma=0.5)
    return optimizer, scheduler


def train(args, train_loader=None, val_loader=None):
    """diffusion_RDUnet.py:230-288 (TensorBoard if importable)."""
    try:
        from torch.utils.tensorboard import SummaryWriter
        writer = SummaryWriter(log_dir=os.path.join("runs", "diffusion_checkpointed", os.path.basename(args.output_dir)))
    except Exception:  # tensorboard is optional
        writer = None
    if train_loader is None or val_loader is None:
        train_loader, val_loader = load_data(args)
    unet = RDUNet_T(base_filters=args.base_filters).to(device)
    unet.set_compute_dtype(getattr(args, "dtype", "fp32"))
    model = DiffusionModel(unet, timesteps=args.timesteps).to(device)
    unet.apply(init_weights())
    captured = getattr(args, "step_mode", "eager") == 'graph'
    optimizer, scheduler = make_optimizer(args, model.parameters(), fused=captured)
    ema = make_ema(args, model)
    start_epoch = load_checkpoint(model, optimizer, scheduler, args.checkpoint_path, ema=ema)
    train_model_checkpointed(model, train_loader, val_loader, optimizer, scheduler, writer, args.output_dir,
                             args.distribution_choice, num_epochs=args.num_epochs, start_epoch=start_epoch,
                             accumulation=getattr(args, "accumulation", "reference"),
                             loss_weights=(getattr(args, "mse_weight", 0.0), getattr(args, "charbonnier_weight", 1.0),
                                           getattr(args, "ssim_weight", 0.0)), captured=captured, ema=ema)
    final_model_path = os.path.join(args.output_dir, "diffusion_RDUNet_model_checkpointed_final.pth")
    torch.save(model.state_dict(), final_model_path)
    print(f"Final model saved at {final_model_path}")
    if ema is not None:
        save_final_ema(model, ema, os.path.join(args.output_dir, "diffusion_RDUNet_model_checkpointed_final_ema.pth"))
    if writer is not None:
        writer.close()


def build_parser():
    """diffusion_RDUnet.py:293-309, plus --dtype, --accumulation, the three
    weights of ``combined_loss`` (:60), --step_mode, --data_pipeline and the EMA flags."""
    parser = argparse.ArgumentParser(description="Train a diffusion model with optional optimizer and scheduler choice.")
    add_data_arguments(parser)
    parser.add_argument('--base_filters', type=int, default=32)
    parser.add_argument('--timesteps', type=int, default=20)
    parser.add_argument('--optimizer_choice', type=str, default='adamw', choices=['adam', 'adamw', 'adadelta'])
    parser.add_argument('--scheduler_choice', type=str, default='step', choices=['cosine', 'step'])
    parser.add_argument('--lr', type=float, default=1e-4)
    parser.add_argument('--weight_decay', type=float, default=1e-4)
    parser.add_argument('--distribution_choice', type=str, default='uniform', choices=['uniform', 'biased'])
    parser.add_argument('--accumulation', type=str, default='reference', choices=list(ACCUMULATION_MODES),
                        help="reference: only every 4th batch's gradient is applied (the reference's rule, "
                             "without the discarded backward passes); fixed: accumulate 4 batches")
    parser.add_argument('--mse_weight', type=float, default=0.0)
    parser.add_argument('--charbonnier_weight', type=float, default=1.0)
    parser.add_argument('--ssim_weight', type=float, default=0.0, help="weight of 1 - SSIM (gaussian 11x11)")
    add_ema_arguments(parser)
    return parser


if __name__ == "__main__":
    train(build_parser().parse_args())
    sys.exit(0)
