"""What the trainers share and no model decides: the epoch loop, the EMA plumbing, the
per-epoch checkpoint and its loader, the dataset dispatch and the command-line flags every
trainer declares.

A trainer hands the loop a *task* -- a plain object of its model's module
(``diffusion_RDUnet.DiffusionTask``, ``RDUNet_model.L1Task``) that says what a batch is:

* ``model``, ``network`` (the fused network inside it);
* ``train_batch(clean, noisy, optimizer, clip_value, zero_grad=True, clip=True, t=None)``:
  forward, loss and backward of one batch, the loss as a device tensor;
* ``loss_batch(clean, noisy, need_loss=True, t=None)``: a train-mode batch without a gradient;
* ``validation_loss(clean, noisy)``: the loss of one validation batch;
* ``takes_t``, ``host_t``, ``draw_t(batch_size)``, ``graph_key``: what ``train_graph`` asks.

This module imports neither trainer module; both import it, and re-export its names.
"""
from __future__ import annotations

import argparse
import os

import torch

from . import train_graph
from .optim import EMA

ACCUMULATION_MODES = ("reference", "fixed")


def use_ema(model, optimizer, ema):
    """How a trainer keeps ``ema`` (optim.EMA, or None): a fused optimizer takes it into
    its own launch (``attach_ema``: nothing more to do, eager or captured) and False is
    returned; beside a torch optimizer the trainer calls ``ema.bind()`` before and
    ``ema.update()`` after every ``optimizer.step()`` and True is returned.  The names of
    ``ema.state_dict()['shadow']`` become those of ``model.state_dict()``."""
    if ema is None:
        return False
    ema.use_names_of(model)
    if hasattr(optimizer, "attach_ema"):
        optimizer.attach_ema(ema)
        return False
    return True


def train_epochs(task, train_loader, val_loader, optimizer, scheduler, writer, checkpoint_name, num_epochs,
                 start_epoch=0, accumulation_steps=4, clip_value=1.0, log_every=1, accumulation='reference',
                 skip_discarded=True, captured=False, ema=None):
    """The epoch loop of every trainer (diffusion_RDUnet.py:117-178, main_diffusion_RDUnet.py:275-336,
    diffusion_RDUnet_direct.py:266-327, UNet/RDUNet_model.py:201-261): every epoch starts with
    ``zero_grad`` (a partial accumulation group left by the previous epoch is dropped), then the
    batches, one validation batch, ``scheduler.step()`` and a checkpoint dict written to
    ``checkpoint_name.format(epoch=...)``.  ``log_every`` > 1 rate-limits the per-batch
    ``loss.item()`` host sync.

    accumulation='reference' keeps the diffusion reference's update rule:
    train_step_checkpointed zeroes the gradients at its top (:78), so only the
    clipped gradient of every ``accumulation_steps``-th batch reaches
    ``optimizer.step()`` (:126-128).  The other batches' backward, clip and (DDP)
    all-reduce are skipped -- their gradient is discarded by the reference -- while
    their timestep draw and, when logged, their forward loss still run, so the
    parameters are the reference's bit for bit at a third of those batches' cost.
    accumulation='fixed' accumulates the gradients of ``accumulation_steps``
    batches and clips + steps once (the rule of UNet/RDUNet_model.py:201-215, the
    baseline's only one).
    ``skip_discarded=False`` runs the discarded backward passes anyway (the
    reference's literal work; tests compare the two bit for bit).

    ``captured=True`` replays each batch as one hipGraph (train_graph.TrainStepGraphs,
    one graph per batch shape and kind, kept on the model) instead of issuing it from
    Python: in the reference mode the ``accumulation_steps``-th batch replays the whole
    step (update included), a logged other batch the forward + loss, and an unlogged one
    only draws its t; in the fixed mode the batches replay backward passes that add into
    a flat accumulator, the ``accumulation_steps``-th with clip and update.  The update
    is inside the graph, so the optimizer must be a fused one
    (``make_optimizer(..., fused=True)``); the parameters, optimizer state and logged
    losses are the eager loop's bit for bit (``skip_discarded`` has no captured form).

    ``ema`` (optim.EMA, no reference counterpart): an exponential moving average of the
    weights, updated with every optimizer update -- inside a fused optimizer's launch
    (eager or captured), by ``ema.update()`` behind a torch optimizer's step.
    ``Loss/validation`` stays the raw weights' loss; ``Loss/validation_ema`` logs the same
    batch under the averaged weights, and the checkpoints gain ``ema_state_dict``."""
    if accumulation not in ACCUMULATION_MODES:
        raise ValueError(f"accumulation must be one of {ACCUMULATION_MODES}, got {accumulation!r}")
    model = task.model
    graphs = train_graph.trainer_graphs(model, optimizer, clip_value=clip_value, task=task) if captured else None
    ema_update = use_ema(model, optimizer, ema)
    dev = next(model.parameters()).device
    for epoch in range(start_epoch, num_epochs):
        model.train()
        optimizer.zero_grad()
        if captured:
            train_graph.clear_accumulator(task.network)   # a leftover partial group is discarded
        n_batches = len(train_loader) if hasattr(train_loader, "__len__") else 0
        for batch_idx, (noisy_images, clean_images) in enumerate(train_loader):
            noisy_images, clean_images = noisy_images.to(dev), clean_images.to(dev)
            step_now = (batch_idx + 1) % accumulation_steps == 0
            log_now = batch_idx % log_every == 0
            if accumulation == 'fixed':
                if captured:
                    loss_t = graphs(clean_images, noisy_images, kind='accum_step' if step_now else 'accum')
                else:
                    loss_t = task.train_batch(clean_images, noisy_images, optimizer, clip_value, zero_grad=False,
                                              clip=step_now)
            elif step_now or not (skip_discarded or captured):
                loss_t = (graphs(clean_images, noisy_images, kind='step') if captured else
                          task.train_batch(clean_images, noisy_images, optimizer, clip_value))
            elif captured and log_now:
                loss_t = graphs(clean_images, noisy_images, kind='loss')
            else:
                loss_t = task.loss_batch(clean_images, noisy_images, need_loss=log_now)
            if step_now and not captured:
                if ema_update:
                    ema.bind()      # (first step: the average starts as the weights before it)
                optimizer.step()
                if ema_update:
                    ema.update()
                optimizer.zero_grad()
            if log_now:
                loss = loss_t.item()
                print(f"Epoch [{epoch + 1}/{num_epochs}], Batch [{batch_idx + 1}/{n_batches}], Loss: {loss:.4f}")
                if writer is not None:
                    writer.add_scalar('Loss/train', loss, epoch * n_batches + batch_idx)
        model.eval()
        validation_loss = ema_loss = float("nan")
        if val_loader is not None:
            val_noisy_images, val_clean_images = next(iter(val_loader))
            val_noisy_images, val_clean_images = val_noisy_images.to(dev), val_clean_images.to(dev)
            validation_loss = task.validation_loss(val_clean_images, val_noisy_images).item()
            if ema is not None:
                with ema.applied():
                    ema_loss = task.validation_loss(val_clean_images, val_noisy_images).item()
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
        save_epoch_checkpoint(model, optimizer, scheduler, epoch + 1, checkpoint_name.format(epoch=epoch + 1), ema=ema)


def save_epoch_checkpoint(model, optimizer, scheduler, epoch, checkpoint_path, ema=None):
    """The per-epoch checkpoint dict of the trainers (:166-174; ``epoch`` counts from 1);
    with an EMA also ``ema_state_dict`` (optim.EMA.state_dict(); no reference counterpart)."""
    os.makedirs(os.path.dirname(checkpoint_path) or ".", exist_ok=True)
    checkpoint = {
        'epoch': epoch,
        'model_state_dict': model.state_dict(),
        'optimizer_state_dict': optimizer.state_dict(),
        'scheduler_state_dict': scheduler.state_dict() if scheduler is not None else None,
    }
    if ema is not None:
        ema.use_names_of(model)
        checkpoint['ema_state_dict'] = ema.state_dict()
    torch.save(checkpoint, checkpoint_path)
    print(f"Model checkpoint saved at {checkpoint_path}")


def restore_ema(ema, checkpoint, model):
    """The EMA part of a ``load_checkpoint`` (after the weights are loaded): restore it from
    ``ema_state_dict``; a checkpoint without one restarts the average from the loaded
    weights at count 0."""
    if ema is None:
        return
    ema.use_names_of(model)
    if isinstance(checkpoint, dict) and checkpoint.get('ema_state_dict') is not None:
        ema.load_state_dict(checkpoint['ema_state_dict'])
    else:
        ema.reset_to_weights()
        print("Checkpoint has no EMA: the average restarts from the loaded weights (0 updates)")


def ema_weights(checkpoint, checkpoint_path=""):
    """The averaged weights of a per-epoch checkpoint dict (``ema_state_dict['shadow']``);
    a clear error when it was trained without an EMA."""
    state = checkpoint.get('ema_state_dict') if isinstance(checkpoint, dict) else None
    if state is None:
        raise KeyError(f"checkpoint {checkpoint_path!r} holds no EMA weights (no 'ema_state_dict': it was trained "
                       "without --ema_decay, or it is a bare state_dict; the file train() writes as "
                       "*_final_ema.pth loads with weights='model')")
    return state['shadow']


def load_checkpoint(model, optimizer, scheduler, checkpoint_path, *, ema=None, bare_weights=False):
    """Resume from a per-epoch checkpoint dict (diffusion_RDUnet.py:180-193,
    main_diffusion_RDUnet.py:339-352; weights-only safe load) and return its epoch; 0 where
    there is no such file.  ``ema`` is restored too (restore_ema).  ``bare_weights`` (the
    baseline's loader): the file may also be the bare ``state_dict`` a ``train`` writes at the
    end -- weights only, the optimizer and scheduler stay as built, returns 0 -- and the
    optimizer may be None."""
    if checkpoint_path is None or not os.path.isfile(checkpoint_path):
        print(f"No checkpoint found at '{checkpoint_path}'")
        return 0
    print(f"Loading checkpoint '{checkpoint_path}'")
    dev = next(model.parameters()).device
    checkpoint = torch.load(checkpoint_path, map_location=dev, weights_only=True)
    if bare_weights and 'model_state_dict' not in checkpoint:
        model.load_state_dict(checkpoint)
        restore_ema(ema, None, model)
        print(f"Loaded weights '{checkpoint_path}'")
        return 0
    model.load_state_dict(checkpoint['model_state_dict'])
    if not (bare_weights and optimizer is None):
        optimizer.load_state_dict(checkpoint['optimizer_state_dict'])
    if scheduler is not None and checkpoint.get('scheduler_state_dict') is not None:
        scheduler.load_state_dict(checkpoint['scheduler_state_dict'])
    restore_ema(ema, checkpoint, model)
    start_epoch = checkpoint['epoch']
    print(f"Loaded checkpoint '{checkpoint_path}' (epoch {start_epoch})")
    return start_epoch


def load_data(args):
    """diffusion_RDUnet.py:222-228 dispatch on ``args.dataset_choice``;
    ``args.data_pipeline == 'gpu'``: the device-side loaders of ``synth`` over the same
    folders (no worker processes)."""
    kw = dict(batch_size=args.batch_size, augment=args.augment, dataset_percentage=args.dataset_percentage,
              validation_split=args.validation_split, use_rgb=True)
    if getattr(args, "data_pipeline", "pil") == 'gpu':
        from . import synth
        load_div2k, load_sidd = synth.load_data_gpu, synth.load_sidd_data_gpu
    else:
        from . import data_loader
        load_div2k, load_sidd = data_loader.load_data, data_loader.load_sidd_data
        kw["num_workers"] = args.num_workers
    if args.dataset_choice == 'DIV2K':
        return load_div2k('dataset/DIV2K_train_HR.nosync', **kw)
    return load_sidd('dataset/SIDD_dataset.nosync/SIDD_Medium_Srgb', **kw)


def add_data_arguments(parser):
    """The flags every training command line declares (diffusion_RDUnet.py:293-309's dataset and
    run flags, plus --dtype, --step_mode and --data_pipeline); a command line whose default
    differs sets it with ``parser.set_defaults``."""
    parser.add_argument('--dataset_choice', type=str, default='SIDD', choices=['DIV2K', 'SIDD'])
    parser.add_argument('--checkpoint_path', type=str, default=None)
    parser.add_argument('--num_epochs', type=int, default=300)
    parser.add_argument('--batch_size', type=int, default=8)
    parser.add_argument('--num_workers', type=int, default=8)
    parser.add_argument('--validation_split', type=float, default=0.2)
    parser.add_argument('--augment', action='store_false')
    parser.add_argument('--dataset_percentage', type=float, default=0.1)
    parser.add_argument('--output_dir', type=str, default='checkpoints')
    parser.add_argument('--dtype', type=str, default='fp32', choices=['fp32', 'bf16'])
    parser.add_argument('--step_mode', type=str, default='eager', choices=['eager', 'graph'],
                        help="graph: fused optimizer, every batch replayed as one captured hipGraph")
    parser.add_argument('--data_pipeline', type=str, default='pil', choices=['pil', 'gpu'],
                        help="gpu: patches cut and augmented on the device (synth loaders), no worker processes")
    return parser


def add_ema_arguments(parser):
    """``--ema_decay`` / ``--ema_warmup`` (no reference counterpart), on every trainer's parser.
    Optional additions to the reference's namespaces: a flag that is not given leaves no
    attribute behind (``argparse.SUPPRESS``) and ``make_ema`` reads them with the defaults
    0 (no EMA) and False."""
    parser.add_argument('--ema_decay', type=float, default=argparse.SUPPRESS,
                        help="keep an exponential moving average of the weights with this decay (default 0: none), "
                             "validate with it too and save it in the checkpoints")
    parser.add_argument('--ema_warmup', action='store_true', default=argparse.SUPPRESS,
                        help="ramp the EMA decay as min(decay, (1 + n) / (10 + n)) over the first updates")
    return parser


def make_ema(args, model):
    """The optim.EMA the ``--ema_decay`` / ``--ema_warmup`` flags ask for, or None."""
    decay = float(getattr(args, "ema_decay", 0.0) or 0.0)
    if decay <= 0.0:
        return None
    return EMA(model, decay, warmup=bool(getattr(args, "ema_warmup", False)))


def save_final_ema(model, ema, path):
    """The averaged weights as a bare ``state_dict`` of ``model`` (what ``denoise_image
    --checkpoint`` and ``model.load_state_dict`` take as it is)."""
    ema.use_names_of(model)
    state = model.state_dict()
    state.update(ema.state_dict()['shadow'])
    torch.save(state, path)
    print(f"Final EMA weights saved at {path}")
