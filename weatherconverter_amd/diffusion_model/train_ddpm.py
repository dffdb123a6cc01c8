"""Drop-in for the reference's ``diffusion_model/train_ddpm.py`` training-loss path (BASELINE config 3).

One training iteration of the reference (``train_ddpm.py:94-114``) is
    noise = randn_like(images); t = randint(0, T, (B,))
    noisy_im = scheduler.add_noise(images, noise, t)        # :105
    noise_pred = model(noisy_im, t)                         # :106
    loss = criterion(noise_pred, noise)                     # :108, criterion = nn.MSELoss() (:177)
followed by ``loss.backward()``, ``optimizer.step()`` and, beyond the reference, ``ema.update()`` (the
exponential moving average of the weights DDPM samples from; ``make_ema``).  All of it runs on HIP kernels:
``wc_add_noise`` (per-sample coefficients), the UNet forward with per-sample timesteps recording its
tape, ``wc_mse_loss`` (fp64-accumulated, deterministic mean, fused with d loss / d noise_pred),
``loss.backward()`` through ``UnetTrainFunction`` (models/train_engine.py: data and weight gradients,
GroupNorm, attention and time-embedding backward kernels), and the Adam update with the optimizer
``make_optimizer`` returns (``optim.Adam``: ``wc_adam_step``, one launch per parameter group, and
``wc_grad_norm`` for clipping by global norm); the reference's own ``torch.optim.Adam`` over the same
parameters keeps working and shares its ``state_dict`` format; then the average's update (``ema.EMA``:
``wc_ema_update``, one launch for the whole model).  ``training_loss`` is the forward;
``TrainForward`` is the same captured into a HIP graph for the forward-only line.  Checkpoints keep the
reference format (``:56-68``): ``{'model_state_dict', 'optimizer_state_dict', 'epoch'}`` saved as
``f'{epoch}-checkpoint.ckpt'``; with an ``EMA`` a fourth key ``'ema_state_dict'`` rides along, which the
reference's loader does not read.
"""
import os
from typing import Optional, Tuple

import torch

from .. import kernels as K
from .config import Config, load_config  # noqa: F401  (reference :19-22)
from .ema import EMA
from .models.unet_base import Unet
from .optim import Adam
from .scheduler.linear_noise_scheduler import LinearNoiseScheduler


def training_loss(model: Unet, scheduler: LinearNoiseScheduler, images: torch.Tensor, noise: torch.Tensor,
                  t: torch.Tensor, *, with_grad: bool = False) -> Tuple[torch.Tensor, ...]:
    """The forward of one training iteration (``train_ddpm.py:105-108``) on the GPU.

    Returns ``(loss, noise_pred)``; with ``with_grad=True`` also d loss / d noise_pred (the seed of
    the backward pass), written by the same MSE sweep.  ``t``: int64 (B,) per-sample timesteps."""
    dev = next(model.parameters()).device
    tt = torch.as_tensor(t).long().reshape(-1).to(dev)
    if tt.numel() != images.shape[0]:
        raise RuntimeError(f'training_loss: {tt.numel()} timesteps for a batch of {images.shape[0]}')
    nz = noise.to(dev, torch.float32).contiguous()
    with torch.no_grad():
        noisy = scheduler.add_noise(images, nz, tt)
        pred = model(noisy, tt)
        out = K.mse_loss(pred, nz, grad=with_grad)
    if with_grad:
        loss, g = out
        return loss, pred, g
    return out, pred


class TrainForward:
    """``training_loss`` captured into a HIP graph over fixed device buffers (images, noise, t):
    copy a batch in, replay, read ``loss``.  Used by the config-3 benchmark."""

    def __init__(self, model: Unet, scheduler: LinearNoiseScheduler, images: torch.Tensor, noise: torch.Tensor,
                 t: torch.Tensor):
        self.model, self.scheduler = model, scheduler
        dev = next(model.parameters()).device
        self.images = images.to(dev, torch.float32).contiguous().clone()
        self.noise = noise.to(dev, torch.float32).contiguous().clone()
        self.t = torch.as_tensor(t).long().reshape(-1).to(dev).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                self.loss, self.pred = training_loss(model, scheduler, self.images, self.noise, self.t)
        torch.cuda.current_stream().wait_stream(s)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.loss, self.pred = training_loss(model, scheduler, self.images, self.noise, self.t)

    def __call__(self, images: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                 t: Optional[torch.Tensor] = None) -> torch.Tensor:
        if images is not None:
            self.images.copy_(images)
        if noise is not None:
            self.noise.copy_(noise)
        if t is not None:
            self.t.copy_(torch.as_tensor(t).reshape(-1))
        self.graph.replay()
        return self.loss


def make_optimizer(model: Unet, training_config, *, max_grad_norm: Optional[float] = None) -> Adam:
    """``train_ddpm.py:190``, ``optimizer = Adam(model.parameters(), lr=config.training.lr)``, with the HIP
    optimizer.  ``training_config``: the ``Config`` or its ``training`` section.  ``max_grad_norm``: the
    clipping the reference carries commented out at ``:112``, fused into the step."""
    training = getattr(training_config, 'training', training_config)
    return Adam(model.parameters(), lr=training.lr, max_grad_norm=max_grad_norm)


def make_ema(model: Unet, decay: float = 0.9999, *, warmup: bool = False) -> EMA:
    """The exponential moving average of ``model``'s weights, to ``update()`` after every ``optimizer.step()``
    and to sample from (``with ema.swapped():``, or a checkpoint's ``load_model(..., weights='ema')``)."""
    return EMA(model, decay, warmup=warmup)


# ----------------------------------------------------------------------------------- checkpoints
def checkpoint_path(folder: str, run_id, epoch: int) -> str:
    """``train_ddpm.py:57`` naming: <checkpoints>/<run_id>/<epoch>-checkpoint.ckpt."""
    return os.path.join(folder, str(run_id), f'{epoch}-checkpoint.ckpt')


def save_checkpoint(epoch: int, model: Unet, opt: torch.optim.Optimizer, folder: str, run_id=0, *,
                    ema: Optional[EMA] = None) -> str:
    """``train_ddpm.py:55-59``: {'model_state_dict', 'optimizer_state_dict', 'epoch'}, and with ``ema`` a
    fourth key 'ema_state_dict' (the reference's loader reads its three and ignores it)."""
    path = checkpoint_path(folder, run_id, epoch)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    ck = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': opt.state_dict(), 'epoch': epoch}
    if ema is not None:
        ck['ema_state_dict'] = ema.state_dict()
    torch.save(ck, path)
    return path


def load_checkpoint(model: Unet, opt: Optional[torch.optim.Optimizer], checkpoint_path: str, *,
                    ema: Optional[EMA] = None):
    """``train_ddpm.py:62-68`` -> (model, opt, epoch).  Tensors and plain containers only
    (``weights_only=True``: nothing in the file is executed).  With ``ema`` the file's 'ema_state_dict' is
    loaded into it; a file without one raises ``RuntimeError``."""
    ck = torch.load(checkpoint_path, map_location='cpu', weights_only=True)
    if ema is not None and 'ema_state_dict' not in ck:
        raise RuntimeError(f"load_checkpoint: {checkpoint_path} has no 'ema_state_dict' (saved without ema=)")
    model.load_state_dict(ck['model_state_dict'])
    if opt is not None and 'optimizer_state_dict' in ck:
        opt.load_state_dict(ck['optimizer_state_dict'])
    if ema is not None:
        ema.load_state_dict(ck['ema_state_dict'])
    return model, opt, ck['epoch']


# ----------------------------------------------------------------------------------- the epoch loop
def train(dataloader, model: Unet, optimizer: torch.optim.Optimizer, scheduler: LinearNoiseScheduler, config: Config, *,
          ema: Optional[EMA] = None, log=None, run_id=0) -> int:
    """The epoch loop of ``train_ddpm.py:71-143`` over a loader of ``(B, 3, S, S)`` device batches
    (``dataloader.get_loader``).  Per batch: ``noise = randn_like(images)``, ``t = randint(0, T, (B,))``, the
    HIP forward with its tape (``add_noise``, the UNet), ``wc_mse_loss`` giving the loss and d loss / d pred
    in one sweep, the HIP backward from that seed, ``optimizer.step()``, then ``ema.update()``.

    ``log`` is called with the reference's two ``wandb.log`` dicts (``{'train_loss', 'epoch'}`` every
    ``log_interval`` batches, ``{'average_epoch_loss', 'epoch'}`` per epoch); ``None`` logs nothing.  The
    losses accumulate on the device and are read once per ``log_interval`` and once per epoch, not once per
    iteration as ``:117-118`` do.  ``resume_training`` loads ``resume_checkpoint`` and runs ``epochs`` more
    epochs from its epoch on, as ``:81-84`` do (the checkpoint's epoch is run again: the reference's count).
    A checkpoint is saved every ``save_interval`` epochs under ``folders.checkpoints/<run_id>/``.  Returns
    the last epoch run."""
    tr = config.training
    start_epoch, num_epochs = 1, tr.epochs
    num_batches = len(dataloader)
    T = config.diffusion.num_timesteps
    if tr.resume_training:
        model, optimizer, start_epoch = load_checkpoint(model, optimizer, tr.resume_checkpoint, ema=ema)
        num_epochs += start_epoch  # :83
        print(f'Resuming training from epoch {start_epoch}')
    dev = next(model.parameters()).device
    epoch_idx = start_epoch - 1
    for epoch_idx in range(start_epoch, num_epochs + 1):
        model.train()
        total = torch.zeros((), dtype=torch.float32, device=dev)
        interval = torch.zeros((), dtype=torch.float32, device=dev)
        for batch_idx, images in enumerate(dataloader):
            optimizer.zero_grad(set_to_none=True)
            images = images.float().to(dev)
            noise = torch.randn_like(images)
            t = torch.randint(0, T, (images.shape[0], )).to(dev)
            noisy = scheduler.add_noise(images, noise, t)
            pred = model(noisy, t)
            loss, g = K.mse_loss(pred.detach(), noise, grad=True)
            pred.backward(g)
            optimizer.step()
            if ema is not None:
                ema.update()
            total += loss
            interval += loss
            if (batch_idx + 1) % tr.log_interval == 0:
                avg = interval.item() / tr.log_interval  # the one host read of the interval
                interval.zero_()
                print(f'Epoch: {epoch_idx} | Batch: {batch_idx + 1}/{num_batches} | Loss: {avg:.4f}')
                if log is not None:
                    log({'train_loss': avg, 'epoch': epoch_idx})
        avg_epoch = total.item() / max(num_batches, 1)
        print(f'Finished epoch: {epoch_idx} | Average Loss: {avg_epoch:.4f}')
        if log is not None:
            log({'average_epoch_loss': avg_epoch, 'epoch': epoch_idx})
        if epoch_idx % tr.save_interval == 0:
            path = save_checkpoint(epoch_idx, model, optimizer, config.folders.checkpoints, run_id, ema=ema)
            print(f'Saved checkpoints into {path}...')
    print('Done Training ...')
    return epoch_idx


def main(config_path: Optional[str] = None, *, ema_decay: Optional[float] = 0.9999, log=None, run_id=0):
    """``train_ddpm.py:146-199``: the loader over ACDC + BDD + DAWN, the model, Adam, the scheduler (and the
    EMA) from the yaml, then ``train``.  ``data.image_size`` is a list in the yaml; its first entry is the
    crop size."""
    import random
    from pathlib import Path

    import numpy as np

    from .dataloader import ACDCDataset, make_loader
    config = load_config(config_path) if config_path else load_config()
    seed = config.training.random_seed  # :31-34
    torch.manual_seed(seed)
    np.random.seed(seed)
    random.seed(seed)
    dev = torch.device('cuda' if config.training.device in ('auto', 'cuda') else config.training.device)
    size = config.data.image_size
    size = int(size[0] if isinstance(size, (list, tuple)) else size)
    root = Path(config.data.root_dir)
    dataset = ACDCDataset(root / config.data.acdc_images, config.data.weather, image_size=size)
    dataset.add_images(root / config.data.bdd_dir)
    dataset.add_images(root / config.data.dawn_dir)
    print(len(dataset))
    loader = make_loader(dataset, config.training.batch_size, config.training.num_workers, device=dev)
    scheduler = LinearNoiseScheduler(config.diffusion.num_timesteps, config.diffusion.beta_start,
                                     config.diffusion.beta_end, device=dev)
    model = Unet(config.model).to(dev).train()
    optimizer = make_optimizer(model, config)
    ema = make_ema(model, ema_decay) if ema_decay is not None else None
    return train(loader, model, optimizer, scheduler, config, ema=ema, log=log, run_id=run_id)


if __name__ == '__main__':
    import sys
    main(sys.argv[1] if len(sys.argv) > 1 else None)
