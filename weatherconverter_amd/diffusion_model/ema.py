"""The exponential moving average (EMA) of the weights, on HIP: the line a DDPM training loop adds after
``optimizer.step()`` (reference ``train_ddpm.py:114``; the reference itself keeps no average, Ho et al.
2020 sample from one with decay 0.9999).

``EMA`` keeps one fp32 shadow tensor per parameter.  ``update()`` moves every shadow towards its
parameter in ONE launch (``wc_ema_update`` over a device job table, as ``optim.Adam`` steps), and
``swap()`` / ``with ema.swapped():`` exchange the weights with their average in place (``wc_ema_swap``),
so the HIP engines sample from the average without a second copy of the model: the parameters' version
counters are bumped and every engine repacks.
"""
import contextlib
from typing import Dict, Optional

import torch

from .. import kernels as K


class EMA:
    """``EMA(model, decay=0.9999, *, warmup=False)``: ``shadow = decay * shadow + (1 - decay) * p``.

    * The shadow holds one fp32 tensor per ``model.named_parameters()`` entry, initialised by a copy of
      the parameter, on the parameter's device, never seen by autograd.  Buffers are NOT tracked (the
      Unet has none: its ``state_dict`` keys are its parameters); a module with buffers keeps its own.
    * ``update()`` counts in ``num_updates`` and uses ``decay``, or with ``warmup``
      ``min(decay, (1 + num_updates) / (10 + num_updates))``.  One launch, no host synchronisation.
      Parameters must be contiguous fp32 tensors on one GPU; anything else raises ``RuntimeError``
      (there is no torch fallback).  Construction and the ``state_dict`` round trip work on the CPU.
    * Between ``swap()`` and the next ``swap()`` (inside ``with ema.swapped():``) the model IS the average
      and the shadow holds the raw weights; ``update()`` and the ``state_dict`` functions raise there.
      A HIP graph captured from the model before a swap keeps replaying the packs it captured: capture
      inside the context (``sample_tensor(graph=True)`` builds its own per call).
    """

    def __init__(self, model: torch.nn.Module, decay: float = 0.9999, *, warmup: bool = False):
        if not 0.0 <= decay <= 1.0:
            raise ValueError(f'Invalid EMA decay: {decay}')
        self.decay = float(decay)
        self.warmup = bool(warmup)
        self.num_updates = 0
        self._params: Dict[str, torch.nn.Parameter] = dict(model.named_parameters())
        self.shadow: Dict[str, torch.Tensor] = {
            name: p.detach().to(torch.float32, copy=True, memory_format=torch.contiguous_format)
            for name, p in self._params.items()}
        self._jobs: Optional[K.EmaJobs] = None
        self._swapped = False

    def decay_at(self, num_updates: int) -> float:
        """The decay the update that makes ``num_updates`` its count uses."""
        if not self.warmup:
            return self.decay
        return min(self.decay, (1 + num_updates) / (10 + num_updates))

    def _table(self) -> K.EmaJobs:
        """The device job table: kept across calls, rebuilt when any address or size in it changed (the
        model moved to another device, a parameter's storage was replaced)."""
        ps = list(self._params.values())
        for name, p in self._params.items():
            if self.shadow[name].device != p.device:  # model.to(device) after construction
                self.shadow[name] = self.shadow[name].to(p.device)
        ss = list(self.shadow.values())
        jobs = self._jobs
        if jobs is not None and len(jobs.words) == 4 * len(ps) and jobs.device == ps[0].device:
            w = jobs.words
            for k in range(len(ps)):
                if w[4 * k] != ss[k].data_ptr() or w[4 * k + 1] != ps[k].data_ptr() or w[4 * k + 2] != ps[k].numel():
                    break
            else:
                return jobs
        self._jobs = K.ema_jobs(ss, ps)
        return self._jobs

    def _unswapped(self, what: str):
        if self._swapped:
            raise RuntimeError(f'EMA.{what}: the weights are swapped with their average (inside swapped()); '
                               f'swap back first')

    def update(self):
        """One averaging step over every parameter (``wc_ema_update``), after ``optimizer.step()``."""
        self._unswapped('update')
        if not self._params:
            return
        jobs = self._table()
        self.num_updates += 1
        K.ema_update(jobs, self.decay_at(self.num_updates))

    def swap(self):
        """Exchange the weights and their average in place, bit for bit (``wc_ema_swap``), and bump the
        parameters' version counters so that every engine repacks.  Twice is the identity."""
        if self._params:
            K.ema_swap(self._table())
            # the kernel wrote through raw addresses: tell autograd and everything keyed on _version
            torch.autograd.graph.increment_version(list(self._params.values()) + list(self.shadow.values()))
        self._swapped = not self._swapped

    @contextlib.contextmanager
    def swapped(self):
        """``with ema.swapped(): sample(model, ...)``: the model is the average inside the block and the
        raw weights again after it, also when the body raises."""
        self._unswapped('swapped')
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    @torch.no_grad()
    def copy_to(self, model: Optional[torch.nn.Module] = None):
        """Overwrite the parameters of ``model`` (default: the averaged model) with the average: a plain
        torch copy, for the end of training."""
        self._unswapped('copy_to')
        params = self._params if model is None else dict(model.named_parameters())
        self._check_names(params, 'copy_to')
        for name, p in params.items():
            p.copy_(self.shadow[name])

    def _check_names(self, other, what: str):
        missing = [n for n in self.shadow if n not in other]
        unexpected = [n for n in other if n not in self.shadow]
        if missing or unexpected:
            raise RuntimeError(f'EMA.{what}: missing names {missing[:5]}, unexpected names {unexpected[:5]}')

    def shadow_state_dict(self) -> Dict[str, torch.Tensor]:
        """``name -> averaged tensor``: what ``Unet.load_state_dict`` takes directly."""
        self._unswapped('shadow_state_dict')
        return dict(self.shadow)

    def state_dict(self) -> dict:
        """``{'decay', 'num_updates', 'warmup', 'shadow': {parameter name: tensor}}``: tensors and plain
        Python values only, so a ``weights_only=True`` load accepts it."""
        self._unswapped('state_dict')
        return {'decay': self.decay, 'num_updates': self.num_updates, 'warmup': self.warmup,
                'shadow': dict(self.shadow)}

    @torch.no_grad()
    def load_state_dict(self, state: dict):
        """Strict on names and shapes; the values are copied into the existing shadow tensors."""
        self._unswapped('load_state_dict')
        shadow = state['shadow']
        self._check_names(shadow, 'load_state_dict')
        for name, t in shadow.items():
            if tuple(t.shape) != tuple(self.shadow[name].shape):
                raise RuntimeError(f'EMA.load_state_dict: {name} has shape {tuple(t.shape)}, expected '
                                   f'{tuple(self.shadow[name].shape)}')
        for name, t in shadow.items():
            self.shadow[name].copy_(t)
        self.decay = float(state['decay'])
        self.num_updates = int(state['num_updates'])
        self.warmup = bool(state['warmup'])
