"""``optimizer.step()`` of the reference's training iteration (``train_ddpm.py:113``) on HIP.

``Adam`` is a ``torch.optim.Optimizer`` with ``torch.optim.Adam``'s arithmetic (and ``AdamW``'s with
``decoupled_weight_decay=True``), its per-parameter state and its ``state_dict`` format, so a
checkpoint written with either loads into the other.  What differs is how a step runs: every tensor of
a parameter group is updated by ONE launch (``wc_adam_step`` over a device job table) instead of a
handful of elementwise launches per tensor list, and gradient clipping by global norm
(``max_grad_norm``; the reference carries ``clip_grad_norm_(model.parameters(), max_norm=1.0)``
commented out at ``:112``) costs one read of the gradients and no host synchronisation: the norm and
the clip coefficient stay on the device and the step multiplies every gradient by the coefficient as
it reads it.
"""
from typing import List, Optional

import torch

from .. import kernels as K

_UNSUPPORTED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'foreach', 'fused')


class Adam(torch.optim.Optimizer):
    """``torch.optim.Adam`` for fp32 device parameters, one HIP launch per parameter group.

    ``Adam(params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, *,
    decoupled_weight_decay=False, max_grad_norm=None)``

    * Parameter groups, ``lr`` schedulers (the hyper-parameters are read from ``param_groups`` at every
      step), ``zero_grad``, hooks, ``state_dict()`` and ``load_state_dict()`` are the base class's.  The
      state per parameter is ``{'step': 0-dim float32 CPU tensor, 'exp_avg', 'exp_avg_sq'}``, created
      at the first step at which the parameter has a gradient; a parameter without a gradient is
      skipped and its ``step`` does not advance.
    * ``amsgrad``, ``maximize``, ``capturable``, ``differentiable``, ``foreach`` and ``fused`` are not
      implemented: passed truthy (or loaded truthy from another optimizer's ``state_dict``) they raise
      ``ValueError``.  Parameters must be contiguous fp32 tensors on one GPU; anything else raises
      ``RuntimeError`` (there is no torch fallback).
    * ``max_grad_norm``: clip by the global L2 norm of the gradients of ALL groups together, the norm
      ``torch.nn.utils.clip_grad_norm_(model.parameters(), max_grad_norm)`` computes, with its
      coefficient ``min(1, max_grad_norm / (norm + 1e-6))``.  After ``step()`` the norm is
      ``opt.grad_norm``, a 0-dim device tensor (reading it is the caller's synchronisation, ``step()``
      has none).  Unlike torch's utility this does NOT scale the ``.grad`` tensors: they are left as
      the backward wrote them and the coefficient is applied inside the update.  A non-finite norm is
      not special-cased (the NaN propagates, as with ``error_if_nonfinite=False``).
    * ``step()`` bumps the version counter of every parameter it updates, as an in-place torch op
      would: the engines' weight packs and autograd's saved-tensor check key on it.
    """

    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0,
                 amsgrad: bool = False, *, foreach: Optional[bool] = None, maximize: bool = False,
                 capturable: bool = False, differentiable: bool = False, fused: Optional[bool] = None,
                 decoupled_weight_decay: bool = False, max_grad_norm: Optional[float] = None):
        if isinstance(lr, torch.Tensor):
            raise ValueError('Adam: a tensor lr is not supported (it exists for capturable steps)')
        if not 0.0 <= lr:
            raise ValueError(f'Invalid learning rate: {lr}')
        if not 0.0 <= eps:
            raise ValueError(f'Invalid epsilon value: {eps}')
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f'Invalid beta parameters: {betas}')
        if not 0.0 <= weight_decay:
            raise ValueError(f'Invalid weight_decay value: {weight_decay}')
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f'Invalid max_grad_norm value: {max_grad_norm}')
        # the keys and defaults of torch.optim.Adam's groups, so either optimizer loads the other's state_dict
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=foreach, capturable=capturable, differentiable=differentiable, fused=fused,
                        decoupled_weight_decay=decoupled_weight_decay)
        self._check_options(defaults)
        super().__init__(params, defaults)
        self.max_grad_norm = max_grad_norm
        self.grad_norm: Optional[torch.Tensor] = None
        self._jobs: Optional[K.AdamJobs] = None

    @staticmethod
    def _check_options(group):
        for name in _UNSUPPORTED:
            if group.get(name):
                raise ValueError(f'weatherconverter_amd Adam: {name}={group[name]!r} is not supported')

    def _plan(self):
        """This step's work: (group, step count, first row, row count) per launch and the operands of
        every row, group by group.  Creates missing state and advances the step counts."""
        launches, ps, gs, ms, vs = [], [], [], [], []
        for group in self.param_groups:
            self._check_options(group)
            by_step = {}  # parameters that joined at different steps differ in bias correction
            for p in group['params']:
                if p.grad is None:
                    continue
                if p.grad.is_sparse:
                    raise RuntimeError('Adam does not support sparse gradients')
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st['step'] += 1
                by_step.setdefault(int(st['step']), []).append(p)
            for step, plist in by_step.items():
                launches.append((group, step, len(ps), len(plist)))
                for p in plist:
                    st = self.state[p]
                    ps.append(p)
                    gs.append(p.grad)
                    ms.append(st['exp_avg'])
                    vs.append(st['exp_avg_sq'])
        return launches, ps, gs, ms, vs

    def _table(self, ps: List[torch.Tensor], gs, ms, vs) -> K.AdamJobs:
        """The device job table of this step's rows: kept across steps, rebuilt when any address or size
        in it changed (the backward allocates the gradients anew; load_state_dict replaces the state)."""
        jobs = self._jobs
        if jobs is not None and len(jobs.words) == 6 * len(ps) and jobs.device == ps[0].device:
            w = jobs.words
            for k in range(len(ps)):
                if (w[6 * k] != ps[k].data_ptr() or w[6 * k + 1] != gs[k].data_ptr() or w[6 * k + 2] != ms[k].data_ptr()
                        or w[6 * k + 3] != vs[k].data_ptr() or w[6 * k + 4] != ps[k].numel()):
                    break
            else:
                return jobs
        self._jobs = K.adam_jobs(ps, gs, ms, vs)
        return self._jobs

    @torch.no_grad()
    def step(self, closure=None):
        """One optimization step; ``closure`` (optional) re-evaluates the model and returns the loss."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        launches, ps, gs, ms, vs = self._plan()
        if not ps:
            return loss
        jobs = self._table(ps, gs, ms, vs)
        clip = None
        if self.max_grad_norm is not None:
            self.grad_norm, clip = K.grad_norm(jobs, self.max_grad_norm)
        for group, step, first, count in launches:
            beta1, beta2 = group['betas']
            K.adam_step(jobs, step=step, lr=group['lr'], beta1=beta1, beta2=beta2, eps=group['eps'],
                        weight_decay=group['weight_decay'],
                        decoupled_weight_decay=bool(group.get('decoupled_weight_decay', False)), clip=clip,
                        first=first, count=count)
        # the kernel wrote through raw addresses: tell autograd (and everything keyed on _version) so
        torch.autograd.graph.increment_version(ps)
        return loss
