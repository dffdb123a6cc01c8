"""GPU: every engine on weights that changed after its first pass.

Every other whole-model test builds a fresh model, runs it once on the weights it was built with and throws
it away.  The engines keep derived state between calls: UnetEngine / OldUnetEngine / SrganEngine cache
packed weights (bf16x6 / f16x3 / Winograd packs, folded BatchNorm) and the range exponents computed from
the weights (f16x3_a_exp from max|gamma|, max|beta|; the attention q / k / v exponents from the
in-projection's row L1 norms; the head's), all keyed by _signature() = (data_ptr, _version) per parameter;
kernels.conv_in keeps a transposed stem weight keyed by _version; TrainEngine re-packs on every forward
and builds some packs lazily in the backward.  This file runs them again after the parameters changed.

The comparison used throughout: after a change, the long-lived model's result must be torch.equal to that
of a FRESH model (a new module, load_state_dict of the long-lived model's current state_dict(), .cuda():
no engine yet).  The kernels are deterministic, so the tolerance is zero.  Two side conditions keep it
from being vacuous: (1) the fresh model is inside the accuracy envelope on the new weights (rel-L2 < 1e-5
of the float64 oracle on those weights, the suite's whole-model bound), and (2) the change matters (the
result moved by rel-L2 > 1e-3 -- per single tensor > 1e-4 -- so a stale engine fails).

The new weights W' of (a), (c): init_synthetic_(seed=1), every GroupNorm weight x 2 and bias + 0.5 (moves
f16x3_a_exp), every in_proj_weight x 2 (moves the attention exponents): W_PRIME below.  The GroupNorm
multiplier was planned as 8 and halved twice, because at 8 and at 4 the FRESH model misses side condition 1
-- and so does PyTorch's own fp32 forward on the CPU: the attention logits grow with the square of the
multiplier, the softmax saturates, and the network itself becomes ill-conditioned; no range is exceeded
(the three precisions miss alike).  Fresh model vs float64 on an MI355X, rel-L2 (f16x3 / bf16x6 / fp32):
  S1    x 8: 9.6e-4 / 1.3e-3 / 1.4e-3 (torch fp32 on the CPU: 6.3e-4)   x 4: 3.4e-5 / 5.6e-5 / 5.8e-5
        x 2: 9.0e-7 / 1.4e-6 / 1.7e-6                                     <- used
  tiny  x 8: 7.3e-1 (torch fp32 on the CPU: 7.4e-1)   x 4: 5.7e-2   x 2: 7.5e-6                 <- used
(each test prints the fresh model's error: `pytest -s`).

What is NOT detected, by design: an in-place write through p.data (or a raw pointer) moves neither
_version nor data_ptr, and a per-forward content check would need a device-to-host sync, which graph
capture forbids.  After such a write the caller calls invalidate_packs() (route r9; INTEGRATION.md, "When
weights change").  test_torch_version_counter_facts (CPU) pins the torch behaviour this rests on.

Mutation checks (run once on a scratch copy on an MI355X; the mutant must fail the named tests while
every pre-existing whole-model test still passes -- the gap this file closes):
  1. UnetEngine.refresh() without the signature comparison: fails (a) r1, r2, r5 and r6 in all three
     precisions (r3, r4, r7, r8 and r9 drop the engine themselves), both cases of (c), and (b) at the ten
     names whose values the engine copies into a pack or an exponent (the conv, projection, time-embedding and resampling
     weights, the GroupNorm weights in front of a conv or an attention); the six names the kernels read from
     the live tensor (conv_in.weight, t_proj.0.weight, norm_out.weight and the biases) pass, as they must;
     tests/test_gpu_unet.py, test_gpu_forms.py and test_gpu_shapes.py: 198 passed.
  2. _signature() without _version: fails (a) r1, r2 and r5 in all three precisions (r6 moves the pointers),
     both cases of (c) and the same ten names of (b); the same three files: 198 passed.
  3. TrainEngine._pack() after an engine's first call puts the first call's packs back instead of packing
     (plainly skipping it raises TypeError in any second forward, the existing Adam-step and accumulation
     tests included: the tape takes the packs with it): fails (d) in all five precisions, by the loss at
     iteration 2 (f16x3: 1.12128 for 1.09989), and both cases of (e) in the clean step after the raise;
     tests/test_gpu_train.py, test_gpu_forms.py, test_gpu_shapes.py and test_train.py: 310 passed, the
     three-step Adam test among them.
  4. OldUnetEngine._signature() without the buffers (the code before this file): fails (g)
     r1_bn_running_var_alone; tests/test_old_unet.py: 2 passed.

(b)'s edits are the prescribed x 4 (a bias + 0.5) for every name, none halved: after each edit the fresh
model is within 5.5e-7 .. 9.0e-7 of float64 (MI355X, f16x3) and the result moves by 5.1e-2 .. 4.2.

Wall time of this file on an MI355X: 22 s for its 64 GPU tests, the slowest 1.9 s (the one that runs the
module's first float64 pass on S1; each case of (b) runs one such pass).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_gpu_forms import FWD_BASE, S1_CONFIG, _Case, _n, _recording
from test_gpu_train import _check

gpu = pytest.mark.gpu

# W': (GroupNorm weight x, GroupNorm bias +, in_proj_weight x) per model; the module docstring says why not 8
W_PRIME = {'s1': (2.0, 0.5, 2.0), 'tiny': (2.0, 0.5, 2.0)}
PRECISIONS = ['f16x3', 'bf16x6', 'fp32']
OTHER_PRECISION = {'f16x3': 'bf16x6', 'bf16x6': 'fp32', 'fp32': 'f16x3'}
INTEGRATION_NOTE = ('torch changed how in-place writes move Tensor._version / data_ptr(): revisit INTEGRATION.md, '
                    '"When weights change", and the engines\' _signature()')


# ------------------------------------------------------------------ helpers
def _cpu_sd(net):
    return {k: v.detach().cpu().clone() for k, v in net.state_dict().items()}


def _digest(sd):
    from weatherconverter_amd.synthetic import state_dict_digest
    return state_dict_digest(sd)


def _w_prime(template, gn_mul, gn_add, qkv_mul):
    """W' as a CPU state dict (the module docstring's recipe)."""
    from weatherconverter_amd.synthetic import init_synthetic_
    m = copy.deepcopy(template)
    init_synthetic_(m, seed=1)
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.mul_(gn_mul)
                mod.bias.add_(gn_add)
            if isinstance(mod, torch.nn.MultiheadAttention):
                mod.in_proj_weight.mul_(qkv_mul)
    return _cpu_sd(m)


class _Life:
    """A _Case (config, CPU template at seed 0, inputs) with W' and, memoised by the weights' digest, the
    float64 oracle's and the fresh models' results, so that every route shares one reference."""

    def __init__(self, config, w_prime, B=2):
        self.case = _Case(config, B=B, oracle=False)
        self.mc = self.case.mc
        self.x, self.t = self.case.x, self.case.t
        self.w1 = _w_prime(self.case.template, *w_prime)
        self._oracle, self._fresh = {}, {}

    def long_lived(self, precision=None, train_precision=None):
        net = self.case.net()
        _set_precision(net, precision, train_precision)
        return net

    def fresh(self, sd, precision=None, train_precision=None):
        """A new Unet, load_state_dict, .cuda(): no engine yet."""
        from weatherconverter_amd.diffusion_model.models.unet_base import Unet
        net = Unet(self.mc)
        net.load_state_dict(sd)
        _set_precision(net, precision, train_precision)
        return net.cuda()

    def oracle(self, sd):
        from oracle.unet_oracle import unet_forward
        key = _digest(sd)
        if key not in self._oracle:
            with torch.no_grad():
                self._oracle[key] = unet_forward({k: v.double() for k, v in sd.items()}, self.mc, self.x.double(), self.t)
        return self._oracle[key]

    def fresh_eval(self, sd, precision=None):
        """The fresh model's eval forward on sd (on the CPU), inside the accuracy envelope (side condition 1)."""
        key = (_digest(sd), precision)
        if key not in self._fresh:
            with torch.no_grad():
                y = self.fresh(sd, precision).eval()(self.x.cuda(), self.t.cuda()).cpu()
            err = rel_l2(y, self.oracle(sd))
            print(f'fresh model ({precision}) vs float64 on the new weights: rel-L2 {err:.3e}')
            assert err < 1e-5, err
            self._fresh[key] = y
        return self._fresh[key]


def _set_precision(net, precision, train_precision):
    if precision is not None:
        net.set_conv_precision(precision)
    if train_precision is not None:
        net.set_train_precision(train_precision)


@pytest.fixture(scope='module')
def s1():
    return _Life(S1_CONFIG, W_PRIME['s1'])


def _tiny_config():
    return json.load(open(os.path.join(GOLDEN, 'manifest.json')))['tiny']['config']


@pytest.fixture(scope='module')
def tiny():
    return _Life(_tiny_config(), W_PRIME['tiny'])


# ------------------------------------------------------------------ the routes by which W' is installed
def _r1(net, sd, precision=None):
    with torch.no_grad():
        for k, p in net.named_parameters():
            p.copy_(sd[k])


def _r2(net, sd, precision=None):
    for k, p in net.named_parameters():
        p.grad = (p.detach() - sd[k].to(p.device))
    torch.optim.SGD(net.parameters(), lr=1).step()
    net.zero_grad()


def _r3(net, sd, precision=None):
    net.load_state_dict(sd)


def _r4(net, sd, precision=None):
    net.load_state_dict({k: v.cuda() for k, v in sd.items()}, assign=True)


def _r5(net, sd, precision=None):
    children = [('conv_in', net.conv_in), ('norm_out', net.norm_out), ('conv_out', net.conv_out), ('t_proj', net.t_proj)]
    for name in ('downs', 'mids', 'ups'):
        children += [(f'{name}.{i}', blk) for i, blk in enumerate(getattr(net, name))]
    seen = 0
    for prefix, child in children:
        sub = {k[len(prefix) + 1:]: v for k, v in sd.items() if k.startswith(prefix + '.')}
        seen += len(sub)
        child.load_state_dict(sub)
    assert seen == len(sd)  # the children cover the whole tree


def _r6(net, sd, precision=None):
    for k, p in net.named_parameters():
        p.data = sd[k].to(p.device).clone()


def _r7(net, sd, precision=None):
    net.cpu()
    _r1(net, sd)
    net.cuda()


def _r8(net, sd, precision):
    net.set_conv_precision(OTHER_PRECISION[precision])
    with torch.no_grad():
        net(torch.zeros((1, net.model_config.im_channels, net.model_config.im_size, net.model_config.im_size),
                        device='cuda'), torch.tensor([1], device='cuda'))
    _r1(net, sd)
    net.set_conv_precision(precision)


def _r9(net, sd, precision=None):
    for k, p in net.named_parameters():
        p.data.copy_(sd[k])
    net.invalidate_packs()


ROUTES = {'r1_copy_': _r1, 'r2_sgd_step': _r2, 'r3_load_state_dict': _r3, 'r4_load_state_dict_assign': _r4,
          'r5_child_load_state_dict': _r5, 'r6_data_rebind': _r6, 'r7_cpu_roundtrip': _r7, 'r8_precision_roundtrip': _r8,
          'r9_data_copy_invalidate': _r9}


# ------------------------------------------------------------------ (a) eval UnetEngine, all parameters
@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('route', list(ROUTES))
def test_eval_engine_all_parameters_updated(s1, route, precision):
    """(a): the model has run one eval forward (its engine is packed for the seed-0 weights); W' arrives by
    one route; the next forward must equal a fresh model's on the model's current state_dict()."""
    from weatherconverter_amd import forms
    x, t = s1.x.cuda(), s1.t.cuda()
    with forms.using(**FWD_BASE), torch.no_grad():
        net = s1.long_lived(precision).eval()
        y0 = net(x, t).cpu()
        ROUTES[route](net, s1.w1, precision)
        with _recording() as rec:
            y1 = net(x, t).cpu()
        sd = _cpu_sd(net)
        yf = s1.fresh_eval(sd, precision)
    packs = _n(rec.counts, 'wc_pack_*')
    print(f'{route} {precision}: vs fresh rel-L2 {rel_l2(y1, yf):.3e} (bit-identical {torch.equal(y1, yf)}), '
          f'moved by {rel_l2(y1, y0):.3e}, pack launches in the second forward {packs}')
    assert rel_l2(yf, y0) > 1e-3  # side condition 2
    assert torch.equal(y1, yf)
    if precision == 'f16x3':
        assert packs >= 1  # the second forward did repack (forms.pack_device: the device pack kernels)


# ------------------------------------------------------------------ (b) eval UnetEngine, one tensor at a time
ONE_AT_A_TIME = [
    'conv_in.weight',
    'downs.0.resnet_conv_first.0.2.weight', 'downs.0.resnet_conv_first.0.0.weight', 'downs.0.resnet_conv_first.0.0.bias',
    'downs.0.t_emb_layers.0.1.weight', 't_proj.0.weight',
    'downs.0.residual_input_conv.0.weight',
    'mids.0.attention_norms.0.weight',
    'mids.0.attentions.0.in_proj_weight', 'mids.0.attentions.0.in_proj_bias', 'mids.0.attentions.0.out_proj.weight',
    'downs.0.down_sample_conv.weight', 'ups.1.up_sample_conv.weight',
    'norm_out.weight', 'conv_out.weight', 'conv_out.bias',
]


# the edit of every name: x 4 (a bias: + 0.5), the prescribed ones; none had to be halved (the fresh model's error
# vs float64 after each edit, MI355X f16x3: see the module docstring)
ONE_AT_A_TIME_MUL, ONE_AT_A_TIME_ADD = 4.0, 0.5


@pytest.fixture(scope='module')
def packed_s1(s1):
    """(b)'s long-lived f16x3 model with its engine packed for the seed-0 weights, and its first result."""
    from weatherconverter_amd import forms
    with forms.using(**FWD_BASE), torch.no_grad():
        net = s1.long_lived('f16x3').eval()
        y0 = net(s1.x.cuda(), s1.t.cuda()).cpu()
    return net, y0


@gpu
@pytest.mark.parametrize('name', ONE_AT_A_TIME)
def test_eval_engine_one_tensor_at_a_time(s1, packed_s1, name):
    """(b), f16x3: on the one packed engine all cases share, one named parameter x 4 (a bias + 0.5) under
    no_grad, compared with a fresh model, then restored (the first result must come back): a signature, pack
    or exponent that misses one KIND of tensor fails at that name.  Both side conditions per name: the fresh
    model within 1e-5 of float64 on the edited weights (s1.fresh_eval), and the result moved by > 1e-4.  One
    case per name: each runs one float64 pass on the CPU."""
    from weatherconverter_amd import forms
    net, y0 = packed_s1
    x, t = s1.x.cuda(), s1.t.cuda()
    p = dict(net.named_parameters())[name]
    with forms.using(**FWD_BASE), torch.no_grad():
        keep = p.detach().clone()
        try:
            if name.endswith('bias'):
                p.add_(ONE_AT_A_TIME_ADD)
            else:
                p.mul_(ONE_AT_A_TIME_MUL)
            y1 = net(x, t).cpu()
            yf = s1.fresh_eval(_cpu_sd(net), 'f16x3')  # asserts side condition 1
        finally:
            p.copy_(keep)
        y2 = net(x, t).cpu()
    moved = rel_l2(yf, y0)
    print(f'{name}: vs fresh rel-L2 {rel_l2(y1, yf):.3e}, moved by {moved:.3e}')
    assert moved > 1e-4, 'the edit is too small to tell a stale engine'
    assert torch.equal(y1, yf)
    assert torch.equal(y2, y0)  # restored: the first result again


@gpu
def test_conv_in_transposed_weight_cache_follows_the_version():
    """kernels.conv_in keeps the [Cin*9][Cout] transpose of the stem weight ON the weight tensor, keyed by
    _version.  Through the model a changed stem weight moves the signature, and the repack makes a new tensor
    object, so (b) never reaches the version key: here the SAME tensor object is changed in place between two
    calls.  Against the same call on a fresh tensor (bit for bit) and float64 conv2d (the fp32 VALU stem: 27
    products per output, rel-L2 < 1e-5, the suite's bound)."""
    from weatherconverter_amd import kernels as K
    g = torch.Generator().manual_seed(4)
    B, H, W = 2, 16, 24
    x = torch.randn((B, 3, H, W), generator=g)
    w = torch.randn((64, 3, 3, 3), generator=g) * 0.2
    b = torch.randn(64, generator=g) * 0.1
    xc, bc = x.cuda(), b.cuda()

    def run(wt):
        out = torch.empty((B, H, W, 64), device='cuda')
        K.GnPart.attach(out, 8)
        v = K.View.full(out)
        assert K.conv_in(xc, wt, bc, v, gn=K.GnPart.of(v))  # True: the form that reads the cached transpose
        return out.cpu()

    wc = w.cuda()
    y0 = run(wc)
    assert getattr(wc, '_wc_t', None) is not None
    wc.mul_(2)
    y1 = run(wc)
    yf = run((w * 2).cuda())
    ref = torch.nn.functional.conv2d(x.double(), (w * 2).double(), b.double(), padding=1).permute(0, 2, 3, 1)
    assert rel_l2(yf, ref) < 1e-5
    assert not torch.equal(yf, y0)
    assert torch.equal(y1, yf)


# ------------------------------------------------------------------ (c) graph sampling around a change
@gpu
@pytest.mark.parametrize('B,split', [(2, None), (4, 2)], ids=['B2', 'B4_split2'])
def test_graph_sampling_around_a_change(tiny, B, split):
    """(c): sample_tensor(graph=True) captures a fresh _GraphStep per call, after the engine has repacked in
    its warm-up.  With split=2 the two image groups run on their own streams: _GraphStep refreshes the packs
    (UnetEngine.refresh) on the warm-up stream BEFORE the groups fork, so neither group reads packs the other
    is still writing; the captured graph itself never packs."""
    from weatherconverter_amd import forms
    from weatherconverter_amd.diffusion_model.sample_ddpm import sample_tensor
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    s = LinearNoiseScheduler(2, 0.0001, 0.02)
    kw = dict(noise='philox', seed=3)
    net = tiny.long_lived().eval()
    with forms.using(graph_split=split):
        a = sample_tensor(net, s, B, 3, 32, graph=True, **kw).clone()
        _r1(net, tiny.w1)
        b = sample_tensor(net, s, B, 3, 32, graph=True, **kw).clone()
    sd = _cpu_sd(net)
    tiny.fresh_eval(sd)  # side condition 1 on tiny's W'
    ref = sample_tensor(tiny.fresh(sd).eval(), s, B, 3, 32, graph=False, **kw)
    print(f'graph sampling B={B} split={split}: vs fresh eager rel-L2 {rel_l2(b, ref):.3e}, moved by {rel_l2(b, a):.3e}')
    assert rel_l2(b, a) > 1e-3
    assert torch.equal(b, ref)


# ------------------------------------------------------------------ (d) training on updated weights
def _train_step(net, case):
    """zero_grad, forward, MSE, backward (train_ddpm.py:106-110, before optimizer.step): (loss, grads on the CPU)."""
    net.zero_grad()
    loss = torch.nn.MSELoss()(net(case.x.cuda(), case.t.cuda()), case.noise.cuda())
    loss.backward()
    return float(loss.detach()), {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}


def _autograd_oracle(life, sd):
    from oracle.unet_oracle import unet_forward
    c = life.case
    w = {k: v.detach().clone().double().requires_grad_(True) for k, v in sd.items()}
    loss = torch.nn.MSELoss()(unet_forward(w, life.mc, c.x.double(), c.t), c.noise.double())
    loss.backward()
    return float(loss.detach()), {k: w[k].grad for k in sd}


# (loss relative, overall, per tensor): test_unet_grads_tiny_vs_oracle_autograd and
# test_unet_grads_16bit_training_lines_vs_oracle_autograd
TRAIN_BOUNDS = {'f16x3': (1e-5, 1e-5, 1e-4), 'bf16x6': (1e-5, 1e-5, 1e-4), 'fp32': (1e-5, 1e-5, 1e-4),
                'f16': (1e-3, 2e-2, 1e-1), 'bf16': (8e-3, 6e-2, 3e-1)}


@gpu
@pytest.mark.parametrize('precision', list(TRAIN_BOUNDS))
def test_training_on_updated_weights_and_train_sample_train(tiny, precision):
    """(d): the reference loop (Adam, lr 1e-3) on one long-lived model.  At iterations 2 and 3 the loss and
    every gradient equal a fresh model's first step on the current weights bit for bit (a pack mixing old
    and new weights fails) and match float64 autograd at those weights; then eval + no_grad (the sampling of
    train_ddpm.py's sample_interval) equals a fresh eval model, and iteration 4, back in train mode, is
    checked like 2 and 3."""
    from weatherconverter_amd import forms
    line = precision in ('f16', 'bf16')
    kw = dict(train_precision=precision) if line else dict(precision=precision)
    lrel, overall, per_tensor = TRAIN_BOUNDS[precision]
    c = tiny.case
    with forms.using(check_gbound=True):
        net = tiny.long_lived(**kw).train()
        opt = torch.optim.Adam(net.parameters(), lr=1e-3)
        for it in (1, 2, 3, 4):
            loss, grads = _train_step(net, c)
            if it >= 2:
                sd = _cpu_sd(net)
                floss, fgrads = _train_step(tiny.fresh(sd, **kw).train(), c)
                diff = [k for k in grads if not torch.equal(grads[k], fgrads[k])]
                print(f'{precision} iteration {it}: loss {loss!r} (fresh {floss!r}), gradients differing from fresh: {diff[:6]}')
                assert loss == floss
                assert not diff, diff[:8]
                if it <= 3:
                    rloss, rgrads = _autograd_oracle(tiny, sd)
                    print(f'{precision} iteration {it}: float64 loss {rloss!r}')
                    assert abs(loss - rloss) <= lrel * abs(rloss), (loss, rloss)
                    _check({k: g.double() for k, g in grads.items()}, rgrads, per_tensor=per_tensor, overall=overall)
            opt.step()
            if it == 3:
                # train -> sample -> train
                sd = _cpu_sd(net)
                net.eval()
                with torch.no_grad():
                    y = net(c.x.cuda(), c.t.cuda()).cpu()
                yf = tiny.fresh_eval(sd, None if line else precision)
                print(f'{precision} eval after 3 steps: vs fresh rel-L2 {rel_l2(y, yf):.3e}')
                assert torch.equal(y, yf)
                net.train()


# ------------------------------------------------------------------ (e) forward, in-place change, backward
@gpu
@pytest.mark.parametrize('name', ['conv_out.weight', 'mids.0.resnet_conv_first.0.2.weight'])
def test_parameter_changed_between_forward_and_backward_raises(tiny, name):
    """(e): UnetTrainFunction saves the parameters so that autograd's version check fires.  conv_out.weight:
    the head's data gradient reads the live weight (wc_head_dgrad), so this is its only guard; a mid-block
    conv weight: its data-gradient pack is built lazily in the backward.  Afterwards a clean step equals a
    fresh model's."""
    c = tiny.case
    net = tiny.long_lived().train()
    loss = torch.nn.MSELoss()(net(c.x.cuda(), c.t.cuda()), c.noise.cuda())
    with torch.no_grad():
        dict(net.named_parameters())[name].mul_(1.01)
    with pytest.raises(RuntimeError, match='modified by an inplace operation'):
        loss.backward()
    del loss
    loss, grads = _train_step(net, c)
    floss, fgrads = _train_step(tiny.fresh(_cpu_sd(net)).train(), c)
    assert loss == floss
    diff = [k for k in grads if not torch.equal(grads[k], fgrads[k])]
    assert not diff, diff[:8]


# ------------------------------------------------------------------ (f) SrganEngine
def _srgan_sd(seed=0):
    from weatherconverter_amd.srgan_model.models import Generator
    from weatherconverter_amd.synthetic import init_synthetic_
    gen = Generator()
    init_synthetic_(gen, seed=seed)  # seed 0: the weights of tests/golden/guided.npz (its srgan_digest)
    return _cpu_sd(gen)


def _srgan(sd):
    from weatherconverter_amd.srgan_model.models import Generator
    gen = Generator()
    gen.load_state_dict(sd)
    return gen.eval()


SRGAN_CASES = {
    'prelu_slope': ['residual.3.block1.act.weight'],
    'depthwise_weight': ['residual.3.block1.cnn.depthwise.weight'],
    'pointwise_weight': ['residual.3.block2.cnn.pointwise.weight'],
    'bn_running_var': ['residual.3.block2.bn.running_var'],
    'bn_weight': ['convblock.bn.weight'],
    'r3_load_state_dict': None,
    'r9_data_copy_invalidate': None,
}


@gpu
@pytest.mark.parametrize('case', list(SRGAN_CASES))
def test_srgan_engine_after_weight_change(case):
    """(f): Generator on the golden weights, (2, 3, 20, 44) as test_srgan_hip_ragged_tiles_prelu_bn_vs_float64;
    after one forward one tensor alone is rewritten in place with three times its value (r1), or everything is
    replaced by the seed-1 weights through load_state_dict (r3) or through .data + invalidate_packs() (r9).  The
    BatchNorm buffer is folded into the pointwise pack, so the signature has to cover buffers.  The change must
    move the result by rel-L2 > 1e-4 for one tensor (as in (b); the smallest seen is 4.1e-4, the depthwise
    weight; fp32 noise here is 3e-8) and > 1e-3 for all of them."""
    sd0 = _srgan_sd()
    assert _digest(sd0) == str(np.load(os.path.join(GOLDEN, 'guided.npz'))['srgan_digest'])
    x = torch.rand((2, 3, 20, 44), generator=torch.Generator().manual_seed(7))
    gen = _srgan(sd0).cuda()
    names = SRGAN_CASES[case]
    with torch.no_grad():
        y0 = gen(x.cuda()).cpu()
        live = gen.state_dict()
        if names is not None:
            assert set(names) <= set(live)
            for k in names:
                live[k].copy_(sd0[k] * 3)
        else:
            new = _srgan_sd(seed=1)
            if case == 'r3_load_state_dict':
                gen.load_state_dict(new)
            else:
                for k, v in live.items():
                    v.data.copy_(new[k])
                gen.invalidate_packs()
        y1 = gen(x.cuda()).cpu()
        sd = _cpu_sd(gen)
        yf = _srgan(sd).cuda()(x.cuda()).cpu()
        ref = _srgan(sd).double()(x.double())
    err = rel_l2(yf, ref)
    print(f'srgan {case}: fresh vs float64 {err:.3e}, vs fresh {rel_l2(y1, yf):.3e}, moved by {rel_l2(y1, y0):.3e}')
    assert err < 1e-5
    assert rel_l2(yf, y0) > (1e-4 if names is not None else 1e-3)  # a stale engine would repeat y0
    assert torch.equal(y1, yf)


# ------------------------------------------------------------------ (g) OldUnetEngine
def _old_unet(sd=None, seed=0):
    from weatherconverter_amd.diffusion_model.models.old_modules import UNet
    from weatherconverter_amd.synthetic import init_synthetic_
    net = UNet()
    if sd is None:
        init_synthetic_(net, seed=seed)
    else:
        net.load_state_dict(sd)
    return net


OLD_BN_VAR = 'down2.residual_blocks.0.double_conv.0.running_var'


@gpu
@pytest.mark.parametrize('route', ['r1_copy_', 'r3_load_state_dict', 'r9_data_copy_invalidate', 'r1_bn_running_var_alone'])
def test_old_unet_engine_after_weight_change(route):
    """(g): the 128-px old UNet, B = 1, on tests/test_old_unet.py's input.  Every case ENDS on the golden
    (seed-0) weights, so that the fresh model has a reference: tests/golden/old_unet.npz at that file's bound,
    rel-L2 < 1e-5.  The long-lived model starts on the seed-1 weights and receives every parameter and buffer by
    r1, r3 or r9; or it starts on the golden weights with one BatchNorm running_var x 3 and that buffer alone
    is put right (r1): the engine folds the running statistics into its packs, so its signature has to cover
    buffers.  The change must move the result by rel-L2 > 1e-3 (the buffer alone: > 1e-4, as in (b))."""
    from weatherconverter_amd.synthetic import synthetic_images
    golden = np.load(os.path.join(GOLDEN, 'old_unet.npz'))
    x = synthetic_images((1, 3, 128, 128), seed=501).cuda()
    t = torch.tensor([[[[0.2860]]]]).cuda()
    new = _cpu_sd(_old_unet(seed=0))
    assert _digest(new) == str(golden['digest'])
    one = route == 'r1_bn_running_var_alone'
    net = _old_unet(seed=0 if one else 1)
    if one:
        with torch.no_grad():
            net.state_dict()[OLD_BN_VAR].mul_(3)
    net = net.cuda().eval()
    with torch.no_grad():
        y0 = net(x, t).cpu()
        if route == 'r1_copy_':
            for k, v in net.state_dict().items():
                v.copy_(new[k])
        elif route == 'r3_load_state_dict':
            net.load_state_dict(new)
        elif route == 'r9_data_copy_invalidate':
            for k, v in net.state_dict().items():
                v.data.copy_(new[k])
            net.invalidate_packs()
        else:
            net.state_dict()[OLD_BN_VAR].copy_(new[OLD_BN_VAR])
        y1 = net(x, t).cpu()
        sd = _cpu_sd(net)
        yf = _old_unet(sd).cuda().eval()(x, t).cpu()
    err = rel_l2(yf, golden['y'])
    print(f'old UNet {route}: fresh vs golden {err:.3e}, vs fresh {rel_l2(y1, yf):.3e}, moved by {rel_l2(yf, y0):.3e}')
    assert _digest(sd) == str(golden['digest'])
    assert err < 1e-5
    assert rel_l2(yf, y0) > (1e-4 if one else 1e-3)
    assert torch.equal(y1, yf)


# ------------------------------------------------------------------ (h) CPU: the torch facts the contract rests on
def test_torch_version_counter_facts():
    """The engines' staleness test is (data_ptr, _version) per parameter.  It sees what moves one of the two:
    in-place ops under no_grad or on a detach(), load_state_dict, an optimizer step (the version), rebinding
    .data (the pointer).  It cannot see in-place writes THROUGH .data, which move neither -- hence
    invalidate_packs().  If a torch upgrade changes any of this, the documented contract changes with it."""
    lin = torch.nn.Linear(4, 3)
    p = lin.weight
    v, ptr = p._version, p.data_ptr()
    p.data.mul_(2)
    p.data.copy_(torch.ones(3, 4))
    assert (p._version, p.data_ptr()) == (v, ptr), INTEGRATION_NOTE
    with torch.no_grad():
        p.mul_(2)
    assert p._version > v and p.data_ptr() == ptr, INTEGRATION_NOTE
    v = p._version
    p.detach().add_(1)
    assert p._version > v, INTEGRATION_NOTE
    v = p._version
    lin.load_state_dict({k: t.clone() + 1 for k, t in lin.state_dict().items()})
    assert lin.weight is p and p._version > v and p.data_ptr() == ptr, INTEGRATION_NOTE
    v = p._version
    p.grad = torch.ones_like(p)
    lin.bias.grad = torch.ones_like(lin.bias)
    for opt in (torch.optim.SGD(lin.parameters(), lr=0.1), torch.optim.Adam(lin.parameters(), lr=0.1)):
        opt.step()
        assert p._version > v, INTEGRATION_NOTE
        v = p._version
    new = torch.zeros(3, 4)
    p.data = new
    assert p.data_ptr() == new.data_ptr() != ptr, INTEGRATION_NOTE
    # assign=True replaces the Parameter objects: new pointers (the caller's tensors), versions from zero
    sd = {k: t.clone() for k, t in lin.state_dict().items()}
    lin.load_state_dict(sd, assign=True)
    assert lin.weight is not p and lin.weight.data_ptr() == sd['weight'].data_ptr(), INTEGRATION_NOTE


def test_invalidate_packs_drops_every_engine():
    """invalidate_packs() exists on the three engine-backed modules, drops what they cache, returns self."""
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.old_modules import UNet
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.srgan_model.models import Generator
    net = Unet(ModelConfig(**_tiny_config()))
    net._engine, net._train_engine = object(), object()
    assert net.invalidate_packs() is net and net._engine is None and net._train_engine is None
    for mod in (UNet(), Generator(num_blocks=1)):
        mod._engine = object()
        assert mod.invalidate_packs() is mod and mod._engine is None
