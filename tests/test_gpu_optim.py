"""GPU: diffusion_model.optim.Adam (wc_adam_step, wc_grad_norm) against torch.optim.Adam and float64.

The yardstick of every numerical check: the same steps are run three ways from identical fp32 inputs --
with optim.Adam, with torch.optim.Adam in fp32 on the GPU, and with a float64 restatement of the
formula (adam_f64 below) -- and for each of p, exp_avg, exp_avg_sq and the displacement p_after -
p_before, over all tensors together, our rel-L2 error against float64 may be at most 2x torch's
against the same float64 (the margin is for rounding order only).
"""
import copy
import json
import os
from types import SimpleNamespace

import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
MODES = {'adam': dict(), 'l2': dict(weight_decay=1e-2), 'adamw': dict(weight_decay=1e-2, decoupled_weight_decay=True)}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _grad(n, g, scale=1.0):
    """n gradient values with per-element magnitudes over 1e-9 .. 10 (|value| >= 5e-10 * scale)."""
    mag = 10.0**(torch.rand(n, generator=g, dtype=torch.float64) * 10 - 9) * (0.5 + 0.5 * torch.rand(n, generator=g))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    return (mag * sign * scale).float()


def adam_f64(p, m, v, g, step, *, lr=LR, betas=BETAS, eps=EPS, weight_decay=0.0, decoupled_weight_decay=False,
             clip=1.0):
    """One Adam / AdamW step in float64 (the formula of the issue and of torch/optim/adam.py)."""
    p, m, v, g = (t.double() for t in (p, m, v, g))
    g = g * clip
    if weight_decay:
        if decoupled_weight_decay:
            p = p * (1 - lr * weight_decay)
        else:
            g = g + weight_decay * p
    m = m + (1 - betas[0]) * (g - m)
    v = betas[1] * v + (1 - betas[1]) * g * g
    bc1, bc2 = 1 - betas[0]**step, 1 - betas[1]**step
    p = p - (lr / bc1) * m / (v.sqrt() / bc2**0.5 + eps)
    return p, m, v


def _cat(ts):
    return torch.cat([t.detach().double().cpu().reshape(-1) for t in ts])


def assert_yardstick(ours, theirs, ref, before, label):
    """ours / theirs / ref: (ps, ms, vs) lists after the steps; before: the ps they all started from."""
    b = _cat(before)
    figures = {}
    for name, k in (('p', 0), ('exp_avg', 1), ('exp_avg_sq', 2)):
        figures[name] = (rel_l2(_cat(ours[k]), _cat(ref[k])), rel_l2(_cat(theirs[k]), _cat(ref[k])))
    figures['displacement'] = (rel_l2(_cat(ours[0]) - b, _cat(ref[0]) - b), rel_l2(_cat(theirs[0]) - b, _cat(ref[0]) - b))
    for name, (eo, et) in figures.items():
        print(f'{label} {name}: ours {eo:.3e} torch {et:.3e} ratio {eo / max(et, 1e-300):.3f}')
    for name, (eo, et) in figures.items():
        assert eo <= 2 * et, (label, name, eo, et)


def _state(opt, ps):
    return [opt.state[p]['exp_avg'] for p in ps], [opt.state[p]['exp_avg_sq'] for p in ps]


def three_ways(p0, grads, Ours, Theirs=torch.optim.Adam, ours_kw=None, theirs_kw=None, f64_kw=None, before_torch=None):
    """Run len(grads) steps from the fp32 CPU tensors p0 with per-step gradient lists; returns
    (ours, theirs, ref) as (ps, ms, vs) and the optimizer of ours."""
    po = [torch.nn.Parameter(p.clone().cuda()) for p in p0]
    pt = [torch.nn.Parameter(p.clone().cuda()) for p in p0]
    oo, ot = Ours(po, lr=LR, betas=BETAS, eps=EPS, **(ours_kw or {})), Theirs(pt, lr=LR, betas=BETAS, eps=EPS,
                                                                             **(theirs_kw or {}))
    r = ([p.double() for p in p0], [torch.zeros_like(p, dtype=torch.float64) for p in p0],
         [torch.zeros_like(p, dtype=torch.float64) for p in p0])
    for k, gs in enumerate(grads, 1):
        for a, b, g in zip(po, pt, gs):
            a.grad, b.grad = g.clone().cuda(), g.clone().cuda()
        oo.step()
        if before_torch is not None:
            before_torch(pt)
        ot.step()
        kw = f64_kw(gs) if callable(f64_kw) else (f64_kw or {})
        new = [adam_f64(p, m, v, g, k, **kw) for p, m, v, g in zip(*r, gs)]
        r = tuple([n[i] for n in new] for i in range(3))
    return (po, *_state(oo, po)), (pt, *_state(ot, pt)), r, oo


# --------------------------------------------------------------------------------------- 1: synthetic list
CHUNK = 4096
# (elements, misalignment of p in floats, of g): sizes around the 4-wide vector and the chunk, every
# combination of 16-byte and 4-byte aligned operands at small and at multi-chunk sizes
CARVE = [(1, 0, 0), (3, 1, 1), (4, 0, 0), (5, 0, 0), (63, 1, 0), (64, 0, 1), (1023, 0, 0), (1024, 1, 1), (CHUNK, 0, 0),
         (CHUNK + 1, 0, 0), (3 * CHUNK + 1, 0, 0), (70001, 0, 0), (CHUNK + 1, 3, 2), (2 * CHUNK + 3, 2, 0),
         (777, 0, 0), (1500, 0, 0)]
NONE_GRAD, ZERO_GRAD = 14, 15  # rows of CARVE: .grad is None / an all-zero gradient
SENTINEL = -1234.5678


def _offsets(mis):
    """Start of each view (in floats): a multiple of 4 plus the wanted misalignment, at least one float
    of gap after the previous view."""
    offs, cur = [], 3
    for (n, *_), d in zip(CARVE, mis):
        o = (cur + 1 + 3) // 4 * 4 + d
        offs.append(o)
        cur = o + n
    return offs, cur + 5


@pytest.fixture(scope='module')
def synthetic():
    from weatherconverter_amd import _native
    assert _native.load().wc_optim_chunk_elems() == CHUNK  # the sizes above are chosen around it
    g = _gen(11)
    p0 = [torch.randn(n, generator=g) for n, _, _ in CARVE]
    grads = [[torch.zeros(n) if i == ZERO_GRAD else _grad(n, g) for i, (n, _, _) in enumerate(CARVE)] for _ in range(5)]
    return p0, grads


def _run_synthetic(p0, grads, **kw):
    """Five steps of ours on views carved out of two sentinel-filled buffers; returns what the checks need."""
    from weatherconverter_amd.diffusion_model.optim import Adam
    poff, pend = _offsets([c[1] for c in CARVE])
    goff, gend = _offsets([c[2] for c in CARVE])
    pbuf = torch.full((pend, ), SENTINEL, device='cuda')
    gbuf = torch.full((gend, ), SENTINEL, device='cuda')
    assert pbuf.data_ptr() % 16 == 0 and gbuf.data_ptr() % 16 == 0
    pmask, gmask = torch.ones(pend, dtype=torch.bool), torch.ones(gend, dtype=torch.bool)
    ps, gviews = [], []
    for (n, dp, dg), o, og, p in zip(CARVE, poff, goff, p0):
        pbuf[o:o + n] = p.cuda()
        ps.append(torch.nn.Parameter(pbuf[o:o + n]))
        gviews.append(gbuf[og:og + n])
        pmask[o:o + n] = False
        gmask[og:og + n] = False
        assert ps[-1].data_ptr() % 16 == 4 * dp and gviews[-1].data_ptr() % 16 == 4 * dg
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS, **kw)
    after_first = None
    for gs in grads:
        for i, (p, gv, gval) in enumerate(zip(ps, gviews, gs)):
            gv.copy_(gval)
            p.grad = None if i == NONE_GRAD else gv
        gsnap = gbuf.clone()
        opt.step()
        assert torch.equal(gbuf.view(torch.int32), gsnap.view(torch.int32))  # the gradient buffer is only read
        if after_first is None:
            after_first = [p.detach().clone() for p in ps]
    sent = torch.tensor(SENTINEL).cuda()
    assert torch.equal(pbuf[pmask.cuda()], sent.expand(int(pmask.sum())))  # nothing written outside a tensor
    assert torch.equal(gbuf[gmask.cuda()], sent.expand(int(gmask.sum())))
    return ps, opt, after_first


@pytest.mark.parametrize('mode', list(MODES))
def test_synthetic_list_five_steps(synthetic, mode):
    from weatherconverter_amd.diffusion_model.optim import Adam
    p0, grads = synthetic
    kw = MODES[mode]
    ps, opt, after_first = _run_synthetic(p0, grads, **kw)
    live = [i for i in range(len(CARVE)) if i != NONE_GRAD]
    # the tensor without a gradient: no state, not a bit changed
    assert ps[NONE_GRAD] not in opt.state and torch.equal(ps[NONE_GRAD].detach().cpu(), p0[NONE_GRAD])
    assert all(float(opt.state[ps[i]]['step']) == 5.0 for i in live)
    assert all(opt.state[ps[i]]['step'].device.type == 'cpu' and opt.state[ps[i]]['step'].dtype == torch.float32
               and opt.state[ps[i]]['step'].dim() == 0 for i in live)
    if mode == 'adam':  # m = v = 0 and p - lr * 0 / (0 + eps) = p
        assert torch.equal(after_first[ZERO_GRAD].cpu(), p0[ZERO_GRAD])
    # the same steps with torch and in float64, on plain (aligned) tensors
    ours_plain, theirs, ref, _ = three_ways([p0[i] for i in live], [[gs[i] for i in live] for gs in grads], Adam,
                                            ours_kw=kw, theirs_kw=kw, f64_kw=kw)
    carved = ([ps[i] for i in live], *_state(opt, [ps[i] for i in live]))
    assert_yardstick(carved, theirs, ref, [p0[i] for i in live], f'synthetic[{mode}]')
    # alignment picks the access width, never the arithmetic: carved views == plain tensors, bit for bit
    for a, b in zip(carved, ours_plain):
        assert all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))
    # rounding p five times bounds each tensor's own error (5 * 2^-24, displacement error far below)
    for i, p, r in zip(live, carved[0], ref[0]):
        assert rel_l2(p.detach(), r) <= 2.0**-21, (CARVE[i], rel_l2(p.detach(), r))


# --------------------------------------------------------------------------------------- 2: determinism
def test_two_runs_are_bit_identical(synthetic):
    p0, grads = synthetic
    runs = []
    for _ in range(2):
        ps, opt, _ = _run_synthetic(p0, grads, weight_decay=1e-2, max_grad_norm=5.0)
        live = [p for i, p in enumerate(ps) if i != NONE_GRAD]
        runs.append([t.detach().clone() for t in (*live, *_state(opt, live)[0], *_state(opt, live)[1], opt.grad_norm)])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*runs))


# --------------------------------------------------------------------------------------- 3: one launch
def test_one_launch_per_group(monkeypatch):
    from weatherconverter_amd import _native
    from weatherconverter_amd.diffusion_model.optim import Adam
    g = _gen(3)
    sizes = [1 + (37 * i) % 200 for i in range(320)] + [5000]
    ps = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in sizes]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    calls = {}
    real = _native.call

    def counting(name, *args):
        calls[name] = calls.get(name, 0) + 1
        return real(name, *args)
    monkeypatch.setattr(_native, 'call', counting)
    before = [p.detach().clone() for p in ps]
    opt = Adam(ps, lr=LR)
    opt.step()
    assert calls == {'wc_adam_step': 1}
    assert all(not torch.equal(a, p.detach()) for a, p in zip(before, ps))  # every tensor was reached
    calls.clear()
    opt.max_grad_norm = 1.0
    opt.step()
    assert calls == {'wc_grad_norm': 1, 'wc_adam_step': 1}
    calls.clear()
    two = Adam([{'params': ps[:100], 'lr': 1e-2}, {'params': ps[100:]}], max_grad_norm=1.0)
    two.step()
    assert calls == {'wc_grad_norm': 1, 'wc_adam_step': 2}  # one global norm, one launch per group


def test_operands_outside_the_kernels_envelope_raise():
    from weatherconverter_amd.diffusion_model.optim import Adam
    p = torch.nn.Parameter(torch.randn(8, 6).cuda().half())
    p.grad = torch.ones_like(p)
    with pytest.raises(RuntimeError, match='fp32'):
        Adam([p]).step()
    q = torch.nn.Parameter(torch.randn(8, 6).cuda().t())
    q.grad = torch.ones_like(q)
    with pytest.raises(RuntimeError, match='contiguous'):
        Adam([q]).step()
    c = torch.nn.Parameter(torch.randn(4))
    c.grad = torch.ones(4)
    with pytest.raises(RuntimeError, match='fp32 tensor on'):
        Adam([c]).step()


# --------------------------------------------------------------------------------------- 4: clipping
@pytest.fixture(scope='module')
def cliplist():
    g = _gen(21)
    sizes = [1, 7, 64, 1000, CHUNK + 1, 30001]
    p0 = [torch.randn(n, generator=g) for n in sizes]
    grads = [[_grad(n, g) for n in sizes] for _ in range(3)]
    return p0, grads


def test_clipping_by_global_norm(cliplist):
    from weatherconverter_amd.diffusion_model.optim import Adam
    p0, grads = cliplist
    norm64 = float(_cat(grads[0]).norm())
    max_norm = norm64 / 10  # the norm is about 10x max_grad_norm

    def clip_torch(pt):
        torch.nn.utils.clip_grad_norm_(pt, max_norm)
    ours, theirs, ref, opt = three_ways(
        p0, grads, Adam, ours_kw=dict(max_grad_norm=max_norm), before_torch=clip_torch,
        f64_kw=lambda gs: dict(clip=min(1.0, max_norm / (float(_cat(gs).norm()) + 1e-6))))
    assert_yardstick(ours, theirs, ref, p0, 'clipped')
    # fp64 accumulation: only the final rounding to fp32 remains
    n64 = float(_cat(grads[-1]).norm())
    assert opt.grad_norm.dim() == 0 and opt.grad_norm.is_cuda and opt.grad_norm.dtype == torch.float32
    assert abs(float(opt.grad_norm) - n64) <= 2.0**-23 * n64
    # .grad is left as the backward wrote it
    assert all(torch.equal(p.grad.cpu(), g) for p, g in zip(ours[0], grads[-1]))


def test_norm_below_the_limit_is_the_unclipped_step(cliplist):
    from weatherconverter_amd.diffusion_model.optim import Adam
    p0, grads = cliplist
    big = 2 * max(float(_cat(gs).norm()) for gs in grads)
    res = []
    for kw in (dict(), dict(max_grad_norm=big)):
        ps = [torch.nn.Parameter(p.clone().cuda()) for p in p0]
        opt = Adam(ps, lr=LR, **kw)
        for gs in grads:
            for p, g in zip(ps, gs):
                p.grad = g.clone().cuda()
            opt.step()
        res.append([t.detach() for t in (*ps, *_state(opt, ps)[0], *_state(opt, ps)[1])])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*res))


def test_non_finite_norm_propagates():
    from weatherconverter_amd.diffusion_model.optim import Adam
    p = torch.nn.Parameter(torch.ones(10).cuda())
    p.grad = torch.full((10, ), float('nan')).cuda()
    opt = Adam([p], max_grad_norm=1.0)
    opt.step()
    assert torch.isnan(opt.grad_norm) and torch.isnan(p).all()  # as clip_grad_norm_(error_if_nonfinite=False) + Adam


# --------------------------------------------------------------------------------------- 5: interop
@pytest.mark.parametrize('first', ['ours', 'torch'])
def test_state_dict_moves_between_the_optimizers(cliplist, first):
    from weatherconverter_amd.diffusion_model.optim import Adam
    p0, grads = cliplist
    A, B = (Adam, torch.optim.Adam) if first == 'ours' else (torch.optim.Adam, Adam)
    pa = [torch.nn.Parameter(p.clone().cuda()) for p in p0]
    oa = A(pa, lr=LR, betas=BETAS, eps=EPS, weight_decay=1e-2)
    for gs in grads[:2]:
        for p, g in zip(pa, gs):
            p.grad = g.clone().cuda()
        oa.step()
    # the hand-over point: the fp32 state all three third steps start from
    start = [p.detach().clone().cpu() for p in pa]
    m0, v0 = ([t.clone().cpu() for t in ts] for ts in _state(oa, pa))
    pb = [torch.nn.Parameter(p.clone().cuda()) for p in start]
    ob = B(pb, lr=0.5)  # every hyper-parameter comes from the loaded groups
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert ob.param_groups[0]['lr'] == LR and ob.param_groups[0]['weight_decay'] == 1e-2
    assert all(float(ob.state[p]['step']) == 2.0 for p in pb)
    for p, q, g in zip(pa, pb, grads[2]):
        p.grad, q.grad = g.clone().cuda(), g.clone().cuda()
    oa.step()
    ob.step()
    ref = [adam_f64(p, m, v, g, 3, weight_decay=1e-2) for p, m, v, g in zip(start, m0, v0, grads[2])]
    ref = tuple([r[i] for r in ref] for i in range(3))
    ra, rb = (pa, *_state(oa, pa)), (pb, *_state(ob, pb))
    ours, theirs = (ra, rb) if first == 'ours' else (rb, ra)
    assert_yardstick(ours, theirs, ref, start, f'third step after {first}')


# --------------------------------------------------------------------------------------- 6: tiny UNet
def _tiny():
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.synthetic import init_synthetic_
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    mc = ModelConfig(**man['tiny']['config'])
    net = Unet(mc)
    init_synthetic_(net, seed=0)
    g = _gen(5)
    x = torch.randn((2, 3, 32, 32), generator=g).cuda()
    noise = torch.randn((2, 3, 32, 32), generator=g).cuda()
    t = torch.tensor([5, 700]).cuda()
    return mc, net.cuda().train(), x, noise, t


def _fresh_copy(mc, net):
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    other = Unet(mc)
    other.load_state_dict({k: v.detach().clone().cpu() for k, v in net.state_dict().items()})
    return other.cuda()


def test_tiny_unet_step_under_the_yardstick():
    from weatherconverter_amd.diffusion_model.optim import Adam
    mc, net, x, noise, t = _tiny()
    torch.nn.MSELoss()(net(x, t), noise).backward()
    ps = list(net.parameters())
    p0 = [p.detach().clone().cpu() for p in ps]
    grads = [p.grad.detach().clone().cpu() for p in ps]
    versions = [p._version for p in ps]
    opt = Adam(ps, lr=LR, betas=BETAS, eps=EPS)
    opt.step()
    assert all(p._version > v for p, v in zip(ps, versions))
    pt = [torch.nn.Parameter(p.clone().cuda()) for p in p0]
    for p, g in zip(pt, grads):
        p.grad = g.clone().cuda()
    ot = torch.optim.Adam(pt, lr=LR, betas=BETAS, eps=EPS)
    ot.step()
    ref = [adam_f64(p, torch.zeros_like(p), torch.zeros_like(p), g, 1) for p, g in zip(p0, grads)]
    ref = tuple([r[i] for r in ref] for i in range(3))
    assert_yardstick((ps, *_state(opt, ps)), (pt, *_state(ot, pt)), ref, p0, 'tiny UNet')


def test_forward_after_step_runs_on_the_updated_weights():
    """The stale-pack test: the engines cache packed weights keyed on the parameters' version counters,
    and wc_adam_step writes through raw addresses -- without step()'s version bump the next forward
    would silently run on the packs of the old weights."""
    from weatherconverter_amd.diffusion_model.optim import Adam
    mc, net, x, noise, t = _tiny()
    opt = Adam(net.parameters(), lr=1e-3)
    for _ in range(2):  # after the first step, and again after a second
        opt.zero_grad()
        torch.nn.MSELoss()(net(x, t), noise).backward()
        opt.step()
        out = net(x, t).detach()
        assert torch.equal(out, _fresh_copy(mc, net).train()(x, t).detach())
    with torch.no_grad():
        before = net.eval()(x, t)  # the inference engine packs these weights ...
    opt.zero_grad()
    torch.nn.MSELoss()(net.train()(x, t), noise).backward()
    opt.step()  # ... and this step replaces them
    with torch.no_grad():
        out = net.eval()(x, t)
        assert not torch.equal(out, before)
        assert torch.equal(out, _fresh_copy(mc, net).eval()(x, t))


def test_reference_loop_with_make_optimizer(tmp_path):
    from weatherconverter_amd.diffusion_model import train_ddpm
    from weatherconverter_amd.diffusion_model.optim import Adam
    mc, net, x, noise, t = _tiny()
    opt = train_ddpm.make_optimizer(net, SimpleNamespace(training=SimpleNamespace(lr=1e-4)))
    assert type(opt) is Adam
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.MSELoss()(net(x, t), noise)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    assert all(torch.isfinite(torch.tensor(losses))) and losses[-1] < losses[0]
    # the reference's checkpoint (weights_only loader) round-trips the optimizer, into either class
    path = train_ddpm.save_checkpoint(7, net, opt, str(tmp_path))
    for cls in (Adam, torch.optim.Adam):
        net2 = _fresh_copy(mc, net)
        opt2 = cls(net2.parameters(), lr=0.5)
        _, _, epoch = train_ddpm.load_checkpoint(net2, opt2, path)
        assert epoch == 7 and opt2.param_groups[0]['lr'] == 1e-4
        for p, q in zip(net.parameters(), net2.parameters()):
            assert torch.equal(p, q) and float(opt2.state[q]['step']) == 3.0
            assert torch.equal(opt.state[p]['exp_avg'], opt2.state[q]['exp_avg'])
            assert torch.equal(opt.state[p]['exp_avg_sq'], opt2.state[q]['exp_avg_sq'])
    # a forward, then a step, then that forward's backward: autograd's saved-tensor check sees the update
    loss = torch.nn.MSELoss()(net(x, t), noise)
    opt.step()
    with pytest.raises(RuntimeError):
        loss.backward()
