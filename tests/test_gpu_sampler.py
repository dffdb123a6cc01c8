"""GPU: the strided sampling step (wc_ddim_step) against float64, its bitwise properties, and the loops
built on it: sample_tensor(steps=...), ddim_invert, sample_sharded and the strided guided loop.

Tolerance of every comparison with float64 (derived, not tuned): the kernel applies at most 8 roundings
to intermediates bounded by the sum of the absolute terms, so |x' - ref| <= 8 * 2^-24 * S with
S = sqrt_acp_to * A0 + c_dir * AE + sigma * |z|, A0 = (|x| + s1m |eps|) / sa, AE = |eps|, and for the
elements the clamp changed A0 = 1, AE = (|x| + sa) / s1m.  A numpy fp32 evaluation of the same formula
stays below 0.55 of it over every case here.
"""
import json
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

EPS32 = 2.0**-24
TRANSITIONS = [(999, 949), (999, 998), (500, 480), (20, 0), (1, 0), (0, -1), (0, 20), (480, 500)]
SHAPES = [(2, 3, 8, 8), (3, 1, 2, 2)]  # the second: one float4 per sample (grid tail, per-sample Philox counter)
ETAS = [0.0, 0.5, 1.0]
NONE, TENSOR, PHILOX = 0, 1, 2
SEED, SAMPLE0 = 1234, 3


def _K():
    from weatherconverter_amd import kernels
    return kernels


def _sched(T=1000):
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    return LinearNoiseScheduler(T, 0.0001, 0.02)


@pytest.fixture(scope='module')
def sched():
    return _sched()


_INPUTS = {}


def _inputs(shape):
    """x, eps, z ~ N(0, 1) from a seeded CPU generator, on the device; made once per shape, never written."""
    if shape not in _INPUTS:
        g = torch.Generator().manual_seed(20)
        _INPUTS[shape] = tuple(torch.randn(shape, generator=g).cuda() for _ in range(3))
    return _INPUTS[shape]


def ref_step(x, eps, z, scalars, clip):
    """The transition in float64 from the fp32 scalars and inputs, with the bounds of the module docstring."""
    sa, s1m, sa_to, c_dir, sigma = scalars
    x, eps = x.double().cpu().numpy(), eps.double().cpu().numpy()
    z = np.zeros_like(x) if z is None else z.double().cpu().numpy()
    x0 = (x - s1m * eps) / sa
    A0, AE = (np.abs(x) + s1m * np.abs(eps)) / sa, np.abs(eps)
    changed = np.zeros(x.shape, bool)
    e = eps
    if clip:
        c = np.clip(x0, -1.0, 1.0)
        changed = c != x0
        x0 = c
        e = np.where(changed, (x - sa * x0) / s1m, eps)
        A0 = np.where(changed, 1.0, A0)
        AE = np.where(changed, (np.abs(x) + sa) / s1m, AE)
    mean = sa_to * x0 + c_dir * e
    Sm = sa_to * A0 + c_dir * AE
    return dict(xp=mean + sigma * z, mean=mean, x0=x0, changed=changed, b_xp=8 * EPS32 * (Sm + sigma * np.abs(z)),
                b_mean=8 * EPS32 * Sm, b_x0=8 * EPS32 * A0)


def _within(got, want, bound, what):
    err = np.abs(got.double().cpu().numpy() - want)
    assert np.all(np.isfinite(err)), what
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    assert worst <= 1.0, (what, worst)


def _step(x, eps, scalars, *, clip=False, mode=NONE, z=None, step=0, sample0=SAMPLE0, out=None, sz=False, x0=False):
    """One K.ddim_step into NaN-poisoned outputs; returns (x_out, sz_out, x0_out)."""
    nan = lambda: torch.full_like(x, float('nan'))  # noqa: E731
    out = nan() if out is None else out
    szo, x0o = (nan() if sz else None), (nan() if x0 else None)
    _K().ddim_step(x, eps, out, *scalars, clip_x0=clip, z=z if mode == TENSOR else None, mode=mode, seed=SEED,
                   sample0=sample0, step=step, sz_out=szo, x0_out=x0o)
    return out, szo, x0o


# --------------------------------------------------------------------------------------- kernel vs float64
@pytest.mark.parametrize('mode', [NONE, TENSOR, PHILOX])
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_against_float64(sched, shape, mode):
    K = _K()
    x, eps, zt = _inputs(shape)
    for t, t_to in TRANSITIONS:
        z = {NONE: None, TENSOR: zt, PHILOX: K.philox_normal(shape, x.device, SEED, SAMPLE0, t)}[mode]
        for eta in ETAS:
            scalars = sched.ddim_scalars(t, t_to, eta)
            for clip in (False, True):
                what = (shape, mode, t, t_to, eta, clip)
                ref = ref_step(x, eps, z, scalars, clip)
                out, _, _ = _step(x, eps, scalars, clip=clip, mode=mode, z=z, step=t)
                _within(out, ref['xp'], ref['b_xp'], what)
                if clip and shape == SHAPES[0] and (t, t_to) in ((999, 949), (20, 0)):
                    assert ref['changed'].any() and not ref['changed'].all(), what


@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_outputs_against_float64(sched, shape):
    """The (mean, sigma*z) form, the x0 output and x_out aliasing x."""
    K = _K()
    x, eps, zt = _inputs(shape)
    for t, t_to in TRANSITIONS:
        for eta in (0.0, 1.0):
            scalars = sched.ddim_scalars(t, t_to, eta)
            sigma32 = np.float32(scalars[4])
            for clip in (False, True):
                for mode in (TENSOR, PHILOX):
                    what = (shape, mode, t, t_to, eta, clip)
                    z = zt if mode == TENSOR else K.philox_normal(shape, x.device, SEED, SAMPLE0, t)
                    ref = ref_step(x, eps, z, scalars, clip)
                    mean, sz, x0 = _step(x, eps, scalars, clip=clip, mode=mode, z=z, step=t, sz=True, x0=True)
                    _within(mean, ref['mean'], ref['b_mean'], what + ('mean', ))
                    _within(x0, ref['x0'], ref['b_x0'], what + ('x0', ))
                    assert np.array_equal(sz.cpu().numpy(), sigma32 * z.cpu().numpy()), what  # one fp32 product
                    if clip:
                        assert float(x0.abs().max()) <= 1.0
                    # x_out aliasing x: every lane loads before it stores
                    fused, _, _ = _step(x, eps, scalars, clip=clip, mode=mode, z=z, step=t)
                    xa = x.clone()
                    _step(xa, eps, scalars, clip=clip, mode=mode, z=z, step=t, out=xa)
                    assert torch.equal(xa, fused), what
                    # x_out + sz_out, added in fp32 on the device, is the fused x'
                    assert torch.equal(mean + sz, fused), what


# --------------------------------------------------------------------------------------- bitwise properties
def test_philox_mode_equals_tensor_mode(sched):
    K = _K()
    for shape in SHAPES:
        x, eps, _ = _inputs(shape)
        for t, t_to in ((999, 949), (20, 0), (1, 0)):
            scalars = sched.ddim_scalars(t, t_to, 1.0)
            z = K.philox_normal(shape, x.device, SEED, SAMPLE0, t)
            a, _, _ = _step(x, eps, scalars, mode=PHILOX, step=t)
            b, _, _ = _step(x, eps, scalars, mode=TENSOR, z=z)
            assert torch.equal(a, b), (shape, t)
            # the noise is ddpm_step's for the same key
            d = torch.empty_like(x)
            sz = torch.empty_like(x)
            K.ddpm_step(x, eps, d, 0.01, 0.5, 0.99, 1.0, mode=PHILOX, seed=SEED, sample0=SAMPLE0, step=t, sz_out=sz)
            assert torch.equal(sz, z)


def test_rows_do_not_depend_on_the_sharding(sched):
    g = torch.Generator().manual_seed(21)
    for per in ((3, 8, 8), (1, 2, 2)):
        x, eps = (torch.randn((4, ) + per, generator=g).cuda() for _ in range(2))
        scalars = sched.ddim_scalars(500, 480, 1.0)
        full, _, _ = _step(x, eps, scalars, mode=PHILOX, step=500, sample0=0)
        part, _, _ = _step(x[2:].contiguous(), eps[2:].contiguous(), scalars, mode=PHILOX, step=500, sample0=2)
        assert torch.equal(full[2:], part)


def test_clip_that_changes_nothing_is_bitwise_off(sched):
    x, eps, z = _inputs(SHAPES[0])
    for t, t_to in ((500, 480), (20, 0), (0, -1)):
        scalars = sched.ddim_scalars(t, t_to, 1.0)
        sa, s1m = scalars[0], scalars[1]
        scale = 0.9 * sa / float((x.abs() + s1m * eps.abs()).max())  # |x0| <= 0.9
        xs, es = x * scale, eps * scale
        on = _step(xs, es, scalars, clip=True, mode=TENSOR, z=z, sz=True, x0=True)
        off = _step(xs, es, scalars, clip=False, mode=TENSOR, z=z, sz=True, x0=True)
        assert float(off[2].abs().max()) < 1.0
        assert all(torch.equal(a, b) for a, b in zip(on, off))


def test_every_output_is_fully_written(sched):
    """x_out, sz_out and x0_out start as NaN (in _step) and hold none afterwards, in every noise mode."""
    for shape in SHAPES + [(5, 1, 2, 6)]:
        g = torch.Generator().manual_seed(22)
        x, eps, z = (torch.randn(shape, generator=g).cuda() for _ in range(3))
        for mode in (NONE, TENSOR, PHILOX):
            for clip in (False, True):
                outs = _step(x, eps, sched.ddim_scalars(999, 949, 1.0), clip=clip, mode=mode, z=z, step=999, sz=True,
                             x0=True)
                assert all(bool(torch.isfinite(o).all()) for o in outs), (shape, mode, clip)


def test_wrapper_refuses_what_the_kernel_cannot_read(sched):
    K = _K()
    x, eps, z = _inputs(SHAPES[0])
    sc = sched.ddim_scalars(500, 480, 1.0)
    out = torch.empty_like(x)
    with pytest.raises(RuntimeError):
        K.ddim_step(x.cpu(), eps, out, *sc)
    with pytest.raises(RuntimeError):
        K.ddim_step(x, eps.double(), out, *sc)
    with pytest.raises(RuntimeError):
        K.ddim_step(x, eps[:1], out, *sc)
    with pytest.raises(RuntimeError):
        K.ddim_step(x.transpose(2, 3), eps, out, *sc)
    with pytest.raises(RuntimeError):
        K.ddim_step(x, eps, out, *sc, mode=TENSOR)  # no z
    with pytest.raises(RuntimeError):
        K.ddim_step(x, eps, out, *sc, x0_out=torch.empty((1, ), device='cuda'))
    mis = torch.empty(x.numel() + 1, device='cuda')[1:].view(x.shape)  # 4 bytes past a 16-byte boundary
    with pytest.raises(RuntimeError):
        K.ddim_step(x, eps, mis, *sc)


# --------------------------------------------------------------------------------------- loop wiring (stub model)
def _stub(x, t):
    return 0.1 * x + 1e-3 * t.float().view(-1, 1, 1, 1)


STUB_SHAPE = (2, 3, 8, 8)


@pytest.mark.parametrize('eta', [0.0, 1.0])
@pytest.mark.parametrize('kw', [dict(steps=5), dict(timesteps=[0, 7, 19])], ids=['steps5', 'explicit'])
def test_strided_loop_recomputed_step_by_step(kw, eta):
    from weatherconverter_amd.diffusion_model.sample_ddpm import sample_tensor
    K = _K()
    s = _sched(20)
    tau = s.timestep_sequence(kw.get('steps'), timesteps=kw.get('timesteps'))
    assert tau == ([3, 7, 11, 15, 19] if 'steps' in kw else [0, 7, 19])
    seen, seen_t = [], []
    out = sample_tensor(_stub, s, 2, 3, 8, noise='philox', seed=5, eta=eta, progress=seen_t.append,
                        progress_x=lambda t, x: seen.append((t, x.clone())), **kw)
    assert [t for t, _ in seen] == seen_t == tau[::-1]  # the timestep left, downwards
    assert torch.equal(out, seen[-1][1])
    prev = K.philox_normal(STUB_SHAPE, out.device, 5, 0, 20)  # x_T is keyed by T
    for k, (t, x) in zip(reversed(range(len(tau))), seen):
        t_to = tau[k - 1] if k > 0 else -1  # the last transition is tau_0 -> -1
        eps = _stub(prev, torch.tensor([t], device=prev.device))
        z = K.philox_normal(STUB_SHAPE, out.device, 5, 0, t)  # keyed by the timestep left
        scalars = s.ddim_scalars(t, t_to, eta)
        assert (scalars[4] > 0) == (eta > 0 and k > 0)
        ref = ref_step(prev, eps, z, scalars, False)
        _within(x, ref['xp'], ref['b_xp'], (t, t_to, eta))
        prev = x
    # the final step returns the x0 prediction itself
    _within(out, ref['x0'], ref['b_x0'], 'x0')


def test_strided_loop_clips_and_rejects(sched):
    from weatherconverter_amd.diffusion_model.sample_ddpm import sample_tensor
    s = _sched(20)
    out = sample_tensor(_stub, s, 2, 3, 8, noise='philox', seed=5, steps=5, eta=1.0, clip_x0=True)
    assert float(out.abs().max()) <= 1.0  # the last step returns the clipped x0
    for bad in (dict(steps=0), dict(steps=21), dict(steps=5, spacing='leading'), dict(timesteps=[3, 3])):
        with pytest.raises(ValueError):
            sample_tensor(_stub, s, 2, 3, 8, noise='philox', seed=5, **bad)


@pytest.mark.parametrize('kw', [dict(steps=5), dict(timesteps=[0, 7, 19])], ids=['steps5', 'explicit'])
def test_ddim_invert_recomputed_step_by_step(kw):
    from weatherconverter_amd.diffusion_model.sample_ddpm import ddim_invert
    s = _sched(20)
    tau = s.timestep_sequence(kw.get('steps'), timesteps=kw.get('timesteps'))
    img = torch.rand(STUB_SHAPE, generator=torch.Generator().manual_seed(23)) * 2 - 1
    seen = []

    def model(x, t):
        seen.append((int(t), x.clone()))
        return _stub(x, t)

    lat = ddim_invert(model, s, img, **kw)
    assert [t for t, _ in seen] == tau[:-1]  # eps at the timestep being left, upwards
    assert torch.equal(seen[0][1], img.cuda())  # the image is x at tau_0
    xs = [x for _, x in seen] + [lat]
    for k, t in enumerate(tau[:-1]):
        scalars = s.ddim_scalars(t, tau[k + 1], 0.0)
        assert scalars[4] == 0.0
        ref = ref_step(xs[k], _stub(xs[k], torch.tensor([t], device='cuda')), None, scalars, False)
        _within(xs[k + 1], ref['xp'], ref['b_xp'], (t, tau[k + 1]))
    assert torch.equal(ddim_invert(_stub, s, img, timesteps=[7]), img.cuda())  # nothing to walk


def test_reference_rng_consumption_of_the_strided_loop():
    """noise='torch_cpu': x_T and one full-batch draw per step with sigma > 0, in loop order; the global
    generator ends where those draws leave it (eta = 0: x_T alone)."""
    from weatherconverter_amd.diffusion_model.sample_ddpm import sample_tensor
    s = _sched(20)
    for eta, draws in ((1.0, 1 + 4), (0.0, 1)):
        torch.manual_seed(11)
        zs = [torch.randn(STUB_SHAPE) for _ in range(draws)]
        want = torch.get_rng_state()
        torch.manual_seed(11)
        seen = []
        sample_tensor(_stub, s, 2, 3, 8, noise='torch_cpu', steps=5, eta=eta,
                      progress_x=lambda t, x: (seen.append(x.clone()), torch.randn(3)))  # a drawing callback
        # the callback's own draws come from the global generator; the loop's come from its private one
        torch.manual_seed(11)
        plain = sample_tensor(_stub, s, 2, 3, 8, noise='torch_cpu', steps=5, eta=eta)
        assert torch.equal(torch.get_rng_state(), want), eta
        assert torch.equal(plain, seen[-1])
        # and the draws are used in loop order: the first step's x from x_T = zs[0] and z = zs[1]
        x_T = zs[0].cuda()
        sc = s.ddim_scalars(19, 15, eta)
        ref = ref_step(x_T, _stub(x_T, torch.tensor([19], device='cuda')), zs[1].cuda() if eta else None, sc, False)
        _within(seen[0], ref['xp'], ref['b_xp'], eta)


# --------------------------------------------------------------------------------------- tiny UNet
@pytest.fixture(scope='module')
def tiny():
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.synthetic import init_synthetic_
    mc = ModelConfig(**json.load(open(os.path.join(GOLDEN, 'manifest.json')))['tiny']['config'])
    net = Unet(mc)
    init_synthetic_(net, seed=0)
    return mc, net.cuda().eval()


def test_tiny_unet_graph_sharding_and_defaults(tiny):
    from weatherconverter_amd.diffusion_model.distributed import sample_sharded
    from weatherconverter_amd.diffusion_model.sample_ddpm import ddim_invert, sample_tensor
    mc, net = tiny
    assert (mc.im_channels, mc.im_size) == (3, 32)
    s = _sched(20)
    kw = dict(noise='philox', seed=21, steps=5, eta=1.0)
    full = sample_tensor(net, s, 4, 3, 32, **kw)
    assert torch.isfinite(full).all()
    assert torch.equal(sample_tensor(net, s, 4, 3, 32, graph=True, **kw), full)
    part = sample_tensor(net, s, 2, 3, 32, sample0=2, total_batch=4, **kw)
    assert rel_l2(full[2:], part) < 1e-6
    fc = sample_tensor(net, s, 4, 3, 32, noise='torch_cpu', seed=22, steps=5, eta=1.0)
    pc = sample_tensor(net, s, 2, 3, 32, noise='torch_cpu', seed=22, steps=5, eta=1.0, sample0=2, total_batch=4)
    assert rel_l2(fc[2:], pc) < 1e-6
    # world 1 (no process group): sample_sharded passes the keywords through
    assert torch.equal(sample_sharded(net, s, 4, 3, 32, noise='philox', seed=21, steps=5, eta=1.0), full)
    # steps=None is the loop as it was
    assert torch.equal(sample_tensor(net, s, 2, 3, 32, noise='philox', seed=21, steps=None, timesteps=None, eta=0.7,
                                     clip_x0=True), sample_tensor(net, s, 2, 3, 32, noise='philox', seed=21))
    assert not torch.equal(sample_tensor(net, s, 2, 3, 32, noise='philox', seed=21, steps=20, eta=1.0)[:1], full[:1])
    # inversion through the graph is the eager one
    img = full[:2].clamp(-1, 1)
    lat = ddim_invert(net, s, img, steps=5)
    assert torch.isfinite(lat).all() and torch.equal(ddim_invert(net, s, img, steps=5, graph=True), lat)


# --------------------------------------------------------------------------------------- guided loop
def test_strided_guided_loop(tiny, monkeypatch):
    from test_guided import _seg, _srgan
    from weatherconverter_amd import kernels, translation
    mc, unet = tiny
    sched = _sched(1000)
    seg, gen = _seg().cuda(), _srgan().cuda()
    g = torch.Generator().manual_seed(3)
    x = torch.rand((1, 3, 32, 32), generator=g) * 2 - 1
    gt = torch.randint(0, 19, (1, 128, 128), generator=g).cuda()
    noise = torch.randn((1, 3, 32, 32), generator=g)
    kw = dict(N=6, t_start=torch.tensor([5]), noise=noise, LAMBDA=1e6, return_latent=True, graph=False)
    run = lambda **k: translation.sample_with_sgg(x, unet, sched, seg, gt, gen, **kw, **k)  # noqa: E731

    with pytest.raises(ValueError, match='eta'):
        run(steps=3, eta=0)
    with pytest.raises(ValueError):
        run(steps=7)

    hops, gsg_at, launches = [], [], []
    real_prev, real_gsg, real_step = sched.ddim_prev_timestep, translation.apply_gsg, kernels.ddim_step

    def prev(xt, eps, t, t_to, **k):
        hops.append((t, t_to))
        return real_prev(xt, eps, t, t_to, **k)

    def gsg(*a, **k):
        gsg_at.append(hops[-1][0] if hops else None)
        return real_gsg(*a, **k)

    def step(*a, **k):
        launches.append(1)
        return real_step(*a, **k)

    monkeypatch.setattr(sched, 'ddim_prev_timestep', prev)
    monkeypatch.setattr(translation, 'apply_gsg', gsg)
    monkeypatch.setattr(kernels, 'ddim_step', step)
    torch.manual_seed(9)
    out, lat = run(steps=3)
    assert out.shape == (1, 3, 128, 128) and torch.isfinite(out).all() and torch.isfinite(lat).all()
    assert hops == [(5, 3), (3, 1), (1, -1)] and len(launches) == 3
    assert gsg_at == [3]  # tau = [1, 3, 5]: position 1 is the only odd one
    # positions, not timesteps, decide: tau = [1, 2, 4, 5] guides at positions 1 and 3, timesteps 2 and 5
    del hops[:], gsg_at[:]
    run(steps=4)
    assert hops == [(5, 4), (4, 2), (2, 1), (1, -1)] and gsg_at == [5, 2]
    # the default path is the loop as it was: every timestep, no wc_ddim_step launch
    del hops[:], gsg_at[:], launches[:]
    out, _ = run()
    assert torch.isfinite(out).all() and not hops and not launches and len(gsg_at) == 3  # i = 5, 3, 1
