"""CPU: the strided-sampling C ABI as read from include/wc_sampler.h, the rejections wc_ddim_step makes
before any HIP call, and the host side of the scheduler's strided sampling: timestep_sequence and
ddim_scalars."""
import ctypes
import math
import os

import numpy as np
import pytest

from conftest import ROOT
from weatherconverter_amd import _abi, _native

EPS32 = 2.0**-24  # one fp32 rounding, relative


def _header(name):
    return _abi.read(open(os.path.join(ROOT, 'include', name)).read())


def _scheduler(T=1000):
    import torch
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    return LinearNoiseScheduler(T, 1e-4, 2e-2, device=torch.device('cpu'))


# --------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_one_entry_point():
    abi = _header('wc_sampler.h')
    assert list(abi.functions) == ['wc_ddim_step'] and not abi.structs
    others = (_native.ABI, _native.OPTIM_ABI, _native.EMA_ABI)
    assert not set(abi.functions) & set().union(*(set(o.functions) for o in others))
    assert _native._SIGNATURES['wc_ddim_step'] is _native.SAMPLER_ABI.functions['wc_ddim_step']
    P, I, L, F, U = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64
    assert _native.SAMPLER_ABI.functions['wc_ddim_step'] == abi.functions['wc_ddim_step'] == (
        I, [P] * 6 + [L, L] + [F] * 5 + [I, I, U, L, L, P])


def test_exports_of_the_main_header_are_unchanged():
    assert _native.EXPORTS == list(_header('wc_kernels.h').functions) and len(_native.EXPORTS) == 88
    assert 'wc_ddim_step' not in _native.EXPORTS


def test_the_build_lists_the_header_and_the_source_exists():
    from weatherconverter_amd import _build
    assert 'wc_sampler.h' in _build.ABI_HEADERS
    assert 'wc_misc.hip' in _build.SOURCES  # the kernel sits beside ddpm_step_kernel
    text = open(os.path.join(_build.CSRC, 'wc_misc.hip')).read()
    assert 'ddim_step_kernel' in text and 'wc_ddim_step' in text


# --------------------------------------------------------------------------------------- rejections
@pytest.fixture(scope='module')
def lib():
    from weatherconverter_amd import _build
    if not os.path.exists(_build.LIB_PATH):
        if not os.path.exists(_build.HIPCC):
            pytest.skip('hipcc not available to build the library')
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name, (res, args) in _native.SAMPLER_ABI.functions.items():
        assert hasattr(lib, name), name  # the library exports the symbol
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def test_rejections_come_before_any_launch(lib):
    """Every call here returns from the host checks: no HIP call is made, so no GPU is needed.  The
    pointers are dummies that are never dereferenced."""
    p = 4096
    good = dict(x=p, eps=p, z=p, x_out=p, sz_out=None, x0_out=None, B=1, per=16, sa=0.8, s1m=0.6, sa_to=0.9,
                c_dir=0.4, sigma=0.1, clip=0, mode=_native.NOISE_NONE, seed=0, sample0=0, step=0)

    def call(**kw):
        a = {**good, **kw}
        return lib.wc_ddim_step(a['x'], a['eps'], a['z'], a['x_out'], a['sz_out'], a['x0_out'], a['B'], a['per'],
                                a['sa'], a['s1m'], a['sa_to'], a['c_dir'], a['sigma'], a['clip'], a['mode'], a['seed'],
                                a['sample0'], a['step'], None)

    E_ARG, E_SHAPE = _native.E_ARG, _native.E_SHAPE
    for name in ('x', 'eps', 'x_out'):
        assert call(**{name: None}) == E_ARG, name
    for mode in (-1, 3, 7):
        assert call(mode=mode) == E_ARG
    assert call(mode=_native.NOISE_TENSOR, z=None) == E_ARG
    for per in (15, 2, 18):
        assert call(per=per) == E_SHAPE
    for B in (0, -1):
        assert call(B=B) == E_SHAPE
    nan = float('nan')
    assert call(sa=0.0) == E_ARG and call(sa=-0.5) == E_ARG
    assert call(s1m=-0.1) == E_ARG and call(c_dir=-0.1) == E_ARG and call(sigma=-0.1) == E_ARG
    for name in ('sa', 's1m', 'sa_to', 'c_dir', 'sigma'):
        assert call(**{name: nan}) == E_ARG, name
    assert call(clip=1, sa=1.0, s1m=0.0) == E_ARG
    assert E_ARG != E_SHAPE and _native.OK == 0


# --------------------------------------------------------------------------------------- timestep_sequence
@pytest.mark.parametrize('T,steps', [(1000, 50), (1000, 7), (20, 5), (20, 20), (10, 3)])
def test_timestep_sequence_spacings(T, steps):
    s = _scheduler(T)
    for spacing in ('trailing', 'uniform'):
        tau = s.timestep_sequence(steps, spacing=spacing)
        assert len(tau) == steps and all(type(v) is int for v in tau)
        assert all(b > a for a, b in zip(tau, tau[1:])) and 0 <= tau[0] and tau[-1] < T
    assert s.timestep_sequence(steps)[-1] == T - 1  # trailing is the default
    assert s.timestep_sequence(steps, spacing='uniform')[0] == 0


def test_timestep_sequence_values():
    assert _scheduler(1000).timestep_sequence(50) == list(range(19, 1000, 20))
    assert _scheduler(10).timestep_sequence(3) == [3, 6, 9]
    assert _scheduler(10).timestep_sequence(3, spacing='uniform') == [0, 3, 6]
    for T in (10, 20):
        for spacing in ('trailing', 'uniform'):
            assert _scheduler(T).timestep_sequence(T, spacing=spacing) == list(range(T))
    assert _scheduler(20).timestep_sequence(timesteps=[0, 7, 19]) == [0, 7, 19]
    assert _scheduler(20).timestep_sequence(timesteps=(5, )) == [5]


def test_timestep_sequence_refusals():
    s = _scheduler(20)
    for steps in (0, 21, -3, None, 2.5):
        with pytest.raises(ValueError):
            s.timestep_sequence(steps)
    with pytest.raises(ValueError, match='spacing'):
        s.timestep_sequence(5, spacing='leading')
    for bad in ([7, 0, 19], [0, 7, 7], [0, 20], [-1, 3], [], [0.5, 3]):
        with pytest.raises(ValueError):
            s.timestep_sequence(timesteps=bad)
    with pytest.raises(ValueError):
        s.timestep_sequence(5, timesteps=[0, 7, 19])


# --------------------------------------------------------------------------------------- ddim_scalars
def _closed_form(s, t, t_to, eta):
    acp = s._cpu['alpha_cum_prod'].numpy().astype(np.float64)
    a_t = acp[t]
    a_to = 1.0 if t_to < 0 else acp[t_to]
    sigma = eta * math.sqrt((1 - a_to) / (1 - a_t)) * math.sqrt(max(1 - a_t / a_to, 0.0)) if t_to < t else 0.0
    return math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_to), math.sqrt(max(1 - a_to - sigma**2, 0.0)), sigma, a_to


TRANSITIONS = [(999, 949), (999, 998), (500, 480), (20, 0), (1, 0), (0, -1), (0, 20), (480, 500)]


@pytest.mark.parametrize('eta', [0.0, 0.5, 1.0])
def test_ddim_scalars_against_the_closed_form(eta):
    s = _scheduler(1000)
    for t, t_to in TRANSITIONS:
        got = s.ddim_scalars(t, t_to, eta)
        *want, a_to = _closed_form(s, t, t_to, eta)
        assert len(got) == 5 and all(type(v) is float for v in got)
        for g, w in zip(got, want):
            assert g == float(np.float32(g))  # an fp32 value
            assert abs(g - w) <= EPS32 * abs(w), (t, t_to, eta, g, w)
        sa, s1m, sa_to, c_dir, sigma = got
        assert abs(c_dir**2 + sigma**2 + a_to - 1.0) <= 4 * EPS32, (t, t_to, eta)
        if t_to > t:
            assert sigma == 0.0  # inversion is deterministic whatever eta is
        elif eta > 0 and t_to >= 0:
            assert sigma > 0.0
        if eta == 0:
            assert sigma == 0.0


def test_ddim_scalars_final_step_and_refusals():
    s = _scheduler(1000)
    for t in (0, 19, 999):
        for eta in (0.0, 1.0):
            sa, s1m, sa_to, c_dir, sigma = s.ddim_scalars(t, -1, eta)
            assert (sa_to, c_dir, sigma) == (1.0, 0.0, 0.0) and sa > 0 and s1m > 0
    for t, t_to in ((5, 5), (1000, 3), (-1, 3), (5, -2), (5, 1000)):
        with pytest.raises(ValueError):
            s.ddim_scalars(t, t_to, 0.0)
    with pytest.raises(ValueError, match='eta'):
        s.ddim_scalars(5, 3, -1.0)


def test_eta_one_is_the_posterior_sigma_at_stride_one():
    """At t_to = t - 1 and eta = 1 the DDIM sigma is the DDPM posterior's (the same expression in exact
    arithmetic).  DDIM's takes 1 - acp[t] / acp[t-1] where the posterior takes beta_t: the two fp32 table
    entries carry a relative rounding of 2^-24 each, so the quotient is off by up to 2 * 2^-24 absolute,
    that is 2 * 2^-24 / beta_t relative to beta_t, and half of that on the root; the bound is twice
    that plus 1e-6 for the remaining fp32 operations of the posterior."""
    s = _scheduler(1000)
    betas = s._cpu['betas'].numpy()
    for t in (1, 2, 500, 999):
        sigma = s.ddim_scalars(t, t - 1, 1.0)[4]
        post = s.step_scalars(t, 'posterior')[3]
        assert abs(sigma - post) <= (2 * EPS32 / float(betas[t]) + 1e-6) * post, (t, sigma, post)
