"""GPU: the training backward at the batch regimes the workloads select, against float64.

B selects code in the backward (tests/test_batch_regimes_cpu.py): how the halo weight gradient's pixel
splits lie against images (the kernel switches the per-image GroupNorm scale / shift inside a split), whether
wc_wgrad_reduce adds its slabs in one level or in groups of 32 with a short last group, and whether a
GroupNorm-backward split is short or empty.  The cases are the table of test_batch_regimes_cpu.py, which
proves on the CPU that they cover every class the recorded workloads reach (config 3 at B = 32, 256 px at
B = 5, the reference's 128 px at B = 4).  Each case asserts its regime with the library's split function
and the kernel that ran (K.profile_conv names), compares with float64 autograd on the CPU at the project's
bound (rel-L2 < 1e-5), and runs twice for bit-identical results (the reduce order is fixed).  One image's
gradient is scaled by 1e-3, another image's input by 30, and the GroupNorm scale grows with the image
(sc = 0.5 + 2 b / B): another image's scale or shift is far outside the bound.

Measured on an MI355X (rel-L2 against float64; f16x3 / bf16x6, prologue kinds 1 and 2 agree to two digits):
  wgrad3 (M, C0, B, H, W)   splits x blocks (an image)   regime                              f16x3    bf16x6
    (128, 64, 8, 8, 16)      2 x 4 (1)                    4 whole images a split              2.8e-7   3.9e-7
    (128, 32, 5, 8, 32)      2 x 5 (2)                    a split ends inside image 2         2.6e-7   3.5e-7
    (64, 64, 9, 4, 16)       4 x 5 (2), last short        inside images, 64-channel tiles     1.6e-7   1.9e-7
    (256, 64, 6, 8, 16)      1 x 6 (1)                    one split over six images           3.7e-7   5.1e-7
    (64, 64, 5, 8, 128)      40 x 4 (32)                  aligned, reduce groups 32 + 8       1.7e-7   2.1e-7
    (64, 64, 8, 16, 64)      64 x 4 (32)                  aligned, two full reduce groups     1.7e-7   2.1e-7
  generic (f16x3)            splits x pixels (an image)   regime                              rel-L2
    1x1_raw                  38 x 256 (1920)              spanning, short last, 32 + 6        2.1e-7
    3x3_gn_res               35 x 256 (1760)              spanning, short last, 32 + 3        2.2e-7 (residual 2.1e-7)
    4x4s2_raw                7 x 256 (240)                spanning, partial K-step            2.1e-7
    1x1_gn                   38 x 256 (1920)              as 1x1_raw, GroupNorm prologue      2.1e-7
    1x1_gn_aligned           4 x 256 (512)                aligned, full, one level            2.0e-7
    1x1_gn_64 / 1x1_raw_64   64 x 256 (4096)              aligned, two full groups            2.1e-7 / 2.1e-7
  GN(+SiLU) backward (B, H, W): worst of dx, dgamma, dbeta, closed-form dx sums, plain sums over C and silu
    (17, 32, 32)             60 splits of 18, 3 empty     1.8e-7
    (33, 32, 32)             31 splits of 34, last of 4   2.4e-7
    (5, 10, 10)              6 splits of 17, last of 15   1.6e-7
    (1025, 4, 4), C = 32     1 split (the clamp)          7.8e-7 (dgamma; dx 1.4e-7)
  wino gnb epilogue against the reduce path, (17, 32, 32, 64, 64): dx 1.4e-8, dgamma 2.5e-7, dbeta 2.7e-7, dx sums 2.1e-7
  add_noise B = 17: bit-equal to the fp32 expression, 4.0e-8 against float64 (464 entries of the GPU host's own
    torch tables differ from the reference host's: hence the golden tables)
  tiny, B = 17: overall 7.5e-7 (f16x3), 8.4e-7 (bf16x6), 9.6e-7 (fp32); worst tensor 6.0e-6 / 5.9e-6 / 8.4e-6; weight
    gradients reduced over 5, 17, 34, 68 and 136 splits, GroupNorm backward over 4, 16 and 60

Mutation check (each a value-only change of a scratch copy of the kernel source, no address or bound of a load or
store touched; tests/test_gpu_train.py and this module run once against each):
  1. conv_wgrad3_kernel keeps the first image's GroupNorm scale / shift for the whole split: all 16 cases of the first
     four wgrad3 shapes fail here (the two aligned shapes pass: one image a split).  Of the earlier tests one fails,
     test_conv_wgrad3_halo_kernel[2-True-64-64-2-6-16] (bf16x6, 64-channel tiles, GN+SiLU, one split over two
     images); no f16x3, 128-channel-tile or affine-only case did, and no case here repeats that one's (tile, form,
     prologue, regime), so none is dropped.
  2. wgrad_reduce_groups_kernel leaves out a short last group: wgrad3 (64, 64, 5, 8, 128) in all four forms, generic
     1x1_raw, 3x3_gn_res and 1x1_gn, and the tiny B = 17 step in all three precisions fail; no earlier test fails.
  3. gnb_reduce_kernel leaves out a short last split: the (17, 32, 32), (33, 32, 32) and (5, 10, 10) GroupNorm cases
     (12), the wino gnb comparison and the tiny B = 17 step (3) fail; (1025, 4, 4) passes (one full split); no
     earlier test fails.
"""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_batch_regimes_cpu as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _inputs(g, B, H, W, C0, M, Hm=None, Wm=None):
    """x [B][H][W][C0] with image 1 scaled by 30, dy [B][Hm][Wm][M] with image 0 scaled by 1e-3, and a
    GroupNorm affine that differs strongly per image."""
    x = torch.randn((B, H, W, C0), generator=g)
    x[1] *= 30.0
    dy = torch.randn((B, Hm or H, Wm or W, M), generator=g)
    dy[0] *= 1e-3
    b = torch.arange(B, dtype=torch.float32)[:, None]
    sc = (0.5 + 2.0 * b / B) * (0.75 + 0.5 * torch.rand((B, C0), generator=g))
    sh = 0.4 * b / B - 0.2 + 0.3 * torch.randn((B, C0), generator=g)
    return x, dy, sc, sh


def _prologue(x, sc, sh, pro):
    a = x.double()
    if pro:
        a = a * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    return F.silu(a) if pro == 2 else a


def _x_exp(a):
    """The static f16x3 exponent of a GroupNorm-bounded operand: |a| 2^x_exp <= 2^14."""
    return 13 - int(np.floor(np.log2(float(a.abs().max()))))


@contextlib.contextmanager
def _profiled(K):
    prof = K.profile_conv(True)
    try:
        yield prof
        torch.cuda.synchronize()
    finally:
        K.profile_conv(False)


# ------------------------------------------------------------------ halo 3x3 weight gradient
@pytest.mark.parametrize('pro', R.WGRAD3_PROS)
@pytest.mark.parametrize('form', R.WGRAD3_FORMS)
@pytest.mark.parametrize('shape,rel', R.WGRAD3_CASES, ids=['x'.join(map(str, s)) for s, _ in R.WGRAD3_CASES])
def test_wgrad3_splits_against_images(shape, rel, form, pro):
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.diffusion_model.models.engine import TAPS3
    from weatherconverter_amd.kernels import Seg, View
    M, C0, B, H, W = shape
    splits, bps, bpi, nblk = R.wgrad3_geometry(*shape)
    regimes = R.wgrad3_regimes(*shape)
    assert f'rel:{rel}' in regimes, regimes
    x, dy, sc, sh = _inputs(_gen(41), B, H, W, C0, M)
    a = _prologue(x, sc, sh, pro)
    dyc, xc = dy.cuda(), x.cuda()
    seg = Seg(View.full(xc), TAPS3, scale=sc.cuda(), shift=sh.cuda(), silu=pro == 2)
    assert K.wgrad3_ok(View.full(dyc), seg)
    f3 = K.F3Bounds(K.absmax_images(View.full(dyc)), _x_exp(a)) if form == 'f16x3' else None
    outs = []
    for _ in range(2):
        dw = torch.zeros((M, C0, 3, 3), device='cuda')
        with _profiled(K) as prof:
            K.conv_wgrad(View.full(dyc), [seg], dw, (C0 * 9, 9, 1), x6=True, f3=f3)
        outs.append(dw.cpu())
    WM, TH = (4, 8) if M % 128 == 0 else (2, 2)
    want = f'conv_wgrad3_kernel<{WM}, {TH}, {pro}, {"true" if form == "f16x3" else "false"}>'
    assert want in [n for n, *_ in prof], [n for n, *_ in prof]
    w = torch.zeros((M, C0, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv2d(a.permute(0, 3, 1, 2), w, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    err = rel_l2(outs[0], w.grad)
    print(f'wgrad3 {form} pro={pro} {shape}: {splits} splits of {bps} blocks, {bpi} an image, {sorted(regimes)}: '
          f'rel-L2 {err:.3e}')
    assert err < 1e-5
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ generic weight gradient + the reduce
@pytest.mark.parametrize('form', list(R.GENERIC_CASES))
def test_generic_wgrad_reduce_groups(form):
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.diffusion_model.models.engine import TAPS1, TAPS3, TAPS4S2
    from weatherconverter_amd.kernels import Seg, View
    M, C0, C1, taps, stride, pro, B, H, W = R.GENERIC_CASES[form]
    _, Kc, _, Hm, Wm, _ = R.generic_case_shape(form)
    splits, pps, P = R.generic_geometry(M, Kc, B, Hm, Wm)
    regimes = R.generic_regimes(M, Kc, B, Hm, Wm)
    g = _gen(43)
    x, dy, sc, sh = _inputs(g, B, H, W, C0, M, Hm, Wm)
    xr = torch.randn((B, H, W, max(C1, 4)), generator=g)
    a = _prologue(x, sc, sh, pro)
    tapset = {1: TAPS1, 9: TAPS3, 16: TAPS4S2}[taps]
    wshape = {1: (M, C0), 9: (M, C0, 3, 3), 16: (M, C0, 4, 4)}[taps]
    base, base1 = torch.randn(wshape, generator=g), torch.randn((M, max(C1, 4)), generator=g)
    dyc, xc, xrc = dy.cuda(), x.cuda(), xr.cuda()
    gb = dy.abs().amax((1, 2, 3)).cuda()
    if pro:
        segs = [Seg(View.full(xc), tapset, scale=sc.cuda(), shift=sh.cuda(), silu=pro == 2)]
        f3 = K.F3Bounds(gb, _x_exp(a), None, xr.abs().amax((1, 2, 3)).cuda() if C1 else None)
    else:
        segs = [Seg(View.full(xc), tapset, stride=stride)]
        f3 = K.F3Bounds(gb, 60, x.abs().amax((1, 2, 3)).cuda())
    if C1:
        segs.append(Seg(View.full(xrc), TAPS1, kbase=taps * C0))
    assert not K.wgrad3_ok(View.full(dyc), segs[0])
    s0 = (C0, 1, 0) if taps == 1 else (C0 * taps, taps, 1)
    outs = []
    for _ in range(2):
        dw, dw1 = base.clone().cuda(), base1.clone().cuda()
        with _profiled(K) as prof:
            K.conv_wgrad(View.full(dyc), segs, dw, s0, dw1=dw1 if C1 else None, s1=C1, accumulate=True, x6=True, f3=f3)
        outs.append((dw.cpu(), dw1.cpu()))
    names = [n for n, *_ in prof]
    assert f'conv_wgrad_kernel<128, 128, {pro}, true, true>' in names, names
    w = torch.zeros(wshape, dtype=torch.float64, requires_grad=True)
    if taps == 1:
        (torch.einsum('bhwc,mc->bhwm', a, w) * dy.double()).sum().backward()
    else:
        F.conv2d(a.permute(0, 3, 1, 2), w, stride=stride, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    err = rel_l2(outs[0][0], base.double() + w.grad)
    msg = f'generic {form}: {splits} splits of {pps} pixels, {Hm * Wm} an image, {sorted(regimes)}: rel-L2 {err:.3e}'
    if C1:
        err1 = rel_l2(outs[0][1], base1.double() + torch.einsum('bhwm,bhwc->mc', dy.double(), xr.double()))
        msg += f', residual segment {err1:.3e}'
        assert err1 < 1e-5, msg
    print(msg)
    assert err < 1e-5
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------ GroupNorm(+SiLU) backward
_GN = [(shape, C, silu) for shape, Cs in R.GN_CASES for C in Cs for silu in (True, False)]


@pytest.mark.parametrize('shape,C,silu', _GN, ids=[f'{"x".join(map(str, s))}-C{C}-{"silu" if si else "gn"}' for s, C, si in _GN])
def test_gn_backward_short_and_empty_splits(shape, C, silu):
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import View
    B, H, W = shape
    splits, pps, empty = R.gn_geometry(B, H * W)
    regimes = R.gn_regimes(B, H * W)
    g = _gen(47)
    x = torch.randn((B, H, W, C), generator=g) * 2 + 0.5
    x[1] *= 30.0
    x[:, :, :, ::7] += 3.0  # channels whose mean is far from their group's
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    dz = torch.randn((B, H, W, C), generator=g)
    dz[0] *= 1e-3
    base = torch.randn((B, H, W, C), generator=g)
    xc, dzc, gc, bc = View.full(x.cuda()), View.full(dz.cuda()), gamma.cuda(), beta.cuda()
    sc, sh, a0, o0 = K.gn_stats_pair(xc, gc, bc)
    runs = []
    for _ in range(2):
        dx = base.cuda().clone()
        dg, db = torch.zeros(C, device='cuda'), torch.zeros(C, device='cuda')
        with _profiled(K) as prof:
            K.gn_backward(dzc, xc, a0, o0, gc, bc, silu, View.full(dx), dgamma=dg, dbeta=db, accumulate=True)
        dx2 = torch.empty((B, H, W, C), device='cuda')
        dsum = K.gn_backward(dzc, xc, a0, o0, gc, bc, silu, View.full(dx2), accumulate=False, dx_sums=True)
        plain = K.channel_sums(dzc)  # the reduce without x (bias / time-embedding gradients)
        torch.cuda.synchronize()
        runs.append([t.cpu() for t in (dx, dg, db, dx2, dsum, plain)])
    assert any(n.startswith('gnb_reduce_kernel') for n, *_ in prof), [n for n, *_ in prof]
    xd = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    gd, bd = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    y = F.group_norm(xd, 8, gd, bd, 1e-5)
    (F.silu(y) if silu else y).backward(dz.double().permute(0, 3, 1, 2))
    ref_dx = xd.grad.permute(0, 2, 3, 1)
    dx, dg, db, dx2, dsum, plain = runs[0]
    errs = dict(dx=rel_l2(dx - base, ref_dx), dgamma=rel_l2(dg, gd.grad), dbeta=rel_l2(db, bd.grad), dx_plain=rel_l2(dx2, ref_dx),
                dx_sums=rel_l2(dsum[..., 0], xd.grad.sum((2, 3))), sums=rel_l2(plain[..., 0], dz.double().sum((1, 2))))
    print(f'gn backward B={B} {H}x{W} C={C} silu={silu}: {splits} splits of {pps} pixels, {empty} empty, {sorted(regimes)}: '
          + ', '.join(f'{k} {v:.3e}' for k, v in errs.items()))
    assert dsum.shape == (B, C, 2) and bool((dsum[..., 1] == 0).all()) and bool((plain[..., 1] == 0).all())
    assert all(v < 1e-5 for v in errs.values()), errs
    # every image on its own: the small-gradient image and the large-input image are not carried by the rest
    for b in (0, 1, B - 1):
        assert rel_l2(dx2[b], ref_dx[b]) < 1e-5, b
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_wino_gnb_epilogue_beside_the_reduce_at_b17():
    """The data-gradient conv that forms the GroupNorm+SiLU backward's sums in its epilogue
    (wc_conv3x3_wino_f16x3_gnb) against the reduce path in the regime the case above checks against float64
    (B = 17: 60 reduce splits of 18 pixels, 3 empty): dz bit-identical, gn_backward's results equal to
    fp32 summation order (rel-L2 <= 1e-6, the bound of test_wino.py)."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.diffusion_model.models.engine import TAPS3
    B, H, W, Cg, Co = R.WINO_GNB_CASE
    assert R.gn_geometry(B, H * W) == (60, 18, 3)
    g = _gen(61)
    gy = torch.randn((B, H, W, Cg), generator=g) * 1e-2
    gy[0] *= 1e-3
    gy = gy.cuda()
    w = (torch.randn((Co, 9 * Cg), generator=g) / (9 * Cg)**0.5).cuda()
    x = torch.randn((B, H, W, Co), generator=g) * 2 + 0.5
    x[1] *= 30.0
    x = x.cuda()
    ga = (torch.rand(Co, generator=g) + 0.5).cuda()
    be = (torch.randn(Co, generator=g) * 0.1).cuda()
    xv = K.View.full(x)
    _, _, sc0, sh0 = K.gn_stats_pair(xv, ga, be)
    bound = gy.abs().reshape(B, -1).amax(1).contiguous()
    segs = [K.Seg(K.View.full(gy), TAPS3)]
    assert K.wino_eligible(segs, Co, H, W)
    wp = K.pack_wino(w, Cg)
    res = {}
    for mode in ('reduce', 'epilogue', 'epilogue2'):
        dz = torch.empty((B, H, W, Co), device='cuda')
        pre = K.GnbSums.make(xv, sc0, sh0, ga, be, True, dx_sums=True) if mode != 'reduce' else None
        assert mode == 'reduce' or pre is not None
        with _profiled(K) as prof:
            K.conv3x3_wino(segs, wp, None, K.View.full(dz), Hm=H, Wm=W, a_exp=60, a_bound=bound, gnb=pre)
            dx = torch.empty((B, H, W, Co), device='cuda')
            dgam, dbet = torch.zeros(Co, device='cuda'), torch.zeros(Co, device='cuda')
            dsum = K.gn_backward(K.View.full(dz), xv, sc0, sh0, ga, be, True, K.View.full(dx), dgamma=dgam, dbeta=dbet,
                                 accumulate=False, dx_sums=True, pre=pre)
        names = [n for n, *_ in prof]
        assert any(n.startswith('conv3x3_wino_kernel<') for n in names), names
        assert any(n.startswith('gnb_reduce_kernel') for n in names) == (mode == 'reduce'), names
        res[mode] = [t.cpu() for t in (dz, dx, dgam, dbet, dsum[..., 0])]
    assert torch.equal(res['reduce'][0], res['epilogue'][0])
    errs = [rel_l2(b, a) for a, b in zip(res['reduce'][1:], res['epilogue'][1:])]
    print('wino gnb epilogue against the reduce path (dx, dgamma, dbeta, dx sums): ' + ', '.join(f'{e:.3e}' for e in errs))
    assert all(e <= 1e-6 for e in errs), errs
    for a, b in zip(res['epilogue'], res['epilogue2']):
        assert torch.equal(a, b)


# ------------------------------------------------------------------ add_noise, the iteration's first kernel
def test_add_noise_b17_per_sample_t():
    """add_noise at B = 17, 3 x 8 x 12, per-sample t including 0 and 999: bit-equal to the oracle's fp32
    expression (oracle/scheduler_oracle.py add_noise) on the CPU, and within 1e-6 of float64.  The oracle's
    tables are set to the reference host's (tests/golden/sched.npz): torch's linspace / cumprod / sqrt give
    other bits on other CPUs (linear_noise_scheduler.py), and the product's tables are the reference host's."""
    import os
    import sys
    from conftest import GOLDEN, ROOT
    sys.path.insert(0, ROOT)
    from oracle.scheduler_oracle import OracleScheduler
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    g = _gen(53)
    B = 17
    x0 = torch.rand((B, 3, 8, 12), generator=g) * 2 - 1
    noise = torch.randn((B, 3, 8, 12), generator=g)
    t = torch.randint(1, 999, (B, ), generator=g)
    t[0], t[B - 1], t[5] = 0, 999, 999
    t[6] = 0
    s = LinearNoiseScheduler(1000, 0.0001, 0.02, device=torch.device('cuda:0'))
    outs = [s.add_noise(x0.cuda(), noise.cuda(), t.cuda()).cpu() for _ in range(2)]
    o = OracleScheduler(1000, 0.0001, 0.02)
    gd = np.load(os.path.join(GOLDEN, 'sched.npz'))
    host = 0
    for n in ('alpha_cum_prod', 'sqrt_alpha_cum_prod', 'sqrt_one_minus_alpha_cum_prod'):
        ref_host = torch.from_numpy(gd[f'T1000_{n}'])
        host += int((getattr(o, n) != ref_host).sum())
        setattr(o, n, ref_host)
    ref32 = o.add_noise(x0, noise, t)
    a = torch.sqrt(o.alpha_cum_prod.double())[t].reshape(B, 1, 1, 1)
    b = torch.sqrt(1 - o.alpha_cum_prod.double())[t].reshape(B, 1, 1, 1)
    err = rel_l2(outs[0], a * x0.double() + b * noise.double())
    print(f'add_noise B=17: rel-L2 vs float64 {err:.3e}; differs from the fp32 expression at '
          f'{int((outs[0] != ref32).sum())} of {ref32.numel()} ({host} table entries of this host\'s torch differ from '
          'the reference host\'s)')
    assert torch.equal(outs[0], ref32)
    assert err < 1e-6
    assert torch.equal(outs[0], outs[1])


# ------------------------------------------------------------------ one training step of the tiny model at B = 17
@contextlib.contextmanager
def _split_census():
    """The split counts every wc_wgrad_reduce and wc_gn_bwd_reduce call of the block was given."""
    from weatherconverter_amd import _native
    seen = dict(wc_wgrad_reduce=[], wc_gn_bwd_reduce=[])
    real = _native.call

    def call(name, *args):
        if name == 'wc_wgrad_reduce':
            seen[name].append(int(args[1]))
        elif name == 'wc_gn_bwd_reduce':
            seen[name].append(int(args[12]))
        return real(name, *args)

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, 'call', call)
        yield seen


@pytest.mark.parametrize('precision', ['f16x3', 'bf16x6', 'fp32'])
def test_unet_grads_tiny_b17_vs_oracle_autograd(precision):
    """One MSE training step of the tiny config at B = 17, 32 x 32, per-sample t including 0 and 999, against
    the oracle's float64 autograd under test_gpu_train's bounds (loss 1e-5 relative, gradients 1e-5 overall
    and 1e-4 per tensor); the step reduces a weight gradient over more than 32 splits and a GroupNorm
    backward over 60 (3 of them empty)."""
    import json
    import os
    from conftest import GOLDEN
    from test_gpu_train import _check, _model_grads
    from weatherconverter_amd import forms
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    mc = ModelConfig(**man['tiny']['config'])
    B = 17
    t = torch.randint(1, 999, (B, ), generator=_gen(59))
    t[0], t[B - 1] = 0, 999
    with forms.using(check_gbound=True), _split_census() as seen:
        ours, ref, lo, lr = _model_grads(mc, B, precision, t=t, share_ref=True)
    wg, gn = seen['wc_wgrad_reduce'], seen['wc_gn_bwd_reduce']
    print(f'tiny B=17 {precision}: loss {lo:.7f} vs {lr:.7f}; wgrad reduce splits {sorted(set(wg))}, '
          f'GN backward reduce splits {sorted(set(gn))}')
    assert any(s > R.RG for s in wg), sorted(set(wg))
    assert R.gn_geometry(B, 32 * 32)[0] == 60 and 60 in gn, sorted(set(gn))
    assert abs(lo - lr) <= 1e-5 * abs(lr)
    _check(ours, ref)
