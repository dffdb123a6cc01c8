"""GPU: the training backward (reference train_ddpm.py:106-114 loss.backward()).

Kernel level: conv weight gradients, GroupNorm(+SiLU) backward and attention backward against
PyTorch autograd in float64 on the same inputs (rel-L2 <= 1e-5; fp32-MFMA / bf16x6 arithmetic).
Model level: every parameter gradient of Unet under the reference's own loop
``pred = model(noisy, t); loss = MSELoss()(pred, noise); loss.backward()`` against autograd through
the oracle's restatement of unet_base.Unet (float64), on the tiny config and on the 256-px
BASELINE architecture at B=2.  Tolerance: rel-L2 <= 1e-5 over all gradients together and
<= 1e-4 per parameter tensor (small tensors such as biases sum many cancelling terms).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import rel_l2

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize('x6', [False, True])
@pytest.mark.parametrize('silu,res,M', [(True, True, 96), (False, False, 96), (True, False, 64)])
def test_conv_wgrad_3x3_prologue_residual(silu, res, M, x6):
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS1, TAPS3
    g = _gen(1)
    B, H, W, C0, C1 = 2, 12, 20, 32, 64
    x = torch.randn((B, H, W, C0), generator=g)
    xr = torch.randn((B, H, W, C1), generator=g)
    dy = torch.randn((B, H, W, M), generator=g)
    sc = torch.rand((B, C0), generator=g) + 0.5
    sh = torch.randn((B, C0), generator=g) * 0.3
    dw = torch.zeros((M, C0, 3, 3), device='cuda')
    dwr = torch.zeros((M, C1), device='cuda')
    segs = [Seg(View.full(x.cuda()), TAPS3, scale=sc.cuda(), shift=sh.cuda(), silu=silu)]
    if res:
        segs.append(Seg(View.full(xr.cuda()), TAPS1, kbase=9 * C0))
    K.conv_wgrad(View.full(dy.cuda()), segs, dw, (C0 * 9, 9, 1), dw1=dwr if res else None, s1=C1, x6=x6)
    a = x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    a = F.silu(a) if silu else a
    w = torch.zeros((M, C0, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.permute(0, 3, 1, 2), w, padding=1)
    y.backward(dy.double().permute(0, 3, 1, 2))
    assert rel_l2(dw.cpu(), w.grad) < 1e-5
    if res:
        ref = torch.einsum('bhwm,bhwc->mc', dy.double(), xr.double())
        assert rel_l2(dwr.cpu(), ref) < 1e-5


@pytest.mark.parametrize('pro,res,M,C0,B,H,W', [(2, True, 128, 64, 2, 16, 32), (1, False, 256, 32, 1, 8, 16),
                                                (0, False, 128, 32, 3, 8, 48), (2, True, 64, 64, 2, 6, 16),
                                                (2, False, 64, 128, 1, 4, 32)])
def test_conv_wgrad3_halo_kernel(pro, res, M, C0, B, H, W):
    """The halo-tiled 3x3 weight gradient (wc_conv_wgrad3, bf16x6) against float64 autograd, both
    tile configurations (128- and 64-channel M tiles), every prologue, image borders, several
    images per split, and the residual segment through the generic GEMM beside it."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS1, TAPS3
    g = _gen(3)
    C1 = 32
    x = torch.randn((B, H, W, C0), generator=g)
    xr = torch.randn((B, H, W, C1), generator=g)
    dy = torch.randn((B, H, W, M), generator=g)
    sc = torch.rand((B, C0), generator=g) + 0.5
    sh = torch.randn((B, C0), generator=g) * 0.3
    dw = torch.zeros((M, C0, 3, 3), device='cuda')
    dwr = torch.zeros((M, C1), device='cuda')
    segs = [Seg(View.full(x.cuda()), TAPS3, scale=sc.cuda() if pro else None, shift=sh.cuda() if pro else None,
                silu=pro == 2)]
    if res:
        segs.append(Seg(View.full(xr.cuda()), TAPS1, kbase=9 * C0))
    assert K.wgrad3_ok(View.full(dy.cuda()), segs[0])
    prof = K.profile_conv(True)
    K.conv_wgrad(View.full(dy.cuda()), segs, dw, (C0 * 9, 9, 1), dw1=dwr if res else None, s1=C1, x6=True)
    torch.cuda.synchronize()
    K.profile_conv(False)
    assert any(n.startswith('conv_wgrad3_kernel') for n, *_ in prof)
    a = x.double()
    if pro:
        a = a * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    a = F.silu(a) if pro == 2 else a
    w = torch.zeros((M, C0, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.permute(0, 3, 1, 2), w, padding=1)
    y.backward(dy.double().permute(0, 3, 1, 2))
    assert rel_l2(dw.cpu(), w.grad) < 1e-5
    if res:
        ref = torch.einsum('bhwm,bhwc->mc', dy.double(), xr.double())
        assert rel_l2(dwr.cpu(), ref) < 1e-5


@pytest.mark.parametrize('pro,M,C0,B,H,W', [(2, 128, 64, 2, 16, 32), (1, 256, 32, 1, 8, 16), (2, 64, 128, 3, 4, 32)])
def test_conv_wgrad3_f16x3_vs_float64(pro, M, C0, B, H, W):
    """The halo-tiled 3x3 weight gradient on f16x3 (wc_conv_wgrad3_f16x3): X~ under its own
    exponent, G under the batch's max of the per-image absmax (wc_absmax_images), images whose
    gradients differ by 10^3 in scale; against float64 autograd at rel-L2 <= 1e-5."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS3
    g = _gen(5)
    x = torch.randn((B, H, W, C0), generator=g)
    dy = torch.randn((B, H, W, M), generator=g)
    dy[0] *= 1e-3
    sc = torch.rand((B, C0), generator=g) + 0.5
    sh = torch.randn((B, C0), generator=g) * 0.3
    a = x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :]
    a = F.silu(a) if pro == 2 else a
    x_exp = 13 - int(np.floor(np.log2(float(a.abs().max()))))
    dyc = dy.cuda()
    gb = K.absmax_images(View.full(dyc))
    assert torch.allclose(gb.cpu(), dy.abs().amax((1, 2, 3)))
    dw = torch.zeros((M, C0, 3, 3), device='cuda')
    seg = Seg(View.full(x.cuda()), TAPS3, scale=sc.cuda(), shift=sh.cuda(), silu=pro == 2)
    prof = K.profile_conv(True)
    K.conv_wgrad(View.full(dyc), [seg], dw, (C0 * 9, 9, 1), x6=True, f3=K.F3Bounds(gb, x_exp))
    torch.cuda.synchronize()
    K.profile_conv(False)
    assert any(n.startswith('conv_wgrad3_kernel') and n.endswith('true>') for n, *_ in prof), [n for n, *_ in prof]
    w = torch.zeros((M, C0, 3, 3), dtype=torch.float64, requires_grad=True)
    y = F.conv2d(a.permute(0, 3, 1, 2), w, padding=1)
    y.backward(dy.double().permute(0, 3, 1, 2))
    assert rel_l2(dw.cpu(), w.grad) < 1e-5


@pytest.mark.parametrize('variant', ['', 'bf16'])
@pytest.mark.parametrize('form', ['3x3_gn_res', '4x4s2_raw', '1x1_raw'])
def test_conv_wgrad_generic_f16x3_vs_float64(form, variant):
    """The generic weight-gradient GEMM on f16x3 (wc_conv_wgrad_f16x3): a GroupNorm+SiLU 3x3 segment at
    its static exponent with a raw 1x1 residual segment under its per-image bound (a grid the halo
    kernel does not take), a raw 4x4/s2 conv and a raw 1x1 under per-image bounds (a pixel count that
    ends in a partial K-step); gradients whose images differ by 10^3 in scale; against float64 at
    rel-L2 <= 1e-5.  variant 'bf16': the bf16 training line's single-piece form (one LDS plane, 32
    pixels per barrier) within bf16 operand rounding."""
    import contextlib
    from weatherconverter_amd import _native
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS1, TAPS3, TAPS4S2
    lib = _native.variant(variant) if variant else contextlib.nullcontext()
    tol = 1e-5 if not variant else 2e-2
    ok = (lambda e: e < tol) if not variant else (lambda e: 1e-5 < e < tol)  # noqa: E731
    g = _gen(8)
    B, C0, C1, M = 2, 64, 32, 128
    H, W = {'3x3_gn_res': (12, 20), '4x4s2_raw': (16, 32), '1x1_raw': (11, 21)}[form]
    Hm, Wm = (H // 2, W // 2) if form == '4x4s2_raw' else (H, W)
    x = torch.randn((B, H, W, C0), generator=g) * torch.tensor([1.0, 30.0])[:, None, None, None]
    xr = torch.randn((B, H, W, C1), generator=g)
    dy = torch.randn((B, Hm, Wm, M), generator=g)
    dy[1] *= 1e-3
    gb = dy.abs().amax((1, 2, 3)).cuda()
    dwr = torch.zeros((M, C1), device='cuda')
    if form == '3x3_gn_res':
        sc = torch.rand((B, C0), generator=g) + 0.5
        sh = torch.randn((B, C0), generator=g) * 0.3
        a = F.silu(x.double() * sc.double()[:, None, None, :] + sh.double()[:, None, None, :])
        x_exp = 13 - int(np.floor(np.log2(float(a.abs().max()))))
        segs = [Seg(View.full(x.cuda()), TAPS3, scale=sc.cuda(), shift=sh.cuda(), silu=True),
                Seg(View.full(xr.cuda()), TAPS1, kbase=9 * C0)]
        assert not K.wgrad3_ok(View.full(dy.cuda()), segs[0])
        f3 = K.F3Bounds(gb, x_exp, None, xr.abs().amax((1, 2, 3)).cuda())
        dw = torch.zeros((M, C0, 3, 3), device='cuda')
        with lib:
            K.conv_wgrad(View.full(dy.cuda()), segs, dw, (C0 * 9, 9, 1), dw1=dwr, s1=C1, x6=True, f3=f3)
            torch.cuda.synchronize()
        w = torch.zeros((M, C0, 3, 3), dtype=torch.float64, requires_grad=True)
        F.conv2d(a.permute(0, 3, 1, 2), w, padding=1).backward(dy.double().permute(0, 3, 1, 2))
        ref = torch.einsum('bhwm,bhwc->mc', dy.double(), xr.double())
        assert ok(rel_l2(dwr.cpu(), ref)), rel_l2(dwr.cpu(), ref)
    elif form == '4x4s2_raw':
        f3 = K.F3Bounds(gb, 60, x.abs().amax((1, 2, 3)).cuda())
        dw = torch.zeros((M, C0, 4, 4), device='cuda')
        with lib:
            K.conv_wgrad(View.full(dy.cuda()), [Seg(View.full(x.cuda()), TAPS4S2, stride=2)], dw, (C0 * 16, 16, 1),
                         x6=True, f3=f3)
            torch.cuda.synchronize()
        w = torch.zeros((M, C0, 4, 4), dtype=torch.float64, requires_grad=True)
        F.conv2d(x.double().permute(0, 3, 1, 2), w, stride=2, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    else:
        f3 = K.F3Bounds(gb, 60, x.abs().amax((1, 2, 3)).cuda())
        dw = torch.zeros((M, C0), device='cuda')
        with lib:
            K.conv_wgrad(View.full(dy.cuda()), [Seg(View.full(x.cuda()), TAPS1)], dw, (C0, 1, 0), x6=True, f3=f3)
            torch.cuda.synchronize()
        w = torch.zeros((M, C0), dtype=torch.float64, requires_grad=True)
        (torch.einsum('bhwc,mc->bhwm', x.double(), w) * dy.double()).sum().backward()
    assert ok(rel_l2(dw.cpu(), w.grad)), rel_l2(dw.cpu(), w.grad)


def test_wgrad_reduce_many_splits_two_level():
    """More than 32 pixel splits: the split sums go through the two-level fixed-order reduction
    (groups of 32 slabs in place, then the groups in order); 1x1 weight gradient against float64,
    accumulate into an existing gradient, and bit-identical on a second run."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd._native import load
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS1
    g = _gen(6)
    B, H, W, C, M = 4, 64, 64, 128, 128
    assert load().wc_conv_wgrad_splits(M, C, B * H * W, 2048) > 32
    x = torch.randn((B, H, W, C), generator=g)
    dy = torch.randn((B, H, W, M), generator=g)
    base = torch.randn((M, C), generator=g)
    outs = []
    for _ in range(2):
        dw = base.clone().cuda()
        K.conv_wgrad(View.full(dy.cuda()), [Seg(View.full(x.cuda()), TAPS1)], dw, (C, 1, 0), accumulate=True, x6=True)
        outs.append(dw.cpu())
    ref = base.double() + torch.einsum('bhwm,bhwc->mc', dy.double(), x.double())
    assert rel_l2(outs[0], ref) < 1e-5
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize('x6', [False, True])
def test_conv_wgrad_4x4_stride2_and_transposed(x6):
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS4S2
    g = _gen(2)
    B, H, W, C, N = 2, 16, 24, 32, 64
    x = torch.randn((B, H, W, C), generator=g)
    dy = torch.randn((B, H // 2, W // 2, N), generator=g)
    dw = torch.zeros((N, C, 4, 4), device='cuda')
    K.conv_wgrad(View.full(dy.cuda()), [Seg(View.full(x.cuda()), TAPS4S2, stride=2)], dw, (C * 16, 16, 1), x6=x6)
    w = torch.zeros((N, C, 4, 4), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), w, stride=2, padding=1).backward(dy.double().permute(0, 3, 1, 2))
    assert rel_l2(dw.cpu(), w.grad) < 1e-5
    # ConvTranspose2d(C -> N, 4, 2, 1) weight gradient: x in the gradient role, dY through the 4x4/s2 taps
    xt = torch.randn((B, H // 2, W // 2, C), generator=g)
    dyt = torch.randn((B, H, W, N), generator=g)
    dwt = torch.zeros((C, N, 4, 4), device='cuda')
    K.conv_wgrad(View.full(xt.cuda()), [Seg(View.full(dyt.cuda()), TAPS4S2, stride=2)], dwt, (N * 16, 16, 1), x6=x6)
    wt = torch.zeros((C, N, 4, 4), dtype=torch.float64, requires_grad=True)
    F.conv_transpose2d(xt.double().permute(0, 3, 1, 2), wt, stride=2, padding=1).backward(
        dyt.double().permute(0, 3, 1, 2))
    assert rel_l2(dwt.cpu(), wt.grad) < 1e-5


@pytest.mark.parametrize('silu,C', [(True, 64), (False, 64), (True, 768), (True, 32), (False, 2048)])
def test_groupnorm_backward(silu, C):
    """GN(+SiLU) backward vs float64 autograd; C = 32 ... 2048 spans the finalize's group widths
    (4 ... 256 channels a workgroup)."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import View
    g = _gen(3)
    B, H, W = 3, 16, 8
    x = torch.randn((B, H, W, C), generator=g) * 2 + 0.5
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    dz = torch.randn((B, H, W, C), generator=g)
    base = torch.randn((B, H, W, C), generator=g)
    xc = View.full(x.cuda())
    sc, sh, a0, o0 = K.gn_stats_pair(xc, gamma.cuda(), beta.cuda())
    dx = base.cuda().clone()
    dg = torch.zeros(C, device='cuda')
    db = torch.zeros(C, device='cuda')
    K.gn_backward(View.full(dz.cuda()), xc, a0, o0, gamma.cuda(), beta.cuda(), silu, View.full(dx), dgamma=dg, dbeta=db,
                  accumulate=True)
    xd = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    gd = gamma.double().requires_grad_(True)
    bd = beta.double().requires_grad_(True)
    y = F.group_norm(xd, 8, gd, bd, 1e-5)
    y = F.silu(y) if silu else y
    y.backward(dz.double().permute(0, 3, 1, 2))
    assert rel_l2(dx.cpu() - base, xd.grad.permute(0, 2, 3, 1)) < 1e-5
    assert rel_l2(dg.cpu(), gd.grad) < 1e-5 and rel_l2(db.cpu(), bd.grad) < 1e-5


@pytest.mark.parametrize('silu,C,H,W', [(True, 128, 32, 32), (True, 768, 8, 8), (False, 64, 16, 24)])
def test_groupnorm_backward_closed_form_dx_sums(silu, C, H, W):
    """gn_backward(dx_sums=True): the per-(image, channel) sums of the dx it writes, from the reduce's
    sums in closed form (c0 sum dy + HW c1 + c2 sum xhat), against float64 autograd's dx summed over the
    pixels, within 1e-5 (rel-L2 over [B][C]) -- as close as a channel_sums pass over the written dx."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import View
    g = _gen(9)
    B = 3
    x = torch.randn((B, H, W, C), generator=g) * 2 + 0.5
    x[:, :, :, ::7] += 3.0  # channels whose mean is far from their group's
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.2
    dz = torch.randn((B, H, W, C), generator=g)
    xc = View.full(x.cuda())
    sc, sh, a0, o0 = K.gn_stats_pair(xc, gamma.cuda(), beta.cuda())
    dx = torch.empty((B, H, W, C), device='cuda')
    dsum = K.gn_backward(View.full(dz.cuda()), xc, a0, o0, gamma.cuda(), beta.cuda(), silu, View.full(dx),
                         accumulate=False, dx_sums=True)
    direct = K.channel_sums(View.full(dx))
    xd = x.double().permute(0, 3, 1, 2).requires_grad_(True)
    y = F.group_norm(xd, 8, gamma.double(), beta.double(), 1e-5)
    y = F.silu(y) if silu else y
    y.backward(dz.double().permute(0, 3, 1, 2))
    ref = xd.grad.sum((2, 3))
    assert dsum.shape == (B, C, 2) and bool((dsum[..., 1] == 0).all())
    e_closed, e_direct = rel_l2(dsum[..., 0].cpu(), ref), rel_l2(direct[..., 0].cpu(), ref)
    assert e_closed < 1e-5, (e_closed, e_direct)
    with pytest.raises(Exception):
        K.gn_backward(View.full(dz.cuda()), xc, a0, o0, gamma.cuda(), beta.cuda(), silu, View.full(dx),
                      accumulate=True, dx_sums=True)


@pytest.mark.parametrize('C', [4, 96, 200, 768])
def test_channel_sums_and_deferred_bsum(C):
    """channel_sums (the finalize's 64-channel blocks, ragged last block) vs float64, and the deferred
    bsum (one wc_bsum_batch launch, an output queued twice accumulating in queue order) bit-identical to
    one wc_bsum launch each."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import View
    g = _gen(5)
    B, H, W = 4, 8, 24
    x = torch.randn((B, H, W, C + 8), generator=g)
    sums = K.channel_sums(View(x.cuda(), 4, C))
    ref = x[..., 4:4 + C].double().sum((1, 2))
    assert rel_l2(sums[..., 0].cpu(), ref) < 1e-6 and bool((sums[..., 1] == 0).all())
    s2 = K.channel_sums(View(x.flip(0).contiguous().cuda(), 0, C))
    init = torch.randn(C, generator=g).cuda()
    outs_now = [init.clone(), torch.zeros(C, device='cuda')]
    K.bsum(sums, 0, outs_now[0], accumulate=True)
    K.bsum(s2, 0, outs_now[0], accumulate=True)
    K.bsum(s2, 1, outs_now[1])
    outs_def = [init.clone(), torch.full((C, ), 7.0, device='cuda')]
    K.bsum_defer()
    K.bsum(sums, 0, outs_def[0], accumulate=True)
    K.bsum(s2, 0, outs_def[0], accumulate=True)
    K.bsum(s2, 1, outs_def[1])
    assert bool((outs_def[0] == init).all())  # nothing launched before the flush
    K.bsum_flush()
    torch.cuda.synchronize()
    for a, b in zip(outs_now, outs_def):
        assert torch.equal(a, b)


# head dims 8, 24, 48, 96 and 160 (4 heads) at N = 33, 100, 200: a tail inside one 32-key tile, a tail across
# the 128-key workgroup, more than one workgroup; 24 ... 160 pad to the next multiple of 32 (BwdCfg::DP)
_ATTN_BWD_PADDED = [(C, 4, N) for C in (32, 96, 192, 384, 640) for N in (33, 100, 200) if (C, N) != (32, 33)]


@pytest.mark.parametrize('C,heads,N', [(64, 4, 200), (128, 4, 256), (256, 4, 96), (512, 4, 160), (768, 4, 64),
                                       (32, 4, 33)] + _ATTN_BWD_PADDED)
def test_attention_backward(C, heads, N):
    from weatherconverter_amd import kernels as K
    g = _gen(4)
    B = 2
    d = C // heads
    qkv = torch.randn((B * N, 3 * C), generator=g)
    do = torch.randn((B * N, C), generator=g)
    o = torch.empty((B * N, C), device='cuda')
    lse = torch.empty((B, heads, N), device='cuda')
    K.attention_fwd_lse(qkv.cuda(), o, lse, B, N, C, heads)
    dqkv = torch.empty((B * N, 3 * C), device='cuda')
    K.attention_bwd(qkv.cuda(), o, do.cuda(), lse, dqkv, B, N, C, heads)
    q_ = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    q, k, v = q_.split(C, dim=-1)
    sh = lambda z: z.reshape(B, N, heads, d).transpose(1, 2)  # noqa: E731
    att = torch.softmax((sh(q) * d**-0.5) @ sh(k).transpose(-1, -2), -1)
    out = (att @ sh(v)).transpose(1, 2).reshape(B, N, C)
    out.backward(do.double().reshape(B, N, C))
    assert rel_l2(o.cpu(), out.detach().reshape(B * N, C)) < 1e-5
    assert rel_l2(dqkv.cpu(), q_.grad.reshape(B * N, 3 * C)) < 1e-5


@pytest.mark.parametrize('Ci,N', [(64, 128), (256, 128), (128, 64), (512, 256)])
def test_pack_f16x3_convT_device_equals_cpu_definition(Ci, N):
    """The ConvT f16x3 pack in one device launch (the four parities side by side under their common
    scale) equals the torch definition evaluated on the CPU, bit for bit."""
    from weatherconverter_amd import kernels as K
    g = _gen(13)
    wt = torch.randn((Ci, N, 4, 4), generator=g) * torch.rand((1, N, 1, 1), generator=g) * 2
    dev = K.pack_f16x3_convT(wt.cuda())
    cpu = K.pack_f16x3_convT(wt)
    assert dev.order == cpu.order == 'f16x3t' and (dev.N, dev.BN, dev.C0) == (cpu.N, cpu.BN, cpu.C0)
    assert torch.equal(dev.data.cpu(), cpu.data.reshape(dev.data.shape)) and torch.equal(dev.wsinv.cpu(), cpu.wsinv)


@pytest.mark.parametrize('Co,Ci,res', [(128, 64, True), (256, 256, False), (64, 768, True), (48, 32, False)])
def test_pack_wino_raw_bit_identical_to_relayout(Co, Ci, res):
    """wc_pack_wino_raw from the module's [Co][Ci][3][3] weight (conv + residual, and the data gradient's
    flipped transposed filter) equals wc_pack_wino of the host re-layouts the engine used to build, bit
    for bit (pieces and scales)."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.diffusion_model.models.engine import pack_conv
    g = _gen(12)
    w = (torch.randn((Co, Ci, 3, 3), generator=g) * torch.rand((Co, 1, 1, 1), generator=g) * 3).cuda()
    wr = torch.randn((Co, Ci), generator=g).cuda() if res else None
    a = K.pack_wino_raw(w, wr)
    ref = K.pack_wino(torch.cat([pack_conv(w), wr], 1).contiguous() if res else pack_conv(w), Ci, Ci if res else 0,
                      device=True)
    assert torch.equal(a.data, ref.data) and torch.equal(a.wsinv, ref.wsinv) and (a.N, a.C0, a.C1) == (ref.N, ref.C0, ref.C1)
    if Co % 16 == 0:
        at = K.pack_wino_raw(w, transposed=True)
        reft = K.pack_wino(pack_conv(w.flip([2, 3]).transpose(0, 1)), Co, device=True)
        assert torch.equal(at.data, reft.data) and torch.equal(at.wsinv, reft.wsinv) and at.N == Ci
    # the batched launch (wc_pack_wino_batch, the training step's form) equals one launch each
    w2 = torch.randn((Ci, Co, 3, 3), generator=g).cuda()
    reqs = [(w, wr, False), (w, None, True), (w2, None, False), (w, None, False)]
    batch = K.pack_wino_raw_batch(reqs)
    for (w4, r, t), b in zip(reqs, batch):
        one = K.pack_wino_raw(w4, r, transposed=t)
        assert torch.equal(b.data, one.data) and torch.equal(b.wsinv, one.wsinv) and (b.N, b.C0, b.C1) == (one.N, one.C0, one.C1)


@pytest.mark.parametrize('precision', ['f16x3', 'bf16x6'])
@pytest.mark.parametrize('C,heads,N', [(128, 4, 256), (512, 4, 160), (768, 4, 64), (256, 4, 33), (128, 2, 1000)])
def test_split_attention_lse_matches_float64(precision, C, heads, N):
    """The training forward's split-precision attention (wc_attention_fwd_{f16x3,x6}_lse): output
    and log-sum-exp against float64, and the backward from its lse against float64 autograd."""
    from weatherconverter_amd import kernels as K
    g = _gen(6)
    B = 2
    d = C // heads
    qkv = torch.randn((B * N, 3 * C), generator=g)
    do = torch.randn((B * N, C), generator=g)
    do[:N] *= 1e-3  # images whose output gradients differ in scale (per-image dO exponent)
    o = torch.empty((B * N, C), device='cuda')
    lse = torch.empty((B, heads, N), device='cuda')
    exps = (10, 10, 10) if precision == 'f16x3' else None  # |randn| * 2^10 stays far inside fp16
    K.attention_fwd_lse(qkv.cuda(), o, lse, B, N, C, heads, precision=precision, exps=exps)
    dqkv = torch.empty((B * N, 3 * C), device='cuda')
    dob = do.abs().reshape(B, -1).amax(1).cuda() if precision == 'f16x3' else None
    amx = torch.zeros(B, device='cuda')
    prof = K.profile_conv(True)
    raised = K.attention_bwd(qkv.cuda(), o, do.cuda(), lse, dqkv, B, N, C, heads, precision=precision, exps=exps,
                             dout_bound=dob, dqkv_absmax=amx)
    if raised:  # the epilogue's per-image max |dqkv| equals a pass over what it wrote
        assert torch.equal(amx.cpu(), dqkv.cpu().abs().reshape(B, -1).amax(1))
    torch.cuda.synchronize()
    K.profile_conv(False)
    if C // heads in (32, 64, 128) or (C // heads == 192 and precision == 'f16x3'):
        # the split-precision backward ran (D = 192: dQ with the output dims in three parts, dK / dV with
        # the V rows in LDS; both raise the per-image bound)
        # the exact instantiation rocprofv3 prints, output-dim split DS included (3 at D = 192, else 1)
        f3 = 'true' if precision == 'f16x3' else 'false'
        ds = 3 if C // heads == 192 else 1
        names = [n for n, *_ in prof]
        assert f'attn_bwd6_dq_kernel<{C // heads}, {f3}, {ds}>' in names, names
    q_ = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    q, k, v = q_.split(C, dim=-1)
    sh = lambda z: z.reshape(B, N, heads, d).transpose(1, 2)  # noqa: E731
    sc = (sh(q) * d**-0.5) @ sh(k).transpose(-1, -2)
    ref_lse = torch.logsumexp(sc, -1) / np.log(2.0)  # log2 domain, [B][heads][N]
    out = (torch.softmax(sc, -1) @ sh(v)).transpose(1, 2).reshape(B, N, C)
    out.backward(do.double().reshape(B, N, C))
    assert rel_l2(o.cpu(), out.detach().reshape(B * N, C)) < 1e-5
    assert float((lse.cpu().double() - ref_lse.detach()).abs().max()) < 1e-5 * float(ref_lse.abs().max()) + 1e-6
    assert rel_l2(dqkv.cpu(), q_.grad.reshape(B * N, 3 * C)) < 1e-5
    # the small-gradient image on its own (its dO exponent is its own)
    assert rel_l2(dqkv.cpu()[:N], q_.grad.reshape(B * N, 3 * C)[:N]) < 1e-5


@pytest.mark.parametrize('C,heads,N', [(768, 4, 64), (768, 4, 1024), (512, 4, 160)])
def test_attention_backward_bf16_line_vs_float64(C, heads, N):
    """The bf16 training line's attention backward (libwc_kernels_bf16.so, one bf16 piece per operand):
    at D = 192 the whole head width runs in one workgroup (rows as pieces, no output-dim split:
    attn_bwd6_dq_kernel<192, true, 1> and the V-rows-in-LDS dK / dV at DS = 1), at D = 128 the generic
    pair; against float64 autograd within bf16 operand rounding (2^-9 relative per operand)."""
    from weatherconverter_amd import _native
    from weatherconverter_amd import kernels as K
    g = _gen(16)
    B, d = 2, C // heads
    qkv = torch.randn((B * N, 3 * C), generator=g)
    do = torch.randn((B * N, C), generator=g)
    do[:N] *= 1e-3
    exps = (10, 10, 10)
    with _native.variant('bf16'):
        o = torch.empty((B * N, C), device='cuda')
        lse = torch.empty((B, heads, N), device='cuda')
        K.attention_fwd_lse(qkv.cuda(), o, lse, B, N, C, heads, precision='f16x3', exps=exps)
        dqkv = torch.empty((B * N, 3 * C), device='cuda')
        dob = do.abs().reshape(B, -1).amax(1).cuda()
        amx = torch.zeros(B, device='cuda')
        prof = K.profile_conv(True)
        raised = K.attention_bwd(qkv.cuda(), o, do.cuda(), lse, dqkv, B, N, C, heads, precision='f16x3', exps=exps,
                                 dout_bound=dob, dqkv_absmax=amx)
        torch.cuda.synchronize()
        K.profile_conv(False)
    assert raised and torch.equal(amx.cpu(), dqkv.cpu().abs().reshape(B, -1).amax(1))
    names = [n for n, *_ in prof]
    assert f'attn_bwd6_dq_kernel<{d}, true, 1>' in names, names
    q_ = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    q, k, v = q_.split(C, dim=-1)
    sh = lambda z: z.reshape(B, N, heads, d).transpose(1, 2)  # noqa: E731
    sc = (sh(q) * d**-0.5) @ sh(k).transpose(-1, -2)
    out = (torch.softmax(sc, -1) @ sh(v)).transpose(1, 2).reshape(B, N, C)
    out.backward(do.double().reshape(B, N, C))
    ref = q_.grad.reshape(B * N, 3 * C)
    err = rel_l2(dqkv.cpu(), ref)
    err_small = rel_l2(dqkv.cpu()[:N], ref[:N])  # the small-gradient image, its own dO exponent
    print(f'bf16 line attention backward D={d} N={N}: rel-L2 {err:.3e} (small image {err_small:.3e})')
    assert 1e-5 < err < 2e-2 and err_small < 2e-2


@pytest.mark.parametrize('B,H,W,C,N', [(3, 16, 32, 128, 128), (2, 32, 16, 64, 64), (1, 8, 48, 256, 128)])
def test_dgrad_f16x3_raw_segment_per_image_bound(B, H, W, C, N):
    """The training backward's 3x3 data gradient on f16x3: a raw (no GroupNorm) operand whose
    per-image scale comes from wc_absmax_images; images of very different magnitude in one batch."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import Seg, View
    from weatherconverter_amd.diffusion_model.models.engine import TAPS3, pack_conv
    g = _gen(8)
    x = torch.randn((B, H, W, C), generator=g) * torch.tensor([1e-3, 50.0, 3.0])[:B, None, None, None]
    w = torch.randn((N, C, 3, 3), generator=g) / (9 * C)**0.5
    xv = View.full(x.cuda())
    bnd = K.absmax_images(xv)
    assert torch.equal(bnd.cpu(), x.abs().amax(dim=(1, 2, 3)))
    w3 = K.pack_f16x3(pack_conv(w.cuda()).float(), C)
    out = torch.empty((B, H, W, N), device='cuda')
    K.conv3x3_f16x3([Seg(xv, TAPS3)], w3, None, View.full(out), Hm=H, Wm=W, a_exp=60, a_bound=bnd)
    ref = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), padding=1).permute(0, 2, 3, 1)
    for b in range(B):  # every image to fp32-class accuracy against its own norm
        assert rel_l2(out[b].cpu(), ref[b]) < 1e-5


@pytest.mark.parametrize('N,C0,C1,ntaps,order,res_f16', [
    (128, 64, 0, 9, 'halo', False), (256, 128, 64, 9, 'halo', True), (256, 128, 64, 9, 'halo', False),
    (64, 32, 32, 9, 'halo', True), (96, 48, 0, 9, 'halo', False), (384, 128, 0, 1, 'natural', False),
    (512, 1536, 0, 1, 'natural', False), (130, 64, 0, 4, 'halo', False), (64, 256, 0, 1, 'natural', False)])
def test_device_pack_equals_torch_pack(N, C0, C1, ntaps, order, res_f16):
    """wc_pack_split (one launch per weight) is bit for bit the torch-op definitions pack_f16x3 /
    pack_x6, including row scales (an all-zero row, a power-of-two maximum), tile padding and the
    residual segment in both encodings."""
    from weatherconverter_amd import kernels as K
    g = _gen(12)
    w = torch.randn((N, ntaps * C0 + C1), generator=g) * torch.exp(torch.randn((N, 1), generator=g) * 3)
    w[0] = 0.0
    w[1, 0] = 2.0 * float(w[1].abs().max()) if w.shape[0] > 1 else 0.0
    if N > 2:
        w[2] = w[2] / w[2].abs().max() * 0.25  # maximum exactly 2^-2
    # the reference: the torch definitions evaluated on the CPU (IEEE fp32 / RNE fp16 conversions)
    a = K.pack_f16x3(w.cuda(), C0, C1, ntaps=ntaps, order=order, res_f16=res_f16, device=True)
    b = K.pack_f16x3(w, C0, C1, ntaps=ntaps, order=order, res_f16=res_f16, device=False)
    ad, bd = a.data.cpu(), b.data

    def first_diff(x, y):
        i = int((x != y).flatten().nonzero()[0])
        return f'{int((x != y).sum())} of {x.numel()} differ; first at flat {i}: {int(x.flatten()[i])} vs {int(y.flatten()[i])}'
    assert ad.shape == bd.shape
    assert torch.equal(ad, bd), first_diff(ad, bd)
    assert torch.equal(a.wsinv.cpu(), b.wsinv) and (a.order, a.BN, a.res_f16) == (b.order, b.BN, b.res_f16)
    if order == 'natural' or ntaps == 9:
        a6 = K.pack_x6(w.cuda(), C0, C1, ntaps=ntaps, order=order, device=True)
        b6 = K.pack_x6(w, C0, C1, ntaps=ntaps, order=order, device=False)
        assert torch.equal(a6.data.cpu(), b6.data), first_diff(a6.data.cpu(), b6.data)


@pytest.mark.parametrize('N,C0,C1,ntaps,order,res_f16', [
    (256, 128, 64, 9, 'halo', True), (96, 48, 0, 9, 'halo', False), (384, 128, 0, 1, 'natural', False)])
def test_device_pack_equals_torch_pack_bf16_line(N, C0, C1, ntaps, order, res_f16):
    """The same on the bf16 single-piece library (libwc_kernels_bf16.so): one bf16 piece, the low piece
    zero on both sides (the device packs write l = 0, and so does the CPU definition)."""
    from weatherconverter_amd import _native
    from weatherconverter_amd import kernels as K
    g = _gen(13)
    w = torch.randn((N, ntaps * C0 + C1), generator=g) * torch.exp(torch.randn((N, 1), generator=g) * 3)
    with _native.variant('bf16'):
        a = K.pack_f16x3(w.cuda(), C0, C1, ntaps=ntaps, order=order, res_f16=res_f16, device=True)
        b = K.pack_f16x3(w, C0, C1, ntaps=ntaps, order=order, res_f16=res_f16, device=False)
        torch.cuda.synchronize()
    assert torch.equal(a.data.cpu(), b.data)
    assert torch.equal(a.wsinv.cpu(), b.wsinv)
    # every K-step is [piece 2][k-half 2][BN][8]: the low pieces are all zero
    assert int(torch.count_nonzero(b.data.view(-1, 2, 2 * b.BN * 8)[:, 1])) == 0


# ------------------------------------------------------------------ whole model
_REF_GRADS = {}  # share_ref: (config, B, seed, t) -> (oracle float64 grads, loss)


def _model_grads(mc, B, precision, seed=0, t=None, share_ref=False):
    """(our grads, oracle float64 grads, loss ours, loss ref) for one MSE training iteration;
    precision 'f16' = the 16-bit training line (set_train_precision).  t: the per-sample timesteps
    (int64 [B]; drawn from the seeded generator when None).  share_ref: compute the oracle's gradients
    (they do not depend on the precision) once per (config, B, seed, t) and keep them, unchanged."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    from oracle.unet_oracle import unet_forward
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.synthetic import init_synthetic_
    net = Unet(mc)
    init_synthetic_(net, seed=seed)
    sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in net.state_dict().items()}
    if precision in ('f16', 'bf16'):
        net.set_train_precision(precision)
    else:
        net.set_conv_precision(precision)
    net = net.cuda().train()
    g = _gen(11)
    S = mc.im_size
    x = torch.randn((B, mc.im_channels, S, S), generator=g)
    noise = torch.randn((B, mc.im_channels, S, S), generator=g)
    t_drawn = torch.randint(0, 1000, (B, ), generator=g)
    t = t_drawn if t is None else t
    assert t.shape == (B, ) and t.dtype == torch.int64
    pred = net(x.cuda(), t.cuda())
    loss = torch.nn.MSELoss()(pred, noise.cuda())
    loss.backward()
    ours = {k: p.grad.detach().cpu().double() for k, p in net.named_parameters()}
    key = (mc.model_dump_json(), B, seed, tuple(t.tolist()))
    if not share_ref or key not in _REF_GRADS:
        ref_pred = unet_forward(sd, mc, x.double(), t)
        ref_loss = torch.nn.MSELoss()(ref_pred, noise.double())
        ref_loss.backward()
        if not share_ref:
            return ours, {k: sd[k].grad for k in ours}, float(loss), float(ref_loss)
        _REF_GRADS[key] = ({k: sd[k].grad for k in ours}, float(ref_loss.detach()))
    ref, ref_loss = _REF_GRADS[key]
    return ours, ref, float(loss), ref_loss


def _grad_errors(ours, ref):
    """{name: rel-L2} of every gradient tensor, and of the q, k and v row blocks of every attention
    in-projection gradient as tensors of their own ('name[q]' ...): with a diffuse softmax the q and k rows
    are far smaller than the v rows, so an error in them (the f16x3 attention backward's dS) hides under the
    per-tensor bound of the whole in_proj_weight.  The k block of in_proj_bias is exactly zero in exact
    arithmetic (a constant added to every key moves no softmax: sum_j dS_ij = 0), so its error is measured
    against the norm of the whole bias gradient, as the per-tensor check always measured it."""
    errs = {k: rel_l2(ours[k], ref[k]) for k in ref}
    for k in ref:
        if k.endswith(('in_proj_weight', 'in_proj_bias')):
            c = ref[k].shape[0] // 3
            for i, n in enumerate('qkv'):
                a, b = ours[k][i * c:(i + 1) * c], ref[k][i * c:(i + 1) * c]
                zero = n == 'k' and k.endswith('in_proj_bias')
                errs[f'{k}[{n}]'] = float((a - b).norm() / ref[k].norm()) if zero else rel_l2(a, b)
    return errs


def _check(ours, ref, per_tensor=1e-4, overall=1e-5):
    worst = sorted(((e, k) for k, e in _grad_errors(ours, ref).items()), reverse=True)
    a = torch.cat([ours[k].flatten() for k in ref])
    b = torch.cat([ref[k].flatten() for k in ref])
    tot = rel_l2(a, b)
    print(f'overall grad rel-L2 {tot:.3e}; worst tensors {worst[:4]}')
    print('worst in-projection q / k blocks', [w for w in worst if w[1].endswith(('[q]', '[k]'))][:4])
    assert all(ours[k].shape == ref[k].shape for k in ref)
    assert tot < overall, tot
    assert worst[0][0] < per_tensor, worst[:4]


@pytest.mark.parametrize('precision', ['f16x3', 'bf16x6', 'fp32'])
def test_unet_grads_tiny_vs_oracle_autograd(precision):
    import json
    import os
    from conftest import GOLDEN
    from weatherconverter_amd import forms
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    mc = ModelConfig(**man['tiny']['config'])
    # f16x3: every tracked gradient range bound is checked against a fresh absmax of its tensor
    with forms.using(check_gbound=True):
        ours, ref, lo, lr = _model_grads(mc, 3, precision)
    assert abs(lo - lr) <= 1e-5 * abs(lr)
    _check(ours, ref)


@pytest.mark.parametrize('line', ['f16', 'bf16'])
def test_unet_grads_16bit_training_lines_vs_oracle_autograd(line):
    """The 16-bit training lines (train precision 'f16': the single-piece build, one fp16 piece per
    operand; 'bf16': one bf16 piece per operand on the bf16 MFMA, BASELINE config 3's arithmetic; fp32
    accumulation) on the 256-px architecture at B=2: their gradient error against float64 autograd is
    that of 16-bit operands — bounded here at 2e-2 (f16) / 6e-2 (bf16) overall and 1e-1 / 3e-1 per
    tensor (the fp32-class modes: 1e-5 / 1e-4) — and the single-piece kernels actually ran (their error
    is far above f16x3's)."""
    from weatherconverter_amd import _native, forms
    from weatherconverter_amd.diffusion_model.config import model_config
    with forms.using(check_gbound=True):
        ours, ref, lo, lr = _model_grads(model_config(256), 2, line)
    assert {'f16': 'single16', 'bf16': 'bf16'}[line] in _native._libs
    a = torch.cat([ours[k].flatten() for k in ref])
    b = torch.cat([ref[k].flatten() for k in ref])
    tot = rel_l2(a, b)
    print(f'{line} training line: overall grad rel-L2 {tot:.3e}, loss {lo:.6f} vs {lr:.6f}')
    assert abs(lo - lr) <= (1e-3 if line == 'f16' else 8e-3) * abs(lr)
    overall = 2e-2 if line == 'f16' else 6e-2
    assert 1e-5 < tot < overall
    _check(ours, ref, per_tensor=1e-1 if line == 'f16' else 3e-1, overall=overall)


def test_unet_grads_256_baseline_architecture_vs_oracle_autograd():
    from weatherconverter_amd import forms
    from weatherconverter_amd.diffusion_model.config import model_config
    with forms.using(check_gbound=True):
        ours, ref, lo, lr = _model_grads(model_config(256), 2, 'f16x3')
    assert len(ref) == 358
    assert abs(lo - lr) <= 1e-5 * abs(lr)
    _check(ours, ref)


def test_train_backward_deterministic_and_adam_step():
    """Two backward passes give bit-identical gradients; the reference's loop (Adam step) runs."""
    import json
    import os
    from conftest import GOLDEN
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.synthetic import init_synthetic_
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    mc = ModelConfig(**man['tiny']['config'])
    net = Unet(mc)
    init_synthetic_(net, seed=0)
    net = net.cuda().train()
    g = _gen(5)
    x = torch.randn((2, 3, 32, 32), generator=g).cuda()
    noise = torch.randn((2, 3, 32, 32), generator=g).cuda()
    t = torch.tensor([5, 700]).cuda()
    grads = []
    for _ in range(2):
        net.zero_grad()
        torch.nn.MSELoss()(net(x, t), noise).backward()
        grads.append([p.grad.clone() for p in net.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    opt = torch.optim.Adam(net.parameters(), lr=1e-4)
    before = [p.detach().clone() for p in net.parameters()]
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = torch.nn.MSELoss()(net(x, t), noise)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    assert all(np.isfinite(losses))
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    assert losses[-1] < losses[0]  # same batch, small steps: the loss goes down


def test_two_forwards_then_two_backwards_accumulate():
    """Gradient accumulation: forward(a), forward(b), then backward of each.  Every forward owns its
    tape, so the accumulated gradients equal two separate forward+backward passes; a second backward
    through an already-consumed forward raises instead of returning zeros."""
    import json
    import os
    from conftest import GOLDEN
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.synthetic import init_synthetic_
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    mc = ModelConfig(**man['tiny']['config'])
    net = Unet(mc)
    init_synthetic_(net, seed=0)
    net = net.cuda().train()
    g = _gen(9)
    xa, xb = (torch.randn((2, 3, 32, 32), generator=g).cuda() for _ in range(2))
    na, nb = (torch.randn((2, 3, 32, 32), generator=g).cuda() for _ in range(2))
    ta, tb = torch.tensor([5, 700]).cuda(), torch.tensor([321, 42]).cuda()
    mse = torch.nn.MSELoss()
    net.zero_grad()
    mse(net(xa, ta), na).backward()
    mse(net(xb, tb), nb).backward()
    ref = [p.grad.clone() for p in net.parameters()]
    net.zero_grad()
    la = mse(net(xa, ta), na)
    lb = mse(net(xb, tb), nb)
    la.backward(retain_graph=True)
    lb.backward()
    got = [p.grad.clone() for p in net.parameters()]
    for a, b in zip(got, ref):
        assert torch.allclose(a, b, rtol=1e-6, atol=1e-9), float((a - b).abs().max())
    with pytest.raises(RuntimeError, match='consumed'):
        la.backward()
    with pytest.raises(RuntimeError, match='input image'):
        net(xa.clone().requires_grad_(True), ta)


@pytest.mark.parametrize('B,H,W,C,ld', [(3, 17, 9, 4, 4), (2, 16, 16, 64, 128), (2, 8, 12, 768, 768), (1, 5, 7, 1536, 1600),
                                        (2, 32, 33, 96, 96)])
def test_absmax_images_vs_torch(B, H, W, C, ld):
    """wc_absmax_images: per-image max |x| over a channel view (pitch ld), every channel-quad / pixel mapping
    (C/4 dividing 256 or not, above 256 quads) and ragged pixel ranges."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.kernels import View
    g = _gen(21)
    t = torch.randn((B, H, W, ld), generator=g) * torch.rand((B, 1, 1, 1), generator=g) * 10
    t[..., C:] = 1e6  # outside the view: must not count
    got = K.absmax_images(View(t.cuda(), 0, C))
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), t[..., :C].abs().reshape(B, -1).amax(1))


# ------------------------------------------------------------------ the helpers behind the time-embedding backward
# Each is a plain fp32 loop with no split arithmetic: rel-L2 <= 1e-6 against float64 torch.
@pytest.mark.parametrize('K_', [64, 300])
@pytest.mark.parametrize('ta,tb', [(False, False), (True, False), (False, True), (True, True)])
def test_gemm_small_vs_float64(K_, ta, tb):
    """wc_gemm_small: both kernels (a thread per output below K = 256, a wave per output from there), M x N
    with a tail (5 x 37), either operand stored transposed, non-zero element offsets, alpha != 1, beta 0
    (C is not read: a NaN-filled C comes out finite) and beta 1."""
    from weatherconverter_amd import _native
    from weatherconverter_amd import kernels as K
    g = _gen(31)
    M, N = 5, 37
    oa, ob, oc = 7, 3, 11
    A = torch.randn((M, K_), generator=g)
    Bm = torch.randn((K_, N), generator=g)
    C0 = torch.randn((M, N), generator=g)
    a_st = torch.cat([torch.full((oa, ), 1e9), (A.t() if ta else A).contiguous().flatten()])
    b_st = torch.cat([torch.full((ob, ), 1e9), (Bm.t() if tb else Bm).contiguous().flatten()])
    sa = (1, M) if ta else (K_, 1)
    sb = (1, K_) if tb else (N, 1)
    prod = A.double() @ Bm.double()
    for alpha, beta in ((1.0, 0.0), (-1.5, 0.0), (0.5, 1.0)):
        c_st = torch.cat([torch.zeros(oc), (C0 if beta else torch.full((M, N), float('nan'))).flatten()]).cuda()
        _native.last_kernel_name()
        K.gemm_small(M, N, K_, a_st.cuda(), sa, b_st.cuda(), sb, c_st, N, alpha=alpha, beta=beta, offs=(oa, ob, oc))
        name = _native.last_kernel_name()
        assert name == ('gemm_small_wave_kernel' if K_ >= 256 else ''), name  # only the wave kernel names itself
        out = c_st.cpu()
        assert bool((out[:oc] == 0).all())
        got = out[oc:].reshape(M, N)
        assert bool(torch.isfinite(got).all())
        err = rel_l2(got, alpha * prod + beta * C0.double())
        print(f'gemm_small K={K_} ta={ta} tb={tb} alpha={alpha} beta={beta}: rel-L2 {err:.3e}')
        assert err < 1e-6


def test_colsum_vs_float64():
    """wc_colsum: a column range inside a wider X (col0 / ncol), whole rows, and accumulate."""
    from weatherconverter_amd import kernels as K
    g = _gen(32)
    R, Ntot, col0, ncol = 7, 300, 13, 259  # ncol above one 256-thread block, with a tail
    X = torch.randn((R, Ntot), generator=g)
    init = torch.randn(ncol, generator=g)
    out = torch.full((ncol, ), float('nan'), device='cuda')
    K.colsum(X.cuda(), out, col0=col0, ncol=ncol)
    ref = X[:, col0:col0 + ncol].double().sum(0)
    assert rel_l2(out.cpu(), ref) < 1e-6
    acc = init.clone().cuda()
    K.colsum(X.cuda(), acc, accumulate=True, col0=col0, ncol=ncol)
    assert rel_l2(acc.cpu(), init.double() + ref) < 1e-6
    whole = torch.empty(Ntot, device='cuda')
    K.colsum(X.cuda(), whole)
    assert rel_l2(whole.cpu(), X.double().sum(0)) < 1e-6


def test_silu_map_vs_float64():
    """wc_silu, both modes (silu(y); dz * silu'(y)) at n = 3 * 171 (no multiple of 256)."""
    from weatherconverter_amd import kernels as K
    g = _gen(33)
    y = torch.randn((3, 171), generator=g) * 3
    dz = torch.randn((3, 171), generator=g)
    yd = y.double().requires_grad_(True)
    F.silu(yd).backward(dz.double())
    e0 = rel_l2(K.silu_map(y.cuda()).cpu(), F.silu(y.double()))
    e1 = rel_l2(K.silu_map(y.cuda(), dz.cuda()).cpu(), yd.grad)
    print(f'silu_map rel-L2: value {e0:.3e}, gradient {e1:.3e}')
    assert e0 < 1e-6 and e1 < 1e-6


@pytest.mark.parametrize('D', [64, 128, 256])
def test_time_embedding_both_device_routes(D):
    """wc_time_embedding (the training backward's embedding) at t = 0, 1, 500, 999 against the oracle's fp32
    recipe, and against the embedding inside wc_temb (the forward's): with identity matrices and zero biases
    for t_proj and the projection, wc_temb returns silu(silu(e)) of ITS embedding e exactly (every product
    is by 0 or 1), and wc_silu applied twice to wc_time_embedding's e gives the same of the other route's.
    The two routes evaluate the same expressions (f_k rounded once to fp32, fp32 division, sinf / cosf) and
    agree bit for bit (measured on an MI355X; asserted).  Against the oracle both lie at 2e-8; with f_k from
    powf they lay at 4.8e-6 ... 6.9e-6 (max abs 6.1e-5 at t = 999: one ulp of f_k is one ulp of t / f_k)."""
    import sys
    from conftest import ROOT
    sys.path.insert(0, ROOT)
    from oracle.unet_oracle import time_embedding
    from weatherconverter_amd import kernels as K
    t = torch.tensor([0, 1, 500, 999])
    e = K.time_embedding(t.cuda(), D)
    ref = time_embedding(t, D)
    err = rel_l2(e.cpu(), ref)
    worst = float((e.cpu() - ref).abs().max())
    eye, zero = torch.eye(D, device='cuda'), torch.zeros(D, device='cuda')
    via_temb = K.temb(t.cuda(), eye, zero, eye, zero, eye, zero)
    via_silu = K.silu_map(K.silu_map(e))
    same = torch.equal(via_temb, via_silu)
    print(f'time_embedding D={D}: rel-L2 vs the oracle {err:.3e}, max abs {worst:.3e}; wc_temb and '
          f'wc_time_embedding bit-identical: {same} (max abs {float((via_temb - via_silu).abs().max()):.3e})')
    assert e.shape == (4, D) and bool((e[0, :D // 2] == 0).all()) and bool((e[0, D // 2:] == 1).all())
    assert err < 1e-6
    assert same


@pytest.mark.parametrize('C', [1, 3, 4])
@pytest.mark.parametrize('ldc', [4, 32])
def test_nchw_to_nhwc_zero_padded(C, ldc):
    """wc_nchw_to_nhwc: C image channels into ldc NHWC channels, the rest zero (a copy: exact)."""
    from weatherconverter_amd import kernels as K
    x = torch.randn((3, C, 5, 7), generator=_gen(34))
    out = K.nchw_to_nhwc(x.cuda(), ldc).cpu()
    assert out.shape == (3, 5, 7, ldc)
    assert torch.equal(out[..., :C], x.permute(0, 2, 3, 1)) and bool((out[..., C:] == 0).all())
