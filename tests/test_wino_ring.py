"""The four-buffer halo ring of the 8-wave pre-split Winograd conv (csrc/wc_wino.hip: conv3x3_wino_kernel
<8, 256, 3, *, 2, 8, 4>, wc_conv3x3_wino_f16x3_vp8 through kernels.wino_vp_wide): one barrier per two chunks,
chunks entering the unrolled round of four by remainder, the residual centres written one barrier ahead and
the residual tail's buffer hand-over.

The oracle is the in-conv prologue form (wc_conv3x3_wino_f16x3) on the same inputs: both run every MFMA
in the same order, so the output, the GroupNorm partials and the per-image absmax must be equal bit for bit.
Shapes: the smallest at which the ring can go wrong -- 16-channel chunk counts below, at and above one round of
four, residual chunk counts below, equal to and above the 3x3 count (odd and even tails), one row tile (every
halo row 0 and 9 outside the image) and several, one and three column tiles, one and two output tiles.
"""
import pytest
import torch

TAPS3 = [(ky - 1, kx - 1) for ky in range(3) for kx in range(3)]
B = 2


def _both_forms(H, W, C0, N, C1, res_scale=None):
    """The conv as the in-conv prologue form and as the 8-wave pre-split form: ((out, absmax, GN partials) of
    each, the pre-split launch's kernel name, the residual's per-image bound or None)."""
    from weatherconverter_amd import kernels as K
    g = torch.Generator().manual_seed(61 + C0 + C1)
    x = (torch.randn((B, H, W, C0), generator=g) * 2 + 1).cuda()
    w = (torch.randn((N, 9 * C0 + C1), generator=g) / (9 * C0)**0.5).cuda()
    bias = torch.randn(N, generator=g).cuda()
    temb = torch.randn((B, N), generator=g).cuda()
    sc = (1 + 0.2 * torch.randn((B, C0), generator=g)).cuda()
    sh = (0.2 * torch.randn((B, C0), generator=g)).cuda()
    segs = [K.Seg(K.View.full(x), TAPS3, scale=sc, shift=sh, silu=True)]
    kw = dict(a_exp=6, temb=temb, temb_ld=N)
    if C1:
        xr = torch.randn((B, H, W, C1), generator=g)
        if res_scale is not None:
            xr = xr * torch.tensor(res_scale).reshape(B, 1, 1, 1)
        xr = xr.cuda()
        segs.append(K.Seg(K.View.full(xr), [(0, 0)], kbase=9 * C0))
        kw['a_bound'] = xr.abs().reshape(B, -1).amax(1).contiguous() * 1.5
    wp = K.pack_wino(w, C0, C1)
    res, name = [], None
    prev = K.set_wino_vsplit(0)
    try:
        for presplit in (0, 1):
            K.set_wino_vsplit(presplit)
            y = torch.empty((B, H, W, N), device='cuda')
            gp = K.GnPart.attach(y, 16)
            amax = torch.zeros(B, device='cuda')
            with K.wino_vp_wide(True):
                K.conv3x3_wino(segs, wp, bias, K.View.full(y), Hm=H, Wm=W, absmax=amax, gn=gp, **kw)
            name = K._native.last_kernel_name()
            torch.cuda.synchronize()
            res.append((y.cpu(), amax.cpu(), gp.part.cpu()))
    finally:
        K.set_wino_vsplit(prev)
    return res, name, kw.get('a_bound')


def _assert_bit_identical(H, W, C0, N, C1, res_scale=None):
    (ref, got), name, bound = _both_forms(H, W, C0, N, C1, res_scale)
    assert name.startswith('conv3x3_wino_kernel<8, 256, 3, ' + ('true' if C1 else 'false')), name
    assert torch.isfinite(ref[0]).all()
    for what, a, b in zip(('out', 'absmax', 'gn partials'), ref, got):
        assert torch.equal(a, b), (what, int((a != b).sum()), float((a - b).abs().max()))
    return bound


@pytest.mark.gpu
@pytest.mark.parametrize('C0', [16, 32, 48, 64, 80, 144])
def test_ring_chunk_counts_around_the_round_of_four(C0):
    """nck0 = 1, 2, 3, 4, 5, 9: the last chunk alone, every entry remainder, one and two whole rounds."""
    _assert_bit_identical(16, 16, C0, 256, 0)


@pytest.mark.gpu
@pytest.mark.parametrize('C1', [16, 48, 80, 112])
def test_ring_residual_chunks_below_equal_above(C1):
    """nck0 = 3 with nck1 = 1, 3, 5, 7: residual steps riding in some, all of the 3x3 chunks, then a tail of
    two and of four steps (odd tails: test_ring_residual_odd_tail)."""
    _assert_bit_identical(16, 16, 48, 256, C1)


@pytest.mark.gpu
def test_ring_residual_odd_tail():
    _assert_bit_identical(16, 16, 48, 256, 64)   # nck1 - nck0 = 1
    _assert_bit_identical(16, 16, 32, 256, 80)   # nck0 = 2, a tail of three


@pytest.mark.gpu
@pytest.mark.parametrize('H,W,N,C0,C1', [
    (8, 16, 256, 80, 0),     # one row tile: halo rows 0 and 9 of every workgroup outside the image
    (8, 16, 256, 48, 80),
    (24, 16, 256, 80, 0),    # three row tiles
    (16, 48, 256, 80, 0),    # three column tiles
    (24, 48, 256, 48, 112),
    (16, 16, 512, 80, 0),    # two output tiles per pixel block
    (16, 16, 512, 48, 80),
])
def test_ring_borders_and_tiles(H, W, N, C0, C1):
    _assert_bit_identical(H, W, C0, N, C1)


@pytest.mark.gpu
@pytest.mark.parametrize('line', ['single16', 'bf16'])
def test_ring_single_piece_lines(line):
    """The single-piece builds copy half the planes per chunk (10 LDS-DMA pieces over 8 waves instead of 20):
    the same ring, against the in-conv prologue of the same build."""
    from weatherconverter_amd import _native
    with _native.variant(line):
        _assert_bit_identical(16, 16, 80, 256, 48)


@pytest.mark.gpu
def test_ring_distinct_images():
    """A residual bound per image (x 1 and x 4096): the second image's exponent is clamped by its bound, the
    first's is the GroupNorm one, so s differs across b -- and so do the outputs' scales."""
    bound = _assert_bit_identical(16, 16, 80, 256, 48, res_scale=[1.0, 4096.0])
    # the kernel's s: min(a_exp - 1, 13 - exponent of the bound), a_exp = 6
    s = [min(5, 13 - int(torch.floor(torch.log2(b)))) for b in bound.cpu()]
    assert s[0] == 5 and s[1] < 5, s
