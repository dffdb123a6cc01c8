"""GPU: the kernel arms a SHAPE selects.  UnetEngine and TrainEngine pick most kernels by shape predicates
(wino_eligible, x6_eligible, gn_conv_ok, GnPart.eligible, _sw, qkv_presplit_ok, proj_pa_ok, conv4x4s2_f16x3_ok,
convT4x4s2_f16x3_ok, _dgrad3_ok, wgrad3_ok, the head-dim rules of the attention wrappers, ...), and every other
whole-model test stays on one grid: square power-of-two inputs, channel counts that are multiples of 32, 4 heads,
time_emb_dim 128, 3 image channels.  Each case below is `tiny` (tests/golden/manifest.json) plus overrides that
leave that grid somewhere, and is run
  * forward (eval, no_grad) in f16x3, bf16x6 and fp32 against the float64 oracle, rel-L2 < 1e-5;
  * one training step (train mode, check_gbound) in the three precisions against the oracle's float64 autograd
    with test_gpu_train._check: loss within 1e-5 relative, gradients < 1e-5 overall and < 1e-4 per tensor;
  * for its census: the native entry points the f16x3 forward / training step must and must not reach
    (Shape.fwd_present / fwd_never / train_present / train_never, fnmatch globs over the names
    test_gpu_forms._recording counts), and, for every case whose arm is an entry point, a census that differs
    from tiny's at 2 x 32 x 32 -- a case that reaches exactly tiny's entry points proves nothing about dispatch;
  * row b of the batched forward against image b run alone, bit for bit (the engine's batch independence);
  * forward and training step with every fresh allocation poisoned (test_gpu_forms._poisoned_allocations),
    finite and bit-identical to the plain run: the fallback arms allocate scratch the on-grid run never creates.
Mutation check of the matrix: with GnPart.eligible ignoring HW % 64, rect, sq24, tall and deep fail (forward
and census: wc_gn_partials refuses the 8 x 12, 6 x 6, 10 x 6 and 4 x 4 levels) while every on-grid whole-model
forward test (test_gpu_unet, test_gpu_forms) still passes.
A configuration outside the envelope engine.check_supported states (ch48; training with 6 image channels)
must raise at engine construction before any native call.

The census, f16x3, as counted on an MI355X (entry point: forward count / training-step count; tiny at
2 x 32 x 32 first, then per case only what differs in kind):
  tiny  absmax_images 0/50, attention_bwd 0/7, attention_bwd_f16x3 0/3, attention_fwd 7/0, attention_fwd_f16x3 3/0,
        attention_fwd_f16x3_lse 0/3, attention_fwd_lse 0/7, bsum_batch 0/1, colsum 0/18, conv3x3_f16x3 8/8,
        conv3x3_wino_f16x3 8/8, conv3x3_wino_f16x3_gnb 0/16, conv_igemm_f16x3 21/36, conv_igemm_x6 21/68, conv_in
        1/1, conv_wgrad3_f16x3 0/7, conv_wgrad_f16x3 0/37, conv_wgrad_x6 0/16, convtr4x4s2_f16x3 1/1, gemm_small
        0/22, gn_bwd_apply 0/43, gn_bwd_finalize 0/84, gn_bwd_reduce 0/68, gn_finalize 0/40, gn_finalize_bound 0/12,
        gn_finalize_part 43/34, gn_partials 25/0, gn_stats 0/26, head_conv 1/1, head_dgrad 0/1, head_wgrad 0/1,
        pack_split 128/114, pack_wino 32/0, pack_wino_batch 0/1, silu 0/4, stem_wgrad 0/1, temb 1/1, time_embedding
        0/1, wgrad_reduce 0/60
  rect  absmax_images 0/42, conv3x3_f16x3 4/4, conv3x3_wino_f16x3 4/4, conv3x3_wino_f16x3_gnb 0/8, conv_igemm_f16x3
        20/24, conv_igemm_x6 34/100, conv_wgrad3_f16x3 0/3, conv_wgrad_f16x3 0/31, conv_wgrad_x6 0/24,
        convtr4x4s2_f16x3 0/0, gn_bwd_reduce 0/76, gn_finalize 14/58, gn_finalize_bound 8/14, gn_finalize_part
        21/14, gn_partials 16/0, gn_stats 22/36, pack_split 128/130, wgrad_reduce 0/58
  sq24  absmax_images 0/21, attention_bwd 0/2, attention_fwd 2/0, attention_fwd_lse 0/2, colsum 0/12, conv3x3_f16x3
        0/0, conv3x3_wino_f16x3 0/0, conv3x3_wino_f16x3_gnb 0/0, conv_igemm_f16x3 10/10, conv_igemm_x6 30/80,
        conv_in 0/1, conv_in_gn 1/0, conv_wgrad3_f16x3 0/0, conv_wgrad_f16x3 0/14, conv_wgrad_x6 0/20,
        convtr4x4s2_f16x3 0/0, gemm_small 0/16, gn_bwd_apply 0/26, gn_bwd_finalize 0/51, gn_bwd_reduce 0/51,
        gn_finalize 11/42, gn_finalize_bound 6/10, gn_finalize_part 9/0, gn_partials 9/0, gn_stats 17/26, pack_split
        86/97, pack_wino 20/0, wgrad_reduce 0/34
  tall  absmax_images 0/21, attention_bwd 0/2, attention_fwd 2/0, attention_fwd_lse 0/2, colsum 0/12, conv3x3_f16x3
        0/0, conv3x3_wino_f16x3 0/0, conv3x3_wino_f16x3_gnb 0/0, conv_igemm_f16x3 10/10, conv_igemm_x6 30/80,
        conv_in 0/1, conv_in_gn 1/0, conv_wgrad3_f16x3 0/0, conv_wgrad_f16x3 0/14, conv_wgrad_x6 0/20,
        convtr4x4s2_f16x3 0/0, gemm_small 0/16, gn_bwd_apply 0/26, gn_bwd_finalize 0/51, gn_bwd_reduce 0/51,
        gn_finalize 11/42, gn_finalize_bound 6/10, gn_finalize_part 9/0, gn_partials 9/0, gn_stats 17/26, pack_split
        86/97, pack_wino 20/0, wgrad_reduce 0/34
  ch96  absmax_images 0/47, attention_bwd 0/9, attention_bwd_f16x3 0/0, attention_fwd 9/0, attention_fwd_f16x3 0/0,
        attention_fwd_f16x3_lse 0/0, attention_fwd_lse 0/9, bsum 0/1, colsum 0/16, conv3x3_f16x3 0/0,
        conv3x3_wino_f16x3 16/16, conv4x4s2_f16x3 1/2, conv_igemm_f16x3 18/34, conv_igemm_x6 17/52,
        conv_wgrad3_f16x3 0/3, conv_wgrad_x6 0/14, convtr4x4s2_f16x3 1/2, gemm_small 0/20, gn_bwd_apply 0/38,
        gn_bwd_finalize 0/76, gn_bwd_reduce 0/60, gn_finalize 0/32, gn_finalize_bound 0/10, gn_finalize_part 38/34,
        gn_partials 20/0, gn_stats 0/21, head_conv 1/0, head_dgrad 0/0, head_wgrad 0/0, nchw_to_nhwc 0/2, pack_split
        118/94, pack_wino 28/0, stem_wgrad 0/0, wgrad_reduce 0/54
  d96  absmax_images 0/21, attention_bwd 0/3, attention_bwd_f16x3 0/0, attention_fwd 2/0, attention_fwd_f16x3 1/0,
        attention_fwd_f16x3_lse 0/1, attention_fwd_lse 0/2, colsum 0/10, conv3x3_f16x3 4/4, conv3x3_wino_f16x3 4/4,
        conv3x3_wino_f16x3_gnb 0/8, conv_igemm_f16x3 7/10, conv_igemm_x6 13/42, conv_wgrad3_f16x3 0/3,
        conv_wgrad_f16x3 0/17, conv_wgrad_x6 0/8, gemm_small 0/14, gn_bwd_apply 0/20, gn_bwd_finalize 0/39,
        gn_bwd_reduce 0/31, gn_finalize 0/22, gn_finalize_bound 0/8, gn_finalize_part 20/10, gn_partials 14/0,
        gn_stats 0/15, pack_split 68/58, pack_wino 16/0, wgrad_reduce 0/28
  heads1  attention_bwd 0/0, attention_bwd_f16x3 0/10, attention_fwd 0/0, attention_fwd_f16x3 6/0,
        attention_fwd_f16x3_lse 0/10, attention_fwd_f16x3_presplit 4/0, attention_fwd_lse 0/0, conv_igemm_f16x3
        17/36, conv_igemm_f16x3_qkv 4/0
  heads2  attention_bwd 0/2, attention_bwd_f16x3 0/8, attention_fwd 2/0, attention_fwd_f16x3 6/0,
        attention_fwd_f16x3_lse 0/8, attention_fwd_f16x3_presplit 2/0, attention_fwd_lse 0/2, conv_igemm_f16x3
        19/36, conv_igemm_f16x3_qkv 2/0
  heads8  absmax_images 0/30, attention_bwd 0/4, attention_bwd_f16x3 0/2, attention_fwd 4/0, attention_fwd_f16x3
        2/0, attention_fwd_f16x3_lse 0/2, attention_fwd_lse 0/4, colsum 0/12, conv3x3_f16x3 2/2, conv3x3_wino_f16x3
        6/6, conv3x3_wino_f16x3_gnb 0/8, conv4x4s2_f16x3 1/1, conv_igemm_f16x3 12/20, conv_igemm_x6 17/49, conv_in
        0/1, conv_in_gn 1/0, conv_wgrad3_f16x3 0/8, conv_wgrad_f16x3 0/20, conv_wgrad_x6 0/12, convtr4x4s2_f16x3
        1/2, gemm_small 0/16, gn_bwd_apply 0/27, gn_bwd_finalize 0/54, gn_bwd_reduce 0/46, gn_finalize 0/30,
        gn_finalize_bound 0/10, gn_finalize_part 27/14, gn_partials 18/0, gn_stats 0/20, pack_split 90/78, pack_wino
        20/0, wgrad_reduce 0/40
  gray  bsum 0/1, conv_igemm_x6 21/70, conv_wgrad_x6 0/18, gn_bwd_finalize 0/85, gn_bwd_reduce 0/69, head_conv 1/0,
        head_dgrad 0/0, head_wgrad 0/0, nchw_to_nhwc 0/2, pack_split 128/116, stem_wgrad 0/0, wgrad_reduce 0/62
  rgba  bsum 0/1, conv_igemm_x6 21/70, conv_wgrad_x6 0/18, gn_bwd_finalize 0/85, gn_bwd_reduce 0/69, head_conv 1/0,
        head_dgrad 0/0, head_wgrad 0/0, nchw_to_nhwc 0/2, pack_split 128/116, stem_wgrad 0/0, wgrad_reduce 0/62
  c6  conv_igemm_f16x3 22/-, head_conv 0/-
  temb64  as tiny
  temb256  as tiny
  flat  attention_bwd 0/5, attention_bwd_f16x3 0/1, attention_fwd 5/0, attention_fwd_f16x3 0/0,
        attention_fwd_f16x3_lse 0/1, attention_fwd_f16x3_presplit_a3 1/0, attention_fwd_lse 0/5, conv3x3_f16x3
        12/12, conv3x3_wino_f16x3 20/20, conv3x3_wino_f16x3_gnb 0/32, conv_igemm_f16x3 10/40, conv_igemm_x6 0/0,
        conv_wgrad3_f16x3 0/23, conv_wgrad_f16x3 0/33, conv_wgrad_x6 0/0, convtr4x4s2_f16x3 0/0, gn_bwd_apply 0/39,
        gn_bwd_finalize 0/68, gn_bwd_reduce 0/36, gn_finalize 0/7, gn_finalize_bound 0/7, gn_finalize_part 39/64,
        gn_partials 1/0, gn_stats 0/7, pack_split 90/52, proj_f16x3 1/0, proj_f16x3_qkv 1/0, split_f16x3_tiled 1/0,
        wgrad_reduce 0/56
  deep  absmax_images 0/43, attention_bwd 0/3, attention_fwd 3/0, attention_fwd_lse 0/3, colsum 0/22,
        conv_igemm_f16x3 13/20, conv_igemm_x6 34/98, conv_wgrad3_f16x3 0/3, conv_wgrad_f16x3 0/33, conv_wgrad_x6
        0/24, gemm_small 0/26, gn_bwd_apply 0/47, gn_bwd_finalize 0/86, gn_bwd_reduce 0/70, gn_finalize 14/52,
        gn_finalize_bound 8/16, gn_finalize_part 25/26, gn_partials 12/0, gn_stats 22/34, pack_split 140/131,
        pack_wino 40/0
  ch48  rejected at construction in every precision: no native call
(names without their wc_ prefix; "-": the training step is rejected at construction)
"""
import dataclasses
import json
import os

import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_gpu_forms import _Case, _assert_same_finite, _check_train, _n, _recording

gpu = pytest.mark.gpu

TINY = json.load(open(os.path.join(GOLDEN, 'manifest.json')))['tiny']['config']
PRECISIONS = ('f16x3', 'bf16x6', 'fp32')
T, F = True, False


@dataclasses.dataclass(frozen=True)
class Shape:
    """One off-grid case: tiny + overrides, batch, input H x W, timesteps; the precisions check_supported
    admits (forward, training); the f16x3 census assertions; tiny_census: whether the case's arm is an entry
    point at all (False: the shape only changes loop bounds inside kernels tiny also launches)."""
    id: str
    overrides: dict
    B: int = 2
    hw: tuple = (32, 32)
    t: tuple = (5, 700)
    fwd: tuple = PRECISIONS
    train: tuple = PRECISIONS
    fwd_present: tuple = ()
    fwd_never: tuple = ()
    train_present: tuple = ()
    train_never: tuple = ()
    rejects: str = ''  # the field the rejection message names
    tiny_census: bool = True

    @property
    def config(self):
        return {**TINY, **self.overrides}


_SQ24 = dict(im_size=24, down_channels=[64, 128, 128], mid_channels=[128, 128], down_sample=[T, T],
             attn_resolutions=[12])
CASES = [
    # non-square input; W = 24 and W = 12 levels (Wm % 16 fails: no halo / Winograd kernel below 32 x 48, no
    # space-to-depth or one-launch transposed conv); an 8 x 12 level (HW % 64 fails: no tile partials, np_in == 0);
    # odd B; t at both ends of the schedule
    Shape('rect', {}, B=3, hw=(32, 48), t=(0, 499, 999),
          fwd_present=('wc_conv3x3_wino_*', 'wc_conv_igemm_x6', 'wc_gn_stats', 'wc_gn_finalize_part'),
          fwd_never=('wc_conv4x4s2_f16x3', 'wc_convtr4x4s2_f16x3'),
          train_present=('wc_conv3x3_wino_f16x3', 'wc_conv_igemm_x6'),
          train_never=('wc_conv4x4s2_f16x3', 'wc_convtr4x4s2_f16x3')),
    # no level has W % 16 == 0; attention at N = 144 and N = 36 (N < 64, N no multiple of 32)
    Shape('sq24', _SQ24, hw=(24, 24), fwd_present=('wc_conv_igemm_x6', 'wc_attention_fwd*'),
          fwd_never=('wc_conv3x3_*', 'wc_conv4x4s2_f16x3', 'wc_convtr4x4s2_f16x3', '*presplit*'),
          train_never=('wc_conv3x3_*', 'wc_conv_wgrad3*')),
    # B = 1; H != W with neither on the tile; attention at N = 240 and N = 60
    Shape('tall', {**_SQ24, 'im_size': 40, 'attn_resolutions': [20]}, B=1, hw=(40, 24), t=(611, ),
          fwd_present=('wc_conv_igemm_x6', 'wc_attention_fwd*'), fwd_never=('wc_conv3x3_*', '*presplit*'),
          train_never=('wc_conv3x3_*', 'wc_conv_wgrad3*')),
    # C a multiple of 16 but not of 32 (48, 144): the weight packs take it, but GroupNorm(8) then has 6- and
    # 18-channel groups and wc_gn_stats reads a group four channels at a time, so the envelope rejects it in
    # every precision (before this matrix it failed at the first GroupNorm, after conv_in had run)
    Shape('ch48', dict(down_channels=[48, 96, 144, 144], mid_channels=[144, 144], num_heads=6), fwd=(), train=(),
          rejects='down_channels'),
    # what ch48 was after, inside the envelope: C a multiple of 32 but of no GEMM N tile (96, 192: ragged N
    # tiles); conv_in with Cout != 64; the head conv over six 16-channel chunks; head_small and the stem wgrad
    # off by shape (C = 96); head dims 24 and 48 (fp32-MFMA attention forward and backward, padded to 32 / 64)
    Shape('ch96', dict(down_channels=[96, 96, 192, 192], mid_channels=[192, 192]),
          fwd_present=('wc_conv_in', 'wc_head_conv', 'wc_attention_fwd'),
          fwd_never=('wc_conv_in_gn', '*presplit*', 'wc_attention_fwd_f16x3*'),
          train_present=('wc_attention_bwd', 'wc_attention_fwd_lse', 'wc_nchw_to_nhwc'),
          train_never=('wc_attention_bwd6', 'wc_attention_bwd_f16x3', 'wc_head_wgrad', 'wc_stem_wgrad',
                       'wc_head_dgrad')),
    # head dim 96 (384 channels, 4 heads): the split-precision forward exists, no split backward does
    Shape('d96', dict(down_channels=[32, 64, 64, 384], mid_channels=[384, 64], attn_resolutions=[8], num_down_layers=1,
                      num_up_layers=1), fwd_present=('wc_attention_fwd_f16x3*', ),
          train_present=('wc_attention_fwd_f16x3_lse', 'wc_attention_bwd')),
    # head dims {32, 64, 128}: every attention on the split-precision kernels
    Shape('heads1', dict(num_heads=1), fwd_present=('wc_attention_fwd_f16x3*', ), fwd_never=('wc_attention_fwd', ),
          train_present=('wc_attention_bwd_f16x3', ), train_never=('wc_attention_bwd', 'wc_attention_fwd_lse')),
    # head dims {16, 32, 64}
    Shape('heads2', dict(num_heads=2), fwd_present=('wc_attention_fwd_f16x3*', 'wc_attention_fwd'),
          train_present=('wc_attention_bwd_f16x3', 'wc_attention_bwd')),
    # head dims 8, 16, 32
    Shape('heads8', dict(down_channels=[64, 128, 128, 256], mid_channels=[256, 256, 128], num_heads=8,
                         num_down_layers=1, num_up_layers=1),
          fwd_present=('wc_attention_fwd_f16x3*', 'wc_attention_fwd'),
          train_present=('wc_attention_bwd_f16x3', 'wc_attention_bwd')),
    # conv_in with Cin != 3; head_conv_kernel<4> for NO = 1 and 4; head_small and the stem wgrad off by shape
    Shape('gray', dict(im_channels=1), fwd_present=('wc_head_conv', 'wc_conv_in'), fwd_never=('wc_conv_in_gn', ),
          train_present=('wc_nchw_to_nhwc', ), train_never=('wc_head_wgrad', 'wc_stem_wgrad', 'wc_head_dgrad')),
    Shape('rgba', dict(im_channels=4), fwd_present=('wc_head_conv', 'wc_conv_in'), fwd_never=('wc_conv_in_gn', ),
          train_present=('wc_nchw_to_nhwc', ), train_never=('wc_head_wgrad', 'wc_stem_wgrad', 'wc_head_dgrad')),
    # NO > 4: conv_out on the implicit GEMM with out_nchw; training outside the envelope
    Shape('c6', dict(im_channels=6), train=(), rejects='im_channels', fwd_never=('wc_head_conv', 'wc_conv_in_gn')),
    # wc_temb at D != 128; in training gemm_small_wave_kernel (K >= 256) serves the D x D products
    # (test_gpu_train.test_gemm_small_vs_float64 asserts the kernel name): the same entry points as tiny
    Shape('temb64', dict(time_emb_dim=64), tiny_census=False),
    Shape('temb256', dict(time_emb_dim=256), tiny_census=False),
    # no resampling conv at all: the "written in place" up path, up_convs[k] is None everywhere; every level is
    # 16 x 16, so nothing is left for the bf16x6 implicit GEMM (tiny's resampling convs and 8 x 8 level)
    Shape('flat', dict(im_size=16, down_sample=[F, F, F], attn_resolutions=[8]), hw=(16, 16),
          fwd_never=('wc_conv4x4s2_f16x3', 'wc_convtr4x4s2_f16x3', 'wc_conv_igemm_x6'),
          train_never=('wc_conv4x4s2_f16x3', 'wc_convtr4x4s2_f16x3', 'wc_conv_igemm_x6', 'wc_conv_wgrad_x6')),
    # three resampling levels down to 4 x 4; attention in the mids only; uneven layer counts; one shared
    # timestep (temb_ld == 0) at B = 5
    Shape('deep', dict(down_sample=[T, T, T], attn_resolutions=[], num_down_layers=1, num_mid_layers=3,
                       num_up_layers=3), B=5, t=(321, ), fwd_present=('wc_gn_stats', 'wc_conv_igemm_x6')),
]
assert len(CASES) == 16 and len({c.id for c in CASES}) == 16


@pytest.fixture(scope='module', params=CASES, ids=lambda s: s.id)
def case(request):
    """(the Shape, its _Case with the float64 oracle): built once, alive while the case's tests run (pytest
    groups the tests of a module-scoped parametrised fixture by parameter)."""
    s = request.param
    return s, _Case(s.config, B=s.B, hw=s.hw, t=s.t)


@pytest.fixture(scope='module')
def tiny_census():
    """tiny on the grid (B = 2, 32 x 32, t = [5, 700]): the entry points of its f16x3 forward and training step."""
    c = _Case(TINY, oracle=False)
    _, fwd = c.forward(conv_precision='f16x3')
    _, _, train = c.train(check_gbound=True, conv_precision='f16x3')
    print('tiny forward census:', dict(sorted(fwd.counts.items())))
    print('tiny training census:', dict(sorted(train.counts.items())))
    return dict(fwd.counts), dict(train.counts)


def _assert_rejected(s: Shape, c: _Case, precision: str, training: bool):
    """Outside the envelope: the engine's constructor raises, naming the field, before any native call."""
    from weatherconverter_amd import forms
    assert s.rejects
    with forms.using(conv_precision=precision), _recording() as rec:
        net = c.net()
        net = net.train() if training else net.eval()
        with pytest.raises(RuntimeError, match=s.rejects):
            if training:
                net(c.x.cuda(), c.t.cuda())
            else:
                with torch.no_grad():
                    net(c.x.cuda(), c.t.cuda())
    assert sum(rec.counts.values()) == 0, dict(rec.counts)


@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_forward_vs_oracle(case, precision):
    s, c = case
    if precision not in s.fwd:
        return _assert_rejected(s, c, precision, training=False)
    y, rec = c.forward(conv_precision=precision)
    err = rel_l2(y, c.y_ref)
    print(f'{s.id} forward {precision}: rel-L2 vs float64 {err:.3e}')
    assert y.shape == c.y_ref.shape
    assert err < 1e-5


@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
def test_training_step_vs_oracle(case, precision):
    s, c = case
    if precision not in s.train:
        return _assert_rejected(s, c, precision, training=True)
    loss, grads, rec = c.train(check_gbound=True, conv_precision=precision)
    print(f'{s.id} training {precision}: loss {loss!r}, float64 {c.loss_ref!r}')
    assert set(grads) == set(c.g_ref)
    _check_train(c, loss, grads)


def _assert_census(tag, counts, present, never):
    for pat in present:
        assert _n(counts, pat) >= 1, f'{tag}: {pat} never launched'
    for pat in never:
        assert _n(counts, pat) == 0, f'{tag}: {pat} launched {_n(counts, pat)}x'


@gpu
def test_census(case, tiny_census):
    """The case reached the arm it exists for (and not the on-grid one), and its census is not tiny's."""
    s, c = case
    if 'f16x3' not in s.fwd:
        return _assert_rejected(s, c, 'f16x3', training=False)
    _, fwd = c.forward(conv_precision='f16x3')
    print(f'{s.id} forward census:', dict(sorted(fwd.counts.items())))
    _assert_census(f'{s.id} forward', fwd.counts, s.fwd_present, s.fwd_never)
    train = None
    if 'f16x3' in s.train:
        _, _, train = c.train(check_gbound=True, conv_precision='f16x3')
        print(f'{s.id} training census:', dict(sorted(train.counts.items())))
        _assert_census(f'{s.id} training', train.counts, s.train_present, s.train_never)
    same = dict(fwd.counts) == tiny_census[0] and (train is None or dict(train.counts) == tiny_census[1])
    if s.tiny_census:
        assert not same, f'{s.id}: the same entry points, the same number of times, as tiny on the grid'
    else:
        # the shape only changes loop bounds inside the kernels tiny launches: stated, so that a change that
        # gives the case an entry point of its own is noticed
        assert same, f'{s.id}: census differs from tiny\'s; give the case census assertions'


@gpu
def test_rows_equal_singletons(case):
    """Row b of the batched f16x3 forward equals image b run alone, bit for bit."""
    from weatherconverter_amd import forms
    s, c = case
    if 'f16x3' not in s.fwd:
        return _assert_rejected(s, c, 'f16x3', training=False)
    y, _ = c.forward(conv_precision='f16x3')
    with forms.using(conv_precision='f16x3'), torch.no_grad():
        net = c.net().eval()
        for b in range(s.B):
            tb = c.t if c.t.numel() == 1 else c.t[b:b + 1]
            yb = net(c.x[b:b + 1].cuda(), tb.cuda()).cpu()
            assert torch.equal(yb[0], y[b]), f'{s.id}: row {b} differs from the singleton: rel-L2 {rel_l2(yb[0], y[b]):.3e}'


@gpu
def test_poisoned_allocations(case):
    """f16x3 forward and training step with every fresh allocation poisoned: finite, bit-identical."""
    s, c = case
    if 'f16x3' not in s.fwd:
        return _assert_rejected(s, c, 'f16x3', training=False)
    y, _ = c.forward(conv_precision='f16x3')
    yp, _ = c.forward(poison=True, conv_precision='f16x3')
    _assert_same_finite(yp, y)
    if 'f16x3' not in s.train:
        return
    loss, grads, _ = c.train(check_gbound=True, conv_precision='f16x3')
    lossp, gradsp, _ = c.train(poison=True, check_gbound=True, conv_precision='f16x3')
    bad = [k for k in grads if not bool(torch.isfinite(gradsp[k]).all())]
    assert not bad, f'non-finite gradients (a kernel read memory nobody wrote): {bad[:8]}'
    diff = [k for k in grads if not torch.equal(gradsp[k], grads[k])]
    assert not diff, f'gradients differ from the unpoisoned run: {diff[:8]}'
    assert lossp == loss
