"""CPU: the small backward cases of tests/test_gpu_batch.py sit in the regimes the workloads select.

B is not a loop count in the training backward: through wc_conv_wgrad3_splits, wc_conv_wgrad_splits and
wc_gn_bwd_splits it selects how pixel splits lie against images, how many partial slabs wc_wgrad_reduce
adds (one level up to 32, groups of 32 above), and whether a GroupNorm-backward split is short or empty.
tests/golden/backward_launches.json records what one training iteration selects at config 3 (256 px,
B = 32), at 256 px with B = 5, and at the reference's own 128 px with B = 4
(tools/train_launch_shapes.py --json, the command in its docstring).  Here every recorded launch and every
case of the GPU table below is classified with the library's own split functions (host code) and the
constants they document, and

  * the split count recorded equals what the library returns today (a changed target_blocks or group
    size fails here and names the launch), and
  * every (kernel form, prologue kind, regime) class the workloads reach is reached by a GPU case.

Regimes (each dimension is its own label):
  wgrad3   rel:   'le1_aligned' a split is one image or an aligned part of one; 'whole_images' k >= 2 whole
                  images a split; 'inside_image' some split begins or ends inside an image
           last:  'full' / 'short' last split
  generic  pps:   'aligned' no split crosses an image boundary / 'spanning'
           last:  'full' / 'short' (whole K-steps) / 'partial_kstep' (P no multiple of the 32-pixel K-step)
  both     reduce: 'le32' one level / 'gt32_full' two levels, full last group / 'gt32_short'
  GN bwd   limit: which term of min(1024/B, HW/16, 256) holds ('batch', 'pixels', 'cap'; 'clamp' when 1024/B < 1)
           pps:   'divides' HW or 'ragged';  empty: '0' or 'ge1' splits without a pixel
  wino_gnb 'epilogue': the sums come from the conv epilogue (split count independent of B)
Prologue kind: 0 raw, 1 GroupNorm affine, 2 GroupNorm + SiLU (GN backward: 0 = plain sums, x == NULL).
"""
import json
import math
import os

import pytest

from conftest import GOLDEN
from weatherconverter_amd import _native

RG = 32            # wc_wgrad_reduce: "groups of 32 slabs" (include/wc_kernels.h)
KP = 32            # pixels per K-step of wc_conv_wgrad (WG_KP, csrc/wc_backward.hip); pps is a multiple of it
W3_TARGET = 512    # target_blocks kernels.conv_wgrad passes to wc_conv_wgrad3_splits
WG_TARGET = 2048   # ... and to wc_conv_wgrad_splits

# ---------------------------------------------------------------- the GPU cases (tests/test_gpu_batch.py)
# wgrad3: (M, C0, B, H, W) -> the relation named; each runs as f16x3 and bf16x6 with prologue kinds 1 and 2
WGRAD3_CASES = [
    ((128, 64, 8, 8, 16), 'whole_images'),    # 4 whole images per split
    ((128, 32, 5, 8, 32), 'inside_image'),    # 5 blocks per split against 2 per image: a split ends inside image 2
    ((64, 64, 9, 4, 16), 'inside_image'),     # 64-channel tiles, 5 against 2, short last split
    ((256, 64, 6, 8, 16), 'whole_images'),    # one split over all six images
    # the workloads' halo launches with more than 32 splits (one aligned part of an image per split):
    ((64, 64, 5, 8, 128), 'le1_aligned'),     # 40 splits: groups 32 + 8
    ((64, 64, 8, 16, 64), 'le1_aligned'),     # 64 splits: two full groups
]
WGRAD3_FORMS = ['f16x3', 'bf16x6']
WGRAD3_PROS = [1, 2]
# generic: form -> (M, C0, C1, taps, stride, prologue kind, B, H, W of the source); f16x3 form
GENERIC_CASES = {
    '1x1_raw': (128, 128, 0, 1, 1, 0, 5, 40, 48),       # 38 splits (32 + 6), 256 pixels a split against 1920 an image
    '3x3_gn_res': (128, 64, 32, 9, 1, 2, 5, 40, 44),    # 35 splits (32 + 3); W % 16 != 0: not the halo kernel
    '4x4s2_raw': (128, 64, 0, 16, 2, 0, 7, 24, 40),     # 7 splits spanning images
    # the workloads' GroupNorm-prologue 1x1 (the attention in_proj) and the classes the three above leave open
    '1x1_gn': (128, 128, 0, 1, 1, 1, 5, 40, 48),        # as 1x1_raw under a GroupNorm affine: 32 + 6, spanning, short
    '1x1_gn_aligned': (384, 128, 0, 1, 1, 1, 2, 16, 32),   # splits <= 32, aligned, full last split
    '1x1_gn_64': (128, 128, 0, 1, 1, 1, 4, 64, 64),     # 64 splits: two full groups
    '1x1_raw_64': (128, 128, 0, 1, 1, 0, 4, 64, 64),    # the same raw
}
# GN(+SiLU) backward: (B, H, W, channel counts); each with silu on and off, and the plain sums (kind 0)
GN_CASES = [
    ((17, 32, 32), (64, 96)),     # 60 splits of 18 pixels, 3 of them empty
    ((33, 32, 32), (64, 96)),     # 31 splits of 34, short last split
    ((5, 10, 10), (64, 96)),      # HW = 100: 6 splits of 17
    ((1025, 4, 4), (32, )),       # 1024 / B < 1: the clamp to one split
]
# wino conv with the GN-backward epilogue beside the reduce path in the B = 17 regime (60 splits of 18, 3 empty:
# HW > 960, so 32 x 32 is the smallest grid on the conv's 16-column tiles): (B, H, W, Cg, Co)
WINO_GNB_CASE = (17, 32, 32, 64, 64)


def lib():
    return _native.load()


# ---------------------------------------------------------------- classification
def reduce_regime(splits):
    return 'le32' if splits <= RG else ('gt32_full' if splits % RG == 0 else 'gt32_short')


def wgrad3_geometry(M, C0, B, H, W):
    """(splits, blocks per split, blocks per image, blocks) of wc_conv_wgrad3: TH x 16 pixel blocks, TH = 8
    with the 128-channel tiles (M % 128 == 0), else 2."""
    TH = 8 if M % 128 == 0 else 2
    bpi = (H // TH) * (W // 16)
    nblk = B * bpi
    splits = lib().wc_conv_wgrad3_splits(M, C0, B, H, W, W3_TARGET)
    bps = -(-nblk // splits)
    assert -(-nblk // bps) == splits
    return splits, bps, bpi, nblk


def wgrad3_regimes(M, C0, B, H, W):
    splits, bps, bpi, nblk = wgrad3_geometry(M, C0, B, H, W)
    if bps <= bpi and bpi % bps == 0:
        rel = 'le1_aligned'
    elif bps % bpi == 0:
        rel = 'whole_images'
    else:
        rel = 'inside_image'
    return {f'rel:{rel}', 'last:' + ('short' if nblk % bps else 'full'), 'reduce:' + reduce_regime(splits)}


def generic_geometry(M, Kc, B, Hm, Wm):
    """(splits, pixels per split, pixels) of wc_conv_wgrad: pps a multiple of the K-step."""
    P = B * Hm * Wm
    splits = lib().wc_conv_wgrad_splits(M, Kc, P, WG_TARGET)
    pps = -(-(-(-P // splits)) // KP) * KP
    assert -(-P // pps) == splits
    return splits, pps, P


def generic_regimes(M, Kc, B, Hm, Wm):
    splits, pps, P = generic_geometry(M, Kc, B, Hm, Wm)
    last = 'full' if P % pps == 0 else ('partial_kstep' if P % KP else 'short')
    return {'pps:' + ('aligned' if (Hm * Wm) % pps == 0 else 'spanning'), f'last:{last}',
            'reduce:' + reduce_regime(splits)}


def gn_geometry(B, HW):
    """(splits, pixels per split, splits without a pixel) of wc_gn_bwd_reduce."""
    splits = lib().wc_gn_bwd_splits(B, HW)
    pps = -(-HW // splits)
    return splits, pps, splits - (-(-HW // pps))


def gn_regimes(B, HW):
    splits, pps, empty = gn_geometry(B, HW)
    sp = 1024 // B
    if sp < 1:
        limit = 'clamp'
    elif sp > max(1, HW // 16):
        limit = 'pixels'
    else:
        limit = 'cap' if sp > 256 else 'batch'
    assert splits == {'clamp': 1, 'pixels': max(1, HW // 16), 'cap': 256, 'batch': sp}[limit]
    return {f'limit:{limit}', 'pps:' + ('divides' if HW % pps == 0 else 'ragged'), 'empty:' + ('ge1' if empty else '0')}


def generic_case_shape(form):
    """(M, Kc, B, Hm, Wm, prologue kind) of a GENERIC_CASES row."""
    M, C0, C1, taps, stride, pro, B, H, W = GENERIC_CASES[form]
    return M, taps * C0 + C1, B, H // stride, W // stride, pro


def case_classes():
    """{(kernel form, prologue kind, regime label)} over the GPU cases."""
    out = set()
    for shape, _ in WGRAD3_CASES:
        for form in WGRAD3_FORMS:
            for pro in WGRAD3_PROS:
                out |= {(f'wgrad3_{form}', pro, r) for r in wgrad3_regimes(*shape)}
    for form in GENERIC_CASES:
        M, Kc, B, Hm, Wm, pro = generic_case_shape(form)
        out |= {('wgrad_f16x3', pro, r) for r in generic_regimes(M, Kc, B, Hm, Wm)}
    for (B, H, W), _ in GN_CASES:
        for kind in (0, 1, 2):
            out |= {('gn_bwd_reduce', kind, r) for r in gn_regimes(B, H * W)}
    out.add(('wino_gnb', 0, 'epilogue'))
    return out


_ENTRY_FORM = {'wc_conv_wgrad3_f16x3': 'wgrad3_f16x3', 'wc_conv_wgrad3': 'wgrad3_bf16x6', 'wc_conv_wgrad_f16x3': 'wgrad_f16x3',
               'wc_conv_wgrad_x6': 'wgrad_bf16x6', 'wc_conv_wgrad': 'wgrad_fp32'}


def launch_classes(r):
    """(the split count the library gives this recorded launch today, its classes)."""
    if r['kind'] == 'wgrad':
        form, s0 = _ENTRY_FORM[r['entry']], r['segs'][0]
        if form.startswith('wgrad3'):
            assert len(r['segs']) == 1 and s0['taps'] == 9 and s0['stride'] == 1
            shape = (r['M'], s0['C'], r['B'], r['Hm'], r['Wm'])
            return wgrad3_geometry(*shape)[0], {(form, s0['pro'], x) for x in wgrad3_regimes(*shape)}
        Kc = sum(s['C'] * s['taps'] for s in r['segs'])
        shape = (r['M'], Kc, r['B'], r['Hm'], r['Wm'])
        return generic_geometry(*shape)[0], {(form, s0['pro'], x) for x in generic_regimes(*shape)}
    if r['kind'] == 'gn_bwd_reduce':
        kind = (2 if r['silu'] else 1) if r['has_x'] else 0
        return gn_geometry(r['B'], r['HW'])[0], {('gn_bwd_reduce', kind, x) for x in gn_regimes(r['B'], r['HW'])}
    assert r['kind'] == 'wino_gnb'
    side = math.isqrt(r['HW'])  # the recorded workloads are square
    assert side * side == r['HW']
    return lib().wc_conv3x3_wino_gnb_splits(r['C'], side, side), {('wino_gnb', 0, 'epilogue')}


def fixture():
    with open(os.path.join(GOLDEN, 'backward_launches.json')) as fh:
        return json.load(fh)


# ---------------------------------------------------------------- tests
def test_fixture_holds_the_three_workloads():
    fx = fixture()
    assert fx['precision'] == 'fp32-class' and list(fx['workloads']) == ['256px_B32', '256px_B5', '128px_B4']
    for name, launches in fx['workloads'].items():
        kinds = {r['kind'] for r in launches}
        assert kinds == {'wgrad', 'gn_bwd_reduce', 'wino_gnb'}, (name, kinds)
        assert len({json.dumps(r, sort_keys=True) for r in launches}) == len(launches)  # de-duplicated
        assert all(r['B'] == int(name.split('_B')[1]) for r in launches)
        # the fp32-class line runs the f16x3 forms, named by the library
        assert all(r['kernel'].startswith(('conv_wgrad3_kernel<', 'conv_wgrad_kernel<')) and r['kernel'].endswith('true>')
                   for r in launches if r['kind'] == 'wgrad'), name


@pytest.mark.parametrize('workload', ['256px_B32', '256px_B5', '128px_B4'])
def test_recorded_split_counts_are_what_the_library_returns(workload):
    for r in fixture()['workloads'][workload]:
        splits, classes = launch_classes(r)
        assert splits == r['splits'], f'{r}: the library now gives {splits} splits; classes {sorted(classes)} move'


def test_the_issue_figures_hold_for_config3():
    """The figures the gap was stated with, from the library: at B = 32 the 32x32 levels put 4 and 8 whole
    images into one halo split and reduce 86, 57 and 43 generic splits in two levels with a short last
    group; B = 17 at 32x32 gives 60 GroupNorm-backward splits of 18 pixels, the last 3 empty."""
    assert wgrad3_geometry(512, 512, 32, 32, 32)[:3] == (8, 32, 8) and wgrad3_geometry(768, 768, 32, 32, 32)[:3] == (4, 64, 8)
    assert wgrad3_geometry(512, 256, 32, 64, 64)[:3] == (16, 64, 32)
    got = sorted({r['splits'] for r in fixture()['workloads']['256px_B32']
                  if r['kind'] == 'wgrad' and r['entry'] == 'wc_conv_wgrad_f16x3' and r['Hm'] == 32 and r['splits'] > RG
                  and r['splits'] % RG})
    assert got == [43, 57, 86]  # 32 + 11, 32 + 25, 32 + 32 + 22
    assert gn_geometry(17, 1024) == (60, 18, 3)
    assert gn_geometry(1025, 16) == (1, 16, 0)


def test_gpu_cases_sit_in_the_regimes_they_name():
    for shape, rel in WGRAD3_CASES:
        assert f'rel:{rel}' in wgrad3_regimes(*shape), (shape, wgrad3_regimes(*shape))
    assert wgrad3_geometry(128, 64, 8, 8, 16)[:3] == (2, 4, 1)
    assert wgrad3_geometry(128, 32, 5, 8, 32)[:3] == (2, 5, 2)
    assert wgrad3_geometry(64, 64, 9, 4, 16) == (4, 5, 2, 18) and 'last:short' in wgrad3_regimes(64, 64, 9, 4, 16)
    assert wgrad3_geometry(256, 64, 6, 8, 16)[:3] == (1, 6, 1)
    M, Kc, B, Hm, Wm, _ = generic_case_shape('1x1_raw')
    assert generic_geometry(M, Kc, B, Hm, Wm) == (38, 256, 9600)
    assert generic_regimes(M, Kc, B, Hm, Wm) == {'pps:spanning', 'last:short', 'reduce:gt32_short'}
    M, Kc, B, Hm, Wm, _ = generic_case_shape('3x3_gn_res')
    assert generic_geometry(M, Kc, B, Hm, Wm)[0] == 35 and 'reduce:gt32_short' in generic_regimes(M, Kc, B, Hm, Wm)
    M, Kc, B, Hm, Wm, _ = generic_case_shape('4x4s2_raw')
    assert generic_geometry(M, Kc, B, Hm, Wm)[0] == 7 and 'pps:spanning' in generic_regimes(M, Kc, B, Hm, Wm)
    assert gn_geometry(17, 1024) == (60, 18, 3) and gn_geometry(33, 1024) == (31, 34, 0) and gn_geometry(5, 100) == (6, 17, 0)
    assert gn_regimes(1025, 16) == {'limit:clamp', 'pps:divides', 'empty:0'}


def test_every_workload_class_has_a_gpu_case():
    have = case_classes()
    missing = {}
    for name, launches in fixture()['workloads'].items():
        for r in launches:
            for c in launch_classes(r)[1] - have:
                missing.setdefault(c, f'{name}: {r}')
    assert not missing, '\n'.join(f'{c} has no GPU case; first reached by {r}' for c, r in sorted(missing.items()))
