"""CPU: the dispatch predicates of kernels.py state the library's host rules completely.

A predicate that says yes where the library says no makes the engine raise at launch instead of taking its
fallback arm, so every predicate must carry the whole source-segment rule (check_src_seg of
csrc/wc_conv_host.hpp, kernels._src_view_ok): whole channel chunks, pixel stride and base on the 16-byte
grid, the view inside the 2 GiB buffer range.  The predicates read only Views (here of CPU tensors) and the
library's tile queries.
"""
import os

import pytest
import torch

from weatherconverter_amd import _build

pytestmark = pytest.mark.skipif(not os.path.exists(_build.LIB_PATH), reason='library not built')

TAPS3 = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def _x6(K, v, N, H, W, stride):
    return K.x6_eligible([K.Seg(v, TAPS3, stride=stride)], N, H, W)


def _wino(K, v, N, H, W, stride):
    return K.wino_eligible([K.Seg(v, TAPS3, stride=stride)], N, H, W)


def _s2d(K, v, N, H, W, stride):
    return K.conv4x4s2_f16x3_ok(K.Seg(v, [(ky - 1, kx - 1) for ky in range(4) for kx in range(4)], stride=stride), N, H, W)


def _convT(K, v, N, H, W, stride):
    return K.convT4x4s2_f16x3_ok(K.Seg(v, [(0, 0)], stride=stride), N)


def _vsplit(K, v, N, H, W, stride):
    one = torch.ones((1, v.C))
    return K.wino_vsplit_wanted([K.Seg(v, TAPS3, stride=stride, scale=one, shift=one, silu=True)], N, H, W)


def _proj(K, v, N, H, W, stride):
    return K.proj_pa_ok(v, N)


def _wgrad3(K, v, N, H, W, stride):
    return K.wgrad3_ok(K.View.full(torch.zeros((1, H, W, N))), K.Seg(v, TAPS3, stride=stride))


# predicate -> (adapter, source extent per main-grid pixel, the stride it takes, N that reaches its kernel)
PREDICATES = {
    'x6_eligible': (_x6, 1, 1, 128),
    'wino_eligible': (_wino, 1, 1, 128),
    'conv4x4s2_f16x3_ok': (_s2d, 2, 2, 128),
    'convT4x4s2_f16x3_ok': (_convT, 1, 1, 128),
    'wino_vsplit_wanted': (_vsplit, 1, 1, 512),  # four 128-channel tiles: the default threshold (policy)
    'proj_pa_ok': (_proj, 1, 1, 128),
    'wgrad3_ok': (_wgrad3, 1, 1, 128),
}

# case -> (channels of the tensor, c0 of the view, main grid H, W, wrong stride?); the view has 32 channels
CASES = {
    'full': (32, 0, 16, 16, False),
    'slice_c0_4_of_36': (36, 4, 16, 16, False),  # aligned base, ldc % 4 == 0
    'slice_c0_2_of_34': (34, 2, 16, 16, False),  # ldc % 4 != 0 and the base off by 8 bytes
    'slice_c0_2_of_36': (36, 2, 16, 16, False),  # the base off by 8 bytes
    'H_12': (32, 0, 12, 16, False),
    'W_24': (32, 0, 16, 24, False),
    'wrong_stride': (32, 0, 16, 16, True),
}

ALL_NO = dict.fromkeys(PREDICATES, False)
EXPECTED = {
    'full': dict.fromkeys(PREDICATES, True),
    'slice_c0_4_of_36': dict.fromkeys(PREDICATES, True),
    'slice_c0_2_of_34': ALL_NO,
    'slice_c0_2_of_36': ALL_NO,
    # 12 rows are no whole 8-row tiles; the pre-split pass has no row rule of its own (wino_eligible is asked
    # first); 12 x 16 pixels are no whole 128-pixel projection tiles
    'H_12': {**ALL_NO, 'wino_vsplit_wanted': True},
    # 24 columns are no whole 16-column tiles; 16 x 24 pixels are three whole projection tiles
    'W_24': {**ALL_NO, 'proj_pa_ok': True},
    # a segment read at the other stride (the pre-split pass again leaves that to wino_eligible; a projection
    # has no segment)
    'wrong_stride': {**ALL_NO, 'wino_vsplit_wanted': True, 'proj_pa_ok': None},
}


def _view(K, name, ctot, c0, H, W):
    src = PREDICATES[name][1]
    return K.View(torch.zeros((1, src * H, src * W, ctot)), c0, 32)


@pytest.mark.parametrize('case', list(CASES))
@pytest.mark.parametrize('name', list(PREDICATES))
def test_predicate_answers(name, case):
    from weatherconverter_amd import kernels as K
    want = EXPECTED[case][name]
    if want is None:
        return
    fn, _, stride, N = PREDICATES[name]
    ctot, c0, H, W, wrong = CASES[case]
    assert fn(K, _view(K, name, ctot, c0, H, W), N, H, W, (3 - stride) if wrong else stride) is want


def _wide_view(K, name, ldc):
    """A 32-channel view of a (1, 16, 16, ldc)-shaped main grid without its memory (every stride 0)."""
    src = PREDICATES[name][1]
    return K.View(torch.zeros(64).as_strided((1, src * 16, src * 16, ldc), (0, 0, 0, 0)), 0, 32)


@pytest.mark.parametrize('name', list(PREDICATES))
def test_predicate_refuses_a_view_past_the_buffer_range(name):
    """B*H*W*ldc*4 at 2^31 is refused, four channels under it accepted."""
    from weatherconverter_amd import kernels as K
    fn, src, stride, N = PREDICATES[name]
    ldc = 2**31 // (4 * src * 16 * src * 16)
    assert fn(K, _wide_view(K, name, ldc), N, 16, 16, stride) is False
    assert fn(K, _wide_view(K, name, ldc - 4), N, 16, 16, stride) is True


# The case of each predicate that is refused ONLY by a term the predicate did not state before it used
# _src_view_ok: the base alignment (x6_eligible had the range already) or the buffer range (the others had
# the alignment already, or neither).
NEW_TERM = {
    'x6_eligible': 'base',
    'wino_eligible': 'base',
    'conv4x4s2_f16x3_ok': 'base',
    'convT4x4s2_f16x3_ok': 'base',
    'wino_vsplit_wanted': 'range',
    'proj_pa_ok': 'range',
    'wgrad3_ok': 'range',
}


@pytest.mark.parametrize('name', list(PREDICATES))
def test_new_term_is_wired_in(name, monkeypatch):
    """With the source-view rule cut back to the channel multiple alone the refused view is accepted: the
    refusal comes from _src_view_ok's other terms and from nothing else in the predicate."""
    from weatherconverter_amd import kernels as K
    fn, src, stride, N = PREDICATES[name]
    if NEW_TERM[name] == 'base':
        v = _view(K, name, 36, 2, 16, 16)
    else:
        v = _wide_view(K, name, 2**31 // (4 * src * 16 * src * 16))
    assert fn(K, v, N, 16, 16, stride) is False
    monkeypatch.setattr(K, '_src_view_ok', lambda view, cmult: view.C % cmult == 0)
    assert fn(K, v, N, 16, 16, stride) is True


def test_dgrad3_ok_is_the_halo_predicate():
    """TrainEngine._dgrad3_ok adds nothing to x6_eligible: the alignment terms it carried are implied."""
    from weatherconverter_amd import kernels as K
    from weatherconverter_amd.diffusion_model.models.train_engine import TrainEngine
    for ctot, c0, want in ((32, 0, True), (36, 4, True), (36, 2, False), (34, 2, False)):
        g = K.View(torch.zeros((1, 16, 16, ctot)), c0, 32)
        assert TrainEngine._dgrad3_ok(g, 128) is want
