"""GPU: every kernel-form switch (weatherconverter_amd.forms.Forms) at its non-default setting, and no
read of memory nobody wrote.

The switches pick the kernel form, arithmetic and graph split of a run; most are read once, when
UnetEngine / TrainEngine packs its weights.  A row of the matrices below runs one switch at its other
setting on a fresh model and asserts
  * the effect: which native entry points ran, counted by a recorder around _native.call (every
    native launch goes through it), against the baseline run's counts -- an ignored switch fails here;
  * the result against the float64 oracle (oracle.unet_oracle.unet_forward and its autograd) at the
    project's tolerances: forward rel-L2 < 1e-5; training loss within 1e-5 relative,
    gradients rel-L2 < 1e-5 overall and < 1e-4 per tensor (test_gpu_train._check);
  * bit-identity with the baseline where the two forms are documented as bit-identical.
test_every_switch_has_a_row (CPU) fails when a field of Forms has no row.

The model (S1) is the smallest on which every switch selects something: 64 px, channels 64 / 128 / 256 /
256, so the down convs (128 -> 128 at 64 -> 32, 256 -> 256 at 32 -> 16) are in the space-to-depth kernel's
range, the transposed convs are 128 -> 128 and 64 -> 64, attention runs at 256 channels on 16 x 16 (head
dim 64, 256 pixels: the pre-split / LDS-DMA projection range), the N = 256 convs on 16 x 16 are two
128-channel Winograd tiles (pre-split and 8-wave forms at wino_vp_min_tiles = 2), and the 3 -> 64 stem and
64 -> 3 head are the small-conv kernels' shapes.  B = 2, t = [5, 700].

The poisoned-allocation tests run the same forwards and training steps with every fresh CUDA tensor of
torch.empty / empty_like / new_empty filled with 0xFF bytes (NaN as fp32 / fp16 / bf16, -1 as an integer)
and require finite results bit-identical to the unpoisoned run: a kernel whose result depends on a slot
nobody wrote fails deterministically instead of by the allocator's luck.
"""
import collections
import contextlib
import copy
import dataclasses
import fnmatch
import json
import os
import types

import pytest
import torch

from conftest import GOLDEN, rel_l2
from test_gpu_train import _check

gpu = pytest.mark.gpu

S1_CONFIG = dict(name='ddpm', im_channels=3, im_size=64, down_channels=[64, 128, 256, 256],
                 mid_channels=[256, 256, 256], down_sample=[True, True, False], time_emb_dim=128, num_down_layers=1,
                 num_mid_layers=1, num_up_layers=1, num_heads=4, attn_resolutions=[16])

# The baselines the rows are compared with: the forward at wino_vp_min_tiles = 2 (S1's widest convs have
# two 128-channel tiles; the default threshold 4 would leave the pre-split forms unselected), training
# under check_gbound as the existing gradient tests run it.
FWD_BASE = dict(wino_vp_min_tiles=2)
TRAIN_BASE = dict(check_gbound=True)


@dataclasses.dataclass(frozen=True)
class Row:
    """One switch at its non-default setting.  Entry-point patterns are fnmatch globs over the recorded
    names (no '*': the exact name).
    absent: zero launches in this run AND at least one in the baseline (the switch removed them);
    never: zero launches in this run; present: at least one; more / fewer: strictly more / fewer than the
    baseline; delta: {pattern: this run's count minus the baseline's}; base: {pattern: the baseline's count};
    bit: the result is documented bit-identical to the baseline's."""
    field: str
    switches: dict
    absent: tuple = ()
    never: tuple = ()
    present: tuple = ()
    more: tuple = ()
    fewer: tuple = ()
    delta: dict = dataclasses.field(default_factory=dict)
    base: dict = dataclasses.field(default_factory=dict)
    bit: bool = False

    @property
    def id(self):
        return ','.join(f'{k}={v}' for k, v in self.switches.items())


# The counts each row was seen to change on S1 at B = 2 (baseline -> row), for the reader; the assertions are
# the Row fields.
#   wino=False                wc_conv3x3_wino_f16x3 6 -> 0, _vp 12 -> 0, wc_wino_vsplit_f16x3 12 -> 0, wc_pack_wino 20 -> 0,
#                             wc_conv3x3_f16x3 2 -> 20
#   wino_vp_min_tiles=0       wc_wino_vsplit_f16x3 12 -> 0, wc_conv3x3_wino_f16x3_vp 12 -> 0, wc_conv3x3_wino_f16x3 6 -> 18
#   wino_vp8 (inside wide)    on: wc_conv3x3_wino_f16x3_vp 12 -> 0, _vp8 0 -> 12; off: nothing changes
#   proj_pa=False             wc_proj_f16x3 4 -> 0, wc_proj_f16x3_qkv 4 -> 0, wc_split_f16x3_tiled 4 -> 0,
#                             wc_conv_igemm_f16x3_qkv 0 -> 4, wc_attention_fwd_f16x3_presplit_a3 4 -> 0, _presplit 0 -> 4
#   attn_presplit=False       wc_attention_fwd_f16x3_presplit_a3 4 -> 0, wc_proj_f16x3* 8 -> 0, wc_attention_fwd_f16x3 0 -> 4
#   gn_partials=False         wc_gn_finalize_part 25 -> 0, wc_conv_in_gn 1 -> 0, wc_gn_stats 0 -> 25
#   down_s2d=False            wc_conv4x4s2_f16x3 2 -> 0 (wc_conv_igemm_f16x3 0 -> 2)
#   up_ct=False               wc_convtr4x4s2_f16x3 2 -> 0 (wc_conv_igemm_f16x3 0 -> 8)
#   pack_device=False         wc_pack_split 82 -> 0, wc_pack_wino 20 -> 0
#   pack_device_convt=False   wc_pack_split 82 -> 80
#   conv_precision=bf16x6     every *f16x3* 0, wc_conv3x3_x6 0 -> 20, wc_conv_igemm_x6 0 -> 18, wc_attention_fwd_x6 0 -> 4
#   conv_precision=fp32       every *f16x3* and *_x6* 0, wc_conv_igemm 0 -> 38, wc_attention_fwd 0 -> 4
#   graph_split 1 / 2 / 4     (vp8, vp) launches of the three forwards of a capture: (0, 36) / (72, 0) / (144, 0)
FORWARD_ROWS = [
    Row('wino', dict(wino=False), absent=('wc_conv3x3_wino_*', 'wc_wino_vsplit_*', 'wc_pack_wino*'),
        more=('wc_conv3x3_f16x3', )),
    # include/wc_kernels.h, wc_conv3x3_wino_f16x3_vp: "bit-identical results"
    Row('wino_vp_min_tiles', dict(wino_vp_min_tiles=0), absent=('wc_wino_vsplit_f16x3', 'wc_conv3x3_wino_f16x3_vp'),
        bit=True),
    Row('proj_pa', dict(proj_pa=False), absent=('wc_proj_f16x3*', 'wc_split_f16x3_tiled'),
        present=('wc_conv_igemm_f16x3_qkv', ), bit=True),
    # engine.py: "the bit-identical reference path"
    Row('attn_presplit', dict(attn_presplit=False), absent=('wc_attention_fwd_f16x3_presplit*', '*_qkv'),
        present=('wc_attention_fwd_f16x3', ), bit=True),
    Row('gn_partials', dict(gn_partials=False), absent=('wc_gn_finalize_part', 'wc_conv_in_gn'), more=('wc_gn_stats', )),
    Row('down_s2d', dict(down_s2d=False), absent=('wc_conv4x4s2_f16x3', ), base={'wc_conv4x4s2_f16x3': 2}),
    Row('up_ct', dict(up_ct=False), absent=('wc_convtr4x4s2_f16x3', ), base={'wc_convtr4x4s2_f16x3': 2}),
    # kernels._pack_dev / pack_wino: the device packs are bit for bit the torch-op definitions
    Row('pack_device', dict(pack_device=False), absent=('wc_pack_split', 'wc_pack_wino'), bit=True),
    # kernels.pack_f16x3_convT: on, each of the two transposed convs is ONE wc_pack_split of its four parities;
    # off, the four parities go through the torch-op definition under their common scale (no launch)
    Row('pack_device_convt', dict(pack_device_convt=False), delta={'wc_pack_split': -2},
        present=('wc_convtr4x4s2_f16x3', ), bit=True),
    Row('conv_precision', dict(conv_precision='bf16x6'), absent=('*f16x3*', ), present=('wc_conv3x3_x6', )),
    Row('conv_precision', dict(conv_precision='fp32'), absent=('*f16x3*', ), never=('*_x6*', ),
        present=('wc_conv_igemm', 'wc_attention_fwd')),
]

#   train_gnb_epilogue=False  wc_conv3x3_wino_f16x3_gnb 20 -> 0, wc_gn_bwd_reduce 28 -> 48
#   train_smallconv=False     wc_head_dgrad / wc_head_wgrad / wc_stem_wgrad 1 -> 0 (wc_conv_wgrad_x6 0 -> 2)
#   wgrad3=False              wc_conv_wgrad3_f16x3 20 -> 0 (wc_conv_wgrad_f16x3 22 -> 32)
#   wgrad3_f16x3=False        wc_conv_wgrad3_f16x3 20 -> 0, wc_conv_wgrad3 0 -> 20
#   wgrad_f16x3=False         wc_conv_wgrad_f16x3 22 -> 0, wc_conv_wgrad_x6 0 -> 22
#   attn_bwd_f16x3=False      wc_attention_bwd_f16x3 4 -> 0, wc_attention_bwd6 0 -> 4
#   attn_bwd6=False           wc_attention_bwd_f16x3 4 -> 0, wc_attention_bwd 0 -> 4
#   pack_raw=False            wc_pack_wino_batch 1 -> 0, wc_pack_wino 0 -> 38
#   pack_batch=False          wc_pack_wino_batch 1 -> 0, wc_pack_wino_raw 0 -> 38
#   train_gn_partials=False   wc_gn_stats 7 -> 25 (wc_gn_finalize_part 36 -> 0)
#   train_dh_sums=False       wc_gn_bwd_reduce 28 -> 38
#   check_gbound=False        wc_absmax_images 36 -> 0
#   dgrad_f16x3=False         wc_conv3x3_wino_f16x3_gnb 20 -> 0, wc_conv_wgrad3_f16x3 20 -> 0, wc_conv_wgrad_f16x3 22 -> 0,
#                             wc_attention_bwd_f16x3 4 -> 0, wc_conv_igemm_x6 1 -> 48
#   train_lazy_grad=False     _grad_w overwrite results 12 of 15 -> 0 of 15
TRAIN_ROWS = [
    Row('train_gnb_epilogue', dict(train_gnb_epilogue=False), absent=('wc_conv3x3_wino_f16x3_gnb', ),
        more=('wc_gn_bwd_reduce', )),
    Row('train_smallconv', dict(train_smallconv=False), absent=('wc_head_dgrad', 'wc_head_wgrad', 'wc_stem_wgrad')),
    Row('wgrad3', dict(wgrad3=False), absent=('wc_conv_wgrad3*', )),
    Row('wgrad3_f16x3', dict(wgrad3_f16x3=False), absent=('wc_conv_wgrad3_f16x3', ), present=('wc_conv_wgrad3', )),
    Row('wgrad_f16x3', dict(wgrad_f16x3=False), absent=('wc_conv_wgrad_f16x3', ), more=('wc_conv_wgrad_x6', )),
    Row('attn_bwd_f16x3', dict(attn_bwd_f16x3=False), absent=('wc_attention_bwd_f16x3', ),
        present=('wc_attention_bwd6', )),
    Row('attn_bwd6', dict(attn_bwd6=False), absent=('wc_attention_bwd_f16x3', ), never=('wc_attention_bwd6', ),
        present=('wc_attention_bwd', )),
    # kernels.pack_wino_raw / pack_wino_raw_batch: bit-identical to pack_wino of the host re-layouts
    Row('pack_raw', dict(pack_raw=False), absent=('wc_pack_wino_batch', ), never=('wc_pack_wino_raw', ),
        present=('wc_pack_wino', ), bit=True),
    Row('pack_batch', dict(pack_batch=False), absent=('wc_pack_wino_batch', ), present=('wc_pack_wino_raw', ), bit=True),
    Row('train_gn_partials', dict(train_gn_partials=False), more=('wc_gn_stats', )),
    Row('train_dh_sums', dict(train_dh_sums=False), more=('wc_gn_bwd_reduce', )),
    Row('check_gbound', dict(check_gbound=False), fewer=('wc_absmax_images', )),
    # TrainEngine.f3d: off, no f16x3 data-gradient pack exists and no gradient bound is tracked, so the data
    # gradients run the bf16x6 implicit GEMM and every f16x3 backward kernel (which needs those bounds) is gone;
    # the forward stays f16x3
    Row('dgrad_f16x3', dict(dgrad_f16x3=False),
        absent=('wc_conv3x3_wino_f16x3_gnb', 'wc_conv_wgrad3_f16x3', 'wc_conv_wgrad_f16x3', 'wc_attention_bwd_f16x3'),
        more=('wc_conv_igemm_x6', ), present=('wc_conv3x3_wino_f16x3', 'wc_conv_wgrad3', 'wc_attention_bwd6')),
    # no entry point changes: the row also asserts TrainEngine._grad_w's overwrite results (test_training_row)
    Row('train_lazy_grad', dict(train_lazy_grad=False)),
]

# switches whose row is a test of its own
OTHER_ROWS = {
    'wino_vp8': 'test_forward_wino_vp8_inside_wino_vp_wide',
    'graph_split': 'test_graph_split_from_forms',
    'attn_bwd192_fp32': 'test_attn_bwd192_fp32_kernel_level',
}


def test_every_switch_has_a_row():
    """A switch added to Forms without a row in the matrices above fails here."""
    from weatherconverter_amd.forms import Forms
    fields = {f.name for f in dataclasses.fields(Forms)}
    covered = set()
    for rows, base in ((FORWARD_ROWS, Forms(**FWD_BASE)), (TRAIN_ROWS, Forms(**TRAIN_BASE))):
        for row in rows:
            assert set(row.switches) == {row.field}, row  # a row toggles exactly the switch it is filed under
            assert row.switches[row.field] != getattr(base, row.field), row  # ... away from its baseline's setting
            covered.add(row.field)
    for field, test in OTHER_ROWS.items():
        assert callable(globals().get(test)), test
        covered.add(field)
    assert covered == fields, (sorted(fields - covered), sorted(covered - fields))
    # the baselines only move thresholds / checks, never a form another row relies on being default
    assert set(FWD_BASE) == {'wino_vp_min_tiles'} and set(TRAIN_BASE) == {'check_gbound'}


# ------------------------------------------------------------------ helpers
def _n(counts, pat: str) -> int:
    return sum(c for name, c in counts.items() if fnmatch.fnmatchcase(name, pat))


def _show(tag, row_counts, base_counts):
    """The counts that differ from the baseline's (printed before any assertion: `pytest -s` shows them)."""
    names = sorted(set(row_counts) | set(base_counts))
    diff = {n: (base_counts.get(n, 0), row_counts.get(n, 0)) for n in names if base_counts.get(n, 0) != row_counts.get(n, 0)}
    print(f'{tag}: (baseline, row) counts that differ: {diff}')


def _assert_effect(row: Row, counts, base):
    for pat in row.absent:
        assert _n(base, pat) >= 1, f'{row.id}: the baseline never launched {pat} (vacuous row)'
        assert _n(counts, pat) == 0, f'{row.id}: {pat} still launched {_n(counts, pat)}x'
    for pat in row.never:
        assert _n(counts, pat) == 0, f'{row.id}: {pat} launched {_n(counts, pat)}x'
    for pat in row.present:
        assert _n(counts, pat) >= 1, f'{row.id}: {pat} never launched'
    for pat in row.more:
        assert _n(counts, pat) > _n(base, pat), f'{row.id}: {pat} {_n(counts, pat)} vs baseline {_n(base, pat)}'
    for pat in row.fewer:
        assert _n(counts, pat) < _n(base, pat), f'{row.id}: {pat} {_n(counts, pat)} vs baseline {_n(base, pat)}'
    for pat, d in row.delta.items():
        assert _n(counts, pat) - _n(base, pat) == d, f'{row.id}: {pat} {_n(counts, pat)} vs baseline {_n(base, pat)}'
    for pat, c in row.base.items():
        assert _n(base, pat) == c, f'{row.id}: baseline {pat} {_n(base, pat)}, expected {c}'


@contextlib.contextmanager
def _recording():
    """Count every native entry point called inside the block (all launches go through _native.call); also
    the overwrite results of TrainEngine._grad_w (the lazy-gradient scheme)."""
    from weatherconverter_amd import _native
    from weatherconverter_amd.diffusion_model.models.train_engine import TrainEngine
    rec = types.SimpleNamespace(counts=collections.Counter(), overwrites=[])
    real_call, real_grad_w = _native.call, TrainEngine._grad_w

    def call(name, *args):
        rec.counts[name] += 1
        return real_call(name, *args)

    def grad_w(self, v):
        gv, overwrite = real_grad_w(self, v)
        rec.overwrites.append(overwrite)
        return gv, overwrite

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, 'call', call)
        mp.setattr(TrainEngine, '_grad_w', grad_w)
        yield rec


@contextlib.contextmanager
def _poisoned_allocations():
    """Every non-empty CUDA tensor torch.empty / torch.empty_like / Tensor.new_empty returns inside the block
    starts as 0xFF bytes (outside stream capture, where a fill would be recorded into the graph)."""
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    filled = [0]

    def poison(t):
        if isinstance(t, torch.Tensor) and t.is_cuda and t.numel() > 0 and not torch.cuda.is_current_stream_capturing():
            # a fresh tensor owns its storage: fill all of it, whatever the tensor's strides
            torch.tensor([], dtype=torch.uint8, device=t.device).set_(t.untyped_storage()).fill_(0xFF)
            filled[0] += 1
        return t

    def empty(*a, **k):
        return poison(real[0](*a, **k))

    def empty_like(*a, **k):
        return poison(real[1](*a, **k))

    def new_empty(self, *a, **k):
        return poison(real[2](self, *a, **k))

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, 'empty', empty)
        mp.setattr(torch, 'empty_like', empty_like)
        mp.setattr(torch.Tensor, 'new_empty', new_empty)
        yield filled


class _Case:
    """A model config with its CPU weights, inputs and (when asked for) float64 oracle results; runs are
    memoised by their switches, so a baseline is computed once per module."""

    def __init__(self, config: dict, B: int = 2, oracle: bool = True, hw=None, t=(5, 700)):
        """hw: the input's (H, W) when it is not im_size x im_size; t: the timesteps (one per image, or one
        shared by the batch)."""
        from oracle.unet_oracle import unet_forward
        from weatherconverter_amd.diffusion_model.config import ModelConfig
        from weatherconverter_amd.diffusion_model.models.unet_base import Unet
        from weatherconverter_amd.synthetic import init_synthetic_
        self.mc = mc = ModelConfig(**config)
        self.template = Unet(mc)  # stays on the CPU; every run deep-copies it: fresh engines, conv_precision None
        init_synthetic_(self.template, seed=0)
        g = torch.Generator().manual_seed(1234)
        H, W = hw if hw is not None else (mc.im_size, mc.im_size)
        shape = (B, mc.im_channels, H, W)
        self.x = torch.randn(shape, generator=g)
        self.noise = torch.randn(shape, generator=g)
        self.t = torch.tensor(list(t))
        self._runs = {}
        if oracle:
            sd = {k: v.detach().clone().double().requires_grad_(True) for k, v in self.template.state_dict().items()}
            y = unet_forward(sd, mc, self.x.double(), self.t)
            loss = torch.nn.MSELoss()(y, self.noise.double())
            loss.backward()
            self.y_ref, self.loss_ref = y.detach(), float(loss.detach())
            self.g_ref = {k: sd[k].grad for k, _ in self.template.named_parameters()}

    def net(self):
        return copy.deepcopy(self.template).cuda()

    def forward(self, poison=False, wide=False, **switches):
        """(output on the CPU, recorder) of one eval forward on a fresh model inside forms.using(switches)."""
        from weatherconverter_amd import forms
        key = ('fwd', poison, wide, tuple(sorted(switches.items())))
        if key not in self._runs:
            ctx = _poisoned_allocations() if poison else contextlib.nullcontext([1])
            with forms.using(**switches), _recording() as rec, ctx as filled, torch.no_grad():
                net = self.net().eval()
                with forms.wino_vp_wide(wide):
                    y = net(self.x.cuda(), self.t.cuda())
                torch.cuda.synchronize()
            assert filled[0] > 0
            self._runs[key] = (y.cpu(), rec)
        return self._runs[key]

    def train(self, poison=False, **switches):
        """(loss, {name: gradient on the CPU}, recorder) of one forward + MSELoss + backward in train mode."""
        from weatherconverter_amd import forms
        key = ('train', poison, tuple(sorted(switches.items())))
        if key not in self._runs:
            ctx = _poisoned_allocations() if poison else contextlib.nullcontext([1])
            with forms.using(**switches), _recording() as rec, ctx as filled:
                net = self.net().train()
                loss = torch.nn.MSELoss()(net(self.x.cuda(), self.t.cuda()), self.noise.cuda())
                loss.backward()
                torch.cuda.synchronize()
                grads = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
            assert filled[0] > 0
            self._runs[key] = (float(loss.detach()), grads, rec)
        return self._runs[key]


@pytest.fixture(scope='module')
def s1():
    return _Case(S1_CONFIG)


@pytest.fixture(scope='module')
def tiny():
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    return _Case(man['tiny']['config'], oracle=False)


# ------------------------------------------------------------------ forward matrix
@gpu
def test_forward_baseline_vs_oracle(s1):
    y, rec = s1.forward(**FWD_BASE)
    print('forward baseline counts:', dict(sorted(rec.counts.items())))
    err = rel_l2(y, s1.y_ref)
    print(f'forward baseline rel-L2 {err:.3e}')
    assert err < 1e-5


@gpu
@pytest.mark.parametrize('row', FORWARD_ROWS, ids=lambda r: r.id)
def test_forward_row(s1, row):
    base_y, base = s1.forward(**FWD_BASE)
    y, rec = s1.forward(**{**FWD_BASE, **row.switches})
    _show(row.id, rec.counts, base.counts)
    err = rel_l2(y, s1.y_ref)
    print(f'{row.id}: rel-L2 vs float64 {err:.3e}, vs baseline {rel_l2(y, base_y):.3e}, '
          f'bit-identical {torch.equal(y, base_y)}')
    _assert_effect(row, rec.counts, base.counts)
    assert err < 1e-5
    if row.bit:
        assert torch.equal(y, base_y)


@gpu
def test_forward_wino_vp8_inside_wino_vp_wide(s1):
    """wino_vp8: inside forms.wino_vp_wide() the pre-split convs with N % 256 == 0 take the 8-wave form, with
    the switch off never; both bit-identical to the 4-wave baseline (include/wc_kernels.h,
    wc_conv3x3_wino_f16x3_vp8: the same results bit for bit)."""
    base_y, base = s1.forward(**FWD_BASE)
    assert _n(base.counts, 'wc_conv3x3_wino_f16x3_vp8') == 0 and _n(base.counts, 'wc_conv3x3_wino_f16x3_vp') >= 1
    on_y, on = s1.forward(wide=True, **FWD_BASE, wino_vp8=True)
    off_y, off = s1.forward(wide=True, **FWD_BASE, wino_vp8=False)
    _show('wino_vp8=True, wide', on.counts, base.counts)
    _show('wino_vp8=False, wide', off.counts, base.counts)
    assert _n(on.counts, 'wc_conv3x3_wino_f16x3_vp8') >= 1
    assert _n(off.counts, 'wc_conv3x3_wino_f16x3_vp8') == 0
    assert _n(off.counts, 'wc_conv3x3_wino_f16x3_vp') == _n(base.counts, 'wc_conv3x3_wino_f16x3_vp')
    for y in (on_y, off_y):
        assert rel_l2(y, s1.y_ref) < 1e-5
        assert torch.equal(y, base_y)


@gpu
def test_graph_split_from_forms(s1):
    """graph_split set through Forms reaches _GraphStep: the batch of 8 as 1 / 2 / 4 concurrent image groups
    inside the captured graph, bit-identical; the two-group capture runs the 8-wave pre-split convs
    (wino_vp_wide), the unsplit one does not."""
    from weatherconverter_amd import forms
    from weatherconverter_amd.diffusion_model.sample_ddpm import _GraphStep
    x = torch.randn((8, 3, 64, 64), generator=torch.Generator().manual_seed(77)).cuda()
    t = torch.tensor([321], device='cuda')
    outs, counts = {}, {}
    with forms.using(**FWD_BASE), torch.no_grad():
        net = s1.net().eval()
        for k in (1, 2, 4):
            with forms.using(graph_split=k), _recording() as rec:
                step = _GraphStep(net, x)
            assert step.split == k
            outs[k] = step(x, t).clone()
            counts[k] = rec.counts
            del step
        torch.cuda.synchronize()
    print('graph_split vp8 / vp launches while capturing:',
          {k: (_n(c, 'wc_conv3x3_wino_f16x3_vp8'), _n(c, 'wc_conv3x3_wino_f16x3_vp')) for k, c in counts.items()})
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[1], outs[4])
    assert _n(counts[2], 'wc_conv3x3_wino_f16x3_vp8') >= 1
    assert _n(counts[1], 'wc_conv3x3_wino_f16x3_vp8') == 0 and _n(counts[1], 'wc_conv3x3_wino_f16x3_vp') >= 1


# ------------------------------------------------------------------ training matrix
def _check_train(case, loss, grads):
    assert abs(loss - case.loss_ref) <= 1e-5 * abs(case.loss_ref), (loss, case.loss_ref)
    _check({k: g.double() for k, g in grads.items()}, case.g_ref)


@gpu
def test_training_baseline_vs_oracle(s1):
    loss, grads, rec = s1.train(**TRAIN_BASE)
    print('training baseline counts:', dict(sorted(rec.counts.items())))
    print(f'training baseline: _grad_w overwrite {sum(rec.overwrites)} of {len(rec.overwrites)}')
    _check_train(s1, loss, grads)
    assert any(rec.overwrites)  # train_lazy_grad on: some first writer stores instead of adding to a zero fill


@gpu
@pytest.mark.parametrize('row', TRAIN_ROWS, ids=lambda r: r.id)
def test_training_row(s1, row):
    base_loss, base_grads, base = s1.train(**TRAIN_BASE)
    loss, grads, rec = s1.train(**{**TRAIN_BASE, **row.switches})
    _show(row.id, rec.counts, base.counts)
    same = all(torch.equal(grads[k], base_grads[k]) for k in grads)
    print(f'{row.id}: loss {loss!r} (baseline {base_loss!r}, float64 {s1.loss_ref!r}), gradients bit-identical to '
          f'the baseline: {same}; _grad_w overwrite {sum(rec.overwrites)} of {len(rec.overwrites)}')
    _assert_effect(row, rec.counts, base.counts)
    if row.field == 'train_lazy_grad':
        assert any(base.overwrites) and len(rec.overwrites) == len(base.overwrites)
        assert not any(rec.overwrites)
    _check_train(s1, loss, grads)
    if row.bit:
        assert loss == base_loss and same


@gpu
def test_attn_bwd192_fp32_kernel_level():
    """attn_bwd192_fp32 needs head dim 192: K.attention_bwd at C = 768, heads = 4, N = 64 (a shape of
    test_split_attention_lse_matches_float64), both settings against float64 autograd at the fp32-class
    tolerance 1e-5.  The effect: off, dK / dV run f16x3 and raise the per-image max |dqkv| (returns True);
    on, they run fp32 MFMA, which raises no bound (returns False, the bound stays zero), so dK / dV differ in
    their last bits while dQ (the same f16x3 kernel either way) does not.  (K.profile_conv records the
    launcher's last kernel, the dQ kernel in both forms, so the recorded names cannot tell them apart.)"""
    from weatherconverter_amd import forms
    from weatherconverter_amd import kernels as K
    g = torch.Generator().manual_seed(6)
    B, C, heads, N = 2, 768, 4, 64
    d = C // heads
    qkv = torch.randn((B * N, 3 * C), generator=g)
    do = torch.randn((B * N, C), generator=g)
    do[:N] *= 1e-3
    exps = (10, 10, 10)
    o = torch.empty((B * N, C), device='cuda')
    lse = torch.empty((B, heads, N), device='cuda')
    K.attention_fwd_lse(qkv.cuda(), o, lse, B, N, C, heads, precision='f16x3', exps=exps)
    dob = do.abs().reshape(B, -1).amax(1).cuda()
    q_ = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    q, k, v = q_.split(C, dim=-1)
    sh = lambda z: z.reshape(B, N, heads, d).transpose(1, 2)  # noqa: E731
    sc = (sh(q) * d**-0.5) @ sh(k).transpose(-1, -2)
    out = (torch.softmax(sc, -1) @ sh(v)).transpose(1, 2).reshape(B, N, C)
    out.backward(do.double().reshape(B, N, C))
    ref = q_.grad.reshape(B * N, 3 * C)
    res = {}
    for fp32 in (False, True):
        dqkv = torch.empty((B * N, 3 * C), device='cuda')
        amx = torch.zeros(B, device='cuda')
        with forms.using(attn_bwd192_fp32=fp32), _recording() as rec:
            prof = K.profile_conv(True)
            raised = K.attention_bwd(qkv.cuda(), o, do.cuda(), lse, dqkv, B, N, C, heads, precision='f16x3', exps=exps,
                                     dout_bound=dob, dqkv_absmax=amx)
            torch.cuda.synchronize()
            K.profile_conv(False)
        names = [n for n, *_ in prof]
        err = rel_l2(dqkv.cpu(), ref)
        print(f'attn_bwd192_fp32={fp32}: raised {raised}, kernels {names}, rel-L2 {err:.3e}, '
              f'small image {rel_l2(dqkv.cpu()[:N], ref[:N]):.3e}')
        assert rec.counts['wc_attention_bwd_f16x3'] == 1 and f'attn_bwd6_dq_kernel<{d}, true, 3>' in names
        assert err < 1e-5 and rel_l2(dqkv.cpu()[:N], ref[:N]) < 1e-5
        res[fp32] = (raised, dqkv.cpu(), amx.cpu())
    (r0, g0, a0), (r1, g1, a1) = res[False], res[True]
    assert r0 is True and torch.equal(a0, g0.abs().reshape(B, -1).amax(1))
    assert r1 is False and bool((a1 == 0).all())
    assert torch.equal(g0[:, :C], g1[:, :C])  # dQ: the same kernel
    assert not torch.equal(g0[:, C:], g1[:, C:])  # dK / dV: another kernel


# ------------------------------------------------------------------ fresh memory is never read before it is written
def _assert_same_finite(a, b):
    assert bool(torch.isfinite(a).all()), 'non-finite values: a kernel read memory nobody wrote'
    assert torch.equal(a, b), f'differs from the unpoisoned run: rel-L2 {rel_l2(a, b):.3e}'


@gpu
def test_poison_fills_every_fresh_cuda_tensor():
    """The context manager itself: all three allocators, NaN in the float formats and -1 as an integer, a
    CPU tensor left alone, the originals back afterwards."""
    real = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with _poisoned_allocations() as filled:
        a = torch.empty((3, 5), dtype=torch.float32, device='cuda')
        outs = [a, torch.empty_like(a), a.new_empty((7, )), torch.empty(6, dtype=torch.float16, device='cuda'),
                torch.empty(6, dtype=torch.bfloat16, device='cuda'), torch.empty_like(a[:, ::2])]
        ints = [torch.empty((2, 9), dtype=torch.int16, device='cuda'), a.new_empty((4, ), dtype=torch.int64)]
        torch.empty(4)
        assert filled[0] == len(outs) + len(ints)
    assert all(bool(torch.isnan(t).all()) for t in outs) and all(bool((t == -1).all()) for t in ints)
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == real


@gpu
@pytest.mark.parametrize('case', ['s1', 'tiny'])
def test_poisoned_allocations_eager_forward(case, request):
    c = request.getfixturevalue(case)
    y, _ = c.forward(**FWD_BASE)
    yp, _ = c.forward(poison=True, **FWD_BASE)
    _assert_same_finite(yp, y)


@gpu
@pytest.mark.parametrize('lazy', [True, False], ids=['lazy_grad', 'no_lazy_grad'])
@pytest.mark.parametrize('case', ['s1', 'tiny'])
def test_poisoned_allocations_training_step(case, lazy, request):
    c = request.getfixturevalue(case)
    sw = {**TRAIN_BASE, **({} if lazy else {'train_lazy_grad': False})}
    loss, grads, _ = c.train(**sw)
    lossp, gradsp, _ = c.train(poison=True, **sw)
    bad = [k for k in grads if not bool(torch.isfinite(gradsp[k]).all())]
    assert not bad, f'non-finite gradients (a kernel read memory nobody wrote): {bad[:8]}'
    diff = [k for k in grads if not torch.equal(gradsp[k], grads[k])]
    assert not diff, f'gradients differ from the unpoisoned run: {diff[:8]}'
    assert lossp == loss
