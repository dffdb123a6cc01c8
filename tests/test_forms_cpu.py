"""CPU: the kernel-form switches (weatherconverter_amd/forms.py) — defaults, environment parsing,
using(), the scoped wino_vp_wide flag and the non-default notice."""
import dataclasses
import threading

import pytest

from weatherconverter_amd import forms
from weatherconverter_amd.forms import Forms, from_env

# field -> (environment variable, default): written out, so a changed default shows up here
EXPECTED = {
    'conv_precision': ('WC_CONV_PRECISION', 'f16x3'),
    'pack_device': ('WC_PACK_DEVICE', True),
    'pack_device_convt': ('WC_PACK_DEVICE_CONVT', True),
    'wino': ('WC_WINO', True),
    'wino_vp_min_tiles': ('WC_WINO_VP', 4),
    'wino_vp8': ('WC_WINO_VP8', True),
    'proj_pa': ('WC_PROJ_PA', True),
    'train_gnb_epilogue': ('WC_TRAIN_GNB_EPI', True),
    'train_smallconv': ('WC_TRAIN_SMALLCONV', True),
    'dgrad_f16x3': ('WC_DGRAD_F16X3', True),
    'wgrad3': ('WC_WGRAD3', True),
    'wgrad_f16x3': ('WC_WGRAD_F16X3', True),
    'wgrad3_f16x3': ('WC_WGRAD3_F16X3', True),
    'attn_bwd192_fp32': ('WC_ATTN_BWD192_FP32', False),
    'attn_bwd6': ('WC_ATTN_BWD6', True),
    'attn_bwd_f16x3': ('WC_ATTN_BWD_F16X3', True),
    'graph_split': ('WC_GRAPH_SPLIT', None),
    'attn_presplit': ('WC_ATTN_PRESPLIT', True),
    'gn_partials': ('WC_GN_PARTIALS', True),
    'down_s2d': ('WC_DOWN_S2D', True),
    'up_ct': ('WC_UP_CT', True),
    'pack_raw': ('WC_PACK_RAW', True),
    'pack_batch': ('WC_PACK_BATCH', True),
    'train_gn_partials': ('WC_TRAIN_GN_PARTIALS', True),
    'train_lazy_grad': ('WC_TRAIN_LAZY_GRAD', True),
    'train_dh_sums': ('WC_TRAIN_DH_SUMS', True),
    'check_gbound': ('WC_CHECK_GBOUND', False),
}
DEFAULT_ON = [f for f, (_, d) in EXPECTED.items() if d is True]
DEFAULT_OFF = [f for f, (_, d) in EXPECTED.items() if d is False]


def test_defaults_and_environment_names():
    assert len(EXPECTED) == 27 and len(DEFAULT_ON) == 22 and len(DEFAULT_OFF) == 2
    assert dataclasses.asdict(Forms()) == {f: d for f, (_, d) in EXPECTED.items()}
    assert [f.name for f in dataclasses.fields(Forms)] == list(EXPECTED) == list(forms.ENV)
    assert {f: name for f, (name, _) in forms.ENV.items()} == {f: name for f, (name, _) in EXPECTED.items()}
    assert from_env({}) == Forms()
    assert from_env({'PATH': '/bin', 'WC_KERNEL_LIB': 'x', 'WC_ALLOW_STALE_LIB': '1'}) == Forms()


@pytest.mark.parametrize('field', DEFAULT_ON)
def test_default_on_switch_only_0_turns_off(field):
    name = EXPECTED[field][0]
    assert from_env({name: '0'}) == dataclasses.replace(Forms(), **{field: False})
    for s in ('1', '', '00', 'off', 'false', ' 0', '2'):
        assert from_env({name: s}) == Forms(), s


@pytest.mark.parametrize('field', DEFAULT_OFF)
def test_default_off_switch_only_1_turns_on(field):
    name = EXPECTED[field][0]
    assert from_env({name: '1'}) == dataclasses.replace(Forms(), **{field: True})
    for s in ('0', '', '01', 'on', 'true', ' 1', '2'):
        assert from_env({name: s}) == Forms(), s


def test_int_switches_and_precision():
    assert from_env({'WC_WINO_VP': '0'}).wino_vp_min_tiles == 0
    assert from_env({'WC_WINO_VP': '2'}).wino_vp_min_tiles == 2
    assert from_env({'WC_GRAPH_SPLIT': '4'}).graph_split == 4
    with pytest.raises(ValueError):
        from_env({'WC_WINO_VP': 'x'})
    for p in ('f16x3', 'bf16x6', 'fp32'):
        assert from_env({'WC_CONV_PRECISION': p}).conv_precision == p
    with pytest.raises(RuntimeError) as e:
        from_env({'WC_CONV_PRECISION': 'fp16'})
    assert str(e.value) == ("weatherconverter_amd: WC_CONV_PRECISION must be one of ('f16x3', 'bf16x6', 'fp32'), "
                            "got 'fp16'")


def test_using_nests_restores_and_rejects():
    from weatherconverter_amd import kernels as K
    base = forms.current()
    assert forms.current() is base  # built once
    with forms.using(proj_pa=not base.proj_pa) as a:
        assert forms.current() is a and a == dataclasses.replace(base, proj_pa=not base.proj_pa)
        with forms.using(check_gbound=True, conv_precision='fp32') as b:
            assert forms.current() is b
            assert b == dataclasses.replace(a, check_gbound=True, conv_precision='fp32')
            assert K.default_conv_precision() == 'fp32'
        assert forms.current() is a
    assert forms.current() is base
    with pytest.raises(KeyError):
        with forms.using(wino=not base.wino):
            raise KeyError('in the block')
    assert forms.current() is base
    with pytest.raises(TypeError):
        with forms.using(no_such_switch=True):
            pass
    with pytest.raises(RuntimeError, match='WC_CONV_PRECISION must be one of'):
        with forms.using(conv_precision='fp16'):
            pass
    for bad in ({'wino': 1}, {'wino_vp_min_tiles': '4'}, {'graph_split': 2.0}):
        with pytest.raises(ValueError):
            with forms.using(**bad):
                pass
    assert forms.current() is base


def test_set_wino_vsplit_is_a_set_restore_pair_over_the_active_forms():
    from weatherconverter_amd import kernels as K
    base = forms.current()
    prev = K.set_wino_vsplit(1)
    assert prev == base.wino_vp_min_tiles and forms.current() == dataclasses.replace(base, wino_vp_min_tiles=1)
    assert K.set_wino_vsplit(prev) == 1
    assert forms.current() == base


def test_wino_vp_wide_is_scoped_to_the_calling_context():
    from weatherconverter_amd import kernels as K

    def other_thread():
        seen = []
        th = threading.Thread(target=lambda: seen.append(forms.wino_vp_wide_active()))
        th.start()
        th.join()
        return seen

    with forms.using(wino_vp8=True):
        assert forms.wino_vp_wide_active() is False
        with K.wino_vp_wide():
            assert forms.wino_vp_wide_active() is True
            assert other_thread() == [False]
            with K.wino_vp_wide(False):
                assert forms.wino_vp_wide_active() is False
            assert forms.wino_vp_wide_active() is True
        assert forms.wino_vp_wide_active() is False
        with pytest.raises(KeyError):
            with K.wino_vp_wide(True):
                raise KeyError('in the block')
        assert forms.wino_vp_wide_active() is False
    with forms.using(wino_vp8=False):
        with K.wino_vp_wide():
            assert forms.wino_vp_wide_active() is False


def test_announce_writes_the_notice_once_and_nothing_for_defaults(capsys, monkeypatch):
    with forms.using(**dataclasses.asdict(Forms())):
        monkeypatch.setattr(forms, '_announced', False)
        forms.announce()
        assert capsys.readouterr().err == ''
        monkeypatch.setattr(forms, '_announced', False)
        with forms.using(wino=False):
            forms.announce()
            forms.announce()
        assert capsys.readouterr().err == 'weatherconverter_amd: non-default kernel forms: wino=False\n'


def test_notice_names_exactly_the_non_default_fields():
    assert forms.describe(Forms()) == ''
    assert forms.describe(from_env({})) == ''
    line = forms.describe(Forms(proj_pa=False, wino_vp_min_tiles=0, conv_precision='fp32', graph_split=1))
    assert line == ("weatherconverter_amd: non-default kernel forms: conv_precision='fp32', wino_vp_min_tiles=0, "
                    "proj_pa=False, graph_split=1")
    for f, (_, d) in EXPECTED.items():
        other = {'conv_precision': 'bf16x6', 'wino_vp_min_tiles': 1, 'graph_split': 2}.get(f, not d)
        assert forms.describe(dataclasses.replace(Forms(), **{f: other})).endswith(f'forms: {f}={other!r}')
