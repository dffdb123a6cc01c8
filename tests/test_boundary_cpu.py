"""CPU: the drop-in boundary — package API, parameter tree, config schema, C-ABI library exports."""
import ctypes
import json
import os
import re

import pytest
import torch

from conftest import GOLDEN, ROOT
from weatherconverter_amd.diffusion_model.config import ModelConfig, load_config, model_config
from weatherconverter_amd.diffusion_model.models.unet_base import Unet, get_time_embedding
from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler

MANIFEST = json.load(open(os.path.join(GOLDEN, 'manifest.json')))


@pytest.mark.parametrize('name', ['tiny', 'default_64', 'default_128', 'default_256'])
def test_unet_state_dict_is_reference_layout(name):
    m = MANIFEST[name]
    net = Unet(ModelConfig(**m['config']))
    ours = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert ours == [[k, s] for k, s in m['keys']]  # same keys, shapes AND order


def test_default_config_loads():
    cfg = load_config()
    assert cfg.diffusion.num_timesteps == 1000 and cfg.model.im_size == 128
    assert model_config(256).im_size == 256


def test_unet_forward_refuses_cpu():
    net = Unet(model_config(64)).eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match='GPU only'):
        net(torch.zeros(1, 3, 64, 64), torch.tensor([1]))


def test_scheduler_tables_cpu():
    s = LinearNoiseScheduler(1000, 0.0001, 0.02, device=torch.device('cpu'))
    assert s.betas.dtype == torch.float32 and s.alpha_cum_prod.shape == (1000, )
    b, s1m, sqa, sig = s.step_scalars(500)
    assert 0 < b < 0.02 and 0 < sig < 1 and 0 < sqa < 1


def test_host_time_embedding_helper():
    e = get_time_embedding(torch.tensor([0, 5]), 128)
    assert e.shape == (2, 128) and torch.all(e[0, 64:] == 1)


# ------------------------------------------------------------------ the supported envelope (engine.check_supported)
def _mc(**overrides):
    return ModelConfig(**{**MANIFEST['tiny']['config'], **overrides})


@pytest.mark.parametrize('name', ['tiny', 'default_64', 'default_128', 'default_256'])
@pytest.mark.parametrize('training', [False, True])
@pytest.mark.parametrize('precision', ['f16x3', 'bf16x6', 'fp32'])
def test_check_supported_accepts_golden_configs(name, training, precision):
    from weatherconverter_amd.diffusion_model.models.engine import check_supported
    check_supported(ModelConfig(**MANIFEST[name]['config']), precision, training)
    if training:
        check_supported(ModelConfig(**MANIFEST[name]['config']), 'f16', True)
        check_supported(ModelConfig(**MANIFEST[name]['config']), 'bf16', True)


def test_check_supported_accepts_the_shapes_matrix():
    """Every case x precision tests/test_gpu_shapes.py runs is inside the envelope, and the ones it expects
    to be rejected are outside, with the message naming the field."""
    from test_gpu_shapes import CASES, PRECISIONS
    from weatherconverter_amd.diffusion_model.models.engine import check_supported
    rejected = []
    for s in CASES:
        mc = ModelConfig(**s.config)
        for training, admitted in ((False, s.fwd), (True, s.train)):
            for p in PRECISIONS:
                if p in admitted:
                    check_supported(mc, p, training)
                else:
                    with pytest.raises(RuntimeError, match=s.rejects):
                        check_supported(mc, p, training)
                    rejected.append((s.id, p, training))
    assert sorted(rejected) == sorted([('ch48', p, tr) for p in PRECISIONS for tr in (False, True)] +
                                      [('c6', p, True) for p in PRECISIONS])


@pytest.mark.parametrize('overrides,precision,training,field,value', [
    (dict(down_channels=[24, 64, 64, 128]), 'f16x3', False, 'down_channels', '24'),
    (dict(down_channels=[24, 64, 64, 128]), 'bf16x6', True, 'down_channels', '24'),
    (dict(down_channels=[32, 64, 64, 128], mid_channels=[128, 72, 64]), 'f16x3', False, 'mid_channels', '72'),
    (dict(down_channels=[48, 96, 144, 144], mid_channels=[144, 144], num_heads=6), 'fp32', False, 'down_channels', '48'),
    (dict(down_channels=[48, 96, 144, 144], mid_channels=[144, 144], num_heads=6), 'fp32', True, 'down_channels', '48'),
    (dict(down_channels=[32, 64, 64, 160], mid_channels=[160, 160, 64]), 'f16x3', False, 'num_heads', 'head dim 40'),
    (dict(down_channels=[32, 64, 64, 160], mid_channels=[160, 160, 64]), 'fp32', True, 'num_heads', 'head dim 40'),
    (dict(down_channels=[48, 96, 144, 144], mid_channels=[144, 144], num_heads=6), 'f16x3', False, 'down_channels',
     'GroupNorm'),
    (dict(num_heads=3), 'f16x3', False, 'num_heads', 'must divide'),
    (dict(time_emb_dim=260), 'f16x3', False, 'time_emb_dim', '260'),
    (dict(time_emb_dim=258), 'f16x3', True, 'time_emb_dim', '258'),
    (dict(im_channels=17), 'f16x3', False, 'im_channels', '17'),
    (dict(im_channels=6), 'f16x3', True, 'im_channels', '6'),
])
def test_check_supported_rejects_naming_the_field(overrides, precision, training, field, value):
    from weatherconverter_amd.diffusion_model.models.engine import check_supported
    with pytest.raises(RuntimeError) as e:
        check_supported(_mc(**overrides), precision, training)
    assert f'{field} = ' in str(e.value) and value in str(e.value), str(e.value)


def test_check_supported_reads_no_device(monkeypatch):
    """Pure Python over the config: loading the native library or touching torch.cuda fails the call."""
    from weatherconverter_amd import _native
    from weatherconverter_amd.diffusion_model.models.engine import check_supported

    def boom(*a, **k):
        raise AssertionError('check_supported touched the device')

    monkeypatch.setattr(_native, 'load', boom)
    monkeypatch.setattr(_native, 'call', boom)
    monkeypatch.setattr(torch.cuda, 'current_device', boom)
    check_supported(_mc(), 'f16x3', True)


def _csrc(name):
    return open(os.path.join(ROOT, 'weatherconverter_amd', 'csrc', name)).read()


def _cases(src: str, fn: str):
    """The `case N:` / WC_BWD_CASE(N) labels of the first switch after `fn` in a csrc file."""
    body = src[src.index(fn):]
    body = body[re.search(r'switch \((D|C / heads)\)', body).start():]
    body = body[:body.index('default:')]
    return sorted(int(n) for n in re.findall(r'(?:case\s+|WC_BWD_CASE\()(\d+)', body))


def test_envelope_constants_repeat_the_native_host_checks():
    """check_supported's rules come from constants in kernels.py; each must equal the native check it repeats
    (read from the source: the dispatch switches, BK, wc_temb's and wc_conv_in's limits)."""
    from weatherconverter_amd import kernels as K
    assert list(K.ATTN_FWD_DIMS) == _cases(_csrc('wc_attention.hip'), 'int attention_fwd_any(')
    att6 = _csrc('wc_attention6.hip')
    split = _cases(att6, 'launch_att6')
    assert list(K.ATTN_SPLIT_DIMS) == split
    # the pre-split forms dispatch over the same set
    for m in re.finditer(r'switch \(C / heads\)(.*?)default:', att6, flags=re.S):
        assert sorted(int(n) for n in re.findall(r'case\s+(\d+)', m.group(1))) == split
    assert list(K.ATTN_BWD_DIMS) == _cases(_csrc('wc_attention_bwd.hip'), 'extern "C" int wc_attention_bwd(')
    assert set(K.ATTN_BWD_DIMS) == set(K.ATTN_FWD_DIMS)  # whatever runs forward also trains
    assert list(K.ATTN_BWD_F3_DIMS) == _cases(_csrc('wc_attention_bwd6.hip'), 'static int attention_bwd_split(')
    assert all(d % 8 == 0 for d in K.ATTN_BWD_DIMS)  # BwdCfg: DH = D / 2 read four floats at a time
    assert re.search(r'constexpr int BK = (\d+);', _csrc('wc_conv.hip')).group(1) == str(K.IGEMM_BK)
    misc = _csrc('wc_misc.hip')
    assert f'D > {K.TEMB_MAX_D} || D % 4 != 0' in misc
    assert f'Cin < 1 || Cin > {K.CONV_IN_MAX_CIN}' in misc and 'if (lds > 64 * 1024) return WC_E_SHAPE;' in misc
    assert K.CONV_IN_MAX_LDS == 64 * 1024
    assert f'(C / groups) % {K.GN_VEC} != 0' in _csrc('wc_gn.hip') and K.GN_GROUPS == 8
    # the split-precision packs refuse what SPLIT_CK admits no more of
    pk = open(os.path.join(ROOT, 'weatherconverter_amd', 'kernels.py')).read()
    assert f'% {K.SPLIT_CK} == 0' in pk[pk.index('def pack_x6('):pk.index('def f16x3_a_exp(')]


def _header_functions():
    src = open(os.path.join(ROOT, 'include', 'wc_kernels.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'\b(wc_[a-z0-9_]+)\s*\(', src)))


def test_c_abi_library_exports_every_header_symbol():
    from weatherconverter_amd import _build
    path = _build.LIB_PATH
    if not os.path.exists(path):
        if not os.path.exists(_build.HIPCC):
            pytest.skip('hipcc not available to build the library')
        _build.build()
    lib = ctypes.CDLL(path)
    names = _header_functions()
    assert 'wc_conv_igemm' in names and 'wc_attention_fwd' in names
    for n in names:
        assert hasattr(lib, n), n
    lib.wc_version.restype = ctypes.c_char_p
    assert b'gfx950' in lib.wc_version()
    from weatherconverter_amd import _native
    assert sorted(_native.EXPORTS) == names


def test_every_header_function_has_a_derived_signature():
    """_header_functions() finds the names with a regex of its own; the header reader must have bound exactly
    those (a prototype it missed would be called with ctypes' default types)."""
    from weatherconverter_amd import _native
    names = _header_functions()
    assert len(names) == 88 and sorted(_native.ABI.functions) == names
    assert all(isinstance(a, list) and r is not None for r, a in _native.ABI.functions.values())


def test_library_refuses_sources_other_than_the_trees(tmp_path, monkeypatch):
    """The library carries the digest of the sources it was built from; the loader compares it with the
    tree's and refuses a mismatch (one flipped byte in a copy of csrc/ is enough)."""
    import shutil
    from weatherconverter_amd import _build, _native
    if not os.path.exists(_build.LIB_PATH):
        pytest.skip('library not built')
    lib = ctypes.CDLL(_build.LIB_PATH)
    digest = _native.verify_source_hash(lib, '')  # the in-tree library matches the tree
    lib.wc_version.restype = ctypes.c_char_p
    assert lib.wc_version().decode().endswith('src:' + digest)
    copy = tmp_path / 'csrc'
    shutil.copytree(_build.CSRC, copy)
    src = copy / 'wc_wino.hip'
    data = bytearray(src.read_bytes())
    data[len(data) // 2] ^= 0x01
    src.write_bytes(bytes(data))
    monkeypatch.setattr(_build, 'CSRC', str(copy))
    monkeypatch.delenv('WC_ALLOW_STALE_LIB', raising=False)
    with pytest.raises(RuntimeError, match='built from other sources'):
        _native.verify_source_hash(lib, '')
    monkeypatch.setenv('WC_ALLOW_STALE_LIB', '1')
    assert _native.verify_source_hash(lib, '') == digest  # the developer override


def test_product_package_never_imports_oracle():
    pkg = os.path.join(ROOT, 'weatherconverter_amd')
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith('.py'):
                txt = open(os.path.join(dp, f)).read()
                assert 'oracle' not in re.findall(r'^\s*(?:from|import)\s+(\w+)', txt, flags=re.M), f


def test_kernel_form_selectors_reach_every_library_variant():
    """wc_proj_set_tile keeps static state per library: a setting made before
    the single16 variant is opened is replayed into it, and one made after reaches both (no GPU call)."""
    from weatherconverter_amd import _build, _native
    from weatherconverter_amd import kernels as K
    if not (os.path.exists(_build.LIB_PATH) and os.path.exists(_build.SINGLE16_LIB_PATH)):
        pytest.skip('kernel libraries not built')
    p_tile = K.set_proj_tile(128)
    try:
        with _native.variant('single16'):
            lib16 = _native.load()
        assert lib16.wc_proj_set_tile(128) == 128  # replayed
        K.set_proj_tile(256)
        assert lib16.wc_proj_set_tile(256) == 256  # applied to the already-open variant too
        with pytest.raises(RuntimeError):
            K.set_proj_tile(77)
        assert _native.load().wc_proj_set_tile(256) == 256  # a rejected value changes nothing
    finally:
        K.set_proj_tile(p_tile)
