"""CPU: the weight-averaging C ABI as read from include/wc_ema.h, the rejections its entry points make
before any HIP call, and what diffusion_model.ema.EMA does without a GPU -- construction, the warmup
schedule, the state_dict round trip and the checkpoint keys."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT
from weatherconverter_amd import _abi, _native


def _header(name):
    return _abi.read(open(os.path.join(ROOT, 'include', name)).read())


def _model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.GroupNorm(1, 7), torch.nn.Linear(7, 3))


# --------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_two_entry_points_and_the_job():
    abi = _header('wc_ema.h')
    assert list(abi.functions) == ['wc_ema_update', 'wc_ema_swap'] and list(abi.structs) == ['wc_ema_job']
    P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double
    J = ctypes.POINTER(_native.EmaJob)
    assert _native.EmaJob is _native.EMA_ABI.structs['wc_ema_job']
    assert _native.EMA_ABI.functions['wc_ema_update'] == (I, [J, I, I, D, P])
    assert _native.EMA_ABI.functions['wc_ema_swap'] == (I, [J, I, I, P])
    # rows are written as int64 words: pointer and int64 fields only, in this order, 8 bytes each
    job = abi.structs['wc_ema_job']
    assert [n for n, _ in job._fields_] == ['ema', 'p', 'n', 'chunk0']
    assert all(ctypes.sizeof(t) == 8 for _, t in job._fields_) and ctypes.sizeof(job) == 32
    # the three headers share one library and must not declare a name twice
    assert not set(abi.functions) & (set(_native.ABI.functions) | set(_native.OPTIM_ABI.functions))
    assert not set(abi.structs) & (set(_native.ABI.structs) | set(_native.OPTIM_ABI.structs))
    assert all(_native._SIGNATURES[n] is _native.EMA_ABI.functions[n] for n in ('wc_ema_update', 'wc_ema_swap'))


def test_exports_of_the_main_header_are_unchanged():
    assert _native.EXPORTS == list(_header('wc_kernels.h').functions) and len(_native.EXPORTS) == 88
    assert 'wc_ema_update' not in _native.EXPORTS and 'wc_ema_swap' not in _native.EXPORTS
    assert set(_native.OPTIM_ABI.functions) == {'wc_optim_chunk_elems', 'wc_adam_step', 'wc_grad_norm'}


def test_the_build_lists_the_new_source_and_header():
    from weatherconverter_amd import _build
    assert 'wc_ema.hip' in _build.SOURCES and 'wc_ema.h' in _build.ABI_HEADERS
    assert os.path.exists(os.path.join(_build.CSRC, 'wc_ema.hip'))


# --------------------------------------------------------------------------------------- rejections
@pytest.fixture(scope='module')
def lib():
    from weatherconverter_amd import _build
    if not os.path.exists(_build.LIB_PATH):
        if not os.path.exists(_build.HIPCC):
            pytest.skip('hipcc not available to build the library')
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name, (res, args) in _native.EMA_ABI.functions.items():
        assert hasattr(lib, name), name  # the library exports both symbols
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def test_rejections_come_before_any_launch(lib):
    """Every call here returns from the host checks: no HIP call is made, so no GPU is needed."""
    row = _native.EmaJob(0, 0, 4, 0)  # never dereferenced
    jobs = ctypes.pointer(row)
    null = ctypes.POINTER(_native.EmaJob)()
    assert lib.wc_ema_update(null, 1, 1, 0.9, None) == _native.E_ARG
    assert lib.wc_ema_swap(null, 1, 1, None) == _native.E_ARG
    for njobs, nchunks in ((0, 1), (1, 0), (-1, 1), (1, -3), (0, 0)):
        assert lib.wc_ema_update(jobs, njobs, nchunks, 0.9, None) == _native.E_SHAPE
        assert lib.wc_ema_swap(jobs, njobs, nchunks, None) == _native.E_SHAPE
    for decay in (-0.1, 1.5, float('nan'), float('inf'), -float('inf')):
        assert lib.wc_ema_update(jobs, 1, 1, decay, None) == _native.E_ARG
    assert _native.E_ARG != _native.E_SHAPE and _native.OK == 0


# --------------------------------------------------------------------------------------- EMA on the CPU
def test_construction_copies_the_weights():
    from weatherconverter_amd.diffusion_model.ema import EMA
    net = _model()
    ema = EMA(net)
    assert ema.decay == 0.9999 and ema.warmup is False and ema.num_updates == 0
    names = [n for n, _ in net.named_parameters()]
    assert list(ema.shadow) == names and len(names) == 6
    for n, p in net.named_parameters():
        s = ema.shadow[n]
        assert torch.equal(s, p.detach()) and s.data_ptr() != p.data_ptr()
        assert s.dtype == torch.float32 and s.device == p.device and not s.requires_grad and s.grad_fn is None
    with torch.no_grad():
        net[0].weight.add_(1.0)
    assert not torch.equal(ema.shadow['0.weight'], net[0].weight.detach())  # a copy, not a view
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match='decay'):
            EMA(net, bad)


def test_update_and_swap_need_the_device():
    from weatherconverter_amd.diffusion_model.ema import EMA
    ema = EMA(_model())
    for fn in (ema.update, ema.swap):
        with pytest.raises(RuntimeError):  # no torch fallback: CPU operands are refused
            fn()
    assert ema.num_updates == 0


def test_warmup_schedule():
    from weatherconverter_amd.diffusion_model.ema import EMA
    net = _model()
    warm, flat = EMA(net, 0.9999, warmup=True), EMA(net, 0.9999)
    assert warm.decay_at(1) == 2 / 11 and warm.decay_at(10) == 11 / 20
    assert warm.decay_at(10**6) == 0.9999  # (1 + 1e6) / (10 + 1e6) = 0.999991... is above the decay
    assert (1 + 10**6) / (10 + 10**6) > 0.9999
    assert [flat.decay_at(n) for n in (1, 10, 10**6)] == [0.9999] * 3
    assert EMA(net, 0.5, warmup=True).decay_at(10) == 0.5


def test_state_dict_round_trip(tmp_path):
    from weatherconverter_amd.diffusion_model.ema import EMA
    net = _model()
    ema = EMA(net, 0.99, warmup=True)
    ema.num_updates = 17
    with torch.no_grad():
        for s in ema.shadow.values():
            s.mul_(1.5)
    sd = ema.state_dict()
    assert set(sd) == {'decay', 'num_updates', 'warmup', 'shadow'}
    assert sd['decay'] == 0.99 and sd['num_updates'] == 17 and sd['warmup'] is True
    assert type(sd['num_updates']) is int and type(sd['decay']) is float and type(sd['shadow']) is dict
    assert list(sd['shadow']) == [n for n, _ in net.named_parameters()]
    other = EMA(_model(seed=1))
    other.load_state_dict(sd)
    assert (other.decay, other.num_updates, other.warmup) == (0.99, 17, True)
    assert all(torch.equal(other.shadow[n], ema.shadow[n]) for n in ema.shadow)
    assert all(other.shadow[n].data_ptr() != ema.shadow[n].data_ptr() for n in ema.shadow)
    # through a file and the weights_only loader (tensors and plain Python values only)
    path = str(tmp_path / 'ema.pt')
    torch.save(sd, path)
    third = EMA(_model(seed=2))
    third.load_state_dict(torch.load(path, map_location='cpu', weights_only=True))
    assert (third.decay, third.num_updates, third.warmup) == (0.99, 17, True)
    assert all(torch.equal(third.shadow[n], ema.shadow[n]) for n in ema.shadow)


def test_load_state_dict_is_strict():
    from weatherconverter_amd.diffusion_model.ema import EMA
    ema = EMA(_model())
    before = {n: s.clone() for n, s in ema.shadow.items()}
    sd = EMA(_model(seed=1)).state_dict()
    missing = {**sd, 'shadow': {n: t for n, t in sd['shadow'].items() if n != '2.bias'}}
    with pytest.raises(RuntimeError, match='2.bias'):
        ema.load_state_dict(missing)
    extra = {**sd, 'shadow': {**sd['shadow'], 'nope': torch.zeros(1)}}
    with pytest.raises(RuntimeError, match='nope'):
        ema.load_state_dict(extra)
    shape = {**sd, 'shadow': {**sd['shadow'], '0.weight': torch.zeros(7, 4)}}
    with pytest.raises(RuntimeError, match='0.weight'):
        ema.load_state_dict(shape)
    assert all(torch.equal(ema.shadow[n], before[n]) for n in before)  # a refused load changes nothing


def test_shadow_state_dict_loads_into_a_fresh_module():
    from weatherconverter_amd.diffusion_model.ema import EMA
    net = _model()
    ema = EMA(net)
    with torch.no_grad():
        for s in ema.shadow.values():
            s.add_(0.25)
    fresh = _model(seed=3)
    fresh.load_state_dict(ema.shadow_state_dict())
    for (n, p), q in zip(net.named_parameters(), fresh.parameters()):
        assert torch.equal(q.detach(), ema.shadow[n]) and torch.equal(q.detach(), p.detach() + 0.25)
    # copy_to: the cold path that ends a training run
    ema.copy_to(net)
    assert all(torch.equal(p.detach(), ema.shadow[n]) for n, p in net.named_parameters())


def test_unet_shadow_has_the_unets_state_dict_keys():
    import json
    from conftest import GOLDEN
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.diffusion_model.train_ddpm import make_ema
    from weatherconverter_amd.diffusion_model.ema import EMA
    mc = ModelConfig(**json.load(open(os.path.join(GOLDEN, 'manifest.json')))['tiny']['config'])
    net = Unet(mc)
    ema = make_ema(net, 0.999, warmup=True)
    assert type(ema) is EMA and ema.decay == 0.999 and ema.warmup is True
    assert make_ema(net).decay == 0.9999 and make_ema(net).warmup is False
    assert list(ema.shadow_state_dict()) == list(net.state_dict())  # the Unet has no buffers
    Unet(mc).load_state_dict(ema.shadow_state_dict())  # strict


# --------------------------------------------------------------------------------------- checkpoints
def test_checkpoint_keys_with_and_without_ema(tmp_path):
    from weatherconverter_amd.diffusion_model import train_ddpm
    net = _model()
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    ema = train_ddpm.make_ema(net, 0.99)
    ema.num_updates = 5
    three = train_ddpm.save_checkpoint(1, net, opt, str(tmp_path))
    assert three == train_ddpm.checkpoint_path(str(tmp_path), 0, 1)
    ck = torch.load(three, map_location='cpu', weights_only=True)
    assert set(ck) == {'model_state_dict', 'optimizer_state_dict', 'epoch'}  # exactly the reference's
    four = train_ddpm.save_checkpoint(2, net, opt, str(tmp_path), ema=ema)
    ck = torch.load(four, map_location='cpu', weights_only=True)
    assert set(ck) == {'model_state_dict', 'optimizer_state_dict', 'epoch', 'ema_state_dict'}
    assert set(ck['ema_state_dict']) == {'decay', 'num_updates', 'warmup', 'shadow'}
    # the reference's loader reads its three keys and is unaffected by the fourth
    net2 = _model(seed=1)
    assert train_ddpm.load_checkpoint(net2, None, four)[2] == 2
    # with ema=: restored from the four-key file, refused on the three-key one
    ema2 = train_ddpm.make_ema(net2)
    m, o, epoch = train_ddpm.load_checkpoint(net2, torch.optim.Adam(net2.parameters()), four, ema=ema2)
    assert m is net2 and epoch == 2 and ema2.num_updates == 5 and ema2.decay == 0.99
    assert all(torch.equal(ema2.shadow[n], ema.shadow[n]) for n in ema.shadow)
    with pytest.raises(RuntimeError, match='ema_state_dict'):
        train_ddpm.load_checkpoint(net2, None, three, ema=ema2)


def test_load_model_refuses_an_unknown_weights_argument(tmp_path):
    from weatherconverter_amd.diffusion_model import sample_ddpm
    with pytest.raises(ValueError, match='bogus'):
        sample_ddpm.load_model(str(tmp_path / 'absent.ckpt'), None, weights='bogus')
