"""ctypes binding of ``libwc_kernels.so`` (the C ABI declared in ``include/wc_kernels.h``).

The header is the one declaration of the ABI: the constants, the struct classes and every function's
argument and return types below are read from its text (``_abi.read``) when this module is imported;
nothing here repeats a signature, a field or a value.

There is deliberately no CPU fallback: every product entry point goes through these kernels and a
missing or failing library raises.  ``torch`` is imported before the library is opened so the HIP
runtime torch ships (soname ``libamdhip64.so.7``) is the one the kernels bind to.
"""
import contextlib
import ctypes
import os
import threading

import torch  # noqa: F401  (loads the HIP runtime first)

from . import _abi, _build, forms

ABI = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_kernels.h')).read())  # once per process

EXPORTS = list(ABI.functions)
ConvSeg, ConvArgs, GnbEpi, WgradArgs, WinoPackJob, BsumJob = (ABI.structs[n] for n in (
    'wc_conv_seg', 'wc_conv_args', 'wc_gnb_epi', 'wc_wgrad_args', 'wc_wino_pack_job', 'wc_bsum_job'))
MAX_TAPS, OK, E_SHAPE, E_ARG = (ABI.constants[n] for n in ('WC_MAX_TAPS', 'WC_OK', 'WC_E_SHAPE', 'WC_E_ARG'))
NOISE_NONE, NOISE_TENSOR, NOISE_PHILOX = (ABI.constants['WC_NOISE_' + n] for n in ('NONE', 'TENSOR', 'PHILOX'))
ACT_NONE, ACT_GELU, ACT_SILU, ACT_PRELU, ACT_TANH01 = (ABI.constants['WC_ACT_' + n] for n in (
    'NONE', 'GELU', 'SILU', 'PRELU', 'TANH01'))

# The optimizer entry points (wc_adam_step, wc_grad_norm) are declared in a header of their own.
OPTIM_ABI = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_optim.h')).read())
AdamJob = OPTIM_ABI.structs['wc_adam_job']
# So are the weight-averaging ones (wc_ema_update, wc_ema_swap).
EMA_ABI = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_ema.h')).read())
EmaJob = EMA_ABI.structs['wc_ema_job']
# And the strided sampling step (wc_ddim_step; its kernel sits beside wc_ddpm_step's in wc_misc.hip).
SAMPLER_ABI = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_sampler.h')).read())
# And the training-input kernel (wc_augment_batch: Pillow-exact resize, crop, flip and normalisation).
DATA_ABI = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_data.h')).read())
AugmentJob = DATA_ABI.structs['wc_augment_job']
# And the segmentation label and metric kernels (wc_label_batch, wc_seg_confusion, wc_seg_confusion_pred,
# wc_seg_decode).
SEG_ABI = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_seg.h')).read())
LabelJob = SEG_ABI.structs['wc_label_job']
_SIGNATURES = {**ABI.functions, **OPTIM_ABI.functions, **EMA_ABI.functions, **SAMPLER_ABI.functions,
               **DATA_ABI.functions, **SEG_ABI.functions}

_libs = {}
_active = threading.local()


def lib_path(variant: str = '') -> str:
    """The in-tree library (variant 'single16' / 'bf16': the single-piece builds); WC_KERNEL_LIB
    (WC_KERNEL_LIB_SINGLE16, WC_KERNEL_LIB_BF16) points at another build of it (developer A/B runs only,
    with WC_ALLOW_STALE_LIB=1)."""
    if variant == 'single16':
        return os.environ.get('WC_KERNEL_LIB_SINGLE16', _build.SINGLE16_LIB_PATH)
    if variant == 'bf16':
        return os.environ.get('WC_KERNEL_LIB_BF16', _build.BF16_LIB_PATH)
    return os.environ.get('WC_KERNEL_LIB', _build.LIB_PATH)


@contextlib.contextmanager
def variant(name: str):
    """Route every kernel call of this thread to a library variant inside the block ('' = default,
    'single16' = the single-piece f16 build, 'bf16' = the single-piece bf16 build).  Both libraries stay loaded side by side (RTLD_LOCAL)."""
    prev = getattr(_active, 'v', '')
    _active.v = name
    try:
        yield
    finally:
        _active.v = prev


def active_variant() -> str:
    """The library variant the calling thread's kernel calls go to ('' = the default build)."""
    return getattr(_active, 'v', '')


def _bind(lib, name: str):
    """Give lib.<name> the argument and return types the header declares for it."""
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _SIGNATURES[name]
    return fn


def load(build_if_missing: bool = True):
    """Open the kernel library of the active variant (building it first if it is absent and hipcc
    exists)."""
    v = getattr(_active, 'v', '')
    lib = _libs.get(v)
    if lib is not None:
        return lib
    path = lib_path(v)
    if not os.path.exists(path):
        if not build_if_missing or not os.path.exists(_build.HIPCC):
            raise RuntimeError(f'weatherconverter_amd: HIP kernel library missing at {path}; run '
                               f'python -c "import __graft_entry__ as g; g.build()"')
        _build.build()
    lib = ctypes.CDLL(path)
    verify_source_hash(lib, v)
    forms.announce()  # a run with non-default kernel forms says so before its first native call
    stale_ok = os.environ.get('WC_ALLOW_STALE_LIB', '0') == '1'
    for name in _SIGNATURES:
        if stale_ok and not hasattr(lib, name):  # an older A/B build may lack newer entry points
            continue
        _bind(lib, name)
    for name, value in _selectors.items():  # kernel-form selectors set before this variant was opened
        if hasattr(lib, name) or not stale_ok:
            getattr(lib, name)(value)
    _libs[v] = lib
    return lib


_VARIANT_FLAG = {'': '', 'single16': '1', 'bf16': '2'}


def verify_source_hash(lib, variant: str = ''):
    """Refuse a library built from other sources than this tree's: its compiled-in digest
    (wc_source_hash) must equal _build.source_hash() of the tree's csrc/, header and flags.
    WC_ALLOW_STALE_LIB=1 lets a developer run a deliberately different build (an A/B variant)."""
    stale_ok = os.environ.get('WC_ALLOW_STALE_LIB', '0') == '1'
    if not hasattr(lib, 'wc_source_hash'):
        if stale_ok:  # an older A/B build from before the digest existed
            return None
        raise RuntimeError('weatherconverter_amd: kernel library has no wc_source_hash (built from other sources)')
    got = _bind(lib, 'wc_source_hash')().decode()
    want = _build.source_hash(_VARIANT_FLAG.get(variant, ''))
    if got != want and not stale_ok:
        raise RuntimeError(f'weatherconverter_amd: kernel library {variant or "default"} was built from other sources '
                           f'(library digest {got}, tree digest {want}); rebuild with '
                           f'python -c "import __graft_entry__ as g; g.build()" (or set WC_ALLOW_STALE_LIB=1 for a '
                           f'deliberate A/B build)')
    return got


# Process-wide kernel-form selectors (wc_proj_set_tile): each library variant
# keeps its own static state, so a setting is applied to every loaded variant and replayed into any
# variant opened later (the single16 training line included).
_selectors = {}


def set_selector(name: str, value: int, valid=lambda prev: True) -> int:
    """Apply selector `name` (an int -> previous-int entry point) to every library variant; returns the
    previous value of the active variant's (a result `valid` rejects raises, and nothing is applied)."""
    prev = getattr(load(), name)(int(value))
    if not valid(prev):
        raise RuntimeError(f'weatherconverter_amd kernel {name} failed: bad argument {value}')
    for lib in list(_libs.values()):
        if lib is not load():
            getattr(lib, name)(int(value))
    _selectors[name] = int(value)
    return prev


def check(status: int, op: str):
    if status != 0:
        kind = {E_SHAPE: 'unsupported shape', E_ARG: 'bad argument'}.get(status, f'hipError {status}')
        raise RuntimeError(f'weatherconverter_amd kernel {op} failed: {kind}')


def call(name: str, *args):
    check(getattr(load(), name)(*args), name)


def last_kernel_name() -> str:
    """The exact instantiation (rocprofv3's name) of the kernel the last named launcher started on
    this thread, or '' (wc_last_kernel_name)."""
    return load().wc_last_kernel_name().decode()
