"""The kernel-form switches: which kernel form, arithmetic and graph split a run takes.

``Forms`` lists every switch with its default; ``ENV`` maps each field to the environment variable
that sets it and the parser of its value.  This module is the only reader of those variables: the
process's active ``Forms`` is built from the environment once, at the first ``current()``, and is
process-wide as the environment was (the training backward runs on autograd's worker threads and
must see the forward's choice).  ``using`` swaps it from Python (tests, tools).  The loader and
build settings (WC_KERNEL_LIB*, WC_ALLOW_STALE_LIB, HIPCC, WC_OFFLOAD_ARCH) are not kernel forms
and stay with _native / _build.
"""
import contextlib
import contextvars
import dataclasses
import os
import sys
from typing import Mapping, Optional

CONV_PRECISIONS = ('f16x3', 'bf16x6', 'fp32')


@dataclasses.dataclass(frozen=True)
class Forms:
    # conv / attention arithmetic: 'f16x3' (the GN-prologue 3x3 convs on two-piece fp16 under a provable
    # range bound, everything else bf16x6), 'bf16x6' (exact 3-piece bf16 split) or 'fp32' (fp32 MFMA)
    conv_precision: str = 'f16x3'
    # CUDA weights packed by the one-launch device kernels (off: the torch-op definitions, the f16x3 / Winograd
    # ones evaluated on the CPU: the same packs bit for bit)
    pack_device: bool = True
    pack_device_convt: bool = True  # the ConvTranspose pack as one device pack of its four parities
    wino: bool = True  # ResBlock 3x3 convs on the Winograd F(2,3)-along-x kernel (off: the direct halo kernel)
    wino_vp_min_tiles: int = 4  # pre-split Winograd segment 0 from this many 128-channel output tiles; 0 = never
    wino_vp8: bool = True  # kernels.wino_vp_wide may select the 8-wave pre-split form (off: never)
    proj_pa: bool = True  # 1x1 projections on the LDS-DMA kernel (off: the register-staged implicit GEMM)
    train_gnb_epilogue: bool = True  # GroupNorm-backward sums in the data-gradient conv's epilogue (off: a reduce pass)
    train_smallconv: bool = True  # 3-channel stem / head convs of training on their fp32 VALU kernels
    dgrad_f16x3: bool = True  # training data gradients on f16x3 under per-image bounds (off: bf16x6)
    wgrad3: bool = True  # the halo-tiled 3x3 weight gradient (off: the generic GEMM)
    wgrad_f16x3: bool = True  # the generic weight gradient on f16x3 given bounds (off: bf16x6)
    wgrad3_f16x3: bool = True  # the halo 3x3 weight gradient on f16x3 given bounds (off: bf16x6)
    attn_bwd192_fp32: bool = False  # the d = 192 attention dK / dV on the fp32-MFMA kernel
    attn_bwd6: bool = True  # the bf16x6 attention backward (off: fp32 MFMA)
    attn_bwd_f16x3: bool = True  # the f16x3 attention backward given bounds (off: bf16x6)
    graph_split: Optional[int] = None  # image groups of the sampling graph; None = 2 if B >= 16 and B even, else 1
    attn_presplit: bool = True  # f16x3 attention on the pre-split in-projection (fixed per engine)
    gn_partials: bool = True  # GroupNorm statistics from the producers' epilogue partials (fixed per engine)
    down_s2d: bool = True  # 4x4 stride-2 down convs on the space-to-depth halo kernel (off: the implicit GEMM)
    up_ct: bool = True  # ConvTranspose as one launch of the halo kernel (off: four parity launches)
    pack_raw: bool = True  # training packs straight from the modules' [Co][Ci][3][3] weights
    pack_batch: bool = True  # a training step's weight packs in one launch (off: lazily one by one)
    train_gn_partials: bool = True  # the training forward's GroupNorm from epilogue partials
    train_lazy_grad: bool = True  # weight gradients accumulated lazily into .grad
    train_dh_sums: bool = True  # dh channel sums from the producer's epilogue (off: a channel_sums pass)
    check_gbound: bool = False  # training checks every tracked gradient bound against the measured absmax

    def __post_init__(self):
        if self.conv_precision not in CONV_PRECISIONS:
            raise RuntimeError(f'weatherconverter_amd: WC_CONV_PRECISION must be one of {CONV_PRECISIONS}, '
                               f'got {self.conv_precision!r}')
        for f in dataclasses.fields(self):
            v = getattr(self, f.name)
            if f.type is bool and not isinstance(v, bool):
                raise ValueError(f'weatherconverter_amd: forms.{f.name} takes a bool, got {v!r}')
        if type(self.wino_vp_min_tiles) is not int:
            raise ValueError(f'weatherconverter_amd: forms.wino_vp_min_tiles takes an int, got {self.wino_vp_min_tiles!r}')
        if self.graph_split is not None and type(self.graph_split) is not int:
            raise ValueError(f'weatherconverter_amd: forms.graph_split takes None or an int, got {self.graph_split!r}')


def _on(s: str) -> bool:
    """A default-on switch: only '0' turns it off."""
    return s != '0'


def _off(s: str) -> bool:
    """A default-off switch: only '1' turns it on."""
    return s == '1'


# field -> (environment variable, parser of its value); an unset variable leaves the field's default
ENV = {
    'conv_precision': ('WC_CONV_PRECISION', str),
    'pack_device': ('WC_PACK_DEVICE', _on),
    'pack_device_convt': ('WC_PACK_DEVICE_CONVT', _on),
    'wino': ('WC_WINO', _on),
    'wino_vp_min_tiles': ('WC_WINO_VP', int),
    'wino_vp8': ('WC_WINO_VP8', _on),
    'proj_pa': ('WC_PROJ_PA', _on),
    'train_gnb_epilogue': ('WC_TRAIN_GNB_EPI', _on),
    'train_smallconv': ('WC_TRAIN_SMALLCONV', _on),
    'dgrad_f16x3': ('WC_DGRAD_F16X3', _on),
    'wgrad3': ('WC_WGRAD3', _on),
    'wgrad_f16x3': ('WC_WGRAD_F16X3', _on),
    'wgrad3_f16x3': ('WC_WGRAD3_F16X3', _on),
    'attn_bwd192_fp32': ('WC_ATTN_BWD192_FP32', _off),
    'attn_bwd6': ('WC_ATTN_BWD6', _on),
    'attn_bwd_f16x3': ('WC_ATTN_BWD_F16X3', _on),
    'graph_split': ('WC_GRAPH_SPLIT', int),
    'attn_presplit': ('WC_ATTN_PRESPLIT', _on),
    'gn_partials': ('WC_GN_PARTIALS', _on),
    'down_s2d': ('WC_DOWN_S2D', _on),
    'up_ct': ('WC_UP_CT', _on),
    'pack_raw': ('WC_PACK_RAW', _on),
    'pack_batch': ('WC_PACK_BATCH', _on),
    'train_gn_partials': ('WC_TRAIN_GN_PARTIALS', _on),
    'train_lazy_grad': ('WC_TRAIN_LAZY_GRAD', _on),
    'train_dh_sums': ('WC_TRAIN_DH_SUMS', _on),
    'check_gbound': ('WC_CHECK_GBOUND', _off),
}


def from_env(env: Mapping[str, str] = os.environ) -> Forms:
    """The Forms a mapping of environment variables selects."""
    return Forms(**{field: parse(env[name]) for field, (name, parse) in ENV.items() if name in env})


_active: Optional[Forms] = None


def current() -> Forms:
    """The process's active Forms (from the environment at the first use)."""
    global _active
    if _active is None:
        _active = from_env()
    return _active


def replace(**overrides) -> Forms:
    """Make current() with `overrides` the active Forms; returns the previous one.  An unknown field
    raises TypeError, a value outside a field's range ValueError (conv_precision: the RuntimeError of
    a bad WC_CONV_PRECISION), and nothing changes."""
    global _active
    prev = current()
    _active = dataclasses.replace(prev, **overrides)
    return prev


@contextlib.contextmanager
def using(**overrides):
    """Inside the block the active Forms is current() with `overrides`; nests.  Process-wide, like the
    environment it stands for (every thread sees it): for tests and tools, not for concurrent use."""
    global _active
    prev = replace(**overrides)
    try:
        yield _active
    finally:
        _active = prev


def describe(forms: Forms) -> str:
    """One line naming the fields of `forms` that differ from the defaults, '' if none does."""
    default = Forms()
    diff = [f'{f.name}={getattr(forms, f.name)!r}' for f in dataclasses.fields(Forms)
            if getattr(forms, f.name) != getattr(default, f.name)]
    return 'weatherconverter_amd: non-default kernel forms: ' + ', '.join(diff) if diff else ''


_announced = False


def announce():
    """Write describe(current()) to stderr, once per process and only if it is not empty (called when
    the kernel library is opened for the first native call)."""
    global _announced
    if not _announced:
        _announced = True
        line = describe(current())
        if line:
            print(line, file=sys.stderr)


# The one scoped switch: a flag of the calling context (thread), not of the process.
_vp_wide = contextvars.ContextVar('wc_wino_vp_wide', default=False)


@contextlib.contextmanager
def wino_vp_wide(on: bool = True):
    """Inside the block the pre-split Winograd convs with N % 256 == 0 take the 8-wave form
    (wino_vp8 off: never).  Set while a forward is captured beside another concurrent one (the
    two-group sampling graph), where that form measured faster; alone the 4-wave form is
    (profiles/r06_wino_vp8_ab.txt).  Unlike every field of Forms this is scoped to the calling
    context: the Winograd forward launches from the thread that called it, and a forward on another
    thread during the block keeps the 4-wave form."""
    token = _vp_wide.set(bool(on) and current().wino_vp8)
    try:
        yield
    finally:
        _vp_wide.reset(token)


def wino_vp_wide_active() -> bool:
    """Whether the calling context is inside a wino_vp_wide block that selects the 8-wave form."""
    return _vp_wide.get()
