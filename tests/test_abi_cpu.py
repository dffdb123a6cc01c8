"""CPU: the binding read from include/wc_kernels.h (_abi.read) -- struct layout against the compiler, the
int64 job rows against the header's field order, and the reader's refusals."""
import ctypes
import os
import subprocess

import pytest
import torch

from conftest import ROOT
from weatherconverter_amd import _abi, _build, _native
from weatherconverter_amd import kernels as K

HEADER = os.path.join(ROOT, 'include', 'wc_kernels.h')


def _fields(cls):
    return [n for n, _ in cls._fields_]


def compiler_layout(tmp_path, structs):
    """{struct: (sizeof, {field: offsetof})} of the tree's header as the host compiler lays it out."""
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "wc_kernels.h"', 'int main() {']
    for name, cls in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in _fields(cls)]
    src, exe = tmp_path / 'layout.cpp', tmp_path / 'layout'
    src.write_text('\n'.join(lines + ['  return 0;', '}', '']))
    subprocess.run([_build.HIPCC, '-x', 'c++', '-O0', '-I', os.path.dirname(HEADER), str(src), '-o', str(exe)],
                   check=True, capture_output=True)
    out = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True,
                                                      text=True).stdout.splitlines())
    return {name: (int(out[name]), {f: int(out[f'{name}.{f}']) for f in _fields(cls)})
            for name, cls in structs.items()}


def ctypes_layout(structs):
    return {name: (ctypes.sizeof(cls), {f: getattr(cls, f).offset for f in _fields(cls)})
            for name, cls in structs.items()}


def test_struct_layout_matches_the_compiler(tmp_path):
    if not os.path.exists(_build.HIPCC):
        pytest.skip('hipcc not available to lay the structs out')
    structs = _native.ABI.structs
    assert list(structs) == ['wc_conv_seg', 'wc_conv_args', 'wc_gnb_epi', 'wc_wino_pack_job', 'wc_wgrad_args',
                             'wc_bsum_job']
    want = compiler_layout(tmp_path, structs)
    assert ctypes_layout(structs) == want
    assert [want[n][0] for n in ('wc_conv_seg', 'wc_conv_args', 'wc_wgrad_args', 'wc_gnb_epi')] == [192, 560, 416, 72]


def test_public_names_are_the_headers():
    assert _native.ConvArgs is _native.ABI.structs['wc_conv_args'] and _native.MAX_TAPS == 16
    assert (_native.E_SHAPE, _native.E_ARG, _native.ACT_TANH01, _native.NOISE_PHILOX) == (-1, -2, 4, 2)
    assert _native.ABI.functions['wc_small_wgrad_workspace'] == (ctypes.c_int64, [ctypes.c_int] * 4)
    assert _native.ABI.functions['wc_version'] == (ctypes.c_char_p, [])
    P, I, L, F, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_double
    assert _native.ABI.functions['wc_sgg_update'] == (I, [P, P, P, P, P, I, I, F, D, D, D, I, P])
    assert _native.ABI.functions['wc_pack_wino'] == (I, [P, I, I, I, P, L, P, P])
    assert _native.ABI.functions['wc_conv3x3_wino_f16x3_gnb'][1][6] is ctypes.POINTER(_native.GnbEpi)


def wino_row_fields(job):
    row = K.wino_pack_job_row(0x1111000011110000, 0x2222000022220000, 0x3333000033330000, 0x4444000044440000, 101, 202,
                              303, 1, 64, 707)
    assert len(row) == ctypes.sizeof(job) // 8
    j = job.from_buffer_copy(torch.tensor(row, dtype=torch.int64).numpy().tobytes())
    return {f: getattr(j, f) for f in _fields(job)}


def test_job_rows_land_in_the_headers_fields():
    assert wino_row_fields(_native.WinoPackJob) == dict(
        w=0x1111000011110000, wres=0x2222000022220000, out=0x3333000033330000, wsinv=0x4444000044440000, N=101, C0=202,
        C1=303, transposed=1, BN=64, wg0=707, pad0=0, pad1=0)
    row = K.bsum_job_row(0x5555000055550000, 0x6666000066660000, 404, 1, 1)
    assert len(row) == ctypes.sizeof(_native.BsumJob) // 8
    j = _native.BsumJob.from_buffer_copy(torch.tensor(row, dtype=torch.int64).numpy().tobytes())
    assert {f: getattr(j, f) for f in _fields(_native.BsumJob)} == dict(
        sums=0x5555000055550000, out=0x6666000066660000, C=404, idx=1, accumulate=1, pad=0)


_WRAP = '#include <stdint.h>\n#define WC_N 4\ntypedef struct wc_s {{ int a[WC_N]; float* p; }} wc_s;\n{}\nint wc_g(int x);\n'


def test_reader_reads_the_subset():
    abi = _abi.read(_WRAP.format('int64_t wc_f(const wc_s* s, const float* x, uint64_t seed, double d, void* stream);'))
    assert abi.constants == {'WC_N': 4} and ctypes.sizeof(abi.structs['wc_s']) == 24
    assert abi.functions['wc_f'] == (ctypes.c_int64, [ctypes.POINTER(abi.structs['wc_s']), ctypes.c_void_p,
                                                      ctypes.c_uint64, ctypes.c_double, ctypes.c_void_p])


@pytest.mark.parametrize('decl, named', [
    ('int wc_f(size_t n, void* stream);', 'size_t'),
    ('int wc_f(void (*done)(int), void* stream);', '(*done)'),
    ('typedef struct wc_t { int a : 3; int b; } wc_t;', 'int a : 3'),
    ('#define WC_M (2 * 8)\ntypedef struct wc_t { int a[WC_M]; } wc_t;', '(2 * 8)'),
    ('typedef struct wc_t { int a[WC_M]; } wc_t;', 'WC_M'),
    ('typedef union wc_t { int a; float b; } wc_t;', 'union'),
    ('typedef struct wc_t { float* a, b; } wc_t;', 'float* a, b'),
    ('float wc_f(int n);', 'float'),
    ('int wc_f(int n) { return n; }', 'return n'),
    ('int wc_f(wc_s s);', 'wc_s s'),
    ('int wc_g(int y);', "declared twice: 'int wc_g(int x)'"),
    ('#pragma pack(1)', 'pragma'),
])
def test_reader_refuses_what_it_does_not_understand(decl, named):
    with pytest.raises(_abi.AbiError) as e:
        _abi.read(_WRAP.format(decl))
    assert named in str(e.value)
