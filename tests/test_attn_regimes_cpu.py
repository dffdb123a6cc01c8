"""CPU: the f16x3 attention backward at the exponents the engines pass.

TrainEngine and UnetEngine give every attention layer the exponents of kernels.attention_exps_from_norms
at the layer's own group size N*C//8.  tests/golden/attention_exps.json records them for the 256-px and
128-px models of config.yaml under init_synthetic_ weights (python tools/attention_exps.py --json ...): ev
between 0 and 4, i.e. a static bound on max|V| of 2^10 .. 2^14 where the values reach about 3, against the
hand-picked (10, 10, 10) of the older kernel-level tests.

  * Pin: today's weights and rule reproduce the recorded exponents.
  * dS emulation: wc_attention_bwd_f16x3 scales dS = P (dP - D) by 2^eds and splits it into two fp16 pieces.
    For every recorded (head dim d, ev, N) the split is emulated in float64 with one head, at the layer's own
    N and d, on a diffuse softmax (q, k std 0.6) and a peaked one (std 3), V and dO standard normal:
    h = fp16(x 2^eds), l = fp16(x 2^eds - h), eds from kernels.attention_bwd_exps (the host mirror of
    bwd_scales in csrc/wc_attention_bwd6.hip) under the row-norm bound the engine passes.  Asserted: scaled
    |dS| < 2^15 (the range bound holds) and dQ = dS K, dK = dS^T Q from the quantised dS within 1e-5 rel-L2 of
    the unquantised (the kernel's criterion against float64).
  * Coverage: every recorded layer the f16x3 backward takes is classified by (d, ev, N class) and a case of
    tests/test_gpu_attn_regimes.py must sit in each class.  (eq and ek scale S alone, which is accumulated in
    fp32 and rescaled exactly; ev is the exponent that enters the static eds.)

What the two rules give (worst of dQ, dK; the range over the twelve recorded classes, the largest at d = 128,
ev = 1, N = 4096; `python tests/test_attn_regimes_cpu.py` prints every class):

    rule                                         diffuse              peaked               max scaled |dS|
    static: max|V| <= 2^(14 - ev)                6.7e-5 .. 6.0e-3     3.9e-6 .. 6.2e-5     2^-14.5 .. 2^-2.8
    Cauchy-Schwarz on the measured row norms     5.1e-8 .. 3.7e-7     4.6e-8 .. 6.2e-8     2^-0.5  .. 2^9.2

The static rule was the only one before this module (attention_bwd_exps without row_norms, what the kernel
still does when it gets no row-norm workspace): under it test_ds_split_emulation fails in all twelve diffuse
classes and in eight of the twelve peaked ones; scaled dS lies at or below the smallest normal fp16 (2^-14), the
high piece keeps a few bits and the low piece is zero.  A measured per-image max|V| in place of the static
bound passes (2.6e-7 .. 5.9e-6) with less than a factor 2 to spare at N = 4096 and was not enough on the GPU
(dK 5.1e-6 at d = 128, N = 4096, above 4 x the bf16x6 kernel's error).
"""
import json
import math
import os

import pytest
import torch

from conftest import GOLDEN

from weatherconverter_amd.kernels import ATTN_BWD_F3_DIMS as F3_BWD_DIMS  # head dims wc_attention_bwd_f16x3 takes

# ---------------------------------------------------------------- the GPU cases (tests/test_gpu_attn_regimes.py)
# (B, heads, C, N, the recorded layer whose exponents the case passes, note)
GPU_CASES = [
    (1, 1, 64, 4096, '128px/downs.1.attentions.0', 'd = 64'),
    (1, 1, 128, 1024, '256px/mids.1.attentions.0', 'd = 128'),
    (1, 1, 192, 1024, '256px/downs.3.attentions.0', 'd = 192: dQ in three parts, dK / dV with V rows in LDS'),
    (2, 4, 768, 256, '128px/downs.3.attentions.0', 'd = 192, four heads'),
    (2, 4, 256, 33, '128px/ups.0.attentions.0', 'tail: N % 32 = 1'),
    (2, 4, 128, 100, '256px/ups.1.attentions.1', 'd = 32, tail'),
    (2, 1, 32, 200, '256px/ups.1.attentions.0', 'd = 32, one head'),
    # the classes of the workloads the seven above leave open
    (1, 1, 128, 4096, '256px/downs.2.attentions.0', 'd = 128 at 64x64: the loosest static bound of the workloads'),
    (1, 1, 128, 256, '128px/mids.1.attentions.0', 'd = 128 at 16x16'),
    (1, 1, 64, 1024, '256px/ups.0.attentions.0', 'd = 64 at 32x32'),
    (1, 1, 32, 4096, '256px/ups.1.attentions.0', 'd = 32 at 64x64, ev = 3'),
    (1, 1, 32, 4096, '256px/ups.1.attentions.1', 'd = 32 at 64x64, ev = 2'),
    (1, 1, 32, 1024, '128px/ups.1.attentions.0', 'd = 32 at 32x32, ev = 4'),
    (1, 1, 32, 1024, '128px/ups.1.attentions.1', 'd = 32 at 32x32, ev = 3'),
]


def fixture():
    with open(os.path.join(GOLDEN, 'attention_exps.json')) as fh:
        return json.load(fh)


def recorded(key):
    """The recorded layer 'SIZEpx/state-dict name'."""
    size, name = key.split('/')
    return next(r for r in fixture()[size] if r['layer'] == name)


def n_class(N):
    return 'le256' if N <= 256 else ('le1024' if N <= 1024 else 'le4096')


def layer_class(r):
    return r['C'] // r['heads'], r['exps'][2], n_class(r['N'])


def case_class(case):
    B, heads, C, N, key, _ = case
    return C // heads, recorded(key)['exps'][2], n_class(N)


def f3_layers():
    """The recorded layers the f16x3 backward takes (the 64-channel layer of the 128-px model has head dim
    16: fp32 MFMA)."""
    return [(size, r) for size, rows in fixture().items() for r in rows if r['C'] // r['heads'] in F3_BWD_DIMS]


# ---------------------------------------------------------------- the dS split in float64
def ds_emulation(N, d, ev, std, measured=True, seed=0):
    """(max scaled |dS|, rel-L2 of dQ, of dK) of one head with dS split as the kernel splits it."""
    from weatherconverter_amd import kernels as K
    g = torch.Generator().manual_seed(seed)
    q, k = (torch.randn((N, d), generator=g, dtype=torch.float64) * std for _ in range(2))
    v, do = (torch.randn((N, d), generator=g, dtype=torch.float64) for _ in range(2))
    p = torch.softmax(q @ k.t() * d**-0.5, -1)
    ds = p * (do @ v.t() - (do * (p @ v)).sum(1, keepdim=True))
    rows = (float(do.norm(dim=1).max()), float(v.norm(dim=1).max())) if measured else None
    _, eds, _ = K.attention_bwd_exps(d, ev, float(do.abs().max()), rows)
    scaled = (ds * 2.0**eds).float()  # the kernel forms dS and its scaled value in fp32
    h, l = K._split2(scaled)
    dsq = (h.double() + l.double()) * 2.0**-eds
    err = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    return float(scaled.abs().max()), err(dsq @ k, ds @ k), err(dsq.t() @ q, ds.t() @ q), float(p.max())


def emulation_classes():
    return sorted({(r['C'] // r['heads'], r['exps'][2], r['N']) for _, r in f3_layers()})


# ---------------------------------------------------------------- tests
def test_fixture_holds_both_workloads():
    fx = fixture()
    assert list(fx) == ['256px', '128px']
    for rows in fx.values():
        assert all(r['heads'] == 4 and len(r['exps']) == 3 for r in rows)
        keys = [(r['C'], r['heads'], r['N'], tuple(r['exps'])) for r in rows]
        assert len(set(keys)) == len(keys)  # de-duplicated
    # the regime: the static bound on max|V| is 2^10 .. 2^14
    assert {r['exps'][2] for _, r in f3_layers()} <= {0, 1, 2, 3, 4}
    assert {r['N'] for _, r in f3_layers()} == {256, 1024, 4096}


@pytest.mark.parametrize('size', [256, 128])
def test_synthetic_weights_reproduce_the_recorded_exps(size):
    """kernels.attention_exps_from_norms (through attention_f16x3_exps) on the init_synthetic_ weights at each
    layer's own group size gives the recorded exponents: a changed bound rule, initialisation or config moves
    the regime and fails here."""
    from tools.attention_exps import distinct, layers
    assert distinct(layers(size)) == fixture()[f'{size}px']


def test_attention_bwd_exps_mirrors_bwd_scales():
    """The host statement of the C rule at hand-worked values (bwd_scales: e = floor(log2 max|dO|),
    edo = 13 - e; eds = ev - e - 2 - ceil(log2 d) under the static bound, 11 - fo - fv under the row norms)."""
    from weatherconverter_amd import kernels as K
    assert K.attention_bwd_exps(64, 2, 1.0) == (13, 2 - 0 - 2 - 6, 14)
    assert K.attention_bwd_exps(192, 1, 3.9) == (12, 1 - 1 - 2 - 8, 14)
    assert K.attention_bwd_exps(128, 10, 0.004) == (13 + 8, 10 + 8 - 2 - 7, 14)
    assert K.attention_bwd_exps(64, 2, 1.0, (13.5, 7.9)) == (13, 11 - 3 - 2, 14)  # 2 * 13.5 * 7.9 < 2^(3 + 2 + 3)
    assert K.attention_bwd_exps(64, 2, 1.0, (16.0, 8.0)) == (13, 11 - 4 - 3, 14)  # powers of two: < 2^5, < 2^4
    assert K.attention_bwd_exps(64, 2, 1.0, (0.3, 0.01)) == (13, 11 + 2 + 7, 14)
    assert K.attention_bwd_exps(32, 3, 0.0, (0.0, 1.0)) == (60, 60, 14) and K.attention_bwd_exps(32, 3, 1.0, (1.0, 0.0))[1] == 60
    # Cauchy-Schwarz is never looser than d max max, nor than the static rule for values that respect ev
    for d in F3_BWD_DIMS:
        for ev in range(0, 5):
            for vmax in (0.1, 2.9, 2.0**(14 - ev) * 0.999):
                rows = (d**0.5 * 1.0, d**0.5 * vmax)  # the largest norms rows of such values can have
                assert K.attention_bwd_exps(d, ev, 1.0, rows)[1] >= K.attention_bwd_exps(d, ev, 1.0)[1], (d, ev, vmax)


@pytest.mark.parametrize('std', [0.6, 3.0], ids=['diffuse', 'peaked'])
@pytest.mark.parametrize('d,ev,N', emulation_classes(), ids=lambda v: str(v))
def test_ds_split_emulation(d, ev, N, std):
    top, edq, edk, pmax = ds_emulation(N, d, ev, std)
    print(f'd={d} ev={ev} N={N} std={std}: max P {pmax:.3g}, scaled |dS| <= 2^{math.log2(top):.1f}, '
          f'dQ {edq:.2e}, dK {edk:.2e}')
    assert top < 2.0**15
    assert edq < 1e-5 and edk < 1e-5


def test_gpu_cases_name_layers_of_their_head_dim():
    for case in GPU_CASES:
        B, heads, C, N, key, _ = case
        r = recorded(key)
        assert C // heads == r['C'] // r['heads'] and C // heads in F3_BWD_DIMS, case


def test_every_workload_class_has_a_gpu_case():
    have = {case_class(c) for c in GPU_CASES}
    missing = {layer_class(r): f'{size}/{r["layer"]}' for size, r in f3_layers() if layer_class(r) not in have}
    assert not missing, '\n'.join(f'(d, ev, N class) = {c} has no GPU case; first reached by {k}'
                                  for c, k in sorted(missing.items()))


if __name__ == '__main__':  # the table of the module docstring
    for d, ev, N in emulation_classes():
        for std in (0.6, 3.0):
            row = [f'd={d:3d} ev={ev} N={N:4d} std={std}']
            for measured in (False, True):
                top, edq, edk, pmax = ds_emulation(N, d, ev, std, measured)
                row.append(f'{"measured" if measured else "static"}: 2^{math.log2(top):6.1f} dQ {edq:.2e} dK {edk:.2e}')
            print('  '.join(row))
