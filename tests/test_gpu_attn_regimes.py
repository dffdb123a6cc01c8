"""GPU: the f16x3 attention forward (lse) and backward at the exponents the engines pass.

The cases are tests/test_attn_regimes_cpu.py's GPU_CASES: each passes the exponents recorded for a layer of
the 256-px or 128-px model (tests/golden/attention_exps.json) of its own head dim, not exponents derived from
the test's small shape.  Inputs as the UNet forms them: qkv = GN(y) W_in^T + b_in with synth_tensor-style
weights (uniform +-1/sqrt(C) matrices, gamma 1 + 0.1 n, beta and biases 0.1 u), so |Q|, |K|, |V| respect the
recorded bounds by construction (asserted).  'diffuse' is that input (q, k std 0.6, max P ~ 1/N .. 10/N);
'peaked' scales the q and k rows of W_in by 5 (std 3, max P near 1), with the exponents recomputed at the
recorded layer's group size and never above the recorded ones.  Image 0's dO is 1e-3 of the others'
(per-image edo and eds).  dout_bound is a torch absmax; the row norms the call measures are checked too.

Against float64 autograd: o and lse as test_split_attention_lse_matches_float64 checks them; dq, dk and dv
each on its own, over the batch and per image, at rel-L2 < 1e-5 (the kernel's criterion; over the whole of
dqkv the large dv block hides dq and dk); f16x3 error <= 4 x the error of the kernel precision='bf16x6'
selects on the same inputs + 2e-7 (at head dim 192 that is the fp32-MFMA kernel); dqkv_absmax equals an
absmax of what was written; two runs bit-identical; the attn_bwd6_dq_kernel<d, true, DS> instantiation ran.
The head-dim-192 cases also run with forms.attn_bwd192_fp32 (dK / dV on fp32 MFMA).

The scale of dS: with the workspace for the per-image row norms of dO and V (row_work) the kernels meet the
bound in every case (dq, dk <= 2.8e-6); without it they scale dS under the forward's static bound
2^(14 - ev) on max|V|, and at these exponents dq and dk are 2e-5 .. 1e-2 off float64 in the diffuse cases and
4e-6 .. 1e-4 in the peaked ones, dv unchanged (test_static_v_bound_is_why keeps one such case: the measured
bound is what makes the cases above pass).
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_attn_regimes_cpu as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu

MODES = ['diffuse', 'peaked']
_IDS = [f'B{c[0]}h{c[1]}C{c[2]}N{c[3]}-{c[4].replace("/", ".")}' for c in R.GPU_CASES]
BLOCKS = ('dq', 'dk', 'dv')


@functools.lru_cache(maxsize=None)
def _inputs(ci, mode):
    """(qkv fp32 [B*N][3C], dO, exps, float64 reference dict) of case ci, computed once."""
    from weatherconverter_amd import kernels as K
    B, heads, C, N, key, _ = R.GPU_CASES[ci]
    rec = R.recorded(key)
    d = C // heads
    g = torch.Generator().manual_seed(100 + ci)
    u = lambda *s: torch.rand(s, generator=g) * 2 - 1  # noqa: E731
    y = torch.randn((B, C, N), generator=g) * 2 + 1
    gamma = 1 + 0.1 * torch.randn(C, generator=g)
    beta = 0.1 * u(C)
    w_in = u(3 * C, C) / C**0.5
    b_in = 0.1 * u(3 * C)
    exps = tuple(rec['exps'])
    if mode == 'peaked':
        w_in[:2 * C] *= 5
        again = K.attention_f16x3_exps(w_in, b_in, float(gamma.abs().max()), float(beta.abs().max()),
                                       rec['N'] * rec['C'] // 8)
        exps = tuple(min(a, b) for a, b in zip(exps, again))
    yn = F.group_norm(y.double(), 8, gamma.double(), beta.double(), 1e-5).transpose(1, 2)  # (B, N, C)
    qkv = (yn @ w_in.double().t() + b_in.double()).float().reshape(B * N, 3 * C)
    do = torch.randn((B * N, C), generator=g)
    do[:N] *= 1e-3
    q_ = qkv.double().reshape(B, N, 3 * C).requires_grad_(True)
    q, k, v = q_.split(C, dim=-1)
    sh = lambda z: z.reshape(B, N, heads, d).transpose(1, 2)  # noqa: E731
    sc = (sh(q) * d**-0.5) @ sh(k).transpose(-1, -2)
    p = torch.softmax(sc, -1)
    out = (p @ sh(v)).transpose(1, 2).reshape(B, N, C)
    out.backward(do.double().reshape(B, N, C))
    ref = dict(o=out.detach().reshape(B * N, C), lse=(torch.logsumexp(sc, -1) / np.log(2.0)).detach(),
               dqkv=q_.grad.reshape(B * N, 3 * C), pmax=float(p.detach().max()))
    return qkv, do, exps, ref


def _run(ci, mode, precision, row_bounds=True):
    """One forward + backward of case ci on the GPU: dict(o, lse, dqkv, amx, rows, raised, names)."""
    from weatherconverter_amd import kernels as K
    B, heads, C, N, _, _ = R.GPU_CASES[ci]
    qkv, do, exps, _ = _inputs(ci, mode)
    f3 = precision == 'f16x3'
    qc, dc = qkv.cuda(), do.cuda()
    o = torch.empty((B * N, C), device='cuda')
    lse = torch.empty((B, heads, N), device='cuda')
    K.attention_fwd_lse(qc, o, lse, B, N, C, heads, precision=precision, exps=exps if f3 else None)
    dqkv = torch.full((B * N, 3 * C), float('nan'), device='cuda')
    amx = torch.zeros(B, device='cuda')
    dob = dc.abs().reshape(B, -1).amax(1) if f3 else None
    rows = torch.zeros(2 * B, device='cuda') if f3 and row_bounds else None
    prof = K.profile_conv(True)
    raised = K.attention_bwd(qc, o, dc, lse, dqkv, B, N, C, heads, precision=precision, exps=exps if f3 else None,
                             dout_bound=dob, dqkv_absmax=amx, row_work=rows)
    torch.cuda.synchronize()
    K.profile_conv(False)
    return dict(o=o.cpu(), lse=lse.cpu(), dqkv=dqkv.cpu(), amx=amx.cpu(), raised=raised, names=[n for n, *_ in prof],
                rows=None if rows is None else rows.cpu())


def _block_errors(ci, dqkv, ref):
    """{block: (rel-L2 over the batch, worst image's)} for dq, dk, dv."""
    B, _, C, N, _, _ = R.GPU_CASES[ci]
    out = {}
    for i, blk in enumerate(BLOCKS):
        a, b = dqkv[:, i * C:(i + 1) * C], ref[:, i * C:(i + 1) * C]
        out[blk] = (rel_l2(a, b), max(rel_l2(a[n * N:(n + 1) * N], b[n * N:(n + 1) * N]) for n in range(B)))
    return out


def _fmt(errs):
    return ', '.join(f'{k} {v[0]:.2e} (image {v[1]:.2e})' for k, v in errs.items())


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ci', range(len(R.GPU_CASES)), ids=_IDS)
def test_f16x3_backward_at_the_workload_exponents(ci, mode):
    B, heads, C, N, key, _ = R.GPU_CASES[ci]
    d = C // heads
    qkv, do, exps, ref = _inputs(ci, mode)
    # the recorded bounds hold for these inputs: |Q| 2^eq <= 2^14 ...
    for i, e in enumerate(exps):
        assert float(qkv[:, i * C:(i + 1) * C].abs().max()) * 2.0**e <= 2.0**14, (i, e)
    r = _run(ci, mode, 'f16x3')
    again = _run(ci, mode, 'f16x3')
    x6 = _run(ci, mode, 'bf16x6')
    errs, errs6 = _block_errors(ci, r['dqkv'], ref['dqkv']), _block_errors(ci, x6['dqkv'], ref['dqkv'])
    eo = rel_l2(r['o'], ref['o'])
    elog = float((r['lse'].double() - ref['lse']).abs().max())
    print(f'{_IDS[ci]} {mode}: exps {exps}, max P {ref["pmax"]:.3g}, o {eo:.2e}, lse {elog:.2e}; f16x3 {_fmt(errs)}; '
          f'bf16x6 {_fmt(errs6)}')
    assert rel_l2(r['o'], ref['o']) < 1e-5
    assert elog < 1e-5 * float(ref['lse'].abs().max()) + 1e-6
    ds = 3 if d == 192 else 1
    assert f'attn_bwd6_dq_kernel<{d}, true, {ds}>' in r['names'], r['names']
    for blk in BLOCKS:
        assert errs[blk][0] < 1e-5 and errs[blk][1] < 1e-5, (blk, errs)
        assert errs[blk][0] <= 4 * errs6[blk][0] + 2e-7 and errs[blk][1] <= 4 * errs6[blk][1] + 2e-7, (blk, errs, errs6)
    assert r['raised'] is True and torch.equal(r['amx'], r['dqkv'].abs().reshape(B, -1).amax(1))
    assert torch.equal(r['dqkv'], again['dqkv']) and torch.equal(r['o'], again['o']) and torch.equal(r['lse'], again['lse'])
    # the row norms the call measured (dO, then V) against float64
    rn = lambda z: z.double().reshape(B, N, heads, d).norm(dim=-1).reshape(B, -1).amax(1)  # noqa: E731
    want = torch.cat([rn(do), rn(qkv[:, 2 * C:])])
    assert float(((r['rows'].double() - want) / want).abs().max()) < 1e-6, (r['rows'], want)
    assert torch.equal(r['rows'], again['rows'])


_D192 = [i for i, c in enumerate(R.GPU_CASES) if c[2] // c[1] == 192]


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('ci', _D192, ids=[_IDS[i] for i in _D192])
def test_d192_fp32_dkdv_form_at_the_workload_exponents(ci, mode):
    """forms.attn_bwd192_fp32: dQ on f16x3 (three parts), dK / dV on fp32 MFMA, which raises no bound."""
    from weatherconverter_amd import forms
    _, _, exps, ref = _inputs(ci, mode)
    with forms.using(attn_bwd192_fp32=True):
        r = _run(ci, mode, 'f16x3')
    errs = _block_errors(ci, r['dqkv'], ref['dqkv'])
    print(f'{_IDS[ci]} {mode} attn_bwd192_fp32: exps {exps}, {_fmt(errs)}')
    assert 'attn_bwd6_dq_kernel<192, true, 3>' in r['names'], r['names']
    assert r['raised'] is False and bool((r['amx'] == 0).all())
    for blk in BLOCKS:
        assert errs[blk][0] < 1e-5 and errs[blk][1] < 1e-5, (blk, errs)


def test_static_v_bound_is_why():
    """Without row_work the kernels scale dS under the static bound 2^(14 - ev): at the 64x64 layer's exponents
    the scaled dS of a diffuse softmax lies in fp16's subnormals and dq, dk miss 1e-5 by two orders of
    magnitude, while dv (which does not read dS) is unchanged.  The error the CPU emulation predicts for this
    class under the static rule is 6e-3; a kernel whose static path met 1e-5 here would mean the regime
    moved, and this module's cases no longer pin what they were written for."""
    ci = next(i for i, c in enumerate(R.GPU_CASES) if c[2:4] == (128, 4096))
    _, _, _, ref = _inputs(ci, 'diffuse')
    errs = _block_errors(ci, _run(ci, 'diffuse', 'f16x3', row_bounds=False)['dqkv'], ref['dqkv'])
    print(f'{_IDS[ci]} diffuse, static V bound: {_fmt(errs)}')
    assert errs['dq'][0] > 1e-4 and errs['dk'][0] > 1e-4 and errs['dv'][0] < 1e-5
