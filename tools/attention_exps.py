"""The f16x3 attention exponents the engines pass, per attention layer of a workload (CPU only).

TrainEngine and UnetEngine call kernels.attention_exps_from_norms(l1, |b_in|, max|gamma|, max|beta|, N*C//8)
for every attention layer: the group size N*C//8 is the layer's own, so the exponents of a 64x64 layer are
not those a small test shape derives.  `layers(size)` lists, for the size-px model of config.yaml under the
init_synthetic_ weights (seed 0), every attention layer as dict(layer, C, heads, N, exps) in forward order.

    python tools/attention_exps.py --json tests/golden/attention_exps.json

writes the 256-px and 128-px lists, de-duplicated by (C, heads, N, exps) (read by
tests/test_attn_regimes_cpu.py and tests/test_gpu_attn_regimes.py).
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherconverter_amd import kernels  # noqa: E402
from weatherconverter_amd.diffusion_model.config import model_config  # noqa: E402
from weatherconverter_amd.diffusion_model.models.unet_base import Unet  # noqa: E402
from weatherconverter_amd.synthetic import synth_tensor  # noqa: E402


def attention_sites(net: Unet):
    """(state-dict prefix of the block, index of the attention in it, pixels a side) in forward order: a down
    block runs its attentions before it downsamples, an up block after it upsamples, the mids at the bottom."""
    side = net.model_config.im_size
    sides = []
    for i, blk in enumerate(net.downs):
        sides.append(side)
        if blk.use_attn:
            for j in range(len(blk.attentions)):
                yield f'downs.{i}', j, side
        if net.down_sample[i]:
            side //= 2
    for i, blk in enumerate(net.mids):
        for j in range(len(blk.attentions)):
            yield f'mids.{i}', j, side
    for k, i in enumerate(reversed(range(len(net.downs)))):
        blk = net.ups[k]
        if blk.use_attn:
            for j in range(len(blk.attentions)):
                yield f'ups.{k}', j, sides[i]


def layers(size: int, seed: int = 0):
    """Every attention layer of the size-px model with the exponents the engines compute for it."""
    net = Unet(model_config(size))
    shapes = {k: v.shape for k, v in net.state_dict().items()}
    heads = net.model_config.num_heads

    def syn(key):
        return synth_tensor(key, shapes[key], seed=seed)

    out = []
    for prefix, j, side in attention_sites(net):
        w_in, b_in = syn(f'{prefix}.attentions.{j}.in_proj_weight'), syn(f'{prefix}.attentions.{j}.in_proj_bias')
        gamma, beta = syn(f'{prefix}.attention_norms.{j}.weight'), syn(f'{prefix}.attention_norms.{j}.bias')
        C, N = w_in.shape[1], side * side
        exps = kernels.attention_f16x3_exps(w_in, b_in, float(gamma.abs().max()), float(beta.abs().max()), N * C // 8)
        out.append(dict(layer=f'{prefix}.attentions.{j}', C=C, heads=heads, N=N, exps=list(exps)))
    return out


def distinct(rows):
    """The rows de-duplicated by (C, heads, N, exps), first layer name kept."""
    seen, out = set(), []
    for r in rows:
        key = (r['C'], r['heads'], r['N'], tuple(r['exps']))
        if key not in seen:
            seen.add(key)
            out.append(r)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--json', metavar='PATH', required=True)
    ap.add_argument('--size', type=int, action='append', help='image sizes to record (default 256 and 128)')
    args = ap.parse_args()
    rec = {f'{s}px': distinct(layers(s)) for s in args.size or [256, 128]}
    with open(args.json, 'w') as fh:
        fh.write('{\n' + ',\n'.join('%s: [\n%s\n]' % (json.dumps(k), ',\n'.join(json.dumps(r, sort_keys=True) for r in v))
                                    for k, v in rec.items()) + '\n}\n')
    for k, v in rec.items():
        for r in v:
            print(k, r)
