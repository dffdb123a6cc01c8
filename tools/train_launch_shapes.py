"""Every launch of one training iteration (add_noise + UNet forward + MSE + backward, no Adam) with its
shape and its time (HIP events around each call, min over 2 iterations): the per-shape view of the training
line.  `python tools/train_launch_shapes.py [--precision bf16] [--size 256] [--batch 32] [--top 40]` prints
the launches grouped by (instantiation, shape), largest total first (default: config 3, 256 px, B=32).

`--json PATH` instead records what the backward's batch-dependent launches select, per workload
(`--workload SIZE:BATCH`, repeatable; default the one of --size / --batch):
  every wc_conv_wgrad* call: entry point, M, segments (C, taps, stride, prologue kind 0 raw / 1 GN / 2
    GN+SiLU), Hm, Wm, B, the split count passed, the kernel instantiation the library reports;
  every wc_gn_bwd_reduce and wc_conv3x3_wino_f16x3_gnb call: B, HW, C and the split count.
Each workload's list is de-duplicated and sorted.  tests/golden/backward_launches.json (read by
tests/test_batch_regimes_cpu.py) is the output of

    python tools/train_launch_shapes.py --precision fp32-class --json tests/golden/backward_launches.json \\
        --workload 256:32 --workload 256:5 --workload 128:4
"""
import argparse
import ctypes
import json
import os
import sys
from collections import defaultdict

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from weatherconverter_amd import _native, kernels  # noqa: E402,F401
from weatherconverter_amd.diffusion_model.config import model_config  # noqa: E402
from weatherconverter_amd.diffusion_model.models.unet_base import Unet  # noqa: E402
from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler  # noqa: E402
from weatherconverter_amd.synthetic import init_synthetic_  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument('--precision', default='bf16', choices=['fp32-class', 'f16', 'bf16'])
ap.add_argument('--size', type=int, default=256, help='image size in pixels')
ap.add_argument('--batch', type=int, default=32)
ap.add_argument('--top', type=int, default=40)
ap.add_argument('--json', metavar='PATH', help='write the batch-dependent backward launches instead of the timing table')
ap.add_argument('--workload', action='append', metavar='SIZE:BATCH', help='with --json: a workload to record (repeatable)')
args = ap.parse_args()

rec = []
_orig = _native.call
_ref_t = type(ctypes.byref(ctypes.c_int()))


def _obj(a):
    return a._obj if isinstance(a, _ref_t) else a


def _shape(args_) -> str:
    a = _obj(args_[0]) if args_ else None
    if isinstance(a, _native.ConvArgs):
        segs = ' + '.join(f'{a.seg[i].C}x{a.seg[i].ntaps}t' for i in range(a.nseg))
        return f'[{segs}] -> {a.N} @ {a.Hm}x{a.Wm}' + (' +res' if a.res else '')
    if isinstance(a, _native.WgradArgs):
        segs = ' + '.join(f'{a.seg[i].C}x{a.seg[i].ntaps}t' for i in range(a.nseg))
        return f'dW {a.M} x [{segs}] @ {a.Hm}x{a.Wm}'
    return ''


def _selected(fn, a, name):
    """The JSON record of a batch-dependent backward launch, or None (argument positions: include/wc_kernels.h)."""
    if fn.startswith('wc_conv_wgrad'):
        w = _obj(a[0])
        segs = [dict(C=s.C, taps=s.ntaps, stride=s.sy, pro=(2 if s.silu else 1) if s.scale else 0)
                for s in (w.seg[i] for i in range(w.nseg))]
        return dict(kind='wgrad', entry=fn, M=w.M, segs=segs, Hm=w.Hm, Wm=w.Wm, B=w.B, splits=int(a[2]), kernel=name)
    if fn == 'wc_gn_bwd_reduce':
        return dict(kind='gn_bwd_reduce', B=int(a[9]), HW=int(a[10]), C=int(a[11]), splits=int(a[12]),
                    has_x=a[2] is not None, silu=bool(a[8]))
    if fn == 'wc_conv3x3_wino_f16x3_gnb':
        c, e = _obj(a[0]), _obj(a[6])
        return dict(kind='wino_gnb', B=c.B, HW=c.Hm * c.Wm, C=c.N, splits=e.splits)
    return None


def call(fn, *a):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    r = _orig(fn, *a)
    e1.record()
    name = _native.last_kernel_name() or fn
    rec.append((fn, name, _shape(a), e0, e1, _selected(fn, a, name) if args.json else None))
    return r


dev = torch.device('cuda', 0)


def iterations(size: int, B: int, n: int):
    """n recorded iterations (after one unrecorded) of the size-px model at batch B: [[rec entries]]."""
    net = Unet(model_config(size))
    init_synthetic_(net, seed=0)
    if args.precision in ('f16', 'bf16'):
        net.set_train_precision(args.precision)
    net = net.to(dev).train()
    sched = LinearNoiseScheduler(1000, 0.0001, 0.02)
    g = torch.Generator().manual_seed(5)
    img = (torch.rand((B, 3, size, size), generator=g) * 2 - 1).to(dev)
    noise = torch.randn((B, 3, size, size), generator=g).to(dev)
    t = torch.randint(0, 1000, (B, ), generator=g).to(dev)
    crit = torch.nn.MSELoss()

    def step():
        for p in net.parameters():
            p.grad = None
        loss = crit(net(sched.add_noise(img, noise, t), t), noise)
        loss.backward()

    step()
    torch.cuda.synchronize()
    _native.call = call
    runs = []
    try:
        for _ in range(n):
            rec.clear()
            step()
            torch.cuda.synchronize()
            runs.append(list(rec))
    finally:
        _native.call = _orig
    return runs


if args.json:
    out = {'precision': args.precision, 'workloads': {}}
    for wl in args.workload or [f'{args.size}:{args.batch}']:
        size, B = (int(v) for v in wl.split(':'))
        sel = {json.dumps(r[5], sort_keys=True) for r in iterations(size, B, 1)[0] if r[5] is not None}
        out['workloads'][f'{size}px_B{B}'] = [json.loads(s) for s in sorted(sel)]
        print(f'{size} px, B={B}: {len(sel)} distinct batch-dependent backward launches')
        torch.cuda.empty_cache()
    with open(args.json, 'w') as fh:
        fh.write('{"precision": %s, "workloads": {\n' % json.dumps(out['precision']))
        fh.write(',\n'.join('%s: [\n%s\n]' % (json.dumps(k), ',\n'.join(json.dumps(r, sort_keys=True) for r in v))
                            for k, v in out['workloads'].items()))
        fh.write('\n}}\n')
    sys.exit(0)

runs = [[(fn, name, shape, e0.elapsed_time(e1) * 1e3) for fn, name, shape, e0, e1, _ in r]
        for r in iterations(args.size, args.batch, 2)]
n = min(len(r) for r in runs)
agg = defaultdict(lambda: [0, 0.0])
total = 0.0
for i in range(n):
    fn, name, shape, _ = runs[0][i]
    us = min(r[i][3] for r in runs)
    total += us
    k = (name[:64], shape)
    agg[k][0] += 1
    agg[k][1] += us
print(f'{n} launches, {total / 1e3:.2f} ms (events around each call)')
for (name, shape), (cnt, us) in sorted(agg.items(), key=lambda kv: -kv[1][1])[:args.top]:
    print(f'{us / 1e3:8.3f} ms {cnt:4d} x {us / cnt:8.1f} us  {name:64s} {shape}')
