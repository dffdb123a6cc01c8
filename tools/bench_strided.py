"""Per-step time of strided sampling beside the full schedule's, BASELINE config 2 (256 px UNet, B=16,
Philox noise, HIP graph) on one MI355X: 50 DDIM steps (sample_tensor(steps=50)'s transitions,
wc_ddim_step) and the first 50 steps of T = 1000 (bench.py's loop, wc_ddpm_step), on one captured
UNet graph, in alternating rounds.  Prints one JSON line.

The only expectation is per-step parity (the box spread of bench.py is +-3 %): the UNet forward is the
same graph and the new step kernel moves the same 12 bytes per element as the old.  The factor a user
buys is the number of steps, which this does not measure.

  python tools/bench_strided.py [--steps 50] [--rounds 3] [--eta 1.0] [--trace kernel_stats.csv]

--trace: a rocprofv3 --kernel-trace --stats CSV of a run of this tool; the mean durations of
ddim_step_kernel and ddpm_step_kernel are read from it into the line.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def kernel_means(path):
    """{kernel: mean us} of the two step kernels in a rocprofv3 kernel-stats CSV."""
    out = {}
    for row in csv.DictReader(open(path)):
        for k in ('ddim_step_kernel', 'ddpm_step_kernel'):
            if k + '(' in row['Name']:
                out[k + '_mean_us'] = round(float(row['AverageNs']) / 1e3, 3)
                out[k + '_calls'] = int(row['Calls'])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--timesteps', type=int, default=1000)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--eta', type=float, default=1.0)
    ap.add_argument('--seed', type=int, default=3455)
    ap.add_argument('--trace', default=None)
    a = ap.parse_args()

    from weatherconverter_amd import kernels
    from weatherconverter_amd.diffusion_model.config import model_config
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.diffusion_model.sample_ddpm import _GraphStep
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    from weatherconverter_amd.synthetic import init_synthetic_

    dev = torch.device('cuda', 0)
    mc = model_config(a.size)
    model = Unet(mc)
    init_synthetic_(model, seed=0)
    model.set_conv_precision(kernels.default_conv_precision())
    model = model.to(dev).eval()
    T, K = a.timesteps, a.steps
    sched = LinearNoiseScheduler(T, 0.0001, 0.02, device=dev)
    shape = (a.batch, mc.im_channels, mc.im_size, mc.im_size)
    ts = torch.arange(T, device=dev, dtype=torch.long)
    tau = sched.timestep_sequence(K)
    hops = [(tau[k], tau[k - 1] if k > 0 else -1) for k in reversed(range(K))]

    with torch.no_grad():
        x_T = kernels.philox_normal(shape, dev, a.seed, step=T)
        runner = _GraphStep(model, x_T)
        nxt = torch.empty_like(x_T)

        def full(n):  # the first n steps of the T-step schedule (bench.py's loop)
            nonlocal nxt
            x = x_T.clone()
            for j in range(n):
                i = T - 1 - j
                eps = runner(x, ts[i:i + 1])
                sched.step(x, eps, i, out=nxt, noise='philox', seed=a.seed)
                x, nxt = nxt, x
            return x

        def strided(n):  # the first n transitions of the K-step sub-sequence
            nonlocal nxt
            x = x_T.clone()
            for t, t_to in hops[:n]:
                eps = runner(x, ts[t:t + 1])
                sched.ddim_step(x, eps, t, t_to, out=nxt, eta=a.eta, noise='philox', seed=a.seed)
                x, nxt = nxt, x
            return x

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = fn(K)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / K * 1e3, x

        full(a.warmup)
        strided(a.warmup)
        ms = {'full': [], 'strided': []}
        for _ in range(a.rounds):
            for name, fn in (('full', full), ('strided', strided)):
                t, x = timed(fn)
                ms[name].append(round(t, 4))
        finite = bool(torch.isfinite(x).all())

    med = {k: statistics.median(v) for k, v in ms.items()}
    line = {
        'workload': f'{a.size} px UNet, B={a.batch}, philox, HIP graph: {K} DDIM steps (eta={a.eta}) vs the first {K} '
                    f'steps of T={T}',
        'ms_per_step_strided': round(med['strided'], 4), 'ms_per_step_full': round(med['full'], 4),
        'strided_over_full': round(med['strided'] / med['full'], 4), 'rounds_strided': ms['strided'],
        'rounds_full': ms['full'], 'graph_split': runner.split, 'x0_finite': finite,
        'note': 'per-step parity is the only expectation; a 50-step sample costs 50 of these steps, not 1000',
    }
    if a.trace:
        line.update(kernel_means(a.trace))
    print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
