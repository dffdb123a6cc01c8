"""The streaming segmentation metric, measured; prints one JSON line per case (and writes them to --out).

  python tools/bench_seg_metrics.py [--size 1024] [--classes 19] [--launches 20] [--windows 7] [--warmup 3]
                                    [--out profiles/seg_metrics.json]

Cases: logits (B, 19, 1024, 1024) fp32 with B = 1 and 8 and label maps made of a few large constant regions
plus 5 % ignore (what a label file looks like: whole waves hit one counter), and B = 8 with i.i.d. labels, the
contention-free extreme.  Per case three ways of adding one batch to the confusion matrix, in this process:
  fused      StreamSegMetrics.update(labels, logits): one wc_seg_confusion launch (argmax fused; also timed
             with the uint8 prediction written)
  torch      all on the device: logits.argmax(1), then torch.bincount over the masked C * label + pred
  reference  the reference's path: logits.argmax(1).cpu().numpy(), then np.bincount per image
fused and torch are timed with HIP events around `launches` back-to-back updates, `windows` windows each,
alternating between the two, after `warmup` updates of each; a window's figure is ms per update.  Reported: the
median window, the algorithmic bytes (4 C + 8) B H W (+ B H W with the prediction), achieved GB/s and its
fraction of 8 TB/s, and the run-to-run spread of the torch windows, (max - min) / median.
The condition is relative: fused must not be slower than torch by more than that spread on any case (the
fused kernel's traffic is a strict subset of the torch path's); the exit status is 1 where it is.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_BYTES_PER_S = 8e12  # MI355X HBM3E


def region_labels(B, S, C, seed):
    """A few large constant regions (rectangles over a constant background) plus 5 % ignore pixels."""
    rng = np.random.default_rng(seed)
    lab = np.empty((B, S, S), dtype=np.int64)
    for b in range(B):
        lab[b] = rng.integers(0, C)
        for _ in range(6):
            y0, x0 = rng.integers(0, S - S // 8, size=2)
            h, w = rng.integers(S // 8, S // 2, size=2)
            lab[b, y0:y0 + h, x0:x0 + w] = rng.integers(0, C)
    lab[rng.random((B, S, S)) < 0.05] = 255
    return torch.from_numpy(lab)


def torch_update(hist, labels, logits, C):
    pred = logits.argmax(1)
    mask = (labels >= 0) & (labels < C)
    hist += torch.bincount(C * labels[mask] + pred[mask], minlength=C * C).view(C, C)


def reference_update(hist, labels_np, logits, C):
    pred = logits.argmax(1).cpu().numpy()
    for lt, lp in zip(labels_np, pred):
        lt, lp = lt.reshape(-1), lp.reshape(-1)
        mask = (lt >= 0) & (lt < C)
        hist += np.bincount(C * lt[mask].astype(int) + lp[mask], minlength=C * C).reshape(C, C)


def window(fn, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / launches


def run_case(name, B, S, C, labels, args):
    from weatherconverter_amd.seg_model.metrics import StreamSegMetrics
    dev = torch.device('cuda', 0)
    g = torch.Generator(device=dev).manual_seed(B)
    logits = torch.randn((B, C, S, S), generator=g, device=dev)
    labels = labels.to(dev)
    labels_np = labels.cpu().numpy()
    m = StreamSegMetrics(C, dev)
    pred = torch.empty((B, S, S), dtype=torch.uint8, device=dev)
    th = torch.zeros((C, C), dtype=torch.int64, device=dev)
    legs = {'fused': lambda: m.update(labels, logits),
            'fused_with_pred': lambda: m.update(labels, logits, pred_out=pred),
            'torch': lambda: torch_update(th, labels, logits, C)}
    # the three ways count the same matrix
    m.reset()
    legs['fused']()
    legs['torch']()
    rh = np.zeros((C, C), dtype=np.int64)
    reference_update(rh, labels_np, logits, C)
    same = bool(np.array_equal(m.hist.cpu().numpy(), rh) and np.array_equal(th.cpu().numpy(), rh))
    for fn in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.windows):  # alternating: every leg sees the same drift
        for k, fn in legs.items():
            ms[k].append(window(fn, args.launches))
    ref = []
    for _ in range(3):
        t0 = time.perf_counter()
        reference_update(rh, labels_np, logits, C)
        ref.append((time.perf_counter() - t0) * 1e3)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = (max(ms['torch']) - min(ms['torch'])) / med['torch']
    nbytes = (4 * C + 8) * B * S * S
    out = {'case': name, 'B': B, 'C': C, 'H': S, 'W': S, 'launches': args.launches, 'windows': args.windows,
           'counts_equal_reference': same,
           'fused_ms': round(med['fused'], 4), 'fused_ms_windows': [round(v, 4) for v in ms['fused']],
           'algorithmic_bytes': nbytes, 'fused_gb_per_s': round(nbytes / med['fused'] / 1e6, 1),
           'fused_fraction_of_8TBps': round(nbytes / (med['fused'] * 1e-3) / PEAK_BYTES_PER_S, 4),
           'fused_with_pred_ms': round(med['fused_with_pred'], 4),
           'fused_with_pred_gb_per_s': round((nbytes + B * S * S) / med['fused_with_pred'] / 1e6, 1),
           'torch_ms': round(med['torch'], 4), 'torch_ms_windows': [round(v, 4) for v in ms['torch']],
           'torch_spread': round(spread, 4), 'reference_ms': round(min(ref), 2), 'reference_ms_all': [round(v, 2) for v in ref],
           'fused_not_slower_than_torch': bool(med['fused'] <= med['torch'] * (1 + spread)),
           'source': 'HIP events around back-to-back updates (host calls included), median window after warm-up'}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=1024)
    ap.add_argument('--classes', type=int, default=19)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_seg_metrics: needs a GPU (there is no CPU path to time)')
    S, C = args.size, args.classes
    g = torch.Generator().manual_seed(0)
    iid = torch.randint(0, C, (8, S, S), generator=g)
    cases = [('regions_B1', 1, region_labels(1, S, C, 1)), ('regions_B8', 8, region_labels(8, S, C, 2)),
             ('iid_B8', 8, iid)]
    results = [run_case(name, B, S, C, labels, args) for name, B, labels in cases]
    if args.out:
        with open(args.out, 'w') as fh:
            for r in results:
                fh.write(json.dumps(r) + '\n')
    sys.exit(0 if all(r['fused_not_slower_than_torch'] and r['counts_equal_reference'] for r in results) else 1)


if __name__ == '__main__':
    main()
