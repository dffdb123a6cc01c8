"""The training input path, measured; prints one JSON line (and writes it to --out).

  python tools/bench_input.py [--batch 32] [--size 256] [--launches 30] [--steps 10] [--warmup 3]
                              [--workers 16] [--loader-workers 12] [--images 1024] [--out profiles/input_path.json]

Three legs, B images of 1920 x 1080 to a size x size crop:
  kernel   wc_augment_batch alone: HIP events around `launches` back-to-back launches after warm-up, on the
           minimal source rectangles of random crop windows already in device memory; achieved bytes/s over
           the rectangle bytes it reads plus the fp32 batch it writes.
  pil      the reference's chain (PIL resize BILINEAR -> crop -> flip -> ToTensor-equivalent -> x*2-1) for the
           same B decoded images with the same windows on `workers` processes (decoding excluded; the pool
           is started and closed before this process touches the GPU).
  train    the training iteration of tools/bench_train.py (its train_iteration, as --optimizer wc --ema wc:
           add_noise, UNet forward with tape, MSE, backward, Adam, EMA, plus the per-batch randn / randint) fed (a) by get_loader over a generated folder of JPEG frames
           (`images` files, so that an epoch has many batches and every worker has one to make) with
           `loader-workers` workers and (b) by batches already in device memory, the same iteration code.
No threshold: nobody has measured this before.
"""
import argparse
import json
import multiprocessing as mp
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
W, H = 1920, 1080


def frame(k: int) -> np.ndarray:
    """A generated 1920 x 1080 frame: smooth gradients plus mild noise (it compresses like a photograph)."""
    r = np.random.RandomState(k)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    base = np.stack([x / W * 255, y / H * 255, ((x + y + 37 * k) % 512) / 2], axis=-1)
    return np.clip(base + r.normal(0, 6, size=base.shape), 0, 255).astype(np.uint8)


def _pil_chain(job):
    from PIL import Image
    pixels, S, ow, oh, cx, cy, flip = job
    img = Image.fromarray(pixels, 'RGB').resize((ow, oh), Image.BILINEAR).crop((cx, cy, cx + S, cy + S))
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    t = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous()
    return (t.float().div(255) * 2.0 - 1.0).numpy()


def pil_leg(frames, windows, S, ow, oh, workers, reps=3):
    jobs = [(f, S, ow, oh, cx, cy, flip) for f, (cx, cy, flip) in zip(frames, windows)]
    with mp.get_context('fork').Pool(workers) as pool:
        pool.map(_pil_chain, jobs)  # warm-up: workers started, Pillow imported
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            outs = pool.map(_pil_chain, jobs, chunksize=max(1, len(jobs) // workers))
            times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    _pil_chain(jobs[0])
    one = time.perf_counter() - t0
    return {'ms_batch': round(min(times) * 1e3, 2), 'ms_batch_all': [round(t * 1e3, 2) for t in times],
            'ms_one_image_one_process': round(one * 1e3, 2), 'processes': workers,
            'pillow': __import__('PIL').__version__}, np.stack(outs)


def kernel_leg(frames, windows, S, launches, warmup, expect):
    from weatherconverter_amd import kernels as K
    dev = torch.device('cuda', 0)
    keep, words, nbytes = [], [], 0
    for f, (cx, cy, flip) in zip(frames, windows):
        rect = K.augment_window(W, H, S, cx, cy)
        x, y, rw, rh = rect
        d = torch.from_numpy(np.ascontiguousarray(f[y:y + rh, x:x + rw])).to(dev)
        keep.append(d)
        nbytes += d.numel()
        words += K.augment_job_words(K.augment_geometry(W, H, S, dev), d.data_ptr(), 3 * rw, rect, cx, cy, flip)
    B = len(frames)
    host = torch.tensor(words, dtype=torch.int64).view(B, K.AUGMENT_JOB_WORDS)
    devj = host.to(dev)
    out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)
    for _ in range(warmup):
        K.augment_batch(host, devj, S, out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        K.augment_batch(host, devj, S, out)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / launches
    moved = nbytes + out.numel() * 4
    return {'ms_launch': round(ms, 4), 'launches': launches, 'warmup': warmup,
            'bytes_read_rectangles': nbytes, 'bytes_written': out.numel() * 4,
            'gb_per_s': round(moved / (ms * 1e-3) / 1e9, 1),
            'equals_pil_bit_for_bit': bool(np.array_equal(out.cpu().numpy(), expect)),
            'source': 'HIP events around the back-to-back launches (host call included), after warm-up'}


def train_leg(args, folder):
    from weatherconverter_amd.diffusion_model.config import model_config
    from weatherconverter_amd.diffusion_model.dataloader import get_loader
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    from weatherconverter_amd.diffusion_model.train_ddpm import make_ema, make_optimizer
    from weatherconverter_amd.synthetic import init_synthetic_
    from tools.bench_train import train_iteration
    dev = torch.device('cuda', 0)
    net = Unet(model_config(args.size))
    init_synthetic_(net, seed=0)
    net = net.to(dev).train()

    class _T:
        lr = 1e-4
    opt, ema = make_optimizer(net, _T), make_ema(net)
    sched = LinearNoiseScheduler(1000, 0.0001, 0.02, device=dev)

    crit = torch.nn.MSELoss()

    def iteration(images):
        noise = torch.randn_like(images)
        t = torch.randint(0, 1000, (images.shape[0], )).to(dev)
        return train_iteration(net, opt, sched, crit, images, noise, t, after_step=ema.update)

    def run(batches, n):
        it = iter(batches)
        for _ in range(args.warmup):
            iteration(next(it))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loss = iteration(next(it))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3, float(loss)

    def forever(loader):
        while True:
            for b in loader:
                yield b

    loader = get_loader(folder, ['fog'], image_size=args.size, batch_size=args.batch, num_workers=args.loader_workers)
    first = iter(loader)
    resident = [next(first).clone() for _ in range(2)]
    del first
    ms_mem, loss_mem = run(forever(resident), args.steps)
    ms_loader, loss_loader = run(forever(loader), args.steps)
    # what the loader alone delivers with nothing consuming the GPU
    it = forever(loader)
    next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        next(it)
    torch.cuda.synchronize()
    ms_alone = (time.perf_counter() - t0) / args.steps * 1e3
    # where a loader-fed batch's host time goes: one worker's share per image (decode, cut), the main process's
    # packing of one batch into the pinned buffer with its upload and launch calls
    from weatherconverter_amd.diffusion_model import dataloader as D
    ds = loader.dataset
    t0 = time.perf_counter()
    opened = [D._open_rgb(ds.img_paths[k]) for k in range(4)]
    t1 = time.perf_counter()
    for im in opened:
        D._cut(im, args.size, 0, 0, False)
    t2 = time.perf_counter()
    items = [ds[k] for k in range(args.batch)]
    D.augment_items(items, args.size, dev)  # warm: staging allocated
    torch.cuda.synchronize()
    slot = D._Slot()
    D.augment_items(items, args.size, dev, slot)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    D.augment_items(items, args.size, dev, slot)
    t4 = time.perf_counter()
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    host = {'ms_decode_per_image': round((t1 - t0) / 4 * 1e3, 2), 'ms_cut_per_image': round((t2 - t1) / 4 * 1e3, 2),
            'ms_pack_upload_launch_calls_per_batch': round((t4 - t3) * 1e3, 2),
            'ms_until_batch_ready': round((t5 - t3) * 1e3, 2),
            'rectangle_mbytes_per_batch': round(sum(r.numel() for r, _ in items) / 1e6, 1)}
    return {'host_breakdown': host, 'ms_iter_in_memory': round(ms_mem, 2), 'ms_iter_loader_fed': round(ms_loader, 2),
            'loader_over_in_memory': round(ms_loader / ms_mem, 4), 'ms_batch_loader_alone': round(ms_alone, 2),
            'steps': args.steps, 'warmup': args.warmup, 'workers': args.loader_workers, 'prefetch': True,
            'folder': f'{args.images} files: {args.batch} generated 1920x1080 JPEG frames (quality 90) and hard links to them',
            'iteration': 'tools/bench_train.py train_iteration: add_noise + UNet forward with tape + MSELoss + backward + optim.Adam + EMA '
                         '(fp32-class), as tools/bench_train.py --optimizer wc --ema wc',
            'loss_finite': bool(np.isfinite(loss_mem) and np.isfinite(loss_loader))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=256)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--workers', type=int, default=16)
    ap.add_argument('--loader-workers', type=int, default=12, help='DataLoader workers of the train leg')
    ap.add_argument('--images', type=int, default=1024, help='files in the generated folder')
    ap.add_argument('--no-train', action='store_true', help='skip the training-iteration leg')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from weatherconverter_amd import kernels as K
    S = args.size
    ow, oh = K.resized_size(W, H, S)
    rng = np.random.RandomState(0)
    frames = [frame(k) for k in range(args.batch)]
    windows = [(int(rng.randint(0, ow - S + 1)), int(rng.randint(0, oh - S + 1)), bool(rng.randint(0, 2)))
               for _ in range(args.batch)]
    pil, expect = pil_leg(frames, windows, S, ow, oh, args.workers)  # before the GPU is touched
    res = {'metric': f'training input: {args.batch} x 1920x1080 -> {S} (resize, crop, flip, normalise)',
           'kernel': None, 'pil': pil, 'train': None}
    folder = None
    if not args.no_train:
        from PIL import Image
        folder = tempfile.mkdtemp(prefix='wc_input_')
        os.makedirs(os.path.join(folder, 'fog', 'train'))
        first = []
        for k in range(args.images):  # B distinct files, the rest hard links to them: many batches per epoch
            path = os.path.join(folder, 'fog', 'train', f'{k:05d}.jpg')
            if k < len(frames):
                Image.fromarray(frames[k], 'RGB').save(path, quality=90)
                first.append(path)
            else:
                os.link(first[k % len(first)], path)
    res['kernel'] = kernel_leg(frames, windows, S, args.launches, args.warmup, expect)
    res['kernel_speedup_over_pil_batch'] = round(pil['ms_batch'] / res['kernel']['ms_launch'], 1)
    res['device'] = torch.cuda.get_device_name(0)
    if folder is not None:
        res['train'] = train_leg(args, folder)
        import shutil
        shutil.rmtree(folder, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
