"""A numpy restatement of the reference loader's transform chain, written from the specification alone
(Pillow's BILINEAR ``Image.resize`` in 8-bit fixed point, torchvision's Resize / crop / flip rules, ToTensor
and ``x * 2 - 1``), shared by tests/test_data_cpu.py and tests/test_gpu_data.py.  Plain loops, one output
index at a time: nothing here is shared with weatherconverter_amd.kernels.resample_axis."""
import math

import numpy as np

PRECISION_BITS = 22


def resized_size(w, h, S):
    return (S, int(S * h / w)) if w <= h else (int(S * w / h), S)


def center_crop_origin(w, h, S):
    return int(round((w - S) / 2.0)), int(round((h - S) / 2.0))


def coefficients(in_size, out_size):
    """(bounds [(xmin, n)], coefs [[k]], ksize) of one axis."""
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds, coefs = [], []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        n = xmax - xmin
        w, ww = [], 0.0
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * (1.0 / fs))
            v = 1.0 - a if a < 1.0 else 0.0
            w.append(v)
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds.append((xmin, n))
        coefs.append([int(0.5 + v * (1 << PRECISION_BITS)) for v in w] + [0] * (ksize - n))
    return bounds, coefs, ksize


def one_pass(pixels, bounds, coefs):
    """Resample axis 0 of uint8 [in, ...] -> uint8 [out, ...]."""
    src = pixels.astype(np.int64)
    out = np.empty((len(bounds), ) + pixels.shape[1:], dtype=np.uint8)
    for xx, (xmin, n) in enumerate(bounds):
        acc = np.full(pixels.shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for x in range(n):
            acc = acc + src[xmin + x] * coefs[xx][x]
        assert acc.max() < 2**31  # the kernel's int32 cannot overflow
        out[xx] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize(image, out_w, out_h):
    """uint8 [h, w, 3] -> uint8 [out_h, out_w, 3]: the horizontal pass, then the vertical pass on its bytes."""
    h, w, _ = image.shape
    hb, hc, _ = coefficients(w, out_w)
    vb, vc, _ = coefficients(h, out_h)
    tmp = one_pass(np.ascontiguousarray(image.transpose(1, 0, 2)), hb, hc).transpose(1, 0, 2)
    return one_pass(np.ascontiguousarray(tmp), vb, vc)


def normalise(u8):
    """uint8 [S, S, 3] -> float32 [3, S, S] = fl(fl(u / 255) * 2 - 1)."""
    x = u8.astype(np.float32) / np.float32(255.0)
    x = x * np.float32(2.0) - np.float32(1.0)
    return np.ascontiguousarray(x.transpose(2, 0, 1)).astype(np.float32)


def transform(image, S, crop_x, crop_y, flip):
    """The whole chain for one uint8 [h, w, 3] image: float32 [3, S, S]."""
    h, w, _ = image.shape
    ow, oh = resized_size(w, h, S)
    r = resize(image, ow, oh)[crop_y:crop_y + S, crop_x:crop_x + S]
    if flip:
        r = r[:, ::-1]
    return normalise(r)


# ------------------------------------------------------------------ the golden cases (tests/golden/augment.npz)
# (w, h, S): the ACDC ratio at 4.2x, portrait with ksize 29, upscaling, one identity axis, a no-op, one spare column
GOLDEN_SOURCES = [(270, 152, 36), (333, 500, 24), (40, 30, 64), (96, 64, 64), (64, 64, 64), (17, 16, 16)]
GOLDEN_KINDS = ('noise', 'checker')


def golden_source(kind, w, h):
    """The generated uint8 [h, w, 3] source: seeded noise (numpy's legacy MT19937 stream, fixed across
    versions), or a 0/255 checkerboard whose horizontal period differs per channel.  The golden file keeps
    each source's CRC-32, not its bytes (333 x 500 noise alone is 500 KB)."""
    if kind == 'noise':
        return np.random.RandomState(1000 * w + h).randint(0, 256, size=(h, w, 3), dtype=np.uint8)
    y, x, c = np.meshgrid(np.arange(h), np.arange(w), np.arange(3), indexing='ij')
    return ((((x // (c + 1)) + y) % 2) * 255).astype(np.uint8)


def golden_crops(w, h, S):
    """The crop origins every source is tested at: (0, 0), the maximal offset and one interior offset."""
    ow, oh = resized_size(w, h, S)
    mx, my = ow - S, oh - S
    return sorted({(0, 0), (mx, my), (mx // 2, my // 2)})


def golden_cases():
    """(key, kind, w, h, S, crop_x, crop_y, flip) of every case."""
    out = []
    for w, h, S in GOLDEN_SOURCES:
        for kind in GOLDEN_KINDS:
            for cx, cy in golden_crops(w, h, S):
                for flip in (False, True):
                    out.append((f'{kind}_{w}x{h}_{S}', kind, w, h, S, cx, cy, flip))
    return out
