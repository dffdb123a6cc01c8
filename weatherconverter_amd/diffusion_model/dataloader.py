"""Drop-in for the reference's ``diffusion_model/dataloader.py`` (``ACDCDataset``, ``get_loader``) with the
transform chain of ``train_ddpm.py:150-159`` on the GPU.

The reference's workers run ``Resize(S, BILINEAR) -> RandomCrop(S) -> RandomHorizontalFlip -> ToTensor ->
x * 2 - 1`` on the CPU; the resize, Pillow's antialiased two-pass 8-bit resample of a 1920 x 1080 frame, is
the expensive part, and only the crop window's pixels are ever used.  Here a worker only decodes the file,
draws the crop and flip parameters in torchvision's order and cuts out the uint8 source rectangle the crop
window reads; the batch's rectangles go to the device in one pinned copy and ONE ``wc_augment_batch``
launch (``csrc/wc_data.hip``) writes the ``(B, 3, S, S)`` fp32 batch, bit for bit what the reference's chain
gives.  Workers never touch the GPU.

Draw order (torchvision 0.18 ``RandomCrop.get_params`` / ``RandomHorizontalFlip.forward``; torchvision is
not installed, so this order is taken from its source and not pinned by a test against it):
``i = torch.randint(0, H' - S + 1, (1,)).item()`` then ``j = torch.randint(0, W' - S + 1, (1,)).item()``
(no draw at all when ``(W', H') == (S, S)``), then ``flip = torch.rand(1) < 0.5``.
"""
import glob
import os
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from torch.utils import data

from .. import kernels as K


class AugmentParams(NamedTuple):
    """What one image's job needs beside its bytes: the full size, the crop origin in the resized image,
    the flip bit, the source rectangle (x, y, w, h) the item carries and the item's index in the dataset
    (-1 for an image that comes from no dataset)."""
    w: int
    h: int
    crop_x: int
    crop_y: int
    flip: bool
    rect: Tuple[int, int, int, int]
    index: int = -1


def draw_random_crop_flip(out_w: int, out_h: int, S: int) -> Tuple[int, int, bool]:
    """(crop_x, crop_y, flip) drawn from torch's global generator in torchvision's order (module docstring)."""
    if out_w < S or out_h < S:
        raise ValueError(f'Required crop size {(S, S)} is larger than input image size {(out_h, out_w)}')
    if (out_w, out_h) == (S, S):
        i = j = 0
    else:
        i = int(torch.randint(0, out_h - S + 1, size=(1, )).item())
        j = int(torch.randint(0, out_w - S + 1, size=(1, )).item())
    flip = bool(torch.rand(1) < 0.5)
    return j, i, flip


def _open_rgb(path: str):
    from PIL import Image
    return Image.open(path).convert('RGB')


def _cut(image, S: int, crop_x: int, crop_y: int, flip: bool, index: int = -1):
    """(uint8 [rh, rw, 3] contiguous tensor, AugmentParams): the source rectangle the crop window reads."""
    w, h = image.size
    rect = K.augment_window(w, h, S, crop_x, crop_y)
    x, y, rw, rh = rect
    pixels = np.array(image.crop((x, y, x + rw, y + rh)), dtype=np.uint8, order='C')  # a writable copy
    return torch.from_numpy(pixels), AugmentParams(w, h, crop_x, crop_y, flip, rect, index)


class ACDCDataset(data.Dataset):
    """The reference's dataset (``dataloader.py:9-47``) with its glob rules.  An item is
    ``(rectangle, AugmentParams)``: the uint8 source rectangle the drawn crop window reads and its
    parameters; nothing is resized on the CPU.  ``crop='center'`` takes CenterCrop and no flip instead."""

    def __init__(self, root_dir, selected_conditions=('rain', 'fog', 'night'), image_size: int = 128,
                 crop: str = 'random'):
        if crop not in ('random', 'center'):
            raise ValueError("crop must be 'random' or 'center'")
        self.root_dir = str(root_dir)
        self.selected_conditions = list(selected_conditions)
        self.image_size = int(image_size)
        self.crop = crop
        self.img_paths: List[str] = []
        self.preprocess()

    def preprocess(self):
        for condition in self.selected_conditions:  # reference :20-27
            for split in ['train', 'val', 'test']:
                folder_dir = os.path.join(self.root_dir, condition, split)
                pattern = os.path.join(folder_dir, '**', '*.[jp][pn]g')
                self.img_paths.extend(glob.glob(pattern, recursive=True))

    def add_images(self, image_dir):
        for condition in self.selected_conditions:  # reference :29-34
            folder_dir = os.path.join(str(image_dir), condition)
            pattern = os.path.join(folder_dir, '**', '*.[jp][pn]g')
            self.img_paths.extend(glob.glob(pattern, recursive=True))

    def __len__(self):
        return len(self.img_paths)

    def __getitem__(self, idx):
        image = _open_rgb(self.img_paths[idx])
        S = self.image_size
        ow, oh = K.resized_size(*image.size, S)
        if self.crop == 'center':
            if ow < S or oh < S:
                raise ValueError(f'image {image.size} resizes to {(ow, oh)}, smaller than the crop {S}')
            cx, cy = K.center_crop_origin(ow, oh, S)
            flip = False
        else:
            cx, cy, flip = draw_random_crop_flip(ow, oh, S)
        return _cut(image, S, cx, cy, flip, int(idx))


def _collate_list(items):
    return items


class _Slot:
    """Pinned staging and its device copy (grown on demand), and the event of the kernel that last read
    the device copy."""

    def __init__(self):
        self.host = self.dev = self.event = None

    def reserve(self, nbytes: int, device):
        if self.event is not None:
            self.event.synchronize()  # the kernel that read this slot has finished: refill it
        if self.host is None or self.host.numel() < nbytes:
            cap = max(nbytes, 1 << 16) * 5 // 4
            self.host = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
            self.dev = torch.empty(cap, dtype=torch.uint8, device=device)


def _round_up(n: int, m: int) -> int:
    return -(-n // m) * m


def augment_items(items: Sequence, S: int, device, slot: Optional[_Slot] = None) -> torch.Tensor:
    """The ``(B, 3, S, S)`` fp32 batch of a list of ``(rectangle, AugmentParams)`` items on the current
    stream: the job table and the rectangles packed into one pinned buffer, one H2D copy, one launch."""
    device = torch.device(device)
    slot = slot if slot is not None else _Slot()
    B = len(items)
    table_bytes = _round_up(8 * K.AUGMENT_JOB_WORDS * B, 256)
    offsets, total = [], table_bytes
    for rect, _ in items:
        offsets.append(total)
        total += _round_up(rect.numel(), 16)
    slot.reserve(total, device)
    words = []
    with torch.cuda.device(device):
        base = slot.dev.data_ptr()
        for (rect, p), off in zip(items, offsets):
            assert rect.dtype == torch.uint8 and rect.is_contiguous() and tuple(rect.shape) == (p.rect[3], p.rect[2], 3)
            geom = K.augment_geometry(p.w, p.h, S, device)
            words += K.augment_job_words(geom, base + off, 3 * p.rect[2], p.rect, p.crop_x, p.crop_y, p.flip)
            slot.host[off:off + rect.numel()] = rect.reshape(-1)
        host_jobs = slot.host[:8 * K.AUGMENT_JOB_WORDS * B].view(torch.int64).view(B, K.AUGMENT_JOB_WORDS)
        host_jobs.copy_(torch.tensor(words, dtype=torch.int64).view(B, K.AUGMENT_JOB_WORDS))
        slot.dev[:total].copy_(slot.host[:total], non_blocking=True)
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=device)
        K.augment_batch(host_jobs, slot.dev, S, out)
        if slot.event is None:
            slot.event = torch.cuda.Event()
        slot.event.record()
    return out


class AugmentLoader:
    """Iterates ``(B, 3, S, S)`` fp32 device batches over a ``torch.utils.data.DataLoader`` of
    ``ACDCDataset`` items.  ``prefetch=True``: batch k + 1 is uploaded and launched on a side stream while
    the consumer works on batch k (two slots; the consumer's stream waits on the slot's event; a slot is
    refilled only after the kernel that read it has completed).  ``prefetch=False``: the same work on the
    current stream.  Both give the same bits."""

    def __init__(self, loader: data.DataLoader, image_size: int, device, prefetch: bool = True):
        self.loader, self.image_size, self.device, self.prefetch = loader, int(image_size), torch.device(device), prefetch
        self.dataset = loader.dataset
        self._slots = [_Slot(), _Slot()]
        self._stream = None

    def __len__(self):
        return len(self.loader)

    def __iter__(self):
        if not self.prefetch:
            for k, items in enumerate(self.loader):
                yield augment_items(items, self.image_size, self.device, self._slots[k % 2])
            return
        if self._stream is None:
            self._stream = torch.cuda.Stream(self.device)
        side = self._stream

        def launch(k, items):
            with torch.cuda.stream(side):
                out = augment_items(items, self.image_size, self.device, self._slots[k % 2])
            return out, self._slots[k % 2].event

        pending = None
        for k, items in enumerate(self.loader):
            nxt = launch(k, items)
            if pending is not None:
                yield self._hand_over(*pending)
            pending = nxt
        if pending is not None:
            yield self._hand_over(*pending)

    def _hand_over(self, out, event):
        cur = torch.cuda.current_stream(self.device)
        cur.wait_event(event)
        out.record_stream(cur)  # allocated on the side stream, consumed on this one
        return out


def get_loader(image_dir, selected_attrs, image_size=128, batch_size=16, num_workers=4, *, prefetch: bool = True,
               device=None, shuffle: bool = True) -> AugmentLoader:
    """Build and return a data loader (the reference's signature, ``dataloader.py:50``) that yields
    ``(B, 3, image_size, image_size)`` fp32 batches in [-1, 1] on ``device`` (default: the current one)."""
    dataset = ACDCDataset(root_dir=image_dir, selected_conditions=selected_attrs, image_size=image_size)
    print(len(dataset))  # reference :66
    return make_loader(dataset, batch_size, num_workers, prefetch=prefetch, device=device, shuffle=shuffle)


def make_loader(dataset: ACDCDataset, batch_size=16, num_workers=4, *, prefetch: bool = True, device=None,
                shuffle: bool = True) -> AugmentLoader:
    """``get_loader`` over a dataset that already exists (one that ``add_images`` extended)."""
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    loader = data.DataLoader(dataset=dataset, batch_size=batch_size, shuffle=shuffle, num_workers=num_workers,
                             collate_fn=_collate_list)
    return AugmentLoader(loader, dataset.image_size, device, prefetch=prefetch)


def load_image(path, image_size: int, device=None) -> torch.Tensor:
    """``translation.py:131-143``: ``Resize -> CenterCrop -> ToTensor -> x * 2 - 1`` of one image file through
    the same kernel; ``(1, 3, S, S)`` fp32 on ``device``, the input of ``sample_with_sgg``."""
    if device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    image = _open_rgb(str(path))
    S = int(image_size)
    ow, oh = K.resized_size(*image.size, S)
    if ow < S or oh < S:
        raise ValueError(f'image {image.size} resizes to {(ow, oh)}, smaller than the crop {S}')
    cx, cy = K.center_crop_origin(ow, oh, S)
    return augment_items([_cut(image, S, cx, cy, False)], S, device)
