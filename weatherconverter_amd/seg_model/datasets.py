"""Label side of the reference's ``seg_model/datasets/acdc.py`` and ``seg_model/inference.py:56-115``: the
Cityscapes id -> train-id table, the train-id palette, and the label loader of the segmenter.

The reference builds a label map on the CPU (``ExtResize(NEAREST) -> ExtCenterCrop -> encode_target``); here
only the uint8 rectangle the crop window reads is uploaded and ``wc_label_batch`` (``csrc/wc_seg.hip``) writes
the int64 train-id map, bit for bit what the reference's chain gives.

The tables restate the public Cityscapes label definition (cityscapesScripts ``labels.py``): 34 ids 0..33,
of which 19 are evaluated, then the ``license plate`` entry whose id is -1; ``tests/golden/seg_labels.npz``
pins them against the reference's arrays.
"""
from typing import Optional, Tuple

import numpy as np
import torch

from .. import kernels as K

IGNORE = 255

# the 19 evaluated classes in train-id order: (name, Cityscapes id, colour)
_EVALUATED = (
    ('road', 7, (128, 64, 128)),
    ('sidewalk', 8, (244, 35, 232)),
    ('building', 11, (70, 70, 70)),
    ('wall', 12, (102, 102, 156)),
    ('fence', 13, (190, 153, 153)),
    ('pole', 17, (153, 153, 153)),
    ('traffic light', 19, (250, 170, 30)),
    ('traffic sign', 20, (220, 220, 0)),
    ('vegetation', 21, (107, 142, 35)),
    ('terrain', 22, (152, 251, 152)),
    ('sky', 23, (70, 130, 180)),
    ('person', 24, (220, 20, 60)),
    ('rider', 25, (255, 0, 0)),
    ('car', 26, (0, 0, 142)),
    ('truck', 27, (0, 0, 70)),
    ('bus', 28, (0, 60, 100)),
    ('train', 31, (0, 80, 100)),
    ('motorcycle', 32, (0, 0, 230)),
    ('bicycle', 33, (119, 11, 32)),
)
NUM_CLASSES = len(_EVALUATED)
CLASS_NAMES = tuple(name for name, _, _ in _EVALUATED)


def _id_table() -> np.ndarray:
    t = np.full(35, IGNORE, dtype=np.int64)  # ids 0..33, then 'license plate' (id -1): index 34 and index -1
    for train_id, (_, cs_id, _) in enumerate(_EVALUATED):
        t[cs_id] = train_id
    return t


ID_TO_TRAIN_ID = _id_table()
TRAIN_ID_TO_COLOR = np.array([c for _, _, c in _EVALUATED] + [(0, 0, 0)], dtype=np.int64)  # 19 colours, then black
for _a in (ID_TO_TRAIN_ID, TRAIN_ID_TO_COLOR):
    _a.setflags(write=False)


def _lut() -> torch.Tensor:
    """The 256-entry uint8 table of the device path: ids above 34 map to 255 (the host path raises)."""
    t = torch.full((256, ), IGNORE, dtype=torch.uint8)
    t[:35] = torch.from_numpy(ID_TO_TRAIN_ID.astype(np.uint8))
    return t


_LUT = _lut()
_PALETTE = torch.from_numpy(TRAIN_ID_TO_COLOR.astype(np.uint8)).contiguous()


def _device(device) -> torch.device:
    return torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)


def encode_target(target):
    """Cityscapes ids -> train ids (reference ``ACDCDataset.encode_target``).  A numpy array, a PIL image or a
    host tensor is indexed as the reference does (``ID_TO_TRAIN_ID[np.array(target)]``, an ``IndexError`` for
    an id above 34 included) and returns a numpy array.  A DEVICE tensor (uint8, any shape) goes through
    ``wc_label_batch`` and returns an int64 device tensor; there an id above 34 maps to 255 instead of raising
    (no host sync to find out)."""
    if isinstance(target, torch.Tensor) and target.is_cuda:
        K._req(target.dtype == torch.uint8 and target.numel() >= 1, 'encode_target: a device id map is uint8')
        t = target.contiguous()
        h, w = (t.shape[-2], t.shape[-1]) if t.dim() >= 2 else (1, t.numel())
        planes = t.reshape(-1, h, w)
        rows, cols = np.arange(h, dtype=np.int32), np.arange(w, dtype=np.int32)
        out = _label_launch([(planes[b], rows, cols) for b in range(planes.shape[0])], h, w, t.device)
        return out.reshape(t.shape)
    if isinstance(target, torch.Tensor):
        target = target.numpy()
    return ID_TO_TRAIN_ID[np.array(target)]


def decode_target(target):
    """Train ids -> colours (reference ``ACDCDataset.decode_target``).  Unlike the reference, which rewrites
    255 to 19 IN its argument, this never changes ``target``.  Numpy / host input: ``TRAIN_ID_TO_COLOR[t]``
    with 255 taken as 19 (a numpy array back); a uint8 or int64 DEVICE tensor goes through ``wc_seg_decode``
    (uint8 device colours; every value >= 19 or negative is black)."""
    if isinstance(target, torch.Tensor) and target.is_cuda:
        return K.seg_decode(target.contiguous(), _PALETTE)
    if isinstance(target, torch.Tensor):
        target = target.numpy()
    t = np.array(target)  # a copy
    t[t == IGNORE] = NUM_CLASSES
    return TRAIN_ID_TO_COLOR[t]


class LabelWindow:
    """The geometry of one label map: (w, h) resized to (out_w, out_h) by NEAREST, the (crop_w, crop_h) window
    at (crop_x, crop_y) of the resized map.  ``rect`` = (x, y, w, h) is the source rectangle the window reads
    and ``rows`` / ``cols`` the int32 source row / column of every window row / column RELATIVE to it."""

    def __init__(self, w: int, h: int, out_w: int, out_h: int, crop_x: int, crop_y: int, crop_w: int, crop_h: int):
        K._req(crop_w >= 1 and crop_h >= 1 and 0 <= crop_x <= out_w - crop_w and 0 <= crop_y <= out_h - crop_h,
               f'label window {crop_w}x{crop_h} at ({crop_x}, {crop_y}) outside the {out_w}x{out_h} resized map')
        cols = K.nearest_table(w, out_w)[crop_x:crop_x + crop_w]
        rows = K.nearest_table(h, out_h)[crop_y:crop_y + crop_h]
        x0, y0 = int(cols[0]), int(rows[0])  # the tables are monotone
        self.rect = (x0, y0, int(cols[-1]) - x0 + 1, int(rows[-1]) - y0 + 1)
        self.cols = np.ascontiguousarray(cols - x0, dtype=np.int32)
        self.rows = np.ascontiguousarray(rows - y0, dtype=np.int32)
        self.size = (crop_h, crop_w)


def label_window(w: int, h: int, resize: Tuple[int, int], crop: Tuple[int, int]) -> LabelWindow:
    """``Resize((rh, rw), NEAREST)`` of a w x h map, then torchvision's ``center_crop((ch, cw))`` (origin
    ``int(round((rw - cw) / 2.0))``, ``K.center_crop_origin``'s rule).  Host arithmetic only."""
    (rh, rw), (ch, cw) = resize, crop
    K._req(cw <= rw and ch <= rh, f'crop {(ch, cw)} larger than the resized map {(rh, rw)}')
    cx, cy = int(round((rw - cw) / 2.0)), int(round((rh - ch) / 2.0))
    return LabelWindow(w, h, rw, rh, cx, cy, cw, ch)


def _label_launch(jobs, hc: int, wc: int, device, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One wc_label_batch launch: jobs = [(uint8 (rh, rw) rectangle, rows, cols)], host or device rectangles;
    the job table, the tables and the host rectangles go up in one copy.  ``out``: an int64 (B, hc, wc)
    device tensor to write instead of a new one."""
    B = len(jobs)
    table_words = K.LABEL_JOB_WORDS * B
    chunks, off = [], 8 * table_words

    def place(arr: np.ndarray) -> int:
        nonlocal off
        off = -(-off // 16) * 16
        chunks.append((off, arr))
        off += arr.nbytes
        return chunks[-1][0]

    placed = []
    for rect, rows, cols in jobs:
        K._req(rect.dim() == 2 and rect.dtype == torch.uint8 and rows.size == hc and cols.size == wc,
               'label jobs are (uint8 (rh, rw) rectangle, rows[Hc], cols[Wc])')
        rows, cols = np.ascontiguousarray(rows, np.int32), np.ascontiguousarray(cols, np.int32)
        src_off = None if rect.is_cuda else place(np.ascontiguousarray(rect.numpy()).reshape(-1).view(np.uint8))
        placed.append((rect, src_off, place(rows.view(np.uint8)), place(cols.view(np.uint8)), rows, cols))
    host = torch.zeros(off, dtype=torch.uint8)
    hv = host.numpy()
    for o, arr in chunks:
        hv[o:o + arr.nbytes] = arr
    with torch.cuda.device(device):
        dev = torch.empty(off, dtype=torch.uint8, device=device)
        base, hbase = dev.data_ptr(), host.data_ptr()
        words = []
        for rect, src_off, ro, co, rows, cols in placed:
            rect = rect if not rect.is_cuda or rect.stride(1) == 1 else rect.contiguous()
            src, pitch = (base + src_off, rect.shape[1]) if src_off is not None else (rect.data_ptr(), rect.stride(0))
            words += K.label_job_words(src, pitch, rect.shape[1], rect.shape[0], base + ro, base + co, hbase + ro, hbase + co)
        host[:8 * table_words].view(torch.int64).copy_(torch.tensor(words, dtype=torch.int64))
        dev.copy_(host)  # pageable: returns once the bytes are staged, ordered on the current stream
        if out is None:
            out = torch.empty((B, hc, wc), dtype=torch.int64, device=device)
        K._req(tuple(out.shape) == (B, hc, wc), f'label launch: out is ({B}, {hc}, {wc})')
        K.label_batch(host[:8 * table_words].view(torch.int64).view(B, K.LABEL_JOB_WORDS), dev, _LUT, out)
    return out


def _open_label(path):
    from PIL import Image
    image = Image.open(str(path))
    if image.mode != 'L':
        raise ValueError(f'label file {path} has mode {image.mode!r}; a labelIds file is single-channel 8-bit (L)')
    return image


def _load_window(image, win: LabelWindow, device) -> torch.Tensor:
    x, y, rw, rh = win.rect
    pixels = np.array(image.crop((x, y, x + rw, y + rh)), dtype=np.uint8, order='C')
    return _label_launch([(torch.from_numpy(pixels), win.rows, win.cols)], win.size[0], win.size[1], _device(device))


def load_label(path, resize: Tuple[int, int], crop: Tuple[int, int], device=None) -> torch.Tensor:
    """int64 ``(1, ch, cw)`` train-id map on ``device``: bit-equal to ``Image.open(path).resize((w, h),
    Image.NEAREST)`` -> torchvision ``center_crop((ch, cw))`` -> ``encode_target``, for ``resize=(h, w)`` and
    ``crop=(ch, cw)``.  Mode ``L`` files only."""
    image = _open_label(path)
    return _load_window(image, label_window(*image.size, resize, crop), device)


def label_for_window(w: int, h: int, image_size: int, scale: int = 4) -> LabelWindow:
    """The window of ``label_for``: the field of view ``load_image(path, image_size)`` takes of a w x h frame,
    at ``scale`` times its resolution."""
    S = int(scale) * int(image_size)
    ow, oh = K.resized_size(w, h, S)
    K._req(ow >= S and oh >= S, f'a {w}x{h} map resizes to {(ow, oh)}, smaller than the crop {S}')
    cx, cy = K.center_crop_origin(ow, oh, S)
    return LabelWindow(w, h, ow, oh, cx, cy, S, S)


def label_for(path, image_size: int, scale: int = 4, device=None) -> torch.Tensor:
    """The ``gt`` of ``sample_with_sgg`` for the input ``load_image(path_of_the_frame, image_size)``: the
    label file's smaller side resized (NEAREST) to ``scale * image_size`` by ``K.resized_size``'s rule, centre
    crop ``scale * image_size``; int64 ``(1, S, S)``.  (``preprocess`` keeps the reference's own constants,
    which crop a different window than its diffusion input does.)"""
    image = _open_label(path)
    return _load_window(image, label_for_window(*image.size, image_size, scale), device)


RESIZE = (1080 // 2, 1920 // 2)  # reference seg_model/inference.py:77
CROP = (512, 512)  # :78
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)  # :80


def preprocess(ori_img_path: str, img_path: str, gt_label_ids_path: str, gt_color_path: str, verbose=False,
               device=None):
    """reference ``seg_model/inference.py:56-115``: (original image resized and cropped (PIL), input tensor
    (1, 3, H, W) = ToTensor + Normalize of ``img_path`` (``just_label=True`` leaves it unresized), encoded label
    tensor int64 (1, 512, 512) through ``load_label``, colourised ground truth resized and cropped (PIL))."""
    from PIL import Image
    device = _device(device)
    img = Image.open(img_path).convert('RGB')

    def view(im):  # T.Resize((h, w), BILINEAR) -> T.CenterCrop(512) on a PIL image
        im = im.resize((RESIZE[1], RESIZE[0]), Image.BILINEAR)
        cx, cy = int(round((RESIZE[1] - CROP[1]) / 2.0)), int(round((RESIZE[0] - CROP[0]) / 2.0))
        return im.crop((cx, cy, cx + CROP[1], cy + CROP[0]))

    x = torch.from_numpy(np.array(img, dtype=np.uint8)).permute(2, 0, 1).contiguous().to(device)
    x = x.to(torch.float32).div(255)
    mean = torch.tensor(MEAN, dtype=torch.float32, device=device)[:, None, None]
    std = torch.tensor(STD, dtype=torch.float32, device=device)[:, None, None]
    input_tensor = ((x - mean) / std).unsqueeze(0)
    encoded = load_label(gt_label_ids_path, RESIZE, CROP, device)
    if verbose:
        print(f'Input Tensor Shape: {tuple(input_tensor.shape)}')
        print(f'Label Tensor Shape: {tuple(encoded.shape)}')
    return view(Image.open(ori_img_path).convert('RGB')), input_tensor, encoded, view(Image.open(gt_color_path))
