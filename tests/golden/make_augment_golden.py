"""Writes tests/golden/augment.npz: what the reference loader's transform chain gives for the generated
sources of tests/resample_ref.py, made with Pillow and torch ops only (never with the code under test).

    python tests/golden/make_augment_golden.py        (needs Pillow; torchvision is not used)

Per source `<kind>_<w>x<h>_<S>`:
  `<key>/crc`   CRC-32 of the generated source's bytes (the tests regenerate the source and compare);
  `<key>/full`  float32 [3, H', W'] = ToTensor and x * 2 - 1 (torch ops) of Pillow's
                Image.resize((W', H'), BILINEAR) with (W', H') from torchvision's Resize(S) rule.
A case's expectation is `full[:, cy:cy+S, cx:cx+S]`, flipped along W when the flip bit is set: crop, flip
and the elementwise normalisation commute exactly, and this script asserts, for every case the tests run,
that the literal chain (PIL resize -> PIL crop -> PIL FLIP_LEFT_RIGHT -> ToTensor -> x * 2 - 1) has those
bits.  `load_image/...` is the Resize -> CenterCrop chain of translation.py:136-143 for one source.
"""
import os
import sys
import zlib

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import resample_ref as R  # noqa: E402


def to_tensor_pm1(img):
    """torchvision's ToTensor on a PIL RGB image, then the loader's Lambda x * 2.0 - 1.0."""
    u = torch.from_numpy(np.asarray(img, dtype=np.uint8).copy()).permute(2, 0, 1).contiguous()
    return u.to(torch.float32).div(255) * 2.0 - 1.0


def main():
    out = {}
    table = torch.arange(256, dtype=torch.uint8).float().div(255) * 2.0 - 1.0
    out['table'] = table.numpy()
    for key, kind, w, h, S, cx, cy, flip in R.golden_cases():
        src = R.golden_source(kind, w, h)
        img = Image.fromarray(src, 'RGB')
        ow, oh = R.resized_size(w, h, S)
        resized = img.resize((ow, oh), Image.BILINEAR)
        if key + '/full' not in out:
            out[key + '/crc'] = np.array(zlib.crc32(src.tobytes()), dtype=np.int64)
            out[key + '/full'] = to_tensor_pm1(resized).numpy()
        piece = resized.crop((cx, cy, cx + S, cy + S))
        if flip:
            piece = piece.transpose(Image.FLIP_LEFT_RIGHT)
        want = to_tensor_pm1(piece)
        got = torch.from_numpy(out[key + '/full'])[:, cy:cy + S, cx:cx + S]
        got = got.flip(-1) if flip else got
        assert torch.equal(want, got), (key, cx, cy, flip)
    # translation.py:136-143 on the ACDC-ratio noise source: Resize -> CenterCrop -> ToTensor -> x * 2 - 1
    w, h, S = R.GOLDEN_SOURCES[0]
    img = Image.fromarray(R.golden_source('noise', w, h), 'RGB')
    ow, oh = R.resized_size(w, h, S)
    left, top = R.center_crop_origin(ow, oh, S)
    piece = img.resize((ow, oh), Image.BILINEAR).crop((left, top, left + S, top + S))
    out['load_image/out'] = to_tensor_pm1(piece).numpy()[None]
    out['load_image/origin'] = np.array([left, top], dtype=np.int64)
    path = os.path.join(HERE, 'augment.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(R.golden_cases()), 'cases')


if __name__ == '__main__':
    main()
