"""CPU: the training-input C ABI as read from include/wc_data.h, the host coefficient tables against a numpy
restatement of Pillow's resample (and, where Pillow imports, the restatement against Pillow itself), the
resized-size / centre-crop rules, the dataset's glob rules and draw order, and the rejections
wc_augment_batch makes before any HIP call."""
import ctypes
import os
import zlib

import numpy as np
import pytest
import torch

import resample_ref as R
from conftest import GOLDEN, ROOT
from weatherconverter_amd import _abi, _native
from weatherconverter_amd import kernels as K


def _header(name):
    return _abi.read(open(os.path.join(ROOT, 'include', name)).read())


# --------------------------------------------------------------------------------------- the ABI
def test_header_declares_the_entry_points_and_the_job():
    abi = _header('wc_data.h')
    assert list(abi.functions) == ['wc_augment_batch', 'wc_resample_span'] and list(abi.structs) == ['wc_augment_job']
    P, I, L = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    J = ctypes.POINTER(_native.AugmentJob)
    assert _native.AugmentJob is _native.DATA_ABI.structs['wc_augment_job']
    assert _native.DATA_ABI.functions['wc_augment_batch'] == (I, [J, J, I, I, P, P])
    assert _native.DATA_ABI.functions['wc_resample_span'] == (I, [L, L, L, L, P, P])
    job = abi.structs['wc_augment_job']
    assert [n for n, _ in job._fields_] == [
        'src', 'pitch', 'rect_x', 'rect_y', 'rect_w', 'rect_h', 'img_w', 'img_h', 'out_w', 'out_h', 'hbounds', 'hcoefs',
        'vbounds', 'vcoefs', 'ksize_h', 'ksize_v', 'crop_x', 'crop_y', 'flip']
    # rows are written as int64 words: 8-byte fields only
    assert all(ctypes.sizeof(t) == 8 for _, t in job._fields_) and ctypes.sizeof(job) == 8 * 19
    assert K.AUGMENT_JOB_WORDS == 19


def test_registered_beside_the_main_header_not_in_it():
    from weatherconverter_amd import _build
    assert 'wc_data.hip' in _build.SOURCES and 'wc_data.h' in _build.ABI_HEADERS
    assert os.path.exists(os.path.join(_build.CSRC, 'wc_data.hip'))
    assert _native.EXPORTS == list(_header('wc_kernels.h').functions) and len(_native.EXPORTS) == 88
    others = [_native.ABI, _native.OPTIM_ABI, _native.EMA_ABI, _native.SAMPLER_ABI]
    for name in _native.DATA_ABI.functions:
        assert name not in _native.EXPORTS and not any(name in o.functions for o in others)
        assert _native._SIGNATURES[name] is _native.DATA_ABI.functions[name]
    assert not any('wc_augment_job' in o.structs for o in others)


# --------------------------------------------------------------------------------------- the arithmetic
AXES = [(270, 64), (152, 36), (333, 24), (500, 36), (40, 85), (30, 64), (96, 96), (64, 64), (17, 17), (16, 16),
        (1920, 113), (1080, 64), (1920, 455), (1080, 256), (1920, 227), (1080, 128), (7, 3), (3, 7), (1, 1), (5, 1)]


@pytest.mark.parametrize('in_size,out_size', AXES)
def test_host_tables_equal_the_restatement(in_size, out_size):
    bounds, coefs, ksize = R.coefficients(in_size, out_size)
    kb, kc, kk = K.resample_axis(in_size, out_size)
    assert kk == ksize and ksize >= 3 and ksize % 2 == 1
    assert kb.dtype == np.int32 and kc.dtype == np.int32 and kb.shape == (out_size, 2) and kc.shape == (out_size, ksize)
    assert np.array_equal(kb, np.array(bounds)) and np.array_equal(kc, np.array(coefs))
    # what the kernel relies on: windows inside the axis, monotone bounds, int32 accumulation
    assert (kb[:, 0] >= 0).all() and (kb[:, 0] + kb[:, 1] <= in_size).all() and (kb[:, 1] >= 1).all()
    assert (np.diff(kb[:, 0]) >= 0).all() and (np.diff(kb[:, 0] + kb[:, 1]) >= 0).all()
    assert (kc >= 0).all() and 255 * int(kc.sum(axis=1).max()) + (1 << 21) < 2**31


def test_known_ksizes():
    assert K.resample_axis(333, 24)[2] == 29 and K.resample_axis(1920, 113)[2] == 35
    assert K.resample_axis(40, 85)[2] == 3 and K.resample_axis(64, 64)[2] == 3


def test_an_axis_that_keeps_its_size_is_the_identity():
    b, c, _ = K.resample_axis(64, 64)
    x = np.random.RandomState(0).randint(0, 256, size=(64, 5), dtype=np.uint8)
    assert np.array_equal(R.one_pass(x, [tuple(r) for r in b], c.tolist()), x)


def test_golden_is_the_restatements_chain_of_the_regenerated_sources():
    """Needs no Pillow: the sources regenerate to the recorded CRC-32s, and the committed Pillow results are
    what the restatement computes."""
    g = np.load(os.path.join(GOLDEN, 'augment.npz'))
    for w, h, S in R.GOLDEN_SOURCES:
        ow, oh = R.resized_size(w, h, S)
        for kind in R.GOLDEN_KINDS:
            src = R.golden_source(kind, w, h)
            assert zlib.crc32(src.tobytes()) == int(g[f'{kind}_{w}x{h}_{S}/crc'])
            assert np.array_equal(R.normalise(R.resize(src, ow, oh)), g[f'{kind}_{w}x{h}_{S}/full'])


def test_restatement_equals_pillow_on_the_golden_sources():
    Image = pytest.importorskip('PIL.Image')
    for w, h, S in R.GOLDEN_SOURCES:
        ow, oh = R.resized_size(w, h, S)
        for kind in R.GOLDEN_KINDS:
            src = R.golden_source(kind, w, h)
            assert np.array_equal(R.resize(src, ow, oh),
                                  np.asarray(Image.fromarray(src, 'RGB').resize((ow, oh), Image.BILINEAR)))


def test_golden_table_is_the_fp32_normalisation():
    g = np.load(os.path.join(GOLDEN, 'augment.npz'))
    table = torch.arange(256, dtype=torch.uint8).float().div(255) * 2.0 - 1.0
    assert np.array_equal(g['table'], table.numpy())
    u = np.arange(256, dtype=np.float32)
    assert np.array_equal(g['table'], u / np.float32(255) * np.float32(2) - np.float32(1))
    assert os.path.getsize(os.path.join(GOLDEN, 'augment.npz')) < 300 * 1024


def test_resized_size_and_centre_crop_rules():
    # torchvision Resize(int): the short edge becomes S, the long one int(S * long / short)
    assert K.resized_size(1920, 1080, 256) == (455, 256) and K.resized_size(1920, 1080, 128) == (227, 128)
    assert K.resized_size(1080, 1920, 256) == (256, 455) and K.resized_size(333, 500, 24) == (24, 36)
    assert K.resized_size(40, 30, 64) == (85, 64) and K.resized_size(17, 16, 16) == (17, 16)
    assert K.resized_size(64, 64, 64) == (64, 64) and K.resized_size(1921, 1081, 37) == (65, 37)
    for w, h, S in [(1920, 1080, 256), (333, 500, 24), (1921, 1081, 37), (7, 5, 3), (5, 7, 3)]:
        assert K.resized_size(w, h, S) == R.resized_size(w, h, S)
    # CenterCrop: Python's round (half to even) of the half difference
    assert K.center_crop_origin(455, 256, 256) == (100, 0)   # 99.5 -> 100
    assert K.center_crop_origin(85, 64, 64) == (10, 0)       # 10.5 -> 10
    assert K.center_crop_origin(17, 16, 16) == (0, 0)        # 0.5 -> 0
    assert K.center_crop_origin(19, 16, 16) == (2, 0)        # 1.5 -> 2
    assert K.center_crop_origin(24, 36, 24) == (0, 6) and K.center_crop_origin(64, 64, 64) == (0, 0)


def test_window_is_what_the_bounds_read():
    for w, h, S in R.GOLDEN_SOURCES:
        ow, oh = R.resized_size(w, h, S)
        hb, _, _ = R.coefficients(w, ow)
        vb, _, _ = R.coefficients(h, oh)
        for cx, cy in R.golden_crops(w, h, S):
            x0 = min(b[0] for b in hb[cx:cx + S])
            x1 = max(b[0] + b[1] for b in hb[cx:cx + S])
            y0 = min(b[0] for b in vb[cy:cy + S])
            y1 = max(b[0] + b[1] for b in vb[cy:cy + S])
            assert K.augment_window(w, h, S, cx, cy) == (x0, y0, x1 - x0, y1 - y0)
    with pytest.raises(RuntimeError):
        K.augment_window(40, 30, 64, 22, 0)  # the resized image is 85 wide: 21 is the last origin


# --------------------------------------------------------------------------------------- the dataset
def _png(path, w, h, seed):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.random.RandomState(seed).randint(0, 256, size=(h, w, 3), dtype=np.uint8), 'RGB').save(path)


def test_dataset_globs_as_the_reference_does(tmp_path):
    pytest.importorskip('PIL.Image')
    from weatherconverter_amd.diffusion_model.dataloader import ACDCDataset
    root = str(tmp_path / 'acdc')
    keep = ['fog/train/a/1.png', 'fog/val/2.jpg', 'fog/test/deep/er/3.png', 'rain/train/4.png']
    drop = ['night/train/5.png', 'fog/other/6.png', 'fog/train/7.bmp', 'fog/8.png', 'fog/train/9.jpeg']
    for k, rel in enumerate(keep + drop):
        _png(os.path.join(root, rel), 8, 6, k)
    ds = ACDCDataset(root, ['fog', 'rain'], image_size=4)
    assert sorted(os.path.relpath(p, root) for p in ds.img_paths) == sorted(keep) and len(ds) == 4
    extra = str(tmp_path / 'bdd')
    for k, rel in enumerate(['fog/x/10.png', 'rain/11.jpg', 'night/12.png', 'train/13.png']):
        _png(os.path.join(extra, rel), 8, 6, 20 + k)
    ds.add_images(extra)  # <dir>/<condition>/**, without the split level
    assert sorted(os.path.relpath(p, extra) for p in ds.img_paths[4:]) == ['fog/x/10.png', 'rain/11.jpg'] and len(ds) == 6
    with pytest.raises(ValueError):
        ACDCDataset(root, ['fog'], image_size=4, crop='bottom')


def test_item_is_the_source_rectangle_of_the_drawn_window(tmp_path):
    pytest.importorskip('PIL.Image')
    from weatherconverter_amd.diffusion_model.dataloader import ACDCDataset, AugmentParams
    root = str(tmp_path)
    _png(os.path.join(root, 'fog/train/a.png'), 61, 23, 3)
    src = np.random.RandomState(3).randint(0, 256, size=(23, 61, 3), dtype=np.uint8)
    ds = ACDCDataset(root, ['fog'], image_size=8)
    S, (ow, oh) = 8, R.resized_size(61, 23, 8)
    assert (ow, oh) == (21, 8)
    # the documented draw order: i (rows; skipped... never here: 21 x 8 != 8 x 8), j (columns), then the flip
    torch.manual_seed(11)
    i = int(torch.randint(0, oh - S + 1, size=(1, )).item())
    j = int(torch.randint(0, ow - S + 1, size=(1, )).item())
    flip = bool(torch.rand(1) < 0.5)
    after = torch.rand(1)
    torch.manual_seed(11)
    rect, p = ds[0]
    assert torch.equal(torch.rand(1), after)  # exactly those three draws were made
    assert isinstance(p, AugmentParams) and (p.w, p.h, p.crop_x, p.crop_y, p.flip) == (61, 23, j, i, flip)
    x, y, rw, rh = K.augment_window(61, 23, S, j, i)
    assert p.rect == (x, y, rw, rh) and rect.dtype == torch.uint8 and rect.is_contiguous() and not rect.is_cuda
    assert tuple(rect.shape) == (rh, rw, 3) and np.array_equal(rect.numpy(), src[y:y + rh, x:x + rw])
    assert rw < 61  # nothing but the window's columns travels
    # over many seeds both offsets and both flip values occur
    seen = set()
    for s in range(40):
        torch.manual_seed(s)
        q = ds[0][1]
        assert 0 <= q.crop_x <= ow - S and q.crop_y == 0
        seen.add((q.crop_x in (0, ow - S), q.flip))
    assert {f for _, f in seen} == {False, True}


def test_equal_sizes_draw_no_crop_and_centre_draws_nothing(tmp_path):
    pytest.importorskip('PIL.Image')
    from weatherconverter_amd.diffusion_model.dataloader import ACDCDataset, draw_random_crop_flip
    root = str(tmp_path)
    _png(os.path.join(root, 'fog/train/a.png'), 12, 12, 5)
    torch.manual_seed(4)
    flip = bool(torch.rand(1) < 0.5)  # the flip is the only draw when (W', H') == (S, S)
    torch.manual_seed(4)
    assert draw_random_crop_flip(8, 8, 8) == (0, 0, flip)
    torch.manual_seed(4)
    p = ACDCDataset(root, ['fog'], image_size=8)[0][1]
    assert (p.crop_x, p.crop_y, p.flip, p.rect) == (0, 0, flip, (0, 0, 12, 12))
    _png(os.path.join(root, 'rain/train/b.png'), 40, 30, 6)
    torch.manual_seed(4)
    before = torch.rand(1)
    torch.manual_seed(4)
    p = ACDCDataset(root, ['rain'], image_size=64, crop='center')[0][1]
    assert torch.equal(torch.rand(1), before)  # CenterCrop and no flip: no draw at all
    assert (p.crop_x, p.crop_y, p.flip) == (10, 0, False)
    with pytest.raises(ValueError):
        draw_random_crop_flip(7, 8, 8)


# --------------------------------------------------------------------------------------- rejections
@pytest.fixture(scope='module')
def lib():
    from weatherconverter_amd import _build
    if not os.path.exists(_build.LIB_PATH):
        if not os.path.exists(_build.HIPCC):
            pytest.skip('hipcc not available to build the library')
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name, (res, args) in _native.DATA_ABI.functions.items():
        assert hasattr(lib, name), name
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def _job(**over):
    """A valid job for a 40 x 30 image to S = 64 (resized 85 x 64), whole image uploaded; the pointers are
    host addresses that are never dereferenced."""
    f = dict(src=64, pitch=120, rect_x=0, rect_y=0, rect_w=40, rect_h=30, img_w=40, img_h=30, out_w=85, out_h=64,
             hbounds=64, hcoefs=64, vbounds=64, vcoefs=64, ksize_h=3, ksize_v=3, crop_x=10, crop_y=0, flip=0)
    f.update(over)
    return _native.AugmentJob(**f)


def test_rejections_come_before_any_launch(lib):
    """Every call here returns from the host checks: no HIP call is made, so no GPU is needed."""
    E_ARG, E_SHAPE = _native.E_ARG, _native.E_SHAPE
    good = ctypes.pointer(_job())
    null = ctypes.POINTER(_native.AugmentJob)()
    out = 4096  # 16-byte aligned, never written
    assert lib.wc_augment_batch(null, good, 1, 64, out, None) == E_ARG
    assert lib.wc_augment_batch(good, null, 1, 64, out, None) == E_ARG
    assert lib.wc_augment_batch(good, good, 1, 64, None, None) == E_ARG
    assert lib.wc_augment_batch(good, good, 0, 64, out, None) == E_ARG
    assert lib.wc_augment_batch(good, good, -2, 64, out, None) == E_ARG
    assert lib.wc_augment_batch(good, good, 1, 64, out + 4, None) == E_ARG  # misaligned out
    for S in (0, 2, 3, -4):
        assert lib.wc_augment_batch(good, good, 1, S, out, None) == E_SHAPE
    for S in (6, 30, 63):  # not a multiple of 4
        assert lib.wc_augment_batch(good, good, 1, S, out, None) == E_SHAPE

    def one(**over):
        j = ctypes.pointer(_job(**over))
        return lib.wc_augment_batch(j, good, 1, 64, out, None)
    for name in ('src', 'hbounds', 'hcoefs', 'vbounds', 'vcoefs'):
        assert one(**{name: 0}) == E_ARG
    for bad in (dict(ksize_h=1), dict(ksize_v=1), dict(ksize_h=4), dict(ksize_v=2), dict(ksize_h=-3),
                dict(ksize_h=5), dict(ksize_v=5)):  # < 3, even, or not the geometry's
        assert one(**bad) == E_SHAPE
    for bad in (dict(crop_x=22), dict(crop_x=-1), dict(crop_y=1), dict(flip=2), dict(out_w=60), dict(img_w=0),
                dict(pitch=119), dict(rect_w=41), dict(rect_x=1), dict(rect_h=0)):
        assert one(**bad) == E_SHAPE
    # the window at crop_x = 10 reads source columns [4, 36): a rectangle must cover them
    x0, y0, rw, rh = K.augment_window(40, 30, 64, 10, 0)
    assert (x0, y0, rw, rh) == (4, 0, 32, 30)
    assert one(rect_x=5, rect_w=31, pitch=93) == E_SHAPE
    assert one(rect_x=4, rect_w=31, pitch=93) == E_SHAPE
    assert one(rect_y=1, rect_h=29) == E_SHAPE
    # a second row is checked like the first
    rows = (_native.AugmentJob * 2)(_job(), _job(ksize_h=2))
    assert lib.wc_augment_batch(rows, good, 2, 64, out, None) == E_SHAPE
    # S = 16000 makes an LDS row 48000 bytes and one output row reads two source rows: not even a band of one
    # row fits a workgroup's LDS, and there is no CPU path
    big = dict(img_w=16000, img_h=16000, out_w=16000, out_h=16000, rect_w=16000, rect_h=16000, pitch=48000,
               crop_x=0, crop_y=0)
    j = ctypes.pointer(_job(**big))
    assert lib.wc_augment_batch(j, good, 1, 16000, out, None) == E_SHAPE
    assert E_ARG != E_SHAPE and _native.OK == 0


def test_resample_span_is_the_tables_span(lib):
    first, count = ctypes.c_int64(), ctypes.c_int64()
    for in_size, out_size in AXES:
        b = K.resample_axis(in_size, out_size)[0]
        for o0, o1 in {(0, out_size), (0, 1), (out_size - 1, out_size), (out_size // 3, out_size // 3 + max(1, out_size // 2))}:
            o1 = min(o1, out_size)
            assert lib.wc_resample_span(in_size, out_size, o0, o1, ctypes.byref(first), ctypes.byref(count)) == 0
            assert first.value == b[o0, 0] and first.value + count.value == b[o1 - 1].sum()
    assert lib.wc_resample_span(0, 4, 0, 1, ctypes.byref(first), ctypes.byref(count)) == _native.E_SHAPE
    assert lib.wc_resample_span(4, 4, 2, 2, ctypes.byref(first), ctypes.byref(count)) == _native.E_SHAPE
    assert lib.wc_resample_span(4, 4, 0, 5, ctypes.byref(first), ctypes.byref(count)) == _native.E_SHAPE
    assert lib.wc_resample_span(4, 4, 0, 4, None, ctypes.byref(count)) == _native.E_ARG


def test_tables_that_differ_from_the_native_bounds_are_refused(lib):
    """augment_geometry checks every index of its tables against the arithmetic that sizes the launch."""
    for in_size, out_size in AXES:
        K._check_axis_against_native(in_size, out_size, K.resample_axis(in_size, out_size)[0])
    bad = K.resample_axis(333, 24)[0].copy()
    bad[7, 1] += 1
    with pytest.raises(RuntimeError, match='index 7'):
        K._check_axis_against_native(333, 24, bad)


def test_wrapper_refuses_host_operands():
    jobs = torch.zeros((1, K.AUGMENT_JOB_WORDS), dtype=torch.int64)
    with pytest.raises(RuntimeError):  # no CPU path: the output and the device table must be on the GPU
        K.augment_batch(jobs, jobs, 4, torch.zeros(1, 3, 4, 4))


def test_translation_exports_load_image():
    from weatherconverter_amd import translation
    from weatherconverter_amd.diffusion_model import dataloader, train_ddpm
    assert translation.load_image is dataloader.load_image
    assert callable(train_ddpm.train) and callable(dataloader.get_loader)
