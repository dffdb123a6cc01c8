"""Segmentation labels and metrics without a GPU: the wc_seg.h binding, Pillow's NEAREST index rule, the
label tables and the metric formulas against the reference's recorded results (tests/golden/seg_labels.npz,
written by tests/golden/make_seg_golden.py), the label loader's index arithmetic, and every rejection of the
four entry points (they return from host checks: no HIP call is made)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from weatherconverter_amd import _abi, _build, _native
from weatherconverter_amd import kernels as K
from weatherconverter_amd.seg_model import datasets as D
from weatherconverter_amd.seg_model.metrics import AverageMeter, StreamSegMetrics

G = np.load(os.path.join(GOLDEN, 'seg_labels.npz'))
SEG_FUNCTIONS = ['wc_label_batch', 'wc_seg_confusion', 'wc_seg_confusion_pred', 'wc_seg_decode']


# ------------------------------------------------------------------------------------------- binding
def test_header_is_read_and_registered_beside_the_main_header():
    abi = _abi.read(open(os.path.join(_build.ROOT, 'include', 'wc_seg.h')).read())
    assert list(abi.functions) == SEG_FUNCTIONS == list(_native.SEG_ABI.functions)
    assert _native.LabelJob is _native.SEG_ABI.structs['wc_label_job']
    assert ctypes.sizeof(_native.LabelJob) == 8 * K.LABEL_JOB_WORDS == 64
    I, L, P = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    J = ctypes.POINTER(_native.LabelJob)
    assert _native.SEG_ABI.functions['wc_label_batch'] == (I, [J, J, I, I, I, P, P, P])
    assert _native.SEG_ABI.functions['wc_seg_confusion'] == (I, [P, P, I, I, I, I, P, P, P])
    assert _native.SEG_ABI.functions['wc_seg_confusion_pred'] == (I, [P, P, I, I, I, I, P, P])
    assert _native.SEG_ABI.functions['wc_seg_decode'] == (I, [P, I, L, I, P, P, P])
    for name in SEG_FUNCTIONS:
        assert name not in _native.EXPORTS
        assert _native._SIGNATURES[name] is _native.SEG_ABI.functions[name]
    assert len(_native.EXPORTS) == 88


def test_source_and_header_are_part_of_the_build():
    assert 'wc_seg.hip' in _build.SOURCES and 'wc_seg.h' in _build.ABI_HEADERS
    assert 'wc_seg.hip' not in _build.SINGLE16_SOURCES  # the single-piece variants share the default object


# ------------------------------------------------------------------------------- Pillow's NEAREST rule
def _pillow_nearest_indices(in_size: int, out_size: int):
    """The source index Pillow's NEAREST resize takes for every output index, along x and along y: an index
    image made of two uint8 planes (low and high byte of the position) is resized and read back."""
    from PIL import Image
    pos = np.arange(in_size)
    lo, hi = (pos & 255).astype(np.uint8), (pos >> 8).astype(np.uint8)
    out = []
    for axis in (0, 1):
        planes = []
        for p in (lo, hi):
            img = np.repeat(p[None, :], 3, 0) if axis == 0 else np.repeat(p[:, None], 3, 1)
            size = (out_size, 3) if axis == 0 else (3, out_size)
            r = np.array(Image.fromarray(np.ascontiguousarray(img)).resize(size, Image.NEAREST))
            planes.append((r[1] if axis == 0 else r[:, 1]).astype(np.int64))
        out.append(planes[0] + 256 * planes[1])
    return out


def _nearest_pairs():
    named = [(1920, 960), (1080, 540), (1080, 270), (2048, 1024), (1024, 512), (7, 3), (3, 7), (1, 5), (5, 1),
             (886, 1058), (2499, 1280), (25, 2466)]
    rng = np.random.default_rng(5)
    return named + [(int(rng.integers(1, 3001)), int(rng.integers(1, 3001))) for _ in range(200)]


def test_nearest_table_equals_pillow_on_both_axes():
    pytest.importorskip('PIL.Image')
    for in_size, out_size in _nearest_pairs():
        t = K.nearest_table(in_size, out_size)
        assert t.dtype == np.int32 and t.shape == (out_size, ) and t.min() >= 0 and t.max() < in_size
        along_x, along_y = _pillow_nearest_indices(in_size, out_size)
        assert np.array_equal(t, along_x), (in_size, out_size, 'x')
        assert np.array_equal(t, along_y), (in_size, out_size, 'y')


def test_a_fixed_point_walk_is_not_pillows():
    """Why the table accumulates in double as Pillow does: a 16.16 fixed-point walk of the same map differs
    from it (and so from Pillow, by the test above) on each of these pairs."""
    import math

    def fixed(i, o):
        a = i / o
        step, half = math.floor(a * 65536.0 + 0.5), math.floor(a * 0.5 * 65536.0 + 0.5)
        return np.clip(np.array([(half + x * step) >> 16 for x in range(o)]), 0, i - 1)
    for i, o in [(886, 1058), (2499, 1280), (25, 2466)]:
        assert not np.array_equal(fixed(i, o), K.nearest_table(i, o)), (i, o)


# ------------------------------------------------------------------------- tables against the reference
def test_tables_equal_the_references():
    assert D.ID_TO_TRAIN_ID.shape == (35, ) and np.array_equal(D.ID_TO_TRAIN_ID, G['id_to_train_id'])
    assert D.ID_TO_TRAIN_ID[34] == 255 and D.ID_TO_TRAIN_ID[-1] == 255
    assert D.TRAIN_ID_TO_COLOR.shape == (20, 3) and np.array_equal(D.TRAIN_ID_TO_COLOR, G['train_id_to_color'])
    assert len(D.CLASS_NAMES) == 19 == D.NUM_CLASSES and D.CLASS_NAMES[0] == 'road' and D.CLASS_NAMES[18] == 'bicycle'
    lut = D._LUT.numpy()
    assert np.array_equal(lut[:35], G['id_to_train_id'].astype(np.uint8)) and (lut[35:] == 255).all()


def test_host_encode_and_decode_equal_the_references():
    enc = D.encode_target(G['ids'])
    assert isinstance(enc, np.ndarray) and np.array_equal(enc, G['encoded'])
    assert np.array_equal(D.encode_target(torch.from_numpy(G['ids'])), G['encoded'])
    before = G['encoded'].copy()
    dec = D.decode_target(before)
    assert np.array_equal(dec, G['decoded']) and dec.shape == before.shape + (3, )
    assert np.array_equal(before, G['encoded'])  # the argument is not rewritten (the reference's is)
    with pytest.raises(IndexError):
        D.encode_target(np.array([[35]], dtype=np.uint8))


def _fast_hist(true, pred, n):
    """The reference's _fast_hist restated."""
    true, pred = true.reshape(-1), pred.reshape(-1)
    mask = (true >= 0) & (true < n)
    return np.bincount(n * true[mask].astype(int) + pred[mask], minlength=n * n).reshape(n, n)


def test_results_from_the_recorded_counts_equal_the_references():
    hist = sum(_fast_hist(G[f'true_{k}'], G[f'pred_{k}'], 19) for k in range(2))
    assert hist.dtype == np.int64 and np.array_equal(hist.astype(np.float64), G['hist'])
    r = StreamSegMetrics.results_from(hist)
    assert list(r) == ['Overall Acc', 'Mean Acc', 'FreqW Acc', 'Mean IoU', 'Class IoU']
    for key, name in (('Overall Acc', 'overall'), ('Mean Acc', 'mean_acc'), ('FreqW Acc', 'fwavacc'), ('Mean IoU', 'mean_iu')):
        assert isinstance(r[key], np.float64) and r[key] == G[name], key
    iu = np.array([r['Class IoU'][c] for c in range(19)])
    assert np.array_equal(np.isnan(iu), np.isnan(G['class_iu'])) and np.isnan(iu).sum() == 2
    assert (iu[~np.isnan(iu)] == G['class_iu'][~np.isnan(iu)]).all()
    s = StreamSegMetrics.to_str(r)
    assert s.startswith('\nOverall Acc: ') and s.endswith('\n') and 'Class IoU' not in s and s.count('\n') == 5
    assert 'Mean IoU: %f\n' % G['mean_iu'] in s


def test_average_meter():
    m = AverageMeter()
    m.update('loss', 1.0)
    m.update('loss', 2.0)
    m.update('acc', 4)
    assert m.get_results('loss') == 1.5 and m.get_results('acc') == 4
    m.reset('loss')
    m.update('loss', 3.0)
    assert m.get_results('loss') == 3.0
    m.reset_all()
    with pytest.raises(Exception):
        m.get_results('loss')


# ------------------------------------------------------------------------------------ loader geometry
def _id_png(tmp_path, w=1920, h=1080):
    from PIL import Image
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 34, size=(h // 8, w // 8)).astype(np.uint8).repeat(8, 0).repeat(8, 1)  # 8 x 8 blocks
    ids[::37, ::41] = 255
    ids += (np.add.outer(np.arange(h), np.arange(w)) % 5 == 0).astype(np.uint8) * (ids < 30)  # pixel-level detail
    path = str(tmp_path / 'ids.png')
    Image.fromarray(ids, 'L').save(path)
    return path, ids


def _pillow_chain(path, out_w, out_h, cx, cy, cw, ch):
    from PIL import Image
    r = np.array(Image.open(path).resize((out_w, out_h), Image.NEAREST))
    return r[cy:cy + ch, cx:cx + cw]


def _through_window(ids, win):
    x, y, rw, rh = win.rect
    rect = ids[y:y + rh, x:x + rw]
    assert win.rows.min() == 0 and win.rows.max() == rh - 1 and win.cols.min() == 0 and win.cols.max() == rw - 1
    assert win.rows.dtype == np.int32 and win.cols.dtype == np.int32
    return rect[win.rows[:, None], win.cols[None, :]]


def test_label_windows_reproduce_resize_then_center_crop(tmp_path):
    """Index arithmetic only: the rectangle and the tables a launch would get, applied with numpy."""
    pytest.importorskip('PIL.Image')
    path, ids = _id_png(tmp_path)
    # the reference's constants: Resize((540, 960), NEAREST) -> center_crop(512)
    win = D.label_window(1920, 1080, D.RESIZE, D.CROP)
    assert D.RESIZE == (540, 960) and D.CROP == (512, 512) and win.size == (512, 512)
    cx, cy = int(round((960 - 512) / 2.0)), int(round((540 - 512) / 2.0))
    assert np.array_equal(_through_window(ids, win), _pillow_chain(path, 960, 540, cx, cy, 512, 512))
    assert win.rect[2] < 1920 and win.rect[3] < 1080  # only the window's rectangle is uploaded
    # label_for: the field of view of load_image(path, S) at 4 S
    for S in (64, 256):
        win = D.label_for_window(1920, 1080, S, 4)
        ow, oh = K.resized_size(1920, 1080, 4 * S)
        cx, cy = K.center_crop_origin(ow, oh, 4 * S)
        assert oh == 4 * S and win.size == (4 * S, 4 * S)
        assert np.array_equal(_through_window(ids, win), _pillow_chain(path, ow, oh, cx, cy, 4 * S, 4 * S))
    # an odd geometry with upsampling
    win = D.label_window(1920, 1080, (1217, 2301), (1001, 333))
    cx, cy = int(round((2301 - 333) / 2.0)), int(round((1217 - 1001) / 2.0))
    assert np.array_equal(_through_window(ids, win), _pillow_chain(path, 2301, 1217, cx, cy, 333, 1001))
    with pytest.raises(RuntimeError):
        D.label_window(1920, 1080, (540, 960), (541, 512))


def test_load_label_refuses_other_modes(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    p = str(tmp_path / 'rgb.png')
    Image.fromarray(np.zeros((8, 8, 3), dtype=np.uint8), 'RGB').save(p)
    with pytest.raises(ValueError, match='mode'):
        D.load_label(p, (4, 4), (2, 2), device='cpu')
    with pytest.raises(ValueError, match='mode'):
        D.label_for(p, 2, device='cpu')


# ---------------------------------------------------------------------------------------- rejections
@pytest.fixture(scope='module')
def lib():
    if not os.path.exists(_build.LIB_PATH):
        if not os.path.exists(_build.HIPCC):
            pytest.skip('hipcc not available to build the library')
        _build.build()
    lib = ctypes.CDLL(_build.LIB_PATH)
    for name, (res, args) in _native.SEG_ABI.functions.items():
        assert hasattr(lib, name), name
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


A = 4096  # a 16-byte aligned address that is never dereferenced


def test_label_batch_rejections_come_before_any_launch(lib):
    E = _native.E_SHAPE
    rows = np.arange(6, dtype=np.int32)
    cols = np.arange(5, dtype=np.int32)
    lut = (ctypes.c_ubyte * 256)()

    def job(**over):
        f = dict(src=A, pitch=5, rect_w=5, rect_h=6, rows=A, cols=A, rows_host=rows.ctypes.data, cols_host=cols.ctypes.data)
        f.update(over)
        return _native.LabelJob(**f)

    def call(j=None, jd=None, n=1, hc=6, wc=5, table=lut, out=A):
        j = ctypes.pointer(job()) if j is None else j
        return lib.wc_label_batch(j, ctypes.pointer(job()) if jd is None else jd, n, hc, wc, table, out, None)
    null = ctypes.POINTER(_native.LabelJob)()
    assert call(j=null) == E and call(jd=null) == E and call(table=None) == E and call(out=None) == E
    for name in ('src', 'rows', 'cols', 'rows_host', 'cols_host'):
        assert call(j=ctypes.pointer(job(**{name: 0}))) == E, name
    assert call(n=0) == E and call(n=-1) == E and call(n=65536) == E  # B outside 1..65535
    assert call(hc=0) == E and call(wc=0) == E and call(hc=-3) == E  # an empty window
    assert call(j=ctypes.pointer(job(pitch=4))) == E  # pitch below the rectangle's width
    assert call(j=ctypes.pointer(job(rect_w=0))) == E and call(j=ctypes.pointer(job(rect_h=0))) == E
    for table, at, bad in ((rows, 2, 6), (rows, 0, -1), (cols, 4, 5), (cols, 1, -7)):  # an entry outside the rectangle
        keep = int(table[at])
        table[at] = bad
        assert call() == E
        table[at] = keep
    two = (_native.LabelJob * 2)(job(), job(pitch=1))  # a second row is checked like the first
    assert lib.wc_label_batch(two, two, 2, 6, 5, lut, A, None) == E
    assert E != _native.E_ARG and _native.OK == 0


def test_confusion_rejections_come_before_any_launch(lib):
    E_ARG, E_SHAPE = _native.E_ARG, _native.E_SHAPE
    for fn, tail in ((lib.wc_seg_confusion, (None, None)), (lib.wc_seg_confusion_pred, (None, ))):
        def call(src=A, labels=A, B=1, C=19, H=8, W=8, hist=A):
            return fn(src, labels, B, C, H, W, hist, *tail)
        assert call(src=None) == E_ARG and call(labels=None) == E_ARG and call(hist=None) == E_ARG
        assert call(labels=A + 4) == E_ARG and call(hist=A + 4) == E_ARG
        assert call(C=1) == E_SHAPE and call(C=33) == E_SHAPE and call(C=0) == E_SHAPE
        assert call(B=0) == E_SHAPE and call(B=-1) == E_SHAPE
        assert call(H=0) == E_SHAPE and call(W=0) == E_SHAPE  # H * W of 0
        assert call(B=2**20, H=2**11, W=2**11) == E_SHAPE  # above 2^40 pixels
    for off in (4, 8, 12):  # a misaligned logits pointer
        assert lib.wc_seg_confusion(A + off, A, 1, 19, 8, 8, A, None, None) == E_ARG


def test_decode_rejections_come_before_any_launch(lib):
    E_ARG, E_SHAPE = _native.E_ARG, _native.E_SHAPE
    pal = (ctypes.c_ubyte * 99)()

    def call(m=A, i64=0, n=64, C=19, palette=pal, out=A):
        return lib.wc_seg_decode(m, i64, n, C, palette, out, None)
    assert call(m=None) == E_ARG and call(palette=None) == E_ARG and call(out=None) == E_ARG
    assert call(i64=2) == E_ARG and call(i64=-1) == E_ARG and call(m=A + 4, i64=1) == E_ARG
    assert call(C=1) == E_SHAPE and call(C=33) == E_SHAPE
    assert call(n=0) == E_SHAPE and call(n=-5) == E_SHAPE and call(n=2**40 + 1) == E_SHAPE


def test_wrappers_refuse_host_operands():
    hist = torch.zeros((19, 19), dtype=torch.int64)
    with pytest.raises(RuntimeError):  # no CPU path
        K.seg_confusion(torch.zeros(1, 19, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64), hist)
    with pytest.raises(RuntimeError):
        K.seg_decode(torch.zeros(4, 4, dtype=torch.uint8), D._PALETTE)
    with pytest.raises(RuntimeError):
        K.label_batch(torch.zeros((1, K.LABEL_JOB_WORDS), dtype=torch.int64), torch.zeros(8, dtype=torch.int64), D._LUT,
                      torch.zeros((1, 2, 2), dtype=torch.int64))
    with pytest.raises(RuntimeError):
        K.nearest_table(0, 4)


def test_translation_and_inference_export_the_file_driven_path():
    from weatherconverter_amd import translation
    from weatherconverter_amd.seg_model import inference
    assert callable(translation.translate_files) and callable(translation.main)
    assert callable(inference.predict) and callable(inference.semantic_score)
    assert callable(D.preprocess) and callable(D.load_label) and callable(D.label_for)
