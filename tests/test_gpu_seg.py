"""Segmentation labels and metrics on the GPU (csrc/wc_seg.hip): wc_label_batch against the Pillow chain,
wc_seg_confusion / wc_seg_confusion_pred against numpy.argmax + the reference's _fast_hist restated (exact,
no pixel excluded), wc_seg_decode against palette indexing, StreamSegMetrics streaming on the device, and
translate_files / main end to end at tests/test_guided.py's sizes."""
import os

import numpy as np
import pytest
import torch

from weatherconverter_amd import kernels as K
from weatherconverter_amd.seg_model import datasets as D
from weatherconverter_amd.seg_model.metrics import StreamSegMetrics

pytestmark = pytest.mark.gpu


def _fast_hist(true, pred, n):
    """The reference's _fast_hist restated (numpy, int64 counts)."""
    true, pred = np.asarray(true).reshape(-1), np.asarray(pred).reshape(-1)
    mask = (true >= 0) & (true < n)
    return np.bincount(n * true[mask].astype(int) + pred[mask], minlength=n * n).reshape(n, n)


# ------------------------------------------------------------------------------------ wc_label_batch
# the device table: the reference's for ids 0..34, 255 for every id above (the host path raises there)
LUT = np.r_[D.ID_TO_TRAIN_ID, np.full(256 - 35, 255)].astype(np.int64)


def _id_image(h=135, w=240):
    rng = np.random.default_rng(3)
    ids = rng.integers(0, 34, size=(h, w)).astype(np.uint8)
    ids[0, :35] = np.r_[np.arange(34), 255].astype(np.uint8)  # every id 0..33 and 255
    ids[40:90, 60:200] = 7  # constant regions
    ids[90:130, 10:100] = 26
    ids[::13, ::17] = 255
    return ids


def _pillow_window(ids, out_w, out_h, cx, cy, cw, ch):
    from PIL import Image
    r = np.array(Image.fromarray(ids, 'L').resize((out_w, out_h), Image.NEAREST))
    return torch.from_numpy(LUT[r[cy:cy + ch, cx:cx + cw]])


def _job(ids, win):
    x, y, rw, rh = win.rect
    return torch.from_numpy(np.ascontiguousarray(ids[y:y + rh, x:x + rw])), win.rows, win.cols


def test_label_batch_three_geometries_in_one_launch():
    pytest.importorskip('PIL.Image')
    ids = _id_image()
    h, w = ids.shape
    hc, wc = 61, 119  # one window size per launch; an odd width
    # (resized w, h, crop x, y): a downsampled corner, the centre of an upsampled map, an offset identity window
    geoms = [(120, 67, 1, 6), (480, 270, (480 - wc) // 2, (270 - hc) // 2), (240, 135, 77, 40)]
    wins = [D.LabelWindow(w, h, ow, oh, cx, cy, wc, hc) for ow, oh, cx, cy in geoms]
    buf = torch.full((5, hc, wc), -7, dtype=torch.int64, device='cuda')  # poisoned, with a plane either side
    out = D._label_launch([_job(ids, win) for win in wins], hc, wc, torch.device('cuda'), out=buf[1:4])
    assert out.data_ptr() == buf[1].data_ptr()
    for b, (ow, oh, cx, cy) in enumerate(geoms):
        assert torch.equal(out[b].cpu(), _pillow_window(ids, ow, oh, cx, cy, wc, hc)), geoms[b]
    assert (buf[0] == -7).all() and (buf[4] == -7).all()  # nothing outside the planes is written
    assert set(out.unique().tolist()) <= set(range(19)) | {255}


def test_label_batch_full_image_with_an_odd_width_and_load_label(tmp_path):
    Image = pytest.importorskip('PIL.Image')
    ids = _id_image(135, 239)
    win = D.LabelWindow(239, 135, 239, 135, 0, 0, 239, 135)  # identity, the whole image
    assert win.rect == (0, 0, 239, 135)
    out = D._label_launch([_job(ids, win)], 135, 239, torch.device('cuda'))
    assert out.dtype == torch.int64 and torch.equal(out[0].cpu(), torch.from_numpy(LUT[ids]))
    # the file-driven loaders
    path = str(tmp_path / 'ids.png')
    Image.fromarray(ids, 'L').save(path)
    got = D.load_label(path, resize=(67, 120), crop=(50, 33))
    cx, cy = int(round((120 - 33) / 2.0)), int(round((67 - 50) / 2.0))
    assert got.shape == (1, 50, 33) and got.is_cuda
    assert torch.equal(got[0].cpu(), _pillow_window(ids, 120, 67, cx, cy, 33, 50))
    got = D.label_for(path, 16, scale=4)
    ow, oh = K.resized_size(239, 135, 64)
    cx, cy = K.center_crop_origin(ow, oh, 64)
    assert torch.equal(got[0].cpu(), _pillow_window(ids, ow, oh, cx, cy, 64, 64))
    # a device id map through encode_target: ids above 34 become 255 there
    dev_ids = torch.from_numpy(ids).cuda()
    dev_ids[3, 3] = 200
    want = LUT[ids]
    want[3, 3] = 255
    assert torch.equal(D.encode_target(dev_ids).cpu(), torch.from_numpy(want))


# ---------------------------------------------------------------------------------- wc_seg_confusion
VALUES = torch.tensor([-1.0, 0.0, 0.5, 1.0])


def _case(B, C, H, W, seed, bad_labels=True, device='cuda'):
    """Logits drawn from four values (ties everywhere) and labels in [0, C) with 255, -1, C and 1000 mixed in."""
    g = torch.Generator().manual_seed(seed)
    logits = VALUES[torch.randint(0, 4, (B, C, H, W), generator=g)]
    labels = torch.randint(0, C, (B, H, W), generator=g)
    if bad_labels:
        r = torch.rand((B, H, W), generator=g)
        for lo, v in ((0.00, 255), (0.05, -1), (0.08, C), (0.11, 1000)):
            labels[(r >= lo) & (r < lo + 0.03)] = v
    return logits.to(device), labels.to(device)


def _check(logits, labels, C, seed_hist=None):
    B, _, H, W = logits.shape
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda') if seed_hist is None else seed_hist.clone()
    before = hist.clone()
    pred = torch.full((B + 2, H, W), 77, dtype=torch.uint8, device='cuda')
    labels_before = labels.clone()
    K.seg_confusion(logits, labels, hist, pred[1:B + 1])
    want_pred = logits.cpu().numpy().argmax(1)
    want = _fast_hist(labels.cpu().numpy(), want_pred, C)
    assert np.array_equal(pred[1:B + 1].cpu().numpy(), want_pred)  # every pixel, ignored ones included
    assert (pred[0] == 77).all() and (pred[B + 1] == 77).all()
    assert np.array_equal((hist - before).cpu().numpy(), want)
    assert torch.equal(labels, labels_before)
    # the same matrix without the prediction output, and from the ready prediction map
    for scores in (logits, pred[1:B + 1].contiguous()):
        h2 = torch.zeros((C, C), dtype=torch.int64, device='cuda')
        K.seg_confusion(scores, labels, h2)
        assert np.array_equal(h2.cpu().numpy(), want)
    return want


@pytest.mark.parametrize('B,C,H,W', [(2, 19, 37, 53), (1, 19, 64, 64), (3, 2, 8, 12), (1, 32, 16, 20), (1, 19, 1, 5)])
def test_confusion_equals_argmax_and_fast_hist(B, C, H, W):
    """(2, 19, 37, 53): H*W odd, one pixel per lane; (1, 19, 1, 5): fewer pixels than a wave; C = 2 and 32: the
    class-count limits on the run-time-C kernel; 19 classes take the unrolled one."""
    logits, labels = _case(B, C, H, W, seed=B * 1000 + C)
    want = _check(logits, labels, C)
    assert want.sum() > 0 or H * W < 8


def test_confusion_at_the_workloads_plane():
    logits, labels = _case(1, 19, 1024, 1024, seed=1)
    labels[0, 200:700, 100:900] = 8  # a large constant region among the noise
    want = _check(logits, labels, 19)
    assert want.sum() > 800000


def test_confusion_signed_zeros_and_nans():
    logits, labels = _case(1, 19, 24, 28, seed=5)
    g = torch.Generator().manual_seed(6)
    flat = logits.permute(0, 2, 3, 1).reshape(-1, 19)  # a copy: [pixel][class]
    n = flat.shape[0]
    flat[: n // 4] = torch.where(torch.rand((n // 4, 19), generator=g).cuda() < 0.5, 0.0, -0.0)  # only signed zeros
    flat[n // 4: n // 2, :] = flat[n // 4: n // 2, :].clamp(max=0.0)  # the maximum is a zero ...
    flat[n // 4: n // 2, 7] = -0.0  # ... of either sign
    flat[n // 4: n // 2, 11] = 0.0
    nan_at = torch.randint(0, 19, (n // 4, ), generator=g).cuda()
    rows = torch.arange(n // 2, n // 2 + n // 4).cuda()
    flat[rows, nan_at] = float('nan')  # one NaN: it wins
    flat[rows[::2], (nan_at[::2] + 5) % 19] = float('nan')  # two NaNs: the first wins
    flat[-5:] = float('nan')  # all NaN: class 0
    logits = flat.reshape(1, 24, 28, 19).permute(0, 3, 1, 2).contiguous()
    assert torch.isnan(logits).sum() > n // 4 and (logits == 0).any()
    _check(logits, labels, 19)
    # the same values through the one-pixel-per-lane kernel (H*W odd)
    _check(logits[:, :, :23, :27].contiguous(), labels[:, :23, :27].contiguous(), 19)


def test_confusion_every_pixel_ignored_and_constant_labels():
    logits, _ = _case(2, 19, 32, 48, seed=9)
    seed = torch.arange(361, dtype=torch.int64, device='cuda').reshape(19, 19) + 5
    ignored = torch.full((2, 32, 48), 255, dtype=torch.int64, device='cuda')
    ignored[0, ::3] = -1
    ignored[1, ::5] = 19
    want = _check(logits, ignored, 19, seed_hist=seed)
    assert want.sum() == 0  # and _check saw the histogram unchanged
    constant = torch.full((2, 32, 48), 13, dtype=torch.int64, device='cuda')  # every lane on one row of counters
    want = _check(logits, constant, 19)
    assert want[13].sum() == 2 * 32 * 48 and want.sum() == want[13].sum()
    uniform = torch.zeros((1, 19, 64, 64), device='cuda')
    uniform[:, 4] = 1.0  # one key for every wave: the whole-wave add
    want = _check(uniform, torch.full((1, 64, 64), 13, dtype=torch.int64, device='cuda'), 19)
    assert want[13, 4] == 64 * 64 and want.sum() == 64 * 64


def test_confusion_streams_into_int64_counts():
    C = 19
    seed = (2**40 + torch.arange(C * C, dtype=torch.int64)).reshape(C, C).cuda()
    hist = seed.clone()
    total = np.zeros((C, C), dtype=np.int64)
    for k, shape in enumerate(((2, C, 16, 24), (1, C, 9, 13))):
        logits, labels = _case(*shape, seed=40 + k)
        K.seg_confusion(logits, labels, hist)
        total += _fast_hist(labels.cpu().numpy(), logits.cpu().numpy().argmax(1), C)
    assert total.sum() > 0 and np.array_equal(hist.cpu().numpy(), seed.cpu().numpy() + total)


def test_pred_form_ignores_out_of_range_predictions_and_misaligned_views():
    C = 5
    g = torch.Generator().manual_seed(2)
    pred = torch.randint(0, 8, (2, 12, 20), generator=g).to(torch.uint8)  # 5, 6, 7 are out of range
    labels = torch.randint(0, C, (2, 12, 20), generator=g)
    keep = pred.numpy() < C
    want = _fast_hist(np.where(keep, labels.numpy(), 255), np.where(keep, pred.numpy(), 0), C)
    hist = torch.zeros((C, C), dtype=torch.int64, device='cuda')
    K.seg_confusion(pred.cuda(), labels.cuda(), hist)
    assert np.array_equal(hist.cpu().numpy(), want)
    # operands one element into their allocations: no 16-byte labels / 4-byte map alignment, the narrow kernel
    pbuf, lbuf = torch.zeros(481, dtype=torch.uint8, device='cuda'), torch.zeros(481, dtype=torch.int64, device='cuda')
    pbuf[1:] = pred.reshape(-1).cuda()
    lbuf[1:] = labels.reshape(-1).cuda()
    hist.zero_()
    K.seg_confusion(pbuf[1:].view(2, 12, 20), lbuf[1:].view(2, 12, 20), hist)
    assert np.array_equal(hist.cpu().numpy(), want)


# ------------------------------------------------------------------------------------- wc_seg_decode
def test_decode_equals_palette_indexing_and_leaves_its_input():
    g = torch.Generator().manual_seed(4)
    m8 = torch.randint(0, 19, (2, 13, 17), generator=g).to(torch.uint8)
    m8[0, :3] = 255
    m8[1, 5] = torch.tensor([19, 20, 100, 254, 255] + [3] * 12, dtype=torch.uint8)
    palette = D.TRAIN_ID_TO_COLOR.astype(np.uint8)
    want8 = palette[np.minimum(m8.numpy().astype(np.int64), 19)]
    dev = m8.cuda()
    out = D.decode_target(dev)
    assert out.dtype == torch.uint8 and out.shape == (2, 13, 17, 3) and np.array_equal(out.cpu().numpy(), want8)
    assert torch.equal(dev.cpu(), m8)  # unchanged (the reference rewrites 255 in place)
    m64 = m8.to(torch.int64)
    m64[0, 4, :4] = torch.tensor([-1, 1000, 2**40, -2**40])
    v = m64.numpy()
    want64 = palette[np.where((v >= 0) & (v < 19), v, 19)]
    dev = m64.cuda()
    assert np.array_equal(D.decode_target(dev).cpu().numpy(), want64) and torch.equal(dev.cpu(), m64)


# ---------------------------------------------------------------------------------- StreamSegMetrics
def _same_results(a, b):
    assert list(a) == list(b)
    for k in a:
        if k == 'Class IoU':
            assert list(a[k]) == list(b[k])
            x, y = np.array(list(a[k].values())), np.array(list(b[k].values()))
        else:
            x, y = np.array([a[k]]), np.array([b[k]])
        assert x.dtype == np.float64 and np.array_equal(np.isnan(x), np.isnan(y)) and (x[~np.isnan(x)] == y[~np.isnan(x)]).all(), k


def test_stream_metrics_on_device_over_three_batches():
    C = 19
    m = StreamSegMetrics(C)
    total = np.zeros((C, C), dtype=np.int64)
    for k, shape in enumerate(((2, C, 16, 24), (1, C, 9, 13), (1, C, 8, 8))):
        logits, labels = _case(*shape, seed=70 + k)
        labels[(labels == 3) | (labels == 17)] = 255  # absent classes ...
        logits[:, 3] = -2.0
        logits[:, 17] = -2.0  # ... in the predictions too: NaN IoU rows
        pred = logits.cpu().numpy().argmax(1)
        if k == 0:
            m.update(labels, logits)  # fused
        elif k == 1:
            m.update(labels, torch.from_numpy(pred).cuda())  # a device integer prediction
        else:
            m.update(labels.cpu().numpy(), pred)  # the reference's numpy call
        total += _fast_hist(labels.cpu().numpy(), pred, C)
    cm = m.confusion_matrix
    assert cm.dtype == np.float64 and np.array_equal(cm, total.astype(np.float64))
    # the reference's formulas, restated on the summed numpy histogram
    hist = total.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        iu = np.diag(hist) / (hist.sum(axis=1) + hist.sum(axis=0) - np.diag(hist))
        freq = hist.sum(axis=1) / hist.sum()
        want = {'Overall Acc': np.diag(hist).sum() / hist.sum(), 'Mean Acc': np.nanmean(np.diag(hist) / hist.sum(axis=1)),
                'FreqW Acc': (freq[freq > 0] * iu[freq > 0]).sum(), 'Mean IoU': np.nanmean(iu),
                'Class IoU': dict(zip(range(C), iu))}
    got = m.get_results()
    _same_results(got, want)
    assert np.isnan(got['Class IoU'][3]) and np.isnan(got['Class IoU'][17]) and 0 < got['Mean IoU'] < 1
    with pytest.raises(ValueError):
        m.update(labels.cpu().numpy(), np.full_like(pred, 19))  # a host prediction outside [0, C)
    m.reset()
    assert not m.confusion_matrix.any()


# ------------------------------------------------------------------------------------ translate_files
@pytest.fixture(scope='module')
def models():
    from test_gpu_unet import MANIFEST
    from test_guided import _seg, _srgan
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.diffusion_model.scheduler.linear_noise_scheduler import LinearNoiseScheduler
    from weatherconverter_amd.synthetic import init_synthetic_
    torch.backends.cudnn.allow_tf32 = False
    unet = Unet(ModelConfig(**MANIFEST['tiny']['config']))
    init_synthetic_(unet)
    return unet.cuda().eval(), LinearNoiseScheduler(1000, 0.0001, 0.02), _seg().cuda(), _srgan().cuda()


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    from PIL import Image
    d = tmp_path_factory.mktemp('seg_files')
    rng = np.random.default_rng(8)
    frame = rng.integers(0, 256, size=(45, 80, 3)).astype(np.uint8)
    ids = rng.integers(0, 34, size=(9, 16)).astype(np.uint8).repeat(5, 0).repeat(5, 1)  # 45 x 80, 5 x 5 blocks
    ids[::7, ::9] = 255
    Image.fromarray(frame, 'RGB').save(str(d / 'frame.png'))
    Image.fromarray(ids, 'L').save(str(d / 'ids.png'))
    return d, str(d / 'frame.png'), str(d / 'ids.png'), ids


def test_translate_files_end_to_end(models, files):
    """translate_files against sample_with_sgg on load_image + the Pillow-built label, same t_start / noise.

    The loop is compared bit for bit in mode='reference', where it is deterministic: the guidance is computed from
    the label and then discarded (D1), so every kernel that shapes the output is one of this library's.  In
    mode='applied' the output goes through the segmenter's input gradient, which PyTorch's autograd does not
    reproduce bit for bit from one call to the next (measured here: two calls on equal inputs differ by
    2.7e-12 at a gradient scale of 8.5e-6, relative 3e-7, and with it two sample_with_sgg calls on equal inputs
    by 6e-8 absolute at LAMBDA = 1e6), so there the two are compared with the bound tests/test_guided.py uses for
    the same loop, rel-L2 < 1e-6, and the guidance must have moved the output by more than that."""
    from conftest import rel_l2
    from weatherconverter_amd.translation import load_image, sample_with_sgg, translate_files
    unet, sched, seg, gen = models
    _, frame_path, ids_path, ids = files
    g = torch.Generator().manual_seed(3)
    noise = torch.randn((1, 3, 32, 32), generator=g)
    ow, oh = K.resized_size(80, 45, 128)
    cx, cy = K.center_crop_origin(ow, oh, 128)
    gt = _pillow_window(ids, ow, oh, cx, cy, 128, 128)[None].cuda()  # the Pillow-built label
    out = {}
    for mode in ('reference', 'applied'):
        kw = dict(N=4, t_start=torch.tensor([3]), noise=noise, LAMBDA=1e6, mode=mode)  # grads are ~1e-6
        torch.manual_seed(9)
        res = translate_files(frame_path, ids_path, unet, sched, seg, gen, **kw)
        assert sorted(res) == ['output', 'pred', 'score']
        torch.manual_seed(9)
        want = sample_with_sgg(load_image(frame_path, 32), unet, sched, seg, gt, gen, **kw)
        assert res['output'].shape == (1, 3, 128, 128) and torch.isfinite(res['output']).all()
        if mode == 'reference':
            assert torch.equal(res['output'], want)
        else:
            print('applied: translate_files vs loop rel-L2', rel_l2(res['output'], want))
            assert rel_l2(res['output'], want) < 1e-6
        # the prediction and the score are those of the segmenter on translate_files' own output
        with torch.no_grad():
            pred = seg(res['output']).argmax(1).cpu().numpy()
        assert res['pred'].dtype == torch.uint8 and res['pred'].is_cuda
        assert np.array_equal(res['pred'].cpu().numpy(), pred)
        m = StreamSegMetrics(19)
        m.update(gt.cpu().numpy(), pred)  # fed the numpy way
        _same_results(res['score'], m.get_results())
        assert m.confusion_matrix.sum() == (gt != 255).sum().item() > 0
        out[mode] = res['output']
    print('applied vs reference rel-L2', rel_l2(out['applied'], out['reference']))
    assert rel_l2(out['applied'], out['reference']) > 1e-6  # the label reached the guidance


def test_main_writes_its_two_pngs(models, files, capsys):
    import yaml
    from PIL import Image
    from test_gpu_unet import MANIFEST
    from weatherconverter_amd.diffusion_model.config import DEFAULT_CONFIG_PATH
    from weatherconverter_amd.translation import main
    unet, _, seg, gen = models
    d, frame_path, ids_path, _ = files
    cfg = yaml.safe_load(open(DEFAULT_CONFIG_PATH))
    cfg['model'] = MANIFEST['tiny']['config']
    yaml.safe_dump(cfg, open(str(d / 'config.yaml'), 'w'))
    torch.save({'model_state_dict': unet.state_dict()}, str(d / 'unet.ckpt'))
    torch.save({'model_state_dict': seg.state_dict()}, str(d / 'seg.pth'))
    torch.save({'model': gen.state_dict()}, str(d / 'srgan.pth.tar'))
    out = str(d / 'out')
    res = main(['--image', frame_path, '--labels', ids_path, '--diff-config', str(d / 'config.yaml'), '--diff-ckpt',
                str(d / 'unet.ckpt'), '--seg-ckpt', str(d / 'seg.pth'), '--srgan-ckpt', str(d / 'srgan.pth.tar'),
                '--out', out, '--N', '4'])
    for name in ('output.png', 'pred_color.png'):
        im = Image.open(os.path.join(out, name))
        assert im.size == (128, 128) and im.mode == 'RGB', name
    colours = np.array(Image.open(os.path.join(out, 'pred_color.png')))
    assert np.array_equal(colours, D.TRAIN_ID_TO_COLOR.astype(np.uint8)[res['pred'][0].cpu().numpy()])
    assert 'Mean IoU: ' in capsys.readouterr().out
