"""GPU: diffusion_model.ema.EMA (wc_ema_update, wc_ema_swap) against torch lerp_ and float64.

The yardstick of every numerical check is the one of tests/test_gpu_optim.py: the same updates are run
three ways from identical fp32 inputs -- with wc_ema_update, with torch's lerp_ in fp32 on the GPU, and
with a float64 restatement of the recurrence -- and for the shadow AND for the displacement
shadow_after - shadow_before, over all tensors together, our rel-L2 error against float64 may be at
most 2x torch's against the same float64 (the margin is for rounding order only).  The displacement is
there because at decay 0.9999 the shadow barely moves: its own rel-L2 would hide a wrong update.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN, rel_l2

pytestmark = pytest.mark.gpu

CHUNK = 4096
# (elements, misalignment of the shadow in floats, of p): sizes around the 4-wide vector and the chunk,
# every combination of 16-byte and 4-byte aligned operands at small and at multi-chunk sizes
CARVE = [(1, 0, 0), (3, 1, 1), (4, 0, 0), (5, 0, 0), (63, 1, 0), (64, 0, 1), (1023, 0, 0), (CHUNK, 0, 0),
         (CHUNK + 1, 0, 0), (3 * CHUNK + 1, 0, 0), (CHUNK + 1, 3, 2), (2 * CHUNK + 3, 2, 0), (70001, 0, 0)]
SENTINEL = -1234.5678
STEPS = 5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _cat(ts):
    return torch.cat([t.detach().double().cpu().reshape(-1) for t in ts])


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def assert_yardstick(ours, theirs, ref, before, label):
    """ours / theirs / ref: the shadows after the updates; before: the shadows they all started from."""
    b, o, t, r = _cat(before), _cat(ours), _cat(theirs), _cat(ref)
    figures = {'shadow': (rel_l2(o, r), rel_l2(t, r)), 'displacement': (rel_l2(o - b, r - b), rel_l2(t - b, r - b))}
    for name, (eo, et) in figures.items():
        print(f'{label} {name}: ours {eo:.3e} torch {et:.3e} ratio {eo / max(et, 1e-300):.3f}')
    assert float((r - b).norm()) > 0  # the reference moved: the displacement figures mean something
    for name, (eo, et) in figures.items():
        assert eo <= 2 * et, (label, name, eo, et)


def ema_f64(s, p, decay):
    """One update in float64: s + (1 - decay) (p - s)."""
    return s.double() + (1.0 - decay) * (p.double() - s.double())


def _offsets(mis):
    """Start of each view (in floats): a multiple of 4 plus the wanted misalignment, at least one float
    of gap after the previous view."""
    offs, cur = [], 3
    for (n, *_), d in zip(CARVE, mis):
        o = (cur + 1 + 3) // 4 * 4 + d
        offs.append(o)
        cur = o + n
    return offs, cur + 5


class Carved:
    """Views of the CARVE sizes and alignments in two sentinel-filled buffers, filled from CPU lists."""

    def __init__(self, s0, p0):
        soff, send = _offsets([c[1] for c in CARVE])
        poff, pend = _offsets([c[2] for c in CARVE])
        self.sbuf = torch.full((send, ), SENTINEL, device='cuda')
        self.pbuf = torch.full((pend, ), SENTINEL, device='cuda')
        assert self.sbuf.data_ptr() % 16 == 0 and self.pbuf.data_ptr() % 16 == 0
        smask, pmask = torch.ones(send, dtype=torch.bool), torch.ones(pend, dtype=torch.bool)
        self.ss, self.ps = [], []
        for (n, ds, dp), os_, op, s, p in zip(CARVE, soff, poff, s0, p0):
            self.ss.append(self.sbuf[os_:os_ + n])
            self.ps.append(self.pbuf[op:op + n])
            self.ss[-1].copy_(s)
            self.ps[-1].copy_(p)
            smask[os_:os_ + n] = False
            pmask[op:op + n] = False
            assert self.ss[-1].data_ptr() % 16 == 4 * ds and self.ps[-1].data_ptr() % 16 == 4 * dp
        self.smask, self.pmask = smask.cuda(), pmask.cuda()

    def assert_sentinels_intact(self):
        sent = torch.tensor(SENTINEL).cuda()
        assert torch.equal(self.sbuf[self.smask], sent.expand(int(self.smask.sum())))
        assert torch.equal(self.pbuf[self.pmask], sent.expand(int(self.pmask.sum())))


@pytest.fixture(scope='module')
def synthetic():
    from weatherconverter_amd import _native
    assert _native.load().wc_optim_chunk_elems() == CHUNK  # the sizes above are chosen around it
    g = _gen(11)
    s0 = [torch.randn(n, generator=g) for n, _, _ in CARVE]
    # the parameter drifts away from where the shadow started, a little more at every step
    p = [s + 0.1 * torch.randn(s.shape, generator=g) for s in s0]
    ps = []
    for _ in range(STEPS):
        p = [q + 0.05 * torch.randn(q.shape, generator=g) for q in p]
        ps.append(p)
    return s0, ps


def _run_carved(s0, ps, decay):
    """STEPS updates of ours on the carved views; p is only read and no sentinel is touched."""
    from weatherconverter_amd import kernels as K
    cv = Carved(s0, ps[0])
    jobs = K.ema_jobs(cv.ss, cv.ps)
    for plist in ps:
        for v, p in zip(cv.ps, plist):
            v.copy_(p)
        snap = cv.pbuf.clone()
        K.ema_update(jobs, decay)
        assert torch.equal(_bits(cv.pbuf), _bits(snap))  # the parameter buffer is only read
    cv.assert_sentinels_intact()
    return cv


def _run_plain(s0, ps, decay):
    """The same updates on plain (aligned) tensors of their own."""
    from weatherconverter_amd import kernels as K
    ss = [s.clone().cuda() for s in s0]
    pv = [p.clone().cuda() for p in ps[0]]
    assert all(t.data_ptr() % 16 == 0 for t in ss + pv)
    jobs = K.ema_jobs(ss, pv)
    for plist in ps:
        for v, p in zip(pv, plist):
            v.copy_(p)
        K.ema_update(jobs, decay)
    return ss


# --------------------------------------------------------------------------------------- 1: synthetic list
@pytest.mark.parametrize('decay', [0.9, 0.9999])
def test_synthetic_list_five_updates(synthetic, decay):
    s0, ps = synthetic
    cv = _run_carved(s0, ps, decay)
    theirs = [s.clone().cuda() for s in s0]
    ref = [s.double() for s in s0]
    for plist in ps:
        for s, p in zip(theirs, plist):
            s.lerp_(p.cuda(), 1.0 - decay)
        ref = [ema_f64(s, p, decay) for s, p in zip(ref, plist)]
    assert_yardstick(cv.ss, theirs, ref, s0, f'synthetic[{decay}]')
    # every element on its own: an update rounds the shadow once (2^-24 |s|) and w (p - s) twice
    # (w <= 0.1), all below 2^-23 M with M = |s0| + max |p| bounding every value; later updates shrink
    # what earlier ones left, so STEPS of them stay below STEPS 2^-23 M
    for i, (c, s, r) in enumerate(zip(CARVE, cv.ss, ref)):
        M = s0[i].double().abs() + torch.stack([plist[i] for plist in ps]).double().abs().amax(0)
        assert bool(((s.double().cpu() - r).abs() <= STEPS * 2.0**-23 * M).all()), c


# --------------------------------------------------------------------------------------- 2: bits
def test_bits_across_paths_and_runs(synthetic):
    """Alignment picks the access width, never the arithmetic: the carved views (f32x4 rows, their n % 4
    tails, one-float rows) and plain aligned tensors hold the same bits; so do two runs."""
    s0, ps = synthetic
    a = _run_carved(s0, ps, 0.9999)
    b = _run_carved(s0, ps, 0.9999)
    plain = _run_plain(s0, ps, 0.9999)
    assert torch.equal(_bits(a.sbuf), _bits(b.sbuf))
    for c, x, y in zip(CARVE, a.ss, plain):
        assert torch.equal(x, y) and torch.equal(_bits(x), _bits(y)), c
    assert not any(torch.equal(x.cpu(), s) for x, s in zip(a.ss, s0))  # and every tensor was reached


# --------------------------------------------------------------------------------------- 3: swap
def test_swap_exchanges_the_bits_in_one_launch(monkeypatch):
    from weatherconverter_amd import _native
    from weatherconverter_amd import kernels as K
    g = _gen(7)
    special = torch.tensor([0x7fc00000, 0x7fc00001, -0x3ed432, 0x7f800001, -0x80000000, 0, 0x7f800000, -0x800000, 1,
                            -0x7fffffff], dtype=torch.int32)  # NaNs with payloads, -0.0, 0.0, infinities, subnormals
    vals = []
    for _ in range(2):
        ts = [torch.randint(-2**31, 2**31, (n, ), generator=g, dtype=torch.int64).to(torch.int32) for n, _, _ in CARVE]
        for t in ts:  # the specials first and last, wherever they fit
            k = min(len(special), t.numel())
            t[:k] = special[:k]
            t[t.numel() - k:] = special[:k]
        vals.append([t.view(torch.float32) for t in ts])
    s0, p0 = vals
    assert any(torch.isnan(t).any() for t in s0) and (_bits(s0[-1]) == -2**31).any()
    cv = Carved(s0, p0)
    calls = {}
    real = _native.call

    def counting(name, *args):
        calls[name] = calls.get(name, 0) + 1
        return real(name, *args)
    monkeypatch.setattr(_native, 'call', counting)
    jobs = K.ema_jobs(cv.ss, cv.ps)
    K.ema_swap(jobs)
    assert calls == {'wc_ema_swap': 1}  # the whole table in one launch
    for c, s, p, so, po in zip(CARVE, cv.ss, cv.ps, s0, p0):
        assert torch.equal(_bits(s).cpu(), _bits(po)) and torch.equal(_bits(p).cpu(), _bits(so)), c
    cv.assert_sentinels_intact()
    K.ema_swap(jobs)
    assert calls == {'wc_ema_swap': 2}
    for c, s, p, so, po in zip(CARVE, cv.ss, cv.ps, s0, p0):
        assert torch.equal(_bits(s).cpu(), _bits(so)) and torch.equal(_bits(p).cpu(), _bits(po)), c
    cv.assert_sentinels_intact()
    calls.clear()
    K.ema_update(jobs, 0.5)
    assert calls == {'wc_ema_update': 1}


def test_many_small_tensors_are_all_reached_in_one_launch(monkeypatch):
    """The bisect over a table the size of the 256-px model's (358 rows), one workgroup per tensor mostly."""
    from weatherconverter_amd import _native
    from weatherconverter_amd import kernels as K
    g = _gen(3)
    sizes = [1 + (37 * i) % 200 for i in range(357)] + [5000]
    ss = [torch.randn(n, generator=g).cuda() for n in sizes]
    ps = [torch.randn(n, generator=g).cuda() for n in sizes]
    s0, p0 = [s.clone() for s in ss], [p.clone() for p in ps]
    calls = []
    real = _native.call
    monkeypatch.setattr(_native, 'call', lambda name, *a: (calls.append(name), real(name, *a))[1])
    jobs = K.ema_jobs(ss, ps)
    K.ema_update(jobs, 0.75)
    assert calls == ['wc_ema_update']
    for s, a, p, b in zip(ss, s0, ps, p0):
        # scaling by 0.25 is exact: one rounding of the difference, one of the sum, each below
        # 2^-24 (|a| + |b|)
        err = (s.double() - ema_f64(a, b, 0.75)).abs()
        assert bool((err <= 2.0**-23 * (a.double().abs() + b.double().abs())).all()), s.numel()
        assert not torch.equal(s, a) and torch.equal(p, b)
    after = [s.clone() for s in ss]
    K.ema_swap(jobs)
    assert calls == ['wc_ema_update', 'wc_ema_swap']
    assert all(torch.equal(_bits(p), _bits(a)) for p, a in zip(ps, after))  # every row changed places
    assert all(torch.equal(_bits(s), _bits(b)) for s, b in zip(ss, p0))


# --------------------------------------------------------------------------------------- 4: envelope
def test_operands_outside_the_kernels_envelope_raise():
    from weatherconverter_amd import kernels as K
    ok = torch.randn(8, 6).cuda()
    with pytest.raises(RuntimeError, match='contiguous'):
        K.ema_jobs([torch.randn(6, 8).cuda().t()], [ok])
    with pytest.raises(RuntimeError, match='contiguous'):
        K.ema_jobs([ok.clone()], [torch.randn(6, 8).cuda().t()])
    with pytest.raises(RuntimeError, match='fp32'):
        K.ema_jobs([ok.clone()], [ok.half()])
    with pytest.raises(RuntimeError, match='fp32'):
        K.ema_jobs([ok.half()], [ok])
    with pytest.raises(RuntimeError, match='non-empty'):
        K.ema_jobs([torch.empty(0).cuda()], [torch.empty(0).cuda()])
    with pytest.raises(RuntimeError, match='fp32 tensor on'):
        K.ema_jobs([torch.randn(8, 6)], [ok])
    with pytest.raises(RuntimeError, match='fp32 tensor on'):
        K.ema_jobs([ok.clone()], [torch.randn(8, 6)])
    with pytest.raises(RuntimeError, match='shaped as'):
        K.ema_jobs([torch.randn(48).cuda()], [ok])
    buf = torch.randn(100).cuda()
    with pytest.raises(RuntimeError, match='overlaps'):
        K.ema_jobs([buf[0:60]], [buf[40:100]])
    with pytest.raises(RuntimeError, match='overlaps'):
        K.ema_jobs([ok], [ok])
    K.ema_jobs([buf[0:50]], [buf[50:100]])  # adjacent is not overlapping
    with pytest.raises(RuntimeError, match='one shadow per parameter'):
        K.ema_jobs([], [])
    jobs = K.ema_jobs([ok.clone()], [ok])
    for bad in (-0.1, 1.5, float('nan')):
        with pytest.raises(RuntimeError, match='decay'):
            K.ema_update(jobs, bad)


# --------------------------------------------------------------------------------------- 5-7: tiny UNet
ITERS = 3


def _tiny():
    from weatherconverter_amd.diffusion_model.config import ModelConfig
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    from weatherconverter_amd.synthetic import init_synthetic_
    man = json.load(open(os.path.join(GOLDEN, 'manifest.json')))
    mc = ModelConfig(**man['tiny']['config'])
    net = Unet(mc)
    init_synthetic_(net, seed=0)
    g = _gen(5)
    x = torch.randn((2, 3, 32, 32), generator=g).cuda()
    noise = torch.randn((2, 3, 32, 32), generator=g).cuda()
    t = torch.tensor([5, 700]).cuda()
    return mc, net.cuda().train(), x, noise, t


def _fresh(mc, state):
    from weatherconverter_amd.diffusion_model.models.unet_base import Unet
    other = Unet(mc)
    other.load_state_dict({k: v.detach().clone().cpu() for k, v in state.items()})
    return other.cuda()


@pytest.fixture(scope='module')
def trained():
    """ITERS iterations of the reference loop on the tiny UNet at 32 px, B = 2, with two averages riding
    along (the default decay, and 0.9 with warmup); the parameters are snapshot after every step."""
    from types import SimpleNamespace
    from weatherconverter_amd.diffusion_model import train_ddpm
    mc, net, x, noise, t = _tiny()
    opt = train_ddpm.make_optimizer(net, SimpleNamespace(training=SimpleNamespace(lr=1e-3)))
    emas = {'default': train_ddpm.make_ema(net), 'warm': train_ddpm.make_ema(net, 0.9, warmup=True)}
    start = [p.detach().clone().cpu() for p in net.parameters()]
    snaps = []
    for _ in range(ITERS):
        opt.zero_grad()
        torch.nn.MSELoss()(net(x, t), noise).backward()
        opt.step()
        for e in emas.values():
            e.update()
        snaps.append([p.detach().clone().cpu() for p in net.parameters()])
    return SimpleNamespace(mc=mc, net=net, x=x, noise=noise, t=t, opt=opt, emas=emas, start=start, snaps=snaps)


@pytest.mark.parametrize('which', ['default', 'warm'])
def test_tiny_unet_loop_under_the_yardstick(trained, which):
    ema = trained.emas[which]
    assert ema.num_updates == ITERS
    assert list(ema.shadow) == [n for n, _ in trained.net.named_parameters()]
    theirs = [s.clone().cuda() for s in trained.start]
    ref = [s.double() for s in trained.start]
    for k, snap in enumerate(trained.snaps, 1):
        d = ema.decay_at(k)
        for s, p in zip(theirs, snap):
            s.lerp_(p.cuda(), 1.0 - d)
        ref = [ema_f64(s, p, d) for s, p in zip(ref, snap)]
    assert [ema.decay_at(k) for k in (1, 2, 3)] == ([0.9999] * 3 if which == 'default' else [2 / 11, 3 / 12, 4 / 13])
    assert_yardstick(list(ema.shadow.values()), theirs, ref, trained.start, f'tiny UNet[{which}]')
    assert all(not s.requires_grad and s.is_cuda and s.dtype == torch.float32 for s in ema.shadow.values())


def test_swapped_forward_runs_on_the_average(trained):
    """The stale-pack test: the engines cache packed weights keyed on the parameters' version counters and
    wc_ema_swap writes through raw addresses -- without swap()'s version bump a forward inside the context
    would silently run on the packs of the raw weights, and one after it on the average's."""
    mc, net, x, t, ema = trained.mc, trained.net, trained.x, trained.t, trained.emas['warm']
    raw_bits = [_bits(p).clone() for p in net.parameters()]
    avg_bits = [_bits(s).clone() for s in ema.shadow.values()]
    assert any(not torch.equal(a, b) for a, b in zip(raw_bits, avg_bits))
    try:
        for mode in ('eval', 'train'):  # the inference engine, then the training engine
            def fwd(m):
                if mode == 'eval':
                    with torch.no_grad():
                        return m.eval()(x, t)
                return m.train()(x, t).detach()
            first = fwd(net)  # the packs of the raw weights exist
            want = fwd(_fresh(mc, ema.shadow_state_dict()))
            versions = [p._version for p in net.parameters()]
            with ema.swapped() as inside:
                assert inside is ema
                assert all(p._version > v for p, v in zip(net.parameters(), versions))
                out = fwd(net)
                assert torch.equal(out, want), mode
                assert not torch.equal(out, first), mode
                # the model IS the average and the shadow holds the raw weights
                assert all(torch.equal(_bits(p), b) for p, b in zip(net.parameters(), avg_bits))
                assert all(torch.equal(_bits(s), b) for s, b in zip(ema.shadow.values(), raw_bits))
                with pytest.raises(RuntimeError, match='swapped'):
                    ema.update()
                with pytest.raises(RuntimeError, match='swapped'):
                    ema.state_dict()
            assert torch.equal(fwd(net), first), mode
        n = ema.num_updates
        with pytest.raises(KeyError, match='boom'):
            with ema.swapped():
                raise KeyError('boom')
        assert ema.num_updates == n
        assert all(torch.equal(_bits(p), b) for p, b in zip(net.parameters(), raw_bits))  # swapped back
        assert all(torch.equal(_bits(s), b) for s, b in zip(ema.shadow.values(), avg_bits))
        ema.state_dict()  # and usable again
    finally:
        net.train()


def test_checkpoint_carries_the_average(trained, tmp_path):
    from weatherconverter_amd.diffusion_model import sample_ddpm, train_ddpm
    mc, net, x, t, ema = trained.mc, trained.net, trained.x, trained.t, trained.emas['warm']
    path = train_ddpm.save_checkpoint(3, net, trained.opt, str(tmp_path), ema=ema)
    try:
        with torch.no_grad():
            raw = net.eval()(x, t)
            with ema.swapped():
                avg = net.eval()(x, t)
            loaded = sample_ddpm.load_model(path, mc, weights='ema')
            assert not loaded.training and torch.equal(loaded(x, t), avg)
            assert torch.equal(sample_ddpm.load_model(path, mc)(x, t), raw)  # the default is the raw weights
            assert not torch.equal(raw, avg)
    finally:
        net.train()
    # into a fresh EMA (over a model with other weights): the count, the schedule and the shadow's bits
    net2 = _fresh(mc, {k: torch.zeros_like(v) for k, v in net.state_dict().items()})
    ema2 = train_ddpm.make_ema(net2)
    _, _, epoch = train_ddpm.load_checkpoint(net2, None, path, ema=ema2)
    assert epoch == 3 and ema2.num_updates == ITERS and ema2.decay == 0.9 and ema2.warmup is True
    for (n, s), s2 in zip(ema.shadow.items(), ema2.shadow.values()):
        assert s2.is_cuda and torch.equal(_bits(s), _bits(s2)), n
    # a file saved without ema= names the missing key
    three = train_ddpm.save_checkpoint(4, net, trained.opt, str(tmp_path))
    with pytest.raises(RuntimeError, match='ema_state_dict'):
        sample_ddpm.load_model(three, mc, weights='ema')
    with pytest.raises(RuntimeError, match='ema_state_dict'):
        train_ddpm.load_checkpoint(net2, None, three, ema=ema2)
