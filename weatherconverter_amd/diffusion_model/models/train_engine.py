"""TrainEngine: the reference ``Unet`` training step's forward (with saved activations) and its
backward, as gfx950 HIP kernels — ``loss.backward()`` of ``train_ddpm.py:106-110``.

Forward (same layout as ``UnetEngine``: NHWC fp32 activations, one skip buffer ``U[i]`` per level so
the up path's ``torch.cat`` is free) records a tape; every GroupNorm keeps both its affine
(scale, shift) and the plain normalisation (rstd, -mean*rstd) so the backward recomputes
SiLU(GN(x)) from the stored pre-norm tensor instead of keeping the activation.  Attention keeps its
pre-residual input, q/k/v, its output and the softmax log-sum-exp.

Backward, per layer type (reference modules of unet_base.py):
  Conv2d 3x3 / 1x1 / 4x4-s2, ConvTranspose2d 4x4-s2, in/out projections
      data gradient   the forward kernels on re-packed weights: a 3x3 conv's is the 3x3 conv of dY
                      with W flipped and transposed (halo kernel); a 4x4/s2 conv's is the transposed
                      conv of dY (four parity sub-convs); a transposed conv's is the 4x4/s2 conv of
                      dY with its own weight; a linear layer's is dY W.
      weight gradient wc_conv_wgrad3 (3x3: halo-tiled) or wc_conv_wgrad (GEMM over the pixels), the
                      input re-read through the forward's taps and GN prologue; split partials
                      reduced in a fixed order and scattered into the parameter's layout.
      bias            per-(b, c) pixel sums, summed over b in a fixed order.
  GroupNorm(+SiLU)    wc_gn_bwd_* (dx, dgamma, dbeta).
  attention core      wc_attention_bwd_f16x3 / _bwd6 / _bwd (dq, dk, dv from lse; no N x N matrix).
  time embedding MLP  small GEMM / SiLU kernels (B x 128).
Arithmetic (precision f16x3, the default): forward convs, projections and attention on f16x3 under
the sampler's static bounds; 3x3 and projection data gradients, the 3x3 weight gradients and the
attention backward on f16x3 under per-image range bounds of the gradients, which every kernel
writing a gradient tensor raises as it writes (_gb); the rest on bf16x6 (exact 3-piece bf16 split).
Precision bf16x6 / fp32: bf16x6 / fp32 MFMA throughout.  fp32-class gradients, checked against
PyTorch autograd of the reference restatement in float64.  Every gradient buffer is written in a
fixed order: results are deterministic run to run.
"""
from dataclasses import dataclass, field
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

from ... import forms
from ... import kernels as K
from ...kernels import Seg, View
from .engine import TAPS1, TAPS3, TAPS4S2, UnetEngine, check_supported, pack_conv, pack_convT

_PARITIES = ((0, 0), (0, 1), (1, 0), (1, 1))


def _f32(p: torch.Tensor) -> torch.Tensor:
    """A parameter as the fp32 tensor the kernels read (no copy when it already is one)."""
    return p.detach().float()


def _one_image_tiles(H: int, W: int, C: int) -> bool:
    """The implicit GEMM's M tiles (kernels.igemm_bm of C) lie inside one image each: a per-image A bound holds."""
    return (H * W) % (256 if C <= 64 else 128) == 0


class ConvForms:
    """One conv's weight in every form the training step can launch, named as engine.ConvPack / UpPack name
    them.  A form is given as a builder fn(this record), run (under no_grad) on first read and cached: a
    training step packs only the forms it launches (the f16x3 data-gradient packs, not also the bf16x6 ones;
    packing is host-launched work on every step).  A builder may read another form (a ResBlock conv's packs
    all read its re-layout w), which is then built once.  A form assigned ahead of time (c.wn = pack) is kept."""
    # w [N][K] fp32 (wc_conv_igemm), x6 (wc_conv_igemm_x6), f3 / f3h f16x3 in natural / halo order, wn Winograd,
    # f3s space-to-depth 4x4/s2, f3t one-launch ConvT, parts its four parities as (taps, ConvForms).  A builder
    # gets the record as its argument instead of closing over it, so a record is no reference cycle and a
    # step's packs are freed as soon as the next step's replace them.
    FORMS = ('w', 'x6', 'f3', 'f3h', 'wn', 'f3s', 'f3t', 'parts')

    def __init__(self, **builders: Optional[Callable]):  # None: the conv does not have that form
        assert set(builders) <= set(self.FORMS), sorted(builders)
        self._builders = {k: fn for k, fn in builders.items() if fn is not None}

    def has(self, form: str) -> bool:
        """Whether the conv was given this form, without building it."""
        assert form in self.FORMS, form
        return form in self.__dict__ or form in self._builders

    def __getattr__(self, form: str):  # reached only while `form` is not built (not in __dict__)
        fn = self.__dict__.get('_builders', {}).get(form)
        if fn is None:
            raise AttributeError(f'ConvForms: this conv was not given form {form!r}')
        with torch.no_grad():
            v = fn(self)
        setattr(self, form, v)
        return v


@dataclass
class ResTrain:
    """A ResBlock: conv1, conv2 (+ the 1x1 residual as in engine.ResPack) and their data gradients d1, d2
    (the 3x3 conv with W flipped and transposed) and dr (the residual's: dY W)."""
    ci: int
    co: int
    off: int  # first column of this block's time-embedding projection in temb / dproj
    gn1: torch.nn.Module
    gn2: torch.nn.Module
    mod1: torch.nn.Module
    mod2: torch.nn.Module
    modr: torch.nn.Module
    temb: torch.nn.Module
    b2: torch.Tensor  # conv2's bias + the residual conv's
    conv1: ConvForms
    conv2: ConvForms
    d1: ConvForms
    d2: ConvForms
    dr: ConvForms
    wino_raw: List[Tuple[ConvForms, tuple]]  # the kernels.pack_wino_raw request of every wn form (forms.pack_raw)
    gb1: Tuple[float, float] = (0.0, 0.0)  # (max|gamma|, max|beta|) of gn1 / gn2, on the host (_pack)
    gb2: Tuple[float, float] = (0.0, 0.0)


@dataclass
class AttnTrain:
    C: int
    heads: int
    gn: torch.nn.Module
    mha: torch.nn.Module
    proj_in: ConvForms  # f3: under the GN bound
    proj_out: ConvForms  # f3: under the V bound
    d_in: ConvForms  # the projections' data gradients (dY W); f3: under per-image absmax bounds
    d_out: ConvForms
    qkv_l1: Optional[torch.Tensor] = None  # f16x3: host row-L1 norms of W_in and |b_in| (bounds)
    qkv_babs: Optional[torch.Tensor] = None
    gb: Tuple[float, float] = (0.0, 0.0)


@dataclass
class ScaleTrain:
    """A 4x4 / stride-2 Conv2d (down) or ConvTranspose2d (up) and its data gradient, the other of the two on the
    same weight.  The conv: w / x6 / f3s; the transposed conv: f3t / parts ((taps, ConvForms) per output parity)."""
    mod: torch.nn.Module
    fwd: ConvForms
    dgrad: ConvForms


@dataclass
class HeadTrain:
    small: bool  # the fp32 VALU head kernels (forms.train_smallconv) instead of the implicit GEMMs
    w: torch.Tensor  # conv_out's weight as the forward read it (wc_head_dgrad)
    wp: Optional[torch.Tensor] = None  # small: kernels.pack_head
    fwd: Optional[ConvForms] = None  # not small: the conv, and its data gradient over the 32-channel
    dgrad: Optional[ConvForms] = None  # padded loss gradient


class ConvInRec(NamedTuple):
    x: torch.Tensor
    out: View


class ResRec(NamedTuple):
    X: View
    h: View
    Y: View
    rp: ResTrain
    st1: tuple  # gn1's (scale, shift, rstd, -mean*rstd, per-image bound of |X|)
    st2: tuple


class AttnRec(NamedTuple):
    Ypre: View
    Yout: View
    qkv: torch.Tensor
    o: torch.Tensor
    lse: torch.Tensor
    st: tuple
    ap: AttnTrain


class DownRec(NamedTuple):
    cur: View
    out: View
    sp: ScaleTrain
    bcur: Optional[torch.Tensor]  # the forward's per-image max |cur|


class UpRec(DownRec):
    """The same fields for a ConvTranspose."""


class HeadRec(NamedTuple):
    cur: View
    st: tuple
    hp: HeadTrain


@dataclass
class Tape:
    """Everything one training forward saved for its backward: the layer records in forward order
    (activations, GN statistics, that forward's packed weights; ConvInRec first, HeadRec last) plus the
    timesteps and the time-embedding packs.  One per forward, owned by that forward's autograd node,
    consumed by exactly one backward; the engine keeps nothing of a forward but last_tape."""
    tt: torch.Tensor
    P: int
    tproj: List[torch.Tensor]
    temb_w: torch.Tensor
    res_rows: List[ResTrain]
    records: list = field(default_factory=list)
    raised: Dict[int, bool] = field(default_factory=dict)  # forward only: the bounds (_zrow) a kernel raised
    consumed: bool = False


class TrainEngine:

    def __init__(self, model, precision: Optional[str] = None):
        params = list(model.parameters())
        if not params or not params[0].is_cuda:
            raise RuntimeError('weatherconverter_amd.Unet trains on the GPU only (HIP kernels, no CPU fallback)')
        p = (precision or getattr(model, 'train_precision', None) or getattr(model, 'conv_precision', None)
             or K.default_conv_precision())
        check_supported(model.model_config, p, training=True)
        K._native.load()
        self.model = model
        self.device = params[0].device
        # 'f16': the 16-bit training line — the f16x3 arithmetic of mode f16x3 run on the single-piece
        # build (one fp16 piece per operand: wc_x6.hpp mfma_f16c), every kernel call routed to it
        # 'bf16': the same on the bf16 single-piece build (one bf16 piece per operand on the bf16 MFMA:
        # BASELINE config 3's bf16 training)
        self.variant = {'f16': 'single16', 'bf16': 'bf16'}.get(p, '')
        if p in ('f16', 'bf16'):
            p = 'f16x3'
        # f16x3 needs range bounds that gradients do not have: the backward runs bf16x6; the forward's
        # GroupNorm-prologue convs and projections run f16x3 under their static bounds (as inference)
        self.precision = 'fp32' if p == 'fp32' else 'bf16x6'
        self.f3 = p == 'f16x3'
        # data gradients on f16x3 under per-image absmax bounds of the incoming gradient (mode f16x3)
        self.f3d = self.f3 and forms.current().dgrad_f16x3
        self.last_tape: Optional[Tape] = None

    # ------------------------------------------------------------------ packing (per step)
    def _igemm(self, w2d: Callable, C0: int, ntaps: int, C1: int = 0, **more) -> ConvForms:
        """An implicit-GEMM conv: w = w2d(), the [N][ntaps*C0 + C1] weight (pack_conv), and on bf16x6 its x6
        pack; more: the builders of its other forms."""
        x6 = self.precision == 'bf16x6' and C0 % 16 == 0 and C1 % 16 == 0

        def w(c):
            if not x6 and (C0 % 32 or C1 % 32):
                raise RuntimeError(f'fp32 implicit GEMM needs channel counts % 32 (got {C0}, {C1})')
            return w2d().contiguous().float()

        return ConvForms(w=w, x6=(lambda c: K.pack_x6(c.w, C0, C1, ntaps=ntaps, order='natural')) if x6 else None,
                         **more)

    def _igemm_now(self, w2d: torch.Tensor, C0: int, ntaps: int) -> ConvForms:
        """_igemm of a weight at hand, packed now and not at its first launch."""
        c = self._igemm(lambda: w2d, C0, ntaps)
        _ = c.x6 if c.has('x6') else c.w
        return c

    def _parts(self, wt: torch.Tensor, C0: int):
        """The four output parities of the ConvTranspose with weight wt as implicit-GEMM convs: the
        `parts` form, all four packed before the first is launched."""
        return [(taps, self._igemm_now(wp, C0, len(taps)))
                for taps, wp in (pack_convT(wt, py, px) for py, px in _PARITIES)]

    def _conv(self, segs, c: ConvForms, bias, out: Optional[View], H: int, W: int, **kw):
        if kw.get('absmax', 0) is None:  # no bound tracked (outside the f16x3 backward)
            kw.pop('absmax')
        if c.has('x6'):
            K.conv_igemm_x6(segs, c.x6, bias, out, Hm=H, Wm=W, **kw)
        else:
            K.conv_igemm(segs, c.w, bias, out, Hm=H, Wm=W, **kw)

    def _pack_res(self, blk, i: int, off: int) -> ResTrain:
        f, s, r = blk.resnet_conv_first[i], blk.resnet_conv_second[i], blk.residual_input_conv[i]
        w1, w2, wr = f[2].weight.detach(), s[2].weight.detach(), r.weight.detach()
        ci, co = w1.shape[1], w1.shape[0]
        wr2 = wr.reshape(co, ci)
        f3, f3d = self.f3 and ci % 16 == 0 and co % 16 == 0, self.f3d
        wino = forms.current().wino
        raw = all(t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in (w1, w2)) \
            and 9 * (max(ci, co) + 4) * 4 <= 64 * 1024 and forms.current().pack_raw
        # w: the re-layout every other form of the conv is packed from, built once and only if one of them
        # is (the Winograd forms usually replace the direct f16x3 ones, and pack from the module weights
        # directly when those are fp32 on the device: no host re-layout)
        conv1 = self._igemm(
            lambda: pack_conv(w1), ci, 9, f3h=(lambda c: K.pack_f16x3(c.w, ci)) if f3 else None,
            wn=(lambda c: K.pack_wino_raw(w1) if raw else K.pack_wino(c.w, ci)) if f3 and wino else None)
        conv2 = self._igemm(
            lambda: torch.cat([pack_conv(w2), wr2], 1), co, 9, ci,
            f3h=(lambda c: K.pack_f16x3(c.w, co, ci, res_f16=True)) if f3 else None,
            wn=(lambda c: K.pack_wino_raw(w2, wr2.float().contiguous()) if raw else K.pack_wino(c.w, co, ci))
            if f3 and wino else None)

        def dgrad(w, wn: bool):  # f16x3 forms: the raw gradient operand under its per-image absmax bound
            return self._igemm(
                lambda: pack_conv(w.flip([2, 3]).transpose(0, 1)), co, 9,
                f3h=(lambda c: K.pack_f16x3(c.w, co)) if f3d else None,
                wn=(lambda c: K.pack_wino_raw(w, transposed=True) if raw else K.pack_wino(c.w, co)) if wn else None)

        d1 = dgrad(w1, f3d and wino and ci % 16 == 0 and co % 16 == 0)
        d2 = dgrad(w2, f3d and wino and co % 16 == 0)
        dr = self._igemm(lambda: wr2.t(), co, 1,
                         f3=(lambda c: K.pack_f16x3(c.w, co, ntaps=1, order='natural')) if f3d else None)
        want = ((conv1, (w1, None, False)), (conv2, (w2, wr2.float().contiguous(), False)),
                (d1, (w1, None, True)), (d2, (w2, None, True))) if raw else ()
        return ResTrain(ci, co, off, f[0], s[0], f[2], s[2], r, blk.t_emb_layers[i][1],
                        _f32(s[2].bias + r.bias).contiguous(), conv1, conv2, d1, d2, dr,
                        [(c, req) for c, req in want if c.has('wn')])

    def _pack_attn(self, blk, i: int) -> AttnTrain:
        mha, gn = blk.attentions[i], blk.attention_norms[i]
        C = mha.embed_dim
        w_in, w_out = mha.in_proj_weight.detach(), mha.out_proj.weight.detach()
        f3d = self.f3d and C % 16 == 0  # projection data gradients on f16x3 (per-image absmax bounds)

        def dgrad(w, C0: int):
            return self._igemm(lambda: w.t(), C0, 1,
                               f3=(lambda c: K.pack_f16x3(c.w, C0, ntaps=1, order='natural')) if f3d else None)

        ap = AttnTrain(C, mha.num_heads, gn, mha, self._igemm(lambda: w_in, C, 1), self._igemm(lambda: w_out, C, 1),
                       dgrad(w_in, 3 * C), dgrad(w_out, C))
        if self.f3 and C % 16 == 0:  # every forward launches these two
            ap.proj_in.f3 = K.pack_f16x3(w_in.float(), C, ntaps=1, order='natural')
            ap.proj_out.f3 = K.pack_f16x3(w_out.float(), C, ntaps=1, order='natural')
        return ap

    def _pack_down(self, conv) -> ScaleTrain:
        w = conv.weight.detach()
        co, ci = w.shape[0], w.shape[1]
        f3 = self.f3 and ci % 16 == 0 and co % 16 == 0 and K.x6_tile(co)[1] == 128
        # f16x3 halo forms: the forward on the space-to-depth kernel, the data gradient (the ConvT of dY,
        # in = Co, with the same weight) on the one-launch ConvT kernel
        return ScaleTrain(
            conv, self._igemm(lambda: pack_conv(w), ci, 16, f3s=(lambda c: K.pack_f16x3_s2d(c.w, ci)) if f3 else None),
            ConvForms(parts=lambda c: self._parts(w, co),
                      f3t=(lambda c: K.pack_f16x3_convT(w.float())) if self.f3d and f3 else None))

    def _pack_up(self, conv) -> ScaleTrain:
        wt = conv.weight.detach()  # [Cin][Cout][4][4]
        ci, co = wt.shape[0], wt.shape[1]
        f3 = self.f3 and ci % 16 == 0 and co % 16 == 0
        return ScaleTrain(
            conv, ConvForms(parts=lambda c: self._parts(wt, ci),
                            f3t=(lambda c: K.pack_f16x3_convT(wt.float())) if f3 else None),
            self._igemm(lambda: pack_conv(wt), co, 16, f3s=(lambda c: K.pack_f16x3_s2d(c.w, co))
                        if self.f3d and f3 and K.x6_tile(ci)[1] == 128 else None))

    def _pack(self):
        m = self.model
        self.P = 0

        def stage(blk, n_res):
            res = []
            for i in range(n_res):
                res.append(self._pack_res(blk, i, self.P))
                self.P += res[-1].co
            att = [self._pack_attn(blk, i) for i in range(len(blk.attentions))] if blk.use_attn else []
            return res, att

        with torch.no_grad():
            self.downs = [stage(blk, blk.num_layers) for blk in m.downs]
            self.mids = [stage(blk, blk.num_layers + 1) for blk in m.mids]
            self.ups = [stage(blk, blk.num_layers) for blk in m.ups]
            self.down_pk = [self._pack_down(blk.down_sample_conv) if blk.down_sample else None for blk in m.downs]
            self.up_pk = [self._pack_up(blk.up_sample_conv) if blk.up_sample else None for blk in m.ups]
            tp = m.t_proj
            self.tproj = [_f32(p).contiguous() for p in (tp[0].weight, tp[0].bias, tp[2].weight, tp[2].bias)]
            stages = self.downs + self.mids + self.ups
            rows = [rp for st in stages for rp in st[0]]
            # every ResBlock's Winograd packs (forward and data-gradient forms; the weights change each
            # step) in one launch instead of one each (forms.pack_batch off: built lazily one by one)
            if forms.current().pack_batch:
                reqs = [cr for rp in rows for cr in rp.wino_raw]
                for (c, _), pk in zip(reqs, K.pack_wino_raw_batch([r for _, r in reqs])):
                    c.wn = pk
            # the f16x3 bounds: every layer's reduced on the device (the GroupNorm affines' max |.| in one
            # multi-tensor launch; inf norm: exact), then ONE transfer, one host sync per training forward
            f3a = [ap for st in stages for ap in st[1] if ap.proj_in.has('f3')]
            gns = [g for rp in rows for g in (rp.gn1, rp.gn2)] + [ap.gn for ap in f3a]
            vecs = [v for ap in f3a for v in (ap.mha.in_proj_weight.detach().double().abs().sum(1),
                                              ap.mha.in_proj_bias.detach().double().abs())]
            gmax = torch._foreach_norm([p.detach() for g in gns for p in (g.weight, g.bias)], float('inf'))
            host = torch.cat(vecs + [torch.stack(gmax).double()]).cpu()
            i = 0
            for ap in f3a:
                n = 3 * ap.C
                ap.qkv_l1, ap.qkv_babs = host[i:i + n], host[i + n:i + 2 * n]
                i += 2 * n
            gb = [tuple(p) for p in host[i:].view(-1, 2).tolist()]
            for k, rp in enumerate(rows):
                rp.gb1, rp.gb2 = gb[2 * k], gb[2 * k + 1]
            for ap, p in zip(f3a, gb[2 * len(rows):]):
                ap.gb = p
            self.temb_w = torch.cat([_f32(rp.temb.weight) for rp in rows], 0).contiguous()
            self.temb_b = torch.cat([_f32(rp.temb.bias) for rp in rows], 0).contiguous()
            self.res_rows = rows
            co = m.conv_out.weight.detach()  # [NO][C][3][3]
            NO, C = co.shape[0], co.shape[1]
            # the 3-channel head on its fp32 VALU kernels (wc_head_conv forward, wc_head_wgrad /
            # wc_head_dgrad backward): an MFMA tile pads its 3 channels 20x (forms.train_smallconv off:
            # the generic implicit GEMMs, kept for A/B)
            if forms.current().train_smallconv and NO == 3 and C in (32, 64):
                self.head = HeadTrain(True, co, wp=K.pack_head(co))
            else:
                wt = torch.zeros((C, 32, 3, 3), dtype=torch.float32, device=self.device)
                wt[:, :NO] = co.flip([2, 3]).transpose(0, 1)
                self.head = HeadTrain(False, co, fwd=self._igemm_now(pack_conv(co), C, 9),
                                      dgrad=self._igemm_now(pack_conv(wt), 32, 9))

    # ------------------------------------------------------------------ helpers
    def _new(self, B, H, W, C) -> torch.Tensor:
        return torch.empty((B, H, W, C), dtype=torch.float32, device=self.device)

    def _new_gn(self, B, H, W, C) -> torch.Tensor:
        """A forward activation that also carries GroupNorm tile partials (kernels.GnPart), filled by its
        producer's epilogue when that is a split-precision conv, so its GroupNorm needs no stats pass."""
        t = self._new(B, H, W, C)
        sw = UnetEngine._sw(C)
        if sw is not None and K.GnPart.eligible(t) and forms.current().train_gn_partials:
            K.GnPart.attach(t, sw)
        return t

    def _zrow(self, B: int, n: int = 1) -> torch.Tensor:
        """A zeroed float32[B] on the device (a per-image bound that writers raise): rows of one pooled
        zero fill instead of a fill launch each; n > 1: n rows as one float32[n * B].  A row is never
        handed out twice."""
        pool = getattr(self, '_zpool', None)
        if pool is None or pool.shape[1] != B or self._zi + n > pool.shape[0]:
            self._zpool = pool = torch.zeros((128, B), dtype=torch.float32, device=self.device)
            self._zi = 0
        self._zi += n
        return pool[self._zi - 1] if n == 1 else pool[self._zi - n:self._zi].view(-1)

    def _gview(self, v: View) -> View:
        """The gradient view of a forward view, allocated on first use but NOT yet zeroed: a gradient
        tensor stays unwritten ('fresh') until its first writer overwrites it whole (_grad_w) or
        something reads or accumulates into it (_grad zeroes it then)."""
        key = id(v.t)
        if key not in self.gmap:
            self.gmap[key] = (torch.empty_like(v.t), 0)
            self.gfresh.add(id(self.gmap[key][0]))
        g, off = self.gmap[key]
        return View(g, v.c0 + off, v.C)

    def _grad(self, v: View) -> View:
        """The gradient view of a forward view, zero-initialised if nothing has written it yet."""
        gv = self._gview(v)
        if id(gv.t) in self.gfresh:
            self.gfresh.discard(id(gv.t))
            gv.t.zero_()
        return gv

    def _grad_w(self, v: View) -> Tuple[View, bool]:
        """(gradient view, overwrite) for a writer that adds into it (a conv's res=, an accumulating GN
        backward): overwrite=True when the tensor is still unwritten and the view covers it whole, so the
        writer stores its values instead of adding them to a zero fill (no fill, no read of zeros)."""
        gv = self._gview(v)
        if id(gv.t) in self.gfresh and gv.c0 == 0 and gv.C == gv.t.shape[-1] \
                and forms.current().train_lazy_grad:
            self.gfresh.discard(id(gv.t))
            return gv, True
        return self._grad(v), False

    def _alias_grad(self, t: torch.Tensor, v: View):
        """The full tensor t's gradient IS the gradient of view v (t feeds v through an identity path
        and everything else adds into it afterwards in backward order)."""
        g = self._gview(v)
        self.gmap[id(t)] = (g.t, g.c0)
        self.keep.append(t)

    def _gb(self, v: View) -> Optional[torch.Tensor]:
        """The range bound of v's gradient tensor for the f16x3 backward: float32[B], raised by EVERY
        kernel that writes into that tensor to the max |value| it wrote per image (so it bounds the
        final values), zero while nothing has; None outside the f16x3 backward."""
        if not self.f3d:
            return None
        g = self._gview(v)
        t = self.gbnd.get(id(g.t))
        if t is None:
            t = self._zrow(v.B)
            self.gbnd[id(g.t)] = t
        return t

    def _bound(self, v: View, tracked: Optional[torch.Tensor]) -> torch.Tensor:
        """The per-image bound a consumer uses: the writers' tracked bound (forms.check_gbound: checked
        against a fresh absmax of the view, which it must not be below)."""
        if tracked is None:
            return K.absmax_images(v)
        if forms.current().check_gbound:
            real = K.absmax_images(v)
            if bool((real > tracked).any()):
                raise RuntimeError(f'gradient range bound below the values: {tracked.tolist()} < {real.tolist()}')
        return tracked

    def _pgrad(self, p: torch.nn.Parameter) -> torch.Tensor:
        """p's gradient: a view into one zeroed buffer holding every parameter's (one fill per backward
        instead of one per parameter)."""
        g = self.pgrads.get(id(p))
        if g is None:
            o, n = self.pflat_off[id(p)]
            g = self.pflat[o:o + n].view(p.shape)
            self.pgrads[id(p)] = g
        return g

    # ------------------------------------------------------------------ forward
    def forward(self, x: torch.Tensor, t) -> torch.Tensor:
        with K._native.variant(self.variant):
            return self._forward(x, t)

    def _forward(self, x: torch.Tensor, t) -> torch.Tensor:
        m = self.model
        self._pack()
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, S, S2 = x.shape
        tt = torch.as_tensor(t).long().reshape(-1).to(self.device)
        if tt.numel() == 1 and B > 1:
            tt = tt.expand(B).contiguous()
        if tt.numel() != B:
            raise RuntimeError(f'timestep tensor has {tt.numel()} entries for a batch of {B}')
        tape = Tape(tt, self.P, self.tproj, self.temb_w, self.res_rows)
        temb = K.temb(tt, *self.tproj, self.temb_w, self.temb_b)  # (B, P)
        dc = m.down_channels
        L = len(dc) - 1
        sizes = [(S, S2)]
        for i in range(L):
            h, w = sizes[-1]
            sizes.append((h // 2, w // 2) if m.down_sample[i] else (h, w))
        U = [self._new(B, sizes[i][0], sizes[i][1], 2 * dc[i]) for i in range(L)]
        cur = View(U[0], dc[0], dc[0])
        K.conv_in(x, _f32(m.conv_in.weight).contiguous(), _f32(m.conv_in.bias).contiguous(), cur)
        tape.records.append(ConvInRec(x, cur))

        def block(X: View, tgt: View, rp, att, amx=None) -> View:
            """amx: float32[B] the final writer of tgt raises to its per-image max |value| (the bound a
            following down / up conv needs); left zero when that writer is not an f16x3 kernel."""
            if att is None:
                self._res_fwd(tape, X, tgt, rp, temb, amx)
            else:
                ypre = View.full(self._new_gn(B, X.H, X.W, rp.co))
                self._res_fwd(tape, X, ypre, rp, temb)
                self._attn_fwd(tape, ypre, tgt, att, amx)
            return tgt

        def new_amx():
            return self._zrow(B) if (self.f3 or self.f3d) else None

        def bound_of(v: View, amx):
            """The producer-raised bound when it was raised (nonzero), else a pass over v."""
            if amx is None:
                return None
            return amx if tape.raised.pop(id(amx), False) else K.absmax_images(v)

        for i in range(L):
            res, att = self.downs[i]
            dp = self.down_pk[i]
            H, W = sizes[i]
            final = View(U[i + 1], dc[i + 1], dc[i + 1]) if i < L - 1 else View.full(
                self._new(B, sizes[i + 1][0], sizes[i + 1][1], dc[i + 1]))
            amx = new_amx() if dp is not None else None
            for li, rp in enumerate(res):
                last = li == len(res) - 1
                tgt = final if (last and dp is None) else View.full(self._new_gn(B, H, W, rp.co))
                cur = block(cur, tgt, rp, att[li] if att else None, amx if last else None)
            if dp is not None:
                seg = Seg(cur, TAPS4S2, stride=2)
                bd = _f32(dp.mod.bias).contiguous()
                Hm, Wm = sizes[i + 1]
                f3s = dp.fwd.f3s if dp.fwd.has('f3s') else None  # packed here, also when the shape then declines it
                f3 = f3s is not None and K.conv4x4s2_f16x3_ok(seg, final.C, Hm, Wm)
                bcur = bound_of(cur, amx)  # the conv's A bound and the weight gradient's
                if f3:
                    K.conv4x4s2_f16x3(seg, f3s, bd, final, Hm=Hm, Wm=Wm, a_bound=bcur)
                else:
                    self._conv([seg], dp.fwd, bd, final, Hm, Wm)
                tape.records.append(DownRec(cur, final, dp, bcur))
                cur = final

        amx = None
        for j, (res, att) in enumerate(self.mids):
            last_mid = j == len(self.mids) - 1
            H, W = cur.H, cur.W
            for li, rp in enumerate(res):
                last = last_mid and li == len(res) - 1
                if last and self.up_pk[0] is None:
                    tgt = View(U[L - 1], 0, dc[L - 1])
                else:
                    tgt = View.full(self._new_gn(B, H, W, rp.co))
                if last and self.up_pk[0] is not None:
                    amx = new_amx()
                self._res_fwd(tape, cur, tgt, rp, temb, amx if last and li >= len(att) else None)
                cur = tgt
                if li < len(att):
                    nxt = View.full(self._new_gn(B, H, W, rp.co))
                    self._attn_fwd(tape, cur, nxt, att[li], amx if last else None)
                    cur = nxt

        for k, (res, att) in enumerate(self.ups):
            i = L - 1 - k
            H, W = sizes[i]
            up = self.up_pk[k]
            if up is not None:
                dst = View(U[i], 0, dc[i])
                b = _f32(up.mod.bias).contiguous()
                f3t = up.fwd.f3t if up.fwd.has('f3t') else None  # as f3s above
                f3 = f3t is not None and K.convT4x4s2_f16x3_ok(Seg(cur, [(0, 0)]), dst.C)
                bcur = bound_of(cur, amx)
                if f3:
                    K.convT4x4s2_f16x3(Seg(cur, [(0, 0)]), f3t, b, dst, a_bound=bcur)
                else:
                    for (py, px), (taps, c) in zip(_PARITIES, up.fwd.parts):
                        self._conv([Seg(cur, taps)], c, b, dst, cur.H, cur.W, out_map=(2, 2, py, px))
                tape.records.append(UpRec(cur, dst, up, bcur))
            else:
                assert cur.t is U[i] and cur.c0 == 0, 'non-upsampling level must have been written in place'
            cur = View.full(U[i])
            next_in_place = i > 0 and self.up_pk[k + 1] is None
            amx = new_amx() if k + 1 < len(self.ups) and self.up_pk[k + 1] is not None else None
            for li, rp in enumerate(res):
                last = li == len(res) - 1
                tgt = View(U[i - 1], 0, dc[i - 1]) if (last and next_in_place) else View.full(
                    self._new_gn(B, H, W, rp.co))
                cur = block(cur, tgt, rp, att[li] if att else None, amx if last else None)

        # head: GN -> SiLU -> conv_out, NCHW output
        gn, hp = m.norm_out, self.head
        sc, sh, a0, o0 = K.gn_stats_pair(cur, _f32(gn.weight), _f32(gn.bias), part=getattr(cur, '_wc_gn_done', None))
        out = torch.empty((B, m.model_config.im_channels, S, S2), dtype=torch.float32, device=self.device)
        if hp.small:
            K.head_conv(cur, sc, sh, hp.wp, _f32(m.conv_out.bias).contiguous(), out)
        else:
            self._conv([Seg(cur, TAPS3, scale=sc, shift=sh, silu=True)], hp.fwd, _f32(m.conv_out.bias).contiguous(),
                       None, S, S2, out_nchw=out)
        tape.records.append(HeadRec(cur, (sc, sh, a0, o0), hp))
        self.last_tape = tape
        return out

    def _conv3_fwd(self, segs, c: ConvForms, bias, out: View, gb, kw: dict, **f3kw):
        """A ResBlock 3x3 conv behind its GroupNorm (affine bounds gb): Winograd if packed and eligible, else
        halo f16x3 if packed and eligible, else the implicit GEMM.  kw goes to every arm, f3kw to the f16x3
        ones.  Returns (an f16x3 arm ran, out's GroupNorm partials if its epilogue wrote them)."""
        H, W, co = out.H, out.W, out.C
        wino = c.has('wn') and K.wino_eligible(segs, co, H, W)
        if not wino and not (c.has('f3h') and K.x6_eligible(segs, co, H, W)):
            self._conv(segs, c, bias, out, H, W, **kw)
            return False, None
        gp = K.gn_epilogue(out, co, H, W)
        launch, w = (K.conv3x3_wino, c.wn) if wino else (K.conv3x3_f16x3, c.f3h)
        launch(segs, w, bias, out, Hm=H, Wm=W, a_exp=K.f16x3_a_exp(*gb, H * W * segs[0].view.C // 8), gn=gp,
               **kw, **f3kw)
        return True, gp

    def _res_fwd(self, tape: Tape, X: View, Y: View, rp: ResTrain, temb, amx: Optional[torch.Tensor] = None):
        B, H, W = X.B, X.H, X.W
        co = rp.co
        st1 = K.gn_stats_pair(X, _f32(rp.gn1.weight), _f32(rp.gn1.bias), bound=True,
                              part=getattr(X, '_wc_gn_done', None))
        h = View.full(self._new_gn(B, H, W, co))
        # gp1: h's GroupNorm partials, when conv1's epilogue wrote them
        _, gp1 = self._conv3_fwd([Seg(X, TAPS3, scale=st1[0], shift=st1[1], silu=True)], rp.conv1,
                                 _f32(rp.mod1.bias).contiguous(), h, rp.gb1,
                                 dict(temb=temb[:, rp.off:], temb_ld=temb.shape[1]))
        st2 = K.gn_stats_pair(h, _f32(rp.gn2.weight), _f32(rp.gn2.bias), part=gp1)
        # the residual segment (raw X) in fp16 under GN1's per-image bound of |X|; gp2: Y's partials (an
        # attention block's input), the next GroupNorm's statistics
        f3, gp2 = self._conv3_fwd([Seg(h, TAPS3, scale=st2[0], shift=st2[1], silu=True), Seg(X, TAPS1, kbase=9 * co)],
                                  rp.conv2, rp.b2, Y, rp.gb2, {}, a_bound=st1[4], absmax=amx)
        if f3 and amx is not None:
            tape.raised[id(amx)] = True
        if gp2 is not None:
            Y._wc_gn_done = gp2
        tape.records.append(ResRec(X, h, Y, rp, st1, st2))

    def _attn_fwd(self, tape: Tape, Ypre: View, Yout: View, ap: AttnTrain, amx: Optional[torch.Tensor] = None):
        B, H, W, C = Ypre.B, Ypre.H, Ypre.W, Ypre.C
        N = H * W
        gn, mha = ap.gn, ap.mha
        st = K.gn_stats_pair(Ypre, _f32(gn.weight), _f32(gn.bias), part=getattr(Ypre, '_wc_gn_done', None))
        qkv = self._new(B, H, W, 3 * C)
        seg = [Seg(Ypre, TAPS1, scale=st[0], shift=st[1], silu=False)]
        b_in = _f32(mha.in_proj_bias).contiguous()
        o = self._new(B, H, W, C)
        lse = torch.empty((B, ap.heads, N), dtype=torch.float32, device=self.device)
        b_out = _f32(mha.out_proj.bias).contiguous()
        attn = (qkv.view(B * N, 3 * C), o.view(B * N, C), lse, B, N, C, ap.heads)
        if ap.proj_in.has('f3'):
            # in_proj under the GN bound; attention on f16x3 under the in-projection row-norm bounds
            # of Q, K, V (as the sampler); out_proj: |O| <= max|V| (a convex combination of V rows)
            ng = N * C // 8
            K.conv_igemm_f16x3(seg, ap.proj_in.f3, b_in, View.full(qkv), Hm=H, Wm=W, a_exp=K.f16x3_a_exp(*ap.gb, ng))
            exps = K.attention_exps_from_norms(ap.qkv_l1, ap.qkv_babs, ap.gb[0], ap.gb[1], ng)
            K.attention_fwd_lse(*attn, precision='f16x3', exps=exps)
            gpo = K.gn_epilogue(Yout, C, H, W, K.igemm_bm(C))
            K.conv_igemm_f16x3([Seg(View.full(o), TAPS1)], ap.proj_out.f3, b_out, Yout, Hm=H, Wm=W, a_exp=exps[2],
                               res=Ypre, absmax=amx, gn=gpo)
            if amx is not None:
                tape.raised[id(amx)] = True
            if gpo is not None:
                Yout._wc_gn_done = gpo
        else:
            self._conv(seg, ap.proj_in, b_in, View.full(qkv), H, W)
            K.attention_fwd_lse(*attn, precision=self.precision)
            self._conv([Seg(View.full(o), TAPS1)], ap.proj_out, b_out, Yout, H, W, res=Ypre)
        tape.records.append(AttnRec(Ypre, Yout, qkv, o, lse, st, ap))

    # ------------------------------------------------------------------ backward
    def backward(self, gout: torch.Tensor, tape: Optional[Tape] = None) -> Dict[int, torch.Tensor]:
        """Gradients of every parameter (see _backward), on this engine's library variant."""
        with K._native.variant(self.variant):
            return self._backward(gout, tape)

    def _backward(self, gout: torch.Tensor, tape: Optional[Tape] = None) -> Dict[int, torch.Tensor]:
        """Gradients of every parameter given d loss / d output (B, C, S, S) for the forward that
        recorded ``tape`` (default: the latest forward); returns {id(param): grad}.  A tape is
        consumed (its activations freed) by its backward: a second backward through it raises."""
        tape = tape if tape is not None else self.last_tape
        if tape is None or tape.consumed:
            raise RuntimeError('Unet training backward: this forward\'s saved activations were already consumed '
                               'by an earlier backward (retain_graph / a second backward is not supported)')
        records, tape.records = tape.records, []
        tape.consumed = True
        if self.last_tape is tape:
            self.last_tape = None
        # this backward's gradient bookkeeping (_gview .. _pgrad), cleared again below: gmap {id(forward tensor):
        # (gradient tensor, channel offset)}, gfresh the gradient tensors allocated but not yet written, gbnd
        # {id(gradient tensor): its bound}, pgrads {id(param): grad}, pflat_off {id(param): (offset, numel) in pflat}
        self.gmap, self.gfresh, self.gbnd, self.pgrads, self.pflat_off, self.keep = {}, set(), {}, {}, {}, []
        tot = 0
        for prm in self.model.parameters():
            self.pflat_off[id(prm)] = (tot, prm.numel())
            tot += (prm.numel() + 63) // 64 * 64  # 256-byte aligned views
        self.pflat = torch.zeros(tot, dtype=torch.float32, device=self.device)
        self.dproj = torch.zeros((gout.shape[0], tape.P), dtype=torch.float32, device=self.device)
        gout = gout.to(self.device, torch.float32).contiguous()
        K.bsum_defer()  # the ~200 per-layer dgamma / dbeta / bias sums go out in one launch at the end
        try:
            self._bwd_head(records[-1], gout)
            for rec in reversed(records[:-1]):
                self._BWD[type(rec)](self, rec)
            del records
            self._temb_bwd(tape)
        finally:
            K.bsum_flush()
        grads, self.pgrads = self.pgrads, {}
        self.gmap, self.gfresh, self.gbnd, self.keep, self.pflat, self.dproj = {}, set(), {}, [], None, None
        return grads

    @staticmethod
    def _dgrad3_ok(g: View, n_out: int) -> bool:
        """The 3x3 data gradient of g (n_out output channels) fits the halo f16x3 kernel."""
        return K.x6_eligible([Seg(g, TAPS3)], n_out, g.H, g.W)

    def _dgrad3(self, g: View, c: ConvForms, f3: bool, bound, dz: View, gnb_sums: Callable):
        """dz = the 3x3 data gradient of g through c.  f3 (the f16x3 pack exists and _dgrad3_ok; bound: the per-image
        max |g|): Winograd if packed and eligible, else the halo kernel; otherwise the implicit GEMM.  The Winograd
        arm forms the next GroupNorm backward's sums, gnb_sums(), in its epilogue (no pass over dz) and returns them."""
        seg = [Seg(g, TAPS3)]
        H, W = g.H, g.W
        if not f3:
            self._conv(seg, c, None, dz, H, W)
        elif c.has('wn') and K.wino_eligible(seg, dz.C, H, W):
            pre = gnb_sums() if forms.current().train_gnb_epilogue else None
            K.conv3x3_wino(seg, c.wn, None, dz, Hm=H, Wm=W, a_exp=60, a_bound=bound, gnb=pre)
            return pre
        else:
            K.conv3x3_f16x3(seg, c.f3h, None, dz, Hm=H, Wm=W, a_exp=60, a_bound=bound)
        return None

    def _wgrad(self, g: View, segs, dw0, s0, f3=None, **kw):
        """Weight gradient on bf16x6 (precision bf16x6) or fp32 MFMA; f3 = (x_exp, per-image max |g|):
        the 3x3 halo kernel on f16x3 (mode f16x3)."""
        K.conv_wgrad(g, segs, dw0, s0, x6=self.precision == 'bf16x6', f3=f3 if self.f3d else None, **kw)

    def _bias_grad(self, g: View, *params):
        sums = K.channel_sums(g)
        for p in params:
            K.bsum(sums, 0, self._pgrad(p), accumulate=True)
        return sums

    def _bwd_head(self, rec: HeadRec, gout: torch.Tensor):
        m = self.model
        cur, (sc, sh, a0, o0), hp = rec
        B, NO, S, S2 = gout.shape
        C = cur.C
        if hp.small:
            g = gout.contiguous().float()
            K.head_wgrad(cur, sc, sh, g, self._pgrad(m.conv_out.weight))
            self._pgrad(m.conv_out.bias).copy_(g.sum((0, 2, 3)))
            dz = View.full(self._new(B, S, S2, C))
            K.head_dgrad(g, hp.w, dz)
        else:
            g32 = K.nchw_to_nhwc(gout, 32)
            g4 = View(g32, 0, 4)
            wtmp = torch.zeros((4, C, 3, 3), dtype=torch.float32, device=self.device)
            self._wgrad(g4, [Seg(cur, TAPS3, scale=sc, shift=sh, silu=True)], wtmp, (C * 9, 9, 1))
            self._pgrad(m.conv_out.weight).copy_(wtmp[:NO])
            btmp = torch.zeros(4, dtype=torch.float32, device=self.device)
            K.bsum(K.channel_sums(g4), 0, btmp, now=True)  # read by the copy below
            self._pgrad(m.conv_out.bias).copy_(btmp[:NO])
            dz = View.full(self._new(B, S, S2, C))
            self._conv([Seg(View.full(g32), TAPS3)], hp.dgrad, None, dz, S, S2)
        gn = m.norm_out
        gcur, ow = self._grad_w(cur)
        K.gn_backward(dz, cur, a0, o0, _f32(gn.weight), _f32(gn.bias), True, gcur, dgamma=self._pgrad(gn.weight),
                      dbeta=self._pgrad(gn.bias), accumulate=not ow, absmax=self._gb(cur))

    def _bwd_res(self, rec: ResRec):
        X, h, Y, rp, st1, st2 = rec
        B, H, W = X.B, X.H, X.W
        ci, co = rp.ci, rp.co
        gY = self._grad(Y)
        gX = self._gview(X)  # written first by the residual conv's data gradient below
        self._bias_grad(gY, rp.mod2.bias, rp.modr.bias)
        # per-image max |gY|: the range bound of the f16x3 data gradients and weight gradient
        f3Y = rp.d2.has('f3h') and self._dgrad3_ok(gY, co)
        bY = self._bound(gY, self._gb(Y)) if f3Y else None
        bX = self._gb(X)
        self._wgrad(gY, [Seg(h, TAPS3, scale=st2[0], shift=st2[1], silu=True), Seg(X, TAPS1, kbase=9 * co)],
                    self._pgrad(rp.mod2.weight), (co * 9, 9, 1), dw1=self._pgrad(rp.modr.weight), s1=ci,
                    f3=K.F3Bounds(bY, K.f16x3_a_exp(*rp.gb2, H * W * co // 8), None, st1[4]) if f3Y else None)
        dz2 = View.full(self._new(B, H, W, co))
        ga2, be2 = _f32(rp.gn2.weight), _f32(rp.gn2.bias)
        # dh's per-(image, channel) sums (conv1's bias / time-embedding gradients) in closed form from the
        # GN backward's own sums (forms.train_dh_sums off: a channel_sums pass over dh)
        dh_sums = forms.current().train_dh_sums
        pre2 = self._dgrad3(gY, rp.d2, f3Y, bY, dz2,
                            lambda: K.GnbSums.make(h, st2[2], st2[3], ga2, be2, True, dx_sums=dh_sums))
        gX, ow = self._grad_w(X)
        rX = None if ow else gX
        if f3Y and _one_image_tiles(H, W, ci) and co % 16 == 0:  # per-image bound
            K.conv_igemm_f16x3([Seg(gY, TAPS1)], rp.dr.f3, None, gX, Hm=H, Wm=W, a_exp=60, a_bound=bY, res=rX,
                               absmax=bX)
        else:
            self._conv([Seg(gY, TAPS1)], rp.dr, None, gX, H, W, res=rX, absmax=bX)
        dh = View.full(self._new(B, H, W, co))
        bdh = self._zrow(B) if self.f3d else None
        sums = K.gn_backward(dz2, h, st2[2], st2[3], ga2, be2, True, dh, dgamma=self._pgrad(rp.gn2.weight),
                             dbeta=self._pgrad(rp.gn2.bias), accumulate=False, absmax=bdh, dx_sums=dh_sums, pre=pre2)
        if sums is None:
            sums = K.channel_sums(dh)
        K.bsum(sums, 0, self._pgrad(rp.mod1.bias), accumulate=True)
        self.dproj[:, rp.off:rp.off + co].copy_(sums[:, :, 0])
        f3h = rp.d1.has('f3h') and self._dgrad3_ok(dh, ci)
        bh = self._bound(dh, bdh) if f3h else None
        self._wgrad(dh, [Seg(X, TAPS3, scale=st1[0], shift=st1[1], silu=True)], self._pgrad(rp.mod1.weight),
                    (ci * 9, 9, 1), f3=K.F3Bounds(bh, K.f16x3_a_exp(*rp.gb1, H * W * ci // 8)) if f3h else None)
        dz1 = View.full(self._new(B, H, W, ci))
        ga1, be1 = _f32(rp.gn1.weight), _f32(rp.gn1.bias)
        pre1 = self._dgrad3(dh, rp.d1, f3h, bh, dz1, lambda: K.GnbSums.make(X, st1[2], st1[3], ga1, be1, True))
        K.gn_backward(dz1, X, st1[2], st1[3], ga1, be1, True, gX, dgamma=self._pgrad(rp.gn1.weight),
                      dbeta=self._pgrad(rp.gn1.bias), accumulate=True, absmax=bX, pre=pre1)

    def _bwd_attn(self, rec: AttnRec):
        Ypre, Yout, qkv, o, lse, st, ap = rec
        B, H, W, C = Ypre.B, Ypre.H, Ypre.W, Ypre.C
        N = H * W
        mha, gn = ap.mha, ap.gn
        gY = self._grad(Yout)
        self._bias_grad(gY, mha.out_proj.bias)
        f3a = self.f3d and ap.proj_in.has('f3')
        # the forward's Q / K / V exponents (|O| <= max|V|: O shares V's)
        exps = K.attention_exps_from_norms(ap.qkv_l1, ap.qkv_babs, ap.gb[0], ap.gb[1], N * C // 8) if f3a else None
        bgY = self._bound(gY, self._gb(Yout)) if self.f3d else None
        self._wgrad(gY, [Seg(View.full(o), TAPS1)], self._pgrad(mha.out_proj.weight), (C, 1, 0),
                    f3=K.F3Bounds(bgY, exps[2]) if f3a else None)
        do = self._new(B, H, W, C)
        bdo = self._zrow(B) if self.f3d else None
        f3p = ap.d_out.has('f3') and _one_image_tiles(H, W, C)
        if f3p:
            K.conv_igemm_f16x3([Seg(gY, TAPS1)], ap.d_out.f3, None, View.full(do), Hm=H, Wm=W, a_exp=60,
                               a_bound=bgY, absmax=bdo)
        else:
            self._conv([Seg(gY, TAPS1)], ap.d_out, None, View.full(do), H, W, absmax=bdo)
        dqkv = self._new(B, H, W, 3 * C)
        bgq = None
        args = (*(t.view(B * N, -1) for t in (qkv, o, do)), lse, dqkv.view(B * N, 3 * C), B, N, C, ap.heads)
        if f3a:
            # f16x3 under the forward's Q / K / V exponents and the per-image max |dO|; dS under the per-image
            # row norms of dO and V the call measures into row_work (the static bound behind exps[2] is ~2^11
            # above the values: scaled by it dS falls into fp16's subnormals at N >= 1024); the kernels raise the
            # per-image max |dqkv| as they write it (head dims 32 / 64 / 128)
            bgq = self._zrow(B)
            if not K.attention_bwd(*args, precision='f16x3', exps=exps, dout_bound=self._bound(View.full(do), bdo),
                                   dqkv_absmax=bgq, row_work=self._zrow(B, 2)):
                bgq = None
        else:
            K.attention_bwd(*args, precision=self.precision)
        gq = View.full(dqkv)
        self._bias_grad(gq, mha.in_proj_bias)
        if f3a or f3p:
            bgq = self._bound(gq, bgq) if bgq is not None else K.absmax_images(gq)
        self._wgrad(gq, [Seg(Ypre, TAPS1, scale=st[0], shift=st[1], silu=False)], self._pgrad(mha.in_proj_weight),
                    (C, 1, 0), f3=K.F3Bounds(bgq, K.f16x3_a_exp(*ap.gb, N * C // 8)) if f3a else None)
        da = View.full(self._new(B, H, W, C))
        if f3p:
            K.conv_igemm_f16x3([Seg(gq, TAPS1)], ap.d_in.f3, None, da, Hm=H, Wm=W, a_exp=60, a_bound=bgq)
        else:
            self._conv([Seg(gq, TAPS1)], ap.d_in, None, da, H, W)
        # Yout = Ypre + out_proj(...): Ypre's gradient is Yout's plus the GroupNorm path
        self._alias_grad(Ypre.t, Yout)
        K.gn_backward(da, Ypre, st[2], st[3], _f32(gn.weight), _f32(gn.bias), False, self._grad(Ypre),
                      dgamma=self._pgrad(gn.weight), dbeta=self._pgrad(gn.bias), accumulate=True,
                      absmax=self._gb(Ypre))

    def _bwd_down(self, rec: DownRec):
        cur, final, dp, bcur = rec  # bcur: the forward's per-image max |cur|
        gF = self._grad(final)
        w = dp.mod.weight
        self._bias_grad(gF, dp.mod.bias)
        bgF = self._bound(gF, self._gb(final)) if self.f3d else None
        self._wgrad(gF, [Seg(cur, TAPS4S2, stride=2)], self._pgrad(w), (w.shape[1] * 16, 16, 1),
                    f3=K.F3Bounds(bgF, 60, bcur) if bgF is not None and bcur is not None else None)
        gc, ow = self._grad_w(cur)  # the four output parities together cover every pixel
        rc = None if ow else gc
        f3t = dp.dgrad.f3t if dp.dgrad.has('f3t') else None  # packed here, also when the shape then declines it
        if f3t is not None and K.convT4x4s2_f16x3_ok(Seg(gF, [(0, 0)]), gc.C):
            # the ConvT of dY (same weight) in one launch on f16x3 under dY's tracked bound
            K.convT4x4s2_f16x3(Seg(gF, [(0, 0)]), f3t, None, gc, a_bound=bgF, res=rc, absmax=self._gb(cur))
            return
        for (py, px), (taps, c) in zip(_PARITIES, dp.dgrad.parts):
            self._conv([Seg(gF, taps)], c, None, gc, gF.H, gF.W, out_map=(2, 2, py, px), res=rc, absmax=self._gb(cur))

    def _bwd_up(self, rec: UpRec):
        cur, dst, up, bcur = rec
        gD = self._grad(dst)
        wt = up.mod.weight  # [Cin][Cout][4][4]
        self._bias_grad(gD, up.mod.bias)
        # dW[ci][co][ky][kx] = sum_pixels x[ci] * dY[co] at (2y - 1 + ky, 2x - 1 + kx): the 4x4/s2 tap
        # grid over dY with x in the gradient role
        bgD = self._bound(gD, self._gb(dst)) if self.f3d else None
        self._wgrad(cur, [Seg(gD, TAPS4S2, stride=2)], self._pgrad(wt), (wt.shape[1] * 16, 16, 1),
                    f3=K.F3Bounds(bcur, 60, bgD) if bgD is not None and bcur is not None else None)
        seg = Seg(gD, TAPS4S2, stride=2)
        gc, ow = self._grad_w(cur)
        rc = None if ow else gc
        f3s = up.dgrad.f3s if up.dgrad.has('f3s') else None  # as f3t in _bwd_down
        if f3s is not None and K.conv4x4s2_f16x3_ok(seg, gc.C, cur.H, cur.W):
            # the 4x4/s2 conv of dY on the space-to-depth halo kernel, f16x3 under dY's tracked bound
            K.conv4x4s2_f16x3(seg, f3s, None, gc, Hm=cur.H, Wm=cur.W, a_bound=bgD, res=rc, absmax=self._gb(cur))
            return
        self._conv([seg], up.dgrad, None, gc, cur.H, cur.W, res=rc, absmax=self._gb(cur))

    def _bwd_conv_in(self, rec: ConvInRec):
        m = self.model
        x, cur = rec
        g = self._grad(cur)
        self._bias_grad(g, m.conv_in.bias)
        w = m.conv_in.weight
        if forms.current().train_smallconv and w.shape[1] == 3 and g.C in (32, 64) and x.is_contiguous():
            K.stem_wgrad(x, g, self._pgrad(w))  # fp32 VALU, the 3 input channels unpadded
            return
        xn = K.nchw_to_nhwc(x, 4)
        self._wgrad(g, [Seg(View.full(xn), TAPS3)], self._pgrad(w), (w.shape[1] * 9, 9, 1), Cw=w.shape[1])

    _BWD = {ResRec: _bwd_res, AttnRec: _bwd_attn, DownRec: _bwd_down, UpRec: _bwd_up, ConvInRec: _bwd_conv_in}

    def _temb_bwd(self, tape: Tape):
        """t_proj (Linear, SiLU, Linear) and the t_emb_layers (SiLU, Linear) backward (B x 128)."""
        m = self.model
        w1, b1, w2, b2 = tape.tproj
        D = w1.shape[0]
        B, P = self.dproj.shape
        e = K.time_embedding(tape.tt, D)
        a1 = b1.expand(B, D).contiguous()
        K.gemm_small(B, D, D, e, (D, 1), w1, (1, D), a1, D, beta=1.0)
        h1 = K.silu_map(a1)
        a2 = b2.expand(B, D).contiguous()
        K.gemm_small(B, D, D, h1, (D, 1), w2, (1, D), a2, D, beta=1.0)
        s = K.silu_map(a2)
        dp = self.dproj
        for rp in tape.res_rows:
            K.gemm_small(rp.co, D, B, dp, (1, P), s, (D, 1), self._pgrad(rp.temb.weight), D, offs=(rp.off, 0, 0))
            K.colsum(dp, self._pgrad(rp.temb.bias), col0=rp.off, ncol=rp.co)
        ds = torch.empty((B, D), dtype=torch.float32, device=self.device)
        K.gemm_small(B, D, P, dp, (P, 1), tape.temb_w, (D, 1), ds, D)
        da2 = K.silu_map(a2, ds)
        tp = m.t_proj
        K.gemm_small(D, D, B, da2, (1, D), h1, (D, 1), self._pgrad(tp[2].weight), D)
        K.colsum(da2, self._pgrad(tp[2].bias))
        dh1 = torch.empty((B, D), dtype=torch.float32, device=self.device)
        K.gemm_small(B, D, D, da2, (D, 1), w2, (D, 1), dh1, D)
        da1 = K.silu_map(a1, dh1)
        K.gemm_small(D, D, B, da1, (1, D), e, (D, 1), self._pgrad(tp[0].weight), D)
        K.colsum(da1, self._pgrad(tp[0].bias))


class UnetTrainFunction(torch.autograd.Function):
    """Unet.forward in training mode: the HIP forward records its tape, and autograd's backward runs
    TrainEngine.backward, returning one gradient per parameter (so the reference's own
    ``loss.backward(); optimizer.step()`` loop works unchanged)."""

    @staticmethod
    def forward(ctx, engine: TrainEngine, x: torch.Tensor, t, *params):
        if x.requires_grad:
            raise RuntimeError('Unet training forward: the gradient w.r.t. the input image is not computed; '
                               'pass a tensor that does not require grad (x.detach())')
        with torch.no_grad():
            out = engine.forward(x, t)
        ctx.engine = engine
        ctx.tape = engine.last_tape  # this forward's own saved state (gradient accumulation safe)
        engine.last_tape = None
        ctx.param_ids = [id(p) for p in engine.model.parameters()]
        # the backward builds its data-gradient weight packs lazily from the live parameters: saving
        # them makes autograd's version check raise if one is modified in place (an optimizer / EMA
        # step) between this forward and its backward, instead of mixing old and new weights
        ctx.save_for_backward(*params)
        return out

    @staticmethod
    def backward(ctx, gout):
        ctx.saved_tensors  # noqa: B018  (raises if a parameter changed in place since the forward)
        grads = ctx.engine.backward(gout, ctx.tape)
        ctx.tape = None
        # hand autograd the only references, so it can take each gradient as param.grad instead of
        # copying it
        out = tuple(grads.pop(i, None) for i in ctx.param_ids)
        del grads
        return (None, None, None) + out
