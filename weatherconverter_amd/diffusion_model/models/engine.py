"""UnetEngine: runs the reference ``Unet`` forward (``unet_base.py:451-488``) as gfx950 HIP kernels.

Data layout in HBM
------------------
* Activations are NHWC fp32.  The only NCHW tensors are the UNet's input (read by ``wc_conv_in``,
  which fuses the transpose) and its output (written by the last implicit-GEMM conv).
* Skip concatenation is free: for every level ``i`` the engine allocates one buffer
  ``U[i] = (B, S_i, S_i, 2*C_i)``.  The down path writes the level's input ``X_i`` (= the skip
  ``down_outs[i]``) straight into channels ``[C_i, 2C_i)``; the up path's ConvTranspose (or the
  stage below when it does not upsample) writes channels ``[0, C_i)``.  The up ResBlock then reads
  ``U[i]`` as one contiguous tensor, which is exactly ``torch.cat([x, out_down], dim=1)`` of
  ``unet_base.py:349``.
* Weights are repacked once per ``load_state_dict``: the ResBlock 3x3 convs into the Winograd
  F(2,3)-along-x operand layout (``U = (g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2)`` per kernel row, split
  into two fp16 pieces under a per-channel power-of-two scale), conv2 carrying the 1x1
  ``residual_input_conv`` as a 13th K-step per chunk (its bias folded into conv2's); the
  projections, down convs and ConvT into the pre-split ``[N][K]`` fp16-piece layouts.

Default (f16x3, fp32-class) launches per ResBlock (``unet_base.py:146-150``)::

    sc1, sh1, |X| = GN-finalize(partials of X)             wc_gn_finalize_part (partials came from
                                                            X's producer epilogue: no stats pass)
    h  = conv3x3(SiLU(X*sc1 + sh1)) + b1 + temb            wc_conv3x3_wino_f16x3 (GN+SiLU prologue,
                                                            transform, split per chunk in the conv;
                                                            epilogue writes h's GN partials)
    sc2, sh2 = GN-finalize(partials of h)                  wc_gn_finalize_part
    Y  = conv3x3(SiLU(h*sc2 + sh2)) + conv1x1(X) + b2      wc_conv3x3_wino_f16x3, residual in the
                                                            transform domain under |X|

For convs with >= 4 output-channel tiles of 128 the GN+SiLU + transform + split of segment 0 runs
once per input (``wc_wino_vsplit_f16x3``) and the conv copies its halo planes by LDS-DMA
(``wc_conv3x3_wino_f16x3_vp``); the 64-channel conv2 + residual stays on the direct halo kernel
(``wc_conv3x3_f16x3``, measured faster there).

Per attention layer (``unet_base.py:153-161``), in place on Y::

    sc, sh = GN-finalize(partials of Y)
    a3 = split(GN(Y))                                     wc_split_f16x3_tiled (once per element)
    Q, K, V = a3 W_in^T + b_in, written pre-split           wc_proj_f16x3_qkv (fp16 pieces, V in the
                                                            PV MFMA's key order)
    O = flash-attention(Q, K, V), written pre-split        wc_attention_fwd_f16x3_presplit_a3
    Y = Y + O W_out^T + b_out                              wc_proj_f16x3 (residual in place, Y's GN
                                                            partials from the epilogue)

Modes ``bf16x6`` / ``fp32`` (``set_conv_precision``) run the same structure on the direct halo
kernels (``wc_conv3x3_x6``) and implicit-GEMM convs (``wc_conv_igemm``).
"""
from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from ... import forms
from ... import kernels as K
from ...kernels import TAPS3, Seg, View

TAPS1 = [(0, 0)]
TAPS4S2 = [(ky - 1, kx - 1) for ky in range(4) for kx in range(4)]
# ConvTranspose2d(4, stride 2, pad 1): output row 2m+p gathers input rows m+dy with kernel row ky.
_CT_TAPS = {0: [(0, 1), (-1, 3)], 1: [(1, 0), (0, 2)]}


def pack_conv(w: torch.Tensor) -> torch.Tensor:
    """[Co][Ci][kh][kw] -> [Co][(ky*kw + kx)*Ci + ci]."""
    co = w.shape[0]
    return w.detach().permute(0, 2, 3, 1).reshape(co, -1).contiguous().float()


def pack_convT(wt: torch.Tensor, py: int, px: int) -> Tuple[List[Tuple[int, int]], torch.Tensor]:
    """ConvTranspose weight [Ci][Co][4][4] -> (taps, [Co][tap*Ci + ci]) for output parity (py, px)."""
    taps, cols = [], []
    for dy, ky in _CT_TAPS[py]:
        for dx, kx in _CT_TAPS[px]:
            taps.append((dy, dx))
            cols.append(wt.detach()[:, :, ky, kx].t())
    return taps, torch.cat(cols, dim=1).contiguous().float()


@dataclass
class ConvPack:
    """One conv as the engine can launch it: the bias and every packed form of the weight, each field
    named for the entry point it feeds.  A form the conv was not packed for is None."""
    w: torch.Tensor  # fp32 [N][K] (pack_conv): wc_conv_igemm
    b: torch.Tensor
    x6: Optional[K.X6Weight] = None  # bf16x6, natural K order: wc_conv_igemm_x6
    x6h: Optional[K.X6Weight] = None  # bf16x6, halo order: wc_conv3x3_x6
    f3: Optional[K.X6Weight] = None  # f16x3, natural K order: wc_conv_igemm_f16x3, wc_proj_f16x3(_qkv)
    f3h: Optional[K.X6Weight] = None  # f16x3, halo order: wc_conv3x3_f16x3
    wn: Optional[K.X6Weight] = None  # Winograd F(2,3): wc_conv3x3_wino_f16x3 (forms.wino)
    f3s: Optional[K.X6Weight] = None  # f16x3, space-to-depth: wc_conv4x4s2_f16x3 (forms.down_s2d)
    gb: Tuple[float, float] = (0.0, 0.0)  # (max|gamma|, max|beta|) of the GroupNorm in front (f16x3 bound)


@dataclass
class UpPack:
    """A 4x4 / stride-2 ConvTranspose: one launch of wc_convtr4x4s2_f16x3 (f3t, forms.up_ct), or its
    four output parities as implicit-GEMM convs, (taps, pack) for (py, px) = (0, 0), (0, 1), (1, 0), (1, 1)."""
    b: torch.Tensor
    f3t: Optional[K.X6Weight]
    parts: List[Tuple[List[Tuple[int, int]], ConvPack]]


@dataclass
class ResPack:
    ci: int
    co: int
    g1: torch.Tensor
    be1: torch.Tensor
    g2: torch.Tensor
    be2: torch.Tensor
    temb_off: int
    conv1: ConvPack
    conv2: ConvPack  # weight: conv2 (9*co) ++ residual 1x1 (ci); bias: the sum of the two


@dataclass
class AttnPack:
    c: int
    heads: int
    g: torch.Tensor
    be: torch.Tensor
    proj_in: ConvPack  # f16x3 under the GN bound
    proj_out: ConvPack  # f16x3 under the V bound
    qkv_l1: Optional[torch.Tensor] = None  # f16x3: host row-L1 norms of W_in and |b_in| (bounds)
    qkv_babs: Optional[torch.Tensor] = None
    gb: Tuple[float, float] = (0.0, 0.0)


TRAIN_MAX_IM_CHANNELS = 4  # TrainEngine pads the image and the loss gradient to 4 NHWC channels


def check_supported(mc, precision: str, training: bool = False) -> None:
    """The configurations the engines run, stated once ("Supported configurations").
    Pure Python over the ModelConfig: no device is read and nothing is launched.  UnetEngine and
    TrainEngine call it before anything is packed, so a configuration outside the envelope raises here,
    naming the field, the value and the rule, instead of part-way through a pass with a bare shape
    status.  precision: 'f16x3' / 'bf16x6' / 'fp32' (training also 'f16' / 'bf16', the 16-bit lines on
    the f16x3 kernels)."""
    if precision not in K.CONV_PRECISIONS + ('f16', 'bf16'):
        raise RuntimeError(f'weatherconverter_amd: unknown precision {precision!r}')

    def bad(field, value, rule):
        raise RuntimeError(f'weatherconverter_amd: unsupported configuration: {field} = {value!r}: {rule} '
                           f'(precision {precision!r}, {"training" if training else "inference"})')

    dc, mids = list(mc.down_channels), list(mc.mid_channels)
    # channel counts: every conv's input segments are whole K-steps of its GEMM, and every GroupNorm(8)
    # group is whole 4-channel reads of the statistics pass
    gemm = K.IGEMM_BK if precision == 'fp32' else K.SPLIT_CK
    gn = K.GN_GROUPS * K.GN_VEC
    for field, chans in (('down_channels', dc), ('mid_channels', mids)):
        for c in chans:
            if c <= 0 or c % gemm:
                bad(field, chans, f'every channel count must be a positive multiple of {gemm} (got {c}): ' +
                    (f'the fp32 implicit GEMM reads {K.IGEMM_BK} channels per K-step' if precision == 'fp32' else
                     f'the split-precision weight packs hold {K.SPLIT_CK} channels per K-step'))
            if c % gn:
                bad(field, chans, f'every channel count must be a multiple of {gn} (got {c}): GroupNorm({K.GN_GROUPS}) '
                    f'statistics read each group {K.GN_VEC} channels at a time')
    # attention head dims: downs / ups by the placement rule of Unet.level_has_attn, every mid block
    L = len(dc) - 1
    attn_c = [mids[j + 1] for j in range(len(mids) - 1)]
    for i in range(L):
        if (mc.im_size // (2**i)) in list(mc.attn_resolutions):
            attn_c += [dc[i + 1], dc[i - 1] if i != 0 else dc[0]]
    heads = mc.num_heads
    for c in attn_c:
        if heads <= 0 or c % heads:
            bad('num_heads', heads, f'must divide the attention width {c}')
        d = c // heads
        rule = f'an attention layer of {c} channels has head dim {d}'
        if d not in K.ATTN_FWD_DIMS:
            bad('num_heads', heads, f'{rule}; the attention kernels exist for head dims {K.ATTN_FWD_DIMS}')
        if precision != 'fp32' and d % 32 == 0 and d not in K.ATTN_SPLIT_DIMS:
            bad('num_heads', heads, f'{rule}; the split-precision attention exists for {K.ATTN_SPLIT_DIMS}')
        if training and d not in K.ATTN_BWD_DIMS:
            bad('num_heads', heads, f'{rule}; the attention backward exists for head dims {K.ATTN_BWD_DIMS}')
    D = mc.time_emb_dim
    if D <= 0 or D % 4 or D > K.TEMB_MAX_D:
        bad('time_emb_dim', D, f'must be a multiple of 4 and at most {K.TEMB_MAX_D} (wc_temb keeps the embedding '
            'and the hidden layer in LDS and reads the weights four at a time)')
    ci = mc.im_channels
    if ci < 1 or ci > K.CONV_IN_MAX_CIN or ci * 9 * dc[0] * 4 > K.CONV_IN_MAX_LDS:
        bad('im_channels', ci, f'the stem conv takes 1 to {K.CONV_IN_MAX_CIN} image channels and stages '
            f'im_channels * 9 * down_channels[0] weights in at most {K.CONV_IN_MAX_LDS} bytes of LDS')
    if training and ci > TRAIN_MAX_IM_CHANNELS:
        bad('im_channels', ci, f'training takes at most {TRAIN_MAX_IM_CHANNELS} image channels: the stem and head '
            f'weight gradients read the image and the loss gradient padded to {TRAIN_MAX_IM_CHANNELS} channels')


class UnetEngine:

    def __init__(self, model):
        params = list(model.parameters())
        if not params or not params[0].is_cuda:
            raise RuntimeError('weatherconverter_amd.Unet runs on the GPU only (HIP kernels, no CPU fallback): '
                               'move the model to a ROCm device first')
        check_supported(model.model_config, getattr(model, 'conv_precision', None) or K.default_conv_precision())
        K._native.load()
        self.model = model
        self.device = params[0].device
        self.precision = getattr(model, 'conv_precision', None) or K.default_conv_precision()
        # f16x3 attention on the pre-split in-projection (off: fp32 projection + split in the attention
        # kernel, the bit-identical reference path)
        self.attn_presplit = forms.current().attn_presplit
        # GroupNorm statistics from the producers' epilogue tile partials (False: a stats pass per GN)
        self.gn_partials = forms.current().gn_partials
        self._sig = self._signature()
        self._pack()

    # ------------------------------------------------------------------ packing
    def _signature(self):
        return tuple((p.data_ptr(), p._version) for p in self.model.parameters())

    def _pack(self):
        m = self.model
        self.temb_rows_w, self.temb_rows_b = [], []
        self._temb_P = 0
        with torch.no_grad():
            self.downs = [self._pack_stage(blk, n_res=blk.num_layers, attn=blk.use_attn) for blk in m.downs]
            self.down_convs = []
            for blk in m.downs:
                if blk.down_sample:
                    dn = blk.down_sample_conv
                    p = self._pack_resample(pack_conv(dn.weight), dn.bias.detach().float(), dn.in_channels,
                                            len(TAPS4S2))
                    p.f3s = self._f3s(p.w, dn.in_channels)
                    self.down_convs.append(p)
                else:
                    self.down_convs.append(None)
            self.mids = [self._pack_stage(blk, n_res=blk.num_layers + 1, attn=True) for blk in m.mids]
            self.ups = [self._pack_stage(blk, n_res=blk.num_layers, attn=blk.use_attn) for blk in m.ups]
            self.up_convs = []
            for blk in m.ups:
                if blk.up_sample:
                    up = blk.up_sample_conv
                    b = up.bias.detach().float()
                    parts = [pack_convT(up.weight, py, px) for py in (0, 1) for px in (0, 1)]
                    parts = [(taps, self._pack_resample(w, b, up.in_channels, len(taps))) for taps, w in parts]
                    self.up_convs.append(UpPack(b, self._f3t(up.weight, up.in_channels), parts))
                else:
                    self.up_convs.append(None)
            self.conv_in_w = m.conv_in.weight.detach().float().contiguous()
            self.conv_in_b = m.conv_in.bias.detach().float().contiguous()
            self.norm_out = (m.norm_out.weight.detach().float(), m.norm_out.bias.detach().float())
            co = self.conv_out = ConvPack(pack_conv(m.conv_out.weight), m.conv_out.bias.detach().float().contiguous())
            co.x6 = self._x6(co.w, m.conv_out.in_channels, 9)
            if self.precision == 'f16x3' and m.conv_out.in_channels % 16 == 0:
                co.f3 = K.pack_f16x3(co.w, m.conv_out.in_channels, order='natural')
                co.gb = (float(m.norm_out.weight.abs().max()), float(m.norm_out.bias.abs().max()))
            # <= 4 output channels: the dedicated HBM-bound head kernel (an MFMA tile would waste 20x)
            self.conv_out_head = None
            if m.conv_out.out_channels <= 4 and m.conv_out.in_channels % 16 == 0:
                self.conv_out_head = K.pack_head(m.conv_out.weight)
            tp = m.t_proj
            self.tproj = [tp[0].weight.detach().float().contiguous(), tp[0].bias.detach().float().contiguous(),
                          tp[2].weight.detach().float().contiguous(), tp[2].bias.detach().float().contiguous()]
            self.temb_w = torch.cat(self.temb_rows_w, 0).contiguous()
            self.temb_b = torch.cat(self.temb_rows_b, 0).contiguous()

    def _pack_res(self, blk, i: int) -> ResPack:
        f, s, r = blk.resnet_conv_first[i], blk.resnet_conv_second[i], blk.residual_input_conv[i]
        tl = blk.t_emb_layers[i][1]
        ci, co = f[2].in_channels, f[2].out_channels
        w2 = torch.cat([pack_conv(s[2].weight), r.weight.detach().reshape(co, ci).float()], 1).contiguous()
        c1 = ConvPack(pack_conv(f[2].weight), f[2].bias.detach().float().contiguous())
        c2 = ConvPack(w2, (s[2].bias.detach().float() + r.bias.detach().float()).contiguous())
        p = ResPack(ci=ci, co=co, g1=f[0].weight.detach().float(), be1=f[0].bias.detach().float(),
                    g2=s[0].weight.detach().float(), be2=s[0].bias.detach().float(), temb_off=self._temb_P,
                    conv1=c1, conv2=c2)
        if self.precision in ('bf16x6', 'f16x3') and ci % 16 == 0 and co % 16 == 0:
            # halo-order pack for the 3x3 kernel (bf16x6 mode), natural-order pack for the
            # implicit-GEMM fallback (grids the halo kernel does not tile), f16x3 pack
            f3 = self.precision == 'f16x3'
            c1.x6h = None if f3 else K.pack_x6(c1.w, ci)
            c1.x6 = self._x6(c1.w, ci, 9)
            c2.x6h = None if f3 else K.pack_x6(c2.w, co, ci)
            c2.x6 = self._x6(c2.w, co, 9, ci)
            if f3:
                c1.f3h = K.pack_f16x3(c1.w, ci)
                c2.f3h = K.pack_f16x3(c2.w, co, ci, res_f16=True)  # residual bounded by GN1's stats of X
                if forms.current().wino:
                    c1.wn = K.pack_wino(c1.w, ci)
                    c2.wn = K.pack_wino(c2.w, co, ci)
                c1.gb = (float(p.g1.abs().max()), float(p.be1.abs().max()))
                c2.gb = (float(p.g2.abs().max()), float(p.be2.abs().max()))
        self.temb_rows_w.append(tl.weight.detach().float())
        self.temb_rows_b.append(tl.bias.detach().float())
        self._temb_P += co
        return p

    def _x6(self, w: torch.Tensor, c0: int, ntaps: int, c1: int = 0) -> Optional[K.X6Weight]:
        """bf16x6 (natural K order) re-pack for wc_conv_igemm_x6, or None in fp32 mode."""
        if self.precision == 'fp32' or c0 % 16 or c1 % 16:
            return None
        return K.pack_x6(w, c0, c1, ntaps=ntaps, order='natural')

    def _pack_resample(self, w: torch.Tensor, b: torch.Tensor, c0: int, ntaps: int) -> ConvPack:
        """A resampling conv (the down conv, one ConvT parity): bf16x6 outside fp32 mode; in f16x3 mode
        also the f16x3 pack, for an input whose range comes from its producer's per-image absmax."""
        p = ConvPack(w, b, x6=self._x6(w, c0, ntaps))
        if self.precision == 'f16x3' and c0 % 16 == 0:
            p.f3 = K.pack_f16x3(w, c0, ntaps=ntaps, order='natural')
        return p

    def _f3s(self, w: torch.Tensor, c0: int) -> Optional[K.X6Weight]:
        """f16x3 space-to-depth pack of a 4x4 / stride-2 down conv for wc_conv4x4s2_f16x3 (the halo
        kernel), or None (outside f16x3 mode, N <= 64, or forms.down_s2d off: the implicit GEMM)."""
        if (self.precision != 'f16x3' or c0 % 16 or K.x6_tile(w.shape[0])[1] != 128
                or not forms.current().down_s2d):
            return None
        return K.pack_f16x3_s2d(w, c0)

    def _f3t(self, wt: torch.Tensor, c0: int) -> Optional[K.X6Weight]:
        """f16x3 pack of a 4x4 / stride-2 ConvTranspose for wc_convtr4x4s2_f16x3 (all four parities in
        one launch of the halo kernel), or None (outside f16x3 mode or forms.up_ct off: the four
        implicit-GEMM parities)."""
        if self.precision != 'f16x3' or c0 % 16 or not forms.current().up_ct:
            return None
        return K.pack_f16x3_convT(wt.detach().float())

    def _pack_attn(self, blk, i: int) -> AttnPack:
        mha, gn = blk.attentions[i], blk.attention_norms[i]
        c = mha.embed_dim
        pi = ConvPack(mha.in_proj_weight.detach().float().contiguous(),
                      mha.in_proj_bias.detach().float().contiguous())
        po = ConvPack(mha.out_proj.weight.detach().float().contiguous(),
                      mha.out_proj.bias.detach().float().contiguous())
        p = AttnPack(c=c, heads=mha.num_heads, g=gn.weight.detach().float(), be=gn.bias.detach().float(),
                     proj_in=pi, proj_out=po)
        pi.x6 = self._x6(pi.w, c, 1)
        po.x6 = self._x6(po.w, c, 1)
        if self.precision == 'f16x3':
            pi.f3 = K.pack_f16x3(pi.w, c, ntaps=1, order='natural')
            po.f3 = K.pack_f16x3(po.w, c, ntaps=1, order='natural')
            p.qkv_l1 = pi.w.double().abs().sum(1).cpu()
            p.qkv_babs = pi.b.double().abs().cpu()
            p.gb = (float(p.g.abs().max()), float(p.be.abs().max()))
        return p

    def _pack_stage(self, blk, n_res: int, attn: bool):
        res = [self._pack_res(blk, i) for i in range(n_res)]
        n_attn = len(blk.attentions)
        att = [self._pack_attn(blk, i) for i in range(n_attn)] if attn else []
        return res, att

    # ------------------------------------------------------------------ building blocks
    def _new(self, B, H, W, C, gn_sw: Optional[int] = None) -> torch.Tensor:
        """Scratch activation.  With gn_sw (and a shape the partials tile) it also carries GroupNorm
        tile partials (kernels.GnPart) that its producers' epilogues fill, so that its GroupNorm
        consumers finalize from them instead of re-reading the tensor."""
        t = torch.empty((B, H, W, C), dtype=torch.float32, device=self.device)
        if gn_sw is not None and self.gn_partials and K.GnPart.eligible(t):
            K.GnPart.attach(t, gn_sw)
        return t

    @staticmethod
    def _sw(C: int) -> Optional[int]:
        """Partials sub-slot width for GroupNorm(8) over C channels (and over 2C for the skip buffers)."""
        cpg = C // 8
        for sw in (32, 16, 8, 4):
            if C % 8 == 0 and cpg % sw == 0:
                return sw
        return None

    def _gn(self, v: View, gamma, beta, bound: bool = False):
        """GroupNorm(8) affine of a view: from its tile partials when it has them, else a stats pass."""
        gp = K.GnPart.of(v)
        if gp is not None and (v.C // 8) % gp.sw == 0:
            return K.gn_affine(v, gamma, beta, bound=bound, part=gp)
        return K.gn_affine(v, gamma, beta, bound=bound)

    def _gn_fill(self, v: Optional[View], fused: bool = False):
        """Partials of a view written by a kernel that did not emit them from its epilogue."""
        gp = K.GnPart.of(v)
        if gp is not None and not fused:
            K.gn_partials(v, gp)

    def conv(self, segs, p: ConvPack, out: Optional[View], H: int, W: int, absmax: Optional[torch.Tensor] = None,
             gn_p64: int = 0, gn_defer: bool = False, **kw) -> Tuple[bool, bool]:
        """Any conv: bf16x6 implicit GEMM when packed for it, else fp32 MFMA.  Returns (the per-image
        output absmax was emitted into `absmax`, the output's GN partials came from the epilogue);
        partials not emitted are filled by a stats pass unless gn_defer."""
        gp = None
        if p.x6 is not None:
            gp = K.gn_epilogue(out, p.x6.N, H, W, K.igemm_bm(p.x6.N))
            K.conv_igemm_x6(segs, p.x6, p.b, out, Hm=H, Wm=W, absmax=absmax, gn=gp, gn_p64=gn_p64, **kw)
        else:
            K.conv_igemm(segs, p.w, p.b, out, Hm=H, Wm=W, **kw)
        if not gn_defer:
            self._gn_fill(out, gp is not None)
        return absmax is not None and p.x6 is not None, gp is not None

    def resample(self, segs, p: ConvPack, out: View, H: int, W: int, bound: Optional[torch.Tensor], gn_p64: int = 0,
                 gn_defer: bool = False, **kw) -> bool:
        """Down-sampling conv / one transposed-conv parity: f16x3 implicit GEMM scaled per image by
        the producer's absmax when there is one (and the tiles stay within an image), else bf16x6.
        Returns whether the output's GN partials came from the epilogue."""
        if p.f3 is not None and bound is not None and (H * W) % K.igemm_bm(p.f3.N) == 0:
            gp = K.gn_epilogue(out, p.f3.N, H, W, K.igemm_bm(p.f3.N))
            K.conv_igemm_f16x3(segs, p.f3, p.b, out, Hm=H, Wm=W, a_exp=60, a_bound=bound, gn=gp, gn_p64=gn_p64, **kw)
            if not gn_defer:
                self._gn_fill(out, gp is not None)
            return gp is not None
        return self.conv(segs, p, out, H, W, gn_p64=gn_p64, gn_defer=gn_defer, **kw)[1]

    def conv3(self, segs, p: ConvPack, out: View, H: int, W: int, a_bound: Optional[torch.Tensor] = None,
              absmax: Optional[torch.Tensor] = None, **kw) -> bool:
        """A ResBlock 3x3 stride-1 conv (GN+SiLU prologue): the halo-tiled kernel in f16x3 (bound
        from the GroupNorm affine p.gb and the group size) or bf16x6 when the grid tiles, else the
        bf16x6 implicit GEMM (or fp32 MFMA in fp32 mode).  GN partials of `out` are emitted by the
        split-precision epilogues where they can be, else filled by a stats pass.  Returns whether
        the absmax was emitted."""
        if (p.wn is not None and K.wino_eligible(segs, p.wn.N, H, W) and (len(segs) == 1 or a_bound is not None)
                and (p.f3h is None or K.x6_eligible(segs, p.f3h.N, H, W))):
            # the Winograd F(2,3)-along-x form of the same f16x3 conv (1.5x fewer MFMAs)
            n_group = H * W * segs[0].view.C // 8
            gp = K.gn_epilogue(out, p.wn.N, H, W)
            K.conv3x3_wino(segs, p.wn, p.b, out, Hm=H, Wm=W, a_exp=K.f16x3_a_exp(p.gb[0], p.gb[1], n_group),
                           a_bound=a_bound, absmax=absmax, gn=gp, **kw)
            self._gn_fill(out, gp is not None)
            return absmax is not None
        if p.f3h is not None and K.x6_eligible(segs, p.f3h.N, H, W):
            n_group = H * W * segs[0].view.C // 8
            gp = K.gn_epilogue(out, p.f3h.N, H, W)
            K.conv3x3_f16x3(segs, p.f3h, p.b, out, Hm=H, Wm=W, a_exp=K.f16x3_a_exp(p.gb[0], p.gb[1], n_group),
                            a_bound=a_bound if p.f3h.res_f16 else None, absmax=absmax, gn=gp, **kw)
            self._gn_fill(out, gp is not None)
            return absmax is not None
        if p.x6h is not None and K.x6_eligible(segs, p.x6h.N, H, W):
            gp = K.gn_epilogue(out, p.x6h.N, H, W)
            K.conv3x3_x6(segs, p.x6h, p.b, out, Hm=H, Wm=W, absmax=absmax, gn=gp, **kw)
            self._gn_fill(out, gp is not None)
            return absmax is not None
        return self.conv(segs, p, out, H, W, absmax=absmax, **kw)[0]

    def resblock(self, X: View, Y: View, p: ResPack, temb: torch.Tensor, temb_ld: int,
                 absmax: Optional[torch.Tensor] = None) -> bool:
        B, H, W = X.B, X.H, X.W
        xb = None
        if p.conv2.f3h is not None and p.conv2.f3h.res_f16:
            sc1, sh1, xb = self._gn(X, p.g1, p.be1, bound=True)  # xb bounds |X| (conv2's residual input)
        else:
            sc1, sh1 = self._gn(X, p.g1, p.be1)
        h = View.full(self._new(B, H, W, p.co, gn_sw=self._sw(p.co)))
        self.conv3([Seg(X, TAPS3, scale=sc1, shift=sh1, silu=True)], p.conv1, h, H, W, temb=temb[:, p.temb_off:],
                   temb_ld=temb_ld)
        sc2, sh2 = self._gn(h, p.g2, p.be2)
        return self.conv3([Seg(h, TAPS3, scale=sc2, shift=sh2, silu=True), Seg(X, TAPS1, kbase=9 * p.co)], p.conv2, Y,
                          H, W, a_bound=xb, absmax=absmax)

    def attention(self, Y: View, p: AttnPack, absmax: Optional[torch.Tensor] = None) -> bool:
        B, H, W, C = Y.B, Y.H, Y.W, Y.C
        N = H * W
        sc, sh = self._gn(Y, p.g, p.be)
        pi, po = p.proj_in, p.proj_out
        if pi.f3 is not None:
            # in_proj: GN output bound; attention: q/k/v bounds; out_proj: |O| <= max|V| (convex
            # combination of V rows), so the V exponent bounds it
            a_exp = K.f16x3_a_exp(p.gb[0], p.gb[1], N * C // 8)
            exps = K.attention_exps_from_norms(p.qkv_l1, p.qkv_babs, p.gb[0], p.gb[1], N * C // 8)
            seg = Seg(Y, TAPS1, scale=sc, shift=sh, silu=False)
            if self.attn_presplit and K.qkv_presplit_ok(B, N, C, p.heads):
                # the in_proj epilogue writes Q, K, V already scaled and split (fp16 pieces, V
                # transposed in the PV key order); the attention copies K / V^T tiles by LDS-DMA
                qkv3 = torch.empty(B * 6 * C * N, dtype=torch.int16, device=self.device)
                if forms.current().proj_pa and K.proj_pa_ok(Y, 3 * C):
                    # GN applied and split once per element (not once per 128-column N tile), then
                    # both GEMM operands staged by LDS-DMA
                    a3 = K.split_f16x3_tiled(Y, a_exp, sc, sh)
                    K.proj_f16x3_qkv(Y, a3, pi.f3, pi.b, qkv3, a_exp=a_exp, C=C, heads=p.heads, exps=exps)
                    del a3
                else:
                    K.conv_igemm_f16x3_qkv(seg, pi.f3, pi.b, qkv3, Hm=H, Wm=W, a_exp=a_exp, C=C, heads=p.heads,
                                           exps=exps)
                if forms.current().proj_pa and K.proj_pa_ok(Y, C) and C % 32 == 0:
                    # the attention writes O already scaled and split in the out-projection's LDS
                    # stage order (no fp32 O round trip, no split pass); the GEMM copies it by LDS-DMA
                    a3o = K.attention_presplit_a3(qkv3, B, N, C, p.heads, exps)
                    del qkv3
                    gp = K.gn_epilogue(Y, po.f3.N, H, W, K.igemm_bm(po.f3.N))
                    shape = View(a3o.view(torch.float32).view(B, H, W, C), 0, C)  # the operand's view shape
                    K.proj_f16x3(shape, a3o, po.f3, po.b, Y, a_exp=exps[2], res=Y, absmax=absmax, gn=gp)
                    self._gn_fill(Y, gp is not None)
                    return absmax is not None
                o = self._new(B, H, W, C)
                K.attention_presplit(qkv3, o.view(B * N, C), B, N, C, p.heads, exps)
            else:
                o = self._new(B, H, W, C)
                qkv = self._new(B, H, W, 3 * C)
                K.conv_igemm_f16x3([seg], pi.f3, pi.b, View.full(qkv), Hm=H, Wm=W, a_exp=a_exp)
                K.attention(qkv.view(B * N, 3 * C), o.view(B * N, C), B, N, C, p.heads, 'f16x3', exps)
            gp = K.gn_epilogue(Y, po.f3.N, H, W, K.igemm_bm(po.f3.N))
            K.conv_igemm_f16x3([Seg(View.full(o), TAPS1)], po.f3, po.b, Y, Hm=H, Wm=W, a_exp=exps[2], res=Y,
                               absmax=absmax, gn=gp)
            self._gn_fill(Y, gp is not None)
            return absmax is not None
        qkv = self._new(B, H, W, 3 * C)
        o = self._new(B, H, W, C)
        self.conv([Seg(Y, TAPS1, scale=sc, shift=sh, silu=False)], pi, View.full(qkv), H, W)
        K.attention(qkv.view(B * N, 3 * C), o.view(B * N, C), B, N, C, p.heads, self.precision)
        return self.conv([Seg(View.full(o), TAPS1)], po, Y, H, W, res=Y, absmax=absmax)[0]

    # ------------------------------------------------------------------ forward
    def max_batch(self, S: int, S2: int) -> int:
        """Largest batch one pass can take: the kernels address each source tensor of the whole batch
        through one buffer descriptor (32-bit byte offsets, < 2 GiB).  Per image, the widest tensor at
        level i is the skip buffer (2*dc[i] channels), a ResBlock output (dc[i+1]) or an attention
        in-projection (3*C; 6*C fp16 pieces pre-split, the same bytes)."""
        m = self.model
        dc, mids = m.down_channels, m.mid_channels
        h, w = S, S2
        per_image = 0
        L = len(dc) - 1
        for i in range(L):
            att = m.downs[i].use_attn or m.ups[L - 1 - i].use_attn
            wide = max(2 * dc[i], dc[i + 1], 3 * max(dc[i], dc[i + 1]) if att else 0)
            per_image = max(per_image, h * w * 4 * wide)
            if m.down_sample[i]:
                h, w = h // 2, w // 2
        per_image = max(per_image, h * w * 4 * 3 * max(mids + [dc[-1]]))
        return max(1, ((1 << 31) - 1) // per_image)

    def forward(self, x: torch.Tensor, t) -> torch.Tensor:
        """Batches above max_batch run as consecutive chunks: every op is per image, and every kernel's
        reduction order is independent of the batch, so the result equals one pass bit for bit."""
        m = self.model
        if x.dim() != 4 or x.shape[1] != m.model_config.im_channels:
            raise RuntimeError(f'Unet expects (B, {m.model_config.im_channels}, H, W), got {tuple(x.shape)}')
        B = x.shape[0]
        tt = torch.as_tensor(t).long().reshape(-1).to(self.device)
        if tt.shape[0] not in (1, B):
            raise RuntimeError(f'timestep tensor has {tt.shape[0]} entries for a batch of {B}')
        cap = self.max_batch(x.shape[2], x.shape[3])
        if B <= cap:
            return self._forward(x, tt)
        outs = []
        for b0 in range(0, B, cap):
            tc = tt if tt.shape[0] == 1 else tt[b0:b0 + cap]
            outs.append(self._forward(x[b0:b0 + cap], tc))
        return torch.cat(outs)

    def refresh(self) -> None:
        """Repack, on the current stream, if a parameter changed since the last pack (every forward starts
        with this; a caller that forks streams calls it before the fork, so that no stream reads packs
        another one is still writing)."""
        if self._signature() != self._sig:  # parameters changed in place: repack
            self._sig = self._signature()
            self._pack()

    def _forward(self, x: torch.Tensor, tt: torch.Tensor) -> torch.Tensor:
        self.refresh()
        m = self.model
        x = x.to(device=self.device, dtype=torch.float32).contiguous()
        B, _, S, S2 = x.shape
        nt = tt.shape[0]
        temb = K.temb(tt, *self.tproj, self.temb_w, self.temb_b)
        temb_ld = temb.shape[1] if nt > 1 else 0

        dc = m.down_channels
        L = len(dc) - 1
        sizes = [(S, S2)]
        for i in range(L):
            h, w = sizes[-1]
            sizes.append((h // 2, w // 2) if m.down_sample[i] else (h, w))
        # skip buffers: partials at the sub-slot width of the half (down-path) view, which also tiles
        # the whole (up-path, 2C-channel) view's groups
        U = [self._new(B, sizes[i][0], sizes[i][1], 2 * dc[i], gn_sw=self._sw(dc[i])) for i in range(L)]

        cur = View(U[0], dc[0], dc[0])
        self._gn_fill(cur, K.conv_in(x, self.conv_in_w, self.conv_in_b, cur, gn=K.GnPart.of(cur)))

        # per-image max |x| of each resampling conv's input, emitted by its producer's epilogue
        # (the f16x3 down / transposed convs scale by it; one row per resampling conv)
        amax = None
        if self.precision == 'f16x3':
            amax = torch.zeros((2 * L + 1, B), dtype=torch.float32, device=self.device)
        slots = iter(range(2 * L + 1))

        def bound_slot(needed: bool):
            return amax[next(slots)] if (needed and amax is not None) else None

        def layer(cur: View, tgt: View, stage, li: int, slot):
            """ResBlock li of a stage into tgt, then the layer's attention in place where it has one.
            Returns slot when the last of the two emitted tgt's per-image absmax into it, else None."""
            res, att = stage
            ap = att[li] if li < len(att) else None
            emitted = self.resblock(cur, tgt, res[li], temb, temb_ld, absmax=None if ap is not None else slot)
            if ap is not None:
                emitted = self.attention(tgt, ap, absmax=slot)
            return slot if emitted else None

        # ---------------- down path
        for i in range(L):
            stage, dn = self.downs[i], self.down_convs[i]
            n_res = len(stage[0])
            co = dc[i + 1]
            H, W = sizes[i]
            final = View(U[i + 1], dc[i + 1], dc[i + 1]) if i < L - 1 else View.full(
                self._new(B, sizes[i + 1][0], sizes[i + 1][1], co, gn_sw=self._sw(co)))
            bnd = None
            for li in range(n_res):
                last = li == n_res - 1
                tgt = final if (last and dn is None) else View.full(self._new(B, H, W, co, gn_sw=self._sw(co)))
                bnd = layer(cur, tgt, stage, li, bound_slot(last and dn is not None))
                cur = tgt
            if dn is not None:
                seg = Seg(cur, TAPS4S2, stride=2)
                Hm, Wm = sizes[i + 1]
                if dn.f3s is not None and bnd is not None and K.conv4x4s2_f16x3_ok(seg, dn.f3s.N, Hm, Wm):
                    gp = K.gn_epilogue(final, dn.f3s.N, Hm, Wm)
                    K.conv4x4s2_f16x3(seg, dn.f3s, dn.b, final, Hm=Hm, Wm=Wm, a_bound=bnd, gn=gp)
                    self._gn_fill(final, gp is not None)
                else:
                    self.resample([seg], dn, final, Hm, Wm, bnd)
                cur = final

        # ---------------- mid path
        bnd = None
        for j, stage in enumerate(self.mids):
            res = stage[0]
            H, W = cur.H, cur.W
            for li, rp in enumerate(res):
                last = j == len(self.mids) - 1 and li == len(res) - 1
                if last and self.up_convs[0] is None:
                    tgt = View(U[L - 1], 0, dc[L - 1])
                else:
                    tgt = View.full(self._new(B, H, W, rp.co, gn_sw=self._sw(rp.co)))
                bnd = layer(cur, tgt, stage, li, bound_slot(last and self.up_convs[0] is not None))
                cur = tgt

        # ---------------- up path
        for k, stage in enumerate(self.ups):
            res, up = stage[0], self.up_convs[k]
            i = L - 1 - k
            H, W = sizes[i]
            if up is not None:
                dst = View(U[i], 0, dc[i])
                seg = Seg(cur, [(0, 0)])
                if up.f3t is not None and bnd is not None and K.convT4x4s2_f16x3_ok(seg, up.f3t.N):
                    gp = K.gn_epilogue(dst, up.f3t.N, dst.H, dst.W)
                    K.convT4x4s2_f16x3(seg, up.f3t, up.b, dst, a_bound=bnd, gn=gp)
                    self._gn_fill(dst, gp is not None)
                else:
                    np_in = cur.H * cur.W // 64 if (cur.H * cur.W) % 64 == 0 else 0
                    fused = []
                    for par, ((py, px), (taps, p)) in enumerate(zip(((0, 0), (0, 1), (1, 0), (1, 1)), up.parts)):
                        # each parity covers a quarter of the output pixels: its own range of pixel blocks
                        fused.append(self.resample([Seg(cur, taps)], p, dst, cur.H, cur.W, bnd, gn_p64=par * np_in,
                                                   gn_defer=True, out_map=(2, 2, py, px)))
                    self._gn_fill(dst, all(fused) and np_in > 0)
            else:
                assert cur.t is U[i] and cur.c0 == 0, 'non-upsampling level must have been written in place'
            cur = View.full(U[i])
            next_in_place = i > 0 and self.up_convs[k + 1] is None
            next_up = k + 1 < len(self.ups) and self.up_convs[k + 1] is not None
            bnd = None
            for li, rp in enumerate(res):
                last = li == len(res) - 1
                tgt = View(U[i - 1], 0, dc[i - 1]) if (last and next_in_place) else View.full(
                    self._new(B, H, W, rp.co, gn_sw=self._sw(rp.co)))
                bnd = layer(cur, tgt, stage, li, bound_slot(last and next_up))
                cur = tgt

        # ---------------- head: GN -> SiLU -> conv_out, NCHW output
        sc, sh = self._gn(cur, *self.norm_out)
        out = torch.empty((B, m.model_config.im_channels, S, S2), dtype=torch.float32, device=self.device)
        head = [Seg(cur, TAPS3, scale=sc, shift=sh, silu=True)]
        if self.conv_out_head is not None:
            K.head_conv(cur, sc, sh, self.conv_out_head, self.conv_out.b, out)
        elif self.conv_out.f3 is not None:
            K.conv_igemm_f16x3(head, self.conv_out.f3, self.conv_out.b, None, Hm=S, Wm=S2, out_nchw=out,
                               a_exp=K.f16x3_a_exp(*self.conv_out.gb, S * S2 * cur.C // 8))
        else:
            self.conv(head, self.conv_out, None, S, S2, out_nchw=out)
        return out
