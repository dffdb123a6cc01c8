// Host-side argument rules shared by the entry points that take a wc_conv_args: each rule is stated
// here once and returns WC_OK, WC_E_ARG or WC_E_SHAPE.  Host functions only; no kernel reads this file.
// kernels.py states the same rules for dispatch (_src_view_ok and the *_eligible / *_ok predicates).
#pragma once
#include <stdint.h>

#include "../../include/wc_kernels.h"

namespace wchost {

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The static exponents of the f16x3 operands: 2^e must stay a normal float on both sides.
inline bool exp_ok(int e) { return e >= -60 && e <= 60; }

// The taps are exactly the kh x kw grid with unit spacing whose first tap is (y0, x0), row-major.
inline bool taps_grid(const wc_conv_seg& s, int kh, int kw, int y0, int x0) {
    if (s.ntaps != kh * kw) return false;
    for (int t = 0; t < kh * kw; ++t)
        if (s.dy[t] != y0 + t / kw || s.dx[t] != x0 + t % kw) return false;
    return true;
}

// Any kh x kw grid, recovered from the tap list: tap t = (ty0 + (t / kw) * tdy, tx0 + (t % kw) * tdx).
inline int taps_any_grid(const wc_conv_seg& s, int& kh, int& kw, int& ty0, int& tdy, int& tx0, int& tdx) {
    if (s.ntaps < 1 || s.ntaps > WC_MAX_TAPS) return WC_E_SHAPE;
    for (kw = 1; kw < s.ntaps && s.dy[kw] == s.dy[0];) ++kw;
    if (s.ntaps % kw != 0) return WC_E_SHAPE;
    kh = s.ntaps / kw;
    ty0 = s.dy[0]; tdy = kh > 1 ? s.dy[kw] - s.dy[0] : 0;
    tx0 = s.dx[0]; tdx = kw > 1 ? s.dx[1] - s.dx[0] : 0;
    for (int t = 0; t < s.ntaps; ++t)
        if (s.dy[t] != ty0 + (t / kw) * tdy || s.dx[t] != tx0 + (t % kw) * tdx) return WC_E_SHAPE;
    return WC_OK;
}

// A source view read in 16-byte quads: whole cmult-channel chunks, pixel stride and base on the quad grid.
inline int check_src_layout(const wc_conv_seg& s, int cmult) {
    return (s.C <= 0 || s.C % cmult || s.ldc % 4 || !aligned16(s.src)) ? WC_E_SHAPE : WC_OK;
}

// The source-segment rule (kernels.py: _src_view_ok).  The kernels read a segment through a buffer
// resource (SRD) with a 2 GiB range and 32-bit byte offsets: an out-of-image tap gets an offset past the
// range and reads 0, so the whole view must fit.
inline int check_src_seg(const wc_conv_seg& s, int B, int cmult) {
    if (!s.src) return WC_E_ARG;
    if (check_src_layout(s, cmult) || (long)B * s.H * s.W * s.ldc * 4 >= (1L << 31)) return WC_E_SHAPE;
    return WC_OK;
}

// Segment 1, the fused residual_input_conv: a raw 1x1 read of a view on segment 0's own sampling grid,
// its K columns right after segment 0's (kbase).
inline int check_res_seg(const wc_conv_seg& s1, const wc_conv_seg& s0, long kbase, int B, int cmult) {
    if (!s1.src || s1.scale) return WC_E_ARG;
    if (!taps_grid(s1, 1, 1, 0, 0) || s1.H != s0.H || s1.W != s0.W || s1.sy != s0.sy || s1.sx != s0.sx ||
        s1.kbase != kbase)
        return WC_E_SHAPE;
    return check_src_seg(s1, B, cmult);
}

// The halo kernels' output: a plain NHWC view on the up x main grid (up = 1, or 2 for the transposed
// conv's parities).  Their epilogues address one image of the output / residual with 32-bit offsets
// from the image's base, so one image must stay under 2 GiB; res_quads: the residual is read in quads.
inline int check_out_grid(const wc_conv_args* a, int up, bool res_quads) {
    if (a->out_nchw || a->Ho != up * a->Hm || a->Wo != up * a->Wm || a->osy != up || a->osx != up || a->ooy || a->oox)
        return WC_E_SHAPE;
    const long pix = (long)up * up * a->Hm * a->Wm;
    if (pix * a->ldo * 4 >= (1L << 31)) return WC_E_SHAPE;
    if (a->res && (pix * a->ldres * 4 >= (1L << 31) || (res_quads && a->ldres % 4))) return WC_E_SHAPE;
    return WC_OK;
}

// GroupNorm tile partials from the epilogue (wcx6::gn_tile_partials): the N written channels are whole
// 32-channel blocks at a 32-aligned offset of the gn_ncb blocks; the pixels are 64-pixel blocks of the
// tensor's gn_np64 per image -- all of them (window false: the halo kernels, whose tiles never straddle
// images), or the NHWC rows gn_p64 .. of the implicit GEMM (window true; its tiles must also lie inside
// one image, which its dispatch checks against the M tile).  Sets the partials' fields of a device
// parameter struct (X6Dev, WDev, IgDev).
template <class Dev>
inline int set_gn_part(Dev& d, const wc_conv_args* a, int pixels_per_image, bool window) {
    d.gn_part = a->gn_part;
    if (!a->gn_part) return WC_OK;
    const int sw = a->gn_sw;
    if ((sw != 4 && sw != 8 && sw != 16 && sw != 32) || a->N % 32 || a->gn_c0 % 32 || a->gn_c0 < 0 ||
        a->gn_c0 + a->N > a->gn_ncb * 32)
        return WC_E_SHAPE;
    if (window ? (a->out_nchw || pixels_per_image % 64 || a->gn_p64 < 0 || a->gn_p64 + pixels_per_image / 64 > a->gn_np64)
               : (a->gn_p64 != 0 || a->gn_np64 * 64 != pixels_per_image))
        return WC_E_SHAPE;
    d.gn_ncb = a->gn_ncb; d.gn_sw = sw; d.gn_c0 = a->gn_c0; d.gn_np64 = a->gn_np64;
    return WC_OK;
}

}  // namespace wchost
