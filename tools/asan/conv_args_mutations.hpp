// Single-fault pinning of the fifteen entry points that take a wc_conv_args (included by abi_validation.cpp).
//
// Each entry point starts from one argument set it would accept (B 1, 16 x 16, C 32, N 64 / 128 / 256; host
// buffers stand in for device pointers) and is called only with that set plus ONE mutation, each with the exact
// WC_E_* status it must return.  The accepted set itself is never passed: it would launch.  The expectations
// are the library's answers as they stand; a change to the host validation must leave every one unchanged.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "wc_kernels.h"

namespace mut {

constexpr int A = WC_E_ARG, S = WC_E_SHAPE;

alignas(16) static float g_buf[1 << 12];
static float* const p = g_buf;
static char* const p4 = reinterpret_cast<char*>(g_buf) + 4;  // a base 4 bytes off the 16-byte grid

// Everything any of the entry points takes besides the stream.
struct Case {
    wc_conv_args a;
    bool null_a = false;
    const void* w = p;
    int64_t w_bytes = 0;
    int a_exp = 0;
    const float* wsinv = p;
    const float* bound = nullptr;
    const void* aux = p;  // a3 / vpre / vout
    int64_t aux_bytes = 0;
    void* qkv3 = p;
    int C = 0, heads = 1;
    int exps[3] = {0, 0, 0};
    bool null_exps = false;
    wc_gnb_epi g;
    bool null_g = false;
    const wc_conv_args* args() const { return null_a ? nullptr : &a; }
};

using Fn = std::function<void(Case&)>;
struct Mut {
    const char* name;
    Fn f;
    int want;
};
using Muts = std::vector<Mut>;

static wc_conv_seg grid_seg(int k, int C, int ldc, int H, int W, int stride) {
    wc_conv_seg s;
    std::memset(&s, 0, sizeof(s));
    s.src = p; s.C = C; s.ldc = ldc; s.H = H; s.W = W; s.sy = s.sx = stride;
    s.ntaps = k * k;
    for (int t = 0; t < k * k; ++t) {
        s.dy[t] = k == 1 ? 0 : t / k - 1;
        s.dx[t] = k == 1 ? 0 : t % k - 1;
    }
    return s;
}

// One k x k segment, output a plain NHWC view on the `up` x main grid.
static Case base_case(int k, int C, int H, int W, int stride, int Hm, int Wm, int N, int up = 1) {
    Case c;
    std::memset(&c.a, 0, sizeof(c.a));
    std::memset(&c.g, 0, sizeof(c.g));
    c.a.seg[0] = grid_seg(k, C, C, H, W, stride);
    c.a.nseg = 1;
    c.a.B = 1; c.a.Hm = Hm; c.a.Wm = Wm; c.a.N = N;
    c.a.w = p; c.a.ldw = k * k * C;
    c.a.out = p; c.a.ldo = N;
    c.a.Ho = up * Hm; c.a.Wo = up * Wm; c.a.osy = c.a.osx = up;
    return c;
}

static void add_gn_prologue(Case& c, bool silu) {
    c.a.seg[0].scale = p; c.a.seg[0].shift = p; c.a.seg[0].silu = silu;
}

static void add_res_seg(Case& c) {  // the fused 1x1 residual: 32 raw channels at the same pixel
    const wc_conv_seg& s0 = c.a.seg[0];
    c.a.seg[1] = grid_seg(1, 32, 32, s0.H, s0.W, s0.sy);
    c.a.seg[1].kbase = s0.ntaps * s0.C;
    c.a.nseg = 2;
    c.a.ldw += 32;
}

static void add_gn_part(Case& c, int pixels) {  // tile partials of an N-channel tensor
    c.a.gn_part = p; c.a.gn_sw = 8; c.a.gn_ncb = c.a.N / 32; c.a.gn_c0 = 0; c.a.gn_p64 = 0; c.a.gn_np64 = pixels / 64;
}

static Muts cat(std::initializer_list<Muts> parts) {
    Muts r;
    for (const Muts& m : parts) r.insert(r.end(), m.begin(), m.end());
    return r;
}

// ---- mutation families ----
static Muts m_struct() {
    return {{"null a", [](Case& c) { c.null_a = true; }, A},
            {"null weights", [](Case& c) { c.w = nullptr; c.a.w = nullptr; }, A},
            {"null out", [](Case& c) { c.a.out = nullptr; }, A},
            {"nseg 0", [](Case& c) { c.a.nseg = 0; }, A},
            {"nseg 3", [](Case& c) { c.a.nseg = 3; }, A},
            {"null seg[0].src", [](Case& c) { c.a.seg[0].src = nullptr; }, A},
            {"weight base +4 bytes", [](Case& c) { c.w = p4; c.a.w = reinterpret_cast<const float*>(p4); }, S}};
}

// the source-segment rule on segment i; `range_ldc` puts B*H*W*ldc*4 at 2^31
static Muts m_src(int i, int range_ldc) {
    return {{i ? "seg1 C 0" : "C 0", [i](Case& c) { c.a.seg[i].C = 0; }, S},
            {i ? "seg1 C 24" : "C 24", [i](Case& c) { c.a.seg[i].C = 24; }, S},
            {i ? "seg1 ldc 34" : "ldc 34", [i](Case& c) { c.a.seg[i].ldc = 34; }, S},
            {i ? "seg1 base +4 bytes" : "source base +4 bytes",
             [i](Case& c) { c.a.seg[i].src = reinterpret_cast<const float*>(p4); }, S},
            {i ? "seg1 B*H*W*ldc*4 at 2^31" : "B*H*W*ldc*4 at 2^31", [i, range_ldc](Case& c) { c.a.seg[i].ldc = range_ldc; },
             S}};
}

static Muts m_scale_without_shift() {
    return {{"scale without shift", [](Case& c) { c.a.seg[0].scale = p; c.a.seg[0].shift = nullptr; }, A}};
}

static Muts m_taps(int last) {  // an exact grid of last + 1 taps
    return {{"a tap moved", [](Case& c) { c.a.seg[0].dy[c.a.seg[0].ntaps / 2] += 1; }, S},
            {"ntaps one short", [last](Case& c) { c.a.seg[0].ntaps = last; }, S},
            {"kbase 16", [](Case& c) { c.a.seg[0].kbase = 16; }, S}};
}

static Muts m_stride(int bad) {
    return {{"segment stride", [bad](Case& c) { c.a.seg[0].sy = c.a.seg[0].sx = bad; }, S}};
}

// Hm / Wm off the tile with the source following (so only the tile rule breaks), and a source off the grid
static Muts m_tile(int in_per_out) {
    return {{"Hm 12", [in_per_out](Case& c) { c.a.Hm = 12; c.a.Ho = 12 * c.a.osy; c.a.seg[0].H = 12 * in_per_out; }, S},
            {"Wm 24", [in_per_out](Case& c) { c.a.Wm = 24; c.a.Wo = 24 * c.a.osx; c.a.seg[0].W = 24 * in_per_out; }, S},
            {"seg[0].H off the main grid", [](Case& c) { c.a.seg[0].H += 8; }, S},
            {"B 0", [](Case& c) { c.a.B = 0; }, S}};
}

static Muts m_res_seg() {  // on a two-segment base
    return cat({{{"seg1 null src", [](Case& c) { c.a.seg[1].src = nullptr; }, A},
                 {"seg1 with a scale", [](Case& c) { c.a.seg[1].scale = p; }, A},
                 {"seg1 3 taps", [](Case& c) { c.a.seg[1].ntaps = 3; }, S},
                 {"seg1 tap off the pixel", [](Case& c) { c.a.seg[1].dx[0] = 1; }, S},
                 {"seg1 kbase wrong", [](Case& c) { c.a.seg[1].kbase += 16; }, S},
                 {"seg1 H != seg0 H", [](Case& c) { c.a.seg[1].H += 8; }, S},
                 {"seg1 stride 2", [](Case& c) { c.a.seg[1].sy = c.a.seg[1].sx = 2; }, S}},
                m_src(1, 1 << 21)});
}

// output on the up x main grid; range_ld puts one image of out / res at 2^31 bytes
static Muts m_out_grid(int range_ld) {
    return {{"out_nchw", [](Case& c) { c.a.out_nchw = 1; }, S},
            {"osy off", [](Case& c) { c.a.osy = 3 - c.a.osy; }, S},
            {"ooy 1", [](Case& c) { c.a.ooy = 1; }, S},
            {"Ho off the grid", [](Case& c) { c.a.Ho += 1; }, S},
            {"one image of out at 2^31 bytes", [range_ld](Case& c) { c.a.ldo = range_ld; }, S},
            {"one image of res at 2^31 bytes", [range_ld](Case& c) { c.a.res = p; c.a.ldres = range_ld; }, S}};
}

// GroupNorm tile partials on a base that carries them; halo: the kernels that take gn_p64 == 0 only
static Muts m_gn(bool halo) {
    Muts m = {{"gn_sw 12", [](Case& c) { c.a.gn_sw = 12; }, S},
              {"gn: N 48", [](Case& c) { c.a.N = 48; }, S},
              {"gn_c0 16", [](Case& c) { c.a.gn_c0 = 16; }, S},
              {"gn_c0 + N past gn_ncb * 32", [](Case& c) { c.a.gn_c0 = 32; }, S},
              {"gn_np64 wrong", [](Case& c) { c.a.gn_np64 -= 1; }, S}};
    if (halo) m.push_back({"gn_p64 1", [](Case& c) { c.a.gn_p64 = 1; c.a.gn_np64 += 1; }, S});
    else m.push_back({"gn_p64 past the window", [](Case& c) { c.a.gn_p64 = 1; }, S});
    return m;
}

static Muts m_wbytes() {
    return {{"weight bytes off by 16", [](Case& c) { c.w_bytes += 16; }, S}};
}

static Muts m_a_exp() {
    return {{"a_exp 61", [](Case& c) { c.a_exp = 61; }, A},
            {"a_exp -61", [](Case& c) { c.a_exp = -61; }, A},
            {"null w_inv_scale", [](Case& c) { c.wsinv = nullptr; }, A}};
}

static int failures = 0, checks = 0;

static void run(const char* entry, const std::function<int(const Case&)>& call, const Case& base, const Muts& muts) {
    for (const Mut& m : muts) {
        Case c = base;
        m.f(c);
        const int got = call(c);
        ++checks;
        if (got != m.want) {
            std::printf("FAIL %s [%s] -> %d (want %d)\n", entry, m.name, got, m.want);
            ++failures;
        }
    }
}

// ---- the entry points ----
static int c_igemm(const Case& c) { return wc_conv_igemm(c.args(), nullptr); }
static int c_igemm_x6(const Case& c) { return wc_conv_igemm_x6(c.args(), c.w, c.w_bytes, nullptr); }
static int c_igemm_f3(const Case& c) {
    return wc_conv_igemm_f16x3(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.bound, nullptr);
}
static int c_igemm_qkv(const Case& c) {
    return wc_conv_igemm_f16x3_qkv(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.qkv3, c.C, c.heads,
                                   c.null_exps ? nullptr : c.exps, nullptr);
}
static int c_proj(const Case& c) {
    return wc_proj_f16x3(c.args(), c.aux, c.aux_bytes, c.w, c.w_bytes, c.a_exp, c.wsinv, nullptr);
}
static int c_proj_qkv(const Case& c) {
    return wc_proj_f16x3_qkv(c.args(), c.aux, c.aux_bytes, c.w, c.w_bytes, c.a_exp, c.wsinv, c.qkv3, c.C, c.heads,
                             c.null_exps ? nullptr : c.exps, nullptr);
}
static int c_x6(const Case& c) { return wc_conv3x3_x6(c.args(), c.w, c.w_bytes, nullptr); }
static int c_f3(const Case& c) {
    return wc_conv3x3_f16x3(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.bound, nullptr);
}
static int c_s2d(const Case& c) { return wc_conv4x4s2_f16x3(c.args(), c.w, c.w_bytes, c.wsinv, c.bound, nullptr); }
static int c_convtr(const Case& c) {
    return wc_convtr4x4s2_f16x3(c.args(), c.w, c.w_bytes, c.wsinv, c.bound, nullptr);
}
static int c_wino(const Case& c) {
    return wc_conv3x3_wino_f16x3(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.bound, nullptr);
}
static int c_wino_gnb(const Case& c) {
    return wc_conv3x3_wino_f16x3_gnb(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.bound, c.null_g ? nullptr : &c.g,
                                     nullptr);
}
static int c_wino_vp(const Case& c) {
    return wc_conv3x3_wino_f16x3_vp(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.bound, c.aux, c.aux_bytes, nullptr);
}
static int c_wino_vp8(const Case& c) {
    return wc_conv3x3_wino_f16x3_vp8(c.args(), c.w, c.w_bytes, c.a_exp, c.wsinv, c.bound, c.aux, c.aux_bytes, nullptr);
}
static int c_vsplit(const Case& c) {
    return wc_wino_vsplit_f16x3(c.args(), c.a_exp, c.bound, const_cast<void*>(c.aux), c.aux_bytes, nullptr);
}

static int64_t vbytes(int B, int C, int H, int W) {
    int64_t b = 0;
    wc_wino_vsplit_bytes(B, C, H, W, &b);
    return b;
}

static void implicit_gemm() {
    // wc_conv_igemm (fp32): C % 32, any tap grid and stride, any output map
    Case b = base_case(3, 32, 16, 16, 1, 16, 16, 64);
    run("wc_conv_igemm", c_igemm, b,
        cat({m_struct(), m_src(0, 1 << 21), m_scale_without_shift(), m_taps(8),
             {{"C 16", [](Case& c) { c.a.seg[0].C = 16; }, S},
              {"ntaps 0", [](Case& c) { c.a.seg[0].ntaps = 0; }, S},
              {"ntaps 17", [](Case& c) { c.a.seg[0].ntaps = 17; }, S},
              {"act 5", [](Case& c) { c.a.act = 5; }, A},
              {"act -1", [](Case& c) { c.a.act = -1; }, A},
              {"PReLU without slopes", [](Case& c) { c.a.act = WC_ACT_PRELU; }, A},
              {"activation behind a GN prologue", [](Case& c) { add_gn_prologue(c, false); c.a.act = WC_ACT_GELU; }, A},
              {"absmax_out", [](Case& c) { c.a.absmax_out = p; }, A},
              {"gn_part", [](Case& c) { c.a.gn_part = p; }, A},
              {"ldw short of K", [](Case& c) { c.a.ldw -= 4; }, S},
              {"ldw 290", [](Case& c) { c.a.ldw = 290; }, S},
              {"N 0", [](Case& c) { c.a.N = 0; }, S},
              {"B 0", [](Case& c) { c.a.B = 0; }, S}}}));
    Case b2 = b;
    add_res_seg(b2);
    run("wc_conv_igemm (residual segment)", c_igemm, b2, m_res_seg());

    // prepare() of wc_igemm6.hip through its two plain entry points
    Case x = base_case(3, 32, 16, 16, 1, 16, 16, 128);
    x.w_bytes = (288 / 16) * 128 * 96;
    const Muts prep = cat({m_struct(), m_src(0, 1 << 21), m_scale_without_shift(), m_taps(8), m_wbytes(),
                           {{"ntaps 0", [](Case& c) { c.a.seg[0].ntaps = 0; }, S},
                            {"act 3", [](Case& c) { c.a.act = 3; }, A},
                            {"N 0", [](Case& c) { c.a.N = 0; }, S},
                            {"B 0", [](Case& c) { c.a.B = 0; }, S},
                            {"one image of out at 2^31 bytes", [](Case& c) { c.a.ldo = 1 << 21; }, S},
                            {"one image of res at 2^31 bytes", [](Case& c) { c.a.res = p; c.a.ldres = 1 << 21; }, S}}});
    run("wc_conv_igemm_x6", c_igemm_x6, x, prep);
    Case x2 = x;
    add_res_seg(x2);
    x2.w_bytes = (320 / 16) * 128 * 96;
    run("wc_conv_igemm_x6 (residual segment)", c_igemm_x6, x2, m_res_seg());
    Case xg = x;
    add_gn_part(xg, 256);
    run("wc_conv_igemm_x6 (GN partials)", c_igemm_x6, xg,
        cat({m_gn(false),
             {{"gn with out_nchw", [](Case& c) { c.a.out_nchw = 1; }, S},
              {"gn with tiles that straddle images",
               [](Case& c) { c.a.Hm = c.a.Ho = c.a.seg[0].H = 12; c.a.gn_np64 = 3; }, S}}}));

    Case f = x;
    f.w_bytes = (288 / 16) * 128 * 64;
    run("wc_conv_igemm_f16x3", c_igemm_f3, f,
        cat({prep, m_a_exp(),
             {{"a_bound with tiles that straddle images",
               [](Case& c) { c.bound = p; c.a.Hm = c.a.Ho = c.a.seg[0].H = 12; }, S},
              {"epilogue activation", [](Case& c) { c.a.act = WC_ACT_GELU; }, A}}}));
    Case f2 = f;
    add_res_seg(f2);
    f2.w_bytes = 18 * 128 * 64 + 2 * 128 * 96;
    run("wc_conv_igemm_f16x3 (residual segment)", c_igemm_f3, f2, m_res_seg());

    // the attention in-projection written pre-split: 1x1, C 32, one head, N 96; out is not used
    Case q = base_case(1, 32, 16, 16, 1, 16, 16, 96);
    add_gn_prologue(q, false);
    q.a.out = nullptr;
    q.C = 32; q.heads = 1;
    q.w_bytes = 2 * 128 * 64;
    const Muts qkv = {{"null qkv3", [](Case& c) { c.qkv3 = nullptr; }, A},
                      {"null exps", [](Case& c) { c.null_exps = true; }, A},
                      {"qkv3 base +4 bytes", [](Case& c) { c.qkv3 = p4; }, S},
                      {"heads 3", [](Case& c) { c.heads = 3; }, S},
                      {"head dim 16", [](Case& c) { c.heads = c.C / 16; }, S},
                      {"N != 3 C", [](Case& c) { c.C = 64; c.heads = 2; }, S},
                      {"res", [](Case& c) { c.a.res = p; c.a.ldres = 96; }, A},
                      {"temb", [](Case& c) { c.a.temb = p; }, A},
                      {"absmax_out", [](Case& c) { c.a.absmax_out = p; }, A},
                      {"gn_part", [](Case& c) { c.a.gn_part = p; }, A},
                      {"out_nchw", [](Case& c) { c.a.out_nchw = 1; }, A},
                      {"exps[1] 61", [](Case& c) { c.exps[1] = 61; }, A}};
    run("wc_conv_igemm_f16x3_qkv", c_igemm_qkv, q,
        cat({qkv, m_a_exp(), m_src(0, 1 << 21), m_wbytes(), m_stride(2),
             {{"null a", [](Case& c) { c.null_a = true; }, A},
              {"null weights", [](Case& c) { c.w = nullptr; }, A},
              {"weight base +4 bytes", [](Case& c) { c.w = p4; }, S},
              {"nseg 2", [](Case& c) { c.a.nseg = 2; }, A},
              {"act 1", [](Case& c) { c.a.act = 1; }, A},
              {"scale without shift", [](Case& c) { c.a.seg[0].shift = nullptr; }, A},
              {"a tap moved", [](Case& c) { c.a.seg[0].dy[0] = 1; }, S},
              {"ntaps 9", [](Case& c) { c.a.seg[0] = grid_seg(3, 32, 32, 16, 16, 1); add_gn_prologue(c, false); }, S},
              {"Hm 12", [](Case& c) { c.a.Hm = c.a.seg[0].H = 12; }, S}}}));

    // the projections on a pre-split A operand
    Case pj = base_case(1, 32, 16, 16, 1, 16, 16, 128);
    pj.aux_bytes = 256 * 32 * 4;
    pj.w_bytes = 2 * 128 * 64;
    const Muts pa = {{"null a3", [](Case& c) { c.aux = nullptr; }, A},
                     {"a3 base +4 bytes", [](Case& c) { c.aux = p4; }, A},
                     {"a3 bytes off by 16", [](Case& c) { c.aux_bytes += 16; }, S},
                     {"GN prologue", [](Case& c) { add_gn_prologue(c, false); }, A},
                     {"act 1", [](Case& c) { c.a.act = 1; }, A},
                     {"nseg 2", [](Case& c) { c.a.nseg = 2; }, A},
                     {"a tap moved", [](Case& c) { c.a.seg[0].dy[0] = 1; }, S},
                     {"seg[0].H off the main grid", [](Case& c) { c.a.seg[0].H += 8; }, S},
                     {"Hm 12", [](Case& c) { c.a.Hm = c.a.Ho = c.a.seg[0].H = 12; }, S},
                     {"C 48", [](Case& c) { c.a.seg[0].C = 48; c.a.seg[0].ldc = 48; }, S},
                     {"null a", [](Case& c) { c.null_a = true; }, A},
                     {"null weights", [](Case& c) { c.w = nullptr; }, A},
                     {"weight base +4 bytes", [](Case& c) { c.w = p4; }, S},
                     {"null seg[0].src", [](Case& c) { c.a.seg[0].src = nullptr; }, A}};
    run("wc_proj_f16x3", c_proj, pj,
        cat({pa, m_a_exp(), m_src(0, 1 << 21), m_wbytes(), m_stride(2),
             {{"null out", [](Case& c) { c.a.out = nullptr; }, A},
              {"N 64", [](Case& c) { c.a.N = 64; }, S},
              {"osy 2", [](Case& c) { c.a.osy = 2; }, S},
              {"ldo 130", [](Case& c) { c.a.ldo = 130; }, S},
              {"out base +4 bytes", [](Case& c) { c.a.out = reinterpret_cast<float*>(p4); }, S},
              {"ldres 130", [](Case& c) { c.a.res = p; c.a.ldres = 130; }, S},
              {"res base +4 bytes", [](Case& c) { c.a.res = reinterpret_cast<float*>(p4); c.a.ldres = 128; }, S},
              {"temb", [](Case& c) { c.a.temb = p; }, A}}}));
    Case pjg = pj;
    add_gn_part(pjg, 256);
    run("wc_proj_f16x3 (GN partials)", c_proj, pjg, m_gn(false));

    Case pq = base_case(1, 128, 16, 16, 1, 16, 16, 384);
    pq.a.out = nullptr;
    pq.C = 128; pq.heads = 4;
    pq.aux_bytes = 256 * 128 * 4;
    pq.w_bytes = 3 * 8 * 128 * 64;
    run("wc_proj_f16x3_qkv", c_proj_qkv, pq,
        cat({qkv, pa, m_a_exp(), m_wbytes(), m_stride(2),
             {{"C 0", [](Case& c) { c.a.seg[0].C = 0; }, S},
              {"ldc 130", [](Case& c) { c.a.seg[0].ldc = 130; }, S},
              {"source base +4 bytes", [](Case& c) { c.a.seg[0].src = reinterpret_cast<const float*>(p4); }, S},
              {"B*H*W*ldc*4 at 2^31", [](Case& c) { c.a.seg[0].ldc = 1 << 21; }, S}}}));
}

static void halo_convs() {
    // prepare() of wc_conv6.hip: 3x3 stride 1 on the output's own grid, TH 8 (N 128) and TH 16 (N 64)
    const Muts prep = cat({m_struct(), m_src(0, 1 << 21), m_scale_without_shift(), m_taps(8), m_stride(2), m_tile(1),
                           m_out_grid(1 << 21), m_wbytes(),
                           {{"act 3", [](Case& c) { c.a.act = 3; }, A}, {"N 0", [](Case& c) { c.a.N = 0; }, S}}});
    Case x = base_case(3, 32, 16, 16, 1, 16, 16, 128);
    x.w_bytes = 18 * 128 * 96;
    run("wc_conv3x3_x6", c_x6, x, prep);
    Case x64 = base_case(3, 32, 16, 16, 1, 16, 16, 64);
    x64.w_bytes = 18 * 64 * 96;
    run("wc_conv3x3_x6 (N 64)", c_x6, x64,
        {{"Hm 8 under the 16-row tile", [](Case& c) { c.a.Hm = c.a.Ho = c.a.seg[0].H = 8; }, S},
         {"weight bytes off by 16", [](Case& c) { c.w_bytes += 16; }, S}});
    Case x2 = x;
    add_res_seg(x2);
    x2.w_bytes = 20 * 128 * 96;
    run("wc_conv3x3_x6 (residual segment)", c_x6, x2, m_res_seg());
    Case xg = x;
    add_gn_part(xg, 256);
    run("wc_conv3x3_x6 (GN partials)", c_x6, xg, m_gn(true));

    Case f = x;
    add_gn_prologue(f, true);
    f.w_bytes = 18 * 128 * 64;
    run("wc_conv3x3_f16x3", c_f3, f,
        cat({prep, m_a_exp(),
             {{"raw segment without a_bound", [](Case& c) { c.a.seg[0].scale = c.a.seg[0].shift = nullptr; }, A}}}));
    Case f2 = f;
    add_res_seg(f2);
    f2.w_bytes = 18 * 128 * 64 + 2 * 128 * 96;
    run("wc_conv3x3_f16x3 (residual segment)", c_f3, f2,
        cat({m_res_seg(),
             {{"raw segment 0 beside a residual segment",
               [](Case& c) { c.a.seg[0].scale = c.a.seg[0].shift = nullptr; c.bound = p; c.w_bytes = 20 * 128 * 64; }, A}}}));
    Case fg = f;
    add_gn_part(fg, 256);
    run("wc_conv3x3_f16x3 (GN partials)", c_f3, fg, m_gn(true));

    // the 4x4 stride-2 down conv: input 16 x 32, output 8 x 16, N 128
    const Muts raw16 = {{"null a", [](Case& c) { c.null_a = true; }, A},
                        {"null weights", [](Case& c) { c.w = nullptr; }, A},
                        {"null out", [](Case& c) { c.a.out = nullptr; }, A},
                        {"null w_inv_scale", [](Case& c) { c.wsinv = nullptr; }, A},
                        {"null a_bound", [](Case& c) { c.bound = nullptr; }, A},
                        {"nseg 0", [](Case& c) { c.a.nseg = 0; }, A},
                        {"nseg 2", [](Case& c) { c.a.nseg = 2; }, A},
                        {"act 1", [](Case& c) { c.a.act = 1; }, A},
                        {"null seg[0].src", [](Case& c) { c.a.seg[0].src = nullptr; }, A},
                        {"GN prologue", [](Case& c) { add_gn_prologue(c, true); }, A},
                        {"weight base +4 bytes", [](Case& c) { c.w = p4; }, S},
                        {"kbase 16", [](Case& c) { c.a.seg[0].kbase = 16; }, S},
                        {"ldres 130", [](Case& c) { c.a.res = p; c.a.ldres = 130; }, S}};
    Case d = base_case(4, 32, 16, 32, 2, 8, 16, 128);
    d.bound = p;
    d.w_bytes = 4 * 8 * 128 * 64;
    run("wc_conv4x4s2_f16x3", c_s2d, d,
        cat({raw16, m_src(0, 1 << 20), m_stride(1), m_tile(2), m_out_grid(1 << 22), m_wbytes(),
             {{"a tap moved", [](Case& c) { c.a.seg[0].dy[8] += 1; }, S},
              {"ntaps 15", [](Case& c) { c.a.seg[0].ntaps = 15; }, S},
              {"N 64", [](Case& c) { c.a.N = 64; c.a.ldo = 64; c.w_bytes = 4 * 8 * 64 * 64; }, S}}}));
    Case dg = d;
    add_gn_part(dg, 128);
    run("wc_conv4x4s2_f16x3 (GN partials)", c_s2d, dg, m_gn(true));

    // the 4x4 stride-2 transposed conv: input 16 x 16, output 32 x 32 (the taps are the kernel's own)
    Case t = base_case(3, 32, 16, 16, 1, 16, 16, 128, 2);
    t.bound = p;
    t.w_bytes = 16 * 2 * 128 * 64;
    run("wc_convtr4x4s2_f16x3", c_convtr, t,
        cat({raw16, m_src(0, 1 << 21), m_stride(2), m_tile(1), m_out_grid(1 << 19), m_wbytes(),
             {{"N 0", [](Case& c) { c.a.N = 0; }, S}, {"temb", [](Case& c) { c.a.temb = p; }, S}}}));
    Case t64 = base_case(3, 32, 16, 16, 1, 16, 16, 64, 2);
    t64.bound = p;
    t64.w_bytes = 16 * 2 * 64 * 64;
    run("wc_convtr4x4s2_f16x3 (N 64)", c_convtr, t64,
        {{"Hm 8 under the 16-row tile", [](Case& c) { c.a.Hm = c.a.seg[0].H = 8; c.a.Ho = 16; }, S}});
    Case tg = t;
    add_gn_part(tg, 4 * 256);
    run("wc_convtr4x4s2_f16x3 (GN partials)", c_convtr, tg, m_gn(true));
}

static void winograd() {
    // wino_setup: GN + SiLU segment 0 (+ residual under a_bound), or one raw segment under a_bound
    const Muts setup = cat({m_struct(), m_src(0, 1 << 21), m_scale_without_shift(), m_taps(8), m_stride(2), m_tile(1),
                            m_out_grid(1 << 21), m_wbytes(), m_a_exp(),
                            {{"act 1", [](Case& c) { c.a.act = 1; }, A}, {"N 0", [](Case& c) { c.a.N = 0; }, S}}});
    Case w = base_case(3, 32, 16, 16, 1, 16, 16, 128);
    add_gn_prologue(w, true);
    w.w_bytes = 24 * 128 * 64;
    run("wc_conv3x3_wino_f16x3", c_wino, w,
        cat({setup,
             {{"GN prologue without SiLU", [](Case& c) { c.a.seg[0].silu = 0; }, A},
              {"raw segment without a_bound", [](Case& c) { c.a.seg[0].scale = c.a.seg[0].shift = nullptr; }, A}}}));
    Case w64 = base_case(3, 32, 16, 16, 1, 16, 16, 64);
    add_gn_prologue(w64, true);
    w64.w_bytes = 24 * 64 * 64;
    run("wc_conv3x3_wino_f16x3 (N 64)", c_wino, w64,
        {{"Hm 8 under the 16-row tile", [](Case& c) { c.a.Hm = c.a.Ho = c.a.seg[0].H = 8; }, S}});
    Case w2 = w;
    add_res_seg(w2);
    w2.bound = p;
    w2.w_bytes = 26 * 128 * 64;
    run("wc_conv3x3_wino_f16x3 (residual segment)", c_wino, w2,
        cat({m_res_seg(),
             {{"residual segment without a_bound", [](Case& c) { c.bound = nullptr; }, A},
              {"raw segment 0 beside a residual segment",
               [](Case& c) { c.a.seg[0].scale = c.a.seg[0].shift = nullptr; }, A}}}));
    Case wg = w;
    add_gn_part(wg, 256);
    run("wc_conv3x3_wino_f16x3 (GN partials)", c_wino, wg, m_gn(true));

    // the raw data-gradient form with the GroupNorm backward's sums
    Case gb = base_case(3, 32, 16, 16, 1, 16, 16, 128);
    gb.bound = p;
    gb.w_bytes = 24 * 128 * 64;
    gb.g.x = p; gb.g.ldx = 128; gb.g.sc0 = p; gb.g.sh0 = p; gb.g.part = p;
    gb.g.splits = wc_conv3x3_wino_gnb_splits(128, 16, 16);
    run("wc_conv3x3_wino_f16x3_gnb", c_wino_gnb, gb,
        cat({setup,
             {{"null a_bound", [](Case& c) { c.bound = nullptr; }, A},
              {"null g", [](Case& c) { c.null_g = true; }, A},
              {"null g.x", [](Case& c) { c.g.x = nullptr; }, A},
              {"null g.part", [](Case& c) { c.g.part = nullptr; }, A},
              {"GN prologue", [](Case& c) { add_gn_prologue(c, true); }, A},
              {"g.ldx below N", [](Case& c) { c.g.ldx = 64; }, S},
              {"g.splits wrong", [](Case& c) { c.g.splits += 1; }, S},
              {"B*H*W*ldx*4 at 2^31", [](Case& c) { c.g.ldx = 1 << 21; }, S}}}));

    // the pre-split forms
    const Muts vp = {{"null vpre", [](Case& c) { c.aux = nullptr; }, A},
                     {"vpre base +4 bytes", [](Case& c) { c.aux = p4; }, A},
                     {"v_bytes off by 16", [](Case& c) { c.aux_bytes += 16; }, S},
                     {"raw segment 0", [](Case& c) { c.a.seg[0].scale = c.a.seg[0].shift = nullptr; c.bound = p; }, A}};
    Case v = w;
    v.aux_bytes = vbytes(1, 32, 16, 16);
    run("wc_conv3x3_wino_f16x3_vp", c_wino_vp, v, cat({setup, vp}));
    Case v2 = w2;
    v2.aux_bytes = v.aux_bytes;
    run("wc_conv3x3_wino_f16x3_vp (residual segment)", c_wino_vp, v2, m_res_seg());
    Case v8 = base_case(3, 32, 16, 16, 1, 16, 16, 256);
    add_gn_prologue(v8, true);
    v8.w_bytes = 2 * 24 * 128 * 64;
    v8.aux_bytes = v.aux_bytes;
    run("wc_conv3x3_wino_f16x3_vp8", c_wino_vp8, v8,
        cat({setup, vp,
             {{"N 384", [](Case& c) { c.a.N = c.a.ldo = 384; c.w_bytes = 3 * 24 * 128 * 64; }, S},
              {"N 64", [](Case& c) { c.a.N = c.a.ldo = 64; c.w_bytes = 24 * 64 * 64; }, S}}}));

    Case vs = w;
    vs.aux_bytes = v.aux_bytes;
    run("wc_wino_vsplit_f16x3", c_vsplit, vs,
        {{"null a", [](Case& c) { c.null_a = true; }, A},
         {"null vout", [](Case& c) { c.aux = nullptr; }, A},
         {"nseg 0", [](Case& c) { c.a.nseg = 0; }, A},
         {"nseg 3", [](Case& c) { c.a.nseg = 3; }, A},
         {"null seg[0].src", [](Case& c) { c.a.seg[0].src = nullptr; }, A},
         {"scale without shift", [](Case& c) { c.a.seg[0].shift = nullptr; }, A},
         {"raw segment 0", [](Case& c) { c.a.seg[0].scale = c.a.seg[0].shift = nullptr; }, A},
         {"GN prologue without SiLU", [](Case& c) { c.a.seg[0].silu = 0; }, A},
         {"residual segment without a_bound", [](Case& c) { add_res_seg(c); }, A},
         {"a_exp 61", [](Case& c) { c.a_exp = 61; }, A},
         {"C 0", [](Case& c) { c.a.seg[0].C = 0; c.aux_bytes = 0; }, S},
         {"C 24", [](Case& c) { c.a.seg[0].C = 24; }, S},
         {"ldc 34", [](Case& c) { c.a.seg[0].ldc = 34; }, S},
         {"source base +4 bytes", [](Case& c) { c.a.seg[0].src = reinterpret_cast<const float*>(p4); }, S},
         {"W 24", [](Case& c) { c.a.seg[0].W = 24; c.aux_bytes = vbytes(1, 32, 16, 16) / 16 * 24; }, S},
         {"W 272", [](Case& c) { c.a.seg[0].W = 272; c.aux_bytes = vbytes(1, 32, 16, 272); }, S},
         {"vout base +4 bytes", [](Case& c) { c.aux = p4; }, S},
         {"v_bytes off by 16", [](Case& c) { c.aux_bytes += 16; }, S}});
}

// Runs every mutation; returns the number of expectations missed.
static int run_all() {
    implicit_gemm();
    halo_convs();
    winograd();
    std::printf("conv_args_mutations: %d single-fault calls, %d failure(s)\n", checks, failures);
    return failures;
}

}  // namespace mut
