// Training-input kernel: the reference loader's transform chain (diffusion_model/train_ddpm.py:150-159,
// translation.py:136-143) on uploaded image bytes,
//   Resize(S, BILINEAR) -> crop(S) -> horizontal flip -> ToTensor -> x * 2 - 1,
// where Resize on a PIL image is Pillow's antialiased two-pass resample in 8-bit fixed point
// (include/wc_data.h states the arithmetic).  Integer arithmetic, so the result is Pillow's bit for bit.
//
// One launch per batch over a DEVICE table of wc_augment_job.  Workgroup (band, image): the band is
// `band` rows of the S x S crop window.
//   phase 1  the source rows [ys, ye) the band's vertical bounds cover are resampled horizontally, for the
//            S crop columns x 3 channels only, into LDS bytes laid out [row][channel][S] (the flip is
//            applied here, so phase 2 is the same for both directions).  Lanes run along the output
//            columns: a wave reads one contiguous span of one source row.
//   phase 2  the vertical pass out of LDS, four output columns per lane (one 32-bit LDS word per source
//            row), through the 256-entry fl(fl(u / 255) * 2 - 1) table in LDS, one 16-byte store per lane.
// Only the crop window is computed; the redundancy between bands is the 2 * support rows they share.
#include <math.h>

#include "../../include/wc_data.h"
#include "wc_common.hpp"

namespace {

constexpr int AUG_THREADS = 256;
constexpr int AUG_MAX_BAND = 16;           // output rows per workgroup, at most
constexpr int AUG_TABLE_BYTES = 256 * 4;   // the u8 -> fp32 table at the head of the LDS
constexpr int AUG_LDS_BYTES = 64 * 1024;   // a workgroup's LDS budget (table + rows)
constexpr int PRECISION_BITS = 22;         // Pillow's

typedef __attribute__((address_space(1))) const unsigned char gcu8;
typedef __attribute__((address_space(1))) const int gci32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

WC_DEVICE int clip8(int acc) {
    const int v = acc >> PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

__global__ __launch_bounds__(AUG_THREADS) void augment_kernel(const wc_augment_job* __restrict__ jobs, int S, int band,
                                                              int lds_rows, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* table = reinterpret_cast<float*>(smem);
    unsigned char* rows = smem + AUG_TABLE_BYTES;
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * band;
    if (r0 >= S) return;
    const int r1 = min(S, r0 + band);
    const wc_augment_job j = jobs[blockIdx.y];
    // ToTensor and the normalisation: a true division rounded once, an exact doubling, one subtraction
    table[tid] = __fsub_rn(__fmul_rn(__fdiv_rn((float)tid, 255.0f), 2.0f), 1.0f);

    gci32* vb = (gci32*)j.vbounds;
    gci32* vc = (gci32*)j.vcoefs;
    gci32* hb = (gci32*)j.hbounds;
    gci32* hc = (gci32*)j.hcoefs;
    const int crop_x = (int)j.crop_x, crop_y = (int)j.crop_y;
    const int ksh = (int)j.ksize_h, ksv = (int)j.ksize_v;
    // the bounds are monotone in the output index: the band reads source rows [ys, ye)
    const int ys = vb[2 * (crop_y + r0)];
    const int ye = vb[2 * (crop_y + r1 - 1)] + vb[2 * (crop_y + r1 - 1) + 1];
    const int nrows = ye - ys;
    if (nrows > lds_rows || nrows < 1) {
        // Tables that disagree with the bounds arithmetic the host sized lds_rows from (kernels.augment_geometry
        // refuses to make such tables): the band is written as NaN, never left as it was.
        const float nan = __builtin_nanf("");
        for (int it = tid; it < (r1 - r0) * 3 * S; it += AUG_THREADS) {
            const int col = it % S, rch = it / S;
            out[(((int64_t)blockIdx.y * 3 + rch % 3) * S + (r0 + rch / 3)) * S + col] = nan;
        }
        return;
    }
    const int rect_x = (int)j.rect_x, rect_y = (int)j.rect_y, rect_w = (int)j.rect_w, rect_h = (int)j.rect_h;
    const bool flip = j.flip != 0;
    gcu8* src = (gcu8*)j.src;

    // ---- phase 1: horizontal pass of the band's source rows into LDS bytes
    for (int it = tid; it < nrows * S; it += AUG_THREADS) {
        const int row = it / S, col = it - row * S;
        const int rc = crop_x + (flip ? S - 1 - col : col);
        const int xmin = hb[2 * rc], n = hb[2 * rc + 1];
        const int sy = ys + row - rect_y;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0;
        if (sy >= 0 && sy < rect_h) {
            gcu8* p = src + (int64_t)sy * j.pitch;
            gci32* k = hc + (int64_t)rc * ksh;
            const int x0 = xmin - rect_x;
            for (int x = 0; x < n; ++x) {
                const int sx = x0 + x;
                if (sx < 0 || sx >= rect_w) continue;  // never: the host checked the rectangle
                const int kk = k[x];
                a0 += (int)p[3 * sx] * kk;
                a1 += (int)p[3 * sx + 1] * kk;
                a2 += (int)p[3 * sx + 2] * kk;
            }
        }
        unsigned char* d = rows + (size_t)row * 3 * S + col;
        d[0] = (unsigned char)clip8(a0);
        d[S] = (unsigned char)clip8(a1);
        d[2 * S] = (unsigned char)clip8(a2);
    }
    __syncthreads();

    // ---- phase 2: vertical pass out of LDS, four columns per lane, 16-byte stores along W
    const int S4 = S >> 2;
    const int items = (r1 - r0) * 3 * S4;
    const uint32_t* rows32 = reinterpret_cast<const uint32_t*>(rows);
    for (int it = tid; it < items; it += AUG_THREADS) {
        const int q = it % S4;
        const int rch = it / S4;
        const int ch = rch % 3, r = rch / 3;
        const int orow = crop_y + r0 + r;
        const int ymin = vb[2 * orow], n = vb[2 * orow + 1];
        gci32* k = vc + (int64_t)orow * ksv;
        int a0 = 1 << (PRECISION_BITS - 1), a1 = a0, a2 = a0, a3 = a0;
        const uint32_t* w = rows32 + ((size_t)(ymin - ys) * 3 + ch) * S4 + q;
        for (int y = 0; y < n; ++y) {
            const uint32_t v = w[(size_t)y * 3 * S4];
            const int kk = k[y];
            a0 += (int)(v & 255u) * kk;
            a1 += (int)((v >> 8) & 255u) * kk;
            a2 += (int)((v >> 16) & 255u) * kk;
            a3 += (int)(v >> 24) * kk;
        }
        f32x4 o;
        o[0] = table[clip8(a0)];
        o[1] = table[clip8(a1)];
        o[2] = table[clip8(a2)];
        o[3] = table[clip8(a3)];
        gf32x4* dst = (gf32x4*)(out + (((int64_t)blockIdx.y * 3 + ch) * S + (r0 + r)) * S) + q;
        *dst = o;
    }
}

// (xmin, xmax) of output index xx of the axis inS -> outS: the float64 arithmetic of wc_data.h with every
// rounding as written (no contraction), the same the host tables are made with.
void axis_bounds(int64_t inS, int64_t outS, int64_t xx, int64_t* xmin, int64_t* xmax) {
#pragma clang fp contract(off)
    const double scale = (double)inS / (double)outS;
    const double support = scale > 1.0 ? scale : 1.0;
    const double center = ((double)xx + 0.5) * scale;
    int64_t lo = (int64_t)(center - support + 0.5);
    int64_t hi = (int64_t)(center + support + 0.5);
    *xmin = lo < 0 ? 0 : lo;
    *xmax = hi > inS ? inS : hi;
}

int axis_ksize(int64_t inS, int64_t outS) {
    const double scale = (double)inS / (double)outS;
    return (int)ceil(scale > 1.0 ? scale : 1.0) * 2 + 1;
}

}  // namespace

extern "C" int wc_resample_span(int64_t inS, int64_t outS, int64_t o0, int64_t o1, int64_t* first, int64_t* count) {
    if (!first || !count) return WC_E_ARG;
    if (inS < 1 || outS < 1 || o0 < 0 || o1 <= o0 || o1 > outS) return WC_E_SHAPE;
    int64_t lo, hi, unused;
    axis_bounds(inS, outS, o0, &lo, &unused);
    axis_bounds(inS, outS, o1 - 1, &unused, &hi);
    *first = lo;
    *count = hi - lo;
    return WC_OK;
}

extern "C" int wc_augment_batch(const wc_augment_job* jobs, const wc_augment_job* jobs_dev, int njobs, int S, float* out,
                                void* stream) {
    if (!jobs || !jobs_dev || !out || njobs < 1) return WC_E_ARG;
    if (reinterpret_cast<uintptr_t>(out) & 15) return WC_E_ARG;
    if (S < 4 || S % 4 != 0 || njobs > 65535) return WC_E_SHAPE;
    for (int i = 0; i < njobs; ++i) {
        const wc_augment_job& j = jobs[i];
        if (!j.src || !j.hbounds || !j.hcoefs || !j.vbounds || !j.vcoefs) return WC_E_ARG;
        if (j.ksize_h < 3 || j.ksize_h % 2 == 0 || j.ksize_v < 3 || j.ksize_v % 2 == 0) return WC_E_SHAPE;
        if (j.img_w < 1 || j.img_h < 1 || j.out_w < S || j.out_h < S) return WC_E_SHAPE;
        if (j.img_w > (1 << 24) || j.img_h > (1 << 24) || j.out_w > (1 << 24) || j.out_h > (1 << 24)) return WC_E_SHAPE;
        if (j.ksize_h != axis_ksize(j.img_w, j.out_w) || j.ksize_v != axis_ksize(j.img_h, j.out_h)) return WC_E_SHAPE;
        if (j.crop_x < 0 || j.crop_y < 0 || j.crop_x > j.out_w - S || j.crop_y > j.out_h - S) return WC_E_SHAPE;
        if (j.flip != 0 && j.flip != 1) return WC_E_SHAPE;
        if (j.rect_w < 1 || j.rect_h < 1 || j.rect_x < 0 || j.rect_y < 0 || j.rect_x > j.img_w - j.rect_w ||
            j.rect_y > j.img_h - j.rect_h || j.pitch < 3 * j.rect_w)
            return WC_E_SHAPE;
        int64_t x0, nx, y0, ny;
        wc_resample_span(j.img_w, j.out_w, j.crop_x, j.crop_x + S, &x0, &nx);
        wc_resample_span(j.img_h, j.out_h, j.crop_y, j.crop_y + S, &y0, &ny);
        if (x0 < j.rect_x || x0 + nx > j.rect_x + j.rect_w || y0 < j.rect_y || y0 + ny > j.rect_y + j.rect_h)
            return WC_E_SHAPE;
    }
    // The band height: the largest (at most AUG_MAX_BAND) whose source rows fit the LDS for every job.
    const int64_t max_rows = (AUG_LDS_BYTES - AUG_TABLE_BYTES) / (3 * (int64_t)S);
    int band = S < AUG_MAX_BAND ? S : AUG_MAX_BAND;
    int64_t lds_rows = 0;
    for (; band >= 1; --band) {
        lds_rows = 0;
        for (int i = 0; i < njobs; ++i) {
            const wc_augment_job& j = jobs[i];
            for (int64_t r0 = 0; r0 < S; r0 += band) {
                const int64_t r1 = r0 + band < S ? r0 + band : S;
                int64_t y0, ny;
                wc_resample_span(j.img_h, j.out_h, j.crop_y + r0, j.crop_y + r1, &y0, &ny);
                if (ny > lds_rows) lds_rows = ny;
            }
        }
        if (lds_rows <= max_rows) break;
    }
    if (band < 1) return WC_E_SHAPE;  // one output row's source rows do not fit
    const size_t lds = (size_t)AUG_TABLE_BYTES + (size_t)lds_rows * 3 * S;
    hipLaunchKernelGGL(augment_kernel, dim3((unsigned)((S + band - 1) / band), (unsigned)njobs), dim3(AUG_THREADS), lds,
                       reinterpret_cast<hipStream_t>(stream), jobs_dev, S, band, (int)lds_rows, out);
    WC_CHECK_LAUNCH();
    return WC_OK;
}
