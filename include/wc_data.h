/*
 * wc_data.h — C ABI of the training-input kernel of libwc_kernels.so (the conventions of wc_sampler.h:
 * caller-owned device memory, asynchronous on the given stream, WC_OK / WC_E_* / hipError_t returns).
 *
 * The reference's loader transform (diffusion_model/train_ddpm.py:150-159, translation.py:136-143):
 *   Resize(S, BILINEAR) -> RandomCrop(S) | CenterCrop(S) -> RandomHorizontalFlip -> ToTensor -> x*2-1
 * on a PIL image, i.e. Pillow's antialiased two-pass resample in 8-bit fixed point, reproduced bit for
 * bit for the S x S crop window only, in ONE launch per batch.
 *
 * One axis inS -> outS (float64 on the host): scale = inS/outS, fs = max(scale, 1), support = fs,
 * ksize = 2*ceil(support) + 1; for output index xx: center = (xx + 0.5) scale,
 * xmin = max(int(center - support + 0.5), 0), xmax = min(int(center + support + 0.5), inS), n = xmax - xmin,
 * w[x] = max(0, 1 - |(x + xmin - center + 0.5) * (1/fs)|), divided by their in-order sum,
 * k[x] = int(0.5 + w[x] * 2^22).  A pass is byte = clamp((2^21 + sum_x pixel[xmin + x] k[x]) >> 22, 0, 255)
 * in int32; the horizontal pass runs first, the vertical pass on its BYTES.  Then
 * out = fl(fl(u / 255) * 2 - 1) in fp32.
 */
#ifndef WC_DATA_H
#define WC_DATA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One image of a launch, 8-byte words only (rows are written as int64 words).
 *   src              DEVICE pointer to the uploaded source rectangle: interleaved RGB bytes, `pitch` bytes
 *                    from one row to the next (pitch >= 3 rect_w); only read
 *   rect_x .. rect_h the rectangle's origin in the full image and its size, in pixels
 *   img_w, img_h     the full image; out_w, out_h the resized image (the lengths of the tables)
 *   hbounds, vbounds DEVICE int32 [out][2] = (xmin, n) of the horizontal / vertical axis
 *   hcoefs, vcoefs   DEVICE int32 [out][ksize] = k, zero beyond n
 *   ksize_h, ksize_v the row lengths of the coefficient tables: 2*ceil(max(in/out, 1)) + 1
 *   crop_x, crop_y   origin of the S x S window in the resized image
 *   flip             0 / 1: output column j is resized column crop_x + (flip ? S - 1 - j : j) */
typedef struct wc_augment_job {
    const void* src;
    int64_t pitch, rect_x, rect_y, rect_w, rect_h;
    int64_t img_w, img_h, out_w, out_h;
    const int* hbounds;
    const int* hcoefs;
    const int* vbounds;
    const int* vcoefs;
    int64_t ksize_h, ksize_v, crop_x, crop_y, flip;
} wc_augment_job;

/* out[njobs][3][S][S] fp32 (NCHW, 16-byte aligned) = the transform above of every job, one launch.
 * `jobs` is the HOST copy of the table: it is checked here and sizes the launch; `jobs_dev` is the same
 * njobs rows in DEVICE memory, which the kernel reads (the caller uploads them with the batch).
 * A workgroup owns one image and a band of output rows: it resamples horizontally, for the S crop
 * columns x 3 channels, exactly the source rows the band's vertical bounds cover, into LDS bytes, and
 * runs the vertical pass out of LDS.  The band height (at most 16 rows, one value per launch) is the
 * largest whose rows fit the LDS budget for every job; only the rectangle's bytes the window needs are
 * read, nothing is written outside out.  The launch is sized from the bounds arithmetic above, so the tables
 * must be that arithmetic's: a band whose table bounds ask for more rows than that is written as NaN.
 * Checked before any launch -- WC_E_ARG: null jobs / jobs_dev / out, njobs < 1, out not 16-byte aligned, a
 * job with a null pointer; WC_E_SHAPE: S < 4 or S % 4 != 0, njobs > 65535 (the grid's y extent), an image or
 * resized edge above 2^24, a ksize < 3, even, or not the geometry's, an
 * image / resized size < 1, out_w or out_h < S, a crop window outside the resized image, flip not 0 / 1,
 * a rectangle outside the image or not covering what the window's bounds read, pitch < 3 rect_w, or a
 * geometry whose single output row needs more LDS than a workgroup has (there is no CPU path). */
int wc_augment_batch(const wc_augment_job* jobs, const wc_augment_job* jobs_dev, int njobs, int S, float* out,
                     void* stream);
/* The source span [first, first + count) one axis inS -> outS reads for output indices [o0, o1): the
 * bounds arithmetic above, as the launch check evaluates it (first = xmin(o0), count = xmax(o1-1) - first).
 * WC_E_SHAPE for inS < 1, outS < 1 or an empty / outside index range; first / count must not be null. */
int wc_resample_span(int64_t inS, int64_t outS, int64_t o0, int64_t o1, int64_t* first, int64_t* count);

#ifdef __cplusplus
}
#endif

#endif /* WC_DATA_H */
