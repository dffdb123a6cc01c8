/*
 * wc_seg.h — C ABI of the segmentation label and metric kernels of libwc_kernels.so (the conventions of
 * wc_sampler.h / wc_data.h: caller-owned device memory, asynchronous on the given stream, WC_OK / WC_E_* /
 * hipError_t returns; every argument check runs before any launch).
 *
 * The label side of the reference's segmenter input (seg_model/inference.py:56-115):
 *   ExtResize(size, NEAREST) -> ExtCenterCrop -> ACDCDataset.encode_target
 * and its scoring (seg_model/metrics/stream_metrics.py: StreamSegMetrics._fast_hist over argmax(1)), plus
 * ACDCDataset.decode_target.
 *
 * Pillow's NEAREST resize of one axis in -> out is a scale-only affine map accumulated in double:
 *   a = in / out;  xo = a * 0.5;  for each output index in order: idx = (int)xo; xo += a;
 * The host makes these index tables for the crop window only (kernels.nearest_table), relative to the
 * source rectangle it uploads.
 */
#ifndef WC_SEG_H
#define WC_SEG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One label map of a launch, 8-byte words only.
 *   src                  DEVICE pointer to the uploaded source rectangle: one uint8 id per pixel, `pitch`
 *                        bytes from one row to the next (pitch >= rect_w); only read
 *   rect_w, rect_h       the rectangle's size in pixels
 *   rows, cols           DEVICE int32 [Hc] / [Wc]: the rectangle row / column of every output row / column
 *   rows_host, cols_host the same tables in HOST memory: what the entry point checks (every entry inside
 *                        the rectangle); the kernel never reads them */
typedef struct wc_label_job {
    const void* src;
    int64_t pitch, rect_w, rect_h;
    const int* rows;
    const int* cols;
    const int* rows_host;
    const int* cols_host;
} wc_label_job;

/* out[b][y][x] = lut[src_b[rows_b[y]][cols_b[x]]] as int64 [njobs][Hc][Wc] (contiguous), one launch.
 * `jobs` is the HOST copy of the table: it is checked here; `jobs_dev` is the same njobs rows in DEVICE
 * memory, which the kernel reads.  `lut` is 256 bytes of HOST memory, copied into the kernel arguments.
 * A device table entry outside the rectangle (the device tables then differ from the checked host ones)
 * reads nothing and writes 255, the ignore label.  Nothing outside out is written.
 * Checked before any launch -- WC_E_SHAPE: a null jobs / jobs_dev / lut / out or a job with a null pointer,
 * Hc < 1 or Wc < 1 (an empty window), njobs outside 1..65535, rect_w < 1, rect_h < 1, pitch < rect_w, a
 * host table entry outside [0, rect_h) / [0, rect_w). */
int wc_label_batch(const wc_label_job* jobs, const wc_label_job* jobs_dev, int njobs, int Hc, int Wc,
                   const void* lut, int64_t* out, void* stream);

/* The streaming confusion matrix of a segmenter's logits, argmax fused: for every pixel with
 * 0 <= labels[b][y][x] < C (255 and every other value is ignored)
 *     hist[label][pred] += 1,   pred = the FIRST index of the maximum over the C planes of that pixel,
 * numpy.argmax's result: a later class wins only when strictly greater (ties and -0.0 / +0.0 go to the
 * lower class), a NaN counts as larger than every number and the first NaN wins.
 *   logits  fp32 [B][C][H][W], contiguous, 16-byte aligned, read once
 *   labels  int64 [B][H][W]
 *   hist    int64 [C][C], ADDED TO with 64-bit integer atomics (exact, independent of order): a metric
 *           streams over batches without a host synchronisation; the caller zeroes it once
 *   pred    uint8 [B][H][W] or null: the argmax map, written for every pixel (ignored ones included)
 * One bounded grid with a grid-stride loop; a workgroup counts into C*C 32-bit LDS counters and adds only
 * its non-zero cells to hist at the end.  Four consecutive pixels per lane with 16-byte loads when
 * H*W % 4 == 0 and labels / pred are 16- / 4-byte aligned, one pixel per lane otherwise.
 * Checked before any launch -- WC_E_ARG: null logits / labels / hist, logits not 16-byte aligned, labels or
 * hist not 8-byte aligned; WC_E_SHAPE: B < 1, C outside 2..32, H < 1, W < 1, B*H*W above 2^40. */
int wc_seg_confusion(const float* logits, const int64_t* labels, int B, int C, int H, int W, int64_t* hist,
                     void* pred, void* stream);
/* The same matrix from a ready uint8 prediction map preds[B][H][W] (only read).  A pixel counts when
 * 0 <= label < C AND pred < C: on the device a prediction >= C is ignored like a bad label (the host
 * wrapper rejects one only where the data is on the host).  Checks as above (WC_E_ARG for null preds). */
int wc_seg_confusion_pred(const void* preds, const int64_t* labels, int B, int C, int H, int W,
                          int64_t* hist, void* stream);

/* out[i] = palette[min(map[i], C)] for i < n: a class map to colours, uint8 [n][3] interleaved RGB.
 *   map      uint8 [n] (is_int64 = 0) or int64 [n] (is_int64 = 1, 8-byte aligned); only read, never
 *            changed (the reference's decode_target rewrites 255 in its argument)
 *   palette  (C + 1) x 3 bytes of HOST memory, copied into the kernel arguments; every value >= C or
 *            negative (255 included) takes the last colour
 * Checked before any launch -- WC_E_ARG: null map / palette / out, is_int64 not 0 / 1, a misaligned int64
 * map; WC_E_SHAPE: n < 1 or above 2^40, C outside 2..32. */
int wc_seg_decode(const void* map, int is_int64, int64_t n, int C, const void* palette, void* out,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WC_SEG_H */
