// Host-side AddressSanitizer check of the C ABI (include/wc_kernels.h).
//
// Built by tools/asan/run.sh with `-Xarch_host -fsanitize=address`, so only the host code of every
// entry point is instrumented (GPU ASan is not available on this pool).  It needs no GPU: every call
// below is rejected by the argument / shape validation before any launch, or is a host-only sizing
// helper.  What it proves: the validation code reads nothing outside the caller's structs, and each
// rejection returns the documented WC_E_* code (the Python layer turns these into RuntimeError).
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wc_data.h"
#include "wc_kernels.h"
#include "wc_optim.h"
#include "wc_sampler.h"
#include "wc_seg.h"

#include "conv_args_mutations.hpp"

// The library build generates this symbol (the digest of its sources, _build.py); the harness links the
// objects directly, so it supplies its own for wc_version to refer to.
extern "C" const char* wc_source_hash(void) { return "asan-harness"; }

static int failures = 0;

#define EXPECT(expr, want)                                                                       \
    do {                                                                                         \
        const int got_ = (expr);                                                                 \
        if (got_ != (want)) {                                                                    \
            std::printf("FAIL %s:%d %s -> %d (want %d)\n", __FILE__, __LINE__, #expr, got_, want); \
            ++failures;                                                                          \
        }                                                                                        \
    } while (0)

int main() {
    // Host buffers stand in for device pointers: none of them is dereferenced by the host code.
    std::vector<float> buf(1 << 12, 0.f);
    float* p = buf.data();
    wc_conv_args a;
    std::memset(&a, 0, sizeof(a));

    // Convolution entry points: null struct / weights / output, bad segment count, bad channels.
    EXPECT(wc_conv_igemm(nullptr, nullptr), WC_E_ARG);
    EXPECT(wc_conv_igemm(&a, nullptr), WC_E_ARG);
    a.w = p;
    a.out = p;
    a.nseg = 3;
    EXPECT(wc_conv_igemm(&a, nullptr), WC_E_ARG);
    a.nseg = 1;
    EXPECT(wc_conv_igemm(&a, nullptr), WC_E_ARG);  // seg[0].src == NULL
    a.seg[0].src = p;
    a.seg[0].C = 30;  // not a multiple of the K tile
    a.seg[0].ldc = 32;
    EXPECT(wc_conv_igemm(&a, nullptr), WC_E_SHAPE);
    EXPECT(wc_conv3x3_x6(nullptr, p, 0, nullptr), WC_E_ARG);
    EXPECT(wc_conv3x3_f16x3(nullptr, p, 0, 0, p, nullptr, nullptr), WC_E_ARG);
    a.seg[0].scale = p;  // scale without shift
    EXPECT(wc_conv3x3_f16x3(&a, p, 0, 0, p, nullptr, nullptr), WC_E_ARG);
    a.seg[0].scale = nullptr;
    EXPECT(wc_conv_igemm_x6(nullptr, p, 0, nullptr), WC_E_ARG);
    // Winograd conv: null struct, a raw segment without its per-image bound, a raw segment that is
    // not a 3x3 grid; tile width; the device pack's null / channel / size checks.
    EXPECT(wc_conv3x3_wino_f16x3(nullptr, p, 0, 0, p, p, nullptr), WC_E_ARG);
    EXPECT(wc_conv3x3_wino_f16x3(&a, p, 0, 0, p, nullptr, nullptr), WC_E_ARG);
    EXPECT(wc_conv3x3_wino_f16x3(&a, p, 0, 0, p, p, nullptr), WC_E_SHAPE);  // ntaps 0, C = 30
    EXPECT(wc_conv3x3_wino_tile_n(64), 64);
    EXPECT(wc_conv3x3_wino_tile_n(65), 128);
    EXPECT(wc_pack_wino(nullptr, 128, 32, 0, p, 0, p, nullptr), WC_E_ARG);
    EXPECT(wc_pack_wino(p, 128, 30, 0, p, 0, p, nullptr), WC_E_SHAPE);
    EXPECT(wc_pack_wino(p, 128, 32, 0, p, 12, p, nullptr), WC_E_SHAPE);  // wrong output size

    // Attention: null operands, heads not dividing C, unsupported head width, misaligned strides.
    EXPECT(wc_attention_fwd(nullptr, 96, p, 32, 1, 64, 32, 4, 1.f, nullptr), WC_E_ARG);
    EXPECT(wc_attention_fwd(p, 96, p, 32, 1, 64, 30, 4, 1.f, nullptr), WC_E_SHAPE);
    EXPECT(wc_attention_fwd(p, 96, p, 32, 1, 64, 36, 9, 1.f, nullptr), WC_E_SHAPE);  // D = 4
    EXPECT(wc_attention_fwd(p, 90, p, 32, 1, 64, 32, 4, 1.f, nullptr), WC_E_SHAPE);
    EXPECT(wc_attention_fwd_lse(p, 96, p, 32, nullptr, 1, 64, 32, 4, 1.f, nullptr), WC_E_ARG);
    EXPECT(wc_attention_fwd_f16x3(nullptr, 96, p, 32, 1, 64, 32, 4, 1.f, 0, 0, 0, nullptr), WC_E_ARG);

    // Sampler / training element-wise entry points.
    EXPECT(wc_ddpm_step(nullptr, p, p, p, nullptr, 1, 16, 0.f, 0.f, 1.f, 0.f, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddpm_step(p, p, p, p, nullptr, 1, 15, 0.f, 0.f, 1.f, 0.f, 0, 0, 0, 0, nullptr), WC_E_SHAPE);
    EXPECT(wc_ddpm_step(p, p, p, p, nullptr, 1, 16, 0.f, 0.f, 1.f, 0.f, 7, 0, 0, 0, nullptr), WC_E_ARG);
    // Strided sampling step (wc_sampler.h): null operands, noise mode, shape, scalar ranges, NaN scalars,
    // clipping where sqrt(1 - acp_t) is 0.
    const float qnan = std::nanf("");
    EXPECT(wc_ddim_step(nullptr, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, nullptr, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, nullptr, p, p, 1, 16, .8f, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, .1f, 0, 3, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, .1f, 0, -1, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, nullptr, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, .1f, 0, WC_NOISE_TENSOR, 0, 0, 0,
                        nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 15, .8f, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_SHAPE);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 0, 16, .8f, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_SHAPE);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, 0.f, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, -.6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, -.4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, -.1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, qnan, .6f, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, qnan, .9f, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, qnan, .4f, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, qnan, .1f, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, .8f, .6f, .9f, .4f, qnan, 0, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_ddim_step(p, p, p, p, nullptr, nullptr, 1, 16, 1.f, 0.f, .9f, .4f, .1f, 1, 0, 0, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_mse_loss(nullptr, p, 16, nullptr, 1.f, nullptr, p, nullptr), WC_E_ARG);
    std::vector<double> ws(wc_mse_workspace_doubles());
    EXPECT(wc_mse_loss(p, p, 0, nullptr, 1.f, ws.data(), p, nullptr), WC_E_SHAPE);
    EXPECT(wc_mse_loss(p + 1, p, 16, nullptr, 1.f, ws.data(), p, nullptr), WC_E_SHAPE);  // misaligned

    // Optimizer entry points (wc_optim.h): the job table, the clip outputs and the workspace are device
    // memory the host never reads; null table / outputs / workspace, empty table, no chunks.
    wc_adam_job jobs[2];
    std::memset(jobs, 0, sizeof(jobs));
    EXPECT(wc_adam_step(nullptr, 2, 2, nullptr, 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-3, 0.0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_adam_step(jobs, 0, 2, nullptr, 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-3, 0.0, 0, nullptr), WC_E_SHAPE);
    EXPECT(wc_adam_step(jobs, -1, 2, p, 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-3, 0.0, 0, nullptr), WC_E_SHAPE);
    EXPECT(wc_adam_step(jobs, 2, 0, p, 1e-3, 1.0, 0.9, 0.999, 1e-8, 1e-3, 0.01, 1, nullptr), WC_E_SHAPE);
    EXPECT(wc_grad_norm(nullptr, 2, 2, 1.0, ws.data(), p, p + 1, nullptr), WC_E_ARG);
    EXPECT(wc_grad_norm(jobs, 2, 2, 1.0, nullptr, p, p + 1, nullptr), WC_E_ARG);
    EXPECT(wc_grad_norm(jobs, 2, 2, 1.0, ws.data(), nullptr, p + 1, nullptr), WC_E_ARG);
    EXPECT(wc_grad_norm(jobs, 2, 2, 1.0, ws.data(), p, nullptr, nullptr), WC_E_ARG);
    EXPECT(wc_grad_norm(jobs, 0, 2, 1.0, ws.data(), p, p + 1, nullptr), WC_E_SHAPE);
    EXPECT(wc_grad_norm(jobs, 2, -3, 1.0, ws.data(), p, p + 1, nullptr), WC_E_SHAPE);
    if (wc_optim_chunk_elems() <= 0 || wc_optim_chunk_elems() % 4 != 0 || sizeof(wc_adam_job) % 8 != 0) {
        std::printf("FAIL wc_optim_chunk_elems / wc_adam_job size\n");
        ++failures;
    }

    // Training-input kernel (wc_data.h): the host copy of the job table is read, its pointers never are.
    // A 40 x 30 image to S = 64 (resized 85 x 64, ksize 3 on both axes), the whole image uploaded.
    {
        wc_augment_job good;
        std::memset(&good, 0, sizeof(good));
        good.src = good.hbounds = good.hcoefs = good.vbounds = good.vcoefs = reinterpret_cast<const int*>(p);
        good.pitch = 120;
        good.rect_w = good.img_w = 40;
        good.rect_h = good.img_h = 30;
        good.out_w = 85;
        good.out_h = 64;
        good.ksize_h = good.ksize_v = 3;
        good.crop_x = 10;
        float* out16 = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15));
        EXPECT(wc_augment_batch(nullptr, &good, 1, 64, out16, nullptr), WC_E_ARG);
        EXPECT(wc_augment_batch(&good, nullptr, 1, 64, out16, nullptr), WC_E_ARG);
        EXPECT(wc_augment_batch(&good, &good, 1, 64, nullptr, nullptr), WC_E_ARG);
        EXPECT(wc_augment_batch(&good, &good, 0, 64, out16, nullptr), WC_E_ARG);
        EXPECT(wc_augment_batch(&good, &good, 1, 64, out16 + 1, nullptr), WC_E_ARG);  // misaligned out
        EXPECT(wc_augment_batch(&good, &good, 1, 2, out16, nullptr), WC_E_SHAPE);
        EXPECT(wc_augment_batch(&good, &good, 1, 62, out16, nullptr), WC_E_SHAPE);
        wc_augment_job j = good;
        j.src = nullptr;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_ARG);
        j = good;
        j.vcoefs = nullptr;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_ARG);
        j = good;
        j.ksize_h = 1;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        j.ksize_h = 4;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        j.ksize_h = 5;  // odd, but not this geometry's
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        j = good;
        j.crop_x = 22;  // 85 - 64 = 21 is the last origin
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        j = good;
        j.rect_x = 5;  // the window at crop_x = 10 reads source columns [4, 36)
        j.rect_w = 31;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        j = good;
        j.pitch = 119;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        j = good;
        j.flip = 2;
        EXPECT(wc_augment_batch(&j, &good, 1, 64, out16, nullptr), WC_E_SHAPE);
        wc_augment_job two[2] = {good, good};
        two[1].out_h = 63;
        EXPECT(wc_augment_batch(two, &good, 2, 64, out16, nullptr), WC_E_SHAPE);
        // one output row that does not fit a workgroup's LDS: refused, there is no CPU path
        j = good;
        j.img_w = j.img_h = j.out_w = j.out_h = j.rect_w = j.rect_h = 16000;
        j.pitch = 48000;
        j.crop_x = 0;
        EXPECT(wc_augment_batch(&j, &good, 1, 16000, out16, nullptr), WC_E_SHAPE);
        int64_t first = -1, count = -1;
        EXPECT(wc_resample_span(40, 85, 10, 74, &first, &count), WC_OK);
        if (first != 4 || count != 32) {
            std::printf("FAIL wc_resample_span -> [%lld, +%lld)\n", (long long)first, (long long)count);
            ++failures;
        }
        EXPECT(wc_resample_span(40, 85, 10, 10, &first, &count), WC_E_SHAPE);
        EXPECT(wc_resample_span(40, 85, 0, 86, &first, &count), WC_E_SHAPE);
        EXPECT(wc_resample_span(40, 85, 0, 85, nullptr, &count), WC_E_ARG);
    }

    // Segmentation labels and metrics (include/wc_seg.h): every check runs before any launch.
    {
        alignas(16) static unsigned char lut[256];
        std::vector<int> rows(6), cols(5);
        for (int i = 0; i < 6; ++i) rows[i] = i;
        for (int i = 0; i < 5; ++i) cols[i] = i;
        wc_label_job good;
        std::memset(&good, 0, sizeof(good));
        good.src = p;
        good.pitch = 5;
        good.rect_w = 5;
        good.rect_h = 6;
        good.rows = good.cols = (const int*)p;  // device tables: never read on the host
        good.rows_host = rows.data();
        good.cols_host = cols.data();
        float* a16 = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(p) + 15) & ~uintptr_t(15));
        int64_t* out64 = (int64_t*)a16;
        EXPECT(wc_label_batch(nullptr, &good, 1, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, nullptr, 1, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, &good, 1, 6, 5, nullptr, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, &good, 1, 6, 5, lut, nullptr, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, &good, 0, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, &good, 65536, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, &good, 1, 0, 5, lut, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_label_batch(&good, &good, 1, 6, 0, lut, out64, nullptr), WC_E_SHAPE);
        wc_label_job j = good;
        j.pitch = 4;
        EXPECT(wc_label_batch(&j, &good, 1, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        j = good;
        j.rows_host = nullptr;
        EXPECT(wc_label_batch(&j, &good, 1, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        rows[5] = 6;  // the last row entry outside the rectangle: the whole table is walked, and no further
        EXPECT(wc_label_batch(&good, &good, 1, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        rows[5] = 5;
        cols[4] = -1;
        EXPECT(wc_label_batch(&good, &good, 1, 6, 5, lut, out64, nullptr), WC_E_SHAPE);
        cols[4] = 4;
        wc_label_job two[2] = {good, good};
        two[1].rect_h = 5;  // row entry 5 is outside the second job's rectangle
        EXPECT(wc_label_batch(two, two, 2, 6, 5, lut, out64, nullptr), WC_E_SHAPE);

        const float* lg = a16;
        const int64_t* lb = (const int64_t*)a16;
        EXPECT(wc_seg_confusion(nullptr, lb, 1, 19, 8, 8, out64, nullptr, nullptr), WC_E_ARG);
        EXPECT(wc_seg_confusion(lg, nullptr, 1, 19, 8, 8, out64, nullptr, nullptr), WC_E_ARG);
        EXPECT(wc_seg_confusion(lg, lb, 1, 19, 8, 8, nullptr, nullptr, nullptr), WC_E_ARG);
        EXPECT(wc_seg_confusion(lg + 1, lb, 1, 19, 8, 8, out64, nullptr, nullptr), WC_E_ARG);  // misaligned logits
        EXPECT(wc_seg_confusion(lg, lb, 1, 1, 8, 8, out64, nullptr, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_confusion(lg, lb, 1, 33, 8, 8, out64, nullptr, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_confusion(lg, lb, 0, 19, 8, 8, out64, nullptr, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_confusion(lg, lb, 1, 19, 0, 8, out64, nullptr, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_confusion(lg, lb, 1 << 20, 19, 1 << 11, 1 << 11, out64, nullptr, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_confusion_pred(nullptr, lb, 1, 19, 8, 8, out64, nullptr), WC_E_ARG);
        EXPECT(wc_seg_confusion_pred(p, lb, 1, 33, 8, 8, out64, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_confusion_pred(p, lb, 1, 19, 8, 0, out64, nullptr), WC_E_SHAPE);
        unsigned char palette[20 * 3] = {0};
        EXPECT(wc_seg_decode(nullptr, 0, 64, 19, palette, p, nullptr), WC_E_ARG);
        EXPECT(wc_seg_decode(p, 0, 64, 19, nullptr, p, nullptr), WC_E_ARG);
        EXPECT(wc_seg_decode(p, 0, 64, 19, palette, nullptr, nullptr), WC_E_ARG);
        EXPECT(wc_seg_decode(p, 2, 64, 19, palette, p, nullptr), WC_E_ARG);
        EXPECT(wc_seg_decode((const char*)a16 + 4, 1, 64, 19, palette, p, nullptr), WC_E_ARG);
        EXPECT(wc_seg_decode(p, 0, 0, 19, palette, p, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_decode(p, 0, 64, 1, palette, p, nullptr), WC_E_SHAPE);
        EXPECT(wc_seg_decode(p, 0, 64, 33, palette, p, nullptr), WC_E_SHAPE);
    }

    // Round-3 training entry points: weight gradients, split-precision attention backward, bounds.
    wc_wgrad_args wg;
    std::memset(&wg, 0, sizeof(wg));
    EXPECT(wc_conv_wgrad3(nullptr, p, 1, nullptr), WC_E_ARG);
    EXPECT(wc_conv_wgrad3_f16x3(&wg, p, 1, 0, p, nullptr), WC_E_ARG);  // g == NULL
    wg.g = p;
    wg.nseg = 1;
    wg.seg[0].src = p;
    EXPECT(wc_conv_wgrad3_f16x3(&wg, p, 1, 0, nullptr, nullptr), WC_E_ARG);  // no gradient bound
    EXPECT(wc_conv_wgrad3_f16x3(&wg, p, 1, 99, p, nullptr), WC_E_ARG);       // exponent out of range
    EXPECT(wc_conv_wgrad3(&wg, p, 1, nullptr), WC_E_SHAPE);                   // not a 3x3 tap grid
    EXPECT(wc_conv_wgrad_f16x3(nullptr, p, 1, p, 0, nullptr, nullptr, nullptr), WC_E_ARG);
    EXPECT(wc_conv_wgrad_f16x3(&wg, p, 1, nullptr, 0, nullptr, nullptr, nullptr), WC_E_ARG);  // no G bound
    wg.nseg = 2;
    wg.seg[1].src = p;
    EXPECT(wc_conv_wgrad_f16x3(&wg, p, 1, p, 0, nullptr, nullptr, nullptr), WC_E_ARG);  // segment 1 unbounded
    EXPECT(wc_wgrad_reduce(nullptr, 1, 4, 4, 4, 4, 4, p, 0, 0, 0, nullptr, 0, 0, nullptr), WC_E_ARG);
    EXPECT(wc_wgrad_reduce(p, 1, 4, 8, 4, 4, 4, p, 0, 0, 0, nullptr, 0, 0, nullptr), WC_E_ARG);  // dw1 missing
    EXPECT(wc_attention_bwd_f16x3(p, 96, p, 32, p, 32, p, p, p, 96, 1, 64, 32, 4, 1.f, 0, 0, 0, nullptr, p, nullptr,
                                  nullptr), WC_E_ARG);  // no dO bound (the row-norm workspace does not replace it)
    EXPECT(wc_attention_bwd_f16x3(p, 96, p, 32, p, 32, p, p, p, 96, 1, 64, 32, 4, 1.f, 99, 0, 0, p, nullptr, nullptr,
                                  nullptr), WC_E_ARG);  // exponent out of range
    EXPECT(wc_attention_bwd_f16x3(p, 96, p, 32, p, 32, p, p, p, 96, 1, 64, 30, 4, 1.f, 0, 0, 0, p, p, nullptr,
                                  nullptr), WC_E_SHAPE);  // heads do not divide C
    EXPECT(wc_attention_bwd_dkdv192(p, 96, p, 32, p, p, p, 96, 1, 64, 32, 4, 1.f, nullptr), WC_E_SHAPE);  // D != 192
    EXPECT(wc_attention_bwd6(nullptr, 96, p, 32, p, 32, p, p, p, 96, 1, 64, 32, 4, 1.f, nullptr), WC_E_ARG);
    EXPECT(wc_gn_bwd_apply(nullptr, 4, p, 4, p, p, nullptr, nullptr, 1, p, 1, 16, 4, p, 4, 0, p, nullptr), WC_E_ARG);
    EXPECT(wc_gn_bwd_apply(p, 3, p, 4, p, p, nullptr, nullptr, 1, p, 1, 16, 4, p, 4, 0, p, nullptr), WC_E_SHAPE);
    EXPECT(wc_absmax_images(nullptr, 4, 1, 16, 4, p, nullptr), WC_E_ARG);
    EXPECT(wc_pack_split(p, 144, 4, 16, 9, 0, 0, 0, 0, 100, p, 0, p, nullptr), WC_E_ARG);  // BN not 64 / 128

    // Kernel-form selectors: out-of-range modes rejected, valid ones return the previous setting.
    EXPECT(wc_proj_set_tile(64), WC_E_ARG);
    EXPECT(wc_proj_set_tile(-128), WC_E_ARG);
    if (wc_proj_set_tile(256) != 0 || wc_proj_set_tile(128) != 256 || wc_proj_set_tile(0) != 128) {
        std::printf("FAIL kernel-form selectors\n");
        ++failures;
    }
    // the 256-row projection launcher checks run before any launch (null / misaligned A operand)
    EXPECT(wc_proj_f16x3_qkv(&a, nullptr, 0, p, 0, 0, p, p, 128, 4, nullptr, nullptr), WC_E_ARG);

    // Host-only sizing helpers must be positive and deterministic.
    if (wc_conv3x3_x6_tile_n(64) != 64 || wc_conv3x3_x6_tile_n(320) != 128) {
        std::printf("FAIL wc_conv3x3_x6_tile_n\n");
        ++failures;
    }
    if (wc_gn_num_splits(16, 4096, 320) <= 0 || wc_gn_bwd_splits(16, 4096) <= 0 ||
        wc_conv_wgrad_splits(320, 2880, 65536, 1024) <= 0 || wc_mse_workspace_doubles() <= 0 ||
        wc_conv_wgrad3_splits(128, 128, 32, 256, 256, 512) <= 0 ||
        wc_conv_wgrad3_splits(128, 128, 32, 256, 256, 512) != wc_conv_wgrad3_splits(128, 128, 32, 256, 256, 512)) {
        std::printf("FAIL sizing helpers\n");
        ++failures;
    }

    // The wc_conv_args entry points, one fault at a time.
    failures += mut::run_all();

    std::printf("abi_validation: %d failure(s)\n", failures);
    return failures == 0 ? 0 : 1;
}
