// Segmentation label and metric kernels (include/wc_seg.h states the contracts).
//
//   label_kernel      out[b][y][x] = lut[src_b[rows_b[y]][cols_b[x]]]: the NEAREST resize + crop + id ->
//                     train-id encoding of a batch of label files, one launch over a DEVICE job table.
//   confusion_kernel  argmax over the class planes fused with the reference's _fast_hist.  A lane owns V
//                     consecutive pixels of the flat H*W index (V = 4: one 16-byte load per class plane;
//                     V = 1 when H*W % 4 != 0), walks the C planes once, and counts key = label * C + pred
//                     into the workgroup's C*C LDS counters.  Label maps are piecewise constant: equal keys of
//                     a lane's run are added once, and a wave whose 64 * V keys are all equal adds once for
//                     the whole wave.  A bounded grid strides over the pixel groups; at the end a workgroup
//                     adds only its non-zero cells to the int64 matrix (64-bit integer atomics: exact and
//                     independent of order).
//   decode_kernel     class map -> colours through a palette held in LDS.
#include "../../include/wc_seg.h"
#include "wc_common.hpp"

namespace {

constexpr int SEG_THREADS = 256;
constexpr int SEG_MAX_C = 32;
constexpr int SEG_WG_PER_CU = 4;               // the bounded grid: workgroups per compute unit
constexpr int64_t SEG_MAX_PIXELS = 1ll << 40;  // keeps a workgroup's 32-bit counters far from wrapping

struct LabelLut {
    unsigned char v[256];
};
struct Palette {
    uint32_t rgb[SEG_MAX_C + 1];  // r | g << 8 | b << 16
};

__global__ __launch_bounds__(SEG_THREADS) void label_kernel(const wc_label_job* __restrict__ jobs, int Hc, int Wc,
                                                            LabelLut lut, int64_t* __restrict__ out) {
    __shared__ unsigned char table[256];
    table[threadIdx.x] = lut.v[threadIdx.x];
    __syncthreads();
    const wc_label_job j = jobs[blockIdx.y];
    const unsigned char* src = static_cast<const unsigned char*>(j.src);
    const int64_t n = (int64_t)Hc * Wc;
    int64_t* dst = out + (int64_t)blockIdx.y * n;
    for (int64_t i = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SEG_THREADS) {
        const int y = (int)(i / Wc), x = (int)(i - (int64_t)y * Wc);
        const int r = j.rows[y], c = j.cols[x];
        int64_t v = 255;  // never for the tables the host checked
        if (r >= 0 && r < j.rect_h && c >= 0 && c < j.rect_w) v = table[src[(int64_t)r * j.pitch + c]];
        dst[i] = v;
    }
}

// One more class plane's value against the running best: strict >, a NaN beats every number, the first NaN stays.
WC_DEVICE void argmax_step(float v, int c, float& best, int& arg) {
    if ((v > best || v != v) && best == best) {
        best = v;
        arg = c;
    }
}

// V pixels per lane, CT classes at compile time (0: the run-time C), PRED: a ready prediction map instead of logits.
template <int V, int CT, bool PRED>
__global__ __launch_bounds__(SEG_THREADS) void confusion_kernel(const float* __restrict__ logits,
                                                                const unsigned char* __restrict__ preds,
                                                                const int64_t* __restrict__ labels, int64_t HW, int C_,
                                                                int64_t ngroups,
                                                                unsigned long long* __restrict__ hist,
                                                                unsigned char* __restrict__ pred_out) {
    __shared__ unsigned int counts[SEG_MAX_C * SEG_MAX_C];
    const int C = CT ? CT : C_;
    for (int i = threadIdx.x; i < C * C; i += SEG_THREADS) counts[i] = 0u;
    __syncthreads();

    const int64_t gpi = HW / V;  // pixel groups per image (V divides HW)
    const int64_t stride = (int64_t)gridDim.x * SEG_THREADS;
    // every lane of a wave runs the same number of trips (base is wave-uniform), so the wave votes below are whole
    for (int64_t base = (int64_t)blockIdx.x * SEG_THREADS; base < ngroups; base += stride) {
        const int64_t g = base + threadIdx.x;
        const bool live = g < ngroups;
        int key[V];
#pragma unroll
        for (int k = 0; k < V; ++k) key[k] = -1;
        if (live) {
            const int64_t b = g / gpi;
            const int64_t p = (g - b * gpi) * V;
            int arg[V];
            if constexpr (PRED) {
                const unsigned char* q = preds + b * HW + p;
                if constexpr (V == 4) {
                    const uint32_t w = *reinterpret_cast<const uint32_t*>(q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) arg[k] = (int)((w >> (8 * k)) & 255u);
                } else {
                    arg[0] = q[0];
                }
            } else {
                const float* q = logits + b * C * HW + p;
                float best[V];
                if constexpr (V == 4) {
                    const f32x4 v0 = *reinterpret_cast<const f32x4*>(q);
#pragma unroll
                    for (int k = 0; k < 4; ++k) best[k] = v0[k], arg[k] = 0;
                    if constexpr (CT != 0) {
#pragma unroll
                        for (int c = 1; c < CT; ++c) {
                            const f32x4 v = *reinterpret_cast<const f32x4*>(q + (int64_t)c * HW);
#pragma unroll
                            for (int k = 0; k < 4; ++k) argmax_step(v[k], c, best[k], arg[k]);
                        }
                    } else {
#pragma unroll 4
                        for (int c = 1; c < C; ++c) {
                            const f32x4 v = *reinterpret_cast<const f32x4*>(q + (int64_t)c * HW);
#pragma unroll
                            for (int k = 0; k < 4; ++k) argmax_step(v[k], c, best[k], arg[k]);
                        }
                    }
                } else {
                    best[0] = q[0], arg[0] = 0;
#pragma unroll 4
                    for (int c = 1; c < C; ++c) argmax_step(q[(int64_t)c * HW], c, best[0], arg[0]);
                }
                if (pred_out) {
                    unsigned char* o = pred_out + b * HW + p;
                    if constexpr (V == 4)
                        *reinterpret_cast<uint32_t*>(o) =
                            (uint32_t)arg[0] | (uint32_t)arg[1] << 8 | (uint32_t)arg[2] << 16 | (uint32_t)arg[3] << 24;
                    else
                        o[0] = (unsigned char)arg[0];
                }
            }
            const int64_t* lp = labels + b * HW + p;
            int64_t lab[V];
            if constexpr (V == 4) {
                const longlong2 l0 = *reinterpret_cast<const longlong2*>(lp);
                const longlong2 l1 = *reinterpret_cast<const longlong2*>(lp + 2);
                lab[0] = l0.x, lab[1] = l0.y, lab[2] = l1.x, lab[3] = l1.y;
            } else {
                lab[0] = lp[0];
            }
#pragma unroll
            for (int k = 0; k < V; ++k) {
                const bool ok = (uint64_t)lab[k] < (uint64_t)C && (!PRED || arg[k] < C);
                key[k] = ok ? (int)lab[k] * C + arg[k] : -1;
            }
        }
        // a wave whose keys are all one value (the inside of a constant region) adds once for the wave
        bool same = true;
#pragma unroll
        for (int k = 1; k < V; ++k) same = same && key[k] == key[0];
        const int first = __builtin_amdgcn_readfirstlane(key[0]);
        if (__all(same && key[0] == first)) {
            if (first >= 0 && (threadIdx.x & 63) == 0) atomicAdd(&counts[first], 64u * V);
            continue;
        }
        // otherwise every lane adds its runs of equal keys
        int cur = key[0];
        unsigned int cnt = 1u;
#pragma unroll
        for (int k = 1; k < V; ++k) {
            if (key[k] == cur) {
                ++cnt;
            } else {
                if (cur >= 0) atomicAdd(&counts[cur], cnt);
                cur = key[k];
                cnt = 1u;
            }
        }
        if (cur >= 0) atomicAdd(&counts[cur], cnt);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += SEG_THREADS) {
        const unsigned int v = counts[i];
        if (v) atomicAdd(hist + i, (unsigned long long)v);
    }
}

template <bool I64>
__global__ __launch_bounds__(SEG_THREADS) void decode_kernel(const void* __restrict__ map, int64_t n, int C, Palette pal,
                                                             unsigned char* __restrict__ out) {
    __shared__ uint32_t colours[SEG_MAX_C + 1];
    if (threadIdx.x <= C) colours[threadIdx.x] = pal.rgb[threadIdx.x];
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * SEG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SEG_THREADS) {
        uint64_t v;
        if constexpr (I64)
            v = (uint64_t) static_cast<const int64_t*>(map)[i];  // a negative value becomes a large one
        else
            v = static_cast<const unsigned char*>(map)[i];
        const uint32_t rgb = colours[v < (uint64_t)C ? (int)v : C];
        out[3 * i] = (unsigned char)(rgb & 255u);
        out[3 * i + 1] = (unsigned char)((rgb >> 8) & 255u);
        out[3 * i + 2] = (unsigned char)(rgb >> 16);
    }
}

// The bounded grid: SEG_WG_PER_CU workgroups per compute unit of the current device, at most `want`.
int bounded_grid(int64_t want, unsigned* grid) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return (int)e;
    const int64_t cap = (int64_t)(cus > 0 ? cus : 1) * SEG_WG_PER_CU;
    *grid = (unsigned)(want < cap ? (want < 1 ? 1 : want) : cap);
    return WC_OK;
}

int confusion_check(const void* in, const int64_t* labels, int B, int C, int H, int W, const int64_t* hist) {
    if (!in || !labels || !hist) return WC_E_ARG;
    if ((reinterpret_cast<uintptr_t>(labels) & 7) || (reinterpret_cast<uintptr_t>(hist) & 7)) return WC_E_ARG;
    if (B < 1 || C < 2 || C > SEG_MAX_C || H < 1 || W < 1) return WC_E_SHAPE;
    if ((int64_t)B * H * W > SEG_MAX_PIXELS) return WC_E_SHAPE;
    return WC_OK;
}

template <int V, int CT, bool PRED>
int confusion_launch(const float* logits, const unsigned char* preds, const int64_t* labels, int B, int C, int64_t HW,
                     int64_t* hist, unsigned char* pred_out, hipStream_t stream) {
    const int64_t ngroups = (int64_t)B * (HW / V);
    unsigned grid = 1;
    const int st = bounded_grid((ngroups + SEG_THREADS - 1) / SEG_THREADS, &grid);
    if (st != WC_OK) return st;
    hipLaunchKernelGGL((confusion_kernel<V, CT, PRED>), dim3(grid), dim3(SEG_THREADS), 0, stream, logits, preds, labels, HW,
                       C, ngroups, reinterpret_cast<unsigned long long*>(hist), pred_out);
    WC_CHECK_LAUNCH();
    return WC_OK;
}

// four pixels per lane need whole groups per image and the vector loads' alignment
bool wide_ok(int64_t HW, const void* labels, const void* bytes) {
    return HW % 4 == 0 && (reinterpret_cast<uintptr_t>(labels) & 15) == 0 && (reinterpret_cast<uintptr_t>(bytes) & 3) == 0;
}

}  // namespace

extern "C" int wc_label_batch(const wc_label_job* jobs, const wc_label_job* jobs_dev, int njobs, int Hc, int Wc,
                              const void* lut, int64_t* out, void* stream) {
    if (!jobs || !jobs_dev || !lut || !out) return WC_E_SHAPE;
    if (Hc < 1 || Wc < 1 || njobs < 1 || njobs > 65535) return WC_E_SHAPE;
    for (int i = 0; i < njobs; ++i) {
        const wc_label_job& j = jobs[i];
        if (!j.src || !j.rows || !j.cols || !j.rows_host || !j.cols_host) return WC_E_SHAPE;
        if (j.rect_w < 1 || j.rect_h < 1 || j.pitch < j.rect_w) return WC_E_SHAPE;
        for (int y = 0; y < Hc; ++y)
            if (j.rows_host[y] < 0 || j.rows_host[y] >= j.rect_h) return WC_E_SHAPE;
        for (int x = 0; x < Wc; ++x)
            if (j.cols_host[x] < 0 || j.cols_host[x] >= j.rect_w) return WC_E_SHAPE;
    }
    LabelLut table;
    for (int i = 0; i < 256; ++i) table.v[i] = static_cast<const unsigned char*>(lut)[i];
    const int64_t n = (int64_t)Hc * Wc;
    const int64_t want = (n + SEG_THREADS - 1) / SEG_THREADS;
    const unsigned gx = (unsigned)(want < 1024 ? want : 1024);
    hipLaunchKernelGGL(label_kernel, dim3(gx, (unsigned)njobs), dim3(SEG_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                       jobs_dev, Hc, Wc, table, out);
    WC_CHECK_LAUNCH();
    return WC_OK;
}

extern "C" int wc_seg_confusion(const float* logits, const int64_t* labels, int B, int C, int H, int W, int64_t* hist,
                                void* pred, void* stream) {
    const int st = confusion_check(logits, labels, B, C, H, W, hist);
    if (st != WC_OK) return st;
    if (reinterpret_cast<uintptr_t>(logits) & 15) return WC_E_ARG;
    const int64_t HW = (int64_t)H * W;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char* po = static_cast<unsigned char*>(pred);
    if (!wide_ok(HW, labels, pred)) return confusion_launch<1, 0, false>(logits, nullptr, labels, B, C, HW, hist, po, s);
    if (C == 19) return confusion_launch<4, 19, false>(logits, nullptr, labels, B, C, HW, hist, po, s);
    return confusion_launch<4, 0, false>(logits, nullptr, labels, B, C, HW, hist, po, s);
}

extern "C" int wc_seg_confusion_pred(const void* preds, const int64_t* labels, int B, int C, int H, int W, int64_t* hist,
                                     void* stream) {
    const int st = confusion_check(preds, labels, B, C, H, W, hist);
    if (st != WC_OK) return st;
    const int64_t HW = (int64_t)H * W;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const unsigned char* p = static_cast<const unsigned char*>(preds);
    if (!wide_ok(HW, labels, preds)) return confusion_launch<1, 0, true>(nullptr, p, labels, B, C, HW, hist, nullptr, s);
    return confusion_launch<4, 0, true>(nullptr, p, labels, B, C, HW, hist, nullptr, s);
}

extern "C" int wc_seg_decode(const void* map, int is_int64, int64_t n, int C, const void* palette, void* out,
                             void* stream) {
    if (!map || !palette || !out || (is_int64 != 0 && is_int64 != 1)) return WC_E_ARG;
    if (is_int64 && (reinterpret_cast<uintptr_t>(map) & 7)) return WC_E_ARG;
    if (n < 1 || n > SEG_MAX_PIXELS || C < 2 || C > SEG_MAX_C) return WC_E_SHAPE;
    Palette pal = {};
    const unsigned char* p = static_cast<const unsigned char*>(palette);
    for (int i = 0; i <= C; ++i) pal.rgb[i] = (uint32_t)p[3 * i] | (uint32_t)p[3 * i + 1] << 8 | (uint32_t)p[3 * i + 2] << 16;
    unsigned grid = 1;
    const int st = bounded_grid((n + SEG_THREADS - 1) / SEG_THREADS, &grid);
    if (st != WC_OK) return st;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    unsigned char* o = static_cast<unsigned char*>(out);
    if (is_int64)
        hipLaunchKernelGGL(decode_kernel<true>, dim3(grid), dim3(SEG_THREADS), 0, s, map, n, C, pal, o);
    else
        hipLaunchKernelGGL(decode_kernel<false>, dim3(grid), dim3(SEG_THREADS), 0, s, map, n, C, pal, o);
    WC_CHECK_LAUNCH();
    return WC_OK;
}
