// Weight-averaging kernels: the exponential moving average (EMA) of the weights a DDPM training loop
// keeps after optimizer.step() (reference diffusion_model/train_ddpm.py:114; the reference itself has no
// EMA), and the in-place exchange of the weights with their average that lets the engines sample from it.
//
// Both read a DEVICE table of wc_ema_job with the chunk numbering of wc_adam_job (wc_jobs.hpp): one
// workgroup per chunk of OPT_CHUNK elements finds its job by bisecting the chunk0 column, so ONE launch
// covers every tensor of the model.
//
// A job whose two pointers are 16-byte aligned moves f32x4 (a chunk start is a multiple of 4 elements);
// the n % 4 tail is done by the first lanes of the job's last chunk; any other job takes a coalesced
// one-float-per-lane path.  Nothing outside [0, n) of a tensor is read or written.  Elementwise, no
// atomics, so deterministic; HBM-bound at 8 B read + 4 B written per element (update) or 8 + 8 (swap).
#include "wc_ema.h"
#include "wc_jobs.hpp"

namespace {

using namespace wcjobs;

// UPDATE: e = e + w (p - e), torch's lerp_(p, w) for w < 0.5, with every rounding written out (no
// contraction left to the compiler), so the vector, tail and one-float paths give the same bits for the
// same element; p is left alone.  SWAP: the two values change places (moves only: the bits survive).
template <bool SWAP>
WC_DEVICE void ema_one(float& e, float& p, float w) {
#pragma clang fp contract(off)
    if constexpr (SWAP) {
        const float t = e;
        e = p;
        p = t;
    } else {
        e = fmaf(w, p - e, e);
    }
}

template <bool SWAP>
WC_DEVICE void ema_vec(f32x4& e, f32x4& p, float w) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float ek = e[k], pk = p[k];
        ema_one<SWAP>(ek, pk, w);
        e[k] = ek;
        p[k] = pk;
    }
}

template <bool SWAP>
__global__ __launch_bounds__(OPT_THREADS) void ema_kernel(const wc_ema_job* __restrict__ jobs, int njobs, float w) {
    const int64_t c = jobs[0].chunk0 + blockIdx.x;
    const wc_ema_job j = jobs[find_job(jobs, njobs, c)];
    const int64_t off = (c - j.chunk0) * OPT_CHUNK;
    if (off >= j.n) return;  // a table whose chunk counts exceed its sizes: nothing to do here
    const int64_t left = j.n - off;
    const int tid = threadIdx.x;
    gf32* __restrict__ e = (gf32*)(j.ema + off);
    gf32* __restrict__ p = (gf32*)(j.p + off);
    const bool aligned = ((reinterpret_cast<uintptr_t>(j.ema) | reinterpret_cast<uintptr_t>(j.p)) & 15) == 0;
    if (!aligned) {
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        for (int i = tid; i < cnt; i += OPT_THREADS) {
            float ev = e[i], pv = p[i];  // both loaded before either store
            ema_one<SWAP>(ev, pv, w);
            e[i] = ev;
            if constexpr (SWAP) p[i] = pv;
        }
        return;
    }
    gf32x4* __restrict__ e4 = (gf32x4*)(j.ema + off);
    gf32x4* __restrict__ p4 = (gf32x4*)(j.p + off);
    if (left >= OPT_CHUNK) {  // a full chunk: every load issued before the first use
        f32x4 ev[OPT_VEC], pv[OPT_VEC];
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) {
            const int i = k * OPT_THREADS + tid;
            ev[k] = e4[i];
            pv[k] = p4[i];
        }
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) {
            const int i = k * OPT_THREADS + tid;
            ema_vec<SWAP>(ev[k], pv[k], w);
            e4[i] = ev[k];
            if constexpr (SWAP) p4[i] = pv[k];
        }
        return;
    }
    // the job's last chunk: whole vectors, then the n % 4 tail one float per lane
    const int n4 = (int)(left / 4);
    for (int i = tid; i < n4; i += OPT_THREADS) {
        f32x4 ev = e4[i], pv = p4[i];
        ema_vec<SWAP>(ev, pv, w);
        e4[i] = ev;
        if constexpr (SWAP) p4[i] = pv;
    }
    const int i = n4 * 4 + tid;
    if (tid < 4 && i < (int)left) {
        float ev = e[i], pv = p[i];
        ema_one<SWAP>(ev, pv, w);
        e[i] = ev;
        if constexpr (SWAP) p[i] = pv;
    }
}

}  // namespace

extern "C" int wc_ema_update(const wc_ema_job* jobs, int njobs, int nchunks, double decay, void* stream) {
    if (!jobs) return WC_E_ARG;
    if (njobs <= 0 || nchunks <= 0) return WC_E_SHAPE;
    if (!(decay >= 0.0 && decay <= 1.0)) return WC_E_ARG;  // a NaN fails both comparisons
    hipLaunchKernelGGL(ema_kernel<false>, dim3((unsigned)nchunks), dim3(OPT_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), jobs, njobs, (float)(1.0 - decay));
    WC_CHECK_LAUNCH();
    return WC_OK;
}

extern "C" int wc_ema_swap(const wc_ema_job* jobs, int njobs, int nchunks, void* stream) {
    if (!jobs) return WC_E_ARG;
    if (njobs <= 0 || nchunks <= 0) return WC_E_SHAPE;
    hipLaunchKernelGGL(ema_kernel<true>, dim3((unsigned)nchunks), dim3(OPT_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), jobs, njobs, 0.0f);
    WC_CHECK_LAUNCH();
    return WC_OK;
}
