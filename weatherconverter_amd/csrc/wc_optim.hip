// Optimizer kernels (reference diffusion_model/train_ddpm.py:111-114: clip_grad_norm_ (commented out
// there) and optimizer.step() of torch.optim.Adam): one launch updates every tensor of a parameter
// group, one two-pass launch pair gives the global gradient norm and the clip coefficient.
//
// Both read a DEVICE table of wc_adam_job.  The tensors are cut into chunks of OPT_CHUNK elements;
// job i owns the chunks [chunk0_i, chunk0_{i+1}) of a numbering that runs through the table, and a
// launch over the jobs [first, first + njobs) starts one workgroup per chunk: workgroup b works on
// chunk jobs[0].chunk0 + b and finds its job by bisecting the chunk0 column (<= 9 uniform loads for
// the 256-px model's 358 tensors), so a 30-element bias costs one workgroup and a 2.4-M-element conv
// weight gets 576 of them.
//
// A job whose four pointers are 16-byte aligned moves f32x4 (a chunk start is a multiple of 4
// elements); the n % 4 tail is done by the first lanes of the job's last chunk; any other job takes a
// coalesced one-float-per-lane path.  Nothing outside [0, n) of a tensor is read or written.
// Elementwise, so deterministic; HBM-bound at 16 B read + 12 B written per element.  The square
// root and the division are the correctly rounded ones (no fast-math flag on this file).
#include "wc_jobs.hpp"
#include "wc_optim.h"

namespace {

using namespace wcjobs;  // the chunk geometry, the global pointer types and find_job (shared with wc_ema.hip)

struct AdamHyper {
    float step_size;   // lr / (1 - beta1^step)
    float bc2_sqrt;    // sqrt(1 - beta2^step)
    float w1;          // 1 - beta1
    float beta2, w2;   // beta2, 1 - beta2
    float eps;
    float wd;          // L2 decay added to the gradient (mode 1)
    float shrink;      // 1 - lr * weight_decay (mode 2)
    int mode;          // 0 no decay, 1 L2, 2 decoupled
};

// torch/optim/adam.py _single_tensor_adam, fp32.  Every rounding is written out (no contraction left to
// the compiler), so the vector, tail and one-float paths give the same bits for the same element: the
// fused multiply-adds are those of torch's own kernels (add with alpha, lerp, addcmul, addcdiv).
WC_DEVICE void adam_one(float& p, float g, float& m, float& v, float clip, const AdamHyper& h) {
#pragma clang fp contract(off)
    g = g * clip;
    if (h.mode == 1) g = fmaf(h.wd, p, g);
    if (h.mode == 2) p = p * h.shrink;
    m = fmaf(h.w1, g - m, m);
    v = fmaf(h.w2 * g, g, h.beta2 * v);
    const float denom = sqrtf(v) / h.bc2_sqrt + h.eps;
    p = fmaf(-h.step_size, m / denom, p);
}

WC_DEVICE void adam_vec(f32x4& p, const f32x4& g, f32x4& m, f32x4& v, float clip, const AdamHyper& h) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float pe = p[e], me = m[e], ve = v[e];
        adam_one(pe, g[e], me, ve, clip, h);
        p[e] = pe;
        m[e] = me;
        v[e] = ve;
    }
}

__global__ __launch_bounds__(OPT_THREADS) void adam_step_kernel(const wc_adam_job* __restrict__ jobs, int njobs,
                                                                 const float* __restrict__ clip_ptr, AdamHyper h) {
    const int64_t c = jobs[0].chunk0 + blockIdx.x;
    const wc_adam_job j = jobs[find_job(jobs, njobs, c)];
    const int64_t off = (c - j.chunk0) * OPT_CHUNK;
    if (off >= j.n) return;  // a table whose chunk counts exceed its sizes: nothing to do here
    const float clip = clip_ptr ? clip_ptr[0] : 1.0f;
    const int64_t left = j.n - off;
    const int tid = threadIdx.x;
    const bool aligned = ((reinterpret_cast<uintptr_t>(j.p) | reinterpret_cast<uintptr_t>(j.g) |
                           reinterpret_cast<uintptr_t>(j.m) | reinterpret_cast<uintptr_t>(j.v)) & 15) == 0;
    if (!aligned) {
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        gf32* __restrict__ p = (gf32*)(j.p + off);
        gcf32* __restrict__ g = (gcf32*)(j.g + off);
        gf32* __restrict__ m = (gf32*)(j.m + off);
        gf32* __restrict__ v = (gf32*)(j.v + off);
        for (int i = tid; i < cnt; i += OPT_THREADS) {
            float pv = p[i], mv = m[i], vv = v[i];
            adam_one(pv, g[i], mv, vv, clip, h);
            p[i] = pv;
            m[i] = mv;
            v[i] = vv;
        }
        return;
    }
    gf32x4* __restrict__ p4 = (gf32x4*)(j.p + off);
    gcf32x4* __restrict__ g4 = (gcf32x4*)(j.g + off);
    gf32x4* __restrict__ m4 = (gf32x4*)(j.m + off);
    gf32x4* __restrict__ v4 = (gf32x4*)(j.v + off);
    if (left >= OPT_CHUNK) {  // a full chunk: every load issued before the first use
        f32x4 pv[OPT_VEC], gv[OPT_VEC], mv[OPT_VEC], vv[OPT_VEC];
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) {
            const int i = k * OPT_THREADS + tid;
            pv[k] = p4[i];
            gv[k] = g4[i];
            mv[k] = m4[i];
            vv[k] = v4[i];
        }
#pragma unroll
        for (int k = 0; k < OPT_VEC; ++k) {
            const int i = k * OPT_THREADS + tid;
            adam_vec(pv[k], gv[k], mv[k], vv[k], clip, h);
            p4[i] = pv[k];
            m4[i] = mv[k];
            v4[i] = vv[k];
        }
        return;
    }
    // the job's last chunk: whole vectors, then the n % 4 tail one float per lane
    const int n4 = (int)(left / 4);
    for (int i = tid; i < n4; i += OPT_THREADS) {
        f32x4 pv = p4[i], mv = m4[i], vv = v4[i];
        const f32x4 gv = g4[i];
        adam_vec(pv, gv, mv, vv, clip, h);
        p4[i] = pv;
        m4[i] = mv;
        v4[i] = vv;
    }
    const int i = n4 * 4 + tid;
    if (tid < 4 && i < (int)left) {
        gf32* __restrict__ p = (gf32*)(j.p + off);
        gf32* __restrict__ m = (gf32*)(j.m + off);
        gf32* __restrict__ v = (gf32*)(j.v + off);
        float pv = p[i], mv = m[i], vv = v[i];
        adam_one(pv, ((gcf32*)(j.g + off))[i], mv, vv, clip, h);
        p[i] = pv;
        m[i] = mv;
        v[i] = vv;
    }
}

// workspace[b] = sum of g^2 over chunk b of the table, fp64, in a fixed order: each lane adds its own
// elements in index order, the lanes of a wave by butterfly, the waves in order.
__global__ __launch_bounds__(OPT_THREADS) void grad_sq_kernel(const wc_adam_job* __restrict__ jobs, int njobs,
                                                               double* __restrict__ workspace) {
    const int64_t c = jobs[0].chunk0 + blockIdx.x;
    const wc_adam_job j = jobs[find_job(jobs, njobs, c)];
    const int64_t off = (c - j.chunk0) * OPT_CHUNK;
    const int64_t left = j.n - off;
    const int tid = threadIdx.x;
    double s = 0.0;
    if (left > 0) {
        const int cnt = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
        gcf32* __restrict__ g = (gcf32*)(j.g + off);
        if ((reinterpret_cast<uintptr_t>(j.g) & 15) == 0) {
            gcf32x4* __restrict__ g4 = (gcf32x4*)(j.g + off);
            const int n4 = cnt / 4;
            for (int i = tid; i < n4; i += OPT_THREADS) {
                const f32x4 gv = g4[i];
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fma((double)gv[e], (double)gv[e], s);
            }
            const int i = n4 * 4 + tid;
            if (tid < 4 && i < cnt) s = fma((double)g[i], (double)g[i], s);
        } else {
            for (int i = tid; i < cnt; i += OPT_THREADS) s = fma((double)g[i], (double)g[i], s);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double red[OPT_THREADS / 64];
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = 0.0;
        for (int w = 0; w < OPT_THREADS / 64; ++w) t += red[w];
        workspace[blockIdx.x] = t;
    }
}

// norm = sqrt(sum of the partials, fixed order); clip = min(1, max_norm / (norm + 1e-6)) as
// torch.nn.utils.clip_grad_norm_ computes it in fp32 (a NaN norm gives a NaN clip, as clamp does).
__global__ __launch_bounds__(OPT_THREADS) void grad_norm_final_kernel(const double* __restrict__ partials, int nparts,
                                                                       float max_norm, float* __restrict__ norm,
                                                                       float* __restrict__ clip) {
    __shared__ double red[OPT_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += OPT_THREADS) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = OPT_THREADS / 2; w > 0; w >>= 1) {
        if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float nrm = (float)sqrt(red[0]);
        const float coef = max_norm / (nrm + 1e-6f);
        norm[0] = nrm;
        clip[0] = coef > 1.0f ? 1.0f : coef;
    }
}

}  // namespace

extern "C" int wc_optim_chunk_elems(void) { return OPT_CHUNK; }

extern "C" int wc_adam_step(const wc_adam_job* jobs, int njobs, int nchunks, const float* clip, double step_size,
                            double bc2_sqrt, double beta1, double beta2, double eps, double lr, double weight_decay,
                            int decoupled, void* stream) {
    if (!jobs) return WC_E_ARG;
    if (njobs <= 0 || nchunks <= 0) return WC_E_SHAPE;
    AdamHyper h;
    h.step_size = (float)step_size;
    h.bc2_sqrt = (float)bc2_sqrt;
    h.w1 = (float)(1.0 - beta1);
    h.beta2 = (float)beta2;
    h.w2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.wd = (float)weight_decay;
    h.shrink = (float)(1.0 - lr * weight_decay);
    h.mode = weight_decay == 0.0 ? 0 : (decoupled ? 2 : 1);
    hipLaunchKernelGGL(adam_step_kernel, dim3((unsigned)nchunks), dim3(OPT_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), jobs, njobs, clip, h);
    WC_CHECK_LAUNCH();
    return WC_OK;
}

extern "C" int wc_grad_norm(const wc_adam_job* jobs, int njobs, int nchunks, double max_norm, double* workspace,
                            float* norm, float* clip, void* stream) {
    if (!jobs || !workspace || !norm || !clip) return WC_E_ARG;
    if (njobs <= 0 || nchunks <= 0) return WC_E_SHAPE;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grad_sq_kernel, dim3((unsigned)nchunks), dim3(OPT_THREADS), 0, st, jobs, njobs, workspace);
    WC_CHECK_LAUNCH();
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(OPT_THREADS), 0, st, workspace, nchunks, (float)max_norm,
                       norm, clip);
    WC_CHECK_LAUNCH();
    return WC_OK;
}
