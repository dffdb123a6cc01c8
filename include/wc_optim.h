/*
 * wc_optim.h — C ABI of the optimizer kernels of libwc_kernels.so (the conventions of wc_kernels.h:
 * caller-owned device memory, asynchronous on the given stream, WC_OK / WC_E_* / hipError_t returns).
 *
 * They stand in for the end of the reference's training iteration: optimizer.step()
 * (diffusion_model/train_ddpm.py:114, optimizer = Adam(model.parameters(), lr) at :190) and the
 * clipping the reference carries commented out at :112, clip_grad_norm_(model.parameters(), max_norm).
 */
#ifndef WC_OPTIM_H
#define WC_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor of an optimizer launch: parameter p, gradient g, moments m = exp_avg and v = exp_avg_sq,
 * n fp32 elements each, contiguous.  The tensors are cut into chunks of wc_optim_chunk_elems()
 * elements; chunk0 is the index of this tensor's first chunk in a numbering that runs through the
 * table (chunk0 of row i + 1 = chunk0 of row i + ceil(n_i / chunk)), so any run of consecutive rows is
 * itself a table. */
typedef struct wc_adam_job {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n, chunk0;
} wc_adam_job;
/* Elements per chunk (one workgroup's share of one tensor). */
int wc_optim_chunk_elems(void);
/* torch.optim.Adam / AdamW step (torch/optim/adam.py, the single-tensor path) of every tensor of one
 * parameter group in one launch, fp32, correctly rounded sqrt and division: jobs is a DEVICE array of
 * njobs rows covering nchunks chunks in all.  With g' = g * clip[0] (clip a device float, NULL: 1):
 *   weight_decay != 0: g' += weight_decay * p, or with decoupled p *= 1 - lr * weight_decay;
 *   m += (1 - beta1) (g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= step_size * m / (sqrt(v) / bc2_sqrt + eps),
 * step_size = lr / (1 - beta1^step) and bc2_sqrt = sqrt(1 - beta2^step) computed by the caller in
 * double.  A row whose four pointers are 16-byte aligned moves 16 bytes per lane, any other row 4;
 * nothing outside [0, n) of a tensor is read or written.  Elementwise: deterministic. */
int wc_adam_step(const wc_adam_job* jobs, int njobs, int nchunks, const float* clip, double step_size,
                 double bc2_sqrt, double beta1, double beta2, double eps, double lr, double weight_decay,
                 int decoupled, void* stream);
/* Global L2 norm of the rows' gradients (the total_norm of torch.nn.utils.clip_grad_norm_ over the same
 * tensors): workspace[chunk] (nchunks doubles) = the chunk's sum of squares in fp64, then one
 * workgroup adds them, both in a fixed order (no atomics: deterministic).  norm[0] = the norm,
 * clip[0] = min(1, max_norm / (norm + 1e-6)), device floats; a non-finite norm propagates. */
int wc_grad_norm(const wc_adam_job* jobs, int njobs, int nchunks, double max_norm, double* workspace,
                 float* norm, float* clip, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WC_OPTIM_H */
