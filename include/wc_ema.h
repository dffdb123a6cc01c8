/*
 * wc_ema.h — C ABI of the weight-averaging kernels of libwc_kernels.so (the conventions of wc_optim.h:
 * caller-owned device memory, asynchronous on the given stream, WC_OK / WC_E_* / hipError_t returns).
 *
 * The exponential moving average (EMA) of the weights a DDPM training loop keeps beside its optimizer
 * and samples from (Ho et al. 2020, decay 0.9999).  The reference has none: this goes beyond it, as
 * max_grad_norm did, and follows the last line of the iteration, optimizer.step()
 * (diffusion_model/train_ddpm.py:114).
 */
#ifndef WC_EMA_H
#define WC_EMA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One tensor of an EMA launch: the shadow ema and the parameter p, n fp32 elements each, contiguous,
 * not overlapping.  The tensors are cut into chunks of wc_optim_chunk_elems() elements (wc_optim.h);
 * chunk0 is the index of this tensor's first chunk in a numbering that runs through the table, exactly
 * as in wc_adam_job. */
typedef struct wc_ema_job {
    float* ema;
    float* p;
    int64_t n, chunk0;
} wc_ema_job;
/* ema += (1 - decay) (p - ema) for every tensor of the table in one launch: jobs is a DEVICE array of
 * njobs rows covering nchunks chunks in all.  Per element ema = fmaf(w, p - ema, ema) with
 * w = (float)(1.0 - decay) formed in double; p is only read.  decay outside [0, 1] or NaN: WC_E_ARG.
 * A row whose two pointers are 16-byte aligned moves 16 bytes per lane, any other row 4, with the same
 * bits for the same element; nothing outside [0, n) of a tensor is read or written.  Elementwise:
 * deterministic.  (decay = 0 is not an initialisation: fmaf(1, p - ema, ema) need not give p's bits.) */
int wc_ema_update(const wc_ema_job* jobs, int njobs, int nchunks, double decay, void* stream);
/* Exchange p and ema of every tensor of the table, in place and bit for bit, in one launch (each lane
 * loads both values before it stores either).  Same table, access widths and bounds as wc_ema_update. */
int wc_ema_swap(const wc_ema_job* jobs, int njobs, int nchunks, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WC_EMA_H */
