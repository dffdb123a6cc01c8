/*
 * wc_sampler.h — C ABI of the strided sampling step of libwc_kernels.so (the conventions of
 * wc_kernels.h: caller-owned device memory, asynchronous on the given stream, WC_OK / WC_E_* /
 * hipError_t returns; the WC_NOISE_* modes are wc_kernels.h's).
 *
 * DDIM (Song et al. 2021, eq. 12) walks a sub-sequence of the trained schedule: one general
 * transition t -> t_to of the same eps-model.  eta = 1 is the respaced ancestral DDPM chain, eta = 0
 * run towards larger t is DDIM inversion.  The reference samples every timestep only; this goes
 * beyond it.
 */
#ifndef WC_SAMPLER_H
#define WC_SAMPLER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One transition t -> t_to, per element (fp32, every operation rounded once, no FMA contraction):
 *   x0   = (x - sqrt_1m_acp_t * eps) / sqrt_acp_t
 *   if clip_x0 and clamp(x0, -1, 1) != x0:
 *       x0  = clamp(x0, -1, 1)
 *       eps = (x - sqrt_acp_t * x0) / sqrt_1m_acp_t        (only the elements the clamp changed)
 *   mean = sqrt_acp_to * x0 + c_dir * eps
 *   x'   = mean + sigma * z                                 (sigma * z rounded before the add)
 * sz_out == NULL: x_out = x'; with noise_mode == WC_NOISE_NONE x_out = mean and z is not read.
 * sz_out != NULL: x_out = mean and sz_out = sigma * z, the pair the guided loop consumes (as
 * wc_ddpm_step).  x0_out (optional) receives x0 after clipping.  x_out may alias x: every lane loads
 * before it stores.  The scalars are the host's (LinearNoiseScheduler.ddim_scalars); the final step
 * t_to = -1 is sqrt_acp_to = 1, c_dir = sigma = 0.
 * Elements are (B, per_sample) contiguous, per_sample % 4 == 0, every pointer 16-byte aligned.  Philox
 * z has the bits of wc_ddpm_step / wc_philox_normal for the same (seed, sample0 + b, step, element).
 * Checked before any launch: null x / eps / x_out, noise_mode outside 0..2 or TENSOR without z,
 * sqrt_acp_t <= 0, a negative or NaN scalar, clip_x0 with sqrt_1m_acp_t == 0: WC_E_ARG;
 * per_sample % 4 != 0 or B < 1: WC_E_SHAPE. */
int wc_ddim_step(const float* x, const float* eps, const float* z, float* x_out, float* sz_out,
                 float* x0_out, int64_t B, int64_t per_sample, float sqrt_acp_t, float sqrt_1m_acp_t,
                 float sqrt_acp_to, float c_dir, float sigma, int clip_x0, int noise_mode,
                 uint64_t seed, int64_t sample0, int64_t step, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* WC_SAMPLER_H */
