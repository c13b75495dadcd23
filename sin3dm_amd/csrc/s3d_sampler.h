// s3d_sampler.h — the element-wise sampler update, shared by the stand-alone kernel (k_sampler, s3d_sampler_step) and the
// output head that applies it to the 12 model outputs it holds for a pixel (k_out_head_px<.., true>, SURVEY.md §2b K8 + K9).
// p_mean_variance (START_X | EPSILON, FIXED_* variance, clip) + p_sample / ddim_sample:
// src/diffusion/gaussian_diffusion.py:233-327, 329-335, 346-350, 396-440, 538-600.  Coefficients are the fp32 casts of the
// float64 tables, gathered per sample by t (as _extract_into_tensor does, :934-947).
// The reference evaluates these expressions as separate fp32 tensor operations, each rounded: every product, sum and quotient
// below is an explicit round-to-nearest operation in the reference's order — no fused multiply-add (the EPSILON branch
// subtracts two products of magnitude sqrt(1/alphas_cumprod) ~ 157 at t = 999: a contracted fma differs from the reference in
// the fourth decimal of a clamped x0).
#pragma once
#include "s3d_common.h"

namespace s3d {

// (HIP's __fmul_rn / __fadd_rn are plain `*` / `+` unless OCML_BASIC_ROUNDED_OPERATIONS is defined, i.e. still contractable:
// the functions below switch contraction off with `#pragma clang fp contract(off)`, which travels with the operations when they
// are inlined into a kernel.)
struct SamplerCoef {          // per-sample scalars of one step (gathered once per thread / block)
    float sr, srm1, c1, c2, sig_ddpm, nz;
    float sigma, ca, cb;      // ddim: sigma_t, sqrt(alpha_bar_prev), sqrt(1 - alpha_bar_prev - sigma^2)
};

__device__ __forceinline__ SamplerCoef sampler_coef(const s3d_sampler_args& a, int t) {
#pragma clang fp contract(off)
    SamplerCoef c;
    c.sr = a.tables[S3D_TAB_SQRT_RECIP * a.T + t]; c.srm1 = a.tables[S3D_TAB_SQRT_RECIPM1 * a.T + t];
    c.c1 = a.tables[S3D_TAB_COEF1 * a.T + t]; c.c2 = a.tables[S3D_TAB_COEF2 * a.T + t];
    c.nz = t != 0 ? 1.f : 0.f;
    c.sig_ddpm = c.nz * expf(0.5f * a.tables[S3D_TAB_LOGVAR * a.T + t]);      // nonzero_mask * exp(0.5 * log_variance)
    const float ab = a.tables[S3D_TAB_ACP * a.T + t], abp = a.tables[S3D_TAB_ACP_PREV * a.T + t];
    // eta * sqrt((1 - abp) / (1 - ab)) * sqrt(1 - ab / abp)      (:579-583)
    c.sigma = (a.eta * sqrtf((1.f - abp) / (1.f - ab))) * sqrtf(1.f - ab / abp);
    c.ca = sqrtf(abp);
    c.cb = sqrtf((1.f - abp) - c.sigma * c.sigma);
    return c;
}

// element i of the step: mo = the model's output there, xt = x_t[i], nv = the step's eps there (0 when the step has none).
// Writes sample / pred_xstart / mean as the mode asks; returns the value written to `sample` (x_{t-1}; 0 for MEAN_ONLY).
// STORE = false (sampler_element_known): `sample` is left to the caller, which stores the blended value once.
// LEAN (the output head's known-region instantiations, which sit at the scalar-register limit): the caller vouches that a.mean, a.y0
// and a.mask are null — the posterior-mean output and the x0 replacement are compiled out with the registers that held their pointers.
template <bool STORE = true, bool LEAN = false>
__device__ __forceinline__ float sampler_element(const s3d_sampler_args& a, const SamplerCoef& c, long long i, float mo, float xt, float nv) {
#pragma clang fp contract(off)
    float x0 = mo;
    float xprev = 0.f;
    if (a.mean_type == S3D_MEAN_EPSILON) {                                                                  // _predict_xstart_from_eps (:329-335)
        const float p1 = c.sr * xt, p2 = c.srm1 * mo;
        x0 = p1 - p2;
    }
    if (a.clip_denoised) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    if (a.mode == S3D_STEP_DDIM) {
        if (!LEAN && a.y0 && a.mask) {                                                                               // in-painting (:568-577)
            const float m = a.mask[i];
            const float q1 = m * a.y0[i], q2 = (1.f - m) * x0;
            const float mixed = q1 + q2;
            if (a.is_mask_t0) x0 = mixed;
            else { const float r1 = mixed * c.nz, r2 = x0 * (1.f - c.nz); x0 = r1 + r2; }
        }
        const float p1 = c.sr * xt;
        const float eps = (p1 - x0) / c.srm1;                                                               // _predict_eps_from_xstart (:346-350)
        const float m1 = x0 * c.ca, m2 = c.cb * eps;
        const float mean_pred = m1 + m2;
        const float nzs = (c.nz * c.sigma) * nv;
        xprev = mean_pred + nzs;
        if (STORE) a.sample[i] = xprev;
        a.pred_xstart[i] = x0;
    } else {
        const float m1 = c.c1 * x0, m2 = c.c2 * xt;                                                         // q_posterior_mean_variance (:218-221)
        const float mean = m1 + m2;
        if (!LEAN && a.mean) a.mean[i] = mean;
        a.pred_xstart[i] = x0;
        if (a.mode == S3D_STEP_DDPM) { const float nzs = c.sig_ddpm * nv; xprev = mean + nzs; if (STORE) a.sample[i] = xprev; }
    }
    return xprev;
}
__device__ __forceinline__ float sampler_element(const s3d_sampler_args& a, const SamplerCoef& c, long long i, float mo) {
    return sampler_element(a, c, i, mo, a.x[i], a.noise ? a.noise[i] : 0.f);
}

// Known-region sampling (outpainting / local editing; our own design, the reference has no such code): the
// known part of x_{t-1} is the source latent noised to level t - 1,
//     k      = (sa * y0) + (sb * ek)                     q_sample(y0, t - 1, ek); t == 0: sa = 1, sb = 0 (the table says so)
//     x_prev = (m * k) + ((1 - m) * x_prev_plain)
// every product and sum rounded on its own, in this order.  sa / sb are fp32 casts of float64 table values: derived here from
// S3D_TAB_ACP_PREV they would be one more rounding away from the float64 schedule.
struct KnownCoef { float sa, sb; };
__device__ __forceinline__ KnownCoef known_coef(const s3d_known_region& kr, int T, int t) {
    KnownCoef k;
    k.sa = kr.tables[S3D_KTAB_SQRT_ACP_PREV * T + t]; k.sb = kr.tables[S3D_KTAB_SQRT_1M_ACP_PREV * T + t];
    return k;
}
__device__ __forceinline__ float known_blend(const KnownCoef& kc, float y0, float m, float ek, float xprev_plain) {
#pragma clang fp contract(off)
    const float k1 = kc.sa * y0, k2 = kc.sb * ek;
    const float k = k1 + k2;
    const float b1 = m * k, b2 = (1.f - m) * xprev_plain;
    return b1 + b2;
}
// sampler_element with the blend: pred_xstart / mean as without it, `sample` stored once, blended; returns it.
template <bool LEAN = false>
__device__ __forceinline__ float sampler_element_known(const s3d_sampler_args& a, const SamplerCoef& c, const s3d_known_region& kr,
                                                       const KnownCoef& kc, long long i, float mo, float xt, float nv) {
    const float y0 = kr.y0[i], m = kr.mask[i], ek = kr.noise[i];             // (requested ahead of the update's arithmetic)
    const float plain = sampler_element<false, LEAN>(a, c, i, mo, xt, nv);
    const float xprev = known_blend(kc, y0, m, ek, plain);
    a.sample[i] = xprev;
    return xprev;
}
template <bool LEAN = false>
__device__ __forceinline__ float sampler_element_known(const s3d_sampler_args& a, const SamplerCoef& c, const s3d_known_region& kr,
                                                       const KnownCoef& kc, long long i, float mo) {
    return sampler_element_known<LEAN>(a, c, kr, kc, i, mo, a.x[i], a.noise ? a.noise[i] : 0.f);
}
// DPM-Solver++ multistep update (data prediction, orders 1 and 2M; DESIGN.md section 26 — our own addition, the reference samples
// with DDPM / DDIM only).  The front is sampler_element's: x0 = the model output (START_X) or (sr * x_t) - (srm1 * model_out)
// (EPSILON), clamped when clip_denoised.  Then
//     s = (cx * x_t) + (c0 * x0)              order 1
//     s = s + (c1 * x0_prev)                  order 2: the previous step's pred_xstart
//     s = s + (cn * eps)                      a.noise != null (the SDE form)
// every product and sum rounded on its own, in this order; sample = s, pred_xstart = x0.  cx / c0 / c1 / cn are fp32 casts of float64
// values computed on the host for the schedule's spacing (s3d_multistep.tables); a.tables serves sr / srm1 only.
struct MultistepCoef { float sr, srm1, cx, c0, c1, cn; };
__device__ __forceinline__ MultistepCoef multistep_coef(const s3d_sampler_args& a, const s3d_multistep& ms, int t) {
    MultistepCoef c;
    c.sr = a.tables[S3D_TAB_SQRT_RECIP * a.T + t]; c.srm1 = a.tables[S3D_TAB_SQRT_RECIPM1 * a.T + t];
    c.cx = ms.tables[S3D_MTAB_CX * a.T + t]; c.c0 = ms.tables[S3D_MTAB_C0 * a.T + t];
    c.c1 = ms.tables[S3D_MTAB_C1 * a.T + t]; c.cn = ms.tables[S3D_MTAB_CN * a.T + t];
    return c;
}
// element i of the step: mo / xt / nv as in sampler_element, xp = x0_prev[i] (anything when ms.order == 1: not used).  Writes
// pred_xstart and, with STORE, sample; returns the sample.  STORE = false: the caller stores the (blended) value once.
template <bool STORE = true>
__device__ __forceinline__ float multistep_element(const s3d_sampler_args& a, const s3d_multistep& ms, const MultistepCoef& c, long long i,
                                                   float mo, float xt, float nv, float xp) {
#pragma clang fp contract(off)
    float x0 = mo;
    if (a.mean_type == S3D_MEAN_EPSILON) {
        const float p1 = c.sr * xt, p2 = c.srm1 * mo;
        x0 = p1 - p2;
    }
    if (a.clip_denoised) x0 = fminf(fmaxf(x0, -1.f), 1.f);
    const float q1 = c.cx * xt, q2 = c.c0 * x0;
    float s = q1 + q2;
    if (ms.order == 2) { const float q3 = c.c1 * xp; s = s + q3; }
    if (a.noise) { const float q4 = c.cn * nv; s = s + q4; }
    if (STORE) a.sample[i] = s;
    a.pred_xstart[i] = x0;
    return s;
}
template <bool STORE = true>
__device__ __forceinline__ float multistep_element(const s3d_sampler_args& a, const s3d_multistep& ms, const MultistepCoef& c, long long i, float mo) {
    return multistep_element<STORE>(a, ms, c, i, mo, a.x[i], a.noise ? a.noise[i] : 0.f, ms.order == 2 ? ms.x0_prev[i] : 0.f);
}
// one level of re-noising between two repeats of a step: x_t = (sqrt(1 - beta_t) * x_prev) + (sqrt(beta_t) * er)
__device__ __forceinline__ float renoise_element(float c1mb, float cb, float xprev, float er) {
#pragma clang fp contract(off)
    const float p1 = c1mb * xprev, p2 = cb * er;
    return p1 + p2;
}

}  // namespace s3d
