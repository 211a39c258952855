// Diffusion algebra, RNG and optimiser kernels — all fp32, HBM-bound streaming kernels.
// Reference: gms/diffusion/gaussian_diffusion.py (training_losses :81-172, _run_model :61-77, _cf_guidance :174-187,
// ddim_step :189-213, reverse_dpm_step :215-243, sample :292) and gms/diffusion/diffusion_utils.py
// (diffusion_forward :65-73, diffusion_reverse :34-62, predict_* :76-105, _logsnr_schedule_cosine :198-201);
// torch.optim.Adam as diffusion_model.py:56 constructs it.  gmk_adam_ema_step's weight average has no reference call site (the
// reference keeps no EMA): an extension, defined by torch.lerp; so are gmk_adam_pema_step / gmk_arena_combine (the power-function averages
// of post-hoc EMA and their reconstruction: Karras et al. 2024, section 3.2 and appendix C).  gmk_dpm_solver_step (DPM-Solver++(2M)) is an extension too, and so are
// the variational-bound kernels gmk_q_sample_logsnr / gmk_vlb_term / gmk_vlb_endpoints (Kingma et al. 2021, continuous-time VDM bound) and
// the inpainting merge gmk_inpaint_merge (RePaint, Lugmayr et al. 2022) and dynamic thresholding (gmk_dyn_threshold, gmk_sampler_step_dt,
// gmk_dpm_solver_step_dt; Saharia et al. 2022).  gmk_grad_norm / gmk_adam_step_ctl (global-norm clipping by
// torch.nn.utils.clip_grad_norm_'s rule, and the non-finite guard GradScaler.step gives the reference at diffusion_model.py:71) are extensions.
// gmk_x_loss_w (the SNR+1 weighting of Salimans & Ho 2022 and Min-SNR-gamma, Hang et al. 2023, as w(logsnr) x_mse) and gmk_u_stratified
// (low-discrepancy training times, Kingma et al. 2021) are extensions too.  gmk_slerp (spherical interpolation of latent codes) is an extension as well.
// gmk_box_mean / gmk_box_residual / gmk_sampler_step_ns / gmk_dpm_solver_step_ns (DDNM's range-null-space projection of x-hat for box-mean
// operators: Wang, Yu & Zhang 2023) are extensions too.  gmk_consistency_target / gmk_x_loss_huber / gmk_consistency_step (consistency distillation and
// multistep consistency sampling: Song et al. 2023, Algorithms 1 and 2; the pseudo-Huber metric of Song & Dhariwal 2023) are extensions as well.
// gmk_cfg_rescale (the rescale factor of classifier-free guidance: Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are
// Flawed", section 3.4; the samplers apply it inside the guidance interval of Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval
// Improves Sample and Distribution Quality in Diffusion Models") is an extension, no reference call site.  gmk_stochastic_step is the ancestral
// posterior of diffusion_reverse (diffusion_utils.py:34-62) with all three of its x_logvar forms, of which the reference's sampler calls 'large'
// alone; DDIM with eta > 0 (Song et al. 2021) and SDE-DPM-Solver++(2M) (Lu et al. 2022) through the same entry are extensions.
// gmk_hybrid_loss / gmk_stochastic_step_lv / gmk_add_into (a learned reverse-process variance: Nichol & Dhariwal 2021, "Improved Denoising
// Diffusion Probabilistic Models", section 3.1 - the bound term is normal_kl of diffusion_utils.py:138-163 on diffusion_reverse's variances) are
// extensions, no reference call site.  gmk_gauss_blur / gmk_dps_backproject / gmk_dps_correct (diffusion posterior sampling: Chung et al. 2023,
// Algorithm 1, for box-mean and Gaussian-blur measurements) are extensions as well; they stand at the end of the file.
#include <float.h>
#include <math.h>

#include "gmk_common.h"

#define GMK_REQUIRE_MEAN_TYPE(mt, who) GMK_REQUIRE((mt) >= GMK_MEAN_V && (mt) <= GMK_MEAN_X, who ": mean_type must be 0 (v), 1 (eps) or 2 (x)")

namespace {

// cosine log-SNR schedule constants for logsnr in [-20, 20] (diffusion_utils.py:199-200), rounded to fp32 the way
// torch applies a Python/numpy double scalar to an fp32 tensor.
constexpr float kSchedB = 4.539992973129278e-05f;
constexpr float kSchedA = 1.5707055269354342f;

struct LogsnrCoef {
    float alpha, sigma;   // sqrt(sigmoid(l)), sqrt(sigmoid(-l))
    float c1, c2;         // sqrt(1 + e^l), rsqrt(1 + e^-l)   (predict_eps_from_x)
    float d1, d2;         // sqrt(1 + e^-l), rsqrt(1 + e^l)   (predict_x_from_eps)
};

__device__ __forceinline__ LogsnrCoef logsnr_coef(float l) {
    LogsnrCoef c;
    const float el = expf(l), eml = expf(-l);
    c.alpha = sqrtf(1.0f / (1.0f + eml));
    c.sigma = sqrtf(1.0f / (1.0f + el));
    c.c1 = sqrtf(1.0f + el);
    c.c2 = 1.0f / sqrtf(1.0f + eml);
    c.d1 = sqrtf(1.0f + eml);
    c.d2 = 1.0f / sqrtf(1.0f + el);
    return c;
}

__device__ __forceinline__ float clip1(float x) { return fminf(fmaxf(x, -1.0f), 1.0f); }

__device__ __forceinline__ float block_sum(float v, float* red) {   // 256 threads; every thread gets the total
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// ---- the reference's closed-form log-SNR schedules (diffusion_utils.py:169-201) with the range as arguments; GaussianDiffusion there picks
// 'cosine', -20, 20 (gaussian_diffusion.py:33-34): kSchedA / kSchedB, which gmk_q_sample and gmk_logsnr_schedule pass.
//   GMK_SCHED_COSINE       -2 log(tan(a u + b))        b = atan(exp(-lmax / 2)), a = atan(exp(-lmin / 2)) - b
//   GMK_SCHED_UNIFORM      lmin u + lmax (1 - u)
//   GMK_SCHED_BETA_CONST   -log(expm1(a u + b))        b = softplus(-lmax),      a = softplus(-lmin) - b
//   GMK_SCHED_BETA_LINEAR  -log(expm1(a (u u) + b))    as beta_const
// then + shift (skipped when shift == 0, so that no bit moves; the additive shift of Hoogeboom et al. 2023, an extension).  a, b come from the
// host (float64, rounded to fp32 the way torch applies a double scalar to an fp32 tensor); every operation here is one correctly rounded fp32
// operation in the reference's order - the products and sums through __fmul_rn / __fadd_rn, which the compiler may not contract - so numpy
// float32 restates the argument bit for bit.
// The kind is a run-time value, the same in every thread of a launch: one instantiation.  As a template argument it measured no faster
// (15.3-15.6 us per launch at 3 x 32 x 32, B = 2048, against 15.0-15.3 with the run-time switch).
__device__ __forceinline__ float sched_logsnr(int kind, float a, float b, float lmin, float lmax, float shift, float u) {
    float l;
    if (kind == GMK_SCHED_UNIFORM) {
        l = __fadd_rn(__fmul_rn(lmin, u), __fmul_rn(lmax, __fsub_rn(1.0f, u)));
    } else {
        const float t = __fadd_rn(__fmul_rn(a, kind == GMK_SCHED_BETA_LINEAR ? __fmul_rn(u, u) : u), b);
        l = kind == GMK_SCHED_COSINE ? -2.0f * logf(tanf(t)) : -logf(expm1f(t));
    }
    return shift != 0.0f ? __fadd_rn(l, shift) : l;
}

// grid (ceil(n/1024), B), 256 threads: z = x*alpha + eps*sigma with logsnr = schedule(u[b]), the schedule once per workgroup (every thread of
// it ahead of its loop).  Any n: image b starts at element b n, which is 16-byte aligned only when b n % 4 == 0, so the first `head` =
// (-b n) mod 4 elements of the image go one by one (the first `head` threads of workgroup 0), the 16-byte loads and stores start behind them -
// x, eps and z share the offset, hence the alignment - and the last (n - head) % 4 elements go one by one again.  With n % 4 == 0 (all
// gmk_q_sample takes) head is 0.  Each element is the same three operations on either path.
__global__ __launch_bounds__(256) void q_sample_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                      const float* __restrict__ u, float* __restrict__ logsnr,
                                                      float* __restrict__ z, int64_t n, int kind, float a, float sb, float lmin,
                                                      float lmax, float shift) {
    const int b = blockIdx.y;
    const float l = sched_logsnr(kind, a, sb, lmin, lmax, shift, u[b]);
    if (blockIdx.x == 0 && threadIdx.x == 0) logsnr[b] = l;
    const float alpha = sqrtf(1.0f / (1.0f + expf(-l)));
    const float sigma = sqrtf(1.0f / (1.0f + expf(l)));
    const int64_t base = (int64_t)b * n;
    const int64_t pad = (4 - (base & 3)) & 3;
    const int64_t head = pad < n ? pad : n;
    if (blockIdx.x == 0 && threadIdx.x < head)
        z[base + threadIdx.x] = __fadd_rn(__fmul_rn(x[base + threadIdx.x], alpha), __fmul_rn(sigma, eps[base + threadIdx.x]));
    for (int64_t i = head + (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        if (i + 3 < n) {
            float xv[4], ev[4], o[4];
            load4(x + base + i, xv);
            load4(eps + base + i, ev);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = __fadd_rn(__fmul_rn(xv[k], alpha), __fmul_rn(sigma, ev[k]));
            store4(z + base + i, o);
        } else {
            for (int64_t j = i; j < n; ++j)
                z[base + j] = __fadd_rn(__fmul_rn(x[base + j], alpha), __fmul_rn(sigma, eps[base + j]));
        }
    }
}

// the network output parametrises x (gaussian_diffusion.py:58-73): mean_type 0 'v' (predict_x_from_v), 1 'eps'
// (predict_x_from_eps), 2 'x'; d x / d out is the second function
__device__ __forceinline__ float x_from_out(float out, float zz, const LogsnrCoef& c, int mt) {
    return mt == GMK_MEAN_V ? c.alpha * zz - c.sigma * out : (mt == GMK_MEAN_EPS ? c.d1 * (zz - out * c.d2) : out);
}
__device__ __forceinline__ float dx_dout(const LogsnrCoef& c, int mt) { return mt == GMK_MEAN_V ? -c.sigma : (mt == GMK_MEAN_EPS ? -c.d1 * c.d2 : 1.0f); }

// The three loss kernels' element and their simple loss's gradient, once (tests hold the kernels to one another's bits).  clipped_pred: x-hat, the
// clipped prediction (:58-63, :73), eps-hat from it (:76), and whether the raw prediction lay inside [-1, 1], ends included - where torch.clip
// passes the gradient (a NaN is outside).  simple_loss_grad: torch.maximum routes the gradient to the larger branch, ties split evenly.
struct ClippedPred { float raw, xh, eh;  __device__ __forceinline__ bool inside() const { return raw >= -1.0f && raw <= 1.0f; } };
__device__ __forceinline__ ClippedPred clipped_pred(float out, float zz, const LogsnrCoef& c, int mt) {
    const float raw = x_from_out(out, zz, c, mt);
    const float xh = clip1(raw);
    return {raw, xh, c.c1 * (zz - xh * c.c2)};
}
struct SimpleLossGrad { float kx, ke; };      // d loss / d x-hat = kx (x-hat - x) + ke (eps-hat - eps)
__device__ __forceinline__ SimpleLossGrad simple_loss_grad(float xm, float em, int loss_type, float grad_scale, int64_t n, const LogsnrCoef& c) {
    const float gx = loss_type == 1 ? 0.f : (xm > em ? 1.f : (xm == em ? 0.5f : 0.f));
    const float ge = 1.f - gx;
    return {grad_scale * gx * 2.f / (float)n, grad_scale * ge * 2.f / (float)n * (-c.c1 * c.c2)};
}

// one block per sample: loss and (optionally) d loss / d (network output)
__global__ __launch_bounds__(256) void v_loss_kernel(const float* __restrict__ v, const float* __restrict__ z,
                                                    const float* __restrict__ x, const float* __restrict__ eps,
                                                    const float* __restrict__ logsnr, float* __restrict__ loss_b,
                                                    float* __restrict__ x_mse_o, float* __restrict__ eps_mse_o,
                                                    float* __restrict__ dv, float grad_scale, int64_t n, int loss_type, int mt) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const LogsnrCoef c = logsnr_coef(logsnr[b]);
    const int64_t base = (int64_t)b * n;
    float sx = 0.f, se = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float zz = z[base + i];
        const ClippedPred p = clipped_pred(v[base + i], zz, c, mt);
        const float dx = p.xh - x[base + i], de = p.eh - eps[base + i];
        sx = fmaf(dx, dx, sx);
        se = fmaf(de, de, se);
    }
    sx = block_sum(sx, red);
    se = block_sum(se, red);
    const float xm = sx / (float)n, em = se / (float)n;
    if (threadIdx.x == 0) {
        loss_b[b] = loss_type == 1 ? em : fmaxf(xm, em);                   // :171 'snr' (distillation step1) / :169 'snr_trunc'
        if (x_mse_o) x_mse_o[b] = xm;
        if (eps_mse_o) eps_mse_o[b] = em;
    }
    if (!dv) return;
    const SimpleLossGrad sg = simple_loss_grad(xm, em, loss_type, grad_scale, n, c);
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float zz = z[base + i];
        const float raw = x_from_out(v[base + i], zz, c, mt);      // clipped_pred's lines (the first pass calls it: keep in step), spelled out: through the call this loop takes one more VGPR
        const float xh = clip1(raw);
        const float eh = c.c1 * (zz - xh * c.c2);
        const float dxh = sg.kx * (xh - x[base + i]) + sg.ke * (eh - eps[base + i]);
        dv[base + i] = (raw >= -1.0f && raw <= 1.0f) ? dx_dout(c, mt) * dxh : 0.f;
    }
}

// ---- weighted x-space losses (gmk_x_loss_w); an extension, no reference call site.
// loss_b = w(l) mean_i (x_hat_i - x_i)^2 with w = 1 + e^l (GMK_LOSS_W_SNR_PLUS1: Salimans & Ho 2022, section 4, the v-space MSE) or
// w = min(e^l, gamma) (GMK_LOSS_W_MIN_SNR: Hang et al. 2023), x_hat the clipped prediction of v_loss_kernel.  Neither needs eps or eps-hat,
// so the pass reads v, z and x where v_loss_kernel reads four tensors twice.
//
// One workgroup of 256 threads per image.  The residuals d_i = x_hat_i - x_i go through LDS in chunks of kXLossKeep values: the loads are
// 16 bytes wide where VEC allows (thread t takes elements 4t .. 4t + 3 of every 1024), the sums are not - thread t adds d_i^2 for
// i = t, t + 256, ... in ascending order with fmaf, then block_sum: v_loss_kernel's element-to-thread assignment and order on either path
// (kXLossKeep is a multiple of 256, so a chunk boundary does not move an element to another thread), hence its x_mse bits.
// An image of n <= kXLossKeep values is one chunk, and the gradient pass reads it back from LDS instead of from global memory: each thread
// re-reads the residuals it wrote itself and zeroes those whose raw prediction left [-1, 1] (one bit per element, at most 48, in a register
// pair).  Larger images are read again.  LDS: 4 min(n, kXLossKeep) bytes (12 KiB at 3 x 32 x 32, 48 KiB at the capacity) + 16 for block_sum,
// all of it dynamic so that the 16-byte accesses stay aligned.
// HUBER (gmk_x_loss_huber; the pseudo-Huber metric of Song & Dhariwal 2023, "Improved Techniques for Training Consistency Models", with
// c_paper = c sqrt(n), scaled by 1 / sqrt(n)): the same passes and the same x_mse bits; loss_b = r - c with r = sqrt(x_mse + c^2) and the
// gradient's factor grad_scale / (n r) in place of grad_scale w 2 / n.  `gamma` carries c; weight_type is not read.
constexpr int kXLossKeep = GMK_X_LOSS_KEEP;    // kDynKeys: covers 3 x 64 x 64

template <bool VEC, bool HUBER = false>
__global__ __launch_bounds__(256) void x_loss_w_kernel(const float* __restrict__ v, const float* __restrict__ z, const float* __restrict__ x,
                                                      const float* __restrict__ logsnr, float* __restrict__ loss_b,
                                                      float* __restrict__ x_mse_o, float* __restrict__ dv, float grad_scale, int weight_type,
                                                      float gamma, int64_t n, int mt, int lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float res[];      // lds_floats residuals, then block_sum's four partials
    float* red = res + lds_floats;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const float l = logsnr[b];
    const LogsnrCoef c = logsnr_coef(l);
    const int64_t base = (int64_t)b * n;
    const bool keep = dv && n <= kXLossKeep;
    constexpr int STEP = VEC ? 4 : 1;        // consecutive elements a thread takes per pass over 256 * STEP
    uint64_t clipped = 0;                    // keep: bit (STEP g + k) for element k of this thread's g-th group
    float sx = 0.f;
    for (int64_t c0 = 0; c0 < n; c0 += kXLossKeep) {
        const int m = (int)(n - c0 < kXLossKeep ? n - c0 : kXLossKeep);
        if (c0) __syncthreads();             // the last chunk's residuals have been summed
        int bit = 0;
        for (int i = tid * STEP; i < m; i += 256 * STEP, bit += STEP) {
            float vv[STEP], zv[STEP], xv[STEP], d[STEP];
            if constexpr (VEC) {
                load4(v + base + c0 + i, vv); load4(z + base + c0 + i, zv); load4(x + base + c0 + i, xv);
            } else {
                vv[0] = v[base + c0 + i]; zv[0] = z[base + c0 + i]; xv[0] = x[base + c0 + i];
            }
#pragma unroll
            for (int k = 0; k < STEP; ++k) {
                const ClippedPred p = clipped_pred(vv[k], zv[k], c, mt);
                d[k] = p.xh - xv[k];
                if (keep && !p.inside()) clipped |= (uint64_t)1 << (bit + k);
            }
            if constexpr (VEC) store4(res + i, d); else res[i] = d[0];
        }
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const float dx = res[i];
            sx = fmaf(dx, dx, sx);
        }
    }
    sx = block_sum(sx, red);
    const float xm = sx / (float)n;
    float w, kx;
    if constexpr (HUBER) {
        w = sqrtf(xm + gamma * gamma);       // r: sqrt(c c) is c itself, so a zero residual is a zero loss
        kx = grad_scale / ((float)n * w);
        if (tid == 0) loss_b[b] = w - gamma;
    } else {
        const float el = expf(l);
        w = weight_type == GMK_LOSS_W_SNR_PLUS1 ? 1.0f + el : fminf(el, gamma);
        kx = grad_scale * w * 2.f / (float)n;
        if (tid == 0) loss_b[b] = w * xm;
    }
    if (tid == 0) x_mse_o[b] = xm;
    if (!dv) return;
    // torch.clip passes the gradient inside [-1, 1], ends included (v_loss_kernel's rule); w depends on l alone
    const float dxo = dx_dout(c, mt);
    if (keep) {
        int bit = 0;
        for (int i = tid * STEP; i < (int)n; i += 256 * STEP, bit += STEP) {
            float d[STEP];
            if constexpr (VEC) load4(res + i, d); else d[0] = res[i];
#pragma unroll
            for (int k = 0; k < STEP; ++k) d[k] = ((clipped >> (bit + k)) & 1) ? 0.f : dxo * (kx * d[k]);
            if constexpr (VEC) store4(dv + base + i, d); else dv[base + i] = d[0];
        }
        return;
    }
    for (int64_t i = (int64_t)tid * STEP; i < n; i += 256 * STEP) {
        float vv[STEP], zv[STEP], xv[STEP], d[STEP];
        if constexpr (VEC) {
            load4(v + base + i, vv); load4(z + base + i, zv); load4(x + base + i, xv);
        } else {
            vv[0] = v[base + i]; zv[0] = z[base + i]; xv[0] = x[base + i];
        }
#pragma unroll
        for (int k = 0; k < STEP; ++k) {
            const ClippedPred p = clipped_pred(vv[k], zv[k], c, mt);
            d[k] = p.inside() ? dxo * (kx * (p.xh - xv[k])) : 0.f;
        }
        if constexpr (VEC) store4(dv + base + i, d); else dv[base + i] = d[0];
    }
}

// ---- the hybrid loss of a learned reverse-process variance (gmk_hybrid_loss; Nichol & Dhariwal 2021, "Improved DDPM", section 3.1); an
// extension, no reference call site.  The simple loss, x_mse, eps_mse and dv are v_loss_kernel's: the same expressions, the same
// element-to-thread assignment and summation order (thread t adds elements t, t + 256, ... in ascending order with fmaf, then block_sum), so the
// same bits.  The bound term is the KL divergence of the posterior q(z_s | z_t, x) (diffusion_reverse's 'small' variance) from the model's
// p(z_s | z_t) - the same mean at x_hat (a constant: stop-gradient) and the 'medium' interpolation with the per-element fraction
// f = (nu + 1) / 2 - in the closed form of gmk.h: with D = softplus(ls) - softplus(lt) and g = -expm1(lt - ls) e^ls per image,
//   KL_i = (f D + expm1(-f D) + e^(-f D) g d_i^2) / 2,   d nu_i = grad_scale lambda / n  D / 4  (1 - e^(-f D) (1 + g d_i^2)).
// d nu needs no reduction, so it is written in the first pass: nu is read once whatever n.
// One workgroup of 256 threads per image, x_loss_w_kernel's shape: the residuals d_i = x_hat_i - x_i and eps_hat_i - eps_i go through LDS
// in chunks of kXLossKeep values (16-byte loads where VEC allows; the strided sums read them back), and an image of n <= kXLossKeep values
// is one chunk whose gradient pass reads LDS instead of global memory (v, nu, z, x, eps are read once).  Larger images read v, z, x, eps again.
// LDS: 8 min(n, kXLossKeep) + 16 bytes, dynamic (24 KiB at 3 x 32 x 32, 96 KiB at the capacity).  No atomics.
__device__ __forceinline__ float softplus_f(float l) { return fmaxf(l, 0.0f) + log1pf(expf(-fabsf(l))); }

template <bool VEC>
__global__ __launch_bounds__(256) void hybrid_loss_kernel(const float* __restrict__ v, const float* __restrict__ nu, const float* __restrict__ z,
                                                         const float* __restrict__ x, const float* __restrict__ eps,
                                                         const float* __restrict__ logsnr, const float* __restrict__ logsnr_s,
                                                         float* __restrict__ loss_b, float* __restrict__ vlb_b, float* __restrict__ frac_b,
                                                         float* __restrict__ x_mse_o, float* __restrict__ eps_mse_o, float* __restrict__ dv,
                                                         float* __restrict__ dnu, float grad_scale, float lambda, int64_t n, int loss_type,
                                                         int mt, int lds_floats) {
    extern __shared__ __attribute__((aligned(16))) float hres[];     // lds_floats x residuals, lds_floats eps residuals, block_sum's four partials
    float* resx = hres;
    float* rese = hres + lds_floats;
    float* red = rese + lds_floats;
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const float lt = logsnr[b], ls = logsnr_s[b];
    const LogsnrCoef c = logsnr_coef(lt);
    const float delta = softplus_f(ls) - softplus_f(lt);            // logvar_large - logvar_small
    const float g = -expm1f(lt - ls) * expf(ls);
    const float knu = grad_scale * lambda / (float)n * (0.25f * delta);
    const int64_t base = (int64_t)b * n;
    const bool keep = dv && n <= kXLossKeep;
    constexpr int STEP = VEC ? 4 : 1;
    uint64_t clipped = 0;                    // keep: bit (STEP g + k) for element k of this thread's g-th group
    float sx = 0.f, se = 0.f, skl = 0.f, sf = 0.f;
    for (int64_t c0 = 0; c0 < n; c0 += kXLossKeep) {
        const int m = (int)(n - c0 < kXLossKeep ? n - c0 : kXLossKeep);
        if (c0) __syncthreads();             // the last chunk's residuals have been summed
        int bit = 0;
        for (int i = tid * STEP; i < m; i += 256 * STEP, bit += STEP) {
            float vv[STEP], nv[STEP], zv[STEP], xv[STEP], ev[STEP], dx[STEP], de[STEP], dn[STEP];
            if constexpr (VEC) {
                load4(v + base + c0 + i, vv); load4(nu + base + c0 + i, nv); load4(z + base + c0 + i, zv);
                load4(x + base + c0 + i, xv); load4(eps + base + c0 + i, ev);
            } else {
                vv[0] = v[base + c0 + i]; nv[0] = nu[base + c0 + i]; zv[0] = z[base + c0 + i];
                xv[0] = x[base + c0 + i]; ev[0] = eps[base + c0 + i];
            }
#pragma unroll
            for (int k = 0; k < STEP; ++k) {
                const ClippedPred p = clipped_pred(vv[k], zv[k], c, mt);
                dx[k] = p.xh - xv[k];
                de[k] = p.eh - ev[k];
                if (keep && !p.inside()) clipped |= (uint64_t)1 << (bit + k);
                const float f = 0.5f * (nv[k] + 1.0f);
                const float a = f * delta;
                const float ema = expf(-a);
                const float q = g * (dx[k] * dx[k]);
                skl += 0.5f * (a + expm1f(-a) + ema * q);
                sf += f;
                dn[k] = knu * (1.0f - ema * (1.0f + q));
            }
            if constexpr (VEC) {
                store4(resx + i, dx); store4(rese + i, de);
                if (dnu) store4(dnu + base + c0 + i, dn);
            } else {
                resx[i] = dx[0]; rese[i] = de[0];
                if (dnu) dnu[base + c0 + i] = dn[0];
            }
        }
        __syncthreads();
        for (int i = tid; i < m; i += 256) {
            const float dx = resx[i], de = rese[i];
            sx = fmaf(dx, dx, sx);
            se = fmaf(de, de, se);
        }
    }
    sx = block_sum(sx, red);
    se = block_sum(se, red);
    skl = block_sum(skl, red);
    sf = block_sum(sf, red);
    const float xm = sx / (float)n, em = se / (float)n;
    if (tid == 0) {
        const float vlb = skl / (float)n;
        loss_b[b] = (loss_type == 1 ? em : fmaxf(xm, em)) + lambda * vlb;
        vlb_b[b] = vlb;
        frac_b[b] = sf / (float)n;
        x_mse_o[b] = xm;
        eps_mse_o[b] = em;
    }
    if (!dv) return;
    // v_loss_kernel's gradient of the simple loss: the bound's mean is a constant, so dv has no other term
    const SimpleLossGrad sg = simple_loss_grad(xm, em, loss_type, grad_scale, n, c);
    if (keep) {
        int bit = 0;
        for (int i = tid * STEP; i < (int)n; i += 256 * STEP, bit += STEP) {
            float dx[STEP], de[STEP], o[STEP];
            if constexpr (VEC) { load4(resx + i, dx); load4(rese + i, de); } else { dx[0] = resx[i]; de[0] = rese[i]; }
#pragma unroll
            for (int k = 0; k < STEP; ++k) {
                const float dxh = sg.kx * dx[k] + sg.ke * de[k];
                o[k] = ((clipped >> (bit + k)) & 1) ? 0.f : dx_dout(c, mt) * dxh;
            }
            if constexpr (VEC) store4(dv + base + i, o); else dv[base + i] = o[0];
        }
        return;
    }
    for (int64_t i = (int64_t)tid * STEP; i < n; i += 256 * STEP) {
        float vv[STEP], zv[STEP], xv[STEP], ev[STEP], o[STEP];
        if constexpr (VEC) {
            load4(v + base + i, vv); load4(z + base + i, zv); load4(x + base + i, xv); load4(eps + base + i, ev);
        } else {
            vv[0] = v[base + i]; zv[0] = z[base + i]; xv[0] = x[base + i]; ev[0] = eps[base + i];
        }
#pragma unroll
        for (int k = 0; k < STEP; ++k) {
            const ClippedPred p = clipped_pred(vv[k], zv[k], c, mt);
            const float dxh = sg.kx * (p.xh - xv[k]) + sg.ke * (p.eh - ev[k]);
            o[k] = p.inside() ? dx_dout(c, mt) * dxh : 0.f;
        }
        if constexpr (VEC) store4(dv + base + i, o); else dv[base + i] = o[0];
    }
}

// u[b] = frac(u0[0] + b / B): one uniform offset per batch, evenly spaced times (Kingma et al. 2021, VDM, App. I.1), as
//   s = b / B,  c = 1 - s,  u[b] = u0 >= c ? u0 - c : min(u0 + s, 1 - 2^-24)
// - single correctly rounded fp32 operations, so numpy float32 restates it bit for bit.  The wrap is taken BEFORE the sum: u0 + s itself is
// not exact at or above 1 (fp32 keeps multiples of 2^-23 there: with u0 = 1 - 2^-24 and B = 8 it rounds 1.125 - 2^-24 up to 1.125 and leaves
// [0, 1/8) empty).  With B a power of two and u0 a multiple of 2^-24 (what gmk_rng_uniform draws) every operation here is exact: each
// [k / B, (k + 1) / B) holds exactly one u.  The min only guards other B, where u0 + s just below 1 could round to 1.
__global__ __launch_bounds__(256) void u_stratified_kernel(const float* __restrict__ u0, float* __restrict__ u, int B) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float o = u0[0];
    const float s = __fdiv_rn((float)b, (float)B);
    const float c = __fsub_rn(1.0f, s);
    u[b] = o >= c ? __fsub_rn(o, c) : fminf(__fadd_rn(o, s), 0x1.fffffep-1f);
}

// ---- the per-log-SNR loss profile and the loss-aware time sampler (Nichol & Dhariwal 2021, "Improved DDPM", section 3.3); extensions, no
// reference call site.  GMK_PROFILE_BINS = 64 bins of equal width in u, one per lane of a wavefront; the state is fp32 [5][64]: W (decayed
// sample count), then (S1, S2) = decayed sum and sum of squares of value channel 0 and of value channel 1.  Both kernels are single correctly
// rounded fp32 operations in a stated order (u_stratified_kernel's idiom), so numpy float32 restates them bit for bit.  The square root is
// __builtin_sqrtf, which this build rounds correctly (as it does `/`); __fsqrt_rn is the native approximation without OCML's rounded operations.
constexpr int kProfileBins = GMK_PROFILE_BINS;
constexpr int kProfileTile = 1024;                // samples staged in LDS per pass: bin, v0, v1 = 12 KiB
static_assert(kProfileBins == 64, "one bin per lane of a wavefront");

__device__ __forceinline__ float sqrt_rn(float x) { return __builtin_sqrtf(x); }

struct ProfileAcc {
    int n;
    float a0, q0, a1, q1;
    __device__ __forceinline__ void add(int bin, int lane, float x0, float x1) {
        if (bin == lane) {
            ++n;
            a0 = __fadd_rn(a0, x0); q0 = __fadd_rn(q0, __fmul_rn(x0, x0));
            a1 = __fadd_rn(a1, x1); q1 = __fadd_rn(q1, __fmul_rn(x1, x1));
        }
    }
};

// One workgroup.  All 256 threads stage a tile of samples in LDS as (bin or -1, v0, v1): bin = min((int)(u 64), 63), -1 for a sample that is
// skipped (u outside [0, 1), or a value that is not finite - one NaN loss must not poison the state for the rest of the run).  Then lane k of
// wave 0 walks the tile in ascending b and adds the samples of bin k: n = their count, a_c = the sequential sum of the values, q_c of their
// squares (LDS reads of one address by every lane: broadcasts).  After the last tile a bin with n > 0 takes
//   W = decay W + n,  S1_c = decay S1_c + a_c,  S2_c = decay S2_c + q_c;
// a bin with n = 0 keeps its five words' bits, and rows 3 and 4 keep theirs when v1 is NULL.  No atomics: a pure function of the inputs.
__global__ __launch_bounds__(256) void loss_profile_kernel(const float* __restrict__ u, const float* __restrict__ v0, const float* __restrict__ v1,
                                                           int B, float decay, float* __restrict__ state) {
    __shared__ __align__(16) int s_bin[kProfileTile];
    __shared__ __align__(16) float s_v0[kProfileTile];
    __shared__ __align__(16) float s_v1[kProfileTile];
    const int lane = threadIdx.x;
    ProfileAcc acc = {0, 0.f, 0.f, 0.f, 0.f};
    for (int base = 0; base < B; base += kProfileTile) {
        const int m = min(kProfileTile, B - base);
        const int m4 = (m + 3) & ~3;                    // the walk reads four samples at a time: the tail is padded with skipped ones
        __syncthreads();                                // the previous tile has been walked
        for (int i = threadIdx.x; i < m4; i += 256) {
            int bin = -1;
            float x0 = 0.f, x1 = 0.f;
            if (i < m) {
                const float uu = u[base + i];
                x0 = v0[base + i];
                x1 = v1 ? v1[base + i] : 0.f;
                if (uu >= 0.f && uu < 1.f && isfinite(x0) && isfinite(x1)) bin = min((int)__fmul_rn(uu, 64.f), kProfileBins - 1);
            }
            s_bin[i] = bin; s_v0[i] = x0; s_v1[i] = x1;
        }
        __syncthreads();
        if (threadIdx.x < kProfileBins) {
            for (int i = 0; i < m4; i += 4) {
                const int4 b4 = *reinterpret_cast<const int4*>(s_bin + i);
                const float4 x = *reinterpret_cast<const float4*>(s_v0 + i);
                const float4 y = *reinterpret_cast<const float4*>(s_v1 + i);
                acc.add(b4.x, lane, x.x, y.x);
                acc.add(b4.y, lane, x.y, y.y);
                acc.add(b4.z, lane, x.z, y.z);
                acc.add(b4.w, lane, x.w, y.w);
            }
        }
    }
    if (threadIdx.x < kProfileBins && acc.n > 0) {
        float* W = state + lane;
        W[0] = __fadd_rn(__fmul_rn(decay, W[0]), (float)acc.n);
        W[1 * kProfileBins] = __fadd_rn(__fmul_rn(decay, W[1 * kProfileBins]), acc.a0);
        W[2 * kProfileBins] = __fadd_rn(__fmul_rn(decay, W[2 * kProfileBins]), acc.q0);
        if (v1) {
            W[3 * kProfileBins] = __fadd_rn(__fmul_rn(decay, W[3 * kProfileBins]), acc.a1);
            W[4 * kProfileBins] = __fadd_rn(__fmul_rn(decay, W[4 * kProfileBins]), acc.q1);
        }
    }
}

// The inverse-CDF draw from the profile and its importance weight.  Every workgroup forms the same table in bin order (wave 0, lane k = bin k;
// the two running sums are the same 64 sequential additions in every lane):
//   ready = every W_k >= warm;  r_k = sqrt(S2_k / W_k) (channel 0),  R = r_0 + ... + r_63 in that order
//   p_k = (r_k / R) (1 - floor) + floor / 64  when ready and R is finite and > 0,  else 2^-6 (uniform)
//   c_0 = 0, c_{k+1} = c_k + p_k, C = c_64;  w_k = C / (64 p_k)
// and thread b draws t = u0[b] C, k = the largest index with c_k <= t, f = min((t - c_k) / p_k, 1 - 2^-24),
//   u[b] = min((k + f) 2^-6, the float below (k + 1) 2^-6),  w[b] = w_k.
// The last min keeps u inside bin k and below 1, so w[b] is the table's entry of u[b]'s bin.  With p_k = 2^-6 every operation is exact for
// every fp32 u0 in [0, 1): u = u0 bit for bit and w = 1 - a run inside the sampler's warm-up is the run without it.
__global__ __launch_bounds__(256) void u_importance_kernel(const float* __restrict__ state, const float* __restrict__ u0, float* __restrict__ u,
                                                           float* __restrict__ w, int B, float warm, float floor_, float* __restrict__ p_out,
                                                           float* __restrict__ w_out) {
    __shared__ float s_r[kProfileBins], s_p[kProfileBins], s_w[kProfileBins], s_c[kProfileBins + 1];
    const int k0 = threadIdx.x;
    const bool table = k0 < kProfileBins;               // wave 0, all 64 lanes
    bool ready = false;
    float r = 0.f, p = 0.015625f;
    if (table) {
        const float W = state[k0], S2 = state[2 * kProfileBins + k0];
        ready = __ballot(W >= warm) == ~0ull;
        r = sqrt_rn(__fdiv_rn(S2, W));
        s_r[k0] = r;
    }
    __syncthreads();
    if (table) {
        float R = 0.f;
        for (int j = 0; j < kProfileBins; ++j) R = __fadd_rn(R, s_r[j]);
        if (ready && isfinite(R) && R > 0.f)
            p = __fadd_rn(__fmul_rn(__fdiv_rn(r, R), __fsub_rn(1.0f, floor_)), __fdiv_rn(floor_, 64.f));
        s_p[k0] = p;
    }
    __syncthreads();
    if (table) {
        float c = 0.f, ck = 0.f;
        for (int j = 0; j < kProfileBins; ++j) {
            if (j == k0) ck = c;
            c = __fadd_rn(c, s_p[j]);
        }
        const float wk = __fdiv_rn(c, __fmul_rn(64.f, p));
        s_c[k0] = ck;
        if (k0 == 0) s_c[kProfileBins] = c;
        s_w[k0] = wk;
        if (blockIdx.x == 0) {
            if (p_out) p_out[k0] = p;
            if (w_out) w_out[k0] = wk;
        }
    }
    __syncthreads();
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    const float t = __fmul_rn(u0[b], s_c[kProfileBins]);
    int k = 0;
#pragma unroll
    for (int step = kProfileBins / 2; step > 0; step >>= 1)
        if (s_c[k + step] <= t) k += step;              // k + step <= 63
    const float f = fminf(__fdiv_rn(__fsub_rn(t, s_c[k]), s_p[k]), 0x1.fffffep-1f);
    const float below = __uint_as_float(__float_as_uint(__fmul_rn((float)(k + 1), 0.015625f)) - 1u);      // nextafterf((k + 1) / 64, 0)
    u[b] = fminf(__fmul_rn(__fadd_rn((float)k, f), 0.015625f), below);
    w[b] = s_w[k];
}

// ---- dynamic thresholding (Saharia et al. 2022, Imagen, section 2.3); an extension, no reference call site.
// The UNCLIPPED data prediction of one element: x_from_out of the conditional output, and when guided the extrapolation of sampler_step_kernel
// without its three clips (a prediction clipped at +-1 before the extrapolation would defeat the threshold).  Guidance is defined in eps space,
// e = (1 + w) e_c + (-w) e_u and x_raw = x_from_eps(z, e); eps_from_x and x_from_eps are affine in x and inverse to each other and the weights sum
// to 1, so that is x_raw = (1 + w) x_c + (-w) x_u, which is what is evaluated.  The round trip itself cancels in fp32 at low SNR: at logsnr -20
// it forms z - e d2 with e d2 = z - O(4e-5) and multiplies by d1 = 2e4, a relative error of 1e-3 in x_raw against 1e-7 here (float64 restatement).
// The one definition behind dyn_threshold_kernel's keys and the DT instantiations of the two update kernels: the same bits in both.
__device__ __forceinline__ float x_raw_from_out(float out, float out_u, bool guided, float w, float zz, const LogsnrCoef& c, int mt) {
    float xr = x_from_out(out, zz, c, mt);
    if (guided) xr = (1.0f + w) * xr + (-w) * x_from_out(out_u, zz, c, mt);
    return xr;
}
// x-hat = clamp(x_raw, -s, s) / s, a true division: with s = 1 this is clip1's bits
__device__ __forceinline__ float threshold_x(float xr, float s) { return fminf(fmaxf(xr, -s), s) / s; }

// The network's next time vector, written by one thread per row of a (gx, B) grid.  In the sampler loop u_t(i - 1) = u_s(i)
// (gaussian_diffusion.py:288-290), so this step's logsnr_s IS the next logsnr_t; with `z_dup` the guided sampler's 2B-row vector takes it twice.
__device__ __forceinline__ void write_logsnr_next(float* __restrict__ logsnr_next, const float* z_dup, int b, float l) {
    if (logsnr_next && blockIdx.x == 0 && threadIdx.x == 0) {
        logsnr_next[b] = l;
        if (z_dup) logsnr_next[gridDim.y + b] = l;
    }
}

// x-hat and eps-hat of element j, the one definition behind both update kernels.  Static clip: the clipped prediction, and with `vu` classifier-
// free guidance in eps space between two clips (:176-186).  DT: the raw (guided) prediction clamped to the row's threshold s = thr[b] and divided by it.
template <bool DT>
__device__ __forceinline__ void predict_x_eps(float out, const float* __restrict__ vu, int64_t j, float w, float zz, const LogsnrCoef& c, int mt,
                                              float s, float& xh, float& eh) {
    if (DT) {
        xh = threshold_x(x_raw_from_out(out, vu ? vu[j] : 0.f, vu != nullptr, w, zz, c, mt), s);
        eh = c.c1 * (zz - xh * c.c2);
    } else {
        xh = clip1(x_from_out(out, zz, c, mt));
        eh = c.c1 * (zz - xh * c.c2);
        if (vu) {
            const float xu = clip1(x_from_out(vu[j], zz, c, mt));
            const float eu = c.c1 * (zz - xu * c.c2);
            const float e = (1.0f + w) * eh + (-w) * eu;
            xh = clip1(c.d1 * (zz - e * c.d2));
            eh = c.c1 * (zz - xh * c.c2);
        }
    }
}

// ---- DDNM restoration (Wang, Yu & Zhang 2023, "Zero-Shot Image Restoration Using Denoising Diffusion Null-Space Model", eq. 13-14, without
// noise); an extension, no reference call site.  The operator A is a box mean over NCHW images: cf in {1, C} channels times an N x N spatial
// box, k = cf N^2 members; box g = (c', i, j) holds the elements (c' cf + dc, i N + dy, j N + dx), and the low-resolution layout is
// [B][C / cf][H / N][W / N].  A+ replicates a box's value over its members, so A A+ = I and x + A+(y - A x) projects onto {x : A x = y}.
// i / d for i < 2^31 by one 32 x 32 -> 64-bit multiply and a shift: with s = ceil(log2 d), sh = 31 + s and M = ceil(2^sh / d) (< 2^32),
// M d = 2^sh + e with 0 <= e < d <= 2^s, so i M / 2^sh = i / d + i e / (d 2^sh) and i e < 2^sh: the floor is floor(i / d).  The host forms (M, sh).
struct FastDiv {
    uint32_t M, sh;
};
__device__ __forceinline__ uint32_t fast_div(uint32_t i, FastDiv f) { return (uint32_t)(((uint64_t)i * f.M) >> f.sh); }

struct BoxGeom {
    uint32_t C, H, W, cf, N;
    uint32_t HW, Hb, Wb, n_box;          // H W, H / N, W / N, (C / cf) Hb Wb
    FastDiv by_HW, by_W, by_N;           // the update kernels' divisions, per element
};

// the box of element i (< C H W < 2^31) of an image
__device__ __forceinline__ uint32_t box_of(uint32_t i, const BoxGeom& g) {
    const uint32_t ch = fast_div(i, g.by_HW), rem = i - ch * g.HW;
    const uint32_t y = fast_div(rem, g.by_W), x = rem - y * g.W;
    return ((g.cf == 1 ? ch : 0u) * g.Hb + fast_div(y, g.by_N)) * g.Wb + fast_div(x, g.by_N);      // cf is 1 or C: c' = ch or 0
}

// grid (ceil(n_box / 256), B), one thread per box.  mean = fdiv(s, (float)k), s the sequential fp32 add, from 0, of the box's members in
// row-major (dc, dy, dx) order: single rounded operations in a fixed order, so the same call gives the same bits.
// RES = false (gmk_box_mean): the members are x's, out = mean.
// RES = true (gmk_box_residual): the members are the x-hat predict_x_eps<false> forms for (v, vu, w, z, lt, mt) - the step kernels' own device
// function, hence their bits - and out = fsub(obs, mean).  v, z (and vu) are read once.
template <bool RES>
__global__ __launch_bounds__(256) void box_kernel(const float* __restrict__ v, const float* __restrict__ vu, const float* __restrict__ cond_w,
                                                  const float* __restrict__ z, const float* __restrict__ obs, float lt, int mt,
                                                  float* __restrict__ out, BoxGeom g) {
    const int b = blockIdx.y;
    const uint32_t box = blockIdx.x * 256 + threadIdx.x;
    if (box >= g.n_box) return;
    const uint32_t j = box % g.Wb, t = box / g.Wb, i = t % g.Hb, cp = t / g.Hb;
    LogsnrCoef c = {};
    float w = 0.f;
    if constexpr (RES) {
        c = logsnr_coef(lt);
        w = cond_w ? cond_w[b] : 0.f;
    }
    const int64_t base = (int64_t)b * g.C * g.HW;
    float s = 0.f;
    for (uint32_t dc = 0; dc < g.cf; ++dc)
        for (uint32_t dy = 0; dy < g.N; ++dy) {
            const int64_t row = base + (int64_t)(cp * g.cf + dc) * g.HW + (i * g.N + dy) * g.W + j * g.N;
            for (uint32_t dx = 0; dx < g.N; ++dx) {
                float xh;
                if constexpr (RES) {
                    float eh;
                    predict_x_eps<false>(v[row + dx], vu, row + dx, w, z[row + dx], c, mt, 1.0f, xh, eh);
                } else {
                    xh = v[row + dx];
                }
                s = __fadd_rn(s, xh);
            }
        }
    const float mean = __fdiv_rn(s, (float)(g.cf * g.N * g.N));
    const int64_t o = (int64_t)b * g.n_box + box;
    out[o] = RES ? __fsub_rn(obs[o], mean) : mean;
}

// NS (gmk_sampler_step_ns / gmk_dpm_solver_step_ns): x-hat' = fadd(x-hat, res[b][box of the element]) - with res = gmk_box_residual's output
// that is x-hat + A+(obs - A x-hat), DDNM's projection - and eps-hat = c1 (z - x-hat' c2).  x-hat' is NOT clipped again (a second clip would
// break A x-hat' = obs; it lies in [-3, 3]); everything after it uses x-hat'.
template <bool NS>
__device__ __forceinline__ void null_space_fix(const float* __restrict__ res, const BoxGeom& g, int b, int64_t i, float zz, const LogsnrCoef& c,
                                               float& xh, float& eh) {
    if constexpr (NS) {
        xh = __fadd_rn(xh, res[(int64_t)b * g.n_box + box_of((uint32_t)i, g)]);
        eh = c.c1 * (zz - xh * c.c2);
    }
}

// grid (ceil(n/256), B).  DT (gmk_sampler_step_dt): x-hat is the raw prediction clamped to thr[b] and divided by it instead of the static clip;
// everything after x-hat is shared.  The DT = false instantiation is the kernel gmk_sampler_step and gmk_ddim_step_vec have always launched.
// NS (gmk_sampler_step_ns): `null_space_fix` after the static clip.
template <bool DT, bool NS = false>
__global__ __launch_bounds__(256) void sampler_step_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                          const float* __restrict__ cond_w, const float* __restrict__ z,
                                                          const float* __restrict__ noise, float lt, float ls, int is_last,
                                                          float* __restrict__ z_next, float* __restrict__ x_pred,
                                                          float* __restrict__ eps_pred, int64_t n,
                                                          const float* __restrict__ lt_vec, const float* __restrict__ ls_vec, int mt,
                                                          float* __restrict__ z_dup = nullptr, float* __restrict__ logsnr_next = nullptr,
                                                          const float* __restrict__ thr = nullptr, const float* __restrict__ res = nullptr,
                                                          BoxGeom geom = BoxGeom{}) {
    const int b = blockIdx.y;
    if (lt_vec) { lt = lt_vec[b]; ls = ls_vec[b]; }      // per-sample times (teacher steps of the distillation loss)
    write_logsnr_next(logsnr_next, z_dup, b, ls);
    const LogsnrCoef c = logsnr_coef(lt);
    const float alpha_s = sqrtf(1.0f / (1.0f + expf(-ls)));
    const float sigma_s = sqrtf(1.0f / (1.0f + expf(ls)));
    // ancestral posterior q(z_s | z_t, x) with x_logvar = 'large' (diffusion_utils.py:36-50)
    const float alpha_st = sqrtf((1.0f + expf(-lt)) / (1.0f + expf(-ls)));
    const float r = expf(lt - ls);
    const float omr = -expm1f(lt - ls);
    const float stdv = sqrtf(omr * (1.0f / (1.0f + expf(lt))));
    const float w = cond_w ? cond_w[b] : 0.f;
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float zz = z[base + i];
        float xh, eh;
        predict_x_eps<DT>(v[base + i], vu, base + i, w, zz, c, mt, DT ? thr[b] : 1.0f, xh, eh);
        null_space_fix<NS>(res, geom, b, i, zz, c, xh, eh);
        float zs;
        if (noise) zs = (r * alpha_st * zz + omr * alpha_s * xh) + stdv * noise[base + i];   // :242
        else zs = alpha_s * xh + sigma_s * eh;                                                 // :212
        z_next[base + i] = is_last ? xh : zs;                                                  // :292
        if (z_dup) z_dup[base + i] = is_last ? xh : zs;      // second half of the guided sampler's 2B-image batch (cond + uncond share z)
        if (x_pred) x_pred[base + i] = xh;
        if (eps_pred) eps_pred[base + i] = eh;
    }
}

// grid (ceil(n/256), B): one DPM-Solver++(2M) step (Lu et al. 2022, Algorithm 2, data prediction) on the DDIM time grid.  x-hat / eps-hat
// and the guidance exactly as sampler_step_kernel forms them; then D = (1 + k) x_hat - k x_prev (k = 1 / 2r, 0 on the first step: x_prev
// is then not read) and z_s = c_z z + c_x D with c_z = sigma_s / sigma_t, c_x = -alpha_s expm1(-h), all three from the host.  x_hist
// holds the previous step's x-hat on entry and this step's on exit (same element, same thread).  An extension: no reference call site.
// DT (gmk_dpm_solver_step_dt): x-hat by the dynamic threshold thr[b], as in sampler_step_kernel<true>.  NS (gmk_dpm_solver_step_ns): as there.
template <bool DT, bool NS = false>
__global__ __launch_bounds__(256) void dpm_solver_step_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                             const float* __restrict__ cond_w, const float* __restrict__ z,
                                                             float* __restrict__ x_hist, float lt, float ls, float c_z, float c_x,
                                                             float k_prev, int is_last, float* __restrict__ z_next,
                                                             float* __restrict__ x_pred, float* __restrict__ eps_pred,
                                                             float* __restrict__ z_dup, float* __restrict__ logsnr_next, int64_t n,
                                                             int mt, const float* __restrict__ thr, const float* __restrict__ res = nullptr,
                                                             BoxGeom geom = BoxGeom{}) {
    const int b = blockIdx.y;
    write_logsnr_next(logsnr_next, z_dup, b, ls);
    const LogsnrCoef c = logsnr_coef(lt);
    const float w = cond_w ? cond_w[b] : 0.f;
    const bool second_order = k_prev != 0.0f;            // uniform across the launch
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float zz = z[base + i];
        float xh, eh;
        predict_x_eps<DT>(v[base + i], vu, base + i, w, zz, c, mt, DT ? thr[b] : 1.0f, xh, eh);
        null_space_fix<NS>(res, geom, b, i, zz, c, xh, eh);
        const float d = second_order ? (1.0f + k_prev) * xh - k_prev * x_hist[base + i] : xh;
        const float zs = c_z * zz + c_x * d;
        x_hist[base + i] = xh;
        z_next[base + i] = is_last ? xh : zs;
        if (z_dup) z_dup[base + i] = is_last ? xh : zs;
        if (x_pred) x_pred[base + i] = xh;
        if (eps_pred) eps_pred[base + i] = eh;
    }
}

// ---- the per-image threshold of dynamic thresholding: an exact order-statistic selection in LDS.
// s[b] = max(1, q), q the p-quantile of |x_raw[b]| by torch.quantile's linear rule: q = a[lo] + frac (a[hi] - a[lo]) in fp32, a = |x_raw[b]| sorted
// ascending, lo = k_lo, hi = min(lo + 1, n - 1) (k_lo and frac from the host, in double).  a[lo] and a[hi] are exact order statistics.
//
// One workgroup of 256 threads per image.  key = bits(x_raw) & 0x7fffffff: non-negative floats order as unsigned integers, so the k-th
// smallest key is the k-th smallest |x_raw|.  The keys of an image of n <= kDynKeys values are formed once (one read of v, v_uncond and z)
// and stay in LDS; a larger image re-forms them from global memory in every pass.  Selection is an MSB-first radix select, four 8-bit
// digits: each pass counts, among the keys that share the digits decided so far, the next digit's 256 values (integer LDS atomics into one
// histogram per wave: integer adds commute, so the counts do not depend on timing), scans the counts and narrows to the bin that holds rank
// k_lo.  After the last pass the prefix IS a[lo], and the workgroup knows how many keys lie below it and how many equal it; a[hi] = a[lo]
// when hi == lo or at least k_lo + 2 keys are <= a[lo], else the smallest key above a[lo] (one more pass, an integer LDS min).  No floating-
// point atomics; every loop's trip count depends on n alone, whatever the values (NaNs and infinities are keys like any other).
// LDS: 48 KiB of keys + 4 KiB of histograms + 84 B = 53,332 B per workgroup, so three workgroups (12 waves) share a CU's 160 KiB.
constexpr int kDynKeys = GMK_DYN_THRESHOLD_KEYS;      // LDS-resident keys per image: covers 3 x 64 x 64

// inclusive sum over the 16 lanes of a DPP row (row_shr:1, 2, 4, 8; a lane the shift leaves without a source adds 0)
__device__ __forceinline__ uint32_t row_scan16(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
    return v;
}

__global__ __launch_bounds__(256) void dyn_threshold_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                           const float* __restrict__ cond_w, const float* __restrict__ z, float lt,
                                                           uint32_t k_lo, float frac, float* __restrict__ s_out, float* __restrict__ q_out,
                                                           uint32_t n, int mt) {
    __shared__ __attribute__((aligned(16))) uint32_t keys[kDynKeys];
    __shared__ uint32_t hist[4][256];
    __shared__ uint32_t rowtot[16];
    __shared__ uint32_t sel[4];          // the chosen bin: digit, rank inside it, keys below it, keys in it
    __shared__ uint32_t min_above;
    const int b = blockIdx.x;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const LogsnrCoef c = logsnr_coef(lt);
    const float w = cond_w ? cond_w[b] : 0.f;
    const bool guided = vu != nullptr;
    const bool in_lds = n <= (uint32_t)kDynKeys;
    const bool vec = (n & 3) == 0;       // every row then starts 16-byte aligned
    const int64_t base = (int64_t)b * n;
    auto key_of = [&](float o, float ou, float zz) {
        return __builtin_bit_cast(uint32_t, x_raw_from_out(o, ou, guided, w, zz, c, mt)) & 0x7fffffffu;
    };
    auto key1 = [&](uint32_t i) { return key_of(v[base + i], guided ? vu[base + i] : 0.f, z[base + i]); };
    auto key4 = [&](uint32_t i, uint32_t (&k)[4]) {
        float ov[4], uv[4] = {0.f, 0.f, 0.f, 0.f}, zv[4];
        load4(v + base + i, ov);
        load4(z + base + i, zv);
        if (guided) load4(vu + base + i, uv);
#pragma unroll
        for (int j = 0; j < 4; ++j) k[j] = key_of(ov[j], uv[j], zv[j]);
    };
    // f(key) for every key of the image, from LDS or re-formed from global memory
    auto for_keys = [&](auto&& f) {
        if (in_lds) {
            for (uint32_t i = tid; i < n; i += 256) f(keys[i]);
        } else if (vec) {
            for (uint32_t i = tid * 4; i < n; i += 1024) {
                uint32_t k[4];
                key4(i, k);
#pragma unroll
                for (int j = 0; j < 4; ++j) f(k[j]);
            }
        } else {
            for (uint32_t i = tid; i < n; i += 256) f(key1(i));
        }
    };
    if (tid == 0) min_above = 0xffffffffu;
    if (in_lds) {
        if (vec) {
            for (uint32_t i = tid * 4; i < n; i += 1024) {
                uint32_t k[4];
                key4(i, k);
                *reinterpret_cast<uint4*>(&keys[i]) = make_uint4(k[0], k[1], k[2], k[3]);
            }
        } else {
            for (uint32_t i = tid; i < n; i += 256) keys[i] = key1(i);
        }
    }
    uint32_t prefix = 0;                 // the digits of a[lo] decided so far
    uint32_t rank = k_lo;                // a[lo]'s rank among the keys that share them
    uint32_t below = 0, equal = 0;       // keys below the prefix's range / inside the last chosen bin
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const int shift = 24 - 8 * p;
#pragma unroll
        for (int k = 0; k < 4; ++k) hist[k][tid] = 0;
        __syncthreads();                 // also: the keys are in LDS (p == 0), the last pass's `sel` has been read
        for_keys([&](uint32_t key) {
            if ((uint32_t)((uint64_t)key >> (shift + 8)) == prefix) atomicAdd(&hist[wave][(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        const uint32_t cnt = (hist[0][tid] + hist[1][tid]) + (hist[2][tid] + hist[3][tid]);      // thread t owns digit value t
        const uint32_t inc = row_scan16(cnt);
        if ((tid & 15) == 15) rowtot[tid >> 4] = inc;
        __syncthreads();
        uint32_t before = 0;             // keys in the rows of bins before this thread's
#pragma unroll
        for (uint32_t r = 0; r < 16; ++r) before += r < (tid >> 4) ? rowtot[r] : 0u;
        const uint32_t excl = before + inc - cnt;
        if (excl <= rank && rank < excl + cnt) {      // exactly one thread: the counts sum to the keys that share the prefix, rank is below that
            sel[0] = tid; sel[1] = rank - excl; sel[2] = excl; sel[3] = cnt;
        }
        __syncthreads();
        prefix = (prefix << 8) | sel[0];
        rank = sel[1];
        below += sel[2];
        equal = sel[3];
    }
    // the smallest key above a[lo] (0xffffffff when there is none: then it is not used)
    uint32_t m = 0xffffffffu;
    for_keys([&](uint32_t key) { m = (key > prefix && key < m) ? key : m; });
    atomicMin(&min_above, m);
    __syncthreads();
    if (tid == 0) {
        const bool hi_is_lo = k_lo == n - 1 || below + equal >= k_lo + 2;
        const float a_lo = __builtin_bit_cast(float, prefix);
        const float a_hi = __builtin_bit_cast(float, hi_is_lo ? prefix : min_above);
        const float q = __fadd_rn(a_lo, __fmul_rn(frac, __fsub_rn(a_hi, a_lo)));
        s_out[b] = fmaxf(1.0f, q);
        if (q_out) q_out[b] = q;
    }
}

// ---- RePaint inpainting (Lugmayr et al. 2022, Algorithm 1, jump length 1); an extension, no reference call site.
// The four normals gmk_rng_normal(seed, .) writes at Philox counter `ctr`: rng_kernel<true>'s Box-Muller, the same operations in the same
// order (the library builds with -ffp-contract=off), so a draw made here equals the one a separate gmk_rng_normal launch would store.
__device__ __forceinline__ void philox_normal4(uint64_t ctr, uint64_t seed, float (&o)[4]) {
    uint32_t rnd[4];
    philox4x32(ctr, seed, rnd);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float u1 = 1.0f - u01(rnd[2 * k]);
        const float u2 = u01(rnd[2 * k + 1]);
        const float rad = sqrtf(-2.0f * logf(u1));
        float s, cs;
        sincosf(6.283185307179586f * u2, &s, &cs);
        o[2 * k] = rad * cs; o[2 * k + 1] = rad * s;
    }
}

// grid (ceil(n/1024), B), in place after the sampler update of step t -> s has written z (RePaint Algorithm 1):
//   known = is_last ? x0 : alpha_s x0 + sigma_s eps1;  z = m ? known : z   (a select: where m == 0, z keeps its bits)
//   renoise: z = a z + b eps2, a = alpha_t / alpha_s, b = sqrt(1 - alpha_t^2 / alpha_s^2)   (q(z_t | z_s): back to time t)
// eps1 / eps2 are Philox normals drawn here and never stored: element j of this chunk (j = b n + i) takes counter ctr1 + j / 4 (eps1) and
// ctr2 + j / 4 (eps2), component j % 4.  eps1 is only formed for groups of four with a known pixel (and never when is_last), eps2 only when
// renoise; x0 is only read where a group has a known pixel.  n % 4 == 0: every group of four lies in one row and starts 16-byte aligned.
__global__ __launch_bounds__(256) void inpaint_merge_kernel(float* __restrict__ z, const float* __restrict__ x0,
                                                           const uint8_t* __restrict__ mask, float alpha_s, float sigma_s, float a,
                                                           float b, int is_last, int renoise, float l_next, uint64_t seed,
                                                           uint64_t ctr1, uint64_t ctr2, float* __restrict__ z_dup,
                                                           float* __restrict__ logsnr_next, int64_t n) {
    const int row = blockIdx.y;
    write_logsnr_next(logsnr_next, z_dup, row, l_next);
    const int64_t base = (int64_t)row * n;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        const int64_t j = base + i;
        const uint64_t q = (uint64_t)(j >> 2);
        float zv[4];
        load4(z + j, zv);
        const uchar4 m4 = *reinterpret_cast<const uchar4*>(mask + j);
        const uint8_t m[4] = {m4.x, m4.y, m4.z, m4.w};
        if (m4.x | m4.y | m4.z | m4.w) {
            float xv[4], known[4];
            load4(x0 + j, xv);
            if (is_last) {
#pragma unroll
                for (int k = 0; k < 4; ++k) known[k] = xv[k];
            } else {
                float e[4];
                philox_normal4(ctr1 + q, seed, e);
#pragma unroll
                for (int k = 0; k < 4; ++k) known[k] = alpha_s * xv[k] + sigma_s * e[k];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) zv[k] = m[k] ? known[k] : zv[k];
        }
        if (renoise) {
            float e[4];
            philox_normal4(ctr2 + q, seed, e);
#pragma unroll
            for (int k = 0; k < 4; ++k) zv[k] = a * zv[k] + b * e[k];
        }
        store4(z + j, zv);
        if (z_dup) store4(z_dup + j, zv);
    }
}

// ---- multistep consistency sampling (Song et al. 2023, "Consistency Models", Algorithm 1); an extension, no reference call site.
// grid (ceil(n/1024), B): x-hat / eps-hat and the guidance exactly as sampler_step_kernel forms them (predict_x_eps), then
//   z_next = is_last ? x-hat : alpha_s x-hat + sigma_s eps      (a product, a product, a sum: nothing contracted)
// eps are Philox normals drawn here and never stored: element j of this chunk (j = b n + i) takes counter ctr + j / 4, component j % 4 - what
// gmk_rng_normal(seed, ctr) would store at j.  Not drawn when is_last.  n % 4 == 0: every group of four lies in one row and starts 16-byte
// aligned.  alpha_s, sigma_s come from the host (double, rounded to fp32).
__global__ __launch_bounds__(256) void consistency_step_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                              const float* __restrict__ cond_w, const float* __restrict__ z, float lt, float ls,
                                                              float alpha_s, float sigma_s, int is_last, uint64_t seed, uint64_t ctr,
                                                              float* __restrict__ z_next, float* __restrict__ x_pred,
                                                              float* __restrict__ eps_pred, float* __restrict__ z_dup,
                                                              float* __restrict__ logsnr_next, int64_t n, int mt) {
    const int b = blockIdx.y;
    write_logsnr_next(logsnr_next, z_dup, b, ls);
    const LogsnrCoef c = logsnr_coef(lt);
    const float w = cond_w ? cond_w[b] : 0.f;
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        const int64_t j = base + i;
        float vv[4], zv[4], xh[4], eh[4], zs[4];
        load4(v + j, vv);
        load4(z + j, zv);
#pragma unroll
        for (int k = 0; k < 4; ++k) predict_x_eps<false>(vv[k], vu, j + k, w, zv[k], c, mt, 1.0f, xh[k], eh[k]);
        if (is_last) {
#pragma unroll
            for (int k = 0; k < 4; ++k) zs[k] = xh[k];
        } else {
            float e[4];
            philox_normal4(ctr + (uint64_t)(j >> 2), seed, e);
#pragma unroll
            for (int k = 0; k < 4; ++k) zs[k] = __fadd_rn(__fmul_rn(alpha_s, xh[k]), __fmul_rn(sigma_s, e[k]));
        }
        store4(z_next + j, zs);
        if (z_dup) store4(z_dup + j, zs);
        if (x_pred) store4(x_pred + j, xh);
        if (eps_pred) store4(eps_pred + j, eh);
    }
}

// ---- the stochastic samplers (gmk_stochastic_step): the ancestral posterior of diffusion_utils.py:34-62 with x_logvar 'small' / 'large' /
// 'medium:<frac>', DDIM with eta > 0 (Song et al. 2021, eq. 12 and 16) and SDE-DPM-Solver++(2M) (Lu et al. 2022) are one update, linear in what
// the step kernels already hold; the host (`stochastic_coefs`) forms the four coefficients in double.
// grid (ceil(n/1024), B), consistency_step_kernel's shape: x-hat / eps-hat and the guidance exactly as sampler_step_kernel forms them
// (predict_x_eps<DT>; DT: the row's threshold thr[b]), then
//   d      = k != 0 ? fsub(fmul(1 + k, x-hat), fmul(k, x_prev)) : x-hat                  (x_prev = x_hist on entry; not read when k == 0)
//   z_next = is_last ? x-hat : fadd(fadd(fmul(c_z, z), fmul(c_x, d)), fmul(c_n, xi))     (every operation singly rounded)
// xi are Philox normals drawn here and never stored, by consistency_step_kernel's convention: element j = b n + i takes counter ctr + j / 4,
// component j % 4.  Not drawn when is_last or c_n == 0 (xi = 0 then).  x_hist (nullable) takes this step's x-hat from the thread that read it.
template <bool DT>
__global__ __launch_bounds__(256) void stochastic_step_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                             const float* __restrict__ cond_w, const float* __restrict__ z,
                                                             float* __restrict__ x_hist, const float* __restrict__ thr, float lt, float ls,
                                                             float c_z, float c_x, float c_n, float k_prev, int is_last, uint64_t seed,
                                                             uint64_t ctr, float* __restrict__ z_next, float* __restrict__ x_pred,
                                                             float* __restrict__ eps_pred, float* __restrict__ z_dup,
                                                             float* __restrict__ logsnr_next, int64_t n, int mt) {
    const int b = blockIdx.y;
    write_logsnr_next(logsnr_next, z_dup, b, ls);
    const LogsnrCoef c = logsnr_coef(lt);
    const float w = cond_w ? cond_w[b] : 0.f;
    const float s = DT ? thr[b] : 1.0f;
    const bool second_order = k_prev != 0.0f;            // uniform across the launch, and then x_hist is there (the entry checks)
    const bool draw = !is_last && c_n != 0.0f;
    const float k1 = 1.0f + k_prev;
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        const int64_t j = base + i;
        float vv[4], zv[4], xh[4], eh[4], d[4], zs[4];
        load4(v + j, vv);
        load4(z + j, zv);
#pragma unroll
        for (int k = 0; k < 4; ++k) predict_x_eps<DT>(vv[k], vu, j + k, w, zv[k], c, mt, s, xh[k], eh[k]);
        if (second_order) {
            float xp[4];
            load4(x_hist + j, xp);
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = __fsub_rn(__fmul_rn(k1, xh[k]), __fmul_rn(k_prev, xp[k]));
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) d[k] = xh[k];
        }
        if (is_last) {
#pragma unroll
            for (int k = 0; k < 4; ++k) zs[k] = xh[k];
        } else {
            float e[4] = {0.f, 0.f, 0.f, 0.f};
            if (draw) philox_normal4(ctr + (uint64_t)(j >> 2), seed, e);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                zs[k] = __fadd_rn(__fadd_rn(__fmul_rn(c_z, zv[k]), __fmul_rn(c_x, d[k])), __fmul_rn(c_n, e[k]));
        }
        if (x_hist) store4(x_hist + j, xh);
        store4(z_next + j, zs);
        if (z_dup) store4(z_dup + j, zs);
        if (x_pred) store4(x_pred + j, xh);
        if (eps_pred) store4(eps_pred + j, eh);
    }
}

// ---- the ancestral step under a learned variance (gmk_stochastic_step_lv; Nichol & Dhariwal 2021, section 3.1): stochastic_step_kernel for kind
// 'ancestral' (k_prev = 0, no x_hist) with a noise multiplier per element,
//   c_n_i = fmul(c_n_small, exp(fmul(f_i, half_delta))),  f_i = fmul(0.5, fadd(nu_i, 1)),
// 'medium:f_i' of diffusion_reverse in the form coef_noise_small e^(f D / 2).  nu = -1 gives f = 0, exp(0) = 1 and c_n_i = c_n_small: the
// bits of stochastic_step_kernel under 'small'.  Same grid, same x-hat, same Philox counters; nu is not read on the last step.
template <bool DT>
__global__ __launch_bounds__(256) void stochastic_step_lv_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                                const float* __restrict__ cond_w, const float* __restrict__ z,
                                                                const float* __restrict__ nu, const float* __restrict__ thr, float lt, float ls,
                                                                float c_z, float c_x, float c_n_small, float half_delta, int is_last,
                                                                uint64_t seed, uint64_t ctr, float* __restrict__ z_next,
                                                                float* __restrict__ x_pred, float* __restrict__ eps_pred,
                                                                float* __restrict__ z_dup, float* __restrict__ logsnr_next, int64_t n, int mt) {
    const int b = blockIdx.y;
    write_logsnr_next(logsnr_next, z_dup, b, ls);
    const LogsnrCoef c = logsnr_coef(lt);
    const float w = cond_w ? cond_w[b] : 0.f;
    const float s = DT ? thr[b] : 1.0f;
    const bool draw = !is_last && c_n_small != 0.0f;
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        const int64_t j = base + i;
        float vv[4], zv[4], xh[4], eh[4], zs[4];
        load4(v + j, vv);
        load4(z + j, zv);
#pragma unroll
        for (int k = 0; k < 4; ++k) predict_x_eps<DT>(vv[k], vu, j + k, w, zv[k], c, mt, s, xh[k], eh[k]);
        if (is_last) {
#pragma unroll
            for (int k = 0; k < 4; ++k) zs[k] = xh[k];
        } else {
            float e[4] = {0.f, 0.f, 0.f, 0.f}, nv[4] = {-1.f, -1.f, -1.f, -1.f};
            if (draw) {
                philox_normal4(ctr + (uint64_t)(j >> 2), seed, e);
                load4(nu + j, nv);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float cn = __fmul_rn(c_n_small, expf(__fmul_rn(__fmul_rn(0.5f, __fadd_rn(nv[k], 1.0f)), half_delta)));
                zs[k] = __fadd_rn(__fadd_rn(__fmul_rn(c_z, zv[k]), __fmul_rn(c_x, xh[k])), __fmul_rn(cn, e[k]));
            }
        }
        store4(z_next + j, zs);
        if (z_dup) store4(z_dup + j, zs);
        if (x_pred) store4(x_pred + j, xh);
        if (eps_pred) store4(eps_pred + j, eh);
    }
}

// ---- continuous-time variational bound (Kingma et al. 2021, VDM eq. 17 with lambda as the variable); an extension, no reference call site.
// Every kernel below takes any n: 16-byte vector accesses when n % 4 == 0 (every row then starts 16-byte aligned), element by element otherwise.

// grid (ceil(n/1024), B): z = alpha x + sigma eps at a given per-sample logsnr (q_sample_kernel draws its logsnr from u instead)
__global__ __launch_bounds__(256) void q_sample_logsnr_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                             const float* __restrict__ logsnr, float* __restrict__ z, int64_t n) {
    const int b = blockIdx.y;
    const LogsnrCoef c = logsnr_coef(logsnr[b]);
    const int64_t base = (int64_t)b * n;
    auto elem = [&](float xv, float ev) { return __fadd_rn(__fmul_rn(xv, c.alpha), __fmul_rn(c.sigma, ev)); };
    if ((n & 3) == 0) {
        for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
            float xv[4], ev[4], o[4];
            load4(x + base + i, xv);
            load4(eps + base + i, ev);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = elem(xv[k], ev[k]);
            store4(z + base + i, o);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
            z[base + i] = elem(x[base + i], eps[base + i]);
    }
}

// the network's noise prediction, UNCLIPPED: 'v' sigma z + alpha out, 'eps' out, 'x' (z - alpha out) / sigma in predict_eps_from_x's form
__device__ __forceinline__ float eps_from_out(float out, float zz, const LogsnrCoef& c, int mt) {
    return mt == GMK_MEAN_V ? c.sigma * zz + c.alpha * out : (mt == GMK_MEAN_EPS ? out : c.c1 * (zz - out * c.c2));
}

// one block per sample: acc[b] += weight[b] * sum_i (eps - eps_hat)^2 (one read pass, v_loss_kernel's reduction: a fixed order, so
// repeated calls give the same bits)
__global__ __launch_bounds__(256) void vlb_term_kernel(const float* __restrict__ out, const float* __restrict__ z,
                                                      const float* __restrict__ eps, const float* __restrict__ logsnr,
                                                      const float* __restrict__ weight, float* __restrict__ acc, int64_t n, int mt) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const LogsnrCoef c = logsnr_coef(logsnr[b]);
    const int64_t base = (int64_t)b * n;
    float s = 0.f;
    auto elem = [&](float o, float zz, float e) {
        const float d = e - eps_from_out(o, zz, c, mt);
        s = fmaf(d, d, s);
    };
    if ((n & 3) == 0) {
        for (int64_t i = threadIdx.x * 4; i < n; i += 1024) {
            float ov[4], zv[4], ev[4];
            load4(out + base + i, ov);
            load4(z + base + i, zv);
            load4(eps + base + i, ev);
#pragma unroll
            for (int k = 0; k < 4; ++k) elem(ov[k], zv[k], ev[k]);
        }
    } else {
        for (int64_t i = threadIdx.x; i < n; i += 256) elem(out[base + i], z[base + i], eps[base + i]);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) acc[b] += weight[b] * s;
}

// log(1 - Phi(t)) = log(erfc(t / sqrt 2) / 2): erfcf while it is representable, the asymptotic series (Abramowitz & Stegun 26.2.12, four terms:
// the next is below 3e-7 relative from t = 9) beyond; -inf at t = +inf
__device__ __forceinline__ float log_ndtr_upper(float t) {
    if (t < 9.0f) return logf(0.5f * erfcf(t * 0.70710678118654752f));
    const float r = 1.0f / (t * t);
    return -0.5f * t * t - logf(t) - 0.91893853320467274f + log1pf(r * (-1.0f + r * (3.0f + r * (-15.0f + r * 105.0f))));
}

// log(Phi(a) - Phi(b)) for a > b (a may be +inf, b -inf): the bin's mass as a difference of the smaller tail probabilities, so that it never
// rounds to log 0 when the bin lies far out in one tail, and as log1p of the two tails when it straddles 0
__device__ __forceinline__ float log_bin_mass(float a, float b) {
    if (b > 0.0f) {
        const float la = log_ndtr_upper(a), lb = log_ndtr_upper(b);
        return lb + log1pf(-expf(la - lb));
    }
    if (a < 0.0f) {
        const float la = log_ndtr_upper(-a), lb = log_ndtr_upper(-b);
        return la + log1pf(-expf(lb - la));
    }
    return log1pf(-0.5f * erfcf(a * 0.70710678118654752f) - 0.5f * erfcf(-b * 0.70710678118654752f));
}

// one block per sample: the prior term sum_i KL(N(alpha_1 x, sigma_1^2) || N(0, 1)) = half_a2 sum x^2 + n prior_c (the x-free part in double on
// the host: it cancels in fp32), and the decoder term sum_i -log[Phi((x + delta - m) / s) - Phi((x - delta - m) / s)] with m = z_0 / alpha_0,
// s = sigma_0 / alpha_0, z_0 = alpha_0 x + sigma_0 eps_0.  Then (x - m) / s = -eps_0 exactly, so the standardised edges are +-delta/s - eps_0
// (dscale = delta / s): z_0 is never formed, whose rounding (ulp(x) / s) would swamp the edges.  The top bin (x > hi - delta) has upper edge +inf,
// the bottom bin (x < lo + delta) lower edge -inf.
__global__ __launch_bounds__(256) void vlb_endpoints_kernel(const float* __restrict__ x, const float* __restrict__ eps0, float delta,
                                                           float dscale, float lo, float hi, float half_a2, float prior_c,
                                                           float* __restrict__ out_prior, float* __restrict__ out_dec, int64_t n) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const int64_t base = (int64_t)b * n;
    float sx = 0.f, sd = 0.f;
    auto elem = [&](float xv, float e) {
        sx = fmaf(xv, xv, sx);
        const float a = xv > hi - delta ? INFINITY : dscale - e;
        const float bb = xv < lo + delta ? -INFINITY : -dscale - e;
        // both edges 12 standard deviations out: the bin's mass is 1 - O(1e-33), its -log 0 in fp32.  Every normal draw at lambda_max = 20
        // takes this branch (the edges are +-delta e^10 = +-86 from -eps_0), which keeps the pass at memory speed instead of two erfcf
        if (a >= 12.0f && bb <= -12.0f) return;
        sd -= log_bin_mass(a, bb);
    };
    if ((n & 3) == 0) {
        for (int64_t i = threadIdx.x * 4; i < n; i += 1024) {
            float xv[4], ev[4];
            load4(x + base + i, xv);
            load4(eps0 + base + i, ev);
#pragma unroll
            for (int k = 0; k < 4; ++k) elem(xv[k], ev[k]);
        }
    } else {
        for (int64_t i = threadIdx.x; i < n; i += 256) elem(x[base + i], eps0[base + i]);
    }
    sx = block_sum(sx, red);
    sd = block_sum(sd, red);
    if (threadIdx.x == 0) {
        out_prior[b] = half_a2 * sx + prior_c * (float)n;
        out_dec[b] = sd;
    }
}

template <bool NORMAL>
__global__ __launch_bounds__(256) void rng_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
    const int64_t nq = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        uint32_t rnd[4];
        philox4x32(offset + (uint64_t)q, seed, rnd);
        float o[4];
        if (NORMAL) {   // Box-Muller on two pairs
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float u1 = 1.0f - u01(rnd[2 * k]);          // (0, 1]
                const float u2 = u01(rnd[2 * k + 1]);
                const float rad = sqrtf(-2.0f * logf(u1));
                float s, cs;
                sincosf(6.283185307179586f * u2, &s, &cs);
                o[2 * k] = rad * cs; o[2 * k + 1] = rad * s;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = u01(rnd[k]);
        }
        const int64_t i = q * 4;
        if (i + 3 < n) store4(out + i, o);
        else for (int k = 0; i + k < n; ++k) out[i + k] = o[k];
    }
}

// One Adam update of one element: the single definition behind every adam_kernel instantiation, so they produce the same bits for
// p, m and v (the library builds with -ffp-contract=off; a second copy of these lines would still be a second place for them to drift).
__device__ __forceinline__ void adam_elem(float& p, float g, float& m, float& v, float step_size, float beta1, float beta2, float eps,
                                          float inv_bc2_sqrt, float grad_scale) {
    const float gg = g * grad_scale;
    m = m + (gg - m) * (1.0f - beta1);             // exp_avg.lerp_(grad, 1 - beta1)
    v = v * beta2 + (1.0f - beta2) * gg * gg;      // exp_avg_sq.mul_(b2).addcmul_(g, g, 1 - b2)
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    p = p - step_size * (m / denom);
}

// ema.lerp_(p, w) with torch.lerp's two forms: start + w (end - start) below w = 0.5, end - (end - start)(1 - w) from 0.5 up, so w = 1
// gives end exactly and w = 0 gives start exactly.  Each form is one fused multiply-add (one rounding), as torch's device lerp is compiled;
// w is uniform across the launch: no divergence.
__device__ __forceinline__ float lerp_to(float start, float end, float w) {
    const float diff = end - start;
    return w < 0.5f ? fmaf(w, diff, start) : fmaf(-diff, 1.0f - w, end);
}

// The Adam step behind gmk_adam_step, gmk_adam_ema_step, gmk_adam_step_ctl and gmk_adam_pema_step.
// EMA: Adam, then the EMA of the updated weights in the same pass: ema = lerp(ema, p_new, ema_w).  p is read once, so the EMA costs its own
// read and write only (36 B / parameter against Adam's 28).
// CTL: steered by gmk_grad_norm's state (below): gg = (g grad_scale) coef (adam_elem then multiplies by 1: exact), and no memory is touched
// when apply == 0.  Both values are uniform across the launch.  Without CTL adam_elem forms g grad_scale itself and `state` is not read.
// NP > 0 (gmk_adam_pema_step): NP more averages of the updated weights, the rows of one [NP][stride] arena, row r = lerp(row r, p_new, w[r]):
// 8 B / parameter each, the row loop unrolled.  PVEC: the rows take 16-byte accesses (base aligned, stride % 4 == 0), else scalar ones.
struct PemaArgs {
    float* rows;
    int64_t stride;
    float w[3];
};

template <bool EMA, bool CTL, int NP = 0, bool PVEC = true>
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                  float* __restrict__ v, float* __restrict__ ema, const float* __restrict__ state,
                                                  int64_t n, float step_size, float beta1, float beta2, float eps, float inv_bc2_sqrt,
                                                  float grad_scale, float ema_w, PemaArgs pa) {
    if (CTL && state[GMK_APPLY] == 0.0f) return;
    const float coef = CTL ? state[GMK_CLIP_COEF] : 1.0f;
    auto elem = [&](float& pp, float gk, float& mm, float& vv) {
        adam_elem(pp, CTL ? (gk * grad_scale) * coef : gk, mm, vv, step_size, beta1, beta2, eps, inv_bc2_sqrt, CTL ? 1.0f : grad_scale);
    };
    const int64_t nq = n / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        float pv[4], gv[4], mv[4], vv[4], ev[4], rv[NP ? NP : 1][4];
        load4(p + q * 4, pv); load4(g + q * 4, gv); load4(m + q * 4, mv); load4(v + q * 4, vv);
        if (EMA) load4(ema + q * 4, ev);
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            float* row = pa.rows + r * pa.stride + q * 4;
            if (PVEC) load4(row, rv[r]);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) rv[r][k] = row[k];
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            elem(pv[k], gv[k], mv[k], vv[k]);
            if (EMA) ev[k] = lerp_to(ev[k], pv[k], ema_w);
#pragma unroll
            for (int r = 0; r < NP; ++r) rv[r][k] = lerp_to(rv[r][k], pv[k], pa.w[r]);
        }
        store4(p + q * 4, pv); store4(m + q * 4, mv); store4(v + q * 4, vv);
        if (EMA) store4(ema + q * 4, ev);
#pragma unroll
        for (int r = 0; r < NP; ++r) {
            float* row = pa.rows + r * pa.stride + q * 4;
            if (PVEC) store4(row, rv[r]);
            else {
#pragma unroll
                for (int k = 0; k < 4; ++k) row[k] = rv[r][k];
            }
        }
    }
    // tail (n not a multiple of 4)
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const int64_t i = nq * 4 + threadIdx.x;
        float pp = p[i], mm = m[i], vv = v[i];
        elem(pp, g[i], mm, vv);
        m[i] = mm; v[i] = vv; p[i] = pp;
        if (EMA) ema[i] = lerp_to(ema[i], pp, ema_w);
#pragma unroll
        for (int r = 0; r < NP; ++r) pa.rows[r * pa.stride + i] = lerp_to(pa.rows[r * pa.stride + i], pp, pa.w[r]);
    }
}

// out[i] = fp32(sum_k coef[k] src[k][i]) in double, k in index order, every product and every sum rounded on its own (gmk_arena_combine).
// VEC: one float4 of each row per thread, 16-byte accesses (bases aligned, stride % 4 == 0) and a scalar tail; else one element per thread.
// coef is uniform across the launch: scalar loads.
template <bool VEC>
__global__ __launch_bounds__(256) void arena_combine_kernel(const float* __restrict__ src, int64_t stride, const double* __restrict__ coef, int K,
                                                           float* __restrict__ out, int64_t n) {
    auto one = [&](int64_t i) {
        double acc = __dmul_rn(coef[0], (double)src[i]);
        for (int k = 1; k < K; ++k) acc = __dadd_rn(acc, __dmul_rn(coef[k], (double)src[k * stride + i]));
        out[i] = (float)acc;
    };
    if (!VEC) {
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) one(i);
        return;
    }
    const int64_t nq = n / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        float xv[4];
        double acc[4];
        load4(src + q * 4, xv);
        const double c0 = coef[0];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __dmul_rn(c0, (double)xv[j]);
#pragma unroll 4
        for (int k = 1; k < K; ++k) {
            load4(src + k * stride + q * 4, xv);
            const double c = coef[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = __dadd_rn(acc[j], __dmul_rn(c, (double)xv[j]));
        }
        float o[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = (float)acc[j];
        store4(out + q * 4, o);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) one(nq * 4 + threadIdx.x);
}

// ---- steered optimiser step: global gradient norm, clipping and the non-finite guard without a host sync; an extension (the reference's
// guard is GradScaler.step's, diffusion_model.py:71; it has no clipping).
// Stage 1: workgroup b owns float4s [b * kNormQuads, (b + 1) * kNormQuads) of g and writes their sum of squares to part[b]: kNormLoads 16-byte
// loads per thread, all issued before the first is used.  The grid follows from n alone (never from the CU limit) and every sum has a fixed
// order, so the bits are the same on every call and on every rank.  Longest chain of fp32 additions behind part[b]: kNormLoads per component
// accumulator, 2 to join the four, 1 for the n & 3 tail (workgroup 0), 6 + 2 in block_sum.
constexpr int kNormLoads = 8;
constexpr int kNormQuads = 256 * kNormLoads;

__global__ __launch_bounds__(256) void grad_norm_partial_kernel(const float* __restrict__ g, float* __restrict__ part, int64_t n) {
    __shared__ float red[4];
    const int64_t nq = n / 4;
    const int64_t q0 = (int64_t)blockIdx.x * kNormQuads + threadIdx.x;
    float gv[kNormLoads][4];
#pragma unroll
    for (int k = 0; k < kNormLoads; ++k) {
        const int64_t q = q0 + k * 256;
        if (q < nq) load4(g + q * 4, gv[k]);
        else gv[k][0] = gv[k][1] = gv[k][2] = gv[k][3] = 0.f;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < kNormLoads; ++k)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[c] = fmaf(gv[k][c], gv[k][c], acc[c]);
    float s = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float t = g[nq * 4 + threadIdx.x];
        s = fmaf(t, t, s);
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// Stage 2, one workgroup: thread t adds part[t], part[t + 256], ... in that order (ceil(nparts / 256) additions), then block_sum (6 + 2).
// state: [0] total_norm = grad_scale sqrt(sum), [1] coef = min(1, max_norm / (total_norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; 1 when
// max_norm <= 0), [2] apply = 1 if total_norm is finite (a NaN or inf gradient, or a sum of squares beyond fp32, gives 0), [3] skipped, the
// running count of apply == 0.
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const float* __restrict__ part, int nparts, float grad_scale, float max_norm,
                                                             float* __restrict__ state) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < nparts; i += 256) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) {
        const float total = grad_scale * sqrtf(s);
        const bool finite = isfinite(total);
        state[GMK_GRAD_NORM] = total;
        state[GMK_CLIP_COEF] = max_norm > 0.0f ? fminf(1.0f, max_norm / (total + 1e-6f)) : 1.0f;
        state[GMK_APPLY] = finite ? 1.0f : 0.0f;
        state[GMK_SKIPPED] = state[GMK_SKIPPED] + (finite ? 0.0f : 1.0f);
    }
}

// ---- probability-flow ODE (Song et al. 2021, section 4.3 and App. D.2, in lambda = logsnr); an extension, no reference call site.
// Probes and dequantisation noise use gmk_rng_uniform's counters: element i is component i % 4 of Philox counter offset + i / 4, so the
// host can replay them with a plain uniform draw.
__global__ __launch_bounds__(256) void rng_rademacher_kernel(float* __restrict__ out, int64_t n, uint64_t seed, uint64_t offset) {
    const int64_t nq = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        uint32_t rnd[4];
        philox4x32(offset + (uint64_t)q, seed, rnd);
        float o[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = u01(rnd[k]) >= 0.5f ? 1.0f : -1.0f;
        const int64_t i = q * 4;
        if (i + 3 < n) store4(out + i, o);
        else for (int k = 0; i + k < n; ++k) out[i + k] = o[k];
    }
}

// y = x + delta (2 u - 1): uniform dequantisation inside the bin of half-width delta; u is never stored
__global__ __launch_bounds__(256) void dequantize_kernel(const float* __restrict__ x, float* __restrict__ y, float delta, int64_t n,
                                                        uint64_t seed, uint64_t offset) {
    const int64_t nq = (n + 3) / 4;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (int64_t)gridDim.x * blockDim.x) {
        uint32_t rnd[4];
        philox4x32(offset + (uint64_t)q, seed, rnd);
        const int64_t i = q * 4;
        if (i + 3 < n) {
            float xv[4], o[4];
            load4(x + i, xv);
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = xv[k] + delta * (2.0f * u01(rnd[k]) - 1.0f);
            store4(y + i, o);
        } else {
            for (int k = 0; i + k < n; ++k) y[i + k] = x[i + k] + delta * (2.0f * u01(rnd[k]) - 1.0f);
        }
    }
}

// grid (gx, B); gx = 1 whenever acc or prior is given (one workgroup per image, vlb_term_kernel's fixed-order reduction).  Per element:
// x_hat / eps_hat of the network output at (z, logsnr_i), both unclipped; z = alpha_j x_hat + sigma_j eps_hat in place when `update`;
// x_hat to x_out when given.  Per image: acc += div_a + div_b sum r g (the weighted divergence) and prior = 1/2 sum z^2 + prior_c.
// z is read and written by the same thread (no __restrict__ on it: the prior reads the values the update overwrites - never both in one launch).
__global__ __launch_bounds__(256) void pf_ode_step_kernel(const float* __restrict__ out, float* z, const float* __restrict__ r,
                                                         const float* __restrict__ g, float* __restrict__ acc, float* __restrict__ prior,
                                                         float* __restrict__ x_out, float li, float lj, int update, float div_a,
                                                         float div_b, float prior_c, int64_t n, int mt) {
    __shared__ float red[4];
    const int b = blockIdx.y;
    const LogsnrCoef c = logsnr_coef(li);
    const LogsnrCoef cj = logsnr_coef(lj);
    const bool div = acc != nullptr, pri = prior != nullptr;
    const int64_t base = (int64_t)b * n;
    float srg = 0.f, szz = 0.f;
    auto elem = [&](float o, float zz, float& xh, float& zj) {      // -> x_hat and the updated z
        if (pri) szz = fmaf(zz, zz, szz);
        xh = x_from_out(o, zz, c, mt);
        const float eh = eps_from_out(o, zz, c, mt);
        zj = cj.alpha * xh + cj.sigma * eh;
    };
    if ((n & 3) == 0) {
        for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
            float ov[4], zv[4], xh[4];
            load4(out + base + i, ov);
            load4(z + base + i, zv);
            if (div) {
                float rv[4], gv[4];
                load4(r + base + i, rv);
                load4(g + base + i, gv);
#pragma unroll
                for (int k = 0; k < 4; ++k) srg = fmaf(rv[k], gv[k], srg);
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) elem(ov[k], zv[k], xh[k], zv[k]);
            if (update) store4(z + base + i, zv);
            if (x_out) store4(x_out + base + i, xh);
        }
    } else {
        for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
            if (div) srg = fmaf(r[base + i], g[base + i], srg);
            float xh, zj;
            elem(out[base + i], z[base + i], xh, zj);
            if (update) z[base + i] = zj;
            if (x_out) x_out[base + i] = xh;
        }
    }
    if (div) {
        srg = block_sum(srg, red);
        if (threadIdx.x == 0) acc[b] += div_a + div_b * srg;
    }
    if (pri) {
        szz = block_sum(szz, red);
        if (threadIdx.x == 0) prior[b] = 0.5f * szz + prior_c;
    }
}

// ---- spherical interpolation of latent codes (gmk_slerp; Shoemake 1985, as the DDIM paper's section 5.3 / App. D.5 uses it on x_T); an
// extension, no reference call site.  Per image b, over its n values, in fp32:
//   dot = sum a b, na = sum a^2, nb = sum b^2;  c = clamp(dot / sqrt(na nb), -1, 1), theta = acosf(c), s = sinf(theta)
//   out[k] = w_a a + w_b b,  w_a = sinf((1 - t_k) theta) / s,  w_b = sinf(t_k theta) / s          for every k < K
//   where s < 1e-6 or c is not finite (parallel, antipodal and all-zero rows): w_a = 1 - t_k, w_b = t_k, the lerp - no division, so finite
//   inputs never give a NaN.
// t_k = 0 gives w_a = s / s = 1 and w_b = sinf(0) / s = 0, hence a's values exactly (t_k = 1: b's); the division is IEEE's and the library builds
// with -ffp-contract=off, so nothing here is fused or reordered.  The clamp is written with comparisons: a NaN stays a NaN (fminf / fmaxf would
// drop it) and reaches cos_out as one.
// One workgroup of 256 threads per image, thread t takes elements 4t .. 4t + 3 of every 1024 (16-byte loads and stores, n % 4 == 0).  Each thread
// adds its products in ascending order with fmaf, then block_sum: a fixed order and no floating-point atomics, so the same call gives the same
// bits.  GROUPS > 0: the image has at most 1024 GROUPS values and stays in registers between the reduction and the K output passes (4 GROUPS
// values of a and of b per thread: 96 of the kernel's 114 registers at the capacity kSlerpKeep = 1024 x 12, four waves per SIMD, no scratch), so
// a and b come from HBM once.  GROUPS == 0: any n, a and b are read again for every k.  (A second resident instantiation with GROUPS = 4 for
// n <= 4096, 74 registers, measured 37.7 - 37.9 us against this one's 38.6 at B = 2048, n = 3072, K = 8: not kept.)
constexpr int kSlerpKeep = GMK_SLERP_KEEP;    // kDynKeys, kXLossKeep: covers 3 x 64 x 64

template <int GROUPS>
__global__ __launch_bounds__(256) void slerp_kernel(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ t,
                                                   float* __restrict__ out, float* __restrict__ cos_out, int B, int64_t n, int K) {
    __shared__ float red[4];
    const int img = blockIdx.x;
    const int64_t base = (int64_t)img * n;
    const int64_t i0 = (int64_t)threadIdx.x * 4;
    constexpr int G = GROUPS > 0 ? GROUPS : 1;
    float ra[G][4], rb[G][4];
    float dot = 0.f, na = 0.f, nb = 0.f;
    auto sums = [&](const float (&av)[4], const float (&bv)[4]) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            dot = fmaf(av[j], bv[j], dot);
            na = fmaf(av[j], av[j], na);
            nb = fmaf(bv[j], bv[j], nb);
        }
    };
    if constexpr (GROUPS > 0) {
#pragma unroll
        for (int g = 0; g < GROUPS; ++g) {
            const int64_t i = i0 + (int64_t)g * 1024;
            if (i < n) {
                load4(a + base + i, ra[g]);
                load4(b + base + i, rb[g]);
                sums(ra[g], rb[g]);
            }
        }
    } else {
        for (int64_t i = i0; i < n; i += 1024) {
            load4(a + base + i, ra[0]);
            load4(b + base + i, rb[0]);
            sums(ra[0], rb[0]);
        }
    }
    dot = block_sum(dot, red);
    na = block_sum(na, red);
    nb = block_sum(nb, red);
    const float q = dot / sqrtf(na * nb);
    const float c = q < -1.0f ? -1.0f : (q > 1.0f ? 1.0f : q);
    const float theta = acosf(c);
    const float s = sinf(theta);
    const bool lerp = !(isfinite(c) && s >= 1e-6f);
    if (threadIdx.x == 0 && cos_out) cos_out[img] = c;
    for (int k = 0; k < K; ++k) {
        const float tk = t[k];
        const float wa = lerp ? 1.0f - tk : sinf((1.0f - tk) * theta) / s;
        const float wb = lerp ? tk : sinf(tk * theta) / s;
        float* __restrict__ o = out + ((int64_t)k * B + img) * n;
        auto mix = [&](const float (&av)[4], const float (&bv)[4], int64_t i) {
            float ov[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) ov[j] = wa * av[j] + wb * bv[j];
            store4(o + i, ov);
        };
        if constexpr (GROUPS > 0) {
#pragma unroll
            for (int g = 0; g < GROUPS; ++g) {
                const int64_t i = i0 + (int64_t)g * 1024;
                if (i < n) mix(ra[g], rb[g], i);
            }
        } else {
            for (int64_t i = i0; i < n; i += 1024) {
                load4(a + base + i, ra[0]);
                load4(b + base + i, rb[0]);
                mix(ra[0], rb[0], i);
            }
        }
    }
}

// ---- the rescale factor of classifier-free guidance (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section
// 3.4), which the samplers apply on the steps inside the guidance interval (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval
// Improves Sample and Distribution Quality in Diffusion Models"); an extension, no reference call site.  Per image b, in fp32, with
// x_c = x_raw_from_out(unguided) and x_raw = x_raw_from_out(guided, w_b) - dyn_threshold_kernel's device function, hence its bits, no clip:
//   m_c = (sum x_c) / n, m_r = (sum x_raw) / n;  q_c = sum (x_c - m_c)^2, q_r = sum (x_raw - m_r)^2      (two passes, centred squares)
//   ratio = sqrtf(q_c / q_r) = std(x_c) / std(x_raw);  f = fadd(1, fmul(phi, fsub(ratio, 1)));  thr = 1 / f (a true division)
//   thr = 1 where q_r == 0, f is not finite or f <= 0.
// threshold_x(x, thr) = clamp(x, -thr, thr) / thr = clip(f x, -1, 1) for f > 0, so the _dt update kernels called with this thr are the rescaled update.
// One workgroup of 256 threads per image.  Every one of the four sums is accumulated with ONE element-to-thread assignment and order: thread t
// takes the elements t, t + 256, ... ascending (a plain add for the means, d d + q as fmaf for the squares), then block_sum: per chain
// ceil(n / 256) additions + 6 (wave_sum) + 2.  No floating-point atomics, a fixed order: the same call gives the same bits, a row depends on its
// own image alone, and w_b = 0 (x_raw = 1 x_c + (-0) x_u: x_c's value) gives q_r == q_c bit for bit, hence ratio = 1, f = 1, thr = 1 exactly.
// VEC: the loads are 16 bytes wide - thread t forms x_c and x_raw of the elements 4t .. 4t + 3 of a chunk of 1024 and stores them to LDS (8 KiB
// of staging), then reads the chunk's elements t + 256 k (k < 4) back: the assignment above.  Without VEC thread t loads those elements itself.
// KEEP: the image has at most kRescaleKeep = 12 x 1024 values and both predictions stay in registers between the passes (48 + 48 values per
// thread), so v, v_uncond and z come from HBM once: 12 n bytes per image.  Without KEEP any n: the second pass forms them again (24 n bytes).
constexpr int kRescaleKeep = GMK_CFG_RESCALE_KEEP;    // kDynKeys, kXLossKeep, kSlerpKeep: covers 3 x 64 x 64
static_assert(kRescaleKeep % 1024 == 0, "whole chunks of 1024");

template <bool VEC, bool KEEP>
__global__ __launch_bounds__(256) void cfg_rescale_kernel(const float* __restrict__ v, const float* __restrict__ vu,
                                                         const float* __restrict__ cond_w, const float* __restrict__ z, float lt, float phi,
                                                         float* __restrict__ thr_out, float* __restrict__ ratio_out, int64_t n, int mt) {
    __shared__ __attribute__((aligned(16))) float stage_c[1024];
    __shared__ __attribute__((aligned(16))) float stage_r[1024];
    __shared__ float red[4];
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const LogsnrCoef c = logsnr_coef(lt);
    const float w = cond_w[b];
    const int64_t base = (int64_t)b * n;
    constexpr int CH = KEEP ? kRescaleKeep / 1024 : 1;
    float xc[CH][4], xr[CH][4];
    // x_c and x_raw of the elements c0 + tid + 256 k (k < 4) of the image; an entry whose element lies beyond n is not written (or holds stale
    // LDS) and is never read.  c0 < n is the same in every thread, so the barriers are reached by all of them.
    auto chunk = [&](int64_t c0, float (&oc)[4], float (&orw)[4]) {
        if constexpr (VEC) {
            __syncthreads();             // the staging's last values have been read
            const int64_t i = c0 + tid * 4;
            if (i < n) {                 // n % 4 == 0: the whole group lies inside the image
                float ov[4], uv[4], zv[4], a[4], r[4];
                load4(v + base + i, ov);
                load4(vu + base + i, uv);
                load4(z + base + i, zv);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    a[k] = x_raw_from_out(ov[k], 0.f, false, w, zv[k], c, mt);
                    r[k] = x_raw_from_out(ov[k], uv[k], true, w, zv[k], c, mt);
                }
                store4(stage_c + tid * 4, a);
                store4(stage_r + tid * 4, r);
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                oc[k] = stage_c[tid + 256 * k];
                orw[k] = stage_r[tid + 256 * k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int64_t i = c0 + tid + 256 * k;
                if (i < n) {
                    const float o = v[base + i], zz = z[base + i];
                    oc[k] = x_raw_from_out(o, 0.f, false, w, zz, c, mt);
                    orw[k] = x_raw_from_out(o, vu[base + i], true, w, zz, c, mt);
                }
            }
        }
    };
    // f(x_c, x_raw) for every element of this thread, in ascending order; `load`: form the chunk (else: it is in the registers)
    auto for_elements = [&](bool load, auto&& f) {
        if constexpr (KEEP) {
#pragma unroll
            for (int ch = 0; ch < CH; ++ch) {
                const int64_t c0 = (int64_t)ch * 1024;
                if (c0 < n) {
                    if (load) chunk(c0, xc[ch], xr[ch]);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c0 + tid + 256 * k < n) f(xc[ch][k], xr[ch][k]);
                }
            }
        } else {
            for (int64_t c0 = 0; c0 < n; c0 += 1024) {
                chunk(c0, xc[0], xr[0]);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c0 + tid + 256 * k < n) f(xc[0][k], xr[0][k]);
            }
        }
    };
    float sc = 0.f, sr = 0.f;
    for_elements(true, [&](float a, float r) {
        sc = __fadd_rn(sc, a);
        sr = __fadd_rn(sr, r);
    });
    sc = block_sum(sc, red);
    sr = block_sum(sr, red);
    const float mc = __fdiv_rn(sc, (float)n), mr = __fdiv_rn(sr, (float)n);
    float qc = 0.f, qr = 0.f;
    for_elements(!KEEP, [&](float a, float r) {
        const float dc = __fsub_rn(a, mc), dr = __fsub_rn(r, mr);
        qc = fmaf(dc, dc, qc);
        qr = fmaf(dr, dr, qr);
    });
    qc = block_sum(qc, red);
    qr = block_sum(qr, red);
    if (tid == 0) {
        const float ratio = sqrtf(__fdiv_rn(qc, qr));
        const float f = __fadd_rn(1.0f, __fmul_rn(phi, __fsub_rn(ratio, 1.0f)));
        thr_out[b] = (qr == 0.0f || !isfinite(f) || f <= 0.0f) ? 1.0f : __fdiv_rn(1.0f, f);
        if (ratio_out) ratio_out[b] = ratio;
    }
}

// blocks per row of a (gx, B) grid whose blocks take `per_block` elements per pass: enough for the row, at most 64
int row_grid(int64_t n, int per_block) {
    const int64_t g = (n + per_block - 1) / per_block;
    return (int)(g > 64 ? 64 : g);
}

int stream_grid(int64_t work_items) {
    int64_t g = (work_items + 255) / 256;
    return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g));
}

// 16-byte accesses need every row to start on a 16-byte boundary: n a multiple of 4 and aligned tensors (a null pointer is not accessed)
template <typename... T> static bool rows_aligned16(int64_t n, const T*... ptrs) {
    return n % 4 == 0 && ((reinterpret_cast<uintptr_t>(ptrs) | ...) & 15) == 0;
}

// the dynamic LDS of a loss kernel that keeps `arrays` kinds of residual: each min(n, kXLossKeep) floats rounded up to 4, then block_sum's four partials
struct LossLds { int floats; size_t bytes; };
static LossLds loss_lds(int64_t n, int arrays) {
    const int64_t m = n < kXLossKeep ? n : kXLossKeep;
    const int floats = (int)((m + 3) / 4 * 4);
    return {floats, (size_t)(arrays * floats + 4) * sizeof(float)};
}

// a[i] += b[i] over n elements, n % 8 == 0, 16-byte (bf16) / 32-byte (fp32) accesses: the sum of the two heads' data gradients (gmk_add_into)
template <typename T>
__global__ __launch_bounds__(256) void add_into_kernel(T* __restrict__ a, const T* __restrict__ b, int64_t n) {
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8; i < n; i += (int64_t)gridDim.x * 2048) {
        float x[8], y[8];
        load8(a + i, x);
        load8(b + i, y);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] += y[k];
        store8(a + i, x);
    }
}

}  // namespace

extern "C" int gmk_add_into(void* a, const void* b, int64_t n, int dtype, void* stream) {
    GMK_REQUIRE(a && b, "gmk_add_into: null pointer");
    GMK_REQUIRE(n > 0 && n % 8 == 0, "gmk_add_into: n = %lld (a positive multiple of 8 required)", (long long)n);
    GMK_REQUIRE(dtype == GMK_F32 || dtype == GMK_BF16, "gmk_add_into: dtype must be GMK_F32 or GMK_BF16 (the gradient types)");
    const int grid = stream_grid(n / 8);
    if (dtype == GMK_F32) add_into_kernel<float><<<grid, 256, 0, gmk_stream(stream)>>>((float*)a, (const float*)b, n);
    else add_into_kernel<bf16_t><<<grid, 256, 0, gmk_stream(stream)>>>((bf16_t*)a, (const bf16_t*)b, n);
    return gmk_check_launch("gmk_add_into");
}

extern "C" int gmk_rng_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    GMK_REQUIRE(out && n > 0, "gmk_rng_normal: bad arguments");
    rng_kernel<true><<<stream_grid((n + 3) / 4), 256, 0, gmk_stream(stream)>>>(out, n, seed, offset);
    return gmk_check_launch("gmk_rng_normal");
}

extern "C" int gmk_rng_uniform(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    GMK_REQUIRE(out && n > 0, "gmk_rng_uniform: bad arguments");
    rng_kernel<false><<<stream_grid((n + 3) / 4), 256, 0, gmk_stream(stream)>>>(out, n, seed, offset);
    return gmk_check_launch("gmk_rng_uniform");
}

extern "C" int gmk_q_sample(const float* x, const float* eps, const float* u, float* logsnr, float* z, int B, int64_t n,
                            void* stream) {
    GMK_REQUIRE(x && eps && u && logsnr && z, "gmk_q_sample: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0 && n % 4 == 0, "gmk_q_sample: bad shape B=%d n=%lld (n %% 4 == 0 required)", B,
                (long long)n);
    const int gx = row_grid(n, 1024);
    q_sample_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(x, eps, u, logsnr, z, n, GMK_SCHED_COSINE, kSchedA, kSchedB, 0.f, 0.f, 0.f);
    return gmk_check_launch("gmk_q_sample");
}

#define GMK_REQUIRE_SCHED(kind, a, b, lmin, lmax, shift, who)                                                                      \
    do {                                                                                                                           \
        GMK_REQUIRE((kind) >= GMK_SCHED_COSINE && (kind) <= GMK_SCHED_BETA_LINEAR,                                                 \
                    who ": kind = %d, must be 0 (cosine), 1 (uniform), 2 (beta_const) or 3 (beta_linear)", (int)(kind));           \
        GMK_REQUIRE(isfinite(a) && isfinite(b) && isfinite(lmin) && isfinite(lmax) && isfinite(shift), who ": non-finite schedule argument"); \
    } while (0)

extern "C" int gmk_q_sample_sched(const float* x, const float* eps, const float* u, float* logsnr, float* z, int B, int64_t n, int kind,
                                  float a, float b, float lmin, float lmax, float shift, void* stream) {
    GMK_REQUIRE(x && eps && u && logsnr && z, "gmk_q_sample_sched: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0, "gmk_q_sample_sched: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE_SCHED(kind, a, b, lmin, lmax, shift, "gmk_q_sample_sched");
    const int gx = row_grid(n, 1024);
    q_sample_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(x, eps, u, logsnr, z, n, kind, a, b, lmin, lmax, shift);
    return gmk_check_launch("gmk_q_sample_sched");
}

extern "C" int gmk_v_loss(const float* v, const float* z, const float* x, const float* eps, const float* logsnr,
                          float* loss_b, float* x_mse, float* eps_mse, float* dv, float grad_scale, int loss_type,
                          int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && x && eps && logsnr && loss_b, "gmk_v_loss: null pointer");
    GMK_REQUIRE(B > 0 && n > 0, "gmk_v_loss: bad shape");
    GMK_REQUIRE(loss_type == 0 || loss_type == 1, "gmk_v_loss: loss_type must be 0 (snr_trunc) or 1 (snr)");
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_v_loss");
    v_loss_kernel<<<B, 256, 0, gmk_stream(stream)>>>(v, z, x, eps, logsnr, loss_b, x_mse, eps_mse, dv, grad_scale, n, loss_type, mean_type);
    return gmk_check_launch("gmk_v_loss");
}

extern "C" int gmk_x_loss_w(const float* v, const float* z, const float* x, const float* logsnr, float* loss_b, float* x_mse, float* dv,
                            float grad_scale, int weight_type, float gamma, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && x && logsnr && loss_b && x_mse, "gmk_x_loss_w: null pointer");
    GMK_REQUIRE(B > 0 && n > 0, "gmk_x_loss_w: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE(weight_type == GMK_LOSS_W_SNR_PLUS1 || weight_type == GMK_LOSS_W_MIN_SNR,
                "gmk_x_loss_w: weight_type must be 0 (snr_plus1) or 1 (min_snr)");
    GMK_REQUIRE(isfinite(gamma) && gamma > 0.0f, "gmk_x_loss_w: gamma = %g, need a finite value > 0", (double)gamma);
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_x_loss_w");
    const LossLds lds = loss_lds(n, 1);
    if (rows_aligned16(n, v, z, x, dv)) x_loss_w_kernel<true><<<B, 256, lds.bytes, gmk_stream(stream)>>>(v, z, x, logsnr, loss_b, x_mse, dv, grad_scale, weight_type, gamma, n, mean_type, lds.floats);
    else x_loss_w_kernel<false><<<B, 256, lds.bytes, gmk_stream(stream)>>>(v, z, x, logsnr, loss_b, x_mse, dv, grad_scale, weight_type, gamma, n, mean_type, lds.floats);
    return gmk_check_launch("gmk_x_loss_w");
}

extern "C" int gmk_x_loss_huber(const float* v, const float* z, const float* x, const float* logsnr, float* loss_b, float* x_mse, float* dv,
                                float grad_scale, float c, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && x && logsnr && loss_b && x_mse, "gmk_x_loss_huber: null pointer");
    GMK_REQUIRE(B > 0 && n > 0, "gmk_x_loss_huber: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE(isfinite(c) && c > 0.0f, "gmk_x_loss_huber: c = %g, need a finite value > 0", (double)c);
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_x_loss_huber");
    const LossLds lds = loss_lds(n, 1);
    if (rows_aligned16(n, v, z, x, dv)) x_loss_w_kernel<true, true><<<B, 256, lds.bytes, gmk_stream(stream)>>>(v, z, x, logsnr, loss_b, x_mse, dv, grad_scale, 0, c, n, mean_type, lds.floats);
    else x_loss_w_kernel<false, true><<<B, 256, lds.bytes, gmk_stream(stream)>>>(v, z, x, logsnr, loss_b, x_mse, dv, grad_scale, 0, c, n, mean_type, lds.floats);
    return gmk_check_launch("gmk_x_loss_huber");
}

extern "C" int gmk_hybrid_loss(const float* v, const float* nu, const float* z, const float* x, const float* eps, const float* logsnr,
                               const float* logsnr_s, float* loss_b, float* vlb_b, float* frac_b, float* x_mse, float* eps_mse, float* dv,
                               float* dnu, float grad_scale, float lambda, int loss_type, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && nu && z && x && eps && logsnr && logsnr_s && loss_b && vlb_b && frac_b && x_mse && eps_mse, "gmk_hybrid_loss: null pointer");
    GMK_REQUIRE(B > 0 && n > 0, "gmk_hybrid_loss: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE(loss_type == 0 || loss_type == 1, "gmk_hybrid_loss: loss_type must be 0 (snr_trunc) or 1 (snr)");
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_hybrid_loss");
    GMK_REQUIRE(isfinite(lambda) && lambda >= 0.0f, "gmk_hybrid_loss: lambda = %g, need a finite value >= 0", (double)lambda);
    GMK_REQUIRE(!dv == !dnu, "gmk_hybrid_loss: dv and dnu go together");
    const LossLds lds = loss_lds(n, 2);
    if (lds.bytes > 64 * 1024) {      // above what a launch gets unasked: raise the kernels' limit (96 KiB + 16) once on every device that launches them
        constexpr int kLdsMax = (2 * kXLossKeep + 4) * (int)sizeof(float);
        constexpr int kMaxDevices = 64;
        static bool raised[kMaxDevices] = {};
        int device = -1;
        GMK_REQUIRE(hipGetDevice(&device) == hipSuccess && device >= 0 && device < kMaxDevices, "gmk_hybrid_loss: no current device (%d)", device);
        if (!raised[device]) {
            const hipError_t ev = hipFuncSetAttribute((const void*)hybrid_loss_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
            const hipError_t es = hipFuncSetAttribute((const void*)hybrid_loss_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
            GMK_REQUIRE(ev == hipSuccess && es == hipSuccess, "gmk_hybrid_loss: cannot raise the dynamic LDS limit to %d bytes on device %d: %s", kLdsMax,
                        device, hipGetErrorString(ev != hipSuccess ? ev : es));
            raised[device] = true;
        }
    }
    if (rows_aligned16(n, v, nu, z, x, eps, dv, dnu)) hybrid_loss_kernel<true><<<B, 256, lds.bytes, gmk_stream(stream)>>>(v, nu, z, x, eps, logsnr, logsnr_s, loss_b, vlb_b, frac_b, x_mse, eps_mse, dv, dnu, grad_scale, lambda, n, loss_type, mean_type, lds.floats);
    else hybrid_loss_kernel<false><<<B, 256, lds.bytes, gmk_stream(stream)>>>(v, nu, z, x, eps, logsnr, logsnr_s, loss_b, vlb_b, frac_b, x_mse, eps_mse, dv, dnu, grad_scale, lambda, n, loss_type, mean_type, lds.floats);
    return gmk_check_launch("gmk_hybrid_loss");
}

extern "C" int gmk_u_stratified(const float* u0, float* u, int B, void* stream) {
    GMK_REQUIRE(u0 && u, "gmk_u_stratified: null pointer");
    GMK_REQUIRE(B > 0 && B <= (1 << 24), "gmk_u_stratified: B = %d outside [1, 2^24] (b and B must be exact in fp32)", B);
    u_stratified_kernel<<<(B + 255) / 256, 256, 0, gmk_stream(stream)>>>(u0, u, B);
    return gmk_check_launch("gmk_u_stratified");
}

extern "C" int gmk_loss_profile(const float* u, const float* v0, const float* v1, int B, float decay, float* state, void* stream) {
    GMK_REQUIRE(u && v0 && state, "gmk_loss_profile: null pointer");
    GMK_REQUIRE(B > 0 && B <= (1 << 24), "gmk_loss_profile: B = %d outside [1, 2^24] (a bin's count must be exact in fp32)", B);
    GMK_REQUIRE(decay > 0.0f && decay <= 1.0f, "gmk_loss_profile: decay = %g outside (0, 1]", (double)decay);
    loss_profile_kernel<<<1, 256, 0, gmk_stream(stream)>>>(u, v0, v1, B, decay, state);
    return gmk_check_launch("gmk_loss_profile");
}

extern "C" int gmk_u_importance(const float* state, const float* u0, float* u, float* w, int B, float warm, float floor, float* p_out,
                                float* w_out, void* stream) {
    GMK_REQUIRE(state && u0 && u && w, "gmk_u_importance: null pointer");
    GMK_REQUIRE(B > 0 && B <= (1 << 24), "gmk_u_importance: B = %d outside [1, 2^24]", B);
    GMK_REQUIRE(warm >= 0.0f, "gmk_u_importance: warm = %g, need a count >= 0", (double)warm);
    GMK_REQUIRE(floor > 0.0f && floor <= 1.0f, "gmk_u_importance: floor = %g outside (0, 1]", (double)floor);
    u_importance_kernel<<<(B + 255) / 256, 256, 0, gmk_stream(stream)>>>(state, u0, u, w, B, warm, floor, p_out, w_out);
    return gmk_check_launch("gmk_u_importance");
}

// The checks every entry that forms the (guided) prediction shares: the four gmk_*_step* entries, gmk_ddim_step_vec and gmk_dyn_threshold
static int step_args_check(const char* who, int mean_type, const float* v_uncond, const float* cond_w, int B, int64_t n) {
    GMK_REQUIRE(mean_type >= GMK_MEAN_V && mean_type <= GMK_MEAN_X, "%s: mean_type must be 0 (v), 1 (eps) or 2 (x)", who);
    GMK_REQUIRE((v_uncond == nullptr) == (cond_w == nullptr), "%s: v_uncond and cond_w go together", who);
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0, "%s: bad shape", who);
    return 0;
}

// (M, sh) of fast_div for a divisor 1 <= d < 2^31
static FastDiv fast_div_of(uint32_t d) {
    uint32_t s = 0;
    while (((uint32_t)1 << s) < d) ++s;
    const uint32_t sh = 31 + s;
    return FastDiv{(uint32_t)((((uint64_t)1 << sh) + d - 1) / d), sh};
}

// The box-mean operator's geometry (gmk_box_mean, gmk_box_residual and the *_ns entries): cf in {1, C}, N dividing H and W, B n_box < 2^31
static int box_geom_check(const char* who, int B, int C, int H, int W, int cf, int N, BoxGeom* g) {
    GMK_REQUIRE(B > 0 && B < 65536 && C > 0 && H > 0 && W > 0 && (int64_t)C * H * W < ((int64_t)1 << 31),
                "%s: bad shape B=%d C=%d H=%d W=%d (C H W < 2^31)", who, B, C, H, W);
    GMK_REQUIRE(cf == 1 || cf == C, "%s: cf = %d, the channels averaged together: 1 or C = %d", who, cf, C);
    GMK_REQUIRE(N >= 1 && H % N == 0 && W % N == 0, "%s: N = %d does not divide H = %d and W = %d", who, N, H, W);
    const int64_t n_box = (int64_t)(C / cf) * (H / N) * (W / N);
    GMK_REQUIRE((int64_t)B * n_box < ((int64_t)1 << 31), "%s: B n_box = %lld, need < 2^31", who, (long long)((int64_t)B * n_box));
    *g = BoxGeom{(uint32_t)C, (uint32_t)H, (uint32_t)W, (uint32_t)cf, (uint32_t)N, (uint32_t)(H * W), (uint32_t)(H / N), (uint32_t)(W / N),
                 (uint32_t)n_box, fast_div_of((uint32_t)(H * W)), fast_div_of((uint32_t)W), fast_div_of((uint32_t)N)};
    return 0;
}

extern "C" int gmk_box_mean(const float* x, float* out, int B, int C, int H, int W, int cf, int N, void* stream) {
    GMK_REQUIRE(x && out, "gmk_box_mean: null pointer");
    BoxGeom g;
    if (const int err = box_geom_check("gmk_box_mean", B, C, H, W, cf, N, &g)) return err;
    box_kernel<false><<<dim3((g.n_box + 255) / 256, B), 256, 0, gmk_stream(stream)>>>(x, nullptr, nullptr, nullptr, nullptr, 0.f, 0, out, g);
    return gmk_check_launch("gmk_box_mean");
}

extern "C" int gmk_box_residual(const float* v, const float* v_uncond, const float* cond_w, const float* z, const float* obs, float logsnr_t,
                                float* r, int mean_type, int B, int C, int H, int W, int cf, int N, void* stream) {
    GMK_REQUIRE(v && z && obs && r, "gmk_box_residual: null pointer");
    BoxGeom g;
    if (const int err = box_geom_check("gmk_box_residual", B, C, H, W, cf, N, &g)) return err;
    if (const int err = step_args_check("gmk_box_residual", mean_type, v_uncond, cond_w, B, (int64_t)C * H * W)) return err;
    GMK_REQUIRE(isfinite(logsnr_t), "gmk_box_residual: non-finite time");
    box_kernel<true><<<dim3((g.n_box + 255) / 256, B), 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, obs, logsnr_t, mean_type, r, g);
    return gmk_check_launch("gmk_box_residual");
}

// The argument checks and the launch behind gmk_sampler_step / gmk_sampler_step_dt (DT: thr is required) / gmk_sampler_step_ns (NS: res and
// the box geometry)
template <bool DT, bool NS = false>
static int sampler_step_launch(const char* who, const float* v, const float* v_uncond, const float* cond_w, const float* thr, const float* z,
                               const float* noise, float logsnr_t, float logsnr_s, int is_last, float* z_next, float* x_pred,
                               float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream,
                               const float* res = nullptr, BoxGeom geom = BoxGeom{}) {
    GMK_REQUIRE(v && z && z_next && (!DT || thr) && (!NS || res), "%s: null pointer", who);
    if (const int err = step_args_check(who, mean_type, v_uncond, cond_w, B, n)) return err;
    const int gx = row_grid(n, 256);
    sampler_step_kernel<DT, NS><<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, noise, logsnr_t, logsnr_s, is_last, z_next,
                                                                             x_pred, eps_pred, n, nullptr, nullptr, mean_type, z_dup,
                                                                             logsnr_next, thr, res, geom);
    return gmk_check_launch(who);
}

extern "C" int gmk_sampler_step(const float* v, const float* v_uncond, const float* cond_w, const float* z,
                                const float* noise, float logsnr_t, float logsnr_s, int is_last, float* z_next,
                                float* x_pred, float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n,
                                void* stream) {
    return sampler_step_launch<false>("gmk_sampler_step", v, v_uncond, cond_w, nullptr, z, noise, logsnr_t, logsnr_s, is_last, z_next, x_pred,
                                      eps_pred, z_dup, logsnr_next, mean_type, B, n, stream);
}

extern "C" int gmk_sampler_step_dt(const float* v, const float* v_uncond, const float* cond_w, const float* thr, const float* z,
                                   const float* noise, float logsnr_t, float logsnr_s, int is_last, float* z_next, float* x_pred,
                                   float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream) {
    return sampler_step_launch<true>("gmk_sampler_step_dt", v, v_uncond, cond_w, thr, z, noise, logsnr_t, logsnr_s, is_last, z_next, x_pred,
                                     eps_pred, z_dup, logsnr_next, mean_type, B, n, stream);
}

template <bool DT, bool NS = false>
static int dpm_solver_step_launch(const char* who, const float* v, const float* v_uncond, const float* cond_w, const float* thr,
                                  const float* z, float* x_hist, float logsnr_t, float logsnr_s, float coef_z, float coef_x,
                                  float coef_prev, int is_last, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                                  float* logsnr_next, int mean_type, int B, int64_t n, void* stream, const float* res = nullptr,
                                  BoxGeom geom = BoxGeom{}) {
    GMK_REQUIRE(v && z && x_hist && z_next && (!DT || thr) && (!NS || res), "%s: null pointer", who);
    if (const int err = step_args_check(who, mean_type, v_uncond, cond_w, B, n)) return err;
    GMK_REQUIRE(isfinite(logsnr_t) && isfinite(logsnr_s) && isfinite(coef_z) && isfinite(coef_x) && isfinite(coef_prev),
                "%s: non-finite time or coefficient", who);
    const int gx = row_grid(n, 256);
    dpm_solver_step_kernel<DT, NS><<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, x_hist, logsnr_t, logsnr_s, coef_z,
                                                                                coef_x, coef_prev, is_last, z_next, x_pred, eps_pred, z_dup,
                                                                                logsnr_next, n, mean_type, thr, res, geom);
    return gmk_check_launch(who);
}

extern "C" int gmk_dpm_solver_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, float* x_hist,
                                   float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_prev, int is_last,
                                   float* z_next, float* x_pred, float* eps_pred, float* z_dup, float* logsnr_next, int mean_type,
                                   int B, int64_t n, void* stream) {
    return dpm_solver_step_launch<false>("gmk_dpm_solver_step", v, v_uncond, cond_w, nullptr, z, x_hist, logsnr_t, logsnr_s, coef_z, coef_x,
                                         coef_prev, is_last, z_next, x_pred, eps_pred, z_dup, logsnr_next, mean_type, B, n, stream);
}

extern "C" int gmk_dpm_solver_step_dt(const float* v, const float* v_uncond, const float* cond_w, const float* thr, const float* z,
                                      float* x_hist, float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_prev,
                                      int is_last, float* z_next, float* x_pred, float* eps_pred, float* z_dup, float* logsnr_next,
                                      int mean_type, int B, int64_t n, void* stream) {
    return dpm_solver_step_launch<true>("gmk_dpm_solver_step_dt", v, v_uncond, cond_w, thr, z, x_hist, logsnr_t, logsnr_s, coef_z, coef_x,
                                        coef_prev, is_last, z_next, x_pred, eps_pred, z_dup, logsnr_next, mean_type, B, n, stream);
}

// the *_ns entries: the box geometry must describe the rows, n = C H W
static int ns_geom_check(const char* who, int B, int64_t n, int C, int H, int W, int cf, int N, BoxGeom* g) {
    if (const int err = box_geom_check(who, B, C, H, W, cf, N, g)) return err;
    GMK_REQUIRE(n == (int64_t)C * H * W, "%s: n = %lld is not C H W = %lld", who, (long long)n, (long long)((int64_t)C * H * W));
    return 0;
}

extern "C" int gmk_sampler_step_ns(const float* v, const float* v_uncond, const float* cond_w, const float* r, const float* z,
                                   const float* noise, float logsnr_t, float logsnr_s, int is_last, float* z_next, float* x_pred,
                                   float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, int C, int H, int W,
                                   int cf, int N, void* stream) {
    BoxGeom g;
    if (const int err = ns_geom_check("gmk_sampler_step_ns", B, n, C, H, W, cf, N, &g)) return err;
    return sampler_step_launch<false, true>("gmk_sampler_step_ns", v, v_uncond, cond_w, nullptr, z, noise, logsnr_t, logsnr_s, is_last, z_next,
                                            x_pred, eps_pred, z_dup, logsnr_next, mean_type, B, n, stream, r, g);
}

extern "C" int gmk_dpm_solver_step_ns(const float* v, const float* v_uncond, const float* cond_w, const float* r, const float* z,
                                      float* x_hist, float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_prev,
                                      int is_last, float* z_next, float* x_pred, float* eps_pred, float* z_dup, float* logsnr_next,
                                      int mean_type, int B, int64_t n, int C, int H, int W, int cf, int N, void* stream) {
    BoxGeom g;
    if (const int err = ns_geom_check("gmk_dpm_solver_step_ns", B, n, C, H, W, cf, N, &g)) return err;
    return dpm_solver_step_launch<false, true>("gmk_dpm_solver_step_ns", v, v_uncond, cond_w, nullptr, z, x_hist, logsnr_t, logsnr_s, coef_z,
                                               coef_x, coef_prev, is_last, z_next, x_pred, eps_pred, z_dup, logsnr_next, mean_type, B, n,
                                               stream, r, g);
}

extern "C" int gmk_dyn_threshold(const float* v, const float* v_uncond, const float* cond_w, const float* z, float logsnr_t, int k_lo,
                                 float frac, float* s_out, float* q_out, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && s_out, "gmk_dyn_threshold: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0 && n < ((int64_t)1 << 31), "gmk_dyn_threshold: bad shape B=%d n=%lld (n < 2^31)", B, (long long)n);
    if (const int err = step_args_check("gmk_dyn_threshold", mean_type, v_uncond, cond_w, B, n)) return err;
    GMK_REQUIRE(k_lo >= 0 && k_lo < n, "gmk_dyn_threshold: rank k_lo = %d outside [0, n = %lld)", k_lo, (long long)n);
    GMK_REQUIRE(frac >= 0.0f && frac < 1.0f, "gmk_dyn_threshold: frac = %g outside [0, 1)", (double)frac);
    GMK_REQUIRE(isfinite(logsnr_t), "gmk_dyn_threshold: non-finite time");
    dyn_threshold_kernel<<<B, 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, logsnr_t, (uint32_t)k_lo, frac, s_out, q_out, (uint32_t)n,
                                                            mean_type);
    return gmk_check_launch("gmk_dyn_threshold");
}

extern "C" int gmk_inpaint_merge(float* z, const float* x0, const uint8_t* mask, float alpha_s, float sigma_s, float a, float b,
                                 int is_last, int renoise, float logsnr_t, float logsnr_s, uint64_t seed, uint64_t offset, uint64_t q0,
                                 int B_total, float* z_dup, float* logsnr_next, int B, int64_t n, void* stream) {
    GMK_REQUIRE(z && x0 && mask, "gmk_inpaint_merge: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0 && n % 4 == 0, "gmk_inpaint_merge: bad shape B=%d n=%lld (n %% 4 == 0 required)", B,
                (long long)n);
    // the chunk's counters lie inside the whole batch's: q0 + B n / 4 <= B_total n / 4
    GMK_REQUIRE(B_total >= B && B_total < 65536 && q0 <= (uint64_t)(B_total - B) * (uint64_t)(n / 4),
                "gmk_inpaint_merge: chunk (B=%d, q0=%llu) outside the batch of B_total=%d", B, (unsigned long long)q0, B_total);
    GMK_REQUIRE(!(is_last && renoise), "gmk_inpaint_merge: the last step does not re-noise");
    GMK_REQUIRE(isfinite(alpha_s) && isfinite(sigma_s) && isfinite(a) && isfinite(b) && isfinite(logsnr_t) && isfinite(logsnr_s),
                "gmk_inpaint_merge: non-finite time or coefficient");
    const int gx = row_grid(n, 1024);
    const uint64_t ctr1 = offset + q0;
    const uint64_t ctr2 = offset + (uint64_t)B_total * (uint64_t)(n / 4) + q0;
    inpaint_merge_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(z, x0, mask, alpha_s, sigma_s, a, b, is_last, renoise,
                                                                     renoise ? logsnr_t : logsnr_s, seed, ctr1, ctr2, z_dup, logsnr_next, n);
    return gmk_check_launch("gmk_inpaint_merge");
}

extern "C" int gmk_consistency_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, float logsnr_t, float logsnr_s,
                                    int is_last, uint64_t seed, uint64_t offset, uint64_t q0, float* z_next, float* x_pred, float* eps_pred,
                                    float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && z_next, "gmk_consistency_step: null pointer");
    if (const int err = step_args_check("gmk_consistency_step", mean_type, v_uncond, cond_w, B, n)) return err;
    GMK_REQUIRE(n % 4 == 0, "gmk_consistency_step: n = %lld (n %% 4 == 0 required)", (long long)n);
    GMK_REQUIRE(isfinite(logsnr_t) && isfinite(logsnr_s), "gmk_consistency_step: non-finite time");
    // alpha_s^2 = sigmoid(logsnr_s), sigma_s^2 = sigmoid(-logsnr_s), in double from the fp32 log-SNR
    const double ls = (double)logsnr_s;
    const float alpha_s = (float)sqrt(1.0 / (1.0 + exp(-ls))), sigma_s = (float)sqrt(1.0 / (1.0 + exp(ls)));
    const int gx = row_grid(n, 1024);
    consistency_step_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, logsnr_t, logsnr_s, alpha_s, sigma_s, is_last, seed,
                                                                        offset + q0, z_next, x_pred, eps_pred, z_dup, logsnr_next, n, mean_type);
    return gmk_check_launch("gmk_consistency_step");
}

extern "C" int gmk_stochastic_step(const float* v, const float* v_uncond, const float* cond_w, const float* z, float* x_hist, const float* thr,
                                   float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_noise, float coef_prev, int is_last,
                                   uint64_t seed, uint64_t offset, uint64_t q0, float* z_next, float* x_pred, float* eps_pred, float* z_dup,
                                   float* logsnr_next, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && z_next, "gmk_stochastic_step: null pointer");
    if (const int err = step_args_check("gmk_stochastic_step", mean_type, v_uncond, cond_w, B, n)) return err;
    GMK_REQUIRE(n % 4 == 0, "gmk_stochastic_step: n = %lld (n %% 4 == 0 required)", (long long)n);
    GMK_REQUIRE(isfinite(logsnr_t) && isfinite(logsnr_s) && isfinite(coef_z) && isfinite(coef_x) && isfinite(coef_noise) && isfinite(coef_prev),
                "gmk_stochastic_step: non-finite time or coefficient");
    GMK_REQUIRE(coef_noise >= 0.0f, "gmk_stochastic_step: coef_noise = %g, a standard deviation: need >= 0", (double)coef_noise);
    GMK_REQUIRE(coef_prev == 0.0f || x_hist, "gmk_stochastic_step: coef_prev = %g without x_hist", (double)coef_prev);
    const dim3 grid(row_grid(n, 1024), B);
    if (thr)
        stochastic_step_kernel<true><<<grid, 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, x_hist, thr, logsnr_t, logsnr_s, coef_z, coef_x,
                                                                          coef_noise, coef_prev, is_last, seed, offset + q0, z_next, x_pred,
                                                                          eps_pred, z_dup, logsnr_next, n, mean_type);
    else
        stochastic_step_kernel<false><<<grid, 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, x_hist, nullptr, logsnr_t, logsnr_s, coef_z,
                                                                           coef_x, coef_noise, coef_prev, is_last, seed, offset + q0, z_next,
                                                                           x_pred, eps_pred, z_dup, logsnr_next, n, mean_type);
    return gmk_check_launch("gmk_stochastic_step");
}

extern "C" int gmk_stochastic_step_lv(const float* v, const float* v_uncond, const float* cond_w, const float* z, const float* nu,
                                      const float* thr, float logsnr_t, float logsnr_s, float coef_z, float coef_x, float coef_noise_small,
                                      float half_delta, int is_last, uint64_t seed, uint64_t offset, uint64_t q0, float* z_next, float* x_pred,
                                      float* eps_pred, float* z_dup, float* logsnr_next, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && nu && z_next, "gmk_stochastic_step_lv: null pointer");
    if (const int err = step_args_check("gmk_stochastic_step_lv", mean_type, v_uncond, cond_w, B, n)) return err;
    GMK_REQUIRE(n % 4 == 0, "gmk_stochastic_step_lv: n = %lld (n %% 4 == 0 required)", (long long)n);
    GMK_REQUIRE(isfinite(logsnr_t) && isfinite(logsnr_s) && isfinite(coef_z) && isfinite(coef_x) && isfinite(coef_noise_small) && isfinite(half_delta),
                "gmk_stochastic_step_lv: non-finite time or coefficient");
    GMK_REQUIRE(coef_noise_small >= 0.0f, "gmk_stochastic_step_lv: coef_noise_small = %g, a standard deviation: need >= 0", (double)coef_noise_small);
    GMK_REQUIRE(half_delta >= 0.0f, "gmk_stochastic_step_lv: half_delta = %g, half of logvar_large - logvar_small: need >= 0", (double)half_delta);
    const dim3 grid(row_grid(n, 1024), B);
    if (thr)
        stochastic_step_lv_kernel<true><<<grid, 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, nu, thr, logsnr_t, logsnr_s, coef_z, coef_x,
                                                                             coef_noise_small, half_delta, is_last, seed, offset + q0, z_next,
                                                                             x_pred, eps_pred, z_dup, logsnr_next, n, mean_type);
    else
        stochastic_step_lv_kernel<false><<<grid, 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, nu, nullptr, logsnr_t, logsnr_s, coef_z,
                                                                              coef_x, coef_noise_small, half_delta, is_last, seed, offset + q0,
                                                                              z_next, x_pred, eps_pred, z_dup, logsnr_next, n, mean_type);
    return gmk_check_launch("gmk_stochastic_step_lv");
}

extern "C" int gmk_q_sample_logsnr(const float* x, const float* eps, const float* logsnr, float* z, int B, int64_t n, void* stream) {
    GMK_REQUIRE(x && eps && logsnr && z, "gmk_q_sample_logsnr: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0, "gmk_q_sample_logsnr: bad shape B=%d n=%lld", B, (long long)n);
    const int gx = row_grid(n, 1024);
    q_sample_logsnr_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(x, eps, logsnr, z, n);
    return gmk_check_launch("gmk_q_sample_logsnr");
}

extern "C" int gmk_vlb_term(const float* out, const float* z, const float* eps, const float* logsnr, const float* weight, float* acc,
                            int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(out && z && eps && logsnr && weight && acc, "gmk_vlb_term: null pointer");
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_vlb_term");
    GMK_REQUIRE(B > 0 && n > 0, "gmk_vlb_term: bad shape B=%d n=%lld", B, (long long)n);
    vlb_term_kernel<<<B, 256, 0, gmk_stream(stream)>>>(out, z, eps, logsnr, weight, acc, n, mean_type);
    return gmk_check_launch("gmk_vlb_term");
}

extern "C" int gmk_vlb_endpoints(const float* x, const float* eps0, float delta, float* out_prior, float* out_dec, int B, int64_t n,
                                 void* stream) {
    GMK_REQUIRE(x && eps0 && out_prior && out_dec, "gmk_vlb_endpoints: null pointer");
    GMK_REQUIRE(B > 0 && n > 0, "gmk_vlb_endpoints: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE(delta > 0.0f && delta <= 0.5f, "gmk_vlb_endpoints: delta = %g outside (0, 0.5]", (double)delta);
    // the bound's end points lambda_min = -20 (prior) and lambda_max = 20 (decoder), in double: alpha_1^2 = sigmoid(-20) ~ 2.1e-9, and
    // -a - log1p(-a) = a^2/2 + a^3/3 + ... (the x-free part of the prior KL) is formed by its series, which has no cancellation
    const double a2 = 1.0 / (1.0 + exp(20.0));
    const double prior_c = 0.5 * (a2 * a2 / 2.0 + a2 * a2 * a2 / 3.0);
    const double dscale = (double)delta * exp(10.0);            // delta / s, s = sigma_0 / alpha_0 = exp(-lambda_max / 2)
    // data range: binarised data (delta = 1/2) lie in {0, 1}, everything else in [-1, 1]
    const float lo = delta == 0.5f ? 0.0f : -1.0f;
    vlb_endpoints_kernel<<<B, 256, 0, gmk_stream(stream)>>>(x, eps0, delta, (float)dscale, lo, 1.0f, (float)(0.5 * a2), (float)prior_c,
                                                            out_prior, out_dec, n);
    return gmk_check_launch("gmk_vlb_endpoints");
}

extern "C" int gmk_ddim_step_vec(const float* v, const float* v_uncond, const float* cond_w, const float* z,
                                 const float* logsnr_t, const float* logsnr_s, float* z_next, float* x_pred, float* eps_pred,
                                 int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && z && z_next && logsnr_t && logsnr_s, "gmk_ddim_step_vec: null pointer");
    if (const int err = step_args_check("gmk_ddim_step_vec", mean_type, v_uncond, cond_w, B, n)) return err;
    const int gx = row_grid(n, 256);
    sampler_step_kernel<false><<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(v, v_uncond, cond_w, z, nullptr, 0.f, 0.f, 0, z_next, x_pred,
                                                                            eps_pred, n, logsnr_t, logsnr_s, mean_type);
    return gmk_check_launch("gmk_ddim_step_vec");
}

namespace {
// u -> logsnr = sched_logsnr(u) (diffusion_utils.py:169-201); optionally u = (i + 1) / T - u_shift from integer times (gaussian_diffusion.py:90-91)
__global__ void schedule_kernel(const float* __restrict__ u, const int64_t* __restrict__ ti, float T, float u_shift, int kind, float a,
                                float sb, float lmin, float lmax, float shift, float* __restrict__ u_out, float* __restrict__ logsnr,
                                int B) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    float uu = ti ? __fdiv_rn((float)(ti[b] + 1), T) : u[b];
    uu = __fsub_rn(uu, u_shift);
    if (u_out) u_out[b] = uu;
    logsnr[b] = sched_logsnr(kind, a, sb, lmin, lmax, shift, uu);
}

// gaussian_diffusion.py:147-154: x-target implied by two teacher DDIM steps, its i == 0 select, and the eps-target
__global__ __launch_bounds__(256) void distill_target_kernel(const float* __restrict__ z_teacher, const float* __restrict__ z_t,
                                                            const float* __restrict__ x_pred_teacher,
                                                            const float* __restrict__ logsnr, const float* __restrict__ logsnr_s,
                                                            const int64_t* __restrict__ ti, float* __restrict__ x_target,
                                                            float* __restrict__ eps_target, int64_t n) {
    const int b = blockIdx.y;
    const float l = logsnr[b], ls = logsnr_s[b];
    const float alpha_s = sqrtf(1.0f / (1.0f + expf(-ls)));
    const float alpha_t = sqrtf(1.0f / (1.0f + expf(-l)));
    // F.softplus(x) = log1p(exp(x)) (x <= 20), x beyond the threshold
    const float sp_t = l > 20.f ? l : log1pf(expf(l));
    const float sp_s = ls > 20.f ? ls : log1pf(expf(ls));
    const float frac = expf(0.5f * (sp_t - sp_s));
    const float denom = alpha_s - frac * alpha_t;
    const float c1 = sqrtf(1.0f + expf(l)), c2 = 1.0f / sqrtf(1.0f + expf(-l));
    const bool first = ti[b] == 0;
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float zt = z_t[base + i];
        const float xt = first ? x_pred_teacher[base + i] : (z_teacher[base + i] - frac * zt) / denom;
        x_target[base + i] = xt;
        eps_target[base + i] = c1 * (zt - xt * c2);
    }
}

// consistency distillation (Song et al. 2023, "Consistency Models", Algorithm 2): the target net's clipped data prediction at (z_s, logsnr_s) -
// predict_x_eps, sampler_step_kernel's own x-hat - with the boundary condition f(., t_min) = identity as the i == 0 select of the teacher's final
// prediction, and the eps-target distill_target_kernel ends with.  grid (gx, B); VEC: 16-byte accesses (n % 4 == 0, aligned tensors), else one by
// one - the same operations per element.  Rows with i == 0 read neither v_tgt nor z_s.
template <bool VEC>
__global__ __launch_bounds__(256) void consistency_target_kernel(const float* __restrict__ v_tgt, const float* __restrict__ z_s,
                                                                const float* __restrict__ x_pred_teacher, const float* __restrict__ z_t,
                                                                const float* __restrict__ logsnr_t, const float* __restrict__ logsnr_s,
                                                                const int64_t* __restrict__ ti, float* __restrict__ x_target,
                                                                float* __restrict__ eps_target, int64_t n, int mt) {
    constexpr int STEP = VEC ? 4 : 1;
    const int b = blockIdx.y;
    const float l = logsnr_t[b];
    const LogsnrCoef cs = logsnr_coef(logsnr_s[b]);
    const float c1 = sqrtf(1.0f + expf(l)), c2 = 1.0f / sqrtf(1.0f + expf(-l));
    const bool first = ti[b] == 0;
    const int64_t base = (int64_t)b * n;
    for (int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * STEP; i < n; i += (int64_t)gridDim.x * 256 * STEP) {
        const int64_t j = base + i;
        float zt[STEP], xt[STEP], et[STEP];
        if constexpr (VEC) load4(z_t + j, zt); else zt[0] = z_t[j];
        if (first) {
            if constexpr (VEC) load4(x_pred_teacher + j, xt); else xt[0] = x_pred_teacher[j];
        } else {
            float vv[STEP], zs[STEP], eh;
            if constexpr (VEC) { load4(v_tgt + j, vv); load4(z_s + j, zs); } else { vv[0] = v_tgt[j]; zs[0] = z_s[j]; }
#pragma unroll
            for (int k = 0; k < STEP; ++k) predict_x_eps<false>(vv[k], nullptr, j + k, 0.f, zs[k], cs, mt, 1.0f, xt[k], eh);
        }
#pragma unroll
        for (int k = 0; k < STEP; ++k) et[k] = c1 * (zt[k] - xt[k] * c2);
        if constexpr (VEC) { store4(x_target + j, xt); store4(eps_target + j, et); } else { x_target[j] = xt[0]; eps_target[j] = et[0]; }
    }
}
}  // namespace

extern "C" int gmk_logsnr_schedule(const float* u, const int64_t* i_times, int num_steps, float shift, float* u_out,
                                   float* logsnr, int B, void* stream) {
    GMK_REQUIRE((u != nullptr) != (i_times != nullptr) && logsnr && B > 0, "gmk_logsnr_schedule: give exactly one of u / i_times");
    GMK_REQUIRE(!i_times || num_steps >= 1, "gmk_logsnr_schedule: num_steps");
    schedule_kernel<<<(B + 255) / 256, 256, 0, gmk_stream(stream)>>>(u, i_times, (float)num_steps, shift, GMK_SCHED_COSINE, kSchedA, kSchedB,
                                                                     0.f, 0.f, 0.f, u_out, logsnr, B);
    return gmk_check_launch("gmk_logsnr_schedule");
}

extern "C" int gmk_logsnr_schedule_sched(const float* u, const int64_t* i_times, int num_steps, float u_shift, int kind, float a, float b,
                                         float lmin, float lmax, float shift, float* u_out, float* logsnr, int B, void* stream) {
    GMK_REQUIRE((u != nullptr) != (i_times != nullptr) && logsnr && B > 0, "gmk_logsnr_schedule_sched: give exactly one of u / i_times");
    GMK_REQUIRE(!i_times || num_steps >= 1, "gmk_logsnr_schedule_sched: num_steps");
    GMK_REQUIRE_SCHED(kind, a, b, lmin, lmax, shift, "gmk_logsnr_schedule_sched");
    schedule_kernel<<<(B + 255) / 256, 256, 0, gmk_stream(stream)>>>(u, i_times, (float)num_steps, u_shift, kind, a, b, lmin, lmax, shift, u_out,
                                                                     logsnr, B);
    return gmk_check_launch("gmk_logsnr_schedule_sched");
}

extern "C" int gmk_distill_target(const float* z_teacher, const float* z_t, const float* x_pred_teacher, const float* logsnr,
                                  const float* logsnr_s, const int64_t* i_times, float* x_target, float* eps_target, int B,
                                  int64_t n, void* stream) {
    GMK_REQUIRE(z_teacher && z_t && x_pred_teacher && logsnr && logsnr_s && i_times && x_target && eps_target,
                "gmk_distill_target: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0, "gmk_distill_target: bad shape");
    const int gx = row_grid(n, 256);
    distill_target_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(z_teacher, z_t, x_pred_teacher, logsnr, logsnr_s, i_times,
                                                                       x_target, eps_target, n);
    return gmk_check_launch("gmk_distill_target");
}

extern "C" int gmk_consistency_target(const float* v_tgt, const float* z_s, const float* x_pred_teacher, const float* z_t, const float* logsnr_t,
                                      const float* logsnr_s, const int64_t* i_times, float* x_target, float* eps_target, int mean_type, int B,
                                      int64_t n, void* stream) {
    GMK_REQUIRE(v_tgt && z_s && x_pred_teacher && z_t && logsnr_t && logsnr_s && i_times && x_target && eps_target,
                "gmk_consistency_target: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0, "gmk_consistency_target: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_consistency_target");
    if (rows_aligned16(n, v_tgt, z_s, x_pred_teacher, z_t, x_target, eps_target)) consistency_target_kernel<true><<<dim3(row_grid(n, 1024), B), 256, 0, gmk_stream(stream)>>>(v_tgt, z_s, x_pred_teacher, z_t, logsnr_t, logsnr_s, i_times, x_target, eps_target, n, mean_type);
    else consistency_target_kernel<false><<<dim3(row_grid(n, 256), B), 256, 0, gmk_stream(stream)>>>(v_tgt, z_s, x_pred_teacher, z_t, logsnr_t, logsnr_s, i_times, x_target, eps_target, n, mean_type);
    return gmk_check_launch("gmk_consistency_target");
}

// scalar prologue in double, as torch.optim.adam._single_tensor_adam does on the host, then the one launch of an Adam step
template <bool EMA, bool CTL, int NP = 0, bool PVEC = true>
static int adam_launch(const char* who, float* p, const float* g, float* m, float* v, float* ema, const float* state, int64_t n, float lr,
                       float beta1, float beta2, float eps, int step, float grad_scale, float ema_w, void* stream, PemaArgs pa = PemaArgs{}) {
    const double bc1 = 1.0 - pow((double)beta1, step);
    const double bc2 = 1.0 - pow((double)beta2, step);
    const float step_size = (float)((double)lr / bc1);
    const float inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    adam_kernel<EMA, CTL, NP, PVEC><<<stream_grid(n / 4 + 1), 256, 0, gmk_stream(stream)>>>(p, g, m, v, ema, state, n, step_size, beta1, beta2,
                                                                                            eps, inv_bc2_sqrt, grad_scale, ema_w, pa);
    return gmk_check_launch(who);
}

extern "C" int gmk_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                             float eps, int step, float grad_scale, void* stream) {
    GMK_REQUIRE(p && g && m && v && n > 0 && step >= 1, "gmk_adam_step: bad arguments");
    return adam_launch<false, false>("gmk_adam_step", p, g, m, v, nullptr, nullptr, n, lr, beta1, beta2, eps, step, grad_scale, 0.0f, stream);
}

extern "C" int gmk_adam_ema_step(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1,
                                 float beta2, float eps, int step, float grad_scale, float ema_w, void* stream) {
    GMK_REQUIRE(p && g && m && v && n > 0 && step >= 1, "gmk_adam_ema_step: bad arguments");
    GMK_REQUIRE(ema, "gmk_adam_ema_step: ema is null");
    GMK_REQUIRE(ema_w >= 0.0f && ema_w <= 1.0f, "gmk_adam_ema_step: ema_w = %g outside [0, 1]", (double)ema_w);
    return adam_launch<true, false>("gmk_adam_ema_step", p, g, m, v, ema, nullptr, n, lr, beta1, beta2, eps, step, grad_scale, ema_w, stream);
}

static int64_t grad_norm_parts(int64_t n) {
    const int64_t nq = n / 4;
    return nq <= kNormQuads ? 1 : (nq + kNormQuads - 1) / kNormQuads;
}

extern "C" int64_t gmk_grad_norm_workspace_bytes(int64_t n) { return n > 0 ? grad_norm_parts(n) * (int64_t)sizeof(float) : 0; }

extern "C" int gmk_grad_norm(const float* g, int64_t n, float grad_scale, float max_norm, float* workspace, int64_t workspace_bytes,
                             float* state, void* stream) {
    GMK_REQUIRE(g && workspace && state && n > 0, "gmk_grad_norm: bad arguments");
    GMK_REQUIRE(isfinite(grad_scale) && grad_scale > 0.0f, "gmk_grad_norm: grad_scale = %g must be finite and positive", (double)grad_scale);
    GMK_REQUIRE(!isnan(max_norm), "gmk_grad_norm: max_norm is NaN");
    const int64_t parts = grad_norm_parts(n);
    GMK_REQUIRE(parts < (int64_t)1 << 31, "gmk_grad_norm: n = %lld too large", (long long)n);
    GMK_REQUIRE(workspace_bytes >= parts * (int64_t)sizeof(float), "gmk_grad_norm: workspace of %lld bytes, %lld needed",
                (long long)workspace_bytes, (long long)(parts * (int64_t)sizeof(float)));
    grad_norm_partial_kernel<<<(int)parts, 256, 0, gmk_stream(stream)>>>(g, workspace, n);
    grad_norm_final_kernel<<<1, 256, 0, gmk_stream(stream)>>>(workspace, (int)parts, grad_scale, max_norm, state);
    return gmk_check_launch("gmk_grad_norm");
}

extern "C" int gmk_adam_step_ctl(float* p, const float* g, float* m, float* v, float* ema, int64_t n, float lr, float beta1, float beta2,
                                 float eps, int step, float grad_scale, float ema_w, const float* state, void* stream) {
    GMK_REQUIRE(p && g && m && v && n > 0 && step >= 1, "gmk_adam_step_ctl: bad arguments");
    GMK_REQUIRE(state, "gmk_adam_step_ctl: state is null");
    GMK_REQUIRE(!ema || (ema_w >= 0.0f && ema_w <= 1.0f), "gmk_adam_step_ctl: ema_w = %g outside [0, 1]", (double)ema_w);
    return (ema ? adam_launch<true, true> : adam_launch<false, true>)("gmk_adam_step_ctl", p, g, m, v, ema, state, n, lr, beta1, beta2, eps, step,
                                                                      grad_scale, ema ? ema_w : 0.0f, stream, PemaArgs{});
}

// gmk_adam_pema_step's instantiation: classic average or not, steered or not, for one row count and one row access width
template <int NP, bool PVEC>
static int adam_pema_launch(float* p, const float* g, float* m, float* v, float* ema, const float* state, int64_t n, float lr, float beta1,
                            float beta2, float eps, int step, float grad_scale, float ema_w, void* stream, PemaArgs pa) {
    auto launch = ema ? (state ? adam_launch<true, true, NP, PVEC> : adam_launch<true, false, NP, PVEC>)
                      : (state ? adam_launch<false, true, NP, PVEC> : adam_launch<false, false, NP, PVEC>);
    return launch("gmk_adam_pema_step", p, g, m, v, ema, state, n, lr, beta1, beta2, eps, step, grad_scale, ema ? ema_w : 0.0f, stream, pa);
}

extern "C" int gmk_adam_pema_step(float* p, const float* g, float* m, float* v, float* ema, float* pema, int64_t pema_stride, int n_pema,
                                  int64_t n, float lr, float beta1, float beta2, float eps, int step, float grad_scale, float ema_w, float pw0,
                                  float pw1, float pw2, const float* state, void* stream) {
    GMK_REQUIRE(n_pema >= 1 && n_pema <= 3, "gmk_adam_pema_step: n_pema = %d outside 1 .. 3", n_pema);
    GMK_REQUIRE(p && g && m && v && n > 0 && step >= 1, "gmk_adam_pema_step: bad arguments");
    GMK_REQUIRE(pema, "gmk_adam_pema_step: pema is null");
    GMK_REQUIRE(pema_stride >= n, "gmk_adam_pema_step: pema_stride = %lld below n = %lld", (long long)pema_stride, (long long)n);
    GMK_REQUIRE(!ema || (ema_w >= 0.0f && ema_w <= 1.0f), "gmk_adam_pema_step: ema_w = %g outside [0, 1]", (double)ema_w);
    const PemaArgs pa = {pema, pema_stride, {pw0, pw1, pw2}};
    for (int r = 0; r < n_pema; ++r)
        GMK_REQUIRE(pa.w[r] >= 0.0f && pa.w[r] <= 1.0f, "gmk_adam_pema_step: pw%d = %g outside [0, 1]", r, (double)pa.w[r]);
    const bool pvec = reinterpret_cast<uintptr_t>(pema) % 16 == 0 && pema_stride % 4 == 0;
#define GMK_PEMA_CASE(NP)                                                                                                                   \
    case NP:                                                                                                                                \
        return (pvec ? adam_pema_launch<NP, true> : adam_pema_launch<NP, false>)(p, g, m, v, ema, state, n, lr, beta1, beta2, eps, step,    \
                                                                                 grad_scale, ema_w, stream, pa)
    switch (n_pema) {
        GMK_PEMA_CASE(1);
        GMK_PEMA_CASE(2);
        default: GMK_PEMA_CASE(3);
    }
#undef GMK_PEMA_CASE
}

extern "C" int gmk_arena_combine(const float* src, int64_t src_stride, const double* coef, int K, float* out, int64_t n, void* stream) {
    GMK_REQUIRE(K >= 1 && K <= 64, "gmk_arena_combine: K = %d outside 1 .. 64", K);
    GMK_REQUIRE(src && coef && out && n > 0, "gmk_arena_combine: bad arguments");
    GMK_REQUIRE(src_stride >= n, "gmk_arena_combine: src_stride = %lld below n = %lld", (long long)src_stride, (long long)n);
    const float* src_end = src + (int64_t)(K - 1) * src_stride + n;
    GMK_REQUIRE(out + n <= src || out >= src_end, "gmk_arena_combine: out aliases src");
    const uintptr_t bases = reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out);
    if (bases % 16 == 0 && src_stride % 4 == 0)
        arena_combine_kernel<true><<<stream_grid(n / 4 + 1), 256, 0, gmk_stream(stream)>>>(src, src_stride, coef, K, out, n);
    else
        arena_combine_kernel<false><<<stream_grid(n), 256, 0, gmk_stream(stream)>>>(src, src_stride, coef, K, out, n);
    return gmk_check_launch("gmk_arena_combine");
}

extern "C" int gmk_rng_rademacher(float* out, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    GMK_REQUIRE(out && n > 0, "gmk_rng_rademacher: bad arguments");
    rng_rademacher_kernel<<<stream_grid((n + 3) / 4), 256, 0, gmk_stream(stream)>>>(out, n, seed, offset);
    return gmk_check_launch("gmk_rng_rademacher");
}

extern "C" int gmk_dequantize(const float* x, float* y, float delta, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
    GMK_REQUIRE(x && y && n > 0, "gmk_dequantize: bad arguments");
    GMK_REQUIRE(delta > 0.0f && delta <= 0.5f, "gmk_dequantize: delta = %g outside (0, 0.5]", (double)delta);
    dequantize_kernel<<<stream_grid((n + 3) / 4), 256, 0, gmk_stream(stream)>>>(x, y, delta, n, seed, offset);
    return gmk_check_launch("gmk_dequantize");
}

extern "C" int gmk_pf_ode_step(const float* out, float* z, const float* r, const float* g, float* acc, float* prior, float* x_out,
                               float logsnr_i, float logsnr_j, int update, float div_a, float div_b, float prior_c, int mean_type, int B,
                               int64_t n, void* stream) {
    GMK_REQUIRE(out && z, "gmk_pf_ode_step: null pointer");
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_pf_ode_step");
    GMK_REQUIRE(B > 0 && B < 65536 && n > 0, "gmk_pf_ode_step: bad shape B=%d n=%lld", B, (long long)n);
    GMK_REQUIRE(!acc || (r && g), "gmk_pf_ode_step: the divergence needs the probe r and the VJP g");
    GMK_REQUIRE(!(prior && update), "gmk_pf_ode_step: the prior is taken at the last point, which has no update");
    GMK_REQUIRE(isfinite(logsnr_i) && isfinite(logsnr_j) && isfinite(div_a) && isfinite(div_b) && isfinite(prior_c),
                "gmk_pf_ode_step: non-finite time or coefficient");
    const int gx = (acc || prior) ? 1 : row_grid(n, 1024);
    pf_ode_step_kernel<<<dim3(gx, B), 256, 0, gmk_stream(stream)>>>(out, z, r, g, acc, prior, x_out, logsnr_i, logsnr_j, update, div_a,
                                                                     div_b, prior_c, n, mean_type);
    return gmk_check_launch("gmk_pf_ode_step");
}

extern "C" int gmk_slerp(const float* a, const float* b, const float* t, float* out, float* cos_out, int B, int64_t n, int K, void* stream) {
    GMK_REQUIRE(a && b && t && out, "gmk_slerp: null pointer");
    GMK_REQUIRE(B >= 1 && K >= 1 && n >= 4 && n % 4 == 0, "gmk_slerp: bad shape B=%d n=%lld K=%d (B, K >= 1, n >= 4, n %% 4 == 0 required)", B,
                (long long)n, K);
    GMK_REQUIRE(((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                "gmk_slerp: a, b and out must be 16-byte aligned");
    hipStream_t st = gmk_stream(stream);
    if (n <= kSlerpKeep) slerp_kernel<kSlerpKeep / 1024><<<B, 256, 0, st>>>(a, b, t, out, cos_out, B, n, K);
    else slerp_kernel<0><<<B, 256, 0, st>>>(a, b, t, out, cos_out, B, n, K);
    return gmk_check_launch("gmk_slerp");
}

extern "C" int gmk_cfg_rescale(const float* v, const float* v_uncond, const float* cond_w, const float* z, float logsnr_t, float phi,
                               float* thr_out, float* ratio_out, int mean_type, int B, int64_t n, void* stream) {
    GMK_REQUIRE(v && v_uncond && cond_w && z && thr_out, "gmk_cfg_rescale: null pointer (v, v_uncond, cond_w, z and thr_out are required)");
    GMK_REQUIRE(isfinite(phi) && phi >= 0.0f && phi <= 1.0f, "gmk_cfg_rescale: phi = %g outside [0, 1]", (double)phi);
    GMK_REQUIRE(mean_type >= GMK_MEAN_V && mean_type <= GMK_MEAN_X, "gmk_cfg_rescale: mean_type must be 0 (v), 1 (eps) or 2 (x)");
    GMK_REQUIRE(B >= 1 && n >= 1, "gmk_cfg_rescale: bad shape B=%d n=%lld (B, n >= 1 required)", B, (long long)n);
    GMK_REQUIRE(isfinite(logsnr_t), "gmk_cfg_rescale: non-finite time");
    const bool vec = rows_aligned16(n, v, v_uncond, z);
    const bool keep = n <= kRescaleKeep;
    hipStream_t st = gmk_stream(stream);
    if (vec && keep) cfg_rescale_kernel<true, true><<<B, 256, 0, st>>>(v, v_uncond, cond_w, z, logsnr_t, phi, thr_out, ratio_out, n, mean_type);
    else if (vec) cfg_rescale_kernel<true, false><<<B, 256, 0, st>>>(v, v_uncond, cond_w, z, logsnr_t, phi, thr_out, ratio_out, n, mean_type);
    else if (keep) cfg_rescale_kernel<false, true><<<B, 256, 0, st>>>(v, v_uncond, cond_w, z, logsnr_t, phi, thr_out, ratio_out, n, mean_type);
    else cfg_rescale_kernel<false, false><<<B, 256, 0, st>>>(v, v_uncond, cond_w, z, logsnr_t, phi, thr_out, ratio_out, n, mean_type);
    return gmk_check_launch("gmk_cfg_rescale");
}

// ---- Diffusion posterior sampling (DPS: Chung et al. 2023, "Diffusion Posterior Sampling for General Noisy Inverse Problems", Algorithm 1);
// an extension, no reference call site.  Observation y = A x + noise; per sampler step, with the network output `out` at (z, lt):
//   x-hat = x_from_out(out, z) (UNCLIPPED: a clip has zero gradient where early steps saturate), e = y - A x-hat, u = A^T e, |e|^2 per image
//   (gmk_dps_backproject); g = (d out / d z)^T u (the network's input VJP); z_s += 2 zeta / max(|e|, FLT_MIN) (c_z u + c_o g) (gmk_dps_correct),
//   (c_z, c_o) = d x-hat / d (z, out).  A is the box mean of DDNM (BoxGeom; A^T e = e / k replicated over the box) or a separable Gaussian
//   blur with zero padding (symmetric: A^T = A).  Every sum is single rounded fp32 operations in a fixed order: the same call gives the same bits.
namespace {

constexpr int kBlurSide = GMK_BLUR_MAX_SIDE;        // a plane of at most 64 x 64 floats (16 KiB) is staged in LDS, with a second one for the row pass
constexpr int kBlurTaps = 2 * GMK_BLUR_MAX_R + 1;

struct BlurLds {
    float a[kBlurSide * kBlurSide], t[kBlurSide * kBlurSide], taps[kBlurTaps];
};

// every thread of a 256-thread workgroup: the first 2 R + 1 stage the taps
__device__ __forceinline__ void blur_stage_taps(BlurLds& s, const float* __restrict__ taps, int R) {
    if ((int)threadIdx.x < 2 * R + 1) s.taps[threadIdx.x] = taps[threadIdx.x];
}

// The blur of the H x W plane staged in s.a, in place, by every thread of a 256-thread workgroup (barriers inside: one ahead of the first read of
// s.a and s.taps, one behind the last write).  Rows first, s.t[y][x] = sum_k taps[k + R] a[y][x + k], then columns, a[y][x] = sum_k taps[k + R]
// t[y + k][x]; each sum starts from 0 and adds fmul(tap, value) for k = -R ... R in that order, the terms outside the plane (zero padding) left
// out.  Thread i % 256 writes element i in both passes.
__device__ __forceinline__ void blur_plane(BlurLds& s, int R, int H, int W) {
    const int n = H * W;
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int y = i / W, x = i - y * W;
        const int k0 = x < R ? -x : -R, k1 = W - 1 - x < R ? W - 1 - x : R;
        float acc = 0.f;
        for (int k = k0; k <= k1; ++k) acc = __fadd_rn(acc, __fmul_rn(s.taps[k + R], s.a[i + k]));
        s.t[i] = acc;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) {
        const int y = i / W;
        const int k0 = y < R ? -y : -R, k1 = H - 1 - y < R ? H - 1 - y : R;
        float acc = 0.f;
        for (int k = k0; k <= k1; ++k) acc = __fadd_rn(acc, __fmul_rn(s.taps[k + R], s.t[i + k * W]));
        s.a[i] = acc;
    }
    __syncthreads();
}

// grid B, one workgroup per image, which loops over the channels: out = A x
__global__ __launch_bounds__(256) void gauss_blur_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ taps,
                                                        int R, int C, int H, int W) {
    __shared__ BlurLds s;
    const int n = H * W;
    blur_stage_taps(s, taps, R);
    for (int ch = 0; ch < C; ++ch) {
        const int64_t base = ((int64_t)blockIdx.x * C + ch) * n;
        for (int i = threadIdx.x; i < n; i += 256) s.a[i] = x[base + i];
        blur_plane(s, R, H, W);
        for (int i = threadIdx.x; i < n; i += 256) out[base + i] = s.a[i];
    }
}

// grid B, one workgroup per image.  x-hat = x_from_out(v, z) per element (v and z are read once), then
//   BLUR: per channel, A x-hat by blur_plane (gauss_blur_kernel's function: its bits), e = fsub(obs, A x-hat) over the plane, u = blur_plane(e);
//   box:  per box (one thread each, 256 at a time), box_kernel's sequential mean of x-hat, e = fsub(obs, mean), u = fdiv(e, (float)k) stored to
//         the k members.
// enorm2[b] = |e_b|^2: every thread adds fmul(e, e) of its elements to a partial in the order it visits them (from 0), the 256 partials are
// summed by a binary tree in LDS (red[t] += red[t + s] for s = 128, 64 ... 1).  No atomics.
template <bool BLUR>
__global__ __launch_bounds__(256) void dps_backproject_kernel(const float* __restrict__ v, const float* __restrict__ z,
                                                             const float* __restrict__ obs, float lt, int mt, const float* __restrict__ taps,
                                                             int R, float* __restrict__ u, float* __restrict__ enorm2, BoxGeom g) {
    __shared__ float red[256];
    const int b = blockIdx.x;
    const LogsnrCoef c = logsnr_coef(lt);
    float part = 0.f;
    if constexpr (BLUR) {
        __shared__ BlurLds s;
        const int n = g.HW;
        blur_stage_taps(s, taps, R);
        for (uint32_t ch = 0; ch < g.C; ++ch) {
            const int64_t base = ((int64_t)b * g.C + ch) * n;
            for (int i = threadIdx.x; i < n; i += 256) s.a[i] = x_from_out(v[base + i], z[base + i], c, mt);
            blur_plane(s, R, g.H, g.W);
            for (int i = threadIdx.x; i < n; i += 256) {
                const float e = __fsub_rn(obs[base + i], s.a[i]);
                part = __fadd_rn(part, __fmul_rn(e, e));
                s.a[i] = e;
            }
            blur_plane(s, R, g.H, g.W);
            for (int i = threadIdx.x; i < n; i += 256) u[base + i] = s.a[i];
        }
    } else {
        const float k = (float)(g.cf * g.N * g.N);
        const int64_t base = (int64_t)b * g.C * g.HW;
        for (uint32_t box = threadIdx.x; box < g.n_box; box += 256) {
            const uint32_t j = box % g.Wb, t = box / g.Wb, i = t % g.Hb, cp = t / g.Hb;
            float sum = 0.f;
            for (uint32_t dc = 0; dc < g.cf; ++dc)
                for (uint32_t dy = 0; dy < g.N; ++dy) {
                    const int64_t row = base + (int64_t)(cp * g.cf + dc) * g.HW + (i * g.N + dy) * g.W + j * g.N;
                    for (uint32_t dx = 0; dx < g.N; ++dx) sum = __fadd_rn(sum, x_from_out(v[row + dx], z[row + dx], c, mt));
                }
            const float e = __fsub_rn(obs[(int64_t)b * g.n_box + box], __fdiv_rn(sum, k));
            part = __fadd_rn(part, __fmul_rn(e, e));
            const float ue = __fdiv_rn(e, k);
            for (uint32_t dc = 0; dc < g.cf; ++dc)
                for (uint32_t dy = 0; dy < g.N; ++dy) {
                    const int64_t row = base + (int64_t)(cp * g.cf + dc) * g.HW + (i * g.N + dy) * g.W + j * g.N;
                    for (uint32_t dx = 0; dx < g.N; ++dx) u[row + dx] = ue;
                }
        }
    }
    red[threadIdx.x] = part;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = __fadd_rn(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x == 0) enorm2[b] = red[0];
}

// grid (ceil(n / 1024), B), n % 4 == 0, in place: z = fadd(z, fmul(scale, fadd(fmul(c_z, u), fmul(c_o, g)))) with scale = min(fdiv(zeta2,
// max(sqrt(enorm2[b]), FLT_MIN)), FLT_MAX), zeta2 = 2 zeta from the host (the min keeps 0 times the scale 0 when |e| = 0)
__global__ __launch_bounds__(256) void dps_correct_kernel(float* __restrict__ z, const float* __restrict__ u, const float* __restrict__ g,
                                                         const float* __restrict__ enorm2, float c_z, float c_o, float zeta2, int64_t n) {
    const int b = blockIdx.y;
    const float scale = fminf(__fdiv_rn(zeta2, fmaxf(sqrtf(enorm2[b]), FLT_MIN)), FLT_MAX);
    const int64_t base = (int64_t)b * n;
    for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x * 4; i < n; i += (int64_t)gridDim.x * 1024) {
        float zv[4], uv[4], gv[4];
        load4(z + base + i, zv);
        load4(u + base + i, uv);
        load4(g + base + i, gv);
#pragma unroll
        for (int k = 0; k < 4; ++k) zv[k] = __fadd_rn(zv[k], __fmul_rn(scale, __fadd_rn(__fmul_rn(c_z, uv[k]), __fmul_rn(c_o, gv[k]))));
        store4(z + base + i, zv);
    }
}

}  // namespace

static int blur_args_check(const char* who, const float* taps, int R, int B, int C, int H, int W) {
    GMK_REQUIRE(taps, "%s: null pointer (taps)", who);
    GMK_REQUIRE(R >= 1 && R <= GMK_BLUR_MAX_R, "%s: R = %d outside [1, %d]", who, R, GMK_BLUR_MAX_R);
    GMK_REQUIRE(B > 0 && B < 65536 && C > 0 && H > 0 && W > 0 && H <= GMK_BLUR_MAX_SIDE && W <= GMK_BLUR_MAX_SIDE,
                "%s: bad shape B=%d C=%d H=%d W=%d (H, W <= %d: the plane is staged in LDS)", who, B, C, H, W, GMK_BLUR_MAX_SIDE);
    return 0;
}

extern "C" int gmk_gauss_blur(const float* x, float* out, const float* taps, int R, int B, int C, int H, int W, void* stream) {
    GMK_REQUIRE(x && out, "gmk_gauss_blur: null pointer");
    if (const int err = blur_args_check("gmk_gauss_blur", taps, R, B, C, H, W)) return err;
    gauss_blur_kernel<<<B, 256, 0, gmk_stream(stream)>>>(x, out, taps, R, C, H, W);
    return gmk_check_launch("gmk_gauss_blur");
}

extern "C" int gmk_dps_backproject(const float* v, const float* z, const float* obs, float logsnr_t, int op, int cf, int N, const float* taps,
                                   int R, float* u, float* enorm2, int mean_type, int B, int C, int H, int W, void* stream) {
    GMK_REQUIRE(v && z && obs && u && enorm2, "gmk_dps_backproject: null pointer");
    GMK_REQUIRE_MEAN_TYPE(mean_type, "gmk_dps_backproject");
    GMK_REQUIRE(isfinite(logsnr_t), "gmk_dps_backproject: non-finite time");
    GMK_REQUIRE(op == GMK_DPS_BOX || op == GMK_DPS_BLUR, "gmk_dps_backproject: op = %d, expected 0 (box) or 1 (blur)", op);
    BoxGeom g;
    if (op == GMK_DPS_BLUR) {
        if (const int err = blur_args_check("gmk_dps_backproject", taps, R, B, C, H, W)) return err;
        if (const int err = box_geom_check("gmk_dps_backproject", B, C, H, W, 1, 1, &g)) return err;      // (the shape fields alone are read)
        dps_backproject_kernel<true><<<B, 256, 0, gmk_stream(stream)>>>(v, z, obs, logsnr_t, mean_type, taps, R, u, enorm2, g);
    } else {
        if (const int err = box_geom_check("gmk_dps_backproject", B, C, H, W, cf, N, &g)) return err;
        dps_backproject_kernel<false><<<B, 256, 0, gmk_stream(stream)>>>(v, z, obs, logsnr_t, mean_type, nullptr, 0, u, enorm2, g);
    }
    return gmk_check_launch("gmk_dps_backproject");
}

extern "C" int gmk_dps_correct(float* z, const float* u, const float* g, const float* enorm2, float c_z, float c_o, float zeta, int B, int64_t n,
                               void* stream) {
    GMK_REQUIRE(z && u && g && enorm2, "gmk_dps_correct: null pointer");
    GMK_REQUIRE(B > 0 && B < 65536 && n >= 4 && n % 4 == 0, "gmk_dps_correct: bad shape B=%d n=%lld (n %% 4 == 0 required)", B, (long long)n);
    GMK_REQUIRE(((reinterpret_cast<uintptr_t>(z) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(g)) & 15) == 0,
                "gmk_dps_correct: z, u and g must be 16-byte aligned");
    GMK_REQUIRE(isfinite(c_z) && isfinite(c_o) && isfinite(zeta) && zeta >= 0.0f && isfinite(2.0f * zeta),
                "gmk_dps_correct: c_z = %g, c_o = %g, zeta = %g: finite, zeta >= 0", (double)c_z, (double)c_o, (double)zeta);
    if (zeta == 0.0f) return 0;      // no guidance: nothing is launched, z keeps its bits (a sum z + 0 would turn -0 into +0)
    dps_correct_kernel<<<dim3(row_grid(n, 1024), B), 256, 0, gmk_stream(stream)>>>(z, u, g, enorm2, c_z, c_o, 2.0f * zeta, n);
    return gmk_check_launch("gmk_dps_correct");
}
