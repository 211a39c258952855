"""CPU restatement of DDNM restoration for box-mean operators (Wang, Yu & Zhang 2023, "Zero-Shot Image Restoration Using Denoising Diffusion
Null-Space Model", eq. 13-14, noise-free; `GaussianDiffusion.restore`, gmk_box_mean, gmk_box_residual, gmk_sampler_step_ns,
gmk_dpm_solver_step_ns) - test infrastructure.

Images are [B, C, H, W].  The operator A has parameters (cf, N): cf in {1, C} channels averaged together, an N x N spatial box, k = cf N^2;
the observation is [B, C / cf, H / N, W / N].
    A x      the mean of every box                                  (`A`)
    A+ u     every member of a box gets the box's value             (`A_pinv`)
    A A+ = I, so  x + A+(y - A x)  projects onto {x : A x = y}      (`project`)
One network evaluation at (z, logsnr_t): x_hat is the samplers' clipped (and, guided, extrapolated between two clips) data prediction, then
    r = obs - A x_hat,   x_hat' = x_hat + A+ r   (not clipped again),   eps_hat' = eps(z, x_hat'),
and the sampler's update - DDIM, the ancestral step, DPM-Solver++(2M) - runs on (x_hat', eps_hat'); the last step returns x_hat'.
A, A+, the residual, the projection and the three updates are float64 on the `predict_*` functions of oracle.diffusion_ref.  The whole chain
(`sample`) is modelled on tests/inpaint_ref.py: x_hat of every network evaluation is the oracle's own (`sampler_ref.oracle_predict`: `run_model`
+ `cf_guidance` on oracle.unet_ref's forward, fp32, exactly as the oracle's DDIM step forms it), and everything restoration adds runs in float64
on it.  The guided x_hat is not restated in float64 for the chains: at the first network time (logsnr -20) the reference's guidance forms
x = d1 (z - e d2) with e d2 = z - O(4e-5) and d1 = 2e4, which cancels in fp32 to 1e-3 (1 + 2 w) of x; the oracle and the kernels share that
formula operation by operation, a float64 x_hat would measure the formula instead of the restoration (`x_hat` below is that float64 form, for
single evaluations away from the cancellation).  `box_mean_fp32` restates the kernel's own fp32 arithmetic (sequential sum, one division) in
numpy, for the consistency bound."""
import numpy as np
import torch

from oracle import diffusion_ref as D

import sampler_ref as S


def geometry(shape, cf, N):
    B, C, H, W = shape
    assert cf in (1, C) and N >= 1 and H % N == 0 and W % N == 0, (shape, cf, N)
    return B, C, H, W, C // cf, H // N, W // N


def A(x, cf, N):
    """The box mean in x's dtype (float64 for the restatement): [B, C, H, W] -> [B, C / cf, H / N, W / N]."""
    B, C, H, W, Cb, Hb, Wb = geometry(tuple(x.shape), cf, N)
    return x.reshape(B, Cb, cf, Hb, N, Wb, N).mean(dim=(2, 4, 6))


def A_pinv(u, cf, N):
    """Replication: [B, C / cf, H / N, W / N] -> [B, C, H, W]."""
    return u.repeat_interleave(cf, dim=1).repeat_interleave(N, dim=2).repeat_interleave(N, dim=3)


def project(x, obs, cf, N):
    """x + A+(obs - A x)"""
    return x + A_pinv(obs - A(x, cf, N), cf, N)


def box_index(shape, cf, N):
    """int64 [C, H, W]: the box (c', i, j), flattened over [C / cf, H / N, W / N], of every element of an image."""
    _, C, H, W, Cb, Hb, Wb = geometry((1,) + tuple(shape), cf, N)
    c, y, x = torch.meshgrid(torch.arange(C), torch.arange(H), torch.arange(W), indexing="ij")
    return ((c // cf) * Hb + y // N) * Wb + x // N


def box_mean_fp32(x, cf, N):
    """A x exactly as gmk_box_mean is defined to evaluate it: the sequential fp32 add, from 0, of a box's members in row-major (dc, dy, dx)
    order, then one fp32 division by k.  x: fp32 tensor -> fp32 numpy."""
    a = x.detach().cpu().numpy().astype(np.float32)
    B, C, H, W, Cb, Hb, Wb = geometry(a.shape, cf, N)
    m = a.reshape(B, Cb, cf, Hb, N, Wb, N).transpose(0, 1, 3, 5, 2, 4, 6).reshape(B, Cb, Hb, Wb, cf * N * N)
    s = np.zeros(m.shape[:-1], dtype=np.float32)
    for j in range(m.shape[-1]):
        s = (s + m[..., j]).astype(np.float32)
    return (s / np.float32(cf * N * N)).astype(np.float32)


def x_from_out(out, z, logsnr, mean_type):
    if mean_type == "v":
        return D.predict_x_from_v(z, out, logsnr)
    if mean_type == "eps":
        return D.predict_x_from_eps(z, out, logsnr)
    if mean_type == "x":
        return out
    raise NotImplementedError(mean_type)


def x_hat(out, z, logsnr, mean_type="v", out_uncond=None, w=None):
    """The samplers' data prediction (float64): clip(x(out)); guided e = (1 + w) eps(z, x_c) + (-w) eps(z, clip(x(out_uncond))),
    clip(x(z, e)) (gaussian_diffusion.py:58-79, :174-187).  out / z: [B, ...]; logsnr, w: [B]."""
    out, z, logsnr = out.double(), z.double(), logsnr.double()
    x = torch.clip(x_from_out(out, z, logsnr, mean_type), -1.0, 1.0)
    if out_uncond is None:
        return x
    e_c = D.predict_eps_from_x(z, x, logsnr)
    e_u = D.predict_eps_from_x(z, torch.clip(x_from_out(out_uncond.double(), z, logsnr, mean_type), -1.0, 1.0), logsnr)
    ww = D.bcast(w.double(), z.shape)
    return torch.clip(D.predict_x_from_eps(z, (1 + ww) * e_c + (-ww) * e_u, logsnr), -1.0, 1.0)


def residual(xh, obs, cf, N):
    """obs - A x_hat (float64)"""
    return obs.double() - A(xh.double(), cf, N)


def projected(xh, r, z, logsnr, cf, N):
    """(x_hat', eps_hat') = (x_hat + A+ r, eps(z, x_hat')), float64."""
    xp = xh.double() + A_pinv(r.double(), cf, N)
    return xp, D.predict_eps_from_x(z.double(), xp, logsnr.double())


def ddim_update(xp, ep, logsnr_s):
    a_s, s_s = S.alpha_sigma(logsnr_s)
    return a_s * xp + s_s * ep


def ancestral_update(xp, z, noise, logsnr_t, logsnr_s):
    """The ancestral posterior q(z_s | z_t, x) with x_logvar = 'large' (oracle.diffusion_ref.reverse_dpm_step's formulas), float64."""
    lt, ls = torch.as_tensor(float(logsnr_t), dtype=torch.float64), torch.as_tensor(float(logsnr_s), dtype=torch.float64)
    alpha_st = torch.sqrt((1.0 + torch.exp(-lt)) / (1.0 + torch.exp(-ls)))
    alpha_s = torch.sqrt(torch.sigmoid(ls))
    r = torch.exp(lt - ls)
    omr = -torch.expm1(lt - ls)
    return r * alpha_st * z.double() + omr * alpha_s * xp + torch.sqrt(omr * torch.sigmoid(-lt)) * noise.double()


def ancestral(predict, noises):
    """The ancestral update on `predict` with the injected noises[f].  -> step (tests/sampler_ref.py's convention)"""
    def step(z_t, logsnr_t, logsnr_s, f):
        xp, ep = predict(z_t, logsnr_t)
        return ancestral_update(xp, z_t, noises[f], logsnr_t, logsnr_s), xp, ep
    return step


def sample(params, init_x, obs, cf, N, guide, num_steps, sampler="ddim", cond_w=None, noises=None, mean_type="v", record=True):
    """The restoring chain on the samplers' time grid: sampler 'ddim', 'noisy' (noises[f], one per network evaluation) or 'dpmpp_2m' (the
    update of tests/dpm_solver_ref.py) on (x_hat', eps_hat'); the last step returns x_hat'.  cond_w: resolved per-sample guidance weights or
    None.  -> (zs, xs, es) float64 [T, B, ...] when `record`, else the final z."""
    oracle = S.oracle_predict(params, guide, cond_w, mean_type)

    def predict64(z_t, logsnr_t):
        lt = torch.broadcast_to(logsnr_t.reshape(()), (z_t.shape[0],))
        xh = oracle(z_t.float(), logsnr_t)[0].double()
        return projected(xh, residual(xh, obs, cf, N), z_t, lt, cf, N)
    if sampler == "ddim":
        step = S.ddim(predict64)
    elif sampler == "dpmpp_2m":
        step = S.dpmpp_2m(predict64)
    elif sampler == "noisy":
        step = ancestral(predict64, noises)
    else:
        raise NotImplementedError(sampler)
    return S.chain(init_x.double(), num_steps, step, record=record)


# ---- the learning check (tests/test_gpu_restore.py, tools/restore_probe.py) ---------------------------------------------------------------
# The two 1x28x28 images of tests/inpaint_ref.py (`two_modes`): their 4x4 box means differ everywhere, so a net trained on them alone has to
# return, from degrade(x_k), an image nearer to x_k than to the other one.
LEARNING_CHECK_FACTOR = 4


def restore_accuracy(model, per_mode=32, seed=0, factor=LEARNING_CHECK_FACTOR):
    """Restore `per_mode` copies of degrade(mode k) for both modes (label 0, initial noise from PhiloxStream(1000 + seed)) and draw as many
    unconditional samples from the same initial noise.  -> (fraction of restorations nearer (L2, the whole image) their own mode, fraction of
    the unconditional samples nearer mode 0)"""
    from functools import partial

    import inpaint_ref
    from generative_models_amd.diffusion.gaussian_diffusion import PhiloxStream
    modes = inpaint_ref.two_modes().cuda()
    x0 = modes.repeat_interleave(per_mode, 0)
    truth = torch.arange(2, device="cuda").repeat_interleave(per_mode)
    init = PhiloxStream(1000 + seed).normal(tuple(x0.shape), "cuda")
    net = partial(model._sampling_net(), guide=torch.zeros((x0.shape[0],), dtype=torch.long, device="cuda"))
    out = model.diffusion.restore(net=net, obs=model.degrade(x0, factor=factor), factor=factor, init_x=init)[0][-1]
    free = model.diffusion.sample(net=net, init_x=init, record=False)[0][-1]
    nearest = lambda s: ((s[:, None] - modes[None]) ** 2).flatten(2).sum(-1).argmin(1)
    return float((nearest(out) == truth).float().mean()), float((nearest(free) == 0).float().mean())
