"""CPU restatement of the guided samplers' two options (`GaussianDiffusion(guidance_interval=(lo, hi), cfg_rescale=phi)`) - test infrastructure.

The guidance interval (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and Distribution Quality in
Diffusion Models"): a step at network time logsnr_t is guided iff lo <= logsnr_t <= hi (None: every step).  The rescale (Lin et al. 2023,
"Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4) acts on guided steps only.  One network evaluation:
  outside the interval            the oracle's unguided prediction (`sampler_ref.oracle_predict` without a weight);
  inside, phi = 0                 the oracle's own guided prediction (`sampler_ref.oracle_predict`);
  inside, phi > 0                 x_c and x_raw = dyn_threshold_ref.x_raw without / with guidance (float64, no clip anywhere), per image
                                  f = 1 + phi (std(x_c) / std(x_raw) - 1), x_hat = clip(f x_raw, -1, 1), eps_hat = eps(z, x_hat).
The chains are `sampler_ref.chain` over the update rules `sampler_ref.ddim` / `sampler_ref.dpmpp_2m`, carried in float64; the network runs in
fp32 as the oracle's does."""
import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U

import dyn_threshold_ref as R
import sampler_ref as S


def inside(interval, logsnr_t):
    """Is a step at network time logsnr_t guided?"""
    return interval is None or float(interval[0]) <= float(logsnr_t) <= float(interval[1])


def ratio(x_c, x_raw):
    """std(x_c) / std(x_raw) per image, float64 [B]."""
    return x_c.double().flatten(1).std(dim=1, unbiased=False) / x_raw.double().flatten(1).std(dim=1, unbiased=False)


def factor(x_c, x_raw, phi):
    """f = 1 + phi (std(x_c) / std(x_raw) - 1) per image, float64 [B]."""
    return 1.0 + float(phi) * (ratio(x_c, x_raw) - 1.0)


def predict(out, z, logsnr, phi, mean_type, out_uncond, w):
    """The rescaled guided prediction of one network evaluation (phi > 0): -> (x_hat, eps_hat, f [B], ratio [B]), float64."""
    x_c = R.x_raw(out, z, logsnr, mean_type)
    x_r = R.x_raw(out, z, logsnr, mean_type, out_uncond, w)
    f = factor(x_c, x_r, phi)
    x_hat = torch.clamp(D.bcast(f, x_r.shape) * x_r, -1.0, 1.0)
    return x_hat, D.predict_eps_from_x(z.double(), x_hat, logsnr.double()), f, ratio(x_c, x_r)


def predictor(params, guide, cond_w, interval=None, phi=0.0, mean_type="v"):
    """-> predict(z_t, logsnr_t) -> (x_hat, eps_hat) in float64 for `sampler_ref.ddim` / `dpmpp_2m`.  cond_w: the resolved weights [B]."""
    unguided = S.oracle_predict(params, guide, None, mean_type)
    guided = S.oracle_predict(params, guide, cond_w, mean_type)

    def pred(z_t, logsnr_t):
        z32 = z_t.float()
        if not inside(interval, logsnr_t):
            x, e = unguided(z32, logsnr_t)
            return x.double(), e.double()
        if float(phi) == 0.0:
            x, e = guided(z32, logsnr_t)
            return x.double(), e.double()
        lt = torch.broadcast_to(logsnr_t.reshape(()), (z_t.shape[0],))
        out = U.unet_forward(params, z32, lt, guide=guide)
        out_u = U.unet_forward(params, z32, lt, guide=-torch.ones_like(guide))
        return predict(out, z_t, lt, phi, mean_type, out_u, cond_w)[:2]
    return pred


def sample(params, init_x, guide, num_steps, cond_w, interval=None, phi=0.0, sampler="ddim", mean_type="v", merge=None, resample=1,
           record=True):
    """The chain on the samplers' time grid: sampler 'ddim' or 'dpmpp_2m', `merge` / `resample` as `sampler_ref.chain` takes them (RePaint).
    -> (zs, xs, es) float64 [T, B, ...] when `record`, else the final z."""
    if sampler not in ("ddim", "dpmpp_2m"):
        raise NotImplementedError(sampler)
    step = getattr(S, sampler)(predictor(params, guide, cond_w, interval, phi, mean_type))
    return S.chain(init_x.double(), num_steps, step, merge, resample, record)


def grid(num_steps):
    """The network times of the chain's steps i = T-1 ... 0, as Python floats."""
    return [float(D.logsnr_schedule_cosine(torch.tensor(D.sampler_times(i, num_steps)[0]))) for i in range(num_steps)[::-1]]
