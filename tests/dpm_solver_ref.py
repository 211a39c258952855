"""CPU restatement of sampler='dpmpp_2m' (DPM-Solver++(2M), Lu et al. 2022, Algorithm 2, data prediction) - test infrastructure.

Built on the oracle's reference pieces: the prediction of each step is `run_model` (+ `cf_guidance`) exactly as the DDIM step forms it, on
DDIM's time grid (`sampler_times`, `logsnr_schedule_cosine`).  The solver's coefficients are computed here in float64 from the fp32
log-SNRs, independently of the package's `dpm_solver_coefs`:
    lambda = logsnr / 2, alpha = sqrt(sigmoid(logsnr)), sigma = sqrt(sigmoid(-logsnr)), h = lambda_s - lambda_t
    first step:  z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) x_hat
    later steps: D = (1 + 1/(2r)) x_hat - 1/(2r) x_hat_prev, r = h_prev / h;  z_s = (sigma_s / sigma_t) z_t - alpha_s expm1(-h) D
    last step:   z = x_hat
The recorded trajectory is (z, x_hat, eps_hat) - the prediction, not D."""
import math

import torch

from oracle import diffusion_ref as D


def _alpha_sigma(l):
    l = float(l)
    return math.sqrt(1.0 / (1.0 + math.exp(-l))), math.sqrt(1.0 / (1.0 + math.exp(l)))


def sample(params, init_x, guide, num_steps, cond_w=None, mean_type="v", record=True):
    """-> (zs, xs, es) stacked [T, B, ...] when `record`, else the final z.  `cond_w`: resolved per-sample guidance weights or None."""
    z_t = init_x
    zs, xs, es = [], [], []
    x_prev, h_prev = None, None
    B = init_x.shape[0]
    for i in range(num_steps)[::-1]:
        u_t, u_s = D.sampler_times(i, num_steps)
        logsnr_t = D.logsnr_schedule_cosine(torch.tensor(u_t))
        logsnr_s = D.logsnr_schedule_cosine(torch.tensor(u_s))
        lt = torch.broadcast_to(logsnr_t.reshape(()), (B,))
        out = D.run_model(params, z_t, lt, guide=guide, mean_type=mean_type)
        x_pred, eps_pred = out["model_x"], out["model_eps"]
        if cond_w is not None:
            x_pred, eps_pred = D.cf_guidance(params, z_t, eps_pred, lt, cond_w, guide, mean_type)
        (a_t, s_t), (a_s, s_s) = _alpha_sigma(logsnr_t), _alpha_sigma(logsnr_s)
        h = 0.5 * (float(logsnr_s) - float(logsnr_t))
        if x_prev is None:
            d = x_pred
        else:
            k = 1.0 / (2.0 * (h_prev / h))
            d = (1.0 + k) * x_pred - k * x_prev
        z_s = (s_s / s_t) * z_t + (-a_s * math.expm1(-h)) * d
        x_prev, h_prev = x_pred, h
        z_t = x_pred if i == 0 else z_s
        if record:
            zs.append(z_t); xs.append(x_pred); es.append(eps_pred)
    if record:
        return torch.stack(zs), torch.stack(xs), torch.stack(es)
    return z_t
