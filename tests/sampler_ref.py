"""The samplers' chain loop, restated once on the CPU - test infrastructure behind the `sample` of dpm_solver_ref, inpaint_ref and
dyn_threshold_ref.  `chain` walks the oracle's time grid (`sampler_times`, `logsnr_schedule_cosine`) with a step
step(z_t, logsnr_t, logsnr_s, f) -> (z_s, x_hat, eps_hat), f the network evaluation's index - the oracle's own `ddim_step` / `reverse_dpm_step`
(prediction and update in one, fp32), or an update rule (`ddim`, `dpmpp_2m`) on a prediction (`oracle_predict`: `run_model` + `cf_guidance`,
fp32; or dyn_threshold_ref's float64 one) - and an optional merge after every evaluation (`repaint`).
Every coefficient is computed here in float64 from the fp32 log-SNRs, independently of the package's `dpm_solver_coefs` / `inpaint_coefs`."""
import math

import torch

from oracle import diffusion_ref as D


def alpha_sigma(l):
    """-> (alpha, sigma) = (sqrt(sigmoid(l)), sqrt(sigmoid(-l))) in float64."""
    l = float(l)
    return math.sqrt(1.0 / (1.0 + math.exp(-l))), math.sqrt(1.0 / (1.0 + math.exp(l)))


def oracle_predict(params, guide, cond_w=None, mean_type="v"):
    """-> predict(z_t, logsnr_t) -> (x_hat, eps_hat), exactly as the oracle's DDIM step forms them."""
    def predict(z_t, logsnr_t):
        lt = torch.broadcast_to(logsnr_t.reshape(()), (z_t.shape[0],))
        out = D.run_model(params, z_t, lt, guide=guide, mean_type=mean_type)
        x_pred, eps_pred = out["model_x"], out["model_eps"]
        if cond_w is not None:
            x_pred, eps_pred = D.cf_guidance(params, z_t, eps_pred, lt, cond_w, guide, mean_type)
        return x_pred, eps_pred
    return predict


def ddim(predict):
    """The update z_s = alpha_s x_hat + sigma_s eps_hat on `predict`.  -> step"""
    def step(z_t, logsnr_t, logsnr_s, f):
        x_hat, eps_hat = predict(z_t, logsnr_t)
        a_s, s_s = alpha_sigma(logsnr_s)
        return a_s * x_hat + s_s * eps_hat, x_hat, eps_hat
    return step


def dpmpp_2m(predict):
    """The DPM-Solver++(2M) update on `predict` (the formulas: tests/dpm_solver_ref.py); it keeps the previous x_hat and h of its chain.  -> step"""
    x_prev, h_prev = None, None

    def step(z_t, logsnr_t, logsnr_s, f):
        nonlocal x_prev, h_prev
        x_hat, eps_hat = predict(z_t, logsnr_t)
        (a_t, s_t), (a_s, s_s) = alpha_sigma(logsnr_t), alpha_sigma(logsnr_s)
        h = 0.5 * (float(logsnr_s) - float(logsnr_t))
        if x_prev is None:
            d = x_hat
        else:
            k = 1.0 / (2.0 * (h_prev / h))
            d = (1.0 + k) * x_hat - k * x_prev
        x_prev, h_prev = x_hat, h
        return (s_s / s_t) * z_t + (-a_s * math.expm1(-h)) * d, x_hat, eps_hat
    return step


def oracle_step(params, guide, sampler, cond_w=None, mean_type="v", noises=None):
    """The fp32 step of `sampler`: 'ddim' / 'noisy' (noises[f]) are the oracle's, 'dpmpp_2m' the solver on the oracle's prediction."""
    if sampler == "ddim":
        return lambda z_t, lt, ls, f: D.ddim_step(params, lt, ls, z_t, guide, cond_w, mean_type)
    if sampler == "noisy":
        return lambda z_t, lt, ls, f: D.reverse_dpm_step(params, lt, ls, z_t, noises[f], guide, cond_w, mean_type)
    if sampler == "dpmpp_2m":
        return dpmpp_2m(oracle_predict(params, guide, cond_w, mean_type))
    raise NotImplementedError(sampler)


def repaint(x0, mask, eps1, eps2):
    """RePaint's merge after the update of evaluation f (the formulas: tests/inpaint_ref.py).  -> merge"""
    known_px = torch.broadcast_to(mask.bool(), x0.shape)

    def merge(z, is_last, renoise, logsnr_t, logsnr_s, f):
        (a_t, s_t), (a_s, s_s) = alpha_sigma(logsnr_t), alpha_sigma(logsnr_s)
        z = torch.where(known_px, x0 if is_last else a_s * x0 + s_s * eps1[f], z)
        if renoise:
            a = a_t / a_s
            z = a * z + math.sqrt(1.0 - a * a) * eps2[f]
        return z
    return merge


def chain(init_x, num_steps, step, merge=None, resample=1, record=True):
    """-> (zs, xs, es) stacked [T, B, ...] when `record` - the (z, x_hat, eps_hat) of the last pass of each step - else the final z.
    Every step runs `resample` passes, all but its last re-noised by the merge; the last step (i == 0) runs once and returns x_hat."""
    z_t = init_x
    zs, xs, es = [], [], []
    f = 0
    for i in range(num_steps)[::-1]:
        u_t, u_s = D.sampler_times(i, num_steps)
        logsnr_t = D.logsnr_schedule_cosine(torch.tensor(u_t))
        logsnr_s = D.logsnr_schedule_cosine(torch.tensor(u_s))
        npass = 1 if i == 0 else resample
        for p in range(npass):
            z_s, x_pred, eps_pred = step(z_t, logsnr_t, logsnr_s, f)
            z_t = x_pred if i == 0 else z_s
            if merge is not None:
                z_t = merge(z_t, i == 0, p < npass - 1, logsnr_t, logsnr_s, f)
            f += 1
        if record:
            zs.append(z_t); xs.append(x_pred); es.append(eps_pred)
    if record:
        return torch.stack(zs), torch.stack(xs), torch.stack(es)
    return z_t
