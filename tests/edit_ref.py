"""CPU restatement of `GaussianDiffusion.edit` (SDEdit, Meng et al. 2022) and of the latent interpolation of `GaussianDiffusion.interpolate`
(gmk_slerp) - test infrastructure.

    slerp    per image, float64: c = clamp(a.b / sqrt(|a|^2 |b|^2), -1, 1), theta = acos(c), s = sin(theta),
             out_k = (sin((1 - t_k) theta) a + sin(t_k theta) b) / s; where s < 1e-6 or c is not finite: (1 - t_k) a + t_k b
    noised   z_k = alpha x + sigma eps at logsnr(k / T), the fp32 log-SNR of the oracle's grid, alpha and sigma in float64
    chain    a sampler chain that starts part-way: its own loop over i = k-1 ... 0 on the oracle's time grid, driving the step constructors
             of tests/sampler_ref.py (`oracle_step`, and `repaint` for a masked edit: one merge per step, never a jump back)
The random draws are inputs, one entry per network evaluation f = 0 ... k-1: noises[f] (sampler 'noisy') and eps1[f] (the merge)."""
import torch

import sampler_ref as S
from oracle import diffusion_ref as D


def slerp(a, b, t):
    """a, b: [B, ...]; t: K numbers.  -> (out float64 [K, B, ...], c float64 [B])"""
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    af, bf = a.flatten(1), b.flatten(1)
    dot, na, nb = (af * bf).sum(1), (af * af).sum(1), (bf * bf).sum(1)
    c = (dot / torch.sqrt(na * nb)).clamp(-1.0, 1.0)                 # 0 / 0 stays NaN through the clamp
    theta = torch.acos(c)
    s = torch.sin(theta)
    lerp = ~(torch.isfinite(c) & (s >= 1e-6))
    col = lambda v: v.reshape((-1,) + (1,) * (a.dim() - 1))
    out = []
    for tk in t:
        tk = float(tk)
        wa = torch.where(lerp, torch.full_like(s, 1.0 - tk), torch.sin((1.0 - tk) * theta) / s)
        wb = torch.where(lerp, torch.full_like(s, tk), torch.sin(tk * theta) / s)
        out.append(col(wa) * a + col(wb) * b)
    return torch.stack(out), c


def lerp(a, b, t):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return torch.stack([(1.0 - float(tk)) * a + float(tk) * b for tk in t])


def grid_logsnr(i, num_steps):
    """(logsnr_t, logsnr_s) of loop iteration i, 0-dim fp32 tensors: the oracle's grid."""
    u_t, u_s = D.sampler_times(i, num_steps)
    return D.logsnr_schedule_cosine(torch.tensor(u_t)), D.logsnr_schedule_cosine(torch.tensor(u_s))


def noised(x, eps, start, num_steps):
    """z_k = alpha x + sigma eps at the logsnr_t of iteration k - 1, in float64."""
    alpha, sigma = S.alpha_sigma(grid_logsnr(start - 1, num_steps)[0])
    return alpha * x.double() + sigma * eps.double()


def chain(init_x, num_steps, start, step, merge=None, record=True):
    """The iterations i = start-1 ... 0 from init_x (z at logsnr(start / T)).  -> (zs, xs, es) stacked [start, B, ...] when `record`, else the
    final z.  The last step (i == 0) returns x_hat; `merge` (sampler_ref.repaint) follows every update and never re-noises."""
    z_t = init_x
    zs, xs, es = [], [], []
    for f, i in enumerate(range(start)[::-1]):
        logsnr_t, logsnr_s = grid_logsnr(i, num_steps)
        z_s, x_pred, eps_pred = step(z_t, logsnr_t, logsnr_s, f)
        z_t = x_pred if i == 0 else z_s
        if merge is not None:
            z_t = merge(z_t, i == 0, False, logsnr_t, logsnr_s, f)
        zs.append(z_t); xs.append(x_pred); es.append(eps_pred)
    if record:
        return torch.stack(zs), torch.stack(xs), torch.stack(es)
    return z_t


def sample(params, init_x, guide, num_steps, start, sampler="ddim", cond_w=None, noises=None, mean_type="v", x0=None, mask=None, eps1=None,
           record=True):
    """A truncated chain of `sampler` on the oracle's steps; with x0 / mask / eps1 the RePaint merge against x0 after every update."""
    step = S.oracle_step(params, guide, sampler, cond_w, mean_type, noises)
    merge = None if mask is None else S.repaint(x0, mask, eps1, None)
    return chain(init_x, num_steps, start, step, merge, record)


def edit(params, x, eps, guide, num_steps, start, sampler="ddim", cond_w=None, noises=None, mean_type="v", mask=None, eps1=None, record=True):
    """`GaussianDiffusion.edit` from its draws: eps (the forward noise), noises / eps1 per evaluation.  -> (z_k float64, the chain's result)"""
    z_k = noised(x, eps, start, num_steps)
    return z_k, sample(params, z_k.float(), guide, num_steps, start, sampler, cond_w, noises, mean_type, x0=x, mask=mask, eps1=eps1,
                       record=record)
