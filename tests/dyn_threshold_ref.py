"""CPU restatement of dynamic thresholding (Saharia et al. 2022, Imagen, section 2.3; `GaussianDiffusion(dyn_threshold=p)`) - test infrastructure.

For one image of n values at network time logsnr_t, given 0 < p <= 1:
  1. x_raw, no clip anywhere: x_c = x(out) by mean type; guided e_c = eps(z, x_c), e_u = eps(z, x(out_uncond)), e = (1 + w) e_c + (-w) e_u,
     x_raw = x(z, e).
  2. q = a[lo] + frac (a[hi] - a[lo]), a = |x_raw| sorted ascending, pos = p (n - 1), lo = floor(pos), hi = min(lo + 1, n - 1), frac = pos - lo
     (torch.quantile's linear rule).
  3. s = max(1, q), x_hat = min(max(x_raw, -s), s) / s.
  4. eps_hat = eps(z, x_hat).
Everything here is float64 on the `predict_*` functions of oracle.diffusion_ref (steps 1 - 4, the DDIM and DPM-Solver++(2M) chains over
oracle.unet_ref.unet_forward), except `quantile_fp32`: step 2 in fp32 exactly as the kernel is defined to evaluate it, for the bit test."""
import math

import numpy as np
import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U

import sampler_ref as S


def x_from_out(out, z, logsnr, mean_type):
    if mean_type == "v":
        return D.predict_x_from_v(z, out, logsnr)
    if mean_type == "eps":
        return D.predict_x_from_eps(z, out, logsnr)
    if mean_type == "x":
        return out
    raise NotImplementedError(mean_type)


def x_raw(out, z, logsnr, mean_type="v", out_uncond=None, w=None):
    """Step 1 (float64).  out / z: [B, ...]; logsnr: [B]; out_uncond, w ([B]): the guided case."""
    out, z, logsnr = out.double(), z.double(), logsnr.double()
    x = x_from_out(out, z, logsnr, mean_type)
    if out_uncond is None:
        return x
    e_c = D.predict_eps_from_x(z, x, logsnr)
    e_u = D.predict_eps_from_x(z, x_from_out(out_uncond.double(), z, logsnr, mean_type), logsnr)
    ww = D.bcast(w.double(), z.shape)
    return D.predict_x_from_eps(z, (1 + ww) * e_c + (-ww) * e_u, logsnr)


def rank(p, n):
    """-> (lo, hi, pos - lo) of step 2, in double."""
    pos = float(p) * (n - 1)
    lo = int(math.floor(pos))
    return lo, min(lo + 1, n - 1), pos - lo


def quantile(x, p):
    """Step 2 per image in x's dtype (float64 for the restatement): x [B, ...] -> q [B]."""
    a = x.abs().flatten(1).sort(dim=1).values
    lo, hi, frac = rank(p, a.shape[1])
    return a[:, lo] + frac * (a[:, hi] - a[:, lo])


def quantile_fp32(x, p):
    """Step 2 as the kernel is defined to evaluate it: fp32 values, exact order statistics, frac rounded to fp32 and
    q = a[lo] + frac * (a[hi] - a[lo]) in fp32 in exactly this order.  x: fp32 [B, ...] -> (q, s) as fp32 numpy [B]."""
    a = np.sort(np.abs(x.detach().cpu().numpy().astype(np.float32).reshape(x.shape[0], -1)), axis=1)
    lo, hi, frac = rank(p, a.shape[1])
    frac = np.float32(frac)
    diff = (a[:, hi] - a[:, lo]).astype(np.float32)
    q = (a[:, lo] + (frac * diff).astype(np.float32)).astype(np.float32)
    return q, np.maximum(np.float32(1.0), q)


def threshold(xr, p, force_s=None):
    """Steps 2 and 3: -> (x_hat, s [B], q [B])."""
    q = quantile(xr, p)
    s = torch.clamp(q, min=1.0) if force_s is None else torch.full_like(q, float(force_s))
    sb = D.bcast(s, xr.shape)
    return torch.minimum(torch.maximum(xr, -sb), sb) / sb, s, q


def predict(out, z, logsnr, p, mean_type="v", out_uncond=None, w=None, force_s=None):
    """Steps 1 - 4 of one network evaluation: -> (x_hat, eps_hat, s, q), float64."""
    xr = x_raw(out, z, logsnr, mean_type, out_uncond, w)
    x_hat, s, q = threshold(xr, p, force_s)
    return x_hat, D.predict_eps_from_x(z.double(), x_hat, logsnr.double()), s, q


def sample(params, init_x, guide, num_steps, p, sampler="ddim", cond_w=None, mean_type="v", force_s=None, record=True):
    """The thresholded chain on the samplers' time grid: sampler 'ddim' (z_s = alpha_s x_hat + sigma_s eps_hat) or 'dpmpp_2m' (the update of
    tests/dpm_solver_ref.py on x_hat); the last step returns x_hat.  The network runs in fp32 as the oracle's does, the algebra in float64.
    cond_w: resolved per-sample guidance weights or None.  -> (zs, xs, es) float64 [T, B, ...] when `record`, else the final z."""
    def predict64(z_t, logsnr_t):
        lt = torch.broadcast_to(logsnr_t.reshape(()), (z_t.shape[0],))
        z32 = z_t.float()
        out = U.unet_forward(params, z32, lt, guide=guide)
        out_u = U.unet_forward(params, z32, lt, guide=-torch.ones_like(guide)) if cond_w is not None else None
        return predict(out, z_t, lt, p, mean_type, out_u, cond_w, force_s)[:2]
    if sampler not in ("ddim", "dpmpp_2m"):
        raise NotImplementedError(sampler)
    return S.chain(init_x.double(), num_steps, getattr(S, sampler)(predict64), record=record)
