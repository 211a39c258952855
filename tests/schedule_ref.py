"""The closed-form log-SNR schedules (reference gms/diffusion/diffusion_utils.py:169-201), restated for the tests - test infrastructure.

Written from the formulas, independently of the package's `Schedule`: u in [0, 1] -> logsnr, u = 0 the top of the range,
    cosine       -2 log(tan(a u + b))      b = atan(exp(-lmax / 2)),  a = atan(exp(-lmin / 2)) - b
    uniform      lmin u + lmax (1 - u)
    beta_const   -log(expm1(a u + b))      b = softplus(-lmax),       a = softplus(-lmin) - b
    beta_linear  -log(expm1(a u^2 + b))    as beta_const
then + shift.  `logsnr64` is that in float64; `logsnr32` goes step by step in fp32 the way the reference's fp32 torch tensors do (a, b formed in
float64 and rounded to fp32, then one fp32 operation after another, the shift skipped when it is 0).  `chain` walks a schedule's sampler grid
with the CPU restatements of the samplers (tests/sampler_ref.py), and `dpm_rows` / `inpaint_rows` are the float64 formulas of the
coefficient tables on given log-SNRs."""
import math
import os

import numpy as np
import torch

KINDS = ("cosine", "uniform", "beta_const", "beta_linear")
RANGES = ((-20.0, 20.0), (-15.0, 15.0), (-10.0, 20.0))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "logsnr_schedules.npz")
F = np.float32


def golden_key(kind, lmin, lmax):
    num = lambda v: f"{v:g}".replace("-", "m")
    return f"{kind}_{num(lmin)}_{num(lmax)}"


def load_golden():
    return np.load(GOLDEN, allow_pickle=False)


def coefs64(kind, lmin, lmax):
    """-> (a, b) in float64 (0, 0 for 'uniform', which has none)."""
    softplus = lambda x: np.logaddexp(x, 0.0)
    if kind == "cosine":
        b = np.arctan(np.exp(-0.5 * lmax))
        return np.arctan(np.exp(-0.5 * lmin)) - b, b
    if kind in ("beta_const", "beta_linear"):
        b = softplus(-lmax)
        return softplus(-lmin) - b, b
    assert kind == "uniform", kind
    return 0.0, 0.0


def logsnr64(kind, lmin, lmax, shift, u):
    u = np.asarray(u, dtype=np.float64)
    a, b = coefs64(kind, lmin, lmax)
    if kind == "cosine":
        l = -2.0 * np.log(np.tan(a * u + b))
    elif kind == "uniform":
        l = lmin * u + lmax * (1.0 - u)
    else:
        l = -np.log(np.expm1(a * (u * u if kind == "beta_linear" else u) + b))
    return l + shift


def logsnr32(kind, lmin, lmax, shift, u):
    """fp32 in, fp32 out; every intermediate is rounded to fp32 (numpy float32 arithmetic)."""
    u = np.asarray(u, dtype=F)
    a, b = (F(c) for c in coefs64(kind, lmin, lmax))
    if kind == "cosine":
        t = (a * u).astype(F) + b
        l = F(-2.0) * np.log(np.tan(t.astype(F)).astype(F)).astype(F)
    elif kind == "uniform":
        l = (F(lmin) * u).astype(F) + (F(lmax) * (F(1.0) - u).astype(F)).astype(F)
    else:
        w = (u * u).astype(F) if kind == "beta_linear" else u
        t = (a * w).astype(F) + b
        l = -np.log(np.expm1(t.astype(F)).astype(F)).astype(F)
    l = l.astype(F)
    return (l + F(shift)).astype(F) if shift != 0 else l


def sampler_times(i, T):
    """(u_t, u_s) of loop iteration i, fp32 (reference gaussian_diffusion.py:288-290)."""
    return F(F(i + 1.0) / F(T)), F(F(i) / F(T))


def grid(kind, lmin, lmax, shift, T):
    """[(i, logsnr_t, logsnr_s)] for i = T-1 ... 0, fp32 scalars."""
    return [(i, *(logsnr32(kind, lmin, lmax, shift, u)[()] for u in sampler_times(i, T))) for i in range(T)[::-1]]


def chain(sched, init_x, num_steps, step, start=None, record=True):
    """tests/sampler_ref.py's `chain` on the grid of `sched` = (kind, lmin, lmax, shift): the iterations i = start-1 ... 0 (start None: all)
    with step(z_t, logsnr_t, logsnr_s, f) -> (z_s, x_hat, eps_hat); the last one returns x_hat.  -> (zs, xs, es) stacked, or the final z."""
    z_t = init_x
    zs, xs, es = [], [], []
    rows = grid(*sched, num_steps)
    rows = rows if start is None else rows[num_steps - start:]
    for f, (i, lt, ls) in enumerate(rows):
        z_s, x_pred, eps_pred = step(z_t, torch.tensor(lt), torch.tensor(ls), f)
        z_t = x_pred if i == 0 else z_s
        if record:
            zs.append(z_t); xs.append(x_pred); es.append(eps_pred)
    return (torch.stack(zs), torch.stack(xs), torch.stack(es)) if record else z_t


def q_sample64(x, eps, logsnr):
    """z = x sqrt(sigmoid(l)) + eps sqrt(sigmoid(-l)) in float64; logsnr [B] broadcast over the image dimensions."""
    l = torch.as_tensor(np.asarray(logsnr, dtype=np.float64)).reshape((-1,) + (1,) * (x.dim() - 1))
    return x.double() * torch.sqrt(torch.sigmoid(l)) + eps.double() * torch.sqrt(torch.sigmoid(-l))


def dpm_rows(rows):
    """DPM-Solver++(2M)'s per-step (h, coef_z, coef_x, coef_prev) in float64 on grid rows (i, lt, ls), by `dpm_solver_coefs`'s docstring:
    h = (ls - lt) / 2, coef_z = sigma_s / sigma_t, coef_x = -alpha_s expm1(-h), coef_prev = h / (2 h_prev), 0 on the first and on the last."""
    sigma = lambda l: math.sqrt(1.0 / (1.0 + math.exp(l)))
    alpha = lambda l: math.sqrt(1.0 / (1.0 + math.exp(-l)))
    out, h_prev = [], None
    for n, (i, lt, ls) in enumerate(rows):
        lt, ls = float(lt), float(ls)
        h = 0.5 * (ls - lt)
        k = 0.0 if (n == 0 or i == 0 or not h_prev) else h / (2.0 * h_prev)
        out.append((h, sigma(ls) / sigma(lt), -alpha(ls) * math.expm1(-h), k))
        h_prev = h
    return out


def inpaint_rows(rows):
    """RePaint's per-step (alpha_s, sigma_s, a, b) in float64 on grid rows, by `inpaint_coefs`'s docstring: a = alpha_t / alpha_s,
    b^2 = 1 - a^2."""
    sig = lambda l: 1.0 / (1.0 + math.exp(-l))
    out = []
    for i, lt, ls in rows:
        lt, ls = float(lt), float(ls)
        a = math.sqrt(sig(lt) / sig(ls))
        out.append((math.sqrt(sig(ls)), math.sqrt(sig(-ls)), a, math.sqrt(max(0.0, 1.0 - a * a))))
    return out
