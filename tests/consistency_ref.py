"""Float64 restatement of consistency distillation's target and pseudo-Huber loss and of the multistep consistency sampler's update (test
infrastructure, not a test; written from the definitions, not from the kernels).

Notation: alpha(l) = sqrt(sigmoid(l)), sigma(l) = sqrt(sigmoid(-l)); x_hat(out, z, l) = clip(x_raw(out, z, l), -1, 1) with x_raw by mean_type
(tests/loss_weight_ref.x_raw); eps_from_x(z, x, l) = (z - alpha x) / sigma.

  target (Song et al. 2023, "Consistency Models", Algorithm 2), per image b:
    x*   = i_times[b] == 0 ? x_pred_teacher[b] : x_hat(v_tgt[b], z_s[b], logsnr_s[b])        (boundary condition: f(., t_min) = identity)
    eps* = eps_from_x(z_t[b], x*[b], logsnr_t[b])
  pseudo-Huber (Song & Dhariwal 2023, "Improved Techniques for Training Consistency Models"), n values per image:
    m_b = mean_j (x_hat_j - x_j)^2,  loss_b = sqrt(m_b + c^2) - c      (the paper's sqrt(|d|^2 + c_p^2) - c_p with c_p = c sqrt(n), over sqrt(n))
    dv_j = grad_scale (x_hat_j - x_j) / (n sqrt(m_b + c^2)) d x_raw / d out  where -1 <= x_raw_j <= 1, else 0
  sampler step t -> s (Algorithm 1):  z_next = is_last ? x_hat : alpha_s x_hat + sigma_s eps
"""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from loss_weight_ref import MEAN_TYPES, _col, loss_inputs, x_raw  # noqa: E402,F401

U24 = 2.0 ** -24                        # half an fp32 ulp of a value in [1, 2): the unit of the tests' bounds


def alpha_sigma(logsnr, ndim=1):
    """-> (alpha, sigma), float64, shaped to broadcast over [B, ...] tensors of `ndim` dimensions."""
    l = _col(logsnr, ndim)
    return np.sqrt(1.0 / (1.0 + np.exp(-l))), np.sqrt(1.0 / (1.0 + np.exp(l)))


def x_hat(out, z, logsnr, mean_type):
    return np.clip(x_raw(out, z, logsnr, mean_type)[0], -1.0, 1.0)


def eps_from_x(z, x, logsnr):
    z, x = np.asarray(z, dtype=np.float64), np.asarray(x, dtype=np.float64)
    alpha, sigma = alpha_sigma(logsnr, z.ndim)
    return (z - alpha * x) / sigma


def consistency_target(v_tgt, z_s, x_pred_teacher, z_t, logsnr_t, logsnr_s, i_times, mean_type="v"):
    """-> (x*, eps*), float64."""
    first = _col(np.asarray(i_times) == 0, np.asarray(z_t).ndim).astype(bool)
    xs = np.where(first, np.asarray(x_pred_teacher, dtype=np.float64), x_hat(v_tgt, z_s, logsnr_s, mean_type))
    return xs, eps_from_x(z_t, xs, logsnr_t)


def huber(m, c):
    """loss_b of a mean squared residual m."""
    return np.sqrt(np.asarray(m, dtype=np.float64) + float(c) ** 2) - float(c)


def x_loss_huber(out, z, x, logsnr, c, grad_scale=1.0, mean_type="v"):
    """-> dict(loss_b [B], x_mse [B], dv (out's shape), clipped (bool, out's shape)), all float64."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    n = x.size // B
    raw, dxo = x_raw(out, z, logsnr, mean_type)
    inside = (raw >= -1.0) & (raw <= 1.0)
    res = np.clip(raw, -1.0, 1.0) - x
    m = np.square(res).reshape(B, -1).mean(1)
    r = np.sqrt(m + float(c) ** 2)
    dv = np.where(inside, float(grad_scale) * res / (n * _col(r, x.ndim)) * dxo, 0.0)
    return {"loss_b": r - float(c), "x_mse": m, "dv": dv, "clipped": ~inside}


def consistency_step(x_pred, eps, logsnr_s, is_last):
    """z_next of one sampler step from the step's data prediction and its fresh noise; logsnr_s a scalar.  float64."""
    x_pred = np.asarray(x_pred, dtype=np.float64)
    if is_last:
        return x_pred.copy()
    l = float(logsnr_s)
    return math.sqrt(1.0 / (1.0 + math.exp(-l))) * x_pred + math.sqrt(1.0 / (1.0 + math.exp(l))) * np.asarray(eps, dtype=np.float64)


def target_inputs(B, n, logsnr_t, logsnr_s, seed):
    """fp32 test inputs [B, n] of the target kernel: v_tgt, z_s, x_pred_teacher (in [-1, 1]), z_t - values of order one, which is all an
    elementwise formula needs; some of x_hat(v_tgt, z_s) are clipped."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1.0, 1.0, (B, n))
    a_t, s_t = alpha_sigma(logsnr_t, 2)
    a_s, s_s = alpha_sigma(logsnr_s, 2)
    z_t = a_t * x + s_t * rng.standard_normal((B, n))
    z_s = a_s * x + s_s * rng.standard_normal((B, n))
    v_tgt = rng.standard_normal((B, n)) * 1.5
    x_pred = np.clip(x + 0.3 * rng.standard_normal((B, n)), -1.0, 1.0)
    return tuple(a.astype(np.float32) for a in (v_tgt, z_s, x_pred, z_t))
