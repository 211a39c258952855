"""NumPy float64 restatement of post-hoc EMA (Karras et al. 2024, section 3.2 / appendix C), written from the definitions and not from
generative_models_amd/posthoc_ema.py: the gamma root, the discrete weight vector of a power-function average, a midpoint quadrature of the
profiles' inner products and the sequential double-precision combine."""
import math

import numpy as np


def sigma_rel(gamma):
    return math.sqrt(gamma + 1.0) / ((gamma + 2.0) * math.sqrt(gamma + 3.0))


def gamma_root(s):
    """Newton on f(gamma) = log sigma_rel(gamma) - log s from gamma = 1 / s^2 (the large-gamma limit), finished by a few secant-free
    bisection steps: f decreases monotonically, f' = 1 / (2 (gamma + 1)) - 1 / (gamma + 2) - 1 / (2 (gamma + 3))."""
    g = max(1.0 / (s * s) - 3.0, 0.5)
    for _ in range(100):
        f = math.log(sigma_rel(g)) - math.log(s)
        df = 0.5 / (g + 1.0) - 1.0 / (g + 2.0) - 0.5 / (g + 3.0)
        step = f / df
        g = max(g - step, 0.0)
        if abs(step) <= 1e-15 * max(g, 1.0):
            break
    return g


def weight(gamma, t):
    """1 - beta_t = 1 - (1 - 1/t)^(gamma + 1) through expm1 / log1p."""
    return 1.0 if t == 1 else -np.expm1((gamma + 1.0) * np.log1p(-1.0 / t))


def discrete_weights(gamma, T, length=None):
    """[length or T] float64: entry tau - 1 is the weight of theta(tau) in the average read at step T, w_tau prod_{s > tau} beta_s
    (zero past T)."""
    out = np.zeros(length or T, dtype=np.float64)
    tail = 1.0
    for tau in range(T, 0, -1):
        w = weight(gamma, tau)
        out[tau - 1] = w * tail
        tail *= 1.0 - w
    return out


def quadrature_dot(ga, ta, gb, tb, points=10 ** 6):
    """Midpoint rule for the integral over [0, min(ta, tb)] of p_a p_b, p(tau) = (gamma + 1) tau^gamma / t^(gamma + 1) = (gamma + 1) / t
    (tau / t)^gamma."""
    m = min(ta, tb)
    tau = (np.arange(points, dtype=np.float64) + 0.5) * (m / points)
    pa = (ga + 1.0) / ta * np.exp(ga * np.log(tau / ta))
    pb = (gb + 1.0) / tb * np.exp(gb * np.log(tau / tb))
    return float(np.sum(pa * pb) * (m / points))


def combine(rows, coef):
    """fp32 [n]: acc = coef[0] row_0, then acc = acc + coef[k] row_k in index order, all in float64 (NumPy rounds the product and the sum
    separately), rounded once to float32.  rows: float32 [K][n]."""
    rows = np.asarray(rows, dtype=np.float32)
    coef = np.asarray(coef, dtype=np.float64)
    acc = coef[0] * rows[0].astype(np.float64)
    for k in range(1, rows.shape[0]):
        acc = acc + coef[k] * rows[k].astype(np.float64)
    return acc.astype(np.float32)
