"""Float64 restatement of the stochastic samplers' coefficients and of one of their steps (test infrastructure, not a test; written from the
definitions, not from the host code or the kernel).

Notation: alpha(l) = sqrt(sigmoid(l)), sigma(l) = sqrt(sigmoid(-l)); a step goes from log-SNR lt to ls > lt; r = SNR(t) / SNR(s) = exp(lt - ls).

  ancestral (the posterior q(z_s | z_t, x) of a variance-preserving diffusion; Ho et al. 2020, eq. 6-7, in log-SNR form):
    mean = r (alpha_s / alpha_t) z_t + (1 - r) alpha_s x,   var_small = (1 - r) sigma_s^2,   var_large = (1 - r) sigma_t^2,
    var_medium(f) = var_large^f var_small^(1 - f)           (the interpolation in the log domain)
  DDIM with eta (Song et al. 2021, eq. 12 and 16):
    z_s = alpha_s x + sqrt(sigma_s^2 - c_n^2) eps_hat + c_n xi,  eps_hat = (z_t - alpha_t x) / sigma_t,  c_n = eta sqrt(var_small)
    sigma_s^2 - c_n^2 = sigma_s^2 (1 - eta^2 (1 - r)) = sigma_s^2 ((1 - eta)(1 + eta) + eta^2 r)        (the form without cancellation)
  SDE-DPM-Solver++(2M) (Lu et al. 2022), lambda = l / 2, h = lambda_s - lambda_t:
    z_s = (sigma_s / sigma_t) e^-h z_t + alpha_s (1 - e^-2h) D + sigma_s sqrt(1 - e^-2h) xi,  D = (1 + k) x - k x_prev,  k = h / (2 h_prev)
  one step:  z_s = is_last ? x : c_z z_t + c_x ((1 + k) x - k x_prev) + c_n xi
"""
import math

import numpy as np

U24 = 2.0 ** -24                        # half an fp32 ulp of a value in [1, 2): the unit of the tests' bounds
MEAN_TYPES = ("v", "eps", "x")
KINDS = ("ancestral", "ddim_eta", "sde_dpmpp_2m")


def alpha_sigma(l):
    l = float(l)
    return math.sqrt(1.0 / (1.0 + math.exp(-l))), math.sqrt(1.0 / (1.0 + math.exp(l)))


def frac_of(posterior_var):
    return {"small": 0.0, "large": 1.0}[posterior_var] if ":" not in posterior_var else float(posterior_var.split(":")[1])


def coefs(kind, lt, ls, frac=1.0, eta=0.0):
    """(c_z, c_x, c_n) of one step lt -> ls, float64.  A zero-length step is the identity."""
    lt, ls = float(lt), float(ls)
    if lt == ls:
        return 1.0, 0.0, 0.0
    (a_t, s_t), (a_s, s_s) = alpha_sigma(lt), alpha_sigma(ls)
    r, omr = math.exp(lt - ls), -math.expm1(lt - ls)
    if kind == "ancestral":
        return r * a_s / a_t, omr * a_s, math.sqrt(omr) * s_t ** frac * s_s ** (1.0 - frac)
    if kind == "ddim_eta":
        c_z = s_s * math.sqrt((1.0 - eta) * (1.0 + eta) + eta * eta * r) / s_t
        return c_z, a_s - a_t * c_z, eta * math.sqrt(omr) * s_s
    assert kind == "sde_dpmpp_2m", kind
    h = 0.5 * ls - 0.5 * lt
    return s_s / s_t * math.exp(-h), a_s * -math.expm1(-2.0 * h), s_s * math.sqrt(-math.expm1(-2.0 * h))


def second_order_k(grid):
    """k = h / (2 h_prev) per row of a grid [(i, lt, ls)] as a chain walks it: 0 on its first row, on i == 0 and after a zero-length step."""
    ks, h_prev = [], None
    for i, lt, ls in grid:
        h = 0.5 * (float(ls) - float(lt))
        ks.append(0.0 if (not h_prev or i == 0) else h / (2.0 * h_prev))
        h_prev = h
    return ks


def step(z, x_hat, xi, c_z, c_x, c_n, k=0.0, x_prev=None, is_last=False):
    """z_s of one step, float64 arrays; x_prev is read only when k != 0, xi only when c_n != 0 and not is_last."""
    x_hat = np.asarray(x_hat, dtype=np.float64)
    if is_last:
        return x_hat.copy()
    d = x_hat if k == 0.0 else (1.0 + k) * x_hat - k * np.asarray(x_prev, dtype=np.float64)
    out = c_z * np.asarray(z, dtype=np.float64) + c_x * d
    return out if c_n == 0.0 else out + c_n * np.asarray(xi, dtype=np.float64)


def step_bound(z, x_hat, xi, c_z, c_x, c_n, k=0.0, x_prev=None):
    """8 u (|c_z z| + |c_x| (|(1 + k) x_hat| + |k x_prev|) + |c_n xi|): the kernel rounds each coefficient once (from double), each product
    once and each sum once, at most 7 roundings on the path of any term, every one relative to a partial result no larger than the sum of the
    terms' magnitudes; 8 leaves the second-order terms (u^2) room."""
    z, x_hat, xi = (np.abs(np.asarray(t, dtype=np.float64)) for t in (z, x_hat, xi))
    prev = 0.0 if k == 0.0 else abs(k) * np.abs(np.asarray(x_prev, dtype=np.float64))
    return 8.0 * U24 * (abs(c_z) * z + abs(c_x) * (abs(1.0 + k) * x_hat + prev) + abs(c_n) * xi)
