"""Float64 CPU restatement of the continuous-time variational bound (`GaussianDiffusion.nll`; Kingma et al. 2021, VDM eq. 17 with the
log-SNR lambda as the variable) from given draws, and its closed form for a network whose output is identically zero - test infrastructure.

    lambda in [-20, 20], Delta = 40, alpha^2 = sigmoid(lambda), sigma^2 = sigmoid(-lambda), D = C H W
    lambda_{b,k} = 20 - Delta frac(u0_b + k / K);  z = alpha x + sigma eps_k
    eps_hat: 'v' sigma z + alpha out,  'eps' out,  'x' (z - alpha out) / sigma     (the network output, unclipped)
    diffusion = mean_k 1/2 Delta |eps_k - eps_hat_k|^2
    prior     = sum_i 1/2 (alpha_1^2 x_i^2 - alpha_1^2 - log1p(-alpha_1^2)),   lambda_1 = -20
    decoder   = sum_i -log[Phi((x + delta - m) / s) - Phi((x - delta - m) / s)],  m = z_0 / alpha_0, s = sigma_0 / alpha_0,
                z_0 = alpha_0 x + sigma_0 eps_0, lambda_0 = 20; the top bin's upper edge +inf, the bottom bin's lower edge -inf
    nlogp     = (prior + decoder + diffusion) / D, se = std_k(1/2 Delta |eps_k - eps_hat_k|^2) / sqrt(K) / D

The decoder is computed literally from z_0 here (float64 leaves its cancellation at ~1e-12 of a bin); the kernel uses (x - m) / s = -eps_0."""
import math

import torch

LMAX, LMIN = 20.0, -20.0
DELTA_L = LMAX - LMIN


def _d(t):
    return torch.as_tensor(t).double()


def logsnr_strata(u0, K):
    """float64 [K, B]"""
    k = torch.arange(K, dtype=torch.float64)[:, None] / K
    return LMAX - DELTA_L * torch.remainder(_d(u0)[None, :] + k, 1.0)


def _coef(logsnr, shape):
    l = _d(logsnr).reshape((-1,) + (1,) * (len(shape) - 1))
    return torch.sqrt(torch.sigmoid(l)), torch.sqrt(torch.sigmoid(-l))


def q_sample(x, eps, logsnr):
    a, s = _coef(logsnr, x.shape)
    return a * _d(x) + s * _d(eps)


def eps_hat(out, z, logsnr, mean_type):
    out, z = _d(out), _d(z)
    a, s = _coef(logsnr, z.shape)
    if mean_type == "v":
        return s * z + a * out
    if mean_type == "eps":
        return out
    if mean_type == "x":
        return (z - a * out) / s
    raise ValueError(mean_type)


def sq_err(out, z, eps, logsnr, mean_type):
    """float64 [B]: sum over each image of (eps - eps_hat)^2"""
    d = _d(eps) - eps_hat(out, z, logsnr, mean_type)
    return (d * d).flatten(1).sum(1)


def _log_bin_mass(a, b):
    """log(Phi(a) - Phi(b)), a > b elementwise (+-inf allowed), through log_ndtr on the side away from 1"""
    up = b > 0                                   # both edges in the upper tail: Phi(a) - Phi(b) = Phi(-b) - Phi(-a)
    hi = torch.where(up, -b, a)
    lo = torch.where(up, -a, b)
    lh, ll = torch.special.log_ndtr(hi), torch.special.log_ndtr(lo)
    return lh + torch.log1p(-torch.exp(ll - lh))


def endpoints(x, eps0, delta, lo=None, logsnr_max=LMAX, logsnr_min=LMIN):
    """-> (prior [B], decoder [B]) in nats per image.  lo: the data's lowest value (default: 0 for delta = 1/2, else -1); the highest is 1.
    logsnr_max / logsnr_min: the end points (the bound's are 20 / -20; other values make the edges matter in tests)."""
    x, eps0 = _d(x), _d(eps0)
    lo = (0.0 if delta == 0.5 else -1.0) if lo is None else lo
    a2 = 1.0 / (1.0 + math.exp(-logsnr_min))
    prior = (0.5 * (a2 * x * x - a2 - math.log1p(-a2))).flatten(1).sum(1)
    a0, s0 = math.sqrt(1.0 / (1.0 + math.exp(-logsnr_max))), math.sqrt(1.0 / (1.0 + math.exp(logsnr_max)))
    z0 = a0 * x + s0 * eps0
    m, s = z0 / a0, s0 / a0
    up = torch.where(x > 1.0 - delta, torch.full_like(x, math.inf), (x + delta - m) / s)
    dn = torch.where(x < lo + delta, torch.full_like(x, -math.inf), (x - delta - m) / s)
    dec = (-_log_bin_mass(up, dn)).flatten(1).sum(1)
    return prior, dec


def estimate(x, u0, eps, eps0, forward, delta, mean_type="v"):
    """The bound from given draws.  eps: [K, B, ...]; forward(z, logsnr) -> network output (any dtype; z float64 [B, ...], logsnr float64 [B]).
    -> dict of float64 [B] per dimension: nlogp, se, diffusion, prior, decoder."""
    K, B = eps.shape[0], x.shape[0]
    D = x[0].numel()
    lam = logsnr_strata(u0, K)
    vals = []
    for k in range(K):
        z = q_sample(x, eps[k], lam[k])
        vals.append(0.5 * DELTA_L * sq_err(forward(z, lam[k]), z, eps[k], lam[k], mean_type))
    vals = torch.stack(vals)
    prior, dec = endpoints(x, eps0, delta)
    diff = vals.mean(0)
    se = vals.std(0) / math.sqrt(K) if K > 1 else torch.full((B,), math.nan, dtype=torch.float64)
    return {"nlogp": (prior + dec + diff) / D, "se": se / D, "diffusion": diff / D, "prior": prior / D, "decoder": dec / D}


def zero_output_integrand(lam, x):
    """1/2 E_eps |eps - eps_hat|^2 at log-SNR lam for a 'v' network with output 0: eps - eps_hat = alpha (alpha eps - sigma x), so
    E = alpha^2 (alpha^2 D + sigma^2 |x|^2).  x: one image; float64."""
    x = _d(x)
    a2 = 1.0 / (1.0 + math.exp(-lam))
    return 0.5 * a2 * (a2 * x.numel() + (1.0 - a2) * float((x * x).sum()))


def zero_output_diffusion(x):
    """E[diffusion term] per image, nats: 1/2 [D (softplus(l) - sigmoid(l)) + |x|^2 sigmoid(l)] from l = -20 to 20 (an antiderivative of
    `zero_output_integrand`).  x: [B, ...] -> float64 [B]."""
    x = _d(x)
    D = x[0].numel()
    sp = lambda l: math.log1p(math.exp(l)) if l < 30 else l + math.log1p(math.exp(-l))
    sg = lambda l: 1.0 / (1.0 + math.exp(-l))
    F = lambda l, x2: 0.5 * (D * (sp(l) - sg(l)) + x2 * sg(l))
    x2 = (x * x).flatten(1).sum(1)
    return torch.tensor([F(LMAX, float(v)) - F(LMIN, float(v)) for v in x2], dtype=torch.float64)
