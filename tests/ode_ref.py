"""Float64 CPU restatement of the probability-flow ODE of `GaussianDiffusion.encode / decode / ode_nll` (Song et al. 2021, section 4.3 and
App. D.2, in the log-SNR lambda) from given draws - test infrastructure.  It takes the network as two callables:

    forward(z, lam) -> out                 the network output at (z, lambda), z float64 [B, ...], lam a float
    vjp(z, lam, r)  -> g = (d out / d z)^T r

    alpha^2 = sigmoid(lambda), sigma^2 = sigmoid(-lambda), D = C H W
    eps_hat: 'v' sigma z + alpha out,  'eps' out,  'x' (z - alpha out) / sigma     (unclipped)
    x_hat:   'v' alpha z - sigma out,  'eps' (z - sigma out) / alpha,  'x' out       (= (z - sigma eps_hat) / alpha)
    grid     lambda_i = -2 log tan(a i / N + b), i = 0 ... N (lambda_0 = 20, lambda_N = -20), or the caller's
    update   z_j = alpha_j x_hat_i + sigma_j eps_hat_i   (j = i + 1 encoding, i - 1 decoding)
    d_i      = 1/2 sigma_i^2 D - 1/2 sigma_i (c_z D + c_o r_i . g_i),  (c_z, c_o) = (sigma, alpha) 'v', (0, 1) 'eps', (1/sigma, -alpha/sigma) 'x'
    log p(y) = log N(z_N; 0, I) - sum_{i<N} 1/2 (lambda_i - lambda_{i+1}) (d_i + d_{i+1}),   y = x + delta (2 u - 1)
    nlogp    = -log p(y) / D - log(2 delta)

Draws (`GaussianDiffusion.ode_nll`): u [B, ...] uniform in [0, 1), then one probe per evaluation i = 0 ... N, r = +1 where its uniform is
>= 1/2, else -1 (`rademacher`)."""
import math

import torch

LMAX, LMIN = 20.0, -20.0
SCHED_B = math.atan(math.exp(-0.5 * LMAX))
SCHED_A = math.atan(math.exp(-0.5 * LMIN)) - SCHED_B


def _d(t):
    return torch.as_tensor(t).double()


def logsnr_grid(N):
    return [-2.0 * math.log(math.tan(SCHED_A * i / N + SCHED_B)) for i in range(N + 1)]


def coef(lam):
    """-> (alpha, sigma) as floats"""
    return math.sqrt(1.0 / (1.0 + math.exp(-lam))), math.sqrt(1.0 / (1.0 + math.exp(lam)))


def predictions(out, z, lam, mean_type):
    """-> (x_hat, eps_hat), unclipped"""
    out, z = _d(out), _d(z)
    a, s = coef(lam)
    if mean_type == "v":
        return a * z - s * out, s * z + a * out
    if mean_type == "eps":
        return (z - s * out) / a, out
    if mean_type == "x":
        return out, (z - a * out) / s
    raise ValueError(mean_type)


def update(out, z, lam_i, lam_j, mean_type):
    xh, eh = predictions(out, z, lam_i, mean_type)
    a, s = coef(lam_j)
    return a * xh + s * eh


def divergence(lam, r, g, mean_type):
    """float64 [B]: d_i per image"""
    r, g = _d(r), _d(g)
    D = r[0].numel()
    a, s = coef(lam)
    cz, co = {"v": (s, a), "eps": (0.0, 1.0), "x": (1.0 / s, -a / s)}[mean_type]
    return 0.5 * s * s * D - 0.5 * s * (cz * D + co * (r * g).flatten(1).sum(1))


def trapezoid_weights(lam):
    N = len(lam) - 1
    return [0.5 * ((lam[i - 1] - lam[i] if i > 0 else 0.0) + (lam[i] - lam[i + 1] if i < N else 0.0)) for i in range(N + 1)]


def log_normal(z):
    """float64 [B]: log N(z; 0, I) per image"""
    z = _d(z).flatten(1)
    return -0.5 * (z * z).sum(1) - 0.5 * z.shape[1] * math.log(2.0 * math.pi)


def rademacher(u):
    return torch.where(_d(u) >= 0.5, 1.0, -1.0).double()


def encode(forward, x, N, mean_type, lam=None):
    lam = logsnr_grid(N) if lam is None else lam
    z = _d(x).clone()
    for i in range(N):
        z = update(forward(z, lam[i]), z, lam[i], lam[i + 1], mean_type)
    return z


def decode(forward, z, N, mean_type, lam=None):
    lam = logsnr_grid(N) if lam is None else lam
    z = _d(z).clone()
    for i in range(N, 1, -1):
        z = update(forward(z, lam[i]), z, lam[i], lam[i - 1], mean_type)
    return predictions(forward(z, lam[1]), z, lam[1], mean_type)[0]


def ode_nll(forward, vjp, x, N, u, probes, delta, mean_type, lam=None):
    """u: x's shape, uniform draws; probes: N + 1 tensors of x's shape (+-1).  -> dict of float64 [B]: nlogp, prior, divergence (per dimension)
    and z_N"""
    lam = logsnr_grid(N) if lam is None else lam
    w = trapezoid_weights(lam)
    x = _d(x)
    D = x[0].numel()
    z = x + delta * (2.0 * _d(u) - 1.0)
    acc = torch.zeros(x.shape[0], dtype=torch.float64)
    for i in range(N + 1):
        out = forward(z, lam[i])
        r = _d(probes[i])
        acc = acc + w[i] * divergence(lam[i], r, vjp(z, lam[i], r), mean_type)
        if i < N:
            z = update(out, z, lam[i], lam[i + 1], mean_type)
    prior = -log_normal(z)
    return {"nlogp": (prior + acc) / D - math.log(2.0 * delta), "prior": prior / D, "divergence": acc / D, "z": z}
