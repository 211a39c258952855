"""Float64 restatement of the weighted x-space losses and the fp32 restatement of the stratified time rule (test infrastructure; written from
the definitions, not from the kernels).

Per image b, lambda = logsnr[b] (SNR = e^lambda), n values per image, alpha^2 = sigmoid(lambda), sigma^2 = sigmoid(-lambda):
  x_raw  = alpha z - sigma out ('v'),  sqrt(1 + e^-lambda) (z - out / sqrt(1 + e^lambda)) ('eps'),  out ('x')
  x_hat  = clip(x_raw, -1, 1),  m_b = mean_i (x_hat_i - x_i)^2
  loss_b = w(lambda) m_b,  w = 1 + e^lambda ('snr_plus1': Salimans & Ho 2022, section 4),  min(e^lambda, gamma) ('min_snr': Hang et al. 2023)
  dv_i   = grad_scale w (2 / n) (x_hat_i - x_i) d x_raw / d out  where -1 <= x_raw_i <= 1, else 0
           d x_raw / d out = -sigma ('v'), -sqrt(1 + e^-lambda) / sqrt(1 + e^lambda) ('eps'), 1 ('x')
Stratified times (Kingma et al. 2021, VDM, App. I.1): u_b = frac(u0 + b / B) as s = fl(b / B), c = fl(1 - s),
u_b = u0 >= c ? fl(u0 - c) : min(fl(u0 + s), 1 - 2^-24), every fl a correctly rounded fp32 operation.  (The wrap precedes the sum: fl(u0 + s) is
not exact at or above 1, where fp32 keeps multiples of 2^-23 - u0 = 1 - 2^-24, B = 8, b = 1 would round up to 1.125 and land in [1/8, 2/8).)
"""
import numpy as np

LAMBDAS = (-20.0, -3.0, 0.0, float(np.log(5.0)), 3.0, 20.0)      # the six log-SNRs of the tests: both ends of the schedule, both sides of ln 5
WEIGHTS = ("snr_plus1", "min_snr")
MEAN_TYPES = ("v", "eps", "x")


def _col(logsnr, ndim):
    return np.asarray(logsnr, dtype=np.float64).reshape((-1,) + (1,) * (ndim - 1))


def x_raw(out, z, logsnr, mean_type):
    """-> (x_raw, d x_raw / d out), float64; out, z [B, ...], logsnr [B]."""
    out, z = np.asarray(out, dtype=np.float64), np.asarray(z, dtype=np.float64)
    l = _col(logsnr, out.ndim)
    if mean_type == "v":
        alpha, sigma = np.sqrt(1.0 / (1.0 + np.exp(-l))), np.sqrt(1.0 / (1.0 + np.exp(l)))
        return alpha * z - sigma * out, -sigma * np.ones_like(out)
    if mean_type == "eps":
        d1, d2 = np.sqrt(1.0 + np.exp(-l)), 1.0 / np.sqrt(1.0 + np.exp(l))
        return d1 * (z - out * d2), -d1 * d2 * np.ones_like(out)
    if mean_type == "x":
        return out.copy(), np.ones_like(out)
    raise ValueError(mean_type)


def weight(logsnr, name, gamma):
    l = np.asarray(logsnr, dtype=np.float64)
    if name == "snr_plus1":
        return 1.0 + np.exp(l)
    if name == "min_snr":
        return np.minimum(np.exp(l), float(gamma))
    raise ValueError(name)


def x_loss_w(out, z, x, logsnr, name, gamma, grad_scale=1.0, mean_type="v"):
    """-> dict(loss_b [B], x_mse [B], dv (out's shape), clipped (bool, out's shape), x_raw), all float64."""
    x = np.asarray(x, dtype=np.float64)
    B = x.shape[0]
    n = x.size // B
    raw, dxo = x_raw(out, z, logsnr, mean_type)
    inside = (raw >= -1.0) & (raw <= 1.0)
    res = np.clip(raw, -1.0, 1.0) - x
    m = np.square(res).reshape(B, -1).mean(1)
    w = weight(logsnr, name, gamma)
    dv = np.where(inside, float(grad_scale) * _col(w, x.ndim) * (2.0 / n) * res * dxo, 0.0)
    return {"loss_b": w * m, "x_mse": m, "dv": dv, "clipped": ~inside, "x_raw": raw}


def u_stratified(u0, B):
    """fp32 [B]: the rule above in numpy float32 (each operation on float32 operands is correctly rounded)."""
    u0 = np.float32(u0)
    s = np.arange(B, dtype=np.float32) / np.float32(B)
    c = np.float32(1.0) - s
    lo, hi = u0 - c, np.minimum(u0 + s, np.float32(1.0 - 2.0 ** -24))
    assert s.dtype == c.dtype == lo.dtype == hi.dtype == np.float32
    return np.where(u0 >= c, lo, hi)


def loss_inputs(B, n, logsnr, mean_type, seed):
    """Test inputs of B images of n values at the given log-SNRs, fp32: x uniform in [-0.9, 0.9], eps normal, z = alpha x + sigma eps, and
    out = the exact target of the parameterisation moved so that x_raw = x + rho, rho of random sign with |rho| in [0.25, 1.25]: a good
    share of the raw predictions leaves [-1, 1], and every residual x_hat - x is at least 0.1.

    The float64 restatement is a fair judge of an fp32 evaluation to 1e-5 only where the formulas themselves are well conditioned in fp32;
    that is a property of gmk_v_loss's formulas (whose x_mse bits the new kernel has to reproduce), not of a kernel.  Three choices follow.
    (1) The perturbation is sized in x space, not in the output's: sized in the output's it would shrink to sigma rho = 4.5e-5 rho at
    lambda = 20, a residual of the size of x's own fp32 rounding.  (2) Where the map from out to x_raw amplifies by more than 16 ('eps' at
    lambda = -20: d x_raw / d out = -e^(-lambda / 2) = -2.2e4, so fp32 knows x_raw to 1e-3 only) |rho| is in [2.25, 3.25]: every prediction is
    clipped and x_hat is exactly +-1.  (3) A raw prediction within `margin` of +-1 could fall on the other side of the clip in fp32, where dv
    jumps between 0 and its full value: such an element gets 2 rho instead, which moves it outward by at least 0.25.
    -> (out, z, x, eps) as float32 arrays [B, n]"""
    rng = np.random.default_rng(seed)
    l = _col(logsnr, 2)
    x = rng.uniform(-0.9, 0.9, (B, n))
    eps = rng.standard_normal((B, n))
    alpha, sigma = np.sqrt(1.0 / (1.0 + np.exp(-l))), np.sqrt(1.0 / (1.0 + np.exp(l)))
    x32, eps32 = x.astype(np.float32), eps.astype(np.float32)
    z32 = (alpha * x32 + sigma * eps32).astype(np.float32)
    target = {"v": alpha * eps32 - sigma * x32, "eps": eps32.astype(np.float64), "x": x32.astype(np.float64)}[mean_type]
    dxo = x_raw(target, z32, logsnr, mean_type)[1]                  # d x_raw / d out, constant per image
    gain = np.abs(dxo)
    rho = (rng.uniform(0.25, 1.25, (B, n)) + np.where(gain > 16.0, 2.0, 0.0)) * rng.choice([-1.0, 1.0], (B, n))
    out32 = (target + rho / dxo).astype(np.float32)
    margin = 1e-3 * np.maximum(1.0, gain)
    for _ in range(4):
        raw, _ = x_raw(out32, z32, logsnr, mean_type)
        near = np.abs(np.abs(raw) - 1.0) < margin
        if not near.any():
            break
        out32 = np.where(near, (target + 2.0 * (out32 - target)).astype(np.float32), out32)
    raw, _ = x_raw(out32, z32, logsnr, mean_type)
    assert not (np.abs(np.abs(raw) - 1.0) < margin).any()
    return out32, z32, x32, eps32
