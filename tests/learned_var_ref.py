"""Float64 restatement of the learned reverse-process variance (Nichol & Dhariwal 2021, "Improved DDPM", section 3.1) as gmk_hybrid_loss and
gmk_stochastic_step_lv define it (include/gmk.h), in torch on the CPU: test infrastructure, no kernel.

Per image with lt = logsnr_t, ls = logsnr_s >= lt, and per element with f = (nu + 1) / 2 (unclamped):
    D   = softplus(ls) - softplus(lt)                        logvar_large - logvar_small of diffusion_reverse
    g   = -expm1(lt - ls) e^ls
    d   = x_hat - x                                          x_hat the clipped prediction, a constant for the bound (stop-gradient)
    KL  = (f D + expm1(-f D) + e^(-f D) g d^2) / 2           normal_kl(q(z_s | z_t, x), p(z_s | z_t)), p's variance 'medium' with fraction f
    vlb = mean_i KL_i,  loss = simple + lambda vlb,  d nu = grad_scale lambda / n  D / 4  (1 - e^(-f D) (1 + g d^2))
The functions take the dtype of their inputs, so that the same closed form can be evaluated in fp32 (the error a device kernel may make) and in
float64 (the reference value).
"""
import math

import torch


def softplus(l):
    return torch.clamp(l, min=0.0) + torch.log1p(torch.exp(-l.abs()))


def pair_terms(lt, ls):
    """-> (D, g) of a batch of time pairs, lt / ls tensors of one shape."""
    return softplus(ls) - softplus(lt), -torch.expm1(lt - ls) * torch.exp(ls)


def coefs(l):
    """alpha, sigma and the four factors of predict_eps_from_x / predict_x_from_eps at log-SNR l."""
    el, eml = torch.exp(l), torch.exp(-l)
    return dict(alpha=torch.sqrt(1.0 / (1.0 + eml)), sigma=torch.sqrt(1.0 / (1.0 + el)), c1=torch.sqrt(1.0 + el), c2=1.0 / torch.sqrt(1.0 + eml),
                d1=torch.sqrt(1.0 + eml), d2=1.0 / torch.sqrt(1.0 + el))


def x_from_out(out, z, c, mean_type):
    if mean_type == "v":
        return c["alpha"] * z - c["sigma"] * out
    if mean_type == "eps":
        return c["d1"] * (z - out * c["d2"])
    assert mean_type == "x"
    return out


def kl_elem(f, D, g, d):
    """KL per element from the fraction f, the pair's (D, g) (broadcast) and the residual d = x_hat - x."""
    a = f * D
    return 0.5 * (a + torch.expm1(-a) + torch.exp(-a) * (g * (d * d)))


def dnu_elem(f, D, g, d, scale):
    """d (scale sum_i KL_i) / d nu_i: scale = grad_scale lambda / n."""
    a = f * D
    return scale * (0.25 * D) * (1.0 - torch.exp(-a) * (1.0 + g * (d * d)))


def hybrid_loss(v, nu, z, x, eps, lt, ls, lam, grad_scale=1.0, loss_type=0, mean_type="v"):
    """The whole of gmk_hybrid_loss in the dtype of the inputs: v, nu, z, x, eps [B, n]; lt, ls [B].
    -> dict(loss, vlb, frac, x_mse, eps_mse, dnu), dnu analytic."""
    B, n = v.shape
    c = {k: t[:, None] for k, t in coefs(lt).items()}
    xh = torch.clamp(x_from_out(v, z, c, mean_type), -1.0, 1.0)
    eh = c["c1"] * (z - xh * c["c2"])
    x_mse, eps_mse = ((xh - x) ** 2).mean(1), ((eh - eps) ** 2).mean(1)
    simple = eps_mse if loss_type == 1 else torch.maximum(x_mse, eps_mse)
    D, g = pair_terms(lt, ls)
    f = 0.5 * (nu + 1.0)
    d = (xh - x).detach()
    kl = kl_elem(f, D[:, None], g[:, None], d)
    vlb = kl.mean(1)
    return dict(loss=simple + lam * vlb, vlb=vlb, frac=f.mean(1), x_mse=x_mse, eps_mse=eps_mse,
                dnu=dnu_elem(f, D[:, None], g[:, None], d, grad_scale * lam / n))


def hybrid_grads_autograd(v, nu, z, x, eps, lt, ls, lam, grad_scale=1.0, loss_type=0, mean_type="v"):
    """(dv, dnu) of grad_scale sum_b loss_b through torch autograd, the bound's mean detached."""
    v = v.detach().clone().requires_grad_(True)
    nu = nu.detach().clone().requires_grad_(True)
    out = hybrid_loss(v, nu, z, x, eps, lt, ls, lam, grad_scale, loss_type, mean_type)
    (grad_scale * out["loss"].sum()).backward()
    return v.grad, nu.grad


def noise_scale(nu, coef_noise_small, half_delta):
    """The per-element noise multiplier of gmk_stochastic_step_lv."""
    return coef_noise_small * torch.exp((0.5 * (nu + 1.0)) * half_delta)


def reverse_moments(lt, ls, z_t, x):
    """Float64 mean and the 'small' / 'large' variances of q(z_s | z_t, x) in the closed forms of `stochastic_row` (Python floats in, out)."""
    sig = lambda l: 1.0 / (1.0 + math.exp(-l))
    r, omr = math.exp(lt - ls), -math.expm1(lt - ls)
    mean = r * math.sqrt((1.0 + math.exp(-lt)) / (1.0 + math.exp(-ls))) * z_t + omr * math.sqrt(sig(ls)) * x
    return mean, omr * sig(-ls), omr * sig(-lt)
