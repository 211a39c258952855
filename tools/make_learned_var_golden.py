"""Golden vectors of the learned reverse-process variance (test infrastructure; needs a checkout of the reference).

Imports the reference's `get_logsnr_schedule`, `diffusion_reverse` and `normal_kl` (gms/diffusion/diffusion_utils.py) at generation time only
- nothing of the reference is copied here - evaluates them on float64 torch tensors and writes tests/golden/learned_var.npz: data only.

    GMS_REFERENCE=<reference checkout> python tools/make_learned_var_golden.py

Rows are time pairs (lt, ls) = (schedule(u), schedule(max(u - 1 / T, 0))) of the cosine schedule on [-20, 20] for T in {10, 100, 1000}: per T the
pair at each end (u = 1 / T, the first step, and u = 1, the last), a few fixed times, and uniform draws (numpy PCG64, seed 0) in [1 / T, 1]; a
zero-length pair has no KL in the reference (log 0) and is left out.  Per row also a latent z_t, a data value x and a prediction x_hat != x.
Keys, all float64: `T`, `u`, `lt`, `ls`, `z_t`, `x`, `x_hat` [N]; `mean_q`, `mean_p` [N] = the reference's `mean` of diffusion_reverse at x and
at x_hat (the same under 'small' and 'large', both are stored: `mean_q_large`, `mean_p_large`); `var_small`, `var_large` [N] = its `var`;
`fracs` [F] in [-0.2, 1.2]; `kl` [N, F] = normal_kl(mean_q, log(var_small), mean_p, f log(var_large) + (1 - f) log(var_small)).

log(var) is used for every log-variance: the reference's own `logvar` field is NaN on these inputs - diffusion_reverse calls log1mexp with
logsnr_s - logsnr_t, a positive argument, where log1mexp takes the logarithm of 1 - e^x - and its 'medium:' branch, which interpolates the two
`logvar`s, inherits that.  `var` of 'small' and 'large' is formed without it and is finite.
"""
import os
import sys

import numpy as np
import torch

STEPS = (10, 100, 1000)
FRACS = (-0.2, 0.0, 0.3, 0.5, 1.0, 1.2)
PER_T = 21
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "learned_var.npz")


def golden_rows():
    gen = np.random.Generator(np.random.PCG64(0))
    T_all, u_all = [], []
    for T in STEPS:
        fixed = [1.0 / T, 1.0, max(2.0 / T, 0.05), 0.25, 0.5, 0.75, 0.97]
        draws = 1.0 / T + (1.0 - 1.0 / T) * gen.random(PER_T - len(fixed))
        u_all.append(np.concatenate([np.array(fixed), draws]))
        T_all.append(np.full(PER_T, float(T)))
    u, T = np.concatenate(u_all), np.concatenate(T_all)
    z_t = gen.standard_normal(len(u))
    x = gen.uniform(-1.0, 1.0, len(u))
    off = gen.uniform(0.05, 0.6, len(u)) * np.where(gen.random(len(u)) < 0.5, -1.0, 1.0)
    x_hat = np.clip(x + off, -1.0, 1.0)
    x_hat = np.where(x_hat == x, x - off, x_hat)
    return T, u, z_t, x, x_hat


def main():
    ref = os.environ.get("GMS_REFERENCE")
    if not ref:
        sys.exit("set GMS_REFERENCE to a checkout of the reference (the directory that holds gms/)")
    sys.path.insert(0, ref)
    from gms.diffusion.diffusion_utils import diffusion_reverse, get_logsnr_schedule, normal_kl

    T, u, z_t, x, x_hat = golden_rows()
    sched = get_logsnr_schedule("cosine", logsnr_min=-20.0, logsnr_max=20.0)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    lt = sched(t64(u))
    ls = sched(t64(np.maximum(u - 1.0 / T, 0.0)))
    assert lt.dtype == torch.float64 and bool((ls > lt).all())
    rev = lambda xx, kind: diffusion_reverse(x=t64(xx), z_t=t64(z_t), logsnr_s=ls, logsnr_t=lt, x_logvar=kind)
    q_small, q_large, p_small, p_large = rev(x, "small"), rev(x, "large"), rev(x_hat, "small"), rev(x_hat, "large")
    var_small, var_large = q_small["var"], q_large["var"]
    assert bool((var_small > 0).all()) and bool((var_large >= var_small).all())
    kl = torch.stack([normal_kl(q_small["mean"], torch.log(var_small), p_small["mean"],
                                f * torch.log(var_large) + (1.0 - f) * torch.log(var_small)) for f in FRACS], dim=1)
    assert bool(torch.isfinite(kl).all())
    out = {"T": T, "u": u, "lt": lt.numpy(), "ls": ls.numpy(), "z_t": z_t, "x": x, "x_hat": x_hat,
           "mean_q": q_small["mean"].numpy(), "mean_q_large": q_large["mean"].numpy(), "mean_p": p_small["mean"].numpy(),
           "mean_p_large": p_large["mean"].numpy(), "var_small": var_small.numpy(), "var_large": var_large.numpy(),
           "fracs": np.array(FRACS), "kl": kl.numpy()}
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
