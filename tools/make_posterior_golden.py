"""Golden vectors of the ancestral posterior q(z_s | z_t, x) (test infrastructure; needs a checkout of the reference).

Imports the reference's `diffusion_reverse` (gms/diffusion/diffusion_utils.py:34-62) and `get_logsnr_schedule` (:228-239) at generation time
only - nothing of the reference is copied here - walks the cosine sampler grids the way `GaussianDiffusion.sample` there forms them
(gaussian_diffusion.py:287-290: fp32 tensors (i + 1) / T and i / T through the schedule), evaluates the posterior in FLOAT64 on those fp32
log-SNRs for every x_logvar, and writes tests/golden/posterior_var.npz: data only.

    GMS_REFERENCE=<reference checkout> python tools/make_posterior_golden.py

Keys: `steps` int64 (the T's); `x_logvars` (the cases); per T `T<T>_logsnr` fp32 [T, 2] = (logsnr_t, logsnr_s) of the iterations
i = T-1 ... 0; per T and case `T<T>_<case>` float64 [T, 3] = (mean at z = 1, x = 0; mean at z = 0, x = 1; std), the case's ':' and '.'
spelled '_' and 'p' (medium_0p25).  The mean does not depend on x_logvar; it is stored per case all the same, as the reference returns it.
The std of the 'medium' cases is NaN, as the reference returns it (see `main`); the test forms their yardstick from the 'small' and 'large' rows.
"""
import os
import sys

import numpy as np
import torch

STEPS = (1, 2, 3, 4, 8, 20, 250)
X_LOGVARS = ("small", "large", "medium:0.25", "medium:0.5", "medium:0.75")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "posterior_var.npz")


def case_key(T, x_logvar):
    return f"T{T}_" + x_logvar.replace(":", "_").replace(".", "p")


def main():
    ref = os.environ.get("GMS_REFERENCE")
    if not ref:
        sys.exit("set GMS_REFERENCE to a checkout of the reference (the directory that holds gms/)")
    sys.path.insert(0, ref)
    from gms.diffusion.diffusion_utils import diffusion_reverse, get_logsnr_schedule

    schedule = get_logsnr_schedule("cosine", logsnr_min=-20.0, logsnr_max=20.0)
    out = {"steps": np.array(STEPS, dtype=np.int64), "x_logvars": np.array(X_LOGVARS)}
    one, zero = torch.ones((), dtype=torch.float64), torch.zeros((), dtype=torch.float64)
    for T in STEPS:
        pairs = []
        for i in range(T)[::-1]:
            torch_i = torch.tensor(i)
            lt, ls = schedule((torch_i + 1.0) / T), schedule(torch_i / T)
            assert lt.dtype == ls.dtype == torch.float32
            pairs.append((lt.item(), ls.item()))
        pairs = np.array(pairs, dtype=np.float32)
        out[f"T{T}_logsnr"] = pairs
        for x_logvar in X_LOGVARS:
            rows = []
            for lt, ls in pairs:
                kw = dict(logsnr_t=torch.tensor(float(lt), dtype=torch.float64), logsnr_s=torch.tensor(float(ls), dtype=torch.float64),
                          x_logvar=x_logvar)
                at_z, at_x = diffusion_reverse(x=zero, z_t=one, **kw), diffusion_reverse(x=one, z_t=zero, **kw)
                assert at_z["mean"].dtype == at_z["std"].dtype == torch.float64
                rows.append((at_z["mean"].item(), at_x["mean"].item(), at_z["std"].item()))
            rows = np.array(rows, dtype=np.float64)
            # 'medium:<frac>' there is exp(logvar), and its logvar goes through log1mexp(logsnr_s - logsnr_t) - a positive argument, for which
            # that function returns NaN (:40, :108-123): the reference's 'medium' std is NaN at every step and is recorded as it comes.
            # 'small' and 'large' take var = one_minus_r sigmoid(.) directly and are finite.
            assert np.isfinite(rows[:, :2]).all() and (x_logvar.startswith("medium:") or np.isfinite(rows[:, 2]).all()), (T, x_logvar)
            out[case_key(T, x_logvar)] = rows
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
