"""Golden vectors of the closed-form log-SNR schedules (test infrastructure; needs a checkout of the reference).

Imports the reference's `get_logsnr_schedule` (gms/diffusion/diffusion_utils.py:228-239) at generation time only - nothing of the
reference is copied here - evaluates the four closed-form kinds on fp32 torch tensors, as `GaussianDiffusion` there does, and writes
tests/golden/logsnr_schedules.npz: data only.

    GMS_REFERENCE=<reference checkout> python tools/make_schedule_golden.py

Keys: `u` fp32 [N]; `kinds` / `ranges` (the cases); `<kind>_<lmin>_<lmax>` fp32 [N] = schedule(u) with negative numbers spelled m20.
u holds 0, 1, 1/64, 63/64, 0.999, 1e-4, 0.03, 0.4, then 300 uniform draws (numpy PCG64, seed 0), then the samplers' grids i / T in fp32 for
T = 4 (i = 0 ... 4) and T = 250 (i = 0 ... 250): `grid_T4` / `grid_T250` are their [start, stop) index ranges in `u`.
"""
import os
import sys

import numpy as np
import torch

KINDS = ("cosine", "uniform", "beta_const", "beta_linear")
RANGES = ((-20.0, 20.0), (-15.0, 15.0), (-10.0, 20.0))
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "logsnr_schedules.npz")


def case_key(kind, lmin, lmax):
    num = lambda v: f"{v:g}".replace("-", "m")
    return f"{kind}_{num(lmin)}_{num(lmax)}"


def golden_u():
    fixed = np.array([0.0, 1.0, 1.0 / 64, 63.0 / 64, 0.999, 1e-4, 0.03, 0.4], dtype=np.float32)
    draws = np.random.Generator(np.random.PCG64(0)).random(300, dtype=np.float32)
    grids, spans, at = [], {}, len(fixed) + len(draws)
    for T in (4, 250):
        g = np.arange(T + 1, dtype=np.float32) / np.float32(T)
        spans[f"grid_T{T}"] = np.array([at, at + len(g)])
        grids.append(g)
        at += len(g)
    return np.concatenate([fixed, draws] + grids), spans


def main():
    ref = os.environ.get("GMS_REFERENCE")
    if not ref:
        sys.exit("set GMS_REFERENCE to a checkout of the reference (the directory that holds gms/)")
    sys.path.insert(0, ref)
    from gms.diffusion.diffusion_utils import get_logsnr_schedule

    u, spans = golden_u()
    out = {"u": u, "kinds": np.array(KINDS), "ranges": np.array(RANGES, dtype=np.float64), **spans}
    t = torch.from_numpy(u)
    for kind in KINDS:
        for lmin, lmax in RANGES:
            l = get_logsnr_schedule(kind, logsnr_min=lmin, logsnr_max=lmax)(t)
            assert l.dtype == torch.float32 and bool(torch.isfinite(l).all()), (kind, lmin, lmax)
            out[case_key(kind, lmin, lmax)] = l.numpy()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
