"""CPU restatement of the steered optimiser step (DG.grad_clip / DG.skip_nonfinite / the learning-rate schedule): the global gradient norm
in float64, torch.nn.utils.clip_grad_norm_'s coefficient, the schedule FusedAdam.lr_at follows, and the a-priori error bound of the norm
kernel's summation.  Nothing here imports the package under test."""
import math

import numpy as np
import torch

# ---- the norm kernel's summation tree (csrc/diffusion_ew.hip: kNormLoads, kNormQuads, grad_norm_partial_kernel / grad_norm_final_kernel)
NORM_LOADS = 8                       # 16-byte loads per thread: additions into each of a thread's four component accumulators
NORM_QUADS = 256 * NORM_LOADS        # float4s per workgroup
JOIN, TAIL, WAVE, BLOCK = 2, 1, 6, 2     # (a0 + a1) + (a2 + a3); the n & 3 tail element; the 64-lane butterfly; (r0 + r1) + (r2 + r3)


def norm_parts(n):
    nq = n // 4
    return 1 if nq <= NORM_QUADS else -(-nq // NORM_QUADS)


def norm_chain(n):
    """d: the longest chain of fp32 additions behind the kernel's sum of squares of n elements.  Stage 1 (one partial per workgroup):
    NORM_LOADS + JOIN + TAIL + WAVE + BLOCK; stage 2 (one workgroup): ceil(parts / 256) per thread, then WAVE + BLOCK."""
    return (NORM_LOADS + JOIN + TAIL + WAVE + BLOCK) + (-(-norm_parts(n) // 256) + WAVE + BLOCK)


def norm_rel_bound(n):
    """Relative error of the NORM: the sum of squares carries at most (d + 1) roundings of 2^-24 each (d additions and the square), the square
    root halves it."""
    return 0.5 * (norm_chain(n) + 1) * 2.0 ** -24


def norm64(g, grad_scale=1.0):
    """grad_scale * ||g||_2 with the squares and their sum in float64."""
    g = g.detach().double().reshape(-1)
    return float(grad_scale) * math.sqrt(float((g * g).sum()))


def clip_coef(total_norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient in fp32 arithmetic: min(1, max_norm / (total_norm + 1e-6)); max_norm <= 0: 1."""
    if max_norm <= 0:
        return np.float32(1.0)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.minimum(np.float32(1.0), np.float32(max_norm) / (np.float32(total_norm) + np.float32(1e-6)))


def lr_at(lr, t, scheduler="none", warmup=0, decay_steps=0, min_ratio=0.1):
    """Learning rate after t earlier steps: warm-up factor min(1, (t + 1) / warmup); 'cosine': lr -> min_ratio lr over decay_steps steps
    after the warm-up, constant afterwards."""
    f = 1.0
    if warmup > 0:
        f = min(1.0, (t + 1.0) / warmup)
    if scheduler == "cosine":
        x = min(max(t - warmup, 0), decay_steps) / decay_steps
        f *= min_ratio + (1.0 - min_ratio) * 0.5 * (1.0 + math.cos(math.pi * x))
    return lr * f


def clip_grad_norm_double(grads, max_norm):
    """torch.nn.utils.clip_grad_norm_'s return value on CPU double copies of the gradients."""
    params = []
    for g in grads:
        p = torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64))
        p.grad = g.detach().double().cpu().clone()
        params.append(p)
    return float(torch.nn.utils.clip_grad_norm_(params, max_norm))
