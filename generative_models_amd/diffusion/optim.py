"""Fused Adam over the flat parameter arena (one kernel launch per step) — replaces the per-tensor
torch.optim.Adam(self.net.parameters(), lr=G.lr) of reference gms/diffusion/diffusion_model.py:56,71.
Same update rule and defaults (betas 0.9/0.999, eps 1e-8, no weight decay, bias-corrected); `grad_scale` folds in
the 1/world factor of data-parallel training.  Parameters without a gradient keep a zero gradient slice, which
leaves them unchanged exactly as torch's skip of `grad is None` does.

With `ema_net` and `ema_decay > 0` (an extension: the reference keeps no weight average) the same launch also updates an exponential
moving average of the weights in `ema_net.flat_params` (same arena layout): ema.lerp_(p_new, 1 - decay_t) with the warm-up of
`ema_decay_at`.  The EMA starts as a copy of the weights at the first step, or at `seed_ema()`."""
import torch

from .. import ops


def ema_decay_at(decay, t):
    """Decay of the EMA update after `t` earlier optimiser steps: min(decay, (1 + t) / (10 + t)), in double.  The warm-up keeps the first
    updates from being dominated by the initial weights (decay 0.1 at t = 0, 0.5 at t = 8, 0.99 at t = 890)."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


class FusedAdam:
    def __init__(self, net, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, ema_net=None, ema_decay=0.0):
        self.net, self.lr, self.betas, self.eps = net, float(lr), betas, float(eps)
        self.step_count = 0
        self.m = self.v = None
        self.ema_decay = float(ema_decay)
        if self.ema_decay > 0 and ema_net is None:
            raise ValueError("ema_decay > 0 needs an ema_net to hold the average")
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError(f"ema_decay must be in [0, 1), got {ema_decay}")
        self.ema_net = ema_net if self.ema_decay > 0 else None
        self.ema_seeded = False

    def zero_grad(self):
        self.net.flat_grads.zero_()

    def seed_ema(self):
        """Start the average from the current weights (first step, a checkpoint without EMA weights, a data-parallel broadcast)."""
        self.ema_net.flat_params.copy_(self.net.flat_params)
        self.ema_net.mark_params_changed()
        self.ema_seeded = True

    def step(self, grad_scale=1.0):
        p = self.net.flat_params
        if self.m is None or self.m.device != p.device:
            self.m = torch.zeros_like(p)
            self.v = torch.zeros_like(p)
        if self.ema_net is None:
            self.step_count += 1
            ops.adam_step(p, self.net.flat_grads, self.m, self.v, self.lr, self.betas[0], self.betas[1], self.eps,
                          self.step_count, grad_scale)
            self.net.mark_params_changed()
            return
        if not self.ema_seeded:
            self.seed_ema()
        decay_t = ema_decay_at(self.ema_decay, self.step_count)
        self.step_count += 1
        ops.adam_ema_step(p, self.net.flat_grads, self.m, self.v, self.ema_net.flat_params, self.lr, self.betas[0], self.betas[1],
                          self.eps, self.step_count, decay_t, grad_scale)
        self.net.mark_params_changed()
        self.ema_net.mark_params_changed()

    def state_dict(self):
        return {"step": self.step_count, "m": self.m, "v": self.v, "lr": self.lr}

    def load_state_dict(self, sd):
        self.step_count, self.m, self.v, self.lr = sd["step"], sd["m"], sd["v"], sd["lr"]
