"""Fused Adam over the flat parameter arena (one kernel launch per step) — replaces the per-tensor
torch.optim.Adam(self.net.parameters(), lr=G.lr) of reference gms/diffusion/diffusion_model.py:56,71.
Same update rule and defaults (betas 0.9/0.999, eps 1e-8, no weight decay, bias-corrected); `grad_scale` folds in
the 1/world factor of data-parallel training.  Parameters without a gradient keep a zero gradient slice, which
leaves them unchanged exactly as torch's skip of `grad is None` does.

With `ema_net` and `ema_decay > 0` (an extension: the reference keeps no weight average) the same launch also updates an exponential
moving average of the weights in `ema_net.flat_params` (same arena layout): ema.lerp_(p_new, 1 - decay_t) with the warm-up of
`ema_decay_at`.  The EMA starts as a copy of the weights at the first step, or at `seed_ema()`.

Three more extensions, all off by default (step() then makes exactly the calls above):
  * `grad_clip = c > 0`: the gradient is scaled by min(1, c / (norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s rule, with `norm` the global L2
    norm of the gradient Adam consumes (after `grad_scale`);
  * `skip_nonfinite`: a step whose gradient norm is inf or NaN changes nothing - p, m, v and the EMA keep their bits - which is what the
    reference's GradScaler.step does.  `grad_clip > 0` implies this guard: a non-finite norm has no clipping coefficient worth applying;
  * a learning-rate schedule on the host, `lr_at`.
The norm and the decision are formed on the device (ops.grad_norm) and read by the Adam launch (ops.adam_step_ctl): no host sync.  A skipped
step therefore STILL advances `step_count`, and with it the bias correction, the schedule and the EMA warm-up; GradScaler does not advance the
optimiser on a skipped step.  The count of skipped steps lives on the device (`ctl_state[ops.SKIPPED]`).

With `ema_sigma_rel` (one to three relative widths, an extension, off by default) the same launch also keeps one power-function average of
the updated weights per width (posthoc_ema.py; Karras et al. 2024): the rows of `pema`, an fp32 [K][n] arena this optimiser owns - no network
is built for them.  Row k after step t is lerp(row k, p_new, w_k(t)), w_k(t) = posthoc_ema.power_weight(gamma_k, t) from the host in double,
the way the EMA's decay travels; w_k(1) = 1, so the rows are zero until step 1 overwrites them with the first updated weights and need no
seeding.  One launch per step in every combination (steered or not, `ema_decay` on or off): ops.adam_pema_step, 28 + 8 (averages) B per
parameter.  A step the non-finite guard skips on the device still advances t (as it does for the bias correction and the EMA warm-up): the
rows keep their bits and the profile a reconstruction assumes is then off by the skipped steps."""
import math

import torch

from .. import ops, posthoc_ema


def ema_decay_at(decay, t):
    """Decay of the EMA update after `t` earlier optimiser steps: min(decay, (1 + t) / (10 + t)), in double.  The warm-up keeps the first
    updates from being dominated by the initial weights (decay 0.1 at t = 0, 0.5 at t = 8, 0.99 at t = 890)."""
    return min(float(decay), (1.0 + t) / (10.0 + t))


class FusedAdam:
    def __init__(self, net, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, ema_net=None, ema_decay=0.0, grad_clip=0.0, skip_nonfinite=False,
                 lr_scheduler="none", lr_warmup=0, lr_decay_steps=0, lr_min_ratio=0.1, ema_sigma_rel=()):
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
        self.grad_clip, self.skip_nonfinite = float(grad_clip), bool(skip_nonfinite)
        if not self.grad_clip >= 0.0:
            raise ValueError(f"grad_clip must be >= 0 (0: off), got {grad_clip}")
        self.lr_scheduler, self.lr_warmup, self.lr_decay_steps = lr_scheduler, int(lr_warmup), int(lr_decay_steps)
        self.lr_min_ratio = float(lr_min_ratio)
        if self.lr_scheduler not in ("none", "cosine"):
            raise ValueError(f"lr_scheduler must be 'none' or 'cosine', got {lr_scheduler!r}")
        if self.lr_warmup < 0 or self.lr_decay_steps < 0:
            raise ValueError(f"lr_warmup and lr_decay_steps must be >= 0, got {lr_warmup} and {lr_decay_steps}")
        if not 0.0 <= self.lr_min_ratio <= 1.0:
            raise ValueError(f"lr_min_ratio must be in [0, 1], got {lr_min_ratio}")
        if self.lr_scheduler == "cosine" and self.lr_decay_steps == 0:
            raise ValueError("lr_scheduler 'cosine' needs lr_decay_steps > 0")
        self.steered = self.grad_clip > 0 or self.skip_nonfinite          # step() goes through ops.grad_norm / ops.adam_step_ctl
        self.scheduled = self.lr_scheduler != "none" or self.lr_warmup > 0
        self.ctl_state = self._ctl_ws = None                              # device: [grad_norm, clip coefficient, apply, skipped steps]
        self._skipped0 = 0.0                                              # the count a loaded state dict carries, until ctl_state exists
        self.last_lr = self.lr
        self.sigma_rel = posthoc_ema.parse_sigma_rel(ema_sigma_rel)       # () : off, step() makes the calls it always made
        self.gamma = tuple(posthoc_ema.gamma_from_sigma_rel(s) for s in self.sigma_rel)
        self.pema = self._pema_store = None                               # device fp32 [K][n] (a view of rows padded to 16 bytes), from the first step on

    def lr_at(self, t):
        """Learning rate of the step taken after `t` earlier ones, in double.  Warm-up: times min(1, (t + 1) / lr_warmup).  'cosine': from lr
        down to lr_min_ratio * lr over the lr_decay_steps steps that follow the warm-up, constant from there on."""
        if not self.scheduled:
            return self.lr
        f = 1.0
        if self.lr_warmup > 0:
            f = min(1.0, (t + 1.0) / self.lr_warmup)
        if self.lr_scheduler == "cosine":
            x = min(max(t - self.lr_warmup, 0), self.lr_decay_steps) / self.lr_decay_steps
            f *= self.lr_min_ratio + (1.0 - self.lr_min_ratio) * 0.5 * (1.0 + math.cos(math.pi * x))
        return self.lr * f

    def zero_grad(self):
        self.net.flat_grads.zero_()

    def seed_ema(self):
        """Start the average from the current weights (first step, a checkpoint without EMA weights, a data-parallel broadcast)."""
        self.ema_net.flat_params.copy_(self.net.flat_params)
        self.ema_net.mark_params_changed()
        self.ema_seeded = True

    def _ensure_pema(self):
        """The power-function arena on the parameters' device: zeros (step 1 overwrites them), or what it held on another device."""
        p = self.net.flat_params
        if self.pema is None or self.pema.device != p.device:
            n = p.numel()
            store = torch.zeros((len(self.gamma), (n + 3) // 4 * 4), dtype=torch.float32, device=p.device)
            if self.pema is not None:
                store[:, :n].copy_(self.pema)
            self._pema_store, self.pema = store, store[:, :n]
        return self.pema

    def power_weights(self, t):
        """The K lerp weights of the update after optimiser step t (doubles; the launch rounds each once to fp32)."""
        return [posthoc_ema.power_weight(gamma, t) for gamma in self.gamma]

    def step(self, grad_scale=1.0):
        p, g = self.net.flat_params, self.net.flat_grads
        if self.m is None or self.m.device != p.device:
            self.m = torch.zeros_like(p)
            self.v = torch.zeros_like(p)
        lr = self.last_lr = self.lr_at(self.step_count) if self.scheduled else self.lr
        if self.steered:
            if self.ctl_state is None or self.ctl_state.device != p.device:
                self.ctl_state = torch.tensor([0.0, 1.0, 1.0, self._skipped0], dtype=torch.float32, device=p.device)
                self._ctl_ws = ops.grad_norm_workspace(p.numel(), p.device)
            ops.grad_norm(g, self.ctl_state, grad_scale, self.grad_clip, self._ctl_ws)
        ema, decay_t = None, 0.0
        if self.ema_net is not None:
            if not self.ema_seeded:
                self.seed_ema()
            ema, decay_t = self.ema_net.flat_params, ema_decay_at(self.ema_decay, self.step_count)
        self.step_count += 1                        # also when the device skips a steered step: the host never learns of it
        adam = (lr, self.betas[0], self.betas[1], self.eps, self.step_count)
        if self.gamma:
            ops.adam_pema_step(p, g, self.m, self.v, self._ensure_pema(), self.power_weights(self.step_count), *adam, grad_scale, ema=ema,
                               decay_t=decay_t, state=self.ctl_state if self.steered else None)
        elif self.steered:
            ops.adam_step_ctl(p, g, self.m, self.v, self.ctl_state, *adam, grad_scale, ema=ema, decay_t=decay_t)
        elif ema is not None:
            ops.adam_ema_step(p, g, self.m, self.v, ema, *adam, decay_t, grad_scale)
        else:
            ops.adam_step(p, g, self.m, self.v, *adam, grad_scale)
        self.net.mark_params_changed()
        if ema is not None:
            self.ema_net.mark_params_changed()

    def skipped_steps(self):
        """Steps the non-finite guard has dropped so far (reads the device: a host sync)."""
        return int(self._skipped0 if self.ctl_state is None else self.ctl_state[ops.SKIPPED].item())

    def state_dict(self):
        """`m` and `v` are None before the first step (a checkpoint taken at epoch 0)."""
        sd = {"step": self.step_count, "m": self.m, "v": self.v, "lr": self.lr, "skipped": self.skipped_steps(),
              "ema_seeded": self.ema_seeded}
        if self.gamma:                  # with ema_sigma_rel only: without it the dictionary has the keys it always had
            sd["pema"] = None if self.pema is None else self.pema.contiguous()
            sd["pema_sigma_rel"] = list(self.sigma_rel)
        return sd

    def load_state_dict(self, sd):
        """The moments move to the arena's device; one of another size (another hidden_size, in_channels or attention flag) is refused."""
        p = self.net.flat_params
        moments = {}
        for name in ("m", "v"):
            t = sd[name]
            if t is not None:
                if t.dtype != p.dtype or t.numel() != p.numel():
                    raise ValueError(f"optimizer state '{name}' holds {t.numel()} {t.dtype} elements, the parameter arena {p.numel()} "
                                     f"{p.dtype}: the state was saved by a model of another shape")
                t = t.detach().reshape(p.shape).to(p.device)
            moments[name] = t
        if (moments["m"] is None) != (moments["v"] is None):
            raise ValueError("optimizer state holds one of 'm' and 'v' only: both, or neither (a state saved before the first step)")
        pema = None
        if self.gamma:
            if "pema" not in sd or [float(s) for s in sd.get("pema_sigma_rel", ())] != list(self.sigma_rel):
                raise ValueError(f"optimizer state tracks the power-function averages {sd.get('pema_sigma_rel', [])}, this run ema_sigma_rel = "
                                 f"{list(self.sigma_rel)}: resume with the widths the state was saved with")
            pema = sd["pema"]
            if pema is not None and (pema.dtype != p.dtype or tuple(pema.shape) != (len(self.gamma), p.numel())):
                raise ValueError(f"optimizer state 'pema' holds {pema.dtype} {tuple(pema.shape)}, this run needs {p.dtype} "
                                 f"{(len(self.gamma), p.numel())}: the state was saved by a model of another shape")
            if (pema is None) != (moments["m"] is None):
                raise ValueError("optimizer state holds one of 'pema' and the moments only: both, or neither (a state saved before the first step)")
        self.step_count, self.m, self.v, self.lr = int(sd["step"]), moments["m"], moments["v"], sd["lr"]
        if self.gamma:
            self.pema = self._pema_store = None
            if pema is not None:
                self._ensure_pema().copy_(pema.detach())
        self.ema_seeded = bool(sd.get("ema_seeded", self.ema_seeded))
        self._skipped0 = float(sd.get("skipped", 0))
        if self.ctl_state is not None:
            self.ctl_state[ops.SKIPPED] = self._skipped0
