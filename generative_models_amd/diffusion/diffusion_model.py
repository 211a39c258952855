"""`DiffusionModel` plugin — drop-in for reference gms/diffusion/diffusion_model.py:14-111 on the HIP path.

Same class name (registry key `diffusion_model`, alias `diffusion`), same `DG` keys and defaults (:15-29), same
method surface the driver calls: train_step(x, y) -> {'loss', 'loss_scale'}, loss(x, y) -> (loss, metrics),
sample(n, y) -> [n, C, S, S] in [-1, 1], evaluate(writer, x, y, epoch), save (inherited).  State-dict keys are
`net.<reference names>`.

How it differs underneath: 16-bit MFMA compute with fp32 master weights - forward activations and forward weight packs in fp16 (the
precision of the reference's fp16 autocast forward), gradients in bf16 - instead of fp16 autocast + GradScaler (bf16 gradients need no
loss scaling; `loss_scale` is reported as 1.0 to keep the metric key); one fused pass
(forward -> loss -> explicit backward -> bucketed RCCL all-reduce -> fused Adam) instead of autograd + per-tensor
optimiser; RNG from counter-based Philox streams on the device.  `make_plugin(base)` builds the same class on top of
the REFERENCE's `gms.common.GM`, which is what a `gms/` checkout needs for `discover_models()` to pick it up
(INTEGRATION.md).
"""
import math
import random
from functools import partial
from pathlib import Path

import os

import torch

from .. import checkpoint, common, ops, parallel, posthoc_ema
from .gaussian_diffusion import (GaussianDiffusion, PhiloxStream, Schedule, consistency_check, dyn_threshold_check, edit_start, guidance_check,
                                 loss_weight_check, restore_operator, schedule_check, stochastic_check, time_importance_check, learned_var_check,
                                 FLAG_WORDS, sampler_caps, sampler_compat_check, dps_check, dps_zeta_check, measurement_op)
from .optim import FusedAdam
from .simple_unet import SimpleUnet

_DTYPES = {"bf16": torch.bfloat16, "fp32": torch.float32}


def make_plugin(GMBase, AttrDict):
    class DiffusionModel(GMBase):
        DG = AttrDict()  # default G  (diffusion_model.py:15-29)
        DG.binarize = 0
        DG.timesteps = 250             # sampler steps (network evaluations per sample); also the distillation discretisation (teacher_path)
        DG.hidden_size = 128
        DG.dropout = 0.0
        DG.sampler = "ddim"            # 'ddim' | 'noisy' | 'teacher_test' (reference) | 'dpmpp_2m' (extension: DPM-Solver++(2M), second order, no training)
                                       # | 'consistency' (extension: multistep consistency sampling, for a net trained with teacher_mode 'consistency')
                                       # | 'ancestral' ('noisy' with the variance of posterior_var, its noise drawn in the update kernel)
                                       # | 'sde_dpmpp_2m' (extension: SDE-DPM-Solver++(2M), Lu et al. 2022: second order, stochastic)
        DG.posterior_var = "large"     # sampler 'ancestral': the reference's x_logvar (diffusion_utils.py:44-61), 'small' | 'large' (what 'noisy' hard-codes)
                                       # | 'medium:<frac>', frac in [0, 1] the log-domain weight of 'large' | 'learned' (the network's own, per element
                                       # and per step: needs learn_var = 1)
        DG.ddim_eta = 0.0              # sampler 'ddim': eta in (0, 1], the noise share of Song et al. 2021 (1: ancestral 'small'); 0: deterministic DDIM, as ever
        DG.mean_type = "v"
        DG.eval_heavy = 1
        DG.class_cond = 1
        DG.sample_cond_w = -1.0
        DG.cf_drop_prob = 0.1
        DG.teacher_path = Path(".")
        DG.teacher_mode = "step1"        # 'step1' | 'step2' (reference: progressive distillation) | 'consistency' (extension: consistency distillation,
                                       # Song et al. 2023, Algorithm 2: one training run for 1-4 step sampling; needs teacher_path)
        DG.lr_scheduler = "none"         # 'none' (reference: nothing reads it there) | 'cosine' (extension: FusedAdam.lr_at)
        # additions of the HIP path
        DG.compute_dtype = "bf16"      # 'bf16' (16-bit MFMA mode: bf16 gradients) or 'fp32' (exact-fp32 MFMA, 1e-3 parity mode)
        DG.act_dtype = os.environ.get("GMK_ACT_DTYPE", "fp16")      # 16-bit mode only: storage of forward activations / forward weight packs, 'fp16' (the precision of the
                                       # reference's fp16 autocast forward, diffusion_model.py:68) or 'bf16' (the all-bf16 path, A/B)
        DG.in_channels = 1             # reference: 1 (simple_unet.py:93,41)
        DG.attention = 0               # 1: self-attention block behind `turn` (north_star / BASELINE config 5; not in the reference); 2: the same
                                       # with QK^T / PV on the fp8 matrix cores
        DG.seed = 0
        DG.ema_decay = 0.0             # > 0: keep an exponential moving average of the weights (`ema_net`, updated inside the fused Adam launch)
                                       # and sample / evaluate with it; not in the reference, off by default
        DG.nlogp_samples = 0           # > 0: loss() also reports the variational bound (`nlogp`, logged as eval/nlogp, and `bpd`) of the sampling
                                       # net with that many log-SNR draws per image; not in the reference, off by default
        DG.ode_nlogp_steps = 0         # N > 0: loss() also reports the probability-flow ODE likelihood (`ode_nlogp`, logged as
                                       # <model>/test/ode_nlogp) of the sampling net on N steps; not in the reference, off by default
        DG.inpaint_eval = 0            # r >= 1: evaluate() also fills in the bottom half of the first 25 test images (RePaint, resample = r) as
                                       # last_eval['inpaint'] / grid 'inpaint'; not in the reference, off by default
        DG.edit_eval = 0.0             # strength in (0, 1]: evaluate() also edits the first 25 test images (SDEdit: noised up to that share of the chain and
                                       # denoised from there) as last_eval['edit'] / frames 'edit'; not in the reference, off by default
        DG.interp_eval = 0             # K >= 2: evaluate() also interpolates test images 0-4 into 5-9 through their latent codes in K frames (DDIM
                                       # inversion, slerp, decode) as last_eval['interp'] / frames 'interp'; not in the reference, off by default
        DG.restore_eval = 0            # N >= 2: evaluate() also restores the first 25 test images from their N x N box means (DDNM super-resolution,
                                       # Wang, Yu & Zhang 2023) as last_eval['restore'] / frames 'restore', 'restore_input', with last_eval['restore_psnr'];
                                       # not in the reference, off by default
        DG.restore_gray = 0            # 1: that restoration also (or, with restore_eval = 0, only) starts from the channel mean (colourisation)
        DG.dps_eval = ""               # 'box:N' | 'gray' | 'gray_box:N' | 'blur:SIGMA': evaluate() also restores the first 25 test images from that measurement
                                       # plus noise by diffusion posterior sampling (DPS, Chung et al. 2023) as last_eval['dps'] / frames 'dps', 'dps_input',
                                       # with last_eval['dps_psnr'], ['dps_input_psnr'] and ['dps_residual']; samplers 'ddim', 'noisy', 'ancestral'; '': off
        DG.dps_noise = 0.05            # the standard deviation of that measurement's noise, >= 0 (dps_residual is comparable with it)
        DG.dps_zeta = 1.0              # the DPS step size zeta >= 0 of evaluate() and posterior_sample(); untuned: the paper's values lie in 0.3 ... 1
        DG.dyn_threshold = 0.0         # p in (0, 1]: sample() / evaluate() / inpaint() clamp each image's x-hat to its own p-th percentile of |x| and rescale
                                       # (dynamic thresholding, Saharia et al. 2022; e.g. 0.995) instead of the clip at 1; not in the reference, off by default
        DG.guidance_lo = float("-inf") # the guidance interval (Kynkaanniemi et al. 2024): a guided sampler step whose log-SNR lies outside [guidance_lo, guidance_hi]
        DG.guidance_hi = float("inf")  # evaluates the conditional batch alone (B images forwarded instead of 2 B); both infinite: off (guidance at every step);
                                       # e.g. -3, 3; not in the reference
        DG.cfg_rescale = 0.0           # phi in (0, 1]: on guided steps x-hat is the guided prediction scaled by 1 + phi (std(x_cond) / std(x_guided) - 1) per image,
                                       # then clipped (Lin et al. 2023, section 3.4; e.g. 0.7); not with dyn_threshold, restore_eval / restore_gray or
                                       # sampler 'consistency'; not in the reference, off by default
        DG.grad_clip = 0.0             # c > 0: clip the global gradient norm to c inside the optimiser step (torch.nn.utils.clip_grad_norm_'s rule) and
                                       # report train/grad_norm, train/skipped_steps; implies skip_nonfinite; not in the reference, off by default
        DG.skip_nonfinite = 0          # 1: a step whose gradients hold an inf or a NaN changes nothing (the guard of the reference's GradScaler.step)
        DG.lr_warmup = 0               # W > 0: lr times min(1, (t + 1) / W) after t steps, under either lr_scheduler
        DG.lr_decay_steps = 0          # 'cosine': steps from lr down to lr_min_ratio * lr, counted from the end of the warm-up
        DG.lr_min_ratio = 0.1
        DG.loss_weight = "snr_trunc"   # the training loss: 'snr_trunc' (reference: max(x_mse, eps_mse)) | 'snr' (eps_mse) | 'snr_plus1' ((1 + SNR) x_mse, the v-space
                                       # MSE of Salimans & Ho 2022) | 'min_snr' (min(SNR, loss_gamma) x_mse, Hang et al. 2023); other than the default
                                       # loss() also reports `x_mse` (logged as <model>/test/x_mse); not with teacher_path; not in the reference
        DG.loss_gamma = 5.0            # Min-SNR's gamma, finite and > 0
        DG.time_sampler = "uniform"    # 'uniform' (reference: independent times) | 'stratified' (one offset per batch, evenly spaced times: Kingma et al.
                                       # 2021, VDM App. I.1; every rank of a data-parallel run stratifies its own batch); not with teacher_path
        DG.time_importance = 0         # 1: draw the training times with p(t) proportional to sqrt(E[L_t^2]) of a running 64-bin loss profile and reweight by
                                       # 1 / p (Nichol & Dhariwal 2021, section 3.3; gmk_u_importance); uniform until every bin holds importance_warmup
                                       # samples; one rank only; not with teacher_path; not in the reference, off by default
        DG.importance_decay = 0.9      # per-bin decay of the profile, in (0, 1]: a window of about 1 / (1 - decay) of the bin's own samples (untuned)
        DG.importance_warmup = 5       # samples every bin must hold before the sampler leaves uniform, <= 0.5 / (1 - importance_decay) (untuned)
        DG.importance_floor = 0.01     # the uniform share of the sampling distribution, in (0, 1] (untuned)
        DG.loss_profile = 0            # 1: keep the per-time profile of the train and test losses (gmk_loss_profile) and write it to
                                       # <logdir>/loss_profile.csv after every evaluation; nothing is sampled from it; not with teacher_path
        DG.logsnr_schedule = "cosine"  # the noise schedule u -> logsnr of training: 'cosine' (reference) | 'uniform' | 'beta_const' | 'beta_linear', the closed-form
                                       # schedules of the reference's registry (diffusion_utils.py:169-201); other than the defaults: not in the reference's plugin
        DG.logsnr_min = -20.0          # its range, -20 <= logsnr_min < logsnr_max <= 20 (the reference's pick: -20, 20); the likelihoods (nlogp_samples,
        DG.logsnr_max = 20.0           # ode_nlogp_steps) are integrated over [-20, 20] and refuse another range or a shift
        DG.logsnr_shift = 0.0          # added to the log-SNR, |shift| <= 10: 2 log(32 / d) for d x d images (Hoogeboom et al. 2023), -1.386 at 64 x 64
        DG.sample_logsnr_schedule = "" # the curve the samplers walk (sample, evaluate, inpaint, edit, restore, encode / decode): '' the training one, else a
                                       # kind as above on the same range and shift ('uniform' is DPM-Solver++'s grid for few steps)
        DG.consistency_grid = 0        # teacher_mode 'consistency': the number N >= 1 of training time points (0: timesteps), so that a run can train on
                                       # a 256-point grid while --timesteps 2 --sampler consistency evaluates in two steps
        DG.consistency_loss = "l2"     # teacher_mode 'consistency': 'l2' (the truncated-SNR loss of step2, against the consistency target) | 'huber'
                                       # (pseudo-Huber on x, Song & Dhariwal 2023; gmk_x_loss_huber)
        DG.consistency_huber_c = 0.00054  # its c, finite and > 0: the paper's 0.00054 sqrt(d) per dimension
        DG.learn_var = 0               # 1: the network gets a second head `out_var` whose output nu sets the reverse-process variance per element, and trains on
                                       # the hybrid loss simple + vlb_lambda vlb (Nichol & Dhariwal 2021, section 3.1; gmk_hybrid_loss); loss() also reports
                                       # `vlb` and `var_frac`; not with teacher_path, loss_weight 'snr_trunc' / 'snr' only; not in the reference, off by default
        DG.vlb_lambda = 0.001          # the weight of the bound term, finite and >= 0 (the paper's value)
        DG.vlb_steps = 1000            # T >= 1: the bound term compares the times u and max(u - 1 / T, 0)
        DG.ema_sigma_rel = ""          # 's1[,s2[,s3]]': keep a power-function average of the weights per relative width (strictly increasing, each in
                                       # [0.01, 0.25]) inside the fused Adam launch and snapshot them under <logdir>/ema_snapshots; the weights of any
                                       # width in between are reconstructed after training (posthoc_ema.py; Karras et al. 2024); evaluate() and sample()
                                       # keep using the online or the ema_decay net; not in the reference, off by default
        DG.ema_snapshot_every = 0      # optimiser steps between those snapshots (needs logdir); 0: one at every save() only
        DG.image_size = 0              # S > 0: images are S x S (CIFAR-10: 32 with in_channels 3); 0: the reference's 28, or 32 with pad32

        def __init__(self, G):
            super().__init__(G)
            get = lambda k: G[k] if k in G else self.DG[k]
            self.ema_sigma_rel, self.ema_snapshot_every = posthoc_ema.check_flags(get("ema_sigma_rel"), get("ema_snapshot_every"))
            if self.ema_snapshot_every > 0 and "logdir" not in G:
                raise ValueError(f"ema_snapshot_every = {self.ema_snapshot_every} without logdir: the snapshots go to <logdir>/ema_snapshots")
            cdt = _DTYPES[get("compute_dtype")]
            adt = cdt if cdt == torch.float32 else {"fp16": torch.float16, "bf16": torch.bfloat16}[get("act_dtype")]
            if get("learn_var") not in (0, 1):
                raise ValueError(f"learn_var = {get('learn_var')!r}: 0 (off) or 1")
            self.net = SimpleUnet(get("hidden_size"), get("dropout"), in_channels=get("in_channels"),
                                  compute_dtype=cdt, attention=int(get("attention")), act_dtype=adt, learn_var=bool(get("learn_var")))
            weights_from = Path(G["weights_from"]) if "weights_from" in G else Path(".")
            if Path(get("teacher_path")) != Path(".") and weights_from == Path("."):      # diffusion_model.py:34-43
                print("Loading teacher model")
                self.load_state_dict(torch.load(get("teacher_path"), map_location="cpu"), strict=False)
                self.teacher_net = SimpleUnet(get("hidden_size"), get("dropout"), in_channels=get("in_channels"),
                                              compute_dtype=cdt, attention=int(get("attention")), act_dtype=adt)
                self.teacher_net.load_state_dict(self.net.state_dict())
                self.teacher_net.eval()
                for param in self.teacher_net.parameters():
                    param.requires_grad = False
            else:
                self.teacher_net = None
            consistency, consistency_grid, consistency_loss, consistency_huber_c = consistency_check(
                get("teacher_mode"), self.teacher_net is not None, get("consistency_grid"), get("consistency_loss"), get("consistency_huber_c"))
            self.nlogp_samples = int(get("nlogp_samples"))
            if self.nlogp_samples < 0:
                raise ValueError(f"nlogp_samples = {self.nlogp_samples}: 0 (off) or the number of draws per image")
            if self.nlogp_samples > 0 and self.teacher_net is not None:
                raise ValueError("nlogp_samples > 0 with teacher_path: a distilled student is conditioned on cond_w; its variational bound "
                                 "is not defined")
            self.ode_nlogp_steps = int(get("ode_nlogp_steps"))
            if self.ode_nlogp_steps < 0:
                raise ValueError(f"ode_nlogp_steps = {self.ode_nlogp_steps}: 0 (off) or the number of ODE steps")
            if self.ode_nlogp_steps > 0 and self.teacher_net is not None:
                raise ValueError("ode_nlogp_steps > 0 with teacher_path: a distilled student is conditioned on cond_w; its probability-flow "
                                 "ODE has no density")
            self.inpaint_eval = int(get("inpaint_eval"))
            if self.inpaint_eval < 0:
                raise ValueError(f"inpaint_eval = {self.inpaint_eval}: 0 (off) or the resample count r >= 1")
            try:
                self.edit_eval = float(get("edit_eval"))
            except (TypeError, ValueError):
                raise ValueError(f"edit_eval = {get('edit_eval')!r}: 0 (off) or the strength in (0, 1]") from None
            if not 0.0 <= self.edit_eval <= 1.0:
                raise ValueError(f"edit_eval = {self.edit_eval}: 0 (off) or the strength in (0, 1]")
            self.interp_eval = int(get("interp_eval"))
            if self.interp_eval < 0 or self.interp_eval == 1 or self.interp_eval != float(get("interp_eval")):
                raise ValueError(f"interp_eval = {get('interp_eval')}: 0 (off) or the number of frames K >= 2")
            if self.interp_eval > 0 and self.teacher_net is not None:
                raise ValueError("interp_eval > 0 with teacher_path: a distilled student is conditioned on cond_w; its probability-flow ODE has "
                                 "no density")
            self.restore_eval = int(get("restore_eval"))
            if self.restore_eval < 0 or self.restore_eval == 1 or self.restore_eval != float(get("restore_eval")):
                raise ValueError(f"restore_eval = {get('restore_eval')}: 0 (off) or the super-resolution factor N >= 2")
            if get("restore_gray") not in (0, 1):
                raise ValueError(f"restore_gray = {get('restore_gray')!r}: 0 (off) or 1")
            self.restore_gray = int(get("restore_gray"))
            if self.restore_gray and int(get("in_channels")) == 1:
                raise ValueError("restore_gray = 1 with in_channels = 1: there is no colour to restore")
            self.binarize = int(get("binarize"))
            self.dps_eval = get("dps_eval")
            if not isinstance(self.dps_eval, str):
                raise ValueError(f"dps_eval = {self.dps_eval!r}: '' (off) or a measurement, 'box:N', 'gray', 'gray_box:N' or 'blur:SIGMA'")
            self.dps_zeta = dps_zeta_check(get("dps_zeta"), "dps_zeta")
            try:
                self.dps_noise = float(get("dps_noise"))
            except (TypeError, ValueError):
                raise ValueError(f"dps_noise = {get('dps_noise')!r}: the noise's standard deviation, finite and >= 0") from None
            if not (0.0 <= self.dps_noise < float("inf")):
                raise ValueError(f"dps_noise = {self.dps_noise}: the noise's standard deviation, finite and >= 0")
            dyn_threshold = dyn_threshold_check(get("dyn_threshold"))
            learn_var, vlb_lambda, vlb_steps = learned_var_check(get("learn_var"), get("vlb_lambda"), get("vlb_steps"), self.teacher_net is not None,
                                                                 get("loss_weight"))
            _, posterior_var, ddim_eta = stochastic_check(get("sampler"), get("posterior_var"), get("ddim_eta"), learn_var)
            guidance_interval, cfg_rescale = guidance_check((get("guidance_lo"), get("guidance_hi")), get("cfg_rescale"), get("sampler"),
                                                            dyn_threshold)
            # what goes with the sampler, by the loop's own table: asked once per evaluation extra (each is a sampler run of its own at evaluate())
            for one in (dict(inpaint=min(self.inpaint_eval, 1)), dict(restore=self.restore_eval or self.restore_gray)):
                sampler_compat_check(sampler_caps(get("sampler"), ddim_eta), dyn_threshold=dyn_threshold, cfg_rescale=cfg_rescale, words=FLAG_WORDS, **one)
            loss_weight, loss_gamma, time_sampler = loss_weight_check(get("loss_weight"), get("loss_gamma"), get("time_sampler"),
                                                                      self.teacher_net is not None)
            time_importance, importance_decay, importance_warmup, importance_floor, loss_profile = time_importance_check(
                get("time_importance"), get("importance_decay"), get("importance_warmup"), get("importance_floor"), get("loss_profile"),
                self.teacher_net is not None, parallel.world())
            self.loss_profile = loss_profile
            schedule, sample_schedule = schedule_check(get("logsnr_schedule"), get("logsnr_min"), get("logsnr_max"), get("logsnr_shift"),
                                                       get("sample_logsnr_schedule"))
            for name in ("nlogp_samples", "ode_nlogp_steps"):
                if getattr(self, name) > 0 and not schedule.full_range:
                    raise ValueError(f"{name} > 0 with logsnr_min = {schedule.logsnr_min:g}, logsnr_max = {schedule.logsnr_max:g}, logsnr_shift = "
                                     f"{schedule.shift:g}: the likelihoods are integrated over logsnr in [-20, 20]; leave the three at -20, 20, 0")
            # the defaults are the reference's pick, which the original entries hold as constants: None keeps a default run on them
            # (a sampling schedule of None would mean the training one, so it is only dropped together with it)
            if schedule == Schedule():
                sample_schedule = None if sample_schedule == schedule else sample_schedule
                schedule = None
            seed = int(get("seed")) * 1000 + parallel.rank()
            # EMA of the weights (an extension): a second SimpleUnet of the same arena layout, so one fused launch updates both.  It is seeded
            # from `net` at the first optimiser step (after a data-parallel broadcast of the initial weights) or by a checkpoint load; under
            # teacher_mode 'consistency' it is also the method's target network and is seeded ahead of the first forward (`_seed_target`).
            self.ema_decay = float(get("ema_decay"))
            self.ema_net = None
            if self.ema_decay > 0:
                self.ema_net = SimpleUnet(get("hidden_size"), get("dropout"), in_channels=get("in_channels"),
                                          compute_dtype=cdt, attention=int(get("attention")), act_dtype=adt, learn_var=learn_var)
                for param in self.ema_net.parameters():
                    param.requires_grad = False
                self.ema_net.eval()
            self.diffusion = GaussianDiffusion(mean_type=get("mean_type"), num_steps=int(get("timesteps")),
                                               sampler=get("sampler"), teacher_net=self.teacher_net,
                                               teacher_mode=get("teacher_mode"), sample_cond_w=get("sample_cond_w"),
                                               seed=seed, dyn_threshold=dyn_threshold, loss_weight=loss_weight, loss_gamma=loss_gamma,
                                               time_sampler=time_sampler, time_importance=time_importance, importance_decay=importance_decay,
                                               importance_warmup=importance_warmup, importance_floor=importance_floor, loss_profile=loss_profile,
                                               schedule=schedule, sample_schedule=sample_schedule,
                                               target_net=self.ema_net if consistency else None, consistency_grid=consistency_grid,
                                               consistency_loss=consistency_loss, consistency_huber_c=consistency_huber_c,
                                               guidance_interval=guidance_interval, cfg_rescale=cfg_rescale,
                                               posterior_var=posterior_var, ddim_eta=ddim_eta, learn_var=int(learn_var), vlb_lambda=vlb_lambda,
                                               vlb_steps=vlb_steps)
            self.net.drop_seed = seed + 104729              # per-rank dropout masks (only used when dropout > 0)
            grad_clip, lr_min_ratio = float(get("grad_clip")), float(get("lr_min_ratio"))
            lr_warmup, lr_decay_steps = int(get("lr_warmup")), int(get("lr_decay_steps"))
            if not grad_clip >= 0.0:
                raise ValueError(f"grad_clip = {grad_clip}: 0 (off) or the largest global gradient norm")
            if int(get("skip_nonfinite")) not in (0, 1):
                raise ValueError(f"skip_nonfinite = {get('skip_nonfinite')}: 0 (off) or 1")
            if get("lr_scheduler") not in ("none", "cosine"):
                raise ValueError(f"lr_scheduler = {get('lr_scheduler')!r}: 'none' or 'cosine'")
            if lr_warmup < 0 or lr_decay_steps < 0:
                raise ValueError(f"lr_warmup = {lr_warmup}, lr_decay_steps = {lr_decay_steps}: 0 (off) or a number of steps")
            if not 0.0 <= lr_min_ratio <= 1.0:
                raise ValueError(f"lr_min_ratio = {lr_min_ratio}: the final fraction of lr, in [0, 1]")
            if get("lr_scheduler") == "cosine" and lr_decay_steps == 0:
                raise ValueError("lr_scheduler = 'cosine' with lr_decay_steps = 0: give the number of steps of the decay")
            self.optimizer = FusedAdam(self.net, lr=G.lr if "lr" in G else 3e-4, ema_net=self.ema_net, ema_decay=self.ema_decay,
                                       grad_clip=grad_clip, skip_nonfinite=bool(int(get("skip_nonfinite"))), lr_scheduler=get("lr_scheduler"),
                                       lr_warmup=lr_warmup, lr_decay_steps=lr_decay_steps, lr_min_ratio=lr_min_ratio,
                                       ema_sigma_rel=self.ema_sigma_rel)
            self.size = 32 if ("pad32" in G and G.pad32) else 28
            if int(get("image_size")) < 0:
                raise ValueError(f"image_size = {get('image_size')}: 0 (28, or 32 with pad32) or the side of the square images")
            self._size_declared = int(get("image_size")) > 0
            if self._size_declared:
                self.size = int(get("image_size"))
            self._aux_rng = PhiloxStream(seed + 7919)
            if self.dps_eval:               # the string against this model's images, the sampler and its options against what DPS runs with
                measurement_op(self.dps_eval, (1, int(get("in_channels")), self.size, self.size))
                fixed_w = get("sample_cond_w") is not None and float(get("sample_cond_w")) != -1.0
                dps_check(sampler=get("sampler"), ddim_eta=ddim_eta, mean_type=get("mean_type"), cond_w=fixed_w, dyn_threshold=dyn_threshold,
                          cfg_rescale=cfg_rescale, learned_var=posterior_var == "learned", student=self.teacher_net is not None, what="dps_eval")
            self._sync = None

        def train(self, mode=True):
            super().train(mode)
            if self.ema_net is not None:            # the average is never trained: no dropout in its forwards
                self.ema_net.eval()
            return self

        def load_state_dict(self, state_dict, strict=True, assign=False):
            # weights saved without the variance head, loaded into a learn_var model: the head keeps its fresh initialisation (the average's
            # head follows the net's), so that a variance head can be fine-tuned onto a trained model
            if getattr(self.net, "learn_var", False) and not any(k.startswith("net.out_var.") for k in state_dict):
                print("Loaded weights have no out_var.* keys: the variance head starts from its initialisation")
                state_dict = dict(state_dict)
                head = {k: v.detach().clone() for k, v in self.net.state_dict().items() if k.startswith("out_var.")}
                has_ema = any(k.startswith("ema_net.") for k in state_dict)
                for k, v in head.items():
                    state_dict["net." + k] = v
                    if has_ema:
                        state_dict["ema_net." + k] = v
            if getattr(self, "ema_net", None) is None:          # EMA off (or the teacher load inside __init__, before the EMA net exists)
                return super().load_state_dict(state_dict, strict=strict, assign=assign)
            if not any(k.startswith("ema_net.") for k in state_dict):      # an ordinary checkpoint: the average restarts from the loaded weights
                out = super().load_state_dict(state_dict, strict=False, assign=assign)
                missing = [k for k in out.missing_keys if not k.startswith("ema_net.")]
                if strict and (missing or out.unexpected_keys):
                    raise RuntimeError(f"Error(s) in loading state_dict for {type(self).__name__}: missing {missing}, "
                                       f"unexpected {out.unexpected_keys}")
                self.optimizer.seed_ema()
                return type(out)(missing, out.unexpected_keys)
            out = super().load_state_dict(state_dict, strict=strict, assign=assign)
            self.optimizer.ema_seeded = True
            return out

        # -- power-function averages (an extension, ema_sigma_rel): snapshots for the reconstruction of posthoc_ema.py
        def save(self, path, test_x=None, test_y=None):
            super().save(path, test_x, test_y)
            self.write_ema_snapshot(path)

        def write_ema_snapshot(self, logdir=None):
            """The power-function arenas as they stand, to <logdir>/ema_snapshots/step_<t>.pt (rank 0; reads the device: a host sync).
            Nothing before the first optimiser step, and nothing without ema_sigma_rel.  -> the path, or None"""
            opt = self.optimizer
            if not opt.gamma or opt.pema is None or opt.step_count < 1 or parallel.rank() != 0:
                return None
            return posthoc_ema.write_snapshot(self.G.logdir if logdir is None else logdir, opt.step_count, opt.sigma_rel, opt.gamma, opt.pema)

        def _after_step(self):
            if self.ema_snapshot_every > 0 and self.optimizer.step_count % self.ema_snapshot_every == 0:
                self.write_ema_snapshot()

        # -- the state of a resumable run (an extension; checkpoint.py writes it beside model.pt as train_state.pt)
        def arena_digests(self):
            """64-bit digests (ops.arena_digest) of the four arenas a resumed run must find again; None for one that does not exist (yet)."""
            opt = self.optimizer
            arenas = {"params": self.net.flat_params, "ema": None if self.ema_net is None else self.ema_net.flat_params, "m": opt.m, "v": opt.v}
            if opt.gamma:                           # with ema_sigma_rel only: one digest per power-function arena
                arenas.update({f"pema{k}": None if opt.pema is None else opt.pema[k] for k in range(len(opt.gamma))})
            return {name: None if t is None else checkpoint.arena_digest(t) for name, t in arenas.items()}

        def train_state(self):
            """Everything a continued run needs beside the weights of `state_dict()`: Adam's moments, step count and skipped-step count, the
            counters of the three Philox streams (noise and timesteps; label drop and sampling; dropout masks) and the arena digests; with
            time_importance or loss_profile on also `time_profile`, the CPU copy of the train pass's loss profile (fp32 [5, 64])."""
            state = {"optimizer": self.optimizer.state_dict(), "rng": self.diffusion.rng.state_dict(), "aux_rng": self._aux_rng.state_dict(),
                     "dropout": self.net.dropout_state(), "digests": self.arena_digests()}
            if self._profiled():
                prof = self.diffusion.time_profile
                state["time_profile"] = torch.zeros((5, ops.PROFILE_BINS)) if prof is None else prof.detach().cpu().clone()
            return state

        def _profiled(self):
            return bool(self.diffusion.time_importance or self.diffusion.loss_profile)

        def load_train_state(self, state):
            """The inverse of train_state(), on a model that has loaded the `state_dict()` saved with it: the parameter and EMA arenas must
            carry the digests the state recorded - weights of another checkpoint are refused before anything is changed."""
            want, have = state["digests"], self.arena_digests()
            for name in ("params", "ema"):
                if want[name] != have[name]:
                    as_hex = lambda d: "none" if d is None else f"{d:#018x}"
                    raise RuntimeError(f"the train state was saved with a '{name}' arena of digest {as_hex(want[name])}, the loaded weights have "
                                       f"{as_hex(have[name])}: model.pt and train_state.pt come from different checkpoints (or the ema_decay "
                                       f"flag changed) - restore the pair from one checkpoint, or start from the weights with --weights_from")
            self.optimizer.load_state_dict(state["optimizer"])
            self.diffusion.rng.load_state_dict(state["rng"])
            self._aux_rng.load_state_dict(state["aux_rng"])
            self.net.load_dropout_state(state["dropout"])
            if self._profiled():                    # a state saved without the flags carries no profile: the sampler warms up again from zeros
                prof = state.get("time_profile")
                prof = torch.zeros((5, ops.PROFILE_BINS)) if prof is None else prof.float().reshape(5, ops.PROFILE_BINS)
                self.diffusion.time_profile = prof.to(self.net.flat_params.device).contiguous()
            have = self.arena_digests()
            for name in ("m", "v"):
                if want[name] != have[name]:
                    raise RuntimeError(f"optimizer moment '{name}' does not carry the digest recorded with it: train_state.pt is damaged")
            for name in (k for k in have if k.startswith("pema")):
                if want.get(name) != have[name]:
                    raise RuntimeError(f"power-function arena '{name}' does not carry the digest recorded with it: train_state.pt is damaged")

        def _sampling_net(self):
            """The network sample() and evaluate() run: the weight average when EMA is on."""
            if self.ema_net is None:
                return self.net
            if not self.optimizer.ema_seeded:
                self.optimizer.seed_ema()
            return self.ema_net

        def _seed_target(self):
            """Consistency distillation's target network is the weight average: it has to hold the student's weights BEFORE the first target
            forward, which comes ahead of the first optimiser step (where the average is seeded otherwise).  Called at the top of train_step
            and loss(): after the constructor's teacher load, a weights_from load and a data-parallel broadcast of the initial weights."""
            if self.diffusion.target_net is not None and not self.optimizer.ema_seeded:
                self.optimizer.seed_ema()

        def _step_metrics(self, loss):
            """What train_step returns: the reference's two keys; with clipping or the guard on also `grad_norm` and `skipped_steps` (device
            scalars copied from the optimiser's state: no host sync), with a schedule on also `lr`."""
            metrics = {"loss": loss, "loss_scale": torch.tensor(1.0)}
            opt = self.optimizer
            if opt.steered:
                metrics["grad_norm"] = opt.ctl_state[ops.GRAD_NORM].clone()
                metrics["skipped_steps"] = opt.ctl_state[ops.SKIPPED].clone()
            if opt.scheduled:
                metrics["lr"] = torch.tensor(opt.last_lr, dtype=torch.float64)
            return metrics

        def _check_image(self, x):
            """A batch that cannot be this model's fails here, by name, instead of deep inside a kernel wrapper: the channel count always, the
            spatial size once `image_size` declares it (with image_size = 0 callers keep training at sizes of their own, as before; `size`
            then only shapes sample() and evaluate())."""
            C, S = self.net.in_channels, self.size
            if x.dim() != 4 or x.shape[1] != C or (self._size_declared and tuple(x.shape[2:]) != (S, S)):
                raise ValueError(f"batch of shape {tuple(x.shape)}: this model takes [B, {C}, {S}, {S}] (in_channels = {C}, image size {S}: set "
                                 f"--in_channels / --image_size / --pad32 to match the data)")

        # -- training (diffusion_model.py:63-74)
        def train_step(self, x, y):
            self._check_image(x)
            self._seed_target()
            B = x.shape[0]
            # classifier-free label drop (:67): mutates the caller's y in place like the reference, but the mask comes from the
            # device RNG inside one small kernel (the reference's CPU-generated mask forces a host sync every step)
            p_drop = float(self.G.cf_drop_prob if "cf_drop_prob" in self.G else self.DG.cf_drop_prob)
            if y.dtype == torch.int64 and y.is_contiguous() and y.data_ptr() % 16 == 0:
                ops.label_drop(y, p_drop, self._aux_rng.seed, self._aux_rng._take(B))
            else:                                   # odd label tensors (a slice, int32): same draw, torch does the masking
                y.masked_fill_(self._aux_rng.uniform((B,), x.device) < p_drop, -1)
            if self._sync is None:
                self._sync = parallel.GradSync(self.net)
            world = parallel.world()
            if self._graphable(x, world):
                return self._train_step_graphed(x, y)
            try:
                out = self.diffusion.train_forward_backward(net=partial(self.net, guide=y), x=x, grad_scale=1.0 / B,
                                                            on_grads_ready=self._sync.hook if parallel.exchanging() else None, join_side_before_ready=False)
            except BaseException:
                self._sync.abort()                  # a raise between hook() and finish() must not leave the process on the carved CU limit
                raise
            self._sync.finish()
            self.optimizer.step(grad_scale=1.0 / world)
            self._after_step()
            metrics = self._step_metrics(ops.mean(out["loss"]))
            ops.throttle()                          # at most two steps queued on the GPU (see ops.throttle)
            return metrics

        # -- small batches: the step as a replayed HIP graph ------------------------------------------------------------------
        # The reference's default invocation trains at bs = 32 (BASELINE configs[0]).  At that size a step is ~ 350 kernel launches whose host
        # side (ctypes + torch allocations, 4.6 - 5.0 ms) exceeds the GPU's work (3.5 ms): forward, loss, backward and the loss mean are captured once
        # per input shape and replayed; the random draws (same Philox streams, same order), the label drop on the CALLER's y, the copies into
        # the static inputs and the fused Adam (its step count changes every step; with it the gradient-norm launches of grad_clip / skip_nonfinite) stay outside.  Same kernels, same arguments: the
        # parameters after k steps equal the kernel-by-kernel path's bit for bit (tests/test_gpu_unet.py).  The weight gradients run on the main
        # stream inside the capture (the side stream pays at sizes that fill the chip).  Measured, same box: bs = 32 5.00 -> 3.46 ms per step,
        # bs = 64 4.69 -> 4.14, bs = 128 5.11 -> 5.23 (hence the 64 Ki-pixel limit).  GMK_TRAIN_GRAPH_PIXELS=0 turns it off.
        TRAIN_GRAPH_MAX_PIXELS = int(os.environ.get("GMK_TRAIN_GRAPH_PIXELS", str(64 * 1024)))

        def _graphable(self, x, world):
            # (the loss-profile kernels are not captured: with time_importance or loss_profile the small-batch step runs kernel by kernel)
            return (world == 1 and not parallel.exchanging() and self.teacher_net is None and self.net.dropout == 0.0 and x.is_cuda and x.dim() == 4 and
                    0 < x.shape[0] * x.shape[2] * x.shape[3] <= self.TRAIN_GRAPH_MAX_PIXELS and ops.PROFILE is None and not self._profiled())

        def _train_step_graphed(self, x, y):
            B, dev = x.shape[0], x.device
            u, eps = self.diffusion.draw_eps_u(x)               # outside the capture, like every draw ('stratified': one draw + gmk_u_stratified)
            key = (tuple(x.shape), y.dtype)
            graphs = self.__dict__.setdefault("_train_graphs", {})
            ent = graphs.get(key)
            if ent is None:
                xs, ys, es, us = x.float().clone(), y.clone(), eps.clone(), u.clone()
                side_was, side_stream = ops.WGRAD_STREAM, self.net._side
                # nothing outside the capturing stream may be joined from inside the capture; the weight gradients stay on the main stream
                # (GMK_TRAIN_GRAPH_SIDE=1 gives them a side stream of the capture's own: measured slower at these sizes, 3.68 vs 3.46 ms at bs = 32)
                ops.WGRAD_STREAM, self.net._side = side_was and os.environ.get("GMK_TRAIN_GRAPH_SIDE", "0") == "1", None
                try:
                    run = lambda: self.diffusion.train_forward_backward(net=partial(self.net, guide=ys), x=xs, grad_scale=1.0 / B, u=us, eps=es,
                                                                        on_grads_ready=self._sync.hook if parallel.exchanging() else None, join_side_before_ready=False)
                    warm = torch.cuda.Stream(device=dev)        # warm-up off the capture: packs, workspaces, allocator pools (gradients only)
                    warm.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(warm):
                        run()
                    torch.cuda.current_stream().wait_stream(warm)
                    self.net.mark_params_changed()              # the captured forward has to contain the weight re-pack every step needs
                    graph = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(graph):
                        loss = ops.mean(run()["loss"])
                finally:
                    ops.WGRAD_STREAM, self.net._side = side_was, side_stream
                ent = graphs[key] = (graph, xs, ys, es, us, loss)
                if len(graphs) > 4:
                    graphs.pop(next(iter(graphs)))
            graph, xs, ys, es, us, loss = ent
            xs.copy_(x); ys.copy_(y); es.copy_(eps); us.copy_(u)
            graph.replay()
            self.optimizer.step(grad_scale=1.0)
            self._after_step()
            metrics = self._step_metrics(loss.clone())
            ops.throttle()
            return metrics

        # -- loss (:76-80): differentiable through torch.autograd; used by the driver's test-set pass
        def loss(self, x, y):
            self._check_image(x)
            self._seed_target()
            metrics = self.diffusion.training_losses(net=partial(self.net, guide=y), x=x)
            metrics = {key: val.mean() for key, val in metrics.items()}
            if self.nlogp_samples > 0:              # the unconditional bound, nats/dim; the driver logs `nlogp` as eval/nlogp (gms/main.py:170-174)
                nlogp = self.nlogp(x)["nlogp"].mean()
                metrics["nlogp"] = nlogp
                metrics["bpd"] = nlogp / math.log(2.0)
            if self.ode_nlogp_steps > 0:            # the unconditional ODE likelihood, nats/dim; logged as <model>/test/ode_nlogp
                metrics["ode_nlogp"] = self.ode_nlogp(x)["nlogp"].mean()
            return metrics["loss"], metrics

        # -- likelihood (an extension): the variational bound of `GaussianDiffusion.nll` on the net sample() and evaluate() use
        NLOGP_SAMPLES = 16                          # draws per image when neither the call nor `nlogp_samples` gives a number

        def nlogp(self, x, y=None, num_samples=None, seed=0):
            """Per-image bound on -log p(x) (y None: unconditional, guide -1, the classifier-free branch the net is trained on) or on
            -log p(x | y) for labels y, in nats per dimension; bin half-width 1/2 for binarised data, 1/255 otherwise.  -> the dict of
            `GaussianDiffusion.nll` (nlogp, se, diffusion, prior, decoder: fp32 [B])."""
            K = num_samples or self.nlogp_samples or self.NLOGP_SAMPLES
            guide = y if y is not None else torch.full((x.shape[0],), -1, dtype=torch.long, device=x.device)
            delta = 0.5 if self.binarize else 1.0 / 255
            return self.diffusion.nll(net=partial(self._sampling_net(), guide=guide), x=x, num_samples=K, seed=seed, delta=delta)

        # -- probability-flow ODE (an extension): encode / decode / exact likelihood of `GaussianDiffusion` on the net sample() uses
        ODE_NLOGP_STEPS = 512                       # ODE steps of ode_nlogp() when neither the call nor `ode_nlogp_steps` gives a number

        def _ode_guide(self, x, y):
            return y if y is not None else torch.full((x.shape[0],), -1, dtype=torch.long, device=x.device)

        def encode(self, x, y=None, steps=None):
            """The latent code of x ([B, C, S, S]) under the probability-flow ODE (DDIM inversion) on `steps` steps (default `timesteps`);
            y: labels (the conditional ODE), None: unconditional (guide -1).  -> z, x's shape"""
            return self.diffusion.encode(net=partial(self._sampling_net(), guide=self._ode_guide(x, y)), x=x,
                                         num_steps=steps or self.diffusion.num_steps)

        def decode(self, z, y=None, steps=None):
            """The inverse of encode(): the image of the latent code z.  -> x, z's shape"""
            return self.diffusion.decode(net=partial(self._sampling_net(), guide=self._ode_guide(z, y)), z=z,
                                         num_steps=steps or self.diffusion.num_steps)

        def ode_nlogp(self, x, y=None, steps=None, seed=0):
            """Per-image -log p(x) (or -log p(x | y)) of the probability-flow ODE model, in nats per dimension, on `steps` ODE steps (default
            `ode_nlogp_steps`, else ODE_NLOGP_STEPS); bin half-width 1/2 for binarised data, 1/255 otherwise.  -> the dict of
            `GaussianDiffusion.ode_nll` (nlogp, prior, divergence: fp32 [B])."""
            N = steps or self.ode_nlogp_steps or self.ODE_NLOGP_STEPS
            delta = 0.5 if self.binarize else 1.0 / 255
            return self.diffusion.ode_nll(net=partial(self._sampling_net(), guide=self._ode_guide(x, y)), x=x, num_steps=N, seed=seed,
                                          delta=delta)

        # -- sampling (:82-87)
        def sample(self, n, y=None):
            with torch.no_grad():
                dev = self.net.flat_params.device
                noise = self._aux_rng.normal((n, self.net.in_channels, self.size, self.size), dev)
                net = partial(self._sampling_net(), guide=y)
                cond_w = 0.5 if y is not None else None
                return self.diffusion.sample(net=net, init_x=noise, cond_w=cond_w, record=False)[0][-1]

        def _crop(self):
            """Pixels evaluate() and sample_uint8() cut from every side: the pad32 border (:93-94 `x[..., 2:-2, 2:-2]`)."""
            return 2 if ("pad32" in self.G and self.G.pad32) else 0

        def sample_uint8(self, n, y=None):
            """sample(n, y) as bytes (an extension): uint8 [n, C, S', S'] on the device, quantised by evaluate()'s rule with the pad32 border cut -
            the images of a dataset file (data.load_npy's layout)."""
            return ops.to_uint8(self.sample(n, y), crop=self._crop())

        # -- inpainting (an extension): RePaint with this model's sampler on the net sample() uses
        def inpaint(self, x, mask, y=None, resample=1, seed=0):
            """Fill in the pixels of x ([B, C, S, S] in [-1, 1], the shape sample() returns) where `mask` (broadcastable to x, {0, 1}) is 0,
            keeping those where it is 1, with `GaussianDiffusion.inpaint`.  y: labels, as in sample() (then guided with cond_w = 0.5).  The
            initial noise comes from the sampler's auxiliary stream, the known-region noise from PhiloxStream(seed).  -> [B, C, S, S]"""
            with torch.no_grad():
                noise = self._aux_rng.normal(tuple(x.shape), x.device)
                net = partial(self._sampling_net(), guide=y)
                cond_w = 0.5 if y is not None else None
                return self.diffusion.inpaint(net=net, x0=x, mask=mask, init_x=noise, cond_w=cond_w, resample=resample, seed=seed)[0][-1]

        # -- restoration (an extension): DDNM super-resolution and colourisation on the net sample() uses
        def degrade(self, x, factor=1, gray=False):
            """The observation A x that `restore` starts from: x ([B, C, S, S]) averaged over factor x factor pixels and, with gray, over its
            channels (`ops.box_mean`).  -> fp32 [B, C or 1, S / factor, S / factor]"""
            x = ops.aligned(x.float().contiguous())
            cf, N, _ = restore_operator(tuple(x.shape), factor, gray)
            return ops.box_mean(x, cf, N)

        def restore(self, obs, factor=1, gray=False, y=None, seed=0):
            """An image of this model whose `degrade(., factor, gray)` is obs ([B, C or 1, S / factor, S / factor]), with
            `GaussianDiffusion.restore` (DDNM).  y: labels, as in sample() (then guided with cond_w = 0.5).  The initial noise comes from
            PhiloxStream(seed).  -> [B, C, S, S]"""
            with torch.no_grad():
                shape = (obs.shape[0], self.net.in_channels, self.size, self.size)
                noise = PhiloxStream(seed).normal(shape, obs.device)
                net = partial(self._sampling_net(), guide=y)
                cond_w = 0.5 if y is not None else None
                return self.diffusion.restore(net=net, obs=obs, factor=factor, gray=gray, init_x=noise, cond_w=cond_w)[0][-1]

        # -- posterior sampling (an extension): DPS from a noisy box-mean or blurred observation on the net sample() uses
        def measure(self, x, kind, *, noise_std=0.0, seed=0):
            """The observation A x + noise_std n that `posterior_sample` starts from: kind 'box:N', 'gray', 'gray_box:N' (`degrade`'s
            operators and format) or 'blur:SIGMA' (a Gaussian blur, x's shape); n standard normal from PhiloxStream(seed) through
            `ops.rng_normal` (nothing is drawn with noise_std = 0).  -> fp32"""
            x = ops.aligned(x.float().contiguous())
            op, low = measurement_op(kind, tuple(x.shape))
            noise_std = float(noise_std)
            if not (0.0 <= noise_std < float("inf")):
                raise ValueError(f"measure: noise_std = {noise_std}, need a finite standard deviation >= 0")
            obs = ops.measure(x, op)
            return obs if noise_std == 0.0 else obs + noise_std * PhiloxStream(seed).normal(low, x.device)

        def posterior_sample(self, obs, kind, *, zeta=None, y=None, seed=0):
            """An image of this model whose `measure(., kind)` agrees with obs up to the observation's noise, with
            `GaussianDiffusion.posterior_sample` (DPS).  zeta: the step size (None: the dps_zeta flag); y: labels (no guidance: DPS runs
            the conditional model alone).  The initial noise comes from PhiloxStream(seed).  -> [B, C, S, S]"""
            with torch.no_grad():
                shape = (obs.shape[0], self.net.in_channels, self.size, self.size)
                op, _ = measurement_op(kind, shape)
                noise = PhiloxStream(seed).normal(shape, obs.device)
                return self.diffusion.posterior_sample(net=partial(self._sampling_net(), guide=y), obs=obs, op=op, init_x=noise,
                                                       zeta=self.dps_zeta if zeta is None else zeta)[0][-1]

        # -- editing and interpolation (extensions): SDEdit and latent-code interpolation on the net sample() uses
        def edit(self, x, strength, y=None, mask=None, seed=0):
            """Edit x ([B, C, S, S] in [-1, 1]) with `GaussianDiffusion.edit`: noised up to step k = edit_start(strength, timesteps) of the
            chain (strength in (0, 1]; 1 keeps nothing of x but what `mask` keeps) and denoised from there.  y: labels, as in sample() (then
            guided with cond_w = 0.5); mask (broadcastable to x, {0, 1}): pixels with 1 come back as x's own.  The noise comes from
            PhiloxStream(seed).  -> [B, C, S, S]"""
            with torch.no_grad():
                net = partial(self._sampling_net(), guide=y)
                cond_w = 0.5 if y is not None else None
                k = edit_start(strength, self.diffusion.num_steps)
                return self.diffusion.edit(net=net, x=x, start=k, cond_w=cond_w, mask=mask, seed=seed)[0][-1]

        def interpolate(self, xa, xb, frames=9, y=None, steps=None):
            """`frames` images from xa to xb ([B, C, S, S] each) through their latent codes (`GaussianDiffusion.interpolate`) on `steps` ODE
            steps (default `timesteps`); y: labels of the pairs (the conditional ODE), None: unconditional (guide -1).  -> [frames, B, C, S, S]"""
            return self.diffusion.interpolate(net=partial(self._sampling_net(), guide=self._ode_guide(xa, y)), xa=xa, xb=xb, frames=frames,
                                              num_steps=steps or self.diffusion.num_steps)

        INPAINT_EVAL_SEED = 104723                  # evaluate()'s inpainting: initial noise from PhiloxStream(this), known-region noise from this + 1
        RESTORE_EVAL_SEED = 104759                  # evaluate()'s restoration: the initial noise (and nothing else) from PhiloxStream(this)
        DPS_EVAL_SEED = 104773                      # evaluate()'s posterior sampling: the initial noise from PhiloxStream(this), the observation's from this + 1
        EDIT_EVAL_SEED = 104743                     # evaluate()'s editing: the forward noise (and nothing else) from PhiloxStream(this)

        # -- evaluate (:89-111): 25 class-conditional samples without guidance, trajectories as uint8
        def evaluate(self, writer, x, y, epoch):
            crop = self._crop()

            def proc(t):                                              # :92's chain and the pad32 crop in one pass on the device, then the bytes move
                return ops.to_uint8(t, crop=crop).cpu()

            stream = PhiloxStream(0)                                  # :99 torch.manual_seed(0)
            noise = stream.normal((25, self.net.in_channels, self.size, self.size), x.device)
            labels = torch.arange(25, dtype=torch.long, device=x.device) % 10   # :101
            zs, xs, eps = self.diffusion.sample(net=partial(self._sampling_net(), guide=labels), init_x=noise)
            pictures = writer is not None and hasattr(writer, "write_frames")
            if pictures:                                              # an extension (common.ImageWriter): files, from the float trajectories, any shape
                writer.write_frames("samples", zs[-1], epoch, crop=crop)
                writer.write_frames("sampling_process", zs, epoch, crop=crop)
                writer.write_frames("diffusion_model/eps", eps, epoch, crop=crop)
                writer.write_frames("diffusion_model/x", xs, epoch, crop=crop)
            zs, xs, eps = proc(zs), proc(xs), proc(eps)
            self.last_eval = {"samples": zs[-1], "sampling_process": zs, "eps": eps, "x": xs}
            grids = tuple(zs.shape[2:]) == (1, 28, 28)                # the reference's grid helpers take 25 images of 1 x 28 x 28 and nothing else
            if not pictures and writer is not None and grids:         # :105-110, same tags
                common.write_grid(writer, "samples", zs[-1], epoch)
                common.write_gridvid(writer, "sampling_process", zs, epoch)
                common.write_gridvid(writer, "diffusion_model/eps", eps, epoch)
                common.write_gridvid(writer, "diffusion_model/x", xs, epoch)
            if self.inpaint_eval > 0:                                 # an extension: after everything above, on Philox streams of its own
                k = min(25, x.shape[0])
                x0 = x[:k].float()
                mask = torch.ones((1, 1, x0.shape[2], 1), dtype=torch.uint8, device=x.device)
                mask[:, :, x0.shape[2] // 2:] = 0                     # the bottom half (rows >= S / 2) is filled in
                init = PhiloxStream(self.INPAINT_EVAL_SEED).normal(tuple(x0.shape), x.device)
                z = self.diffusion.inpaint(net=partial(self._sampling_net(), guide=None if y is None else y[:k]), x0=x0, mask=mask, init_x=init,
                                           resample=self.inpaint_eval, seed=self.INPAINT_EVAL_SEED + 1)[0][-1]
                self.last_eval["inpaint"] = proc(z)
                if pictures:
                    writer.write_frames("inpaint", z, epoch, crop=crop)
                elif writer is not None and grids and k == 25:
                    common.write_grid(writer, "inpaint", self.last_eval["inpaint"], epoch)
            if self.edit_eval > 0:                                    # an extension, as above: its noise from PhiloxStream(EDIT_EVAL_SEED)
                k = min(25, x.shape[0])
                z = self.diffusion.edit(net=partial(self._sampling_net(), guide=None if y is None else y[:k]), x=x[:k].float(),
                                        start=edit_start(self.edit_eval, self.diffusion.num_steps), seed=self.EDIT_EVAL_SEED)[0][-1]
                self.last_eval["edit"] = proc(z)
                if pictures:
                    writer.write_frames("edit", z, epoch, crop=crop)
                elif writer is not None and grids and k == 25:
                    common.write_grid(writer, "edit", self.last_eval["edit"], epoch)
            if self.interp_eval > 0 and x.shape[0] >= 10:             # an extension: deterministic (no draw), unconditional
                z = self.interpolate(x[0:5].float(), x[5:10].float(), frames=self.interp_eval)
                self.last_eval["interp"] = proc(z)
                if pictures:
                    writer.write_frames("interp", z, epoch, crop=crop)
            if self.restore_eval >= 2 or self.restore_gray:           # an extension, as above: its noise from PhiloxStream(RESTORE_EVAL_SEED)
                k = min(25, x.shape[0])
                x0 = ops.aligned(x[:k].float().contiguous())
                N, gray = max(1, self.restore_eval), bool(self.restore_gray)
                cf = x0.shape[1] if gray else 1
                obs = ops.box_mean(x0, cf, N)
                init = PhiloxStream(self.RESTORE_EVAL_SEED).normal(tuple(x0.shape), x.device)
                z = self.diffusion.restore(net=partial(self._sampling_net(), guide=None if y is None else y[:k]), obs=obs, factor=N, gray=gray,
                                           init_x=init)[0][-1]
                # the replicated observation A+ obs: what a viewer would see without the model
                z_in = obs.repeat_interleave(N, dim=2).repeat_interleave(N, dim=3).repeat_interleave(cf, dim=1)
                psnr = lambda t: 10.0 * torch.log10(4.0 / (t.double() - x0.double()).square().mean(dim=(1, 2, 3)))
                self.last_eval["restore"] = proc(z)
                self.last_eval["restore_psnr"] = psnr(z).cpu()
                self.last_eval["restore_input_psnr"] = psnr(z_in).cpu()
                if pictures:
                    writer.write_frames("restore", z, epoch, crop=crop)
                    writer.write_frames("restore_input", z_in, epoch, crop=crop)
            if self.dps_eval:                                         # an extension, as above: its draws from PhiloxStream(DPS_EVAL_SEED) and the next
                k = min(25, x.shape[0])
                x0 = ops.aligned(x[:k].float().contiguous())
                op, low = measurement_op(self.dps_eval, tuple(x0.shape))
                obs = self.measure(x0, self.dps_eval, noise_std=self.dps_noise, seed=self.DPS_EVAL_SEED + 1)
                init = PhiloxStream(self.DPS_EVAL_SEED).normal(tuple(x0.shape), x.device)
                z = self.diffusion.posterior_sample(net=partial(self._sampling_net(), guide=None if y is None else y[:k]), obs=obs, op=op,
                                                    init_x=init, zeta=self.dps_zeta)[0][-1]
                # what a viewer would see without the model: the replicated box means, or the blurred image itself
                z_in = obs if op.kind == "blur" else obs.repeat_interleave(op.N, dim=2).repeat_interleave(op.N, dim=3).repeat_interleave(op.cf, dim=1)
                psnr = lambda t: 10.0 * torch.log10(4.0 / (t.double() - x0.double()).square().mean(dim=(1, 2, 3)))
                m = math.prod(low[1:])                                # observation values per image
                self.last_eval["dps"] = proc(z)
                self.last_eval["dps_psnr"] = psnr(z).cpu()
                self.last_eval["dps_input_psnr"] = psnr(z_in).cpu()
                # the mean of |obs - A z| / sqrt(m) over the images: comparable with dps_noise
                self.last_eval["dps_residual"] = float(((obs - ops.measure(z, op)).double().flatten(1).norm(dim=1) / math.sqrt(m)).mean())
                if pictures:
                    writer.write_frames("dps", z, epoch, crop=crop)
                    writer.write_frames("dps_input", z_in, epoch, crop=crop)
            random.randint(0, 2 ** 32)                                # :111 keeps the host RNG consumption

    return DiffusionModel


DiffusionModel = make_plugin(common.GM, common.AttrDict)
