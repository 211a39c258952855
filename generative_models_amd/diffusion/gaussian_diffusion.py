"""Host-side mirror of reference gms/diffusion/gaussian_diffusion.py (`GaussianDiffusion`, :19-296) over the HIP kernels.

Same constructor keywords, same `training_losses(net=, x=)` / `sample(net=, init_x=, cond_w=)` call shapes and
return structure; `net` is the HIP `SimpleUnet` or a `functools.partial` of it carrying `guide=` / `cond_w=` exactly
as the reference passes it (diffusion_model.py:77,85).  All arithmetic is in libgmk.so:

* q_sample + log-SNR schedule          gmk_q_sample     (:94-100, diffusion_utils.py:65-73,198-201)
* other schedules (`schedule=`, `sample_schedule=`)  `Schedule`: the reference's closed-form family (diffusion_utils.py:169-201: cosine, uniform, beta_const,
                                        beta_linear with logsnr_min / logsnr_max) plus an additive shift, through gmk_q_sample_sched /
                                        gmk_logsnr_schedule_sched for training and `Schedule.host` for every sampler grid; None is the reference's pick
                                        ('cosine', -20, 20, :33-34) through the entries above
* v -> x_hat/eps_hat, clip, loss, dL/dv gmk_v_loss       (:61-77,:165-169 and their backward)
* DDIM / ancestral / guidance update   gmk_sampler_step (:174-243,:292)
* DPM-Solver++(2M) update              gmk_dpm_solver_step (sampler='dpmpp_2m': an extension, no reference call site)
* variational bound (`nll`)            gmk_q_sample_logsnr, gmk_vlb_term, gmk_vlb_endpoints (an extension, no reference call site)
* RePaint inpainting (`inpaint`)       gmk_inpaint_merge after the update (an extension, no reference call site)
* dynamic thresholding (`dyn_threshold=p`)  gmk_dyn_threshold, then gmk_sampler_step_dt / gmk_dpm_solver_step_dt (Saharia et al. 2022, section 2.3;
                                        an extension, no reference call site)
* probability-flow ODE (`encode`, `decode`, `ode_nll`)  gmk_pf_ode_step, gmk_rng_rademacher, gmk_dequantize and the network's input gradient
                                        (SimpleUnet.input_vjp_hip, gmk_stem_dgrad) (an extension, no reference call site)
* loss weightings (`loss_weight=`)      'snr' through gmk_v_loss(loss_type 1); 'snr_plus1' (Salimans & Ho 2022) and 'min_snr' (Hang et al. 2023) through
                                        gmk_x_loss_w; `time_sampler='stratified'` through gmk_u_stratified (extensions, no reference call site)
* loss profile (`loss_profile=`, `time_importance=`)  gmk_loss_profile keeps the per-time profile of the loss on the device; gmk_u_importance draws
                                        the training times from it (Nichol & Dhariwal 2021, section 3.3) (extensions, no reference call site)
* editing and interpolation (`edit`, `interpolate`)  sampler chains that start part-way (`start=`), gmk_q_sample_logsnr for the forward noising, gmk_slerp
                                        between two latent codes (SDEdit, Meng et al. 2022; DDIM's interpolation, Song et al. 2021; extensions, no reference call site)
* restoration (`restore`)               gmk_box_residual, then gmk_sampler_step_ns / gmk_dpm_solver_step_ns: DDNM's projection of x-hat onto the images that
                                        agree with a low-resolution and / or grey observation (Wang, Yu & Zhang 2023; an extension, no reference call site)
* consistency distillation (`teacher_mode='consistency'`) and sampling (`sampler='consistency'`)  gmk_consistency_target (and, with
                                        `consistency_loss='huber'`, gmk_x_loss_huber) for the training target, gmk_consistency_step for the multistep
                                        sampler (Song et al. 2023, Algorithms 2 and 1; an extension, no reference call site)
* guidance interval and rescale (`guidance_interval=(lo, hi)`, `cfg_rescale=phi`)  host logic over the sampler loop - outside the interval a step
                                        forwards B images, not 2B (Kynkaanniemi et al. 2024) - and gmk_cfg_rescale ahead of the thresholded update
                                        kernels (Lin et al. 2023, section 3.4; extensions, no reference call site)
* stochastic samplers (`sampler='ancestral'` with `posterior_var`, `sampler='ddim'` with `ddim_eta > 0`, `sampler='sde_dpmpp_2m'`)
                                        gmk_stochastic_step on `stochastic_coefs`' rows: the reference's posterior (diffusion_utils.py:34-62)
                                        with each of its three variances; DDIM's eta and SDE-DPM-Solver++(2M) are extensions
* learned variance (`learn_var=1`, `posterior_var='learned'`)  the network's second output nu as the per-element weight of 'large' in the 'medium'
                                        variance (Nichol & Dhariwal 2021, section 3.1): the hybrid loss through gmk_hybrid_loss (the simple loss
                                        with gmk_v_loss's bits plus vlb_lambda times the bound term), sampler 'ancestral' through
                                        gmk_stochastic_step_lv on the 'small' rows (an extension, no reference call site)
* RNG                                   counter-based Philox streams (gmk_rng_*), keyed (seed, rank, draw index)

`mean_type` 'v' (the reference default, diffusion_model.py:21), 'eps' and 'x' (:58-63) are kernel arguments; 'both'
(:64-69) splits a 1-channel output along W in the reference and cannot run there — it raises here too.  Progressive
distillation (:87-91,:105-154) is supported: `teacher_net` is a frozen HIP `SimpleUnet`; teacher DDIM
steps run through gmk_ddim_step_vec / gmk_distill_target, the student is conditioned on the guidance weight.
"""
from collections import namedtuple
from functools import lru_cache, partial

import math
import os

import numpy as np
import torch

from .. import ops

# diffusion_utils.py:199-200 with logsnr in [-20, 20]; applied to fp32 values as fp32 scalars
SCHED_B = np.float32(np.arctan(np.exp(-0.5 * 20.0)))
SCHED_A = np.float32(np.arctan(np.exp(-0.5 * -20.0)) - np.arctan(np.exp(-0.5 * 20.0)))


def sampler_times(i, num_steps):
    """Integer loop index -> fp32 (u_t, u_s), bit-exact with gaussian_diffusion.py:288-290."""
    return np.float32(np.float32(i + 1.0) / np.float32(num_steps)), np.float32(np.float32(i) / np.float32(num_steps))


def logsnr_schedule_cosine_host(u):
    """diffusion_utils.py:198-201 for a host scalar, all in fp32."""
    u = np.float32(u)
    return np.float32(-2.0) * np.log(np.tan(SCHED_A * u + SCHED_B, dtype=np.float32), dtype=np.float32)


SCHEDULE_KINDS = ("cosine", "uniform", "beta_const", "beta_linear")
SCHEDULE_LOGSNR_BOUND = 20.0            # beyond +-20 the cosine form loses its argument to fp32 rounding (at -20 it is already 1e-3 off its float64 value)
SCHEDULE_SHIFT_BOUND = 10.0


def _softplus64(x):
    return np.logaddexp(np.float64(x), 0.0)                   # diffusion_utils.py:173-174


@lru_cache(maxsize=64)
def _schedule_coefs(kind, lmin, lmax):
    """(a, b) of `Schedule`, formed in float64 and rounded to fp32; kept, because a train step asks for them at every launch."""
    if kind == "cosine":
        b = np.arctan(np.exp(-0.5 * lmax))
        a = np.arctan(np.exp(-0.5 * lmin)) - b
    elif kind in ("beta_const", "beta_linear"):
        b = _softplus64(-lmax)
        a = _softplus64(-lmin) - b
    elif kind == "uniform":
        a = b = 0.0
    else:
        raise ValueError(f"schedule kind {kind!r}: one of {', '.join(SCHEDULE_KINDS)}")
    return np.float32(a), np.float32(b)


class Schedule(namedtuple("Schedule", "kind logsnr_min logsnr_max shift", defaults=("cosine", -20.0, 20.0, 0.0))):
    """One of the reference's closed-form log-SNR schedules u in [0, 1] -> logsnr (diffusion_utils.py:169-201; u = 0 is logsnr_max, u = 1
    logsnr_min), plus an additive `shift` (Hoogeboom et al. 2023, "simple diffusion": 2 log(32 / d) for d x d images; an extension):
      'cosine'       -2 log(tan(a u + b))        b = atan(exp(-logsnr_max / 2)), a = atan(exp(-logsnr_min / 2)) - b
      'uniform'      logsnr_min u + logsnr_max (1 - u)
      'beta_const'   -log(expm1(a u + b))        b = softplus(-logsnr_max),      a = softplus(-logsnr_min) - b
      'beta_linear'  -log(expm1(a u^2 + b))      as beta_const
    a, b are formed in float64 and rounded to fp32 (how torch applies a double scalar to an fp32 tensor); `host` is then one fp32 operation
    after another, the arithmetic of gmk_q_sample_sched.  `Schedule()` is what `GaussianDiffusion` picks in the reference (:33-34) and what
    `logsnr_schedule_cosine_host` / gmk_q_sample hold as constants.  The interpolated (table) schedules of the reference are not here."""
    __slots__ = ()

    @property
    def a(self):
        return _schedule_coefs(self.kind, float(self.logsnr_min), float(self.logsnr_max))[0]

    @property
    def b(self):
        return _schedule_coefs(self.kind, float(self.logsnr_min), float(self.logsnr_max))[1]

    @property
    def full_range(self):
        """Does the schedule run over exactly [-20, 20], the range the likelihood kernels hold as constants?"""
        return float(self.shift) == 0.0 and float(self.logsnr_min) == VLB_LOGSNR_MIN and float(self.logsnr_max) == VLB_LOGSNR_MAX

    def host(self, u):
        """logsnr(u) for a host scalar (or array), all in fp32 -> np.float32."""
        u = np.float32(u)
        a, b = self.a, self.b
        if self.kind == "cosine":
            l = np.float32(-2.0) * np.log(np.tan(a * u + b, dtype=np.float32), dtype=np.float32)
        elif self.kind == "uniform":
            l = np.float32(self.logsnr_min) * u + np.float32(self.logsnr_max) * (np.float32(1.0) - u)
        else:
            t = a * (u * u if self.kind == "beta_linear" else u) + b
            l = -np.log(np.expm1(t, dtype=np.float32), dtype=np.float32)
        return l + np.float32(self.shift) if float(self.shift) != 0.0 else l


def schedule_check(logsnr_schedule, logsnr_min, logsnr_max, logsnr_shift, sample_logsnr_schedule=""):
    """The noise-schedule options: logsnr_schedule one of SCHEDULE_KINDS, -20 <= logsnr_min < logsnr_max <= 20, |logsnr_shift| <= 10, and
    sample_logsnr_schedule the samplers' kind ('' or None: the training one; it shares the range and the shift).
    -> (training Schedule, sampling Schedule), or ValueError naming the flag."""
    if logsnr_schedule not in SCHEDULE_KINDS:
        raise ValueError(f"logsnr_schedule = {logsnr_schedule!r}: one of {', '.join(SCHEDULE_KINDS)}")
    sample_kind = logsnr_schedule if sample_logsnr_schedule in ("", None) else sample_logsnr_schedule
    if sample_kind not in SCHEDULE_KINDS:
        raise ValueError(f"sample_logsnr_schedule = {sample_logsnr_schedule!r}: '' (the training schedule) or one of {', '.join(SCHEDULE_KINDS)}")
    nums = {}
    for name, val in (("logsnr_min", logsnr_min), ("logsnr_max", logsnr_max), ("logsnr_shift", logsnr_shift)):
        try:
            nums[name] = float(val)
        except (TypeError, ValueError):
            raise ValueError(f"{name} = {val!r}: a finite number") from None
        if isinstance(val, bool) or not math.isfinite(nums[name]):
            raise ValueError(f"{name} = {val!r}: a finite number")
    lmin, lmax, shift = nums["logsnr_min"], nums["logsnr_max"], nums["logsnr_shift"]
    bound = SCHEDULE_LOGSNR_BOUND
    rule = f"-{bound:g} <= logsnr_min < logsnr_max <= {bound:g}"
    if not -bound <= lmin:
        raise ValueError(f"logsnr_min = {lmin}: below -{bound:g} the cosine form loses its argument to fp32 rounding; {rule}")
    if not lmax <= bound:
        raise ValueError(f"logsnr_max = {lmax}: above {bound:g} the cosine form loses its argument to fp32 rounding; {rule}")
    if not lmin < lmax:
        raise ValueError(f"logsnr_min = {lmin}, logsnr_max = {lmax}: {rule}")
    if abs(shift) > SCHEDULE_SHIFT_BOUND:
        raise ValueError(f"logsnr_shift = {shift}: |logsnr_shift| <= {SCHEDULE_SHIFT_BOUND:g} (2 log(32 / d) is -1.386 at 64 x 64, -4.16 at 256 x 256)")
    return Schedule(logsnr_schedule, lmin, lmax, shift), Schedule(sample_kind, lmin, lmax, shift)


def _schedule_host(schedule):
    """u -> fp32 logsnr on the host: `schedule.host`, or for None the function every default path has always called."""
    return logsnr_schedule_cosine_host if schedule is None else schedule.host


def sampler_grid(num_steps, schedule=None):
    """The samplers' time grid: one row (i, logsnr_t, logsnr_s) per loop iteration i = T-1 ... 0, fp32 host scalars.  The one place that forms
    it; the update kernels, `dpm_solver_coefs` and `inpaint_coefs` all read these values.  schedule: the `Schedule` the samplers walk
    (None: the reference's cosine on [-20, 20])."""
    return [(i, *map(_schedule_host(schedule), sampler_times(i, num_steps))) for i in range(num_steps)[::-1]]


DpmCoef = namedtuple("DpmCoef", "i lt ls h coef_z coef_x coef_prev")


def sampler_start(start, num_steps):
    """The `start` of a sampler chain that begins part-way: None is T = num_steps (the prior end, the whole chain), else an integer k with
    1 <= k <= T: the chain runs the iterations i = k-1 ... 0 from z at logsnr(k / T).  -> k, or ValueError (bools and floats included)."""
    T = int(num_steps)
    if start is None:
        return T
    if isinstance(start, bool) or not isinstance(start, (int, np.integer)) or not 1 <= start <= T:
        raise ValueError(f"start = {start!r}: None (the whole chain) or an integer in [1, num_steps = {T}]")
    return int(start)


def edit_start(strength, num_steps):
    """The `start` of `GaussianDiffusion.edit` for an SDEdit strength in (0, 1] (Meng et al. 2022: the share of the chain that is re-run, 1 the
    whole of it): k = min(T, max(1, floor(strength T + 1/2))).  -> k, or ValueError (NaN included)."""
    try:
        s = float(strength)
    except (TypeError, ValueError):
        raise ValueError(f"strength = {strength!r}: a number in (0, 1]") from None
    if not 0.0 < s <= 1.0:
        raise ValueError(f"strength = {s}: the share of the chain to re-run, in (0, 1]")
    T = int(num_steps)
    return min(T, max(1, int(math.floor(s * T + 0.5))))


def dpm_solver_coefs(num_steps, start=None, schedule=None):
    """Per-step coefficients of sampler='dpmpp_2m' (DPM-Solver++(2M), Lu et al. 2022, Algorithm 2, data prediction; an extension with no
    reference call site), one row per loop iteration i = T-1 ... 0 on DDIM's time grid.  lt / ls are the fp32 log-SNRs the DDIM path uses;
    with lambda = logsnr / 2, alpha = sqrt(sigmoid(logsnr)), sigma = sqrt(sigmoid(-logsnr)) and h = lambda_s - lambda_t:
      coef_z = sigma_s / sigma_t, coef_x = -alpha_s expm1(-h), coef_prev = 1 / (2 r), r = h_prev / h,
    so that z_s = coef_z z_t + coef_x ((1 + coef_prev) x_hat - coef_prev x_hat_prev).  coef_prev is 0 on the first step (first order: DDIM's
    update) and on the last (i == 0 returns x_hat itself, gaussian_diffusion.py:292), so T <= 2 is DDIM.  All in float64 from the fp32 log-SNRs.
    start = k (`sampler_start`) keeps the rows i = k-1 ... 0; the first of them has no history either, so its coef_prev is 0, and every later
    row is the full list's.  schedule: `sampler_grid`'s."""
    k_start = sampler_start(start, num_steps)
    sigma = lambda l: math.sqrt(1.0 / (1.0 + math.exp(l)))
    alpha = lambda l: math.sqrt(1.0 / (1.0 + math.exp(-l)))
    rows, h_prev = [], None
    for i, lt, ls in sampler_grid(num_steps, schedule):
        lt, ls = float(lt), float(ls)
        h = 0.5 * (ls - lt)
        # a zero-length previous step (coincident fp32 log-SNRs, only at extreme T) leaves no slope to extrapolate: first order again
        k = 0.0 if (not h_prev or i == 0) else h / (2.0 * h_prev)
        rows.append(DpmCoef(i, lt, ls, h, sigma(ls) / sigma(lt), -alpha(ls) * math.expm1(-h), k))
        h_prev = h
    rows = rows[len(rows) - k_start:]
    rows[0] = rows[0]._replace(coef_prev=0.0)
    return rows


StochCoef = namedtuple("StochCoef", "i lt ls coef_z coef_x coef_noise coef_prev")
STOCHASTIC_KINDS = ("ancestral", "ddim_eta", "sde_dpmpp_2m")

# What the sampler loop and every option check know about a sampler, one row per name.  tag: how an error message names it; update: the `ops`
# wrapper of its update ('stochastic_step' is 'stochastic_step_lv' under posterior_var 'learned'); noise: "" - none, "arg" - one draw per network
# evaluation, made by ops.rng_normal or injected (`noises`) and handed to the update, "kernel" - one draw per evaluation made inside the update (no
# injected noises, n % 4 == 0); thr: the update has the thresholded form (dyn_threshold, cfg_rescale); x_hist: it keeps the previous x-hat;
# inpaint: the largest `resample` it inpaints with (0: it does not inpaint); restore: it restores (the update's ns form)
SamplerCaps = namedtuple("SamplerCaps", "tag update noise thr x_hist inpaint restore")
SAMPLER_CAPS = {
    "ddim":         SamplerCaps("sampler 'ddim'",         "sampler_step",     "",       True,  False, math.inf, True),
    "noisy":        SamplerCaps("sampler 'noisy'",        "sampler_step",     "arg",    True,  False, math.inf, True),
    "teacher_test": SamplerCaps("sampler 'teacher_test'", "sampler_step",     "",       True,  False, math.inf, False),
    "dpmpp_2m":     SamplerCaps("sampler 'dpmpp_2m'",     "dpm_solver_step",  "",       True,  True,  1,        True),
    "consistency":  SamplerCaps("sampler 'consistency'",  "consistency_step", "kernel", False, False, 0,        False),
    "ancestral":    SamplerCaps("sampler 'ancestral'",    "stochastic_step",  "kernel", True,  False, 0,        False),
    "sde_dpmpp_2m": SamplerCaps("sampler 'sde_dpmpp_2m'", "stochastic_step",  "kernel", True,  True,  0,        False),
}
DDIM_ETA_CAPS = SAMPLER_CAPS["ancestral"]._replace(tag="sampler 'ddim' with ddim_eta > 0")      # the row 'ddim' takes when ddim_eta > 0
STOCHASTIC_SAMPLERS = tuple(name for name, caps in SAMPLER_CAPS.items() if caps.update == "stochastic_step")      # the names gmk_stochastic_step adds


def sampler_caps(sampler, ddim_eta=0.0):
    """The `SAMPLER_CAPS` row of a sampler name under `ddim_eta`; None for a name the loop does not know (`sample` raises NotImplementedError)."""
    return DDIM_ETA_CAPS if sampler == "ddim" and float(ddim_eta) > 0.0 else SAMPLER_CAPS.get(sampler)


# What both training passes and the autograd bridge know about an objective, one row per objective a step can apply (`loss_weight_type`, or
# 'hybrid' under learn_var).  op: the `ops` wrapper, called as op(v, [nu,] z, x, [eps,] logsnr, [logsnr_s,] grad_scale=, mean_type=, **scalars);
# eps: it reads the target noise; nu: it reads the network's variance output (the forward's want_nu, backward_hip's dnu) and logsnr_s =
# `_logsnr_prev(u)`; scalars: (wrapper keyword, attribute of the GaussianDiffusion) pairs, None for `_prepare`'s loss_type; outs: the wrapper's
# return tuple by name; grads: the names among `outs` that are gradients (None without grad_scale).  A new objective is a row here.
LossRow = namedtuple("LossRow", "op eps nu scalars outs grads")
_V_ROW = LossRow("v_loss", True, False, (("loss_type", None),), ("loss", "x_mse", "eps_mse", "dv"), ("dv",))
_XW_ROW = LossRow("x_loss_w", False, False, (("weight", "loss_weight_type"), ("gamma", "loss_gamma")), ("loss", "x_mse", "dv"), ("dv",))
LOSS_TABLE = {
    "snr_trunc": _V_ROW,
    "snr":       _V_ROW,
    "snr_plus1": _XW_ROW,
    "min_snr":   _XW_ROW,
    "huber":     LossRow("x_loss_huber", False, False, (("c", "consistency_huber_c"),), ("loss", "x_mse", "dv"), ("dv",)),
    "hybrid":    LossRow("hybrid_loss", True, True, (("vlb_lambda", "vlb_lambda"), ("loss_type", None)),
                         ("loss", "vlb", "var_frac", "x_mse", "eps_mse", "dv", "dnu"), ("dv", "dnu")),
}
TRAIN_KEYS = ("loss", "x_mse", "eps_mse", "logsnr", "vlb", "var_frac")      # what `train_forward_backward` reports of a row's outputs, in this order


def loss_row(diffusion):
    """The `LOSS_TABLE` row of a `GaussianDiffusion`: 'hybrid' under learn_var (which `learned_var_check` allows over 'snr_trunc' / 'snr'
    only), else the row of its `loss_weight_type`."""
    return LOSS_TABLE["hybrid" if diffusion.learn_var else diffusion.loss_weight_type]


# how a caller names the features in `sampler_compat_check`'s messages: a method of `GaussianDiffusion`, or the model's flags
FEATURE_WORDS = {"inpaint": "inpainting", "restore": "restoration", "dyn_threshold": "dyn_threshold", "cfg_rescale": "cfg_rescale"}
FLAG_WORDS = {**FEATURE_WORDS, "inpaint": "inpaint_eval", "restore": "restore_eval / restore_gray"}


def sampler_compat_check(caps, *, inpaint=0, restore=False, dyn_threshold=False, cfg_rescale=False, noises=False, n1=4, words=FEATURE_WORDS):
    """Does the sampler of row `caps` (`sampler_caps`; None, an unknown name, passes: the loop refuses it) go with what a call wants?  inpaint:
    0, or the `resample` count of inpainting; restore, dyn_threshold, cfg_rescale, noises (injected): is the feature asked for; n1: the values
    per image.  Every caller passes what it knows of, and names the features by `words`.  Restoration goes with none of inpainting,
    dyn_threshold and cfg_rescale (the projected x-hat must not be rescaled), whatever the sampler.  -> None, or ValueError naming both sides."""
    asked = {"inpaint": inpaint > 0, "dyn_threshold": bool(dyn_threshold), "cfg_rescale": bool(cfg_rescale), "restore": bool(restore)}
    able = caps and {"inpaint": caps.inpaint > 0, "dyn_threshold": caps.thr, "cfg_rescale": caps.thr, "restore": caps.restore}
    for feature, on in asked.items():
        if on and asked["restore"] and feature != "restore":
            raise ValueError(f"{words['restore']} together with {words[feature]} is out of scope")
        if on and caps is not None and not able[feature]:
            raise ValueError(f"{caps.tag} together with {words[feature]} is out of scope")
    drawn = caps is not None and caps.noise == "kernel"
    if caps is not None and inpaint > caps.inpaint:
        raise ValueError(f"{caps.tag} takes resample <= {caps.inpaint} only (its x-hat history has no meaning across a jump back)")
    if drawn and noises:
        raise ValueError(f"{caps.tag} draws its noise in the update kernel (self.rng's Philox stream): noises cannot be injected")
    if drawn and n1 % 4:
        raise ValueError(f"{caps.tag}: {n1} values per image, a multiple of 4 is required")


def posterior_var_frac(posterior_var):
    """The ancestral sampler's variance choice as the reference's diffusion_reverse takes it (x_logvar, diffusion_utils.py:44-61): 'small'
    (the posterior's own variance), 'large' (the forward process's) or 'medium:<frac>' (the geometric interpolation, frac in [0, 1] the weight
    of 'large').  -> frac in [0, 1] (0 small, 1 large), or ValueError naming the option."""
    what = f"posterior_var = {posterior_var!r}: 'small', 'large' or 'medium:<frac>' with frac in [0, 1]"
    if posterior_var == "small":
        return 0.0
    if posterior_var == "large":
        return 1.0
    if not isinstance(posterior_var, str) or not posterior_var.startswith("medium:"):
        raise ValueError(what)
    try:
        frac = float(posterior_var.split(":", 1)[1])
    except ValueError:
        raise ValueError(what) from None
    if not 0.0 <= frac <= 1.0:              # a NaN fails this too
        raise ValueError(what)
    return frac


def stochastic_check(sampler, posterior_var="large", ddim_eta=0.0, learn_var=False):
    """The options of the stochastic samplers: `posterior_var` (`posterior_var_frac`) is read by sampler 'ancestral' alone, `ddim_eta` in
    [0, 1] (Song et al. 2021: 0 the deterministic DDIM, 1 the ancestral 'small') by sampler 'ddim' alone; a value other than the default with
    another sampler is refused.  posterior_var 'learned' (the network's own per-element variance, gmk_stochastic_step_lv) goes with sampler
    'ancestral' on a `learn_var` network alone.  -> (kind, posterior_var, float(ddim_eta)), kind the `stochastic_coefs` family the sampler loop
    runs through gmk_stochastic_step or None for the loops that have always been there, or ValueError naming the option (NaNs included)."""
    if posterior_var == "learned":
        if not learn_var:
            raise ValueError("posterior_var = 'learned' without learn_var: the network has no variance head (train it with learn_var = 1)")
    else:
        posterior_var_frac(posterior_var)
    try:
        eta = float(ddim_eta)
    except (TypeError, ValueError):
        raise ValueError(f"ddim_eta = {ddim_eta!r}: a number in [0, 1] (0: deterministic DDIM)") from None
    if isinstance(ddim_eta, bool) or not 0.0 <= eta <= 1.0:
        raise ValueError(f"ddim_eta = {ddim_eta!r}: a number in [0, 1] (0: deterministic DDIM)")
    if posterior_var != "large" and sampler != "ancestral":
        raise ValueError(f"posterior_var = {posterior_var!r} with sampler {sampler!r}: the variance of sampler 'ancestral' only")
    if eta > 0.0 and sampler != "ddim":
        raise ValueError(f"ddim_eta = {eta} with sampler {sampler!r}: the noise share of sampler 'ddim' only")
    kind = sampler if sampler in STOCHASTIC_SAMPLERS else ("ddim_eta" if eta > 0.0 else None)
    return kind, posterior_var, eta


def stochastic_coefs(num_steps, kind, posterior_var="large", ddim_eta=0.0, start=None, schedule=None):
    """Per-step coefficients of gmk_stochastic_step, one row per loop iteration i = T-1 ... 0 on the samplers' grid, so that
      z_s = coef_z z_t + coef_x ((1 + coef_prev) x_hat - coef_prev x_hat_prev) + coef_noise xi,   xi ~ N(0, I).
    With alpha = sqrt(sigmoid(l)), sigma = sqrt(sigmoid(-l)), r = exp(lt - ls), omr = -expm1(lt - ls) and h = (ls - lt) / 2:
      'ancestral'     the posterior q(z_s | z_t, x_hat) of the reference's diffusion_reverse (diffusion_utils.py:34-62):
                      coef_z = r sqrt((1 + e^-lt) / (1 + e^-ls)), coef_x = omr alpha_s, coef_noise = exp(logvar / 2) with
                      logvar = log(omr) + f logsigmoid(-lt) + (1 - f) logsigmoid(-ls), f = `posterior_var_frac(posterior_var)`
      'ddim_eta'      DDIM with noise share eta (Song et al. 2021, eq. 12 and 16): z_s = alpha_s x_hat + sqrt(sigma_s^2 - c_n^2) eps_hat + c_n xi,
                      eps_hat = (z_t - alpha_t x_hat) / sigma_t:  coef_noise = eta sigma_s sqrt(omr),
                      coef_z = (sigma_s / sigma_t) sqrt((1 - eta^2) + eta^2 r) - this form: sqrt(1 - eta^2 omr) cancels to 0 at eta = 1 on the
                      one-step grid - and coef_x = alpha_s - alpha_t coef_z.  eta = 0 gives DDIM's own update.
      'sde_dpmpp_2m'  SDE-DPM-Solver++(2M) (Lu et al. 2022): coef_z = (sigma_s / sigma_t) e^-h, coef_x = -alpha_s expm1(-2 h),
                      coef_noise = sigma_s sqrt(-expm1(-2 h)), coef_prev = `dpm_solver_coefs`' (0 on the first row, on the last and after a
                      zero-length step).
    coef_prev is 0 for the first two kinds.  A zero-length step (coincident fp32 log-SNRs) is the identity: coef_z = 1, coef_x = coef_noise = 0.
    On the last row (i == 0) the kernel returns x_hat and draws nothing.  All in float64 from the fp32 log-SNRs of `sampler_grid`; start = k
    (`sampler_start`) keeps the rows i = k-1 ... 0, as `dpm_solver_coefs` does."""
    if kind not in STOCHASTIC_KINDS:
        raise ValueError(f"kind = {kind!r}: one of {', '.join(STOCHASTIC_KINDS)}")
    frac = 0.0 if posterior_var == "learned" else posterior_var_frac(posterior_var)      # 'learned': the 'small' rows, scaled per element in the kernel
    eta = float(ddim_eta)
    if not 0.0 <= eta <= 1.0:
        raise ValueError(f"ddim_eta = {ddim_eta!r}: a number in [0, 1]")
    k_start = sampler_start(start, num_steps)
    prev = [d.coef_prev for d in dpm_solver_coefs(num_steps, start, schedule)] if kind == "sde_dpmpp_2m" else [0.0] * k_start
    return [StochCoef(i, float(lt), float(ls), *stochastic_row(kind, lt, ls, frac, eta), k)
            for (i, lt, ls), k in zip(sampler_grid(num_steps, schedule)[num_steps - k_start:], prev)]


def stochastic_row(kind, lt, ls, frac=1.0, eta=0.0):
    """(coef_z, coef_x, coef_noise) of one step lt -> ls of `stochastic_coefs` (its closed forms; frac: `posterior_var_frac`'s), Python floats
    in float64 from the two log-SNRs as given."""
    lt, ls = float(lt), float(ls)
    if lt == ls:                                # a zero-length step: the identity, and no log(0)
        return 1.0, 0.0, 0.0
    sig = lambda l: 1.0 / (1.0 + math.exp(-l))
    logsig = lambda l: -float(_softplus64(-l))
    alpha_t, alpha_s, sigma_t, sigma_s = math.sqrt(sig(lt)), math.sqrt(sig(ls)), math.sqrt(sig(-lt)), math.sqrt(sig(-ls))
    r, omr = math.exp(lt - ls), -math.expm1(lt - ls)
    if kind == "ancestral":
        c_z = r * math.sqrt((1.0 + math.exp(-lt)) / (1.0 + math.exp(-ls)))
        c_x = omr * alpha_s
        c_n = math.exp(0.5 * (math.log(omr) + frac * logsig(-lt) + (1.0 - frac) * logsig(-ls)))
    elif kind == "ddim_eta":
        c_n = eta * sigma_s * math.sqrt(omr)
        c_z = (sigma_s / sigma_t) * math.sqrt((1.0 - eta * eta) + eta * eta * r)
        c_x = alpha_s - alpha_t * c_z
    else:
        h = 0.5 * (ls - lt)
        c_z = (sigma_s / sigma_t) * math.exp(-h)
        c_x = -alpha_s * math.expm1(-2.0 * h)
        c_n = sigma_s * math.sqrt(-math.expm1(-2.0 * h))
    return c_z, c_x, c_n


def learned_half_delta(lt, ls):
    """half_delta of gmk_stochastic_step_lv for one step lt -> ls: (softplus(ls) - softplus(lt)) / 2 = (logvar_large - logvar_small) / 2 of
    diffusion_reverse, in float64, so that `stochastic_row`'s 'small' coef_noise times exp(f half_delta) is its 'medium:f' coef_noise."""
    return 0.5 * (float(_softplus64(float(ls))) - float(_softplus64(float(lt))))


VLB_LAMBDA = 0.001          # the weight of the bound term in the hybrid loss (Nichol & Dhariwal 2021, section 3.1)
VLB_STEPS = 1000            # T of the bound's time pairs (u, max(u - 1 / T, 0))


def learned_var_check(learn_var, vlb_lambda=VLB_LAMBDA, vlb_steps=VLB_STEPS, has_teacher=False, loss_weight="snr_trunc"):
    """The options of a learned reverse-process variance (Nichol & Dhariwal 2021, section 3.1; an extension, off by default): `learn_var` 0 / 1
    - the network carries the variance head and trains on the hybrid loss (gmk_hybrid_loss) simple + vlb_lambda vlb; `vlb_lambda` finite and
    >= 0; `vlb_steps` = T >= 1, the grid of the bound's time pairs.  Not with a teacher (teacher_mode step1 / step2 / consistency) and with
    loss_weight 'snr_trunc' or 'snr' only (the two objectives gmk_v_loss forms).  -> (bool(learn_var), float(vlb_lambda), int(vlb_steps)), or
    ValueError naming the option (NaNs included)."""
    if isinstance(learn_var, str) or learn_var not in (0, 1):
        raise ValueError(f"learn_var = {learn_var!r}: 0 (off) or 1")
    try:
        lam = float(vlb_lambda)
    except (TypeError, ValueError):
        raise ValueError(f"vlb_lambda = {vlb_lambda!r}: a finite number >= 0") from None
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"vlb_lambda = {vlb_lambda!r}: a finite number >= 0")
    try:
        T = int(vlb_steps)
        whole = T == float(vlb_steps)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"vlb_steps = {vlb_steps!r}: an integer >= 1") from None
    if not whole or T < 1:
        raise ValueError(f"vlb_steps = {vlb_steps!r}: an integer >= 1")
    if learn_var:
        if has_teacher:
            raise ValueError("learn_var = 1 with teacher_path (teacher_mode step1 / step2 / consistency): a learned variance for the distillation "
                             "modes is out of scope")
        if loss_weight not in ("snr_trunc", "snr"):
            raise ValueError(f"learn_var = 1 with loss_weight = {loss_weight!r}: the hybrid loss adds the bound to 'snr_trunc' or 'snr' only")
    return bool(learn_var), lam, T


def dyn_threshold_check(p):
    """The dynamic-thresholding option: 0 is off, else the percentile p in (0, 1].  -> float(p), or ValueError (NaN included)."""
    try:
        p = float(p)
    except (TypeError, ValueError):
        raise ValueError(f"dyn_threshold = {p!r}: 0 (off) or a percentile in (0, 1]") from None
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dyn_threshold = {p}: 0 (off) or a percentile in (0, 1]")
    return p


def guidance_check(interval, phi, sampler="ddim", dyn_threshold=0.0):
    """The options of the guided samplers beyond the weight: `interval` None (guidance at every step) or (lo, hi), lo <= hi, the band of
    log-SNRs in which a step is guided (Kynkaanniemi et al. 2024; either end may be infinite, (-inf, inf) is None); `phi` the rescale of the
    guided prediction (Lin et al. 2023, section 3.4): 0 is off, else in (0, 1].  phi > 0 does not go with dyn_threshold (both set the update's
    threshold) nor with a sampler whose update has no thresholded form (`sampler_compat_check`).  -> (interval as None or a pair of floats,
    float(phi)), or ValueError naming the option (NaNs included)."""
    if interval is not None:
        try:
            lo, hi = interval
            lo, hi = float(lo), float(hi)
        except (TypeError, ValueError):
            raise ValueError(f"guidance_interval = {interval!r}: None or a pair (lo, hi) of log-SNRs, lo <= hi") from None
        if not lo <= hi:                            # a NaN fails this too
            raise ValueError(f"guidance_interval = ({lo}, {hi}): None or a pair (lo, hi) of log-SNRs, lo <= hi")
        interval = None if (lo == -math.inf and hi == math.inf) else (lo, hi)
    try:
        phi = float(phi)
    except (TypeError, ValueError):
        raise ValueError(f"cfg_rescale = {phi!r}: 0 (off) or a factor in (0, 1]") from None
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"cfg_rescale = {phi}: 0 (off) or a factor in (0, 1]")
    if phi > 0.0 and dyn_threshold:
        raise ValueError(f"cfg_rescale = {phi} together with dyn_threshold = {dyn_threshold}: both set the threshold of the update; choose one")
    sampler_compat_check(sampler_caps(sampler), cfg_rescale=phi > 0.0)
    return interval, phi


def guidance_mask(plan, interval):
    """One bool per row of a `sampler_plan`: is the step guided?  lo <= lt <= hi on the row's fp32 network time lt as a Python float;
    interval None: every row."""
    if interval is None:
        return [True] * len(plan)
    lo, hi = interval
    return [lo <= float(step.lt) <= hi for step in plan]


def guidance_evals(plan, mask, B):
    """Images forwarded by a guided call of B images over `plan`: a guided row costs 2 B per network evaluation (the conditional and the
    unconditional batch), another B."""
    return sum(step.passes * (2 * B if g else B) for step, g in zip(plan, mask))


LOSS_WEIGHTS = ("snr_trunc", "snr", "snr_plus1", "min_snr")
TIME_SAMPLERS = ("uniform", "stratified")


def loss_weight_check(loss_weight, loss_gamma, time_sampler, has_teacher=False):
    """The training-objective options: loss_weight 'snr_trunc' (the reference's max(x_mse, eps_mse)), 'snr' (eps_mse), 'snr_plus1'
    ((1 + e^logsnr) x_mse) or 'min_snr' (min(e^logsnr, loss_gamma) x_mse); loss_gamma finite and > 0; time_sampler 'uniform' (independent
    draws) or 'stratified' (one offset per batch, evenly spaced times).  With a teacher only the defaults: distillation sets its own
    weighting, and its step 2 draws discrete times.  -> (loss_weight, float(loss_gamma), time_sampler), or ValueError naming the flag."""
    if loss_weight not in LOSS_WEIGHTS:
        raise ValueError(f"loss_weight = {loss_weight!r}: one of {', '.join(LOSS_WEIGHTS)}")
    if time_sampler not in TIME_SAMPLERS:
        raise ValueError(f"time_sampler = {time_sampler!r}: one of {', '.join(TIME_SAMPLERS)}")
    try:
        gamma = float(loss_gamma)
    except (TypeError, ValueError):
        raise ValueError(f"loss_gamma = {loss_gamma!r}: a finite number > 0") from None
    if not (math.isfinite(gamma) and gamma > 0.0):
        raise ValueError(f"loss_gamma = {gamma}: a finite number > 0")
    if has_teacher and loss_weight != "snr_trunc":
        raise ValueError(f"loss_weight = {loss_weight!r} with a teacher (teacher_path): distillation sets its own weighting; leave loss_weight "
                         f"at 'snr_trunc'")
    if has_teacher and time_sampler != "uniform":
        raise ValueError(f"time_sampler = {time_sampler!r} with a teacher (teacher_path): distillation step 2 draws discrete times; leave "
                         f"time_sampler at 'uniform'")
    return loss_weight, gamma, time_sampler


def time_importance_check(time_importance, importance_decay, importance_warmup, importance_floor, loss_profile, has_teacher=False, world=1):
    """The loss-profile options: time_importance 0 | 1 (draw training times with p(t) proportional to sqrt(E[L_t^2]) of the running profile and
    reweight by 1 / p: Nichol & Dhariwal 2021, section 3.3), loss_profile 0 | 1 (keep the per-time profile of the train and test losses without
    sampling from it); importance_decay in (0, 1] (a bin's window over its own samples), importance_warmup >= 0 (samples every bin must hold
    before the sampler leaves uniform), importance_floor in (0, 1] (the uniform share of p).  With decay < 1 a bin's count settles at
    1 / (1 - decay); warmup <= 0.5 / (1 - decay), half of that, is asked: then W >= warmup implies decay W + 1 >= warmup, so a bin that has
    reached the warm-up count never falls below it again, and the sampler cannot flip back to uniform.  Not with a teacher (distillation step 2 draws
    discrete times); time_importance not with more than one rank.
    -> (time_importance, decay, warmup, floor, loss_profile) as (int, float, float, float, int), or ValueError naming the flag."""
    flags = {}
    for name, val in (("time_importance", time_importance), ("loss_profile", loss_profile)):
        try:
            ok = not isinstance(val, bool) and float(val) in (0.0, 1.0)
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError(f"{name} = {val!r}: 0 (off) or 1")
        flags[name] = int(val)
    nums = {}
    for name, val in (("importance_decay", importance_decay), ("importance_warmup", importance_warmup), ("importance_floor", importance_floor)):
        try:
            nums[name] = float(val)
        except (TypeError, ValueError):
            raise ValueError(f"{name} = {val!r}: a number") from None
    decay, warmup, floor = nums["importance_decay"], nums["importance_warmup"], nums["importance_floor"]
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"importance_decay = {decay}: the per-bin decay of the loss profile, in (0, 1]")
    if not 0.0 < floor <= 1.0:
        raise ValueError(f"importance_floor = {floor}: the uniform share of the sampling distribution, in (0, 1]")
    if not (warmup >= 0.0 and math.isfinite(warmup)):
        raise ValueError(f"importance_warmup = {warmup}: the sample count every bin must hold before the sampler leaves uniform, >= 0")
    if decay < 1.0 and warmup * (1.0 - decay) > 0.5 + 1e-9:         # (1e-9: 1 - decay is not exact in binary; 0.99 and 50 pass)
        raise ValueError(f"importance_warmup = {warmup} with importance_decay = {decay}: above 0.5 / (1 - decay) = {0.5 / (1.0 - decay):g} a bin that "
                         f"reached the warm-up count could fall below it again (its count settles at {1.0 / (1.0 - decay):g}) and the sampler "
                         f"would flip back to uniform; lower importance_warmup or raise importance_decay")
    for name, on in flags.items():
        if on and has_teacher:
            raise ValueError(f"{name} = 1 with a teacher (teacher_path): distillation step 2 draws discrete times; leave {name} at 0")
    if flags["time_importance"] and int(world) > 1:
        raise ValueError(f"time_importance = 1 on {int(world)} ranks: one train_state.pt serves every rank, and a replicated loss profile needs a "
                         f"per-step collective that nobody here can test; importance sampling runs on one rank only (loss_profile = 1 does run "
                         f"data-parallel: every rank keeps its own profile)")
    return flags["time_importance"], decay, warmup, floor, flags["loss_profile"]


TEACHER_MODES = ("step1", "step2", "consistency")
CONSISTENCY_LOSSES = ("l2", "huber")


def consistency_check(teacher_mode, has_teacher, consistency_grid=0, consistency_loss="l2", consistency_huber_c=0.00054):
    """The consistency-distillation options (Song et al. 2023, Algorithm 2): teacher_mode 'consistency' needs a teacher (teacher_path);
    consistency_grid N >= 0, the training discretisation (0: `timesteps`); consistency_loss 'l2' (the truncated-SNR loss of distillation step 2
    against the consistency target) or 'huber' (pseudo-Huber on x, Song & Dhariwal 2023) with consistency_huber_c finite and > 0.  The grid and
    'huber' belong to teacher_mode 'consistency' alone.  -> (on, int(grid), loss, float(c)), or ValueError naming the flags."""
    on = teacher_mode == "consistency"
    if on and not has_teacher:
        raise ValueError("teacher_mode = 'consistency' without teacher_path: consistency distillation needs a frozen teacher")
    try:
        ok = not isinstance(consistency_grid, bool) and int(consistency_grid) == float(consistency_grid)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"consistency_grid = {consistency_grid!r}: 0 (timesteps) or the number of training time points N >= 1")
    grid = int(consistency_grid)
    if grid < 0:
        raise ValueError(f"consistency_grid = {grid}: 0 (timesteps) or the number of training time points N >= 1")
    if consistency_loss not in CONSISTENCY_LOSSES:
        raise ValueError(f"consistency_loss = {consistency_loss!r}: one of {', '.join(CONSISTENCY_LOSSES)}")
    try:
        c = float(consistency_huber_c)
    except (TypeError, ValueError):
        raise ValueError(f"consistency_huber_c = {consistency_huber_c!r}: a finite number > 0") from None
    if isinstance(consistency_huber_c, bool) or not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"consistency_huber_c = {consistency_huber_c!r}: a finite number > 0")
    if not on and consistency_loss != "l2":
        raise ValueError(f"consistency_loss = {consistency_loss!r} without teacher_mode = 'consistency': the loss of consistency distillation only")
    if not on and grid > 0:
        raise ValueError(f"consistency_grid = {grid} without teacher_mode = 'consistency': the time grid of consistency distillation only")
    return on, grid, consistency_loss, c


def profile_bin_edges(schedule=None):
    """The 64 bins of the loss profile on the host: (u_lo, u_hi, logsnr_hi, logsnr_lo), fp32 [64] each - bin k is [k / 64, (k + 1) / 64) in u,
    and its log-SNR range follows from the training schedule (a `Schedule`'s host, None: `logsnr_schedule_cosine_host`; the schedule falls, so
    u_lo carries the high end)."""
    n = ops.PROFILE_BINS
    u_lo = np.arange(n, dtype=np.float32) / np.float32(n)
    u_hi = np.arange(1, n + 1, dtype=np.float32) / np.float32(n)
    host = _schedule_host(schedule)
    return u_lo, u_hi, host(u_lo), host(u_hi)


def profile_rows(state, p=None, schedule=None):
    """Host view of a profile state (fp32 [5, 64] array): dict of [64] arrays - u_lo, u_hi, logsnr_hi, logsnr_lo (`profile_bin_edges(schedule)`), weight = W,
    loss_mean = S1_0 / W, loss_rms = sqrt(S2_0 / W), x_mse_mean = S1_1 / W (NaN where W = 0), and p: the sampling probabilities given, or None."""
    s = np.asarray(state, dtype=np.float64)
    if s.shape != (5, ops.PROFILE_BINS):
        raise ValueError(f"profile state of shape {s.shape}, expected (5, {ops.PROFILE_BINS})")
    u_lo, u_hi, l_hi, l_lo = profile_bin_edges(schedule)
    with np.errstate(divide="ignore", invalid="ignore"):
        W = s[0]
        rows = {"u_lo": u_lo, "u_hi": u_hi, "logsnr_hi": l_hi, "logsnr_lo": l_lo, "weight": W, "loss_mean": s[1] / W, "loss_rms": np.sqrt(s[2] / W),
                "x_mse_mean": s[3] / W, "p": None if p is None else np.asarray(p, dtype=np.float64)}
    return rows


def dyn_threshold_rank(p, n):
    """Where the p-quantile (0 < p <= 1) of n sorted values lies, by torch.quantile's linear rule: pos = p (n - 1) in double, k_lo = floor(pos),
    frac = fp32(pos - k_lo); the quantile is a[k_lo] + frac (a[min(k_lo + 1, n - 1)] - a[k_lo]).  The arguments of gmk_dyn_threshold, which asks
    for 0 <= frac < 1: a remainder within half an fp32 ulp below 1 (it would round to 1.0f) names the next rank itself, (k_lo + 1, 0).
    p = 1 gives (n - 1, 0), n = 1 gives (0, 0).  -> (k_lo, frac) as Python int and float."""
    p, n = float(p), int(n)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"dyn_threshold_rank: p = {p} outside (0, 1]")
    if n < 1 or n >= 1 << 31:
        raise ValueError(f"dyn_threshold_rank: n = {n} outside [1, 2^31)")
    pos = p * (n - 1)
    k_lo = min(int(math.floor(pos)), n - 1)
    frac = float(np.float32(pos - k_lo))
    if frac >= 1.0:
        k_lo, frac = k_lo + 1, 0.0
    if k_lo >= n - 1:                       # the top rank has no neighbour above it
        k_lo, frac = n - 1, 0.0
    return k_lo, frac


InpaintCoef = namedtuple("InpaintCoef", "i lt ls alpha_s sigma_s a b is_last")


def inpaint_coefs(num_steps, schedule=None):
    """Per-step coefficients of `GaussianDiffusion.inpaint` (RePaint, Lugmayr et al. 2022, Algorithm 1), one row per loop iteration
    i = T-1 ... 0 on DDIM's time grid; lt / ls are the fp32 log-SNRs the sampler uses.  With alpha^2 = sigmoid(l), sigma^2 = sigmoid(-l):
      alpha_s, sigma_s  the known region's noisy copy alpha_s x0 + sigma_s eps at time s
      a, b              the forward transition q(z_t | z_s) = N(a z_s, b^2), a = alpha_t / alpha_s, b^2 = 1 - alpha_t^2 / alpha_s^2,
                        formed as b^2 = -expm1(lt - ls) sigma_t^2 (no cancellation), so that a^2 sigma_s^2 + b^2 = sigma_t^2
      is_last           i == 0: the known region is x0 itself and the step never re-noises.
    All in float64 from the fp32 log-SNRs.  schedule: `sampler_grid`'s."""
    sig = lambda l: 1.0 / (1.0 + math.exp(-l))
    rows = []
    for i, lt, ls in sampler_grid(num_steps, schedule):
        lt, ls = float(lt), float(ls)
        a = math.sqrt(sig(lt) / sig(ls))
        b = math.sqrt(-math.expm1(lt - ls) * sig(-lt))
        rows.append(InpaintCoef(i, lt, ls, math.sqrt(sig(ls)), math.sqrt(sig(-ls)), a, b, i == 0))
    return rows


def inpaint_passes(i, resample):
    """Network evaluations of inpainting step i: `resample`, the last step (i == 0) one - it never re-noises.  A call of T steps costs
    T r - (r - 1) forwards."""
    return 1 if i == 0 else int(resample)


class SamplerStep(namedtuple("SamplerStep", "i lt ls is_last passes dpm inp")):
    """One row of `sampler_plan`.  The seven tuple fields are what they have always been (plans are compared, sliced and unpacked as tuples);
    `sto`, the stochastic samplers' StochCoef row, trails them as an eighth constructor argument that defaults to None and rides as an
    attribute, so a plan without it is the tuple it always was.  Two rows are equal when their tuples and their `sto` are."""

    sto = None                              # (what `_make` leaves: it builds the tuple without the constructor)

    def __new__(cls, i, lt, ls, is_last, passes, dpm, inp, sto=None):
        self = super().__new__(cls, i, lt, ls, is_last, passes, dpm, inp)
        self.sto = sto
        return self

    def __getnewargs__(self):               # copy and pickle keep the row
        return (*self, self.sto)

    def _replace(self, **kwargs):
        sto = kwargs.pop("sto", self.sto)
        return type(self)(*super()._replace(**kwargs), sto)

    def __eq__(self, other):
        return tuple.__eq__(self, other) is True and getattr(other, "sto", None) == self.sto

    def __ne__(self, other):
        return not self == other

    def __hash__(self):
        return hash((tuple(self), self.sto))

    def __repr__(self):
        return super().__repr__()[:-1] + f", sto={self.sto!r})"


# what inpainting adds to the sampler loop: x0 and the uint8 mask [B, n] (of the whole batch, or of a chunk's rows), the known-region
# PhiloxStream, resample, and the whole-batch Philox counter of each network evaluation's merge (filled as the loop reserves them)
InpaintState = namedtuple("InpaintState", "x0 mask rng resample B_total moffs")


# what restoration (DDNM) adds to the sampler loop: the observation obs = A x, fp32 [B, C / cf, H / N, W / N] (of the whole batch, or of a
# chunk's rows), and the box-mean operator's parameters (cf channels averaged together, an N x N spatial box)
RestoreState = namedtuple("RestoreState", "obs cf N")


def restore_operator(shape, factor=1, gray=False):
    """The box-mean operator of `restore` / `degrade` on images of `shape` = [B, C, H, W]: factor = N (the side of the spatial box, N = 1 keeps
    the resolution), gray = average the C channels.  -> (cf, N, observation shape [B, C / cf, H / N, W / N]), or ValueError: a shape that is
    not [B, C, H, W], N not an integer >= 1 dividing H and W, gray with C == 1, or k = cf N^2 < 2 (nothing is degraded)."""
    if len(shape) != 4 or 0 in shape:
        raise ValueError(f"restore: shape {tuple(shape)}, expected [B, C, H, W] with every dimension > 0")
    B, C, H, W = (int(d) for d in shape)
    N = factor
    if isinstance(N, bool) or not isinstance(N, (int, np.integer)) or N < 1:
        raise ValueError(f"restore: factor = {factor!r}, need an integer >= 1")
    N = int(N)
    if H % N or W % N:
        raise ValueError(f"restore: factor = {N} does not divide H = {H} and W = {W}")
    if gray and C == 1:
        raise ValueError("restore: gray = True with one channel: there is no colour to restore")
    cf = C if gray else 1
    if cf * N * N < 2:
        raise ValueError("restore: factor = 1 without gray: the box size k = cf factor^2 is 1, the observation is the image itself")
    return cf, N, (B, C // cf, H // N, W // N)


# what diffusion posterior sampling (DPS) measures with: a linear operator A on [B, C, H, W] images.  kind 'box': `restore_operator`'s (cf, N)
# box mean (sigma 0, no taps); kind 'blur': a separable Gaussian of width sigma with zero padding, taps = `blur_taps(sigma)` (cf = N = 1)
MeasurementOp = namedtuple("MeasurementOp", "kind cf N sigma taps")
BLUR_MAX_SIGMA = 5.0
DPS_SAMPLERS = ("ddim", "noisy", "ancestral")       # the samplers `posterior_sample` runs ('ddim' also with ddim_eta > 0: ancestral's kernel)
DPS_KINDS = "'box:N', 'gray', 'gray_box:N' or 'blur:SIGMA'"


def blur_taps(sigma):
    """The taps of the Gaussian blur: t_k = exp(-k^2 / (2 sigma^2)) for |k| <= R = min(ceil(3 sigma), 15), 0 < sigma <= 5, divided by their
    full sum in float64 and rounded once to fp32.  -> tuple of 2 R + 1 floats (taps[k + R] weighs offset k), or ValueError."""
    try:
        sigma = float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"blur: sigma = {sigma!r}, need a width in (0, {BLUR_MAX_SIGMA:g}]") from None
    if not 0.0 < sigma <= BLUR_MAX_SIGMA:
        raise ValueError(f"blur: sigma = {sigma}, need a width in (0, {BLUR_MAX_SIGMA:g}]")
    R = min(int(math.ceil(3.0 * sigma)), 15)
    t = np.exp(-np.arange(-R, R + 1, dtype=np.float64) ** 2 / (2.0 * sigma * sigma))
    return tuple(float(v) for v in (t / t.sum()).astype(np.float32))


def measurement_op(kind, shape):
    """The `MeasurementOp` a string names on images of `shape` = [B, C, H, W], and its observation's shape: 'box:N' (N x N box means), 'gray'
    (the channel mean), 'gray_box:N' (both) - `restore`'s operators and observation format - or 'blur:SIGMA' (the observation has the image's
    shape; H, W <= 64).  -> (op, observation shape), or ValueError naming the string."""
    bad = ValueError(f"measurement {kind!r}: expected {DPS_KINDS}")
    if not isinstance(kind, str):
        raise bad
    name, sep, arg = kind.partition(":")
    if name not in ("box", "gray", "gray_box", "blur") or (name == "gray") != (sep == "") or (sep and not arg):
        raise bad
    if name == "blur":
        try:
            sigma = float(arg)
        except ValueError:
            raise bad from None
        taps = blur_taps(sigma)
        if len(shape) != 4 or 0 in shape:
            raise ValueError(f"measurement {kind!r}: shape {tuple(shape)}, expected [B, C, H, W] with every dimension > 0")
        if max(int(shape[2]), int(shape[3])) > 64:
            raise ValueError(f"measurement {kind!r}: H = {shape[2]}, W = {shape[3]}, the blur takes at most 64 x 64 images")
        return MeasurementOp("blur", 1, 1, sigma, taps), tuple(int(d) for d in shape)
    try:
        N = int(arg) if sep else 1
    except ValueError:
        raise bad from None
    cf, N, low = restore_operator(shape, N, name.startswith("gray"))
    return MeasurementOp("box", cf, N, 0.0, ()), low


def dps_check(*, sampler, ddim_eta=0.0, mean_type="v", cond_w=False, dyn_threshold=False, cfg_rescale=False, learned_var=False, student=False,
              what="posterior_sample"):
    """Does `posterior_sample` (DPS) go with the options?  sampler: one of `DPS_SAMPLERS`; cond_w (classifier-free guidance), dyn_threshold,
    cfg_rescale, learned_var (posterior_var 'learned'), student (a distilled student): asked for or not; mean_type 'eps' is refused - its
    c_z = 1 / alpha_t is about 2e4 at the first step.  `what` names the caller's side.  -> None, or ValueError naming both sides."""
    if sampler not in DPS_SAMPLERS:
        raise ValueError(f"{what} together with sampler {sampler!r} is out of scope (it runs {', '.join(map(repr, DPS_SAMPLERS))})")
    for on, word in ((cond_w, "classifier-free guidance (cond_w)"), (dyn_threshold, "dyn_threshold"), (cfg_rescale, "cfg_rescale"),
                     (learned_var, "a learned variance (learn_var, posterior_var 'learned')"), (student, "a distilled student (teacher_net)"),
                     (mean_type == "eps", "mean_type 'eps' (c_z = 1 / alpha_t is about 2e4 at the first step)")):
        if on:
            raise ValueError(f"{what} together with {word} is out of scope")
    stochastic_check(sampler, "large", ddim_eta, False)


def dps_zeta_check(zeta, what="posterior_sample"):
    """zeta, the DPS step size: finite, >= 0 (0: no guidance).  -> float, or ValueError"""
    try:
        z = float(zeta)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: zeta = {zeta!r}, need a finite step size >= 0") from None
    if not (math.isfinite(z) and 0.0 <= z < 1e38):
        raise ValueError(f"{what}: zeta = {zeta!r}, need a finite step size >= 0")
    return z


def dps_coefs(logsnr_t, mean_type):
    """(c_z, c_o) = d x-hat / d (z, out) of the unclipped prediction at logsnr_t, in float64: 'v' (alpha_t, -sigma_t), 'eps' (1 / alpha_t,
    -sigma_t / alpha_t), 'x' (0, 1)."""
    l = float(logsnr_t)
    alpha, sigma = math.sqrt(1.0 / (1.0 + math.exp(-l))), math.sqrt(1.0 / (1.0 + math.exp(l)))
    if mean_type == "v":
        return alpha, -sigma
    if mean_type == "eps":
        return 1.0 / alpha, -sigma / alpha
    if mean_type == "x":
        return 0.0, 1.0
    raise ValueError(f"mean_type {mean_type!r}")


def sampler_plan(num_steps, sampler="ddim", resample=None, start=None, schedule=None, posterior_var="large", ddim_eta=0.0, learn_var=False):
    """One row per sampler iteration i = T-1 ... 0: the grid's (i, lt, ls), is_last, the network evaluations of the step (`resample`: the
    inpainting loop's, None outside it) and the step's DpmCoef (sampler 'dpmpp_2m') / InpaintCoef (inpainting) rows, else None ('consistency':
    DDIM's rows - gmk_consistency_step forms its two coefficients from ls itself); `sto`: the step's StochCoef row when `stochastic_check`
    (sampler, posterior_var, ddim_eta) names a kind - samplers 'ancestral', 'sde_dpmpp_2m' and 'ddim' with ddim_eta > 0 - else None.  The loop
    reserves its Philox counters and every chunk spends them by walking the same plan.  start = k (`sampler_start`): a chain that begins
    part-way, from z at plan[0].lt = logsnr(k / T) - the rows i = k-1 ... 0 of the same grid (None: all T of them).  schedule: `sampler_grid`'s."""
    k = sampler_start(start, num_steps)
    skip = num_steps - k
    dpm = dpm_solver_coefs(num_steps, start, schedule) if sampler == "dpmpp_2m" else [None] * k
    inp = inpaint_coefs(num_steps, schedule)[skip:] if resample is not None else [None] * k
    kind, posterior_var, ddim_eta = stochastic_check(sampler, posterior_var, ddim_eta, learn_var)
    sto = stochastic_coefs(num_steps, kind, posterior_var, ddim_eta, start, schedule) if kind else [None] * k
    return [SamplerStep(i, lt, ls, i == 0, 1 if resample is None else inpaint_passes(i, resample), d, c, e)
            for (i, lt, ls), d, c, e in zip(sampler_grid(num_steps, schedule)[skip:], dpm, inp, sto)]


# the variational bound's log-SNR range: the schedule's truncation (diffusion_utils.py:199-200)
VLB_LOGSNR_MAX, VLB_LOGSNR_MIN = 20.0, -20.0


def stratified_logsnr(u0, K):
    """fp32 [K, B] log-SNRs lambda_{b,k} = lambda_max - Delta frac(u0_b + k / K) of `GaussianDiffusion.nll`: uniform in lambda, one draw of
    each image in each of the K equal strata of [lambda_min, lambda_max].  Formed in float64 (an fp32 sum u0 + k / K can round onto the
    next stratum's edge), then rounded to fp32."""
    k = torch.arange(K, device=u0.device, dtype=torch.float64)[:, None] / K
    frac = torch.remainder(u0.double()[None, :] + k, 1.0)
    return (VLB_LOGSNR_MAX - (VLB_LOGSNR_MAX - VLB_LOGSNR_MIN) * frac).float()


def ode_logsnr_grid(num_steps, schedule=None):
    """The probability-flow ODE's time grid, the samplers' own: lambda_i = schedule(i / N) in fp32 for i = 0 ... N (lambda_0 = 20, the data end;
    lambda_N = -20, the prior end, under the default schedule, None: the reference's cosine on [-20, 20]), as Python floats."""
    N = int(num_steps)
    host = _schedule_host(schedule)
    return [float(host(np.float32(np.float32(i) / np.float32(N)))) for i in range(N + 1)]


def ode_trapezoid_weights(lam):
    """w_i of the trapezoid rule over the grid `lam` (decreasing): sum_{i<N} 1/2 (lambda_i - lambda_{i+1}) (d_i + d_{i+1}) = sum_i w_i d_i."""
    N = len(lam) - 1
    return [0.5 * ((lam[i - 1] - lam[i] if i > 0 else 0.0) + (lam[i] - lam[i + 1] if i < N else 0.0)) for i in range(N + 1)]


def ode_divergence_coefs(logsnr, D, mean_type):
    """(a, b) with d = a + b r.g the Hutchinson estimate of the divergence of the probability-flow drift f(z, lambda) = 1/2 sigma^2 z -
    1/2 sigma eps_hat(z, lambda) (dz / d lambda) at one point: d = 1/2 sigma^2 D - 1/2 sigma (c_z D + c_o r.g), g = (d out / d z)^T r,
    (c_z, c_o) = (sigma, alpha) 'v', (0, 1) 'eps', (1 / sigma, -alpha / sigma) 'x'.  In float64; the constant a is formed without
    cancellation ('v': 0, 'x': -1/2 alpha^2 D)."""
    a2 = 1.0 / (1.0 + math.exp(-logsnr))
    s2 = 1.0 / (1.0 + math.exp(logsnr))
    alpha, sigma = math.sqrt(a2), math.sqrt(s2)
    if mean_type == "v":
        return 0.0, -0.5 * sigma * alpha
    if mean_type == "eps":
        return 0.5 * s2 * D, -0.5 * sigma
    if mean_type == "x":
        return -0.5 * a2 * D, 0.5 * alpha
    raise ValueError(f"mean_type {mean_type!r}")


class _EvalForward:
    """`module` without dropout for the duration of a with-block, whatever its training flag (its forward reads the flag)."""

    def __init__(self, module):
        self.module = module

    def __enter__(self):
        self.was = self.module.training
        self.module.training = False
        return self.module

    def __exit__(self, *exc):
        self.module.training = self.was


class PhiloxStream:
    """Counter-based RNG stream: (seed, running counter).  Every draw reserves its own counter range, so a run is
    reproducible from (seed) alone and ranks use disjoint seeds."""

    def __init__(self, seed):
        self.seed = int(seed) & ((1 << 64) - 1)
        self.counter = 0

    def _take(self, n):
        off = self.counter
        self.counter += (n + 3) // 4
        return off

    def state_dict(self):
        return {"seed": self.seed, "counter": self.counter}

    def load_state_dict(self, sd):
        """The counter of a saved stream; the seed is how the stream was built (flags, rank) and has to agree."""
        if int(sd["seed"]) != self.seed:
            raise ValueError(f"saved Philox stream has seed {int(sd['seed'])}, this one {self.seed}: the run was built with another --seed "
                             f"(or on another rank)")
        self.counter = int(sd["counter"])

    def normal(self, shape, device):
        n = int(np.prod(shape))
        return ops.rng_normal(tuple(shape), self.seed, self._take(n), device)

    def uniform(self, shape, device):
        n = int(np.prod(shape))
        return ops.rng_uniform(tuple(shape), self.seed, self._take(n), device)


def _unwrap(net):
    kw = {}
    while isinstance(net, partial):
        kw = {**net.keywords, **kw}
        net = net.func
    if hasattr(net, "__self__"):       # bound method (e.g. module.forward)
        net = net.__self__
    return net, kw.get("guide"), kw.get("cond_w")


def resolve_guidance(*, sample_cond_w, net_cond_w, kw_cond_w, has_teacher, sampler):
    """Guidance-weight policy of `GaussianDiffusion.sample` (gaussian_diffusion.py:246-257,271-278) as a pure function.
    net_cond_w: the per-sample draw 4*U[0,1) made when the caller passed `cond_w` (else None); kw_cond_w: a `cond_w=` keyword the
    caller's partial already carried.  -> (student_w, guidance_w, use_teacher):
      student_w    conditions the network through `cond_w_embed`
      guidance_w   classifier-free guidance weight (None: one unguided forward per step)
      use_teacher  evaluate the frozen teacher instead of `net` (sampler='teacher_test')
    No teacher: guidance_w = sample_cond_w unless that is -1.0 (then the draw, which is None when the caller did not ask) —
    so `--sample_cond_w 2.0` also guides `evaluate()`, which passes no cond_w (:257).  With a teacher the student is
    conditioned on the draw and never guided (:252-255); 'teacher_test' runs the teacher, guided by the weight the student
    would have been conditioned on (:271-278: `net.keywords['cond_w']`), unguided when there is none."""
    fixed = sample_cond_w is not None and float(sample_cond_w) != -1.0
    if has_teacher:
        student_w, guidance_w = net_cond_w, None
    else:
        student_w, guidance_w = kw_cond_w, (sample_cond_w if fixed else net_cond_w)
    if sampler == "teacher_test":
        if not has_teacher:
            raise ValueError("sampler='teacher_test' needs a teacher_net")
        return None, student_w, True
    return student_w, guidance_w, False


class _LossBridge(torch.autograd.Function):
    """A `LOSS_TABLE` row's wrapper under torch.autograd: -> the row's per-image outputs without its gradients, `loss` first and differentiable
    w.r.t. v (and nu where the row has dnu), the others reported numbers only.  tensors: the wrapper's tensor arguments, v (then nu) leading."""

    @staticmethod
    def forward(ctx, row, kw, *tensors):
        lead = len(row.grads)               # the differentiable inputs: one per gradient
        vals = getattr(ops, row.op)(*(t.contiguous() for t in tensors[:lead]), *tensors[lead:], grad_scale=1.0, **kw)
        outs = dict(zip(row.outs, vals))
        ctx.save_for_backward(*(outs.pop(name) for name in row.grads))
        ctx.constants = len(tensors) - lead
        loss, *reported = outs.values()
        ctx.mark_non_differentiable(*reported)
        return (loss, *reported)

    @staticmethod
    def backward(ctx, g, *_):
        g = g.contiguous().float()
        grads = tuple(ops.scale_rows(d.view(d.shape[0], -1), g).view_as(d) for d in ctx.saved_tensors)
        return (None, None) + grads + (None,) * ctx.constants


class GaussianDiffusion:
    def __init__(self, *, mean_type, num_steps, teacher_net=None, teacher_mode=None, sampler="ddim", sample_cond_w=None,
                 seed=0, dyn_threshold=0.0, loss_weight="snr_trunc", loss_gamma=5.0, time_sampler="uniform", time_importance=0,
                 importance_decay=0.9, importance_warmup=5, importance_floor=0.01, loss_profile=0, schedule=None, sample_schedule=None,
                 target_net=None, consistency_grid=0, consistency_loss="l2", consistency_huber_c=0.00054, guidance_interval=None, cfg_rescale=0.0,
                 posterior_var="large", ddim_eta=0.0, learn_var=0, vlb_lambda=VLB_LAMBDA, vlb_steps=VLB_STEPS):
        if mean_type not in ops.MEAN_TYPES:                     # :70-71
            raise NotImplementedError(mean_type)
        # a learned reverse-process variance (`learned_var_check`; Nichol & Dhariwal 2021, section 3.1; an extension, off by default: the same
        # launches as ever): the network's second head gives nu, training adds vlb_lambda times the bound term of the time pair
        # (u, max(u - 1 / vlb_steps, 0)) to the simple loss (gmk_hybrid_loss), and sampler 'ancestral' with posterior_var 'learned' draws with it
        self.learn_var, self.vlb_lambda, self.vlb_steps = learned_var_check(learn_var, vlb_lambda, vlb_steps, teacher_net is not None, loss_weight)
        # the stochastic samplers' options (`stochastic_check`; off by default: the same launches as ever): `posterior_var`, the variance of
        # sampler 'ancestral' (the reference's x_logvar, diffusion_utils.py:44-61), and `ddim_eta`, the noise share of sampler 'ddim'
        _, self.posterior_var, self.ddim_eta = stochastic_check(sampler, posterior_var, ddim_eta, self.learn_var)
        # the noise schedule (`Schedule`; the reference's registry, diffusion_utils.py:228-239, of which it picks 'cosine', -20, 20 at :33-34):
        # `schedule` maps the training times to log-SNRs (q_sample, the distillation targets, the loss profile's bin edges), `sample_schedule`
        # is the curve every sampler, edit, restore and the ODE walk (None: the training one) - the network is conditioned on the log-SNR
        # itself, so the two may differ.  None is that pick through the entries that hold it as constants: the same launches as ever.
        for name, s in (("schedule", schedule), ("sample_schedule", sample_schedule)):
            if s is not None and not isinstance(s, Schedule):
                raise ValueError(f"{name} = {s!r}: None or a Schedule")
            if s is not None:
                schedule_check(s.kind, s.logsnr_min, s.logsnr_max, s.shift)
        self.schedule = schedule
        self.sample_schedule = schedule if sample_schedule is None else sample_schedule
        # dynamic thresholding of the samplers' x-hat (Saharia et al. 2022, section 2.3; an extension, no reference call site): 0 is off (the
        # reference's static clip, the same launches as ever), else each image's x-hat is the unclipped (guided) prediction clamped to its own
        # p-th percentile s of |x| (s >= 1) and divided by s.  sample() and inpaint() only: the ODE is unclipped by definition and the
        # training loss keeps the reference's clip.
        self.dyn_threshold = dyn_threshold_check(dyn_threshold)
        # the guided samplers' two options (`guidance_check`; extensions, no reference call site, off by default: the same launches as ever).
        # `guidance_interval` (Kynkaanniemi et al. 2024): a step whose network time lies outside (lo, hi) evaluates the B-image conditional batch
        # alone and updates without guidance - one forward of B images instead of 2 B.  `cfg_rescale` = phi (Lin et al. 2023, section 3.4): on
        # the guided steps x-hat is clip(f x_raw, -1, 1), f = 1 + phi (std(x_c) / std(x_raw) - 1) per image, through gmk_cfg_rescale and the
        # thresholded update kernels.
        self.guidance_interval, self.cfg_rescale = guidance_check(guidance_interval, cfg_rescale, sampler, self.dyn_threshold)
        self.mean_type = mean_type
        self.num_steps = num_steps
        self.teacher_net = teacher_net
        self.sampler = sampler
        self.sample_cond_w = sample_cond_w
        # the training objective (extensions beside the reference's 'snr_trunc', all off by default): the loss weighting, Min-SNR's gamma and
        # how a batch's times are drawn (`loss_weight_check`); `loss_weight` is the caller's choice, `loss_weight_type` what a step applies
        self.loss_weight, self.loss_gamma, self.time_sampler = loss_weight_check(loss_weight, loss_gamma, time_sampler, teacher_net is not None)
        self.loss_weight_type = self.loss_weight
        # consistency distillation (`consistency_check`; an extension): a third teacher mode beside the reference's two.  `target_net` is the
        # method's target network (the weight average; None: the student itself under stop-gradient), `train_grid` the N of its time grid
        self.consistency, grid, self.consistency_loss, self.consistency_huber_c = consistency_check(
            teacher_mode, teacher_net is not None, consistency_grid, consistency_loss, consistency_huber_c)
        self.target_net = target_net if self.consistency else None
        self.train_grid = grid if grid > 0 else num_steps
        if self.teacher_net is not None:                      # :39-43
            assert teacher_mode in TEACHER_MODES
            self.teacher_mode = teacher_mode
            if self.teacher_mode == "step1":
                self.loss_weight_type = "snr"
            if self.consistency and self.consistency_loss == "huber":
                self.loss_weight_type = "huber"
        # the loss profile (extensions, off by default; `time_importance_check`): with either flag the fused train pass keeps `time_profile`, the
        # fp32 [5, 64] device state of gmk_loss_profile over its own (u, loss_b, x_mse), and with `time_importance` it draws its times from it
        # (gmk_u_importance); with `loss_profile` the test pass (`training_losses`) sums into a state of its own.  Allocated on first use, zeros.
        self.time_importance, self.importance_decay, self.importance_warmup, self.importance_floor, self.loss_profile = time_importance_check(
            time_importance, importance_decay, importance_warmup, importance_floor, loss_profile, teacher_net is not None)
        self.time_profile = None
        self._test_profile = None
        self.rng = PhiloxStream(seed)
        self._graphs = {}                   # small-batch sampling: one captured U-Net forward per (net, shape, conditioning kind)

    # ---- small-batch sampling: the forward as a replayed HIP graph ------------------------------------------------------------
    # The reference's own use of the sampler is small: `evaluate` draws 25 images (diffusion_model.py:98-104), `eval_heavy` the test batch
    # size.  Since round 4's dispatch changes a 25-image forward is 0.93 ms of kernels behind 1.1 ms of host launch work (~ 85 launches through
    # ctypes): the host is the bound, and replaying the captured forward removes it.  (Round 3 had measured a graph at 1.34 = 1.34 ms and
    # dropped it - the kernels, then 30 % longer, were the bound.)  Same kernels in the same order: bit-identical images.
    GRAPH_MAX_PIXELS = int(os.environ.get("GMK_SAMPLER_GRAPH_PIXELS", str(64 * 1024)))       # images x H x W of one forward; 0 turns it off
    SAMPLER_STREAMS = int(os.environ.get("GMK_SAMPLER_STREAMS", "2"))            # 1: every batch on one stream (A/B switch)
    STREAM_MIN_PIXELS = 1 << 18                                                  # images x H x W of a half-batch

    def _graph_path(self, module, nb, H, W):
        """Does a forward of `nb` images of H x W replay a captured graph in the sampler loop?"""
        return 0 < nb * H * W <= self.GRAPH_MAX_PIXELS and self.num_steps >= 16 and not (module.training and module.dropout > 0.0)

    def _forward_runner(self, module, z, guide, student_w, nb_decide=None, want_nu=0):
        """want_nu: 0, or the number of leading rows whose variance output the forward also returns (run(z_t) -> (v, nu) then).
        -> (run(z_t) -> v, lvec): the forward of `module` on a [nb, C, H, W] batch conditioned on `guide` / `student_w`, and the fp32 [nb]
        log-SNR vector it reads (the caller fills it before the first step, the sampler-update kernel writes it afterwards).  nb_decide: the
        batch the captured-graph decision is taken for (a guidance interval runs a B and a 2B forward in one chain: both follow the larger)."""
        nb = z.shape[0]
        dev = z.device
        # (a captured forward would replay ONE dropout mask: training-mode dropout keeps the kernel-by-kernel path)
        small = self._graph_path(module, nb if nb_decide is None else nb_decide, z.shape[2], z.shape[3])
        if not small:
            lvecs = [torch.empty((nb,), device=dev), torch.empty((nb,), device=dev)]      # two buffers alternate (see `sample`)
            return None, lvecs
        # the host-side freshness check of the packed convolution weights runs at capture time only: do it here, before every replay loop
        # (the pack buffer keeps its address, so a re-pack is seen by the captured kernels)
        module.prepare_forward(dev)
        key = (id(module), module.flat_params.data_ptr(), module._pack_buf.data_ptr(), tuple(z.shape), guide is not None, student_w is not None, want_nu)
        ent = self._graphs.get(key)
        if ent is None:
            zs, ls = torch.empty_like(z), torch.zeros((nb,), device=dev)
            gs = guide.clone() if guide is not None else None
            ws = student_w.clone() if student_w is not None else None
            zs.copy_(z)
            side = torch.cuda.Stream(device=dev)                  # warm-up off the capture: weight packs, workspaces, allocator pools
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(2):
                    module.forward_hip(zs, ls, gs, ws, want_nu=want_nu)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                out = module.forward_hip(zs, ls, gs, ws, want_nu=want_nu)
            ent = self._graphs[key] = (graph, zs, ls, gs, ws, out)
            if len(self._graphs) > 8:                             # a handful of shapes at most: drop the oldest capture
                self._graphs.pop(next(iter(self._graphs)))
        graph, zs, ls, gs, ws, out = ent
        if gs is not None:
            gs.copy_(guide)
        if ws is not None:
            ws.copy_(student_w)

        def run(z_t):
            zs.copy_(z_t)
            graph.replay()
            return out
        return run, [ls, ls]

    # ---- training ----------------------------------------------------------------------------------------
    def _teacher_eval(self, z, logsnr, guide, cond_w_net, guided):
        """Teacher forward (no grad).  guided: also the unconditional evaluation, batched as one 2B forward (:176-177)."""
        t = self.teacher_net
        if not guided:
            return t.forward_hip(z, logsnr, guide, cond_w_net), None
        B = z.shape[0]
        v2 = t.forward_hip(torch.cat([z, z]), torch.cat([logsnr, logsnr]), torch.cat([guide, -torch.ones_like(guide)]), None)
        return v2[:B], v2[B:]

    def _target_eval(self, module, z, logsnr, guide, cond_w_net):
        """The target network's forward of consistency distillation (no grad, never with dropout): `target_net`, or without one the student
        `module` itself under stop-gradient - no ctx, and with dropout off its counter does not move, so the student's own pass sees nothing of it."""
        target = module if self.target_net is None else self.target_net
        with _EvalForward(target):
            return target.forward_hip(z, logsnr, guide, cond_w_net)

    def draw_u(self, B, dev):
        """The continuous times of one batch from self.rng, fp32 [B] in [0, 1): 'uniform' B independent draws (:94); 'stratified' ONE draw
        (one Philox counter) expanded to u0 + b / B mod 1 by gmk_u_stratified.  Every pass draws its times through `draw_eps_u`."""
        if self.time_sampler == "stratified":
            return ops.u_stratified(self.rng.uniform((1,), dev), B)
        return self.rng.uniform((B,), dev)

    def draw_eps_u(self, x, u=None, eps=None, want_u=True):
        """The first two draws of a step from self.rng, in the one order every pass and a resumed run share: eps where the caller gave none,
        then (want_u) u where the caller gave none, as aligned fp32.  `_prepare` draws here, and so does a pass that needs u before `_prepare`
        (the bound's time pair, the loss profile, the graphed step's static inputs) - `_prepare` then finds both given.  -> (u, eps)"""
        if eps is None:
            eps = self.rng.normal(x.shape, x.device)
        if want_u:
            if u is None:
                u = self.draw_u(x.shape[0], x.device)
            u = ops.aligned(u.float())
        return u, eps

    # ---- the loss profile and the loss-aware time sampler (extensions, no reference call site) --------------------------------------------
    def profile_state(self, split, dev):
        """The fp32 [5, 64] profile state of `split` ('train': `time_profile`, 'test') on `dev`, allocated as zeros on first use."""
        name = {"train": "time_profile", "test": "_test_profile"}[split]
        t = getattr(self, name)
        if t is None or t.device != torch.device(dev):
            t = torch.zeros((5, ops.PROFILE_BINS), device=dev) if t is None else t.to(dev)
            setattr(self, name, t)
        return t

    def profile(self, split, reset=False):
        """Host arrays of one split's profile (`profile_rows`: bin edges in u and log-SNR, weight, loss_mean, loss_rms, x_mse_mean), None when
        the split has no state yet; for 'train' under time_importance also p, the current sampling probability of each bin.  reset: zero the
        state after the read (the test pass: one evaluation per read).  Reads the device: not for the inside of a step."""
        name = {"train": "time_profile", "test": "_test_profile"}[split]
        t = getattr(self, name)
        if t is None:
            return None
        p = None
        if split == "train" and self.time_importance:
            p = ops.u_importance(t, torch.zeros((1,), device=t.device), self.importance_warmup, self.importance_floor, want_table=True)[2].cpu().numpy()
        rows = profile_rows(t.cpu().numpy(), p, self.schedule)
        if reset:
            t.zero_()
        return rows

    def _prepare(self, net, x, u, eps, i_times=None, cond_w=None):
        """Everything ahead of the student's forward pass: draws, q_sample and (distillation) the teacher's targets.
        -> (module, guide, student cond_w, z_t, logsnr, x_target, eps_target, loss_type)"""
        module, guide, _ = _unwrap(net)
        x = ops.aligned(x.float())
        B, dev = x.shape[0], x.device
        distill = self.teacher_net is not None
        discrete = distill and self.teacher_mode in ("step2", "consistency")      # :87-91 discrete time
        u, eps = self.draw_eps_u(x, u, eps, want_u=not discrete)                  # :83, :94 continuous time
        eps = ops.aligned(eps.float())
        # the discretisation of the discrete-time modes: `timesteps`, or consistency distillation's own grid
        T = self.train_grid if self.consistency else self.num_steps
        if discrete:
            if i_times is None:
                i_times = (self.rng.uniform((B,), dev) * T).long().clamp_(max=T - 1)
            i_times = ops.aligned(i_times.long())
            _, u = ops.logsnr_schedule(B, dev, i_times=i_times, num_steps=T, want_u=True, schedule=self.schedule)
        logsnr, z_t = ops.q_sample(x, eps, u, self.schedule)                      # :95-100
        if not distill:
            return module, guide, None, z_t, logsnr, x, eps, 1 if self.loss_weight_type == "snr" else 0
        if cond_w is None:
            cond_w = 4.0 * self.rng.uniform((B,), dev)                            # :107
        cond_w = ops.aligned(cond_w.float())
        with torch.no_grad():
            logsnr_s = ops.logsnr_schedule(B, dev, u=u, shift=1.0 / T, schedule=self.schedule)      # :118-119
            if self.teacher_mode == "step1":                                      # :121-126 one guided teacher step
                v, vu = self._teacher_eval(z_t, logsnr, guide, None, guided=True)
                _, x_target, eps_target = ops.ddim_step_vec(v, z_t, logsnr, logsnr_s, v_uncond=vu, cond_w=cond_w, mean_type=self.mean_type)
                loss_type = 1
            elif self.consistency:          # Song et al. 2023, Algorithm 2: one teacher step t -> s, then the target net at (z_s, s)
                v_t, _ = self._teacher_eval(z_t, logsnr, guide, cond_w, guided=False)
                z_s, x_pred_teacher, _ = ops.ddim_step_vec(v_t, z_t, logsnr, logsnr_s, mean_type=self.mean_type)
                v_tgt = self._target_eval(module, z_s, logsnr_s, guide, cond_w)
                x_target, eps_target = ops.consistency_target(v_tgt, z_s, x_pred_teacher, z_t, logsnr, logsnr_s, i_times, mean_type=self.mean_type)
                loss_type = 0
            else:                                                                 # :128-154 two w-conditioned teacher steps
                logsnr_mid = ops.logsnr_schedule(B, dev, u=u, shift=0.5 / self.num_steps, schedule=self.schedule)
                v1, _ = self._teacher_eval(z_t, logsnr, guide, cond_w, guided=False)
                z_mid, _, _ = ops.ddim_step_vec(v1, z_t, logsnr, logsnr_mid, mean_type=self.mean_type)
                v2, _ = self._teacher_eval(z_mid, logsnr_mid, guide, cond_w, guided=False)
                z_teacher, x_pred_teacher, _ = ops.ddim_step_vec(v2, z_mid, logsnr_mid, logsnr_s, mean_type=self.mean_type)
                x_target, eps_target = ops.distill_target(z_teacher, z_t, x_pred_teacher, logsnr, logsnr_s, i_times)
                loss_type = 0
        return module, guide, cond_w, z_t, logsnr, x_target, eps_target, loss_type

    def _logsnr_prev(self, u):
        """The log-SNR one step of the bound's grid earlier, schedule(max(u - 1 / vlb_steps, 0)): the clamp is made here because the schedule
        kernel does not clamp and the cosine curve is NaN below u = 0."""
        u_s = ops.aligned((u - 1.0 / self.vlb_steps).clamp_(min=0.0))
        return ops.logsnr_schedule(u.numel(), u.device, u=u_s, schedule=self.schedule)

    def _loss_row(self, module):
        """`loss_row(self)`, refused before the forward when the row needs a variance output that `module` does not have."""
        row = loss_row(self)
        if row.nu and not getattr(module, "learn_var", False):
            raise ValueError("learn_var = 1 with a network that has no variance head (SimpleUnet(learn_var=True))")
        return row

    def _loss(self, row, v, nu, z_t, x_t, eps_t, logsnr, u, loss_type, grad_scale):
        """The objective of `row` on the network's output, for both passes: grad_scale None is `training_losses` (through `_LossBridge` when
        autograd follows v), a number `train_forward_backward`'s.  -> the wrapper's outputs by the row's names"""
        tensors = (v,) + ((nu,) if row.nu else ()) + (z_t, x_t) + ((eps_t,) if row.eps else ()) + (logsnr,) + ((self._logsnr_prev(u),) if row.nu else ())
        kw = {name: loss_type if attr is None else getattr(self, attr) for name, attr in row.scalars}
        kw["mean_type"] = self.mean_type
        if grad_scale is None and torch.is_grad_enabled() and v.requires_grad:
            vals = _LossBridge.apply(row, kw, *tensors)
            return dict(zip((name for name in row.outs if name not in row.grads), vals))
        return dict(zip(row.outs, getattr(ops, row.op)(*tensors, grad_scale=grad_scale, **kw)))

    def training_losses(self, *, net, x, u=None, eps=None, i_times=None, cond_w=None):
        """Reference call shape (:81).  Differentiable through torch.autograd when grad mode is on.  learn_var: the hybrid loss, with `vlb`
        (the bound term, nats per dimension) and `var_frac` (the mean interpolation weight) beside it."""
        assert x.dtype in [torch.float32, torch.float64]
        if self.loss_profile or self.learn_var:                   # both need u after `_prepare`, which does not return it
            u, eps = self.draw_eps_u(x, u, eps)
        module, guide, w, z_t, logsnr, x_t, eps_t, loss_type = self._prepare(net, x, u, eps, i_times, cond_w)
        row = self._loss_row(module)
        pred = module(z_t, logsnr, guide=guide, cond_w=w, **({"want_nu": True} if row.nu else {}))
        v, nu = pred if row.nu else (pred, None)
        v_grad = row.op == "v_loss" and torch.is_grad_enabled() and v.requires_grad
        o = self._loss(row, v, nu, z_t, x_t, eps_t, logsnr, u, loss_type, None)
        if self.loss_profile:                                     # the batch into the test profile at decay 1 (plain sums)
            x_mse = None if v_grad else o["x_mse"]                # (kept as it was: under autograd the v-loss rows hand the profile no x_mse)
            ops.loss_profile(u, o["loss"].detach(), x_mse, self.profile_state("test", u.device), 1.0)
        if row.nu:
            return {"loss": o["loss"], "vlb": o["vlb"], "var_frac": o["var_frac"]}
        # the v-loss rows report the unweighted x_mse only under a weighting the caller chose: one number that compares runs across weightings
        if v_grad or (row.op == "v_loss" and self.loss_weight == "snr_trunc"):      # (kept as it was: under autograd they never report it)
            return {"loss": o["loss"]}
        return {"loss": o["loss"], "x_mse": o["x_mse"]}

    def train_forward_backward(self, *, net, x, grad_scale, u=None, eps=None, i_times=None, cond_w=None,
                               on_grads_ready=None, join_side_before_ready=True):
        """Fused training pass used by DiffusionModel.train_step: forward, loss, dL/dv and the explicit backward
        schedule, leaving d(grad_scale * sum_b loss_b)/d(theta) in `module.flat_grads`.  No autograd graph."""
        # the loss profile: only when this pass draws the times itself.  u0 is today's draw (same stream, same counters: eps, then u); with
        # time_importance it goes through the profile's inverse CDF, and every image's gradient and loss take the importance weight 1 / (64 p).
        profiled = (self.time_importance or self.loss_profile) and u is None
        time_w = None
        if self.learn_var or profiled:          # both need u after `_prepare` (the bound's time pair, the profile)
            u, eps = self.draw_eps_u(x, u, eps)
        if profiled and self.time_importance:
            u, time_w = ops.u_importance(self.profile_state("train", x.device), u, self.importance_warmup, self.importance_floor)
        module, guide, w, z_t, logsnr, x_t, eps_t, loss_type = self._prepare(net, x, u, eps, i_times, cond_w)
        row = self._loss_row(module)
        ctx = {}
        pred = module.forward_hip(z_t, logsnr, guide, w, ctx=ctx, **({"want_nu": True} if row.nu else {}))
        v, nu = pred if row.nu else (pred, None)
        o = self._loss(row, v, nu, z_t, x_t, eps_t, logsnr, u, loss_type, grad_scale)
        dv, dnu = o["dv"], o.get("dnu")
        if time_w is not None:                  # the importance weights scale every row of the output gradients
            dv = ops.scale_rows(dv.view(dv.shape[0], -1), time_w).view_as(dv)
            if dnu is not None:
                dnu = ops.scale_rows(dnu.view(dnu.shape[0], -1), time_w).view_as(dnu)
        module.backward_hip(ctx, dv, on_grads_ready=on_grads_ready, join_side_before_ready=join_side_before_ready, dnu=dnu)
        o["logsnr"] = logsnr
        out = {key: o[key] for key in TRAIN_KEYS if key in o}
        if profiled:                    # the UNWEIGHTED loss enters the profile: p must follow the loss itself, not the loss it reweighted
            ops.loss_profile(u, out["loss"], out["x_mse"], self.profile_state("train", u.device), self.importance_decay)
            out["u"] = u
            if time_w is not None:      # loss: the unbiased estimate of the uniform-time loss
                out.update(loss=time_w * out["loss"], loss_b=out["loss"], time_w=time_w)
        return out

    # ---- likelihood: the continuous-time variational bound (an extension, no reference call site) ------------------------------------------
    @staticmethod
    def _full_range(what, schedule):
        """`nll` and `ode_nll` integrate between the schedule's end points, which gmk_vlb_endpoints (and the ODE's standard-normal prior) hold
        as -20 and 20: any kind of schedule over exactly that range passes, another range or a shift raises."""
        if schedule is not None and not schedule.full_range:
            raise ValueError(f"{what}: the likelihood is integrated over logsnr in [{VLB_LOGSNR_MIN:g}, {VLB_LOGSNR_MAX:g}], this schedule has logsnr_min = "
                             f"{schedule.logsnr_min:g}, logsnr_max = {schedule.logsnr_max:g}, logsnr_shift = {schedule.shift:g}: leave them at "
                             f"{VLB_LOGSNR_MIN:g}, {VLB_LOGSNR_MAX:g}, 0 (a likelihood over another range is not implemented)")

    @torch.no_grad()
    def nll(self, *, net, x, num_samples, seed=0, delta=1.0 / 255):
        """Per-image variational bound on -log p(x) of Kingma et al. 2021 (VDM) for a schedule over [-20, 20] (any kind: the bound is an integral over
        the log-SNR; another logsnr_min / logsnr_max / logsnr_shift raises, `_full_range`), in nats per dimension.
        x [B, C, H, W], D = C H W, lambda = logsnr, alpha^2 = sigmoid(lambda), sigma^2 = sigmoid(-lambda), Delta = 40:
          diffusion  1/2 int_{-20}^{20} E_eps |eps - eps_hat(z_lambda, lambda)|^2 d lambda  (VDM eq. 17 with lambda as the variable), estimated with
                     K = num_samples stratified draws per image, lambda_{b,k} = 20 - Delta frac(u0_b + k / K): mean_k 1/2 Delta |eps_k - eps_hat_k|^2
          prior      sum_i KL(N(alpha_1 x_i, sigma_1^2) || N(0, 1)) at lambda = -20
          decoder    the discretised Gaussian at lambda = 20 with mean z_0 / alpha_0 and scale sigma_0 / alpha_0, bins of half-width `delta`
                     centred on the value (1/255 for [-1, 1] data, 1/2 for binarised {0, 1} data), outermost edges +-inf.
        eps_hat is the network's noise prediction UNCLIPPED ('v': sigma z + alpha out, 'eps': out, 'x': (z - alpha out) / sigma), not the clipped
        x-hat that training and the samplers use: clipping could only tighten the bound, and it would break its closed form for a known network.
        The draws come from a fresh PhiloxStream(seed) in the order u0 [B], eps_k for k = 0 ... K-1, eps_0, so repeated calls (two checkpoints,
        EMA against raw weights) share their random numbers.  The forward runs without dropout, whatever `module.training` is.
        -> dict of fp32 [B]: nlogp = (prior + decoder + diffusion) / D, se (the standard error of the diffusion estimate from the spread of
        the K draws - conservative under stratification; NaN for K = 1), diffusion, prior, decoder, all per dimension."""
        module, guide, kw_cond_w = _unwrap(net)
        if self.teacher_net is not None or kw_cond_w is not None:
            raise ValueError("nll: a distilled student is conditioned on cond_w; its variational bound is not defined")
        self._full_range("nll", self.schedule)
        K = int(num_samples)
        if K < 1:
            raise ValueError(f"nll: num_samples = {num_samples}, need at least 1")
        x = ops.aligned(x.float())
        B, dev = x.shape[0], x.device
        D = x.numel() // B
        Bp = (B + 3) // 4 * 4                      # rows of [K, Bp] buffers start 16-byte aligned
        rng = PhiloxStream(seed)
        u0 = rng.uniform((B,), dev)
        logsnr = torch.empty((K, Bp), device=dev)
        logsnr[:, :B] = stratified_logsnr(u0, K)
        acc = torch.zeros((K, Bp), device=dev)
        weight = torch.full((B,), 0.5 * (VLB_LOGSNR_MAX - VLB_LOGSNR_MIN), device=dev)
        with _EvalForward(module):
            for k in range(K):
                eps = rng.normal(x.shape, dev)
                lk = logsnr[k, :B]
                z = ops.q_sample_logsnr(x, eps, lk)
                out = module.forward_hip(z, lk, guide, None)
                ops.vlb_term(out, z, eps, lk, weight, acc[k, :B], mean_type=self.mean_type)
                ops.throttle()                     # at most two draws queued on the GPU (see ops.throttle)
        eps0 = rng.normal(x.shape, dev)
        prior, dec = ops.vlb_endpoints(x, eps0, delta)
        vals = acc[:, :B]
        diff = vals.mean(0)
        se = vals.std(0) / math.sqrt(K) if K > 1 else torch.full_like(diff, float("nan"))
        return {"nlogp": (prior + dec + diff) / D, "se": se / D, "diffusion": diff / D, "prior": prior / D, "decoder": dec / D}

    # ---- probability-flow ODE: encode, decode, exact likelihood (an extension, no reference call site) -----------------------------------
    # dz / d lambda = f(z, lambda) = 1/2 sigma^2 z - 1/2 sigma eps_hat(z, lambda) (Song et al. 2021, section 4.3 and App. D.2, in lambda = logsnr),
    # discretised on the samplers' grid lambda_i = lambda(i / N) by DDIM's update without the clip: z_j = alpha_j x_hat_i + sigma_j eps_hat_i
    # (j = i + 1 encoding, i - 1 decoding), x_hat / eps_hat the UNCLIPPED predictions of the net output at (z_i, lambda_i).
    def _ode_setup(self, what, net, x, num_steps):
        """The common opening of `encode`, `decode` and `ode_nll`: the checks, then -> (module, guide, N, lam, times) with lam the grid
        (`ode_logsnr_grid`) and times its fp32 [N + 1, B] device table: row i is the network time of evaluation i (rows start 16-byte aligned)."""
        module, guide, kw_cond_w = _unwrap(net)
        if self.teacher_net is not None or kw_cond_w is not None:
            raise ValueError(f"{what}: a distilled student is conditioned on cond_w (a guided ODE): its probability-flow ODE has no density")
        N = int(num_steps)
        if N < 1 or N != num_steps:
            raise ValueError(f"{what}: num_steps = {num_steps}, need an integer >= 1")
        if x.dim() != 4 or x.shape[0] == 0 or x.shape[1] != getattr(module, "in_channels", x.shape[1]):
            raise ValueError(f"{what}: x has shape {tuple(x.shape)}, expected [B, {getattr(module, 'in_channels', 'C')}, H, W] with B > 0")
        lam = ode_logsnr_grid(N, self.sample_schedule)
        B = x.shape[0]
        times = torch.tensor(lam, dtype=torch.float32)[:, None].expand(len(lam), (B + 3) // 4 * 4).contiguous().to(x.device)
        return module, guide, N, lam, times[:, :B]

    @torch.no_grad()
    def encode(self, *, net, x, num_steps):
        """DDIM inversion: the latent code z_N of x under the probability-flow ODE on N = num_steps steps.  z_0 = x, then N updates
        i = 0 ... N-1 (N forwards).  Deterministic: decode(encode(x)) -> x as N grows.  Runs without dropout.  -> z_N, fp32, x's shape."""
        module, guide, N, lam, times = self._ode_setup("encode", net, x, num_steps)
        z = x.float().clone(memory_format=torch.contiguous_format)
        with _EvalForward(module):
            for i in range(N):
                out = module.forward_hip(z, times[i], guide, None)
                ops.pf_ode_step(out, z, lam[i], lam[i + 1], mean_type=self.mean_type)
                ops.throttle()
        return z

    @torch.no_grad()
    def decode(self, *, net, z, num_steps):
        """The inverse of `encode`: from z at lambda_N = -20, N updates i = N ... 1 (N forwards); returns the x_hat of the last evaluation
        (at lambda_1), as the sampler does at its last step.  Runs without dropout.  -> fp32, z's shape."""
        module, guide, N, lam, times = self._ode_setup("decode", net, z, num_steps)
        z = z.float().clone(memory_format=torch.contiguous_format)
        x_hat = torch.empty_like(z)
        with _EvalForward(module):
            for i in range(N, 0, -1):
                out = module.forward_hip(z, times[i], guide, None)
                ops.pf_ode_step(out, z, lam[i], lam[i - 1] if i > 1 else None, mean_type=self.mean_type, x_out=x_hat if i == 1 else None)
                ops.throttle()
        return x_hat

    @staticmethod
    def ode_draw_counters(B, D, num_steps):
        """Philox counters of `ode_nll`'s draws from PhiloxStream(seed), in draw order: the dequantisation u [B, D] (gmk_rng_uniform's
        element order), then the probe of each evaluation i = 0 ... N (r = +1 where the uniform at its counters is >= 1/2, else -1).
        -> [u, r_0, ..., r_N]"""
        q = (B * D + 3) // 4
        return [k * q for k in range(int(num_steps) + 2)]

    @torch.no_grad()
    def ode_nll(self, *, net, x, num_steps, seed=0, delta=1.0 / 255):
        """Per-image negative log-likelihood of the probability-flow ODE model (the deterministic model the samplers draw from), in nats per
        dimension, by the instantaneous change of variables with one Rademacher (Hutchinson) probe per evaluation.  x [B, C, H, W], D = C H W:
          y = x + u, u ~ U(-delta, delta)^D (dequantisation: 1/255 for [-1, 1] data, 1/2 for binarised data)
          z_0 = y, z_{i+1} = the ODE update, N = num_steps;  d_i = 1/2 sigma_i^2 D - 1/2 sigma_i (c_z D + c_o r_i . g_i), g_i = (d out / d z)^T r_i
          log p(y) = log N(z_N; 0, I) - sum_{i<N} 1/2 (lambda_i - lambda_{i+1}) (d_i + d_{i+1})
        N + 1 evaluations (a forward, an input VJP and one gmk_pf_ode_step each).  Draws: a fresh PhiloxStream(seed), u then one probe per
        evaluation (ode_draw_counters).  Runs without dropout.
        -> dict of fp32 [B]: nlogp = -log p(y) / D - log(2 delta) (by Jensen an upper bound on -log P(x's bin) / D, up to the estimator's
        noise), prior = -log N(z_N; 0, I) / D, divergence = the trapezoid sum / D."""
        self._full_range("ode_nll", self.sample_schedule)
        module, guide, N, lam, times = self._ode_setup("ode_nll", net, x, num_steps)
        delta = float(delta)
        if not 0.0 < delta <= 0.5:
            raise ValueError(f"ode_nll: delta = {delta}, the bin half-width must lie in (0, 0.5]")
        x = ops.aligned(x.float())
        B, dev = x.shape[0], x.device
        D = x.numel() // B
        rng = PhiloxStream(seed)
        z = ops.dequantize(x, delta, rng.seed, rng._take(B * D))
        wts = ode_trapezoid_weights(lam)
        acc = torch.zeros((B,), device=dev)
        prior = torch.empty((B,), device=dev)
        with _EvalForward(module):
            for i in range(N + 1):
                store = {}
                out = module.forward_hip(z, times[i], guide, None, ctx=store)
                r = ops.rng_rademacher(tuple(z.shape), rng.seed, rng._take(B * D), dev)
                g = module.input_vjp_hip(store, r)
                a, b = ode_divergence_coefs(lam[i], D, self.mean_type)
                last = i == N
                ops.pf_ode_step(out, z, lam[i], None if last else lam[i + 1], mean_type=self.mean_type, r=r, g=g, acc=acc,
                                div_a=wts[i] * a, div_b=wts[i] * b, prior=prior if last else None)
                ops.throttle()
        return {"nlogp": (prior + acc) / D - math.log(2.0 * delta), "prior": prior / D, "divergence": acc / D}

    # ---- sampling ----------------------------------------------------------------------------------------
    @torch.no_grad()
    def sample(self, *, net, init_x, cond_w=None, record=True, noises=None, net_cond_w=None, start=None):
        """:245-296.  Returns (all_zs, all_xs, all_eps) stacked [T, B, C, H, W] like the reference when `record`;
        with record=False only the final z is produced and returned as a 1-tuple-compatible triple
        (z[None], None, None) — the 3*T*B*C*H*W*4-byte trajectory is the dominant cost at large T*B otherwise.
        `noises` ([T, ...], indexed by step i) / `net_cond_w` inject the random draws (tests).
        start = k (an extension; `sampler_start`): the chain begins part-way - init_x is z at logsnr(k / T), the iterations i = k-1 ... 0 run
        and a recorded trajectory has k rows; None is the reference's chain from the prior end."""
        return self._sample(net=net, init_x=init_x, cond_w=cond_w, record=record, noises=noises, net_cond_w=net_cond_w, start=start)

    # ---- inpainting (RePaint, Lugmayr et al. 2022, Algorithm 1; an extension, no reference call site) -------------------------------------
    @torch.no_grad()
    def inpaint(self, *, net, x0, mask, init_x, cond_w=None, resample=1, seed=0, record=False, start=None):
        """Fill in the unknown part of x0 with this sampler: after every step t -> s the known pixels (mask 1) of z are replaced by a fresh noisy
        copy alpha_s x0 + sigma_s eps of x0 (by x0 itself at the last step), the others keep the sampler's value.  With resample = r > 1 every
        step except the last runs r network evaluations, each but the final one followed by a jump back to time t through q(z_t | z_s) (jump
        length 1), so a call costs T r - (r - 1) forwards.  mask: bool / uint8 / float with values in {0, 1}, broadcastable to x0's shape
        ([B, C, H, W]); x0: init_x's shape.  Samplers 'ddim', 'noisy', 'teacher_test' take any r >= 1; 'dpmpp_2m' only r = 1 (its x-hat
        history has no meaning across a jump back).  `net` / `cond_w` (guidance) as in `sample`, and so is the noise of 'noisy' (one draw from
        self.rng per network evaluation).  The known-region noise comes from a PhiloxStream(seed) of its own, advanced by 2 B n values per
        merge, so calls with the same seed see the same numbers.  start: as in `sample` (init_x is then z at logsnr(k / T)).  -> sample()'s
        triple; with `record` the (z, x_hat, eps_hat) of the last pass of each step, [T, B, C, H, W] each."""
        r = resample
        if isinstance(r, bool) or int(r) != r or r < 1:
            raise ValueError(f"inpaint: resample = {resample}, need an integer >= 1")
        r = int(r)
        sampler_compat_check(sampler_caps(self.sampler, self.ddim_eta), inpaint=r)
        shape = tuple(init_x.shape)
        if tuple(x0.shape) != shape:
            raise ValueError(f"inpaint: x0 shape {tuple(x0.shape)} differs from init_x shape {shape}")
        m = self._inpaint_known(mask, shape, init_x.device)
        inp = InpaintState(ops.aligned(x0.to(init_x.device).float()), m, PhiloxStream(seed), r, shape[0], [])
        return self._sample(net=net, init_x=init_x, cond_w=cond_w, record=record, inp=inp, start=start)

    # ---- restoration from a degraded observation (DDNM, Wang, Yu & Zhang 2023; an extension, no reference call site) -----------------------
    @torch.no_grad()
    def restore(self, *, net, obs, factor=1, gray=False, init_x, cond_w=None, record=False):
        """Sample an image that agrees with the observation obs = A x, A the box mean over factor x factor pixels (super-resolution) and, with
        gray, over the C channels (colourisation): at every step the data prediction x-hat is replaced by x-hat + A+(obs - A x-hat) (DDNM, eq.
        13-14: the observation fixes the range-space part, the network fills in the null-space part), so the result r satisfies A r = obs up to
        fp32 rounding.  obs: fp32 [B, C / cf, H / factor, W / factor] (cf = C with gray, else 1; `ops.box_mean` makes one); init_x: [B, C, H, W]
        noise.  Two extra launches per network evaluation: gmk_box_residual, then the *_ns update.  Samplers 'ddim', 'noisy', 'dpmpp_2m'; `net`
        / `cond_w` (guidance) and the noise of 'noisy' as in `sample`.  Out of scope, and a ValueError: noisy observations (DDNM+), time
        travel, and restoration together with dynamic thresholding or inpainting.  -> sample()'s triple."""
        sampler_compat_check(sampler_caps(self.sampler, self.ddim_eta), restore=True, dyn_threshold=self.dyn_threshold)
        shape = tuple(init_x.shape)
        cf, N, low = restore_operator(shape, factor, gray)
        if not isinstance(obs, torch.Tensor) or tuple(obs.shape) != low:
            raise ValueError(f"restore: obs shape {tuple(obs.shape) if isinstance(obs, torch.Tensor) else type(obs).__name__}, expected {low} for "
                             f"init_x {shape}, factor = {N}, gray = {bool(gray)}")
        rst = RestoreState(ops.aligned(obs.to(init_x.device).float().contiguous()), cf, N)
        return self._sample(net=net, init_x=init_x, cond_w=cond_w, record=record, rst=rst)

    # ---- sampling from a noisy or blurred observation (DPS, Chung et al. 2023, Algorithm 1; an extension, no reference call site) ----------
    @torch.no_grad()
    def posterior_sample(self, *, net, obs, op, init_x, zeta, record=False, noises=None):
        """Sample an image whose measurement agrees with obs = A x + noise, A the linear `MeasurementOp` op (`measurement_op`: box means,
        `restore`'s observation format, or a Gaussian blur), by diffusion posterior sampling: every step t -> s runs the sampler's own update
        (its clipped x-hat, as in `sample`) and then moves z_s along the gradient of the measurement error of the UNCLIPPED, unguided
        prediction x-hat(z_t) = c_z z_t + c_o out:
            e = obs - A x-hat, u = A^T e, g = (d out / d z)^T u;  z_s += 2 zeta / max(|e_b|, FLT_MIN) (c_z u + c_o g)
        - the paper's x' - zeta_i grad |y - A x-hat|^2 with zeta_i = zeta / |y - A x-hat| - at every step, the last one included.  Per step:
        a forward that keeps its activations, gmk_dps_backproject, the network's input VJP, the update, gmk_dps_correct; one stream, kernel
        by kernel, without dropout.  zeta >= 0 is the step size (untuned; 0 gives `sample`'s bits).  Samplers 'ddim' (also with ddim_eta > 0),
        'noisy' and 'ancestral'; labels (`net` carrying guide=) are allowed, the noise of the stochastic samplers comes from self.rng as in
        `sample` (`noises`: injected, 'noisy' only).  A ValueError: any other sampler, classifier-free guidance, dyn_threshold, cfg_rescale, a
        learned variance, a distilled student, mean_type 'eps'.  -> sample()'s triple (with `record` the z after each step's correction and
        the update's clipped x-hat / eps-hat)."""
        module, guide, kw_cond_w = _unwrap(net)
        fixed_w = self.sample_cond_w is not None and float(self.sample_cond_w) != -1.0
        dps_check(sampler=self.sampler, ddim_eta=self.ddim_eta, mean_type=self.mean_type, cond_w=fixed_w or kw_cond_w is not None,
                  dyn_threshold=self.dyn_threshold, cfg_rescale=self.cfg_rescale, learned_var=self.posterior_var == "learned",
                  student=self.teacher_net is not None)
        zeta = dps_zeta_check(zeta)
        if not isinstance(op, MeasurementOp):
            raise ValueError(f"posterior_sample: op = {op!r}, expected a MeasurementOp (measurement_op)")
        shape = tuple(init_x.shape)
        if len(shape) != 4 or 0 in shape:
            raise ValueError(f"posterior_sample: init_x shape {shape}, expected [B, C, H, W] with every dimension > 0")
        B, n1 = shape[0], math.prod(shape[1:])
        caps = sampler_caps(self.sampler, self.ddim_eta)
        sampler_compat_check(caps, noises=noises is not None, n1=n1)
        if n1 % 4:
            raise ValueError(f"posterior_sample: {n1} values per image, a multiple of 4 is required")
        low = ops.box_geometry(shape, op.cf, op.N)[-1] if op.kind == "box" else shape
        if not isinstance(obs, torch.Tensor) or tuple(obs.shape) != tuple(low):
            raise ValueError(f"posterior_sample: obs shape {tuple(obs.shape) if isinstance(obs, torch.Tensor) else type(obs).__name__}, "
                             f"expected {tuple(low)} for init_x {shape} and the {op.kind} operator")
        dev = init_x.device
        obs = ops.aligned(obs.to(dev).float().contiguous())
        plan = sampler_plan(self.num_steps, self.sampler, None, None, self.sample_schedule, self.posterior_var, self.ddim_eta, False)
        z_t = ops.aligned(init_x.float())
        # the network's time vector, as in the sampler loop: two buffers alternate, the update kernel fills the next step's
        lvecs = [torch.full((B,), float(plan[0].lt), device=dev), torch.empty((B,), device=dev)]
        seed = self.rng.seed
        zs, xs, es = [], [], []
        with _EvalForward(module):
            for f, s in enumerate(plan):
                off = self.rng._take(B * n1) if caps.noise and noises is None else None
                store = {}
                out = module.forward_hip(z_t, lvecs[f & 1], guide, None, ctx=store)
                u, enorm2 = ops.dps_backproject(out, z_t, obs, s.lt, op, mean_type=self.mean_type)
                g = module.input_vjp_hip(store, u)
                kw = dict(want_pred=record, mean_type=self.mean_type, logsnr_next=lvecs[(f + 1) & 1])
                if caps.update == "sampler_step":
                    noise = None
                    if caps.noise == "arg":
                        noise = ops.aligned(noises[s.i]) if noises is not None else ops.rng_normal(shape, seed, off, dev)
                    z_s, xp, ep = ops.sampler_step(out, z_t, s.lt, s.ls, s.is_last, noise=noise, **kw)
                else:
                    z_s, xp, ep = ops.stochastic_step(out, z_t, s.lt, s.ls, s.sto.coef_z, s.sto.coef_x, s.sto.coef_noise, s.sto.coef_prev,
                                                      s.is_last, seed, off, **kw)
                c_z, c_o = dps_coefs(s.lt, self.mean_type)
                z_t = ops.dps_correct(z_s, u, g, enorm2, c_z, c_o, zeta)
                if record:
                    zs.append(z_t); xs.append(xp); es.append(ep)
                ops.throttle()
        return (torch.stack(zs), torch.stack(xs), torch.stack(es)) if record else (z_t[None], None, None)

    def _inpaint_known(self, mask, shape, device):
        """The shape rules of the inpainting loop ([B, ...], a multiple of 4 values per image), then the mask -> uint8 [B, n] (`_inpaint_mask`)."""
        if len(shape) < 2 or 0 in shape:
            raise ValueError(f"inpaint: bad shape {shape}, expected [B, ...] with B and every image dimension > 0")
        n1 = math.prod(shape[1:])
        if n1 % 4:
            raise ValueError(f"inpaint: {n1} values per image, a multiple of 4 is required")
        return self._inpaint_mask(mask, shape, device)

    @staticmethod
    def _inpaint_mask(mask, shape, device):
        """bool / integer / float mask with values in {0, 1}, broadcastable to `shape` -> uint8 [B, n] on `device` (1 = known)."""
        if not isinstance(mask, torch.Tensor):
            raise ValueError(f"inpaint: mask must be a tensor, got {type(mask).__name__}")
        try:
            ok = tuple(torch.broadcast_shapes(tuple(mask.shape), shape)) == shape
        except RuntimeError:
            ok = False
        if not ok:
            raise ValueError(f"inpaint: mask shape {tuple(mask.shape)} does not broadcast to {shape}")
        if mask.dtype != torch.bool:
            if mask.is_complex() or not bool(((mask == 0) | (mask == 1)).all()):
                raise ValueError("inpaint: mask values must be 0 or 1")
        m = mask.to(device=device).to(torch.uint8).expand(shape).reshape(shape[0], -1)
        return ops.aligned(m.contiguous())

    # ---- editing a given image (SDEdit, Meng et al. 2022; an extension, no reference call site) ----------------------------------------------
    @torch.no_grad()
    def edit(self, *, net, x, start, cond_w=None, mask=None, seed=0, record=False):
        """Noise x ([B, C, H, W]) up to the intermediate time of `start` = k (1 <= k <= T; `edit_start` turns a strength into it) and denoise
        it from there with this sampler: z_k = alpha_k x + sigma_k eps at logsnr(k / T), then the iterations i = k-1 ... 0 of `sample`
        (k forwards instead of T).  rng = PhiloxStream(seed); eps is its first draw (B n values: ops.rng_normal(x.shape, seed, 0)).
        mask (optional; 1 = keep, `inpaint`'s rules): the loop also runs RePaint's merge with resample 1 against x itself, its draws following
        eps on the same stream (merge f at counter ceil(B n / 4) + f B n / 2), so the known pixels come back as x's own values.  `net`,
        `cond_w` (guidance) and the noise of 'noisy' (self.rng) as in `sample`; every sampler of `inpaint` at r = 1.  -> sample()'s triple;
        with `record` k rows."""
        k = sampler_start(start, self.num_steps)
        if start is None:
            raise ValueError("edit: start = None: give the step k to noise up to (edit_start(strength, num_steps))")
        shape = tuple(x.shape)
        dev = x.device
        m = None if mask is None else self._inpaint_known(mask, shape, dev)
        x = ops.aligned(x.float())
        rng = PhiloxStream(seed)
        eps = rng.normal(shape, dev)
        lt_k = _schedule_host(self.sample_schedule)(sampler_times(k - 1, self.num_steps)[0])      # the grid's logsnr_t of iteration k-1
        z_k = ops.q_sample_logsnr(x, eps, torch.full((shape[0],), float(lt_k), device=dev))
        inp = None if m is None else InpaintState(x, m, rng, 1, shape[0], [])
        return self._sample(net=net, init_x=z_k, cond_w=cond_w, record=record, inp=inp, start=k)

    # ---- interpolating between two images through their latent codes (Song et al. 2021, DDIM, section 5.3; an extension) -------------------
    INTERP_MAX_BATCH = 1024                 # images of one decode() call of `interpolate` (whole frames; one frame when B is larger)

    @torch.no_grad()
    def interpolate(self, *, net, xa, xb, frames, num_steps, return_latents=False):
        """K = frames images from xa to xb ([B, C, H, W] each): ONE `encode` of cat([xa, xb]) (the guide repeated), the spherical
        interpolation z_k = slerp(z_a, z_b, t_k) of the latent codes at t_k = k / (K - 1) (fp32; ops.slerp, one launch), and `decode` of the K B
        latents in chunks of whole frames of at most INTERP_MAX_BATCH images (the guide tiled).  (2 + K) num_steps forwards per pair.
        Deterministic, no guidance; checks as `encode` (a distilled student or a `cond_w` raises).
        -> fp32 [K, B, C, H, W]; with return_latents also the latents, [K, B, C, H, W]."""
        if tuple(xa.shape) != tuple(xb.shape):
            raise ValueError(f"interpolate: xa shape {tuple(xa.shape)} differs from xb shape {tuple(xb.shape)}")
        K = frames
        if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 2:
            raise ValueError(f"interpolate: frames = {frames!r}, need an integer >= 2")
        K = int(K)
        module, guide, N, _, _ = self._ode_setup("interpolate", net, xa, num_steps)
        B = xa.shape[0]
        if math.prod(xa.shape[1:]) % 4:
            raise ValueError(f"interpolate: {math.prod(xa.shape[1:])} values per image, a multiple of 4 is required")
        with_guide = lambda reps: module if guide is None else partial(module, guide=guide.repeat(reps))
        z = self.encode(net=with_guide(2), x=torch.cat([xa.float(), xb.float()]), num_steps=N)
        t = torch.tensor([k / (K - 1) for k in range(K)], dtype=torch.float32, device=z.device)
        lat = ops.slerp(z[:B], ops.aligned(z[B:]), t)
        per = max(1, self.INTERP_MAX_BATCH // B)         # frames per decode
        out = torch.cat([self.decode(net=with_guide(len(c)), z=c.reshape((-1,) + tuple(xa.shape[1:])), num_steps=N).view_as(c)
                         for c in lat.split(per)])
        return (out, lat) if return_latents else out

    def _sample(self, *, net, init_x, cond_w=None, record=True, noises=None, net_cond_w=None, inp=None, start=None, rst=None):
        """The loop behind `sample`, `inpaint`, `edit` and `restore` (inp: None, or the whole batch's InpaintState; start: `sampler_plan`'s; rst:
        None, or the whole batch's RestoreState)."""
        guidance_check(self.guidance_interval, self.cfg_rescale, self.sampler, self.dyn_threshold)      # the attributes may have been set since
        module, guide, kw_cond_w = _unwrap(net)
        B = init_x.shape[0]
        dev = init_x.device
        if self.sampler not in SAMPLER_CAPS:
            raise NotImplementedError(self.sampler)
        # (the attributes may have been set since; the variance head is the sampling network's own)
        stochastic_check(self.sampler, self.posterior_var, self.ddim_eta, getattr(module, "learn_var", False))
        caps = sampler_caps(self.sampler, self.ddim_eta)
        sampler_compat_check(caps, inpaint=0 if inp is None else inp.resample, restore=rst is not None, dyn_threshold=self.dyn_threshold,
                             cfg_rescale=self.cfg_rescale, noises=noises is not None, n1=int(np.prod(init_x.shape[1:])))
        if cond_w is not None and net_cond_w is None:
            net_cond_w = 4.0 * self.rng.uniform((B,), dev)           # :247-251
        student_w, w, use_teacher = resolve_guidance(sample_cond_w=self.sample_cond_w, net_cond_w=net_cond_w, kw_cond_w=kw_cond_w,
                                                     has_teacher=self.teacher_net is not None, sampler=self.sampler)
        if use_teacher:
            module = self.teacher_net
        as_vec = lambda t: (t.to(dev).float().expand(B).contiguous() if isinstance(t, torch.Tensor)
                            else torch.full((B,), float(t), device=dev))
        student_w = ops.aligned(as_vec(student_w)) if student_w is not None else None
        w = ops.aligned(as_vec(w)) if w is not None else None
        if w is not None and guide is None:
            raise ValueError("classifier-free guidance needs class labels (net must carry guide=)")
        plan = sampler_plan(self.num_steps, self.sampler, None if inp is None else inp.resample, start, self.sample_schedule,
                            self.posterior_var, self.ddim_eta, getattr(module, "learn_var", False))
        if w is not None and not any(guidance_mask(plan, self.guidance_interval)):
            w = None                            # no step of this chain lies inside the guidance interval: the conditional model alone
        z_all = ops.aligned(init_x.float())
        n1 = int(np.prod(init_x.shape[1:]))
        # Large batches run as TWO half-batches on two HIP streams (round 5): the chains of different samples never meet (GroupNorm is per
        # sample, the update is elementwise), and a persistent kernel's start-up and tail - about one tile time per launch, ~ 80 launches per
        # forward - then overlap with the other half's kernels: -2.4 ... -3.0 % per forward at the bench configurations (tools/two_stream_probe.py;
        # four quarters are slower than one batch), the same bits.  Small batches (the captured-graph path) and odd batches stay on one stream.
        # Never together with the captured-graph path (both halves would replay ONE graph on ONE set of static buffers, whatever
        # GMK_SAMPLER_GRAPH_PIXELS is set to), and only at hidden_size 128: the bit-identity of the halves rests on the embedding GEMMs' K-split
        # not depending on the row count, which `gemm_ksplit` guarantees for K <= 256 = 2 x 128 only.
        nb_half = (B // 2) * (2 if w is not None else 1)
        two = dev.type == "cuda" and self.SAMPLER_STREAMS >= 2 and B % 2 == 0 and ((B // 2) * n1) % 4 == 0 and (noises is None or isinstance(noises, torch.Tensor)) and \
            (B // 2) * init_x.shape[2] * init_x.shape[3] >= self.STREAM_MIN_PIXELS and module.channels == 128 and \
            not self._graph_path(module, nb_half, init_x.shape[2], init_x.shape[3])
        K = 2 if two else 1
        cut = lambda t, a, b_: None if t is None else ops.aligned(t[a:b_])
        # Philox counter of each network evaluation's noise draw for the WHOLE batch (ancestral sampler), and (inp.moffs) of each inpainting
        # merge's known-region draws: chunks take their slice of them
        offs = []
        cur = torch.cuda.current_stream() if dev.type == "cuda" else None
        streams = [cur] if K == 1 else self._chunk_streams(dev, K)
        gens = []
        for a, b_ in [(k * B // K, (k + 1) * B // K) for k in range(K)]:
            inp_k = None if inp is None else inp._replace(x0=cut(inp.x0, a, b_), mask=cut(inp.mask, a, b_))
            rst_k = None if rst is None else rst._replace(obs=cut(rst.obs, a, b_))
            gens.append(self._sample_chunk(plan, module, cut(guide, a, b_), cut(student_w, a, b_), cut(w, a, b_), cut(z_all, a, b_),
                                           noises if (noises is None or K == 1) else torch.as_tensor(noises)[:, a:b_], record, offs, a * n1 // 4, caps, inp_k, rst_k))
        if K > 1:
            # what a forward builds lazily after a weight update (packed weights, frequency tables) is enqueued HERE, on the stream both chunk
            # streams wait for: the first chunk's forward would otherwise re-pack on ITS stream and clear the host flag, and the second chunk's
            # convolutions would read the pack buffers without ever having waited for that kernel
            module.prepare_forward(dev)
            for st in streams:
                st.wait_stream(cur)

        def advance():
            if K == 1:
                return [next(gens[0])]
            outs = []
            for st, gen in zip(streams, gens):
                with torch.cuda.stream(st):
                    outs.append(next(gen))
            return outs
        for step in plan:
            for _ in range(step.passes):
                if caps.noise and noises is None:
                    offs.append(self.rng._take(B * n1))
                if inp is not None:
                    inp.moffs.append(inp.rng._take(2 * B * n1))     # eps1 and eps2 of one merge, used or not
            advance()
            if K > 1:                                   # the throttle's event has to cover both halves
                for st in streams:
                    cur.wait_stream(st)
            ops.throttle()                              # at most two sampler iterations queued on the GPU (see ops.throttle)
        res = advance()                                 # the chunks' results
        if K == 1:
            return res[0]
        for st in streams:
            cur.wait_stream(st)
        for r in res:
            for t in r:
                if t is not None:
                    t.record_stream(cur)
        return tuple(None if res[0][j] is None else torch.cat([r[j] for r in res], dim=1) for j in range(3))

    def _chunk_streams(self, dev, K):
        if getattr(self, "_streams", None) is None or len(self._streams) < K or self._streams[0].device != dev:
            self._streams = [torch.cuda.Stream(device=dev) for _ in range(K)]
        return self._streams[:K]

    def _sample_chunk(self, plan, module, guide, student_w, w, z_t, noises, record, offs, q0, caps, inp=None, rst=None):
        """The sampler loop over one (chunk of a) batch as a generator: one `next` per step of `plan` (everything it launches goes to the stream
        current at that call), then one more for the result.  offs[f] / q0: Philox counter of network evaluation `f`'s whole-batch noise draw /
        this chunk's offset in it; caps: `sampler_caps`' row.  inp: None, or the InpaintState with this chunk's rows of x0 and mask - inp.moffs[f]
        is the whole-batch Philox counter of evaluation f's merge.  rst: None, or the RestoreState with this chunk's rows of obs."""
        B = z_t.shape[0]
        zs, xs, es = [], [], []
        # the mode of every network evaluation: guided (the 2B-image batch) or not (the B-image batch with the caller's labels alone).  Without a
        # guidance interval all of them share the chain's mode, and one runner issues the launches it always has; with one, the steps whose
        # network time lies outside it are unguided (w = 0: the conditional model), a re-noising inpainting pass staying in its step's mode.
        mask = guidance_mask(plan, self.guidance_interval) if w is not None else [False] * len(plan)
        modes = [g for step, g in zip(plan, mask) for _ in range(step.passes)]
        nb_max = 2 * B if True in modes else B          # the captured-graph decision is taken for the larger of the two forwards
        # per mode: the forward's runner (small batches replay a captured forward: one static log-SNR buffer, safe by stream order; large ones
        # launch it kernel by kernel), its log-SNR buffers and its conditioning
        runners = {}
        # posterior_var 'learned': every forward also runs the variance head, over the conditional rows alone (the first B of a guided 2B batch)
        want_nu = B if self.posterior_var == "learned" and caps.update == "stochastic_step" else 0
        if False in modes:
            runners[False] = self._forward_runner(module, z_t, guide, student_w, nb_max, want_nu) + (guide, student_w)
        if True in modes:       # conditional + unconditional evaluations share one 2B-image forward (:176-177)
            guide2 = torch.cat([guide, -torch.ones_like(guide)])
            student_w2 = None if student_w is None else torch.cat([student_w, student_w])
            z2 = torch.cat([z_t, z_t])      # once: afterwards the update kernel writes both halves of the next 2B batch itself
            runners[True] = self._forward_runner(module, z2, guide2, student_w2, nb_max, want_nu) + (guide2, student_w2)
        # the network's time vector: filled once here, then by the update kernel (the next logsnr_t is this step's logsnr_s);
        # two buffers alternate so that a forward still queued on the GPU never sees its input overwritten
        runners[modes[0]][1][0].fill_(float(plan[0].lt))

        def evaluate(g, z_in, f):
            """Network evaluation f in mode g -> (v, vu, nu): the conditional output, guided the unconditional one (else None), and under
            posterior_var 'learned' the conditional rows' variance output (else None)."""
            graphed, lvecs, gd, sw = runners[g]
            out = graphed(z_in) if graphed else module.forward_hip(z_in, lvecs[f & 1], gd, sw, want_nu=want_nu)
            out, nu = out if want_nu else (out, None)
            return (out[:B], out[B:], nu) if g else (out, None, nu)
        # dpmpp_2m: the previous step's x-hat, [B, ...] also when guided (the kernel reads and rewrites it in place; the first step does not read it)
        x_hist = torch.empty_like(z_t) if caps.x_hist else None
        # the update, chosen once: the wrapper's own leading arguments (s: the step, f: the evaluation) and, where it has the form, thr / ns; the
        # keywords all five share come as `kw`, stated once at the call ('_lv': 'ancestral' under the learned variance, the 'small' row scaled per element)
        seed, name = self.rng.seed, caps.update + ("_lv" if want_nu else "")
        if name == "sampler_step":
            update = lambda s, f, v, z, nu, noise, thr, ns, kw: ops.sampler_step(v, z, s.lt, s.ls, s.is_last, noise=noise, thr=thr, ns=ns, **kw)
        elif name == "dpm_solver_step":
            update = lambda s, f, v, z, nu, noise, thr, ns, kw: ops.dpm_solver_step(
                v, z, x_hist, s.lt, s.ls, s.dpm.coef_z, s.dpm.coef_x, s.dpm.coef_prev, s.is_last, thr=thr, ns=ns, **kw)
        elif name == "consistency_step":
            update = lambda s, f, v, z, nu, noise, thr, ns, kw: ops.consistency_step(v, z, s.lt, s.ls, s.is_last, seed, offs[f], q0=q0, **kw)
        elif name == "stochastic_step":
            update = lambda s, f, v, z, nu, noise, thr, ns, kw: ops.stochastic_step(v, z, s.lt, s.ls,
                s.sto.coef_z, s.sto.coef_x, s.sto.coef_noise, s.sto.coef_prev, s.is_last, seed, offs[f], q0=q0, x_hist=x_hist, thr=thr, **kw)
        else:
            update = lambda s, f, v, z, nu, noise, thr, ns, kw: ops.stochastic_step_lv(v, z, nu, s.lt, s.ls,
                s.sto.coef_z, s.sto.coef_x, s.sto.coef_noise, learned_half_delta(s.lt, s.ls), s.is_last, seed, offs[f], q0=q0, thr=thr, **kw)
        f = 0                                   # network evaluations so far (one per step unless inpainting resamples)
        for step in plan:
            i, lt, ls, mrg = step.i, step.lt, step.ls, step.inp
            for p in range(step.passes):
                # this evaluation's mode and the next one's: every launch that writes the next batch and its time vector (the update, the
                # inpainting merge) does so in the form the NEXT evaluation needs - the duplicate and the 2B vector iff that one is guided
                g, g_next = modes[f], modes[min(f + 1, len(modes) - 1)]
                lnext = runners[g_next][1][(f + 1) & 1]
                v, vu, nu = evaluate(g, z2 if g else z_t, f)
                wg = w if g else None
                noise = None
                if caps.noise == "arg":                     # :241
                    noise = ops.aligned(noises[i]) if noises is not None else ops.rng_normal(tuple(z_t.shape), self.rng.seed, offs[f] + q0, z_t.device)
                # dynamic thresholding: one select launch per network evaluation (per image, so a half-batch gives the whole batch's bits)
                thr = ops.dyn_threshold(v, z_t, lt, self.dyn_threshold, v_uncond=vu, cond_w=wg, mean_type=self.mean_type) if self.dyn_threshold else None
                # the rescaled guided prediction: one reduction launch per guided evaluation (per image too); an unguided one has factor 1
                if self.cfg_rescale and g:
                    thr = ops.cfg_rescale(v, z_t, lt, self.cfg_rescale, vu, wg, mean_type=self.mean_type)
                # restoration: one residual launch per network evaluation (per image, so a half-batch gives the whole batch's bits)
                ns = None if rst is None else (ops.box_residual(v, z_t, rst.obs, lt, rst.cf, rst.N, v_uncond=vu, cond_w=wg, mean_type=self.mean_type),
                                               rst.cf, rst.N)
                z_t, xp, ep = update(step, f, v, z_t, nu, noise, thr, ns, dict(v_uncond=vu, cond_w=wg, want_pred=record, mean_type=self.mean_type,
                                                                               dup=g_next, logsnr_next=lnext))
                if g_next:
                    z_t, z2 = z_t
                if inp is not None:             # the known region, then (all passes but the step's last) the jump back to time t
                    ops.inpaint_merge(z_t, inp.x0, inp.mask, mrg.alpha_s, mrg.sigma_s, mrg.a, mrg.b, mrg.is_last, p < step.passes - 1, lt, ls, inp.rng.seed,
                                      inp.moffs[f], q0=q0, B_total=inp.B_total, z_dup=z2[B:] if g_next else None, logsnr_next=lnext)
                f += 1
            if record:
                zs.append(z_t); xs.append(xp); es.append(ep)
            yield None
        yield (torch.stack(zs), torch.stack(xs), torch.stack(es)) if record else (z_t[None], None, None)
