"""CPU tests (no GPU) of the steered optimiser step (DG.grad_clip, DG.skip_nonfinite, DG.lr_scheduler / lr_warmup / lr_decay_steps /
lr_min_ratio): the schedule against closed-form values, flag validation, the defaults, the C ABI entries and their argument checks."""
import ctypes
import math
import os
import sys
from pathlib import Path

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref  # noqa: E402


def _model_cls():
    from generative_models_amd import common
    return common.discover_models()["diffusion_model"]


def _model(**flags):
    from generative_models_amd import common
    Model = _model_cls()
    G = common.AttrDict(dict(Model.DG))
    G.update(hidden_size=32)
    G.update(flags)
    return Model(G)


def _adam(**kw):
    from generative_models_amd.diffusion.optim import FusedAdam
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    return FusedAdam(SimpleUnet(32), **kw)


@pytest.mark.parametrize("W", [1, 2, 500])
def test_warmup_closed_form(W):
    lr = 3e-4
    for sched in ({"lr_scheduler": "none"}, {"lr_scheduler": "cosine", "lr_decay_steps": 1000}):
        opt = _adam(lr=lr, lr_warmup=W, **sched)
        assert opt.lr_at(0) == pytest.approx(lr / W, rel=1e-15)
        assert opt.lr_at(W - 1) == lr
        if W > 2:
            assert opt.lr_at(W // 2 - 1) == pytest.approx(lr * (W // 2) / W, rel=1e-15)


@pytest.mark.parametrize("W", [0, 10])
@pytest.mark.parametrize("ratio", [0.0, 0.1, 1.0])
def test_cosine_closed_form(W, ratio):
    lr, D = 1e-3, 200
    opt = _adam(lr=lr, lr_scheduler="cosine", lr_warmup=W, lr_decay_steps=D, lr_min_ratio=ratio)
    assert opt.lr_at(W) == lr                                                  # the decay starts at lr ...
    assert opt.lr_at(W + D // 2) == pytest.approx(lr * (1 + ratio) / 2, rel=1e-14)      # ... passes the midpoint ...
    for t in (W + D, W + D + 1, W + 10 * D):
        assert opt.lr_at(t) == pytest.approx(ratio * lr, rel=1e-14, abs=1e-20)        # ... and stays at the floor
    seq = [opt.lr_at(t) for t in range(W, W + D + 1)]
    assert all(a >= b for a, b in zip(seq, seq[1:]))
    for t in (0, 3, W, W + 7, W + D // 3, W + 2 * D):
        assert opt.lr_at(t) == pytest.approx(clip_ref.lr_at(lr, t, "cosine", W, D, ratio), rel=1e-15)


def test_no_schedule_returns_lr_exactly():
    lr = 3e-4
    opt = _adam(lr=lr)
    assert not opt.scheduled and not opt.steered
    assert all(opt.lr_at(t) == lr for t in (0, 1, 7, 10 ** 3, 10 ** 6, 10 ** 9))


@pytest.mark.parametrize("bad", [dict(grad_clip=-1.0), dict(grad_clip=float("nan")), dict(lr_scheduler="linear"), dict(lr_min_ratio=-0.1),
                                 dict(lr_min_ratio=1.5), dict(lr_scheduler="cosine", lr_decay_steps=0), dict(lr_warmup=-1),
                                 dict(lr_scheduler="cosine", lr_decay_steps=-5)])
def test_bad_flags_raise(bad):
    with pytest.raises(ValueError):
        _model(**bad)
    with pytest.raises(ValueError):
        _adam(**bad)


def test_skip_nonfinite_flag_is_zero_or_one():
    with pytest.raises(ValueError):
        _model(skip_nonfinite=2)


def test_defaults_are_off_and_reference_keys_keep_their_defaults():
    M = _model_cls()
    ref_defaults = dict(binarize=0, timesteps=250, hidden_size=128, dropout=0.0, sampler="ddim", mean_type="v", eval_heavy=1, class_cond=1,
                        sample_cond_w=-1.0, cf_drop_prob=0.1, teacher_path=Path("."), teacher_mode="step1", lr_scheduler="none")
    for k, v in ref_defaults.items():
        assert M.DG[k] == v and type(M.DG[k]) is type(v), k
    new = dict(grad_clip=0.0, skip_nonfinite=0, lr_warmup=0, lr_decay_steps=0, lr_min_ratio=0.1)
    for k, v in new.items():
        assert M.DG[k] == v and type(M.DG[k]) is type(v), k
    opt = _model().optimizer
    assert not opt.steered and not opt.scheduled and opt.ctl_state is None
    assert opt.state_dict()["skipped"] == 0


def test_flags_reach_the_optimizer():
    opt = _model(grad_clip=0.5, lr_scheduler="cosine", lr_warmup=3, lr_decay_steps=9, lr_min_ratio=0.25, lr=1e-3).optimizer
    assert opt.steered and opt.scheduled and opt.grad_clip == 0.5 and not opt.skip_nonfinite
    assert opt.lr_at(3 + 9) == pytest.approx(0.25e-3, rel=1e-14)
    opt = _model(skip_nonfinite=1).optimizer
    assert opt.steered and not opt.scheduled and opt.grad_clip == 0.0 and opt.skip_nonfinite
    opt.load_state_dict({"step": 4, "m": None, "v": None, "lr": 1e-3, "skipped": 2})
    assert opt.state_dict()["skipped"] == 2 and opt.step_count == 4


def test_flags_parse_on_the_command_line():
    from generative_models_amd import main
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--grad_clip", "1.0", "--skip_nonfinite", "1", "--lr_scheduler", "cosine",
                                            "--lr_warmup", "2", "--lr_decay_steps", "3", "--lr_min_ratio", "0.2"])
    assert (G.grad_clip, G.skip_nonfinite, G.lr_scheduler, G.lr_warmup, G.lr_decay_steps, G.lr_min_ratio) == (1.0, 1, "cosine", 2, 3, 0.2)
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert (G.grad_clip, G.skip_nonfinite, G.lr_scheduler, G.lr_warmup, G.lr_decay_steps) == (0.0, 0, "none", 0, 0)


def test_header_declares_the_entries_and_the_binding_matches():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    ret, argtypes, argnames = protos["gmk_grad_norm"]
    assert argnames == ["g", "n", "grad_scale", "max_norm", "workspace", "workspace_bytes", "state", "stream"] and ret is ctypes.c_int
    assert argtypes == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                        ctypes.c_void_p]
    ret, argtypes, argnames = protos["gmk_adam_step_ctl"]
    assert argnames == ["p", "g", "m", "v", "ema", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "ema_w", "state", "stream"]
    assert protos["gmk_grad_norm_workspace_bytes"][0] is ctypes.c_int64
    # the two existing optimiser entries are unchanged
    assert protos["gmk_adam_step"][2] == ["p", "g", "m", "v", "n", "lr", "beta1", "beta2", "eps", "step", "grad_scale", "stream"]
    assert len(protos["gmk_adam_ema_step"][2]) == 14


@pytest.mark.parametrize("n", [1, 3, 1003, 8192, 8193, 6033665, 6038276, 10 ** 9])
def test_workspace_size_is_a_function_of_n_alone(n):
    """One float per workgroup; the count restated in clip_ref.  It must not follow the CU limit (data-parallel ranks change it)."""
    from generative_models_amd import _lib
    lib = _lib.lib
    want = 4 * clip_ref.norm_parts(n)
    before = lib.gmk_get_cu_limit()
    assert lib.gmk_grad_norm_workspace_bytes(n) == want
    assert lib.gmk_set_cu_limit(64) == 0
    try:
        assert lib.gmk_grad_norm_workspace_bytes(n) == want
    finally:
        assert lib.gmk_set_cu_limit(before) == 0
    assert lib.gmk_grad_norm_workspace_bytes(0) == 0


def test_entries_reject_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first
    assert lib.gmk_grad_norm(None, 8, 1.0, 1.0, buf, 4, buf, None) == -1
    assert lib.gmk_grad_norm(buf, 8, 1.0, 1.0, buf, 4, None, None) == -1
    assert lib.gmk_grad_norm(buf, 0, 1.0, 1.0, buf, 4, buf, None) == -1
    assert lib.gmk_grad_norm(buf, 8, float("nan"), 1.0, buf, 4, buf, None) == -1 and b"grad_scale" in lib.gmk_last_error()
    assert lib.gmk_grad_norm(buf, 8, 1.0, float("nan"), buf, 4, buf, None) == -1 and b"max_norm" in lib.gmk_last_error()
    assert lib.gmk_grad_norm(buf, 10 ** 6, 1.0, 1.0, buf, 8, buf, None) == -1 and b"workspace" in lib.gmk_last_error()
    args = lambda ema, w, state: (buf, buf, buf, buf, ema, 8, 1e-3, 0.9, 0.999, 1e-8, 1, 1.0, w, state, None)
    assert lib.gmk_adam_step_ctl(*args(None, 0.0, None)) == -1 and b"state" in lib.gmk_last_error()
    assert lib.gmk_adam_step_ctl(*args(buf, 1.5, buf)) == -1 and b"ema_w" in lib.gmk_last_error()


def test_reference_bound_and_formulas():
    """clip_ref's own pieces: the chain lengths behind the bound, and the coefficient on both sides of max_norm."""
    assert clip_ref.norm_parts(1003) == 1 and clip_ref.norm_parts(6033665) == 737
    assert clip_ref.norm_chain(1003) == 19 + 9 and clip_ref.norm_chain(6033665) == 19 + 11
    assert clip_ref.norm_rel_bound(6033665) == 31 * 2.0 ** -25
    assert clip_ref.clip_coef(0.5, 1.0) == 1.0 and clip_ref.clip_coef(4.0, 1.0) < 0.25 and clip_ref.clip_coef(4.0, 0.0) == 1.0
    assert float(clip_ref.clip_coef(4.0, 1.0)) == pytest.approx(1 / (4 + 1e-6), rel=1e-6)
    assert math.isclose(clip_ref.lr_at(1e-3, 0, "none", 4), 2.5e-4)
