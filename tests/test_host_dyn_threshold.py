"""CPU tests (no GPU) of dynamic thresholding (`GaussianDiffusion(dyn_threshold=p)`, gmk_dyn_threshold, gmk_sampler_step_dt,
gmk_dpm_solver_step_dt; an extension): the quantile rule of the restatement (tests/dyn_threshold_ref.py) against torch.quantile, the host's
rank arithmetic, option validation, the C ABI and its argument checks, and the restatement's anchor to the oracle's DDIM chain."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_threshold_ref as R  # noqa: E402

# the (n, p) grid of the GPU bit test (tests/test_gpu_dyn_threshold.py); KEYS is ops.DYN_THRESHOLD_KEYS
GPU_NS = lambda keys: (1, 2, 143, 256, 1027, 12288, keys + 3)
GPU_PS = (1e-3, 0.5, 0.995, 1.0)


@pytest.mark.parametrize("n", [1, 4, 5, 144, 12289])
@pytest.mark.parametrize("p", [0.5, 0.995, 1.0])
def test_quantile_rule_is_torch_quantile(n, p):
    g = torch.Generator().manual_seed(n)
    x = torch.randn((3, n), generator=g, dtype=torch.float64) * 1.7
    x[1] = torch.round(x[1] * 2) / 2                                  # ties
    x[2] = -0.75                                                      # an all-equal image
    want = torch.quantile(x.abs(), p, dim=1)
    got = R.quantile(x, p)
    assert float((got - want).abs().max()) <= 1e-12


def test_quantile_rule_on_ties():
    x = torch.tensor([[1, 1, 1, 2, 2, .5, .5, 3]], dtype=torch.float64)
    assert float(R.quantile(x, 0.6)) == pytest.approx(1.2, abs=1e-12)
    assert float(torch.quantile(x, 0.6)) == pytest.approx(1.2, abs=1e-12)
    q32, s32 = R.quantile_fp32(x.float(), 0.6)
    assert abs(float(q32[0]) - 1.2) <= 2 ** -22 and float(s32[0]) == float(q32[0])
    assert R.quantile_fp32(-x.float() * 0.25, 0.6)[1][0] == 1.0       # s = max(1, q); |.| of negative values


def test_rank_edge_cases():
    from generative_models_amd.diffusion.gaussian_diffusion import dyn_threshold_rank
    for n in (1, 2, 5, 3072, 12288):
        assert dyn_threshold_rank(1.0, n) == (n - 1, 0.0)
    for p in (1e-3, 0.5, 0.995, 1.0):
        assert dyn_threshold_rank(p, 1) == (0, 0.0)
    assert dyn_threshold_rank(0.5, 4) == (1, 0.5)
    assert dyn_threshold_rank(0.6, 8) == (4, float(np.float32(0.6 * 7 - 4)))
    k, f = dyn_threshold_rank(0.995, 3072)
    assert k == math.floor(0.995 * 3071) and f == float(np.float32(0.995 * 3071 - k)) and 0.0 <= f < 1.0
    # a remainder that rounds to 1.0f names the next rank (gmk_dyn_threshold asks for frac < 1): 0.57 * 100 = 56.99999999999999
    assert 0.57 * 100 < 57 and np.float32(0.57 * 100 - 56) == np.float32(1.0)
    assert dyn_threshold_rank(0.57, 101) == (57, 0.0)
    for bad in (0.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            dyn_threshold_rank(bad, 10)
    with pytest.raises(ValueError):
        dyn_threshold_rank(0.5, 0)
    with pytest.raises(ValueError):
        dyn_threshold_rank(0.5, 1 << 31)


def test_rank_is_the_literal_rule_on_the_gpu_tests_grid():
    """On the grid of the GPU bit test the host's (k_lo, frac) is the definition's (floor(pos), fp32(pos - floor(pos))) itself: no case there
    takes the frac -> 1.0f normalisation, so the bit test holds the kernel to the literal rule."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import dyn_threshold_rank
    for n in GPU_NS(ops.DYN_THRESHOLD_KEYS):
        for p in GPU_PS:
            lo, hi, frac = R.rank(p, n)
            k, f = dyn_threshold_rank(p, n)
            if lo == n - 1:
                assert (k, f) == (n - 1, 0.0) and frac == 0.0
            else:
                assert (k, f) == (lo, float(np.float32(frac))) and f < 1.0


def test_lds_capacity_constant_matches_the_kernel():
    from generative_models_amd import ops
    src = open(os.path.join(ROOT, "generative_models_amd", "csrc", "diffusion_ew.hip")).read()
    m = re.search(r"#define GMK_DYN_THRESHOLD_KEYS (\d+)\b", open(os.path.join(ROOT, "include", "gmk.h")).read())      # the kernel's constant is the header's
    assert "constexpr int kDynKeys = GMK_DYN_THRESHOLD_KEYS;" in src and m and int(m.group(1)) == ops.DYN_THRESHOLD_KEYS >= 12288


@pytest.mark.parametrize("bad", [-0.1, 1.0001, float("nan"), "x"])
def test_option_validation(bad):
    from generative_models_amd import common
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    with pytest.raises(ValueError):
        GaussianDiffusion(mean_type="v", num_steps=4, dyn_threshold=bad)
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cpu", dyn_threshold=bad)
    with pytest.raises(ValueError):
        Model(G)


def test_defaults_and_flag():
    from generative_models_amd import common, main
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    Model = common.discover_models()["diffusion_model"]
    assert Model.DG.dyn_threshold == 0.0
    assert GaussianDiffusion(mean_type="v", num_steps=4).dyn_threshold == 0.0
    assert GaussianDiffusion(mean_type="v", num_steps=4, dyn_threshold=1).dyn_threshold == 1.0
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--dyn_threshold", "0.995"])
    assert G.dyn_threshold == 0.995
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G.dyn_threshold == 0.0


def test_header_declares_the_entries():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    ret, argtypes, argnames = protos["gmk_dyn_threshold"]
    assert argnames == ["v", "v_uncond", "cond_w", "z", "logsnr_t", "k_lo", "frac", "s_out", "q_out", "mean_type", "B", "n", "stream"]
    assert argtypes == [P] * 4 + [F, I, F, P, P, I, I, L, P] and ret is ctypes.c_int
    old_s = ["v", "v_uncond", "cond_w", "z", "noise", "logsnr_t", "logsnr_s", "is_last", "z_next", "x_pred", "eps_pred", "z_dup",
             "logsnr_next", "mean_type", "B", "n", "stream"]
    old_d = ["v", "v_uncond", "cond_w", "z", "x_hist", "logsnr_t", "logsnr_s", "coef_z", "coef_x", "coef_prev", "is_last", "z_next", "x_pred",
             "eps_pred", "z_dup", "logsnr_next", "mean_type", "B", "n", "stream"]
    assert protos["gmk_sampler_step"][2] == old_s and protos["gmk_dpm_solver_step"][2] == old_d          # the old two as pinned
    assert protos["gmk_sampler_step"][1] == [P] * 5 + [F, F, I] + [P] * 5 + [I, I, L, P]
    assert protos["gmk_dpm_solver_step"][1] == [P] * 5 + [F] * 5 + [I] + [P] * 5 + [I, I, L, P]
    # the _dt entries: the same lists plus `thr` after cond_w
    assert protos["gmk_sampler_step_dt"][2] == old_s[:3] + ["thr"] + old_s[3:]
    assert protos["gmk_dpm_solver_step_dt"][2] == old_d[:3] + ["thr"] + old_d[3:]
    assert protos["gmk_sampler_step_dt"][1] == [P] * 6 + [F, F, I] + [P] * 5 + [I, I, L, P]
    assert protos["gmk_dpm_solver_step_dt"][1] == [P] * 6 + [F] * 5 + [I] + [P] * 5 + [I, I, L, P]
    assert all(protos[k][0] is ctypes.c_int for k in ("gmk_sampler_step_dt", "gmk_dpm_solver_step_dt"))


def test_entries_reject_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first

    def sel(v=buf, vu=None, w=None, z=buf, s=buf, mt=0, B=2, n=64, k=3, frac=0.5, lt=-1.0):
        return lib.gmk_dyn_threshold(v, vu, w, z, lt, k, frac, s, None, mt, B, n, None)
    for kw in ({"v": None}, {"z": None}, {"s": None}):
        assert sel(**kw) == -1 and b"null pointer" in lib.gmk_last_error()
    for mt in (-1, 3):
        assert sel(mt=mt) == -1 and b"mean_type" in lib.gmk_last_error()
    assert sel(vu=buf) == -1 and b"together" in lib.gmk_last_error()
    assert sel(w=buf) == -1 and b"together" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"n": 0}, {"n": 1 << 31}):
        assert sel(**kw) == -1 and b"shape" in lib.gmk_last_error()
    for k in (-1, 64):
        assert sel(k=k) == -1 and b"k_lo" in lib.gmk_last_error()
    for frac in (-0.25, 1.0, float("nan")):
        assert sel(frac=frac) == -1 and b"frac" in lib.gmk_last_error()
    assert sel(lt=float("inf")) == -1 and b"non-finite" in lib.gmk_last_error()

    def step(thr=buf, v=buf, vu=None, w=None, z=buf, zn=buf, mt=0, B=2, n=64):
        return lib.gmk_sampler_step_dt(v, vu, w, thr, z, None, -1.0, 1.0, 0, zn, None, None, None, None, mt, B, n, None)

    def dpm(thr=buf, v=buf, vu=None, w=None, z=buf, hist=buf, zn=buf, mt=0, B=2, n=64, coef_prev=0.5):
        return lib.gmk_dpm_solver_step_dt(v, vu, w, thr, z, hist, -1.0, 1.0, 0.5, 0.5, coef_prev, 0, zn, None, None, None, None, mt, B, n, None)
    for call in (step, dpm):
        for kw in ({"thr": None}, {"v": None}, {"z": None}, {"zn": None}):
            assert call(**kw) == -1 and b"null pointer" in lib.gmk_last_error()
        assert call(mt=3) == -1 and b"mean_type" in lib.gmk_last_error()
        assert call(vu=buf) == -1 and b"together" in lib.gmk_last_error()
        assert call(B=0) == -1 and b"shape" in lib.gmk_last_error()
    assert dpm(hist=None) == -1 and b"null pointer" in lib.gmk_last_error()
    assert dpm(coef_prev=float("nan")) == -1 and b"non-finite" in lib.gmk_last_error()
    assert b"gmk_dpm_solver_step_dt" in lib.gmk_last_error()           # errors name the entry that was called


def test_restatement_with_s_forced_to_one_is_the_oracles_ddim():
    """With s = 1 and no guidance step 3 is the static clip, so the restatement's chain is oracle.diffusion_ref.sample ('ddim') up to the
    rounding of the oracle's fp32 algebra (C = 32 keeps the CPU U-Net fast)."""
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    params = U.reference_init_params(32, 1, zero_out_layers=False, seed=3)
    g = torch.Generator().manual_seed(4)
    init = torch.randn((2, 1, 8, 8), generator=g)
    y = torch.tensor([2, 5])
    with torch.no_grad():
        for mean_type in ("v", "eps"):
            a = R.sample(params, init, y, 4, 0.9, "ddim", mean_type=mean_type, force_s=1.0)
            b = D.sample(params, init, y, 4, "ddim", mean_type=mean_type)
            for p_, q_ in zip(a, b):
                assert float((p_ - q_.double()).abs().max()) <= 1e-5 * float(q_.abs().max())
        # and the threshold does something: free, the chain differs where q > 1
        c = R.sample(params, init * 2, y, 4, 0.9, "ddim")
        d = R.sample(params, init * 2, y, 4, 0.9, "ddim", force_s=1.0)
        assert float((c[1] - d[1]).abs().max()) > 1e-3 and float(c[1].abs().max()) <= 1.0
