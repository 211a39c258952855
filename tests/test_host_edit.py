"""CPU tests (no GPU) of SDEdit editing and latent interpolation (`GaussianDiffusion.edit` / `interpolate`, gmk_slerp, DG.edit_eval,
DG.interp_eval; extensions): sampler plans that start part-way, the strength table, the entry point's argument checks, the flags, and the
properties of the float64 restatement (tests/edit_ref.py) the GPU tests hold the kernel to."""
import ctypes
import math
import os
import sys

import pytest
import torch
import yaml

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ref  # noqa: E402

STEPS = (1, 2, 5, 250)


# ---- plans that start part-way ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", STEPS)
def test_no_start_is_todays_plan(T):
    """start=None and start=T return the lists the two-argument calls build: the grid, the coefficient rows, the pass counts."""
    from generative_models_amd.diffusion import gaussian_diffusion as G
    grid = G.sampler_grid(T)
    assert [i for i, _, _ in grid] == list(range(T))[::-1]
    for sampler in ("ddim", "noisy", "dpmpp_2m"):
        for resample in (None, 1, 3):
            full = G.sampler_plan(T, sampler, resample)
            assert full == G.sampler_plan(T, sampler, resample, start=None) == G.sampler_plan(T, sampler, resample, start=T)
            assert [(s.i, s.lt, s.ls) for s in full] == grid and len(full) == T
            assert [s.is_last for s in full] == [i == 0 for i, _, _ in grid]
            assert [s.passes for s in full] == [1 if resample is None else G.inpaint_passes(i, resample) for i, _, _ in grid]
            assert [s.inp for s in full] == (G.inpaint_coefs(T) if resample is not None else [None] * T)
            assert [s.dpm for s in full] == (G.dpm_solver_coefs(T) if sampler == "dpmpp_2m" else [None] * T)
    rows = G.dpm_solver_coefs(T)
    assert rows == G.dpm_solver_coefs(T, start=None) == G.dpm_solver_coefs(T, start=T)
    assert rows[0].coef_prev == 0.0 and rows[-1].coef_prev == 0.0 and [r.i for r in rows] == list(range(T))[::-1]


@pytest.mark.parametrize("T", STEPS)
def test_start_keeps_the_tail_of_the_plan(T):
    from generative_models_amd.diffusion import gaussian_diffusion as G
    for k in sorted({1, 2, T // 2, T - 1, T} & set(range(1, T + 1))):
        for sampler in ("ddim", "noisy"):
            for resample in (None, 2):
                assert G.sampler_plan(T, sampler, resample, start=k) == G.sampler_plan(T, sampler, resample)[T - k:]
        full, part = G.sampler_plan(T, "dpmpp_2m"), G.sampler_plan(T, "dpmpp_2m", start=k)
        assert len(part) == k and part[0].i == k - 1
        assert part[0].dpm.coef_prev == 0.0                                       # no history at the first kept row
        assert part[0].dpm._replace(coef_prev=full[T - k].dpm.coef_prev) == full[T - k].dpm
        assert part[0]._replace(dpm=None) == full[T - k]._replace(dpm=None)
        assert part[1:] == full[T - k + 1:]
        assert G.dpm_solver_coefs(T, start=k) == [s.dpm for s in part]
        # z at plan[0].lt is z at logsnr(k / T)
        assert part[0].lt == G.logsnr_schedule_cosine_host(G.sampler_times(k - 1, T)[0])


@pytest.mark.parametrize("T", [1, 5])
def test_bad_start_raises(T):
    from generative_models_amd.diffusion import gaussian_diffusion as G
    for bad in (0, T + 1, 2.5, True, -1, "3", float("nan")):
        with pytest.raises(ValueError, match="start"):
            G.sampler_plan(T, "ddim", start=bad)
        with pytest.raises(ValueError, match="start"):
            G.dpm_solver_coefs(T, start=bad)


def test_edit_start_table():
    from generative_models_amd.diffusion.gaussian_diffusion import edit_start
    table = [(0.5, 5, 3),          # 2.5 rounds up
             (0.3, 5, 2),          # 1.5 rounds up
             (0.1, 5, 1),          # 0.5 rounds up
             (0.7, 5, 4),          # 3.5 (3.4999.. in binary: floor(3.9999..) = 3 would be wrong only if the sum fell short - it does not)
             (0.5, 250, 125), (0.002, 250, 1), (0.006, 250, 2), (0.25, 250, 63),
             (1e-9, 250, 1), (1e-9, 1, 1), (1.0, 250, 250), (1.0, 1, 1), (0.999, 250, 250), (0.997, 250, 249), (0.4, 1, 1), (0.5, 2, 1), (0.75, 2, 2)]
    for strength, T, k in table:
        assert edit_start(strength, T) == min(T, max(1, math.floor(strength * T + 0.5))) == k, (strength, T)
    for bad in (0, 0.0, 1.0001, -0.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="strength"):
            edit_start(bad, 10)


# ---- the restatement's slerp -----------------------------------------------------------------------------------------------------------------
def _rows(B=4, n=96, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, n), generator=g, dtype=torch.float64), torch.randn((B, n), generator=g, dtype=torch.float64)


def test_reference_slerp_keeps_a_common_norm():
    a, b = _rows()
    b = b * (a.norm(dim=1) / b.norm(dim=1))[:, None]
    t = [0.0, 0.125, 0.3, 0.5, 0.9, 1.0]
    out, c = edit_ref.slerp(a, b, t)
    assert out.shape == (6, 4, 96)
    norms = out.norm(dim=2)
    assert float((norms / a.norm(dim=1)[None] - 1).abs().max()) < 1e-12
    assert float((c - (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))).abs().max()) < 1e-12
    # the angle to a grows linearly in t
    ang = torch.acos(((out * a[None]).sum(2) / (norms * a.norm(dim=1)[None])).clamp(-1, 1))
    assert float((ang - torch.tensor(t)[:, None] * torch.acos(c)[None]).abs().max()) < 1e-7


def test_reference_slerp_endpoints_are_exact():
    a, b = _rows(seed=1)
    out, _ = edit_ref.slerp(a * 1.7, b * 0.6, [0.0, 1.0])
    assert torch.equal(out[0], a * 1.7) and torch.equal(out[1], b * 0.6)


def test_reference_slerp_falls_back_to_lerp():
    a, _ = _rows(seed=2)
    b = a.clone()
    b[1] = 2.5 * a[1]                   # parallel
    b[2] = -a[2]                        # antipodal
    a[3] = 0.0                          # a zero row: the cosine is 0 / 0
    t = [0.0, 0.25, 0.5, 1.0]
    out, c = edit_ref.slerp(a, b, t)
    assert bool(torch.isfinite(out).all())
    assert torch.equal(out, edit_ref.lerp(a, b, t))
    assert float(c[1]) == pytest.approx(1.0) and float(c[2]) == pytest.approx(-1.0) and math.isnan(float(c[3]))
    assert torch.equal(out[2, 2], torch.zeros_like(a[2]))                         # half-way between a and -a


def test_reference_noised_and_chain_shapes():
    """noised() is the oracle's q_sample in float64; a chain from start = T is the oracle's sample()."""
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    params = U.reference_init_params(32, 1, zero_out_layers=False, seed=3)
    g = torch.Generator().manual_seed(4)
    x = torch.rand((2, 1, 8, 8), generator=g) * 2 - 1
    eps = torch.randn((2, 1, 8, 8), generator=g)
    T = 3
    for k in (1, 2, 3):
        lt = edit_ref.grid_logsnr(k - 1, T)[0]
        assert torch.allclose(edit_ref.noised(x, eps, k, T).float(), D.q_sample(x, lt, eps), atol=1e-6)
    y = torch.tensor([2, 5])
    with torch.no_grad():
        whole = edit_ref.sample(params, eps, y, T, T, "ddim")
        ref = D.sample(params, eps, y, T, "ddim")
        for p, q in zip(whole, ref):
            assert torch.equal(p, q)
        zs, xs, es = edit_ref.sample(params, whole[0][0], y, T, 2, "ddim")           # from the whole chain's z after its first step
    assert zs.shape == (2, 2, 1, 8, 8) and torch.equal(zs, whole[0][1:]) and torch.equal(xs, whole[1][1:])


# ---- the entry point's checks and the wrappers' -------------------------------------------------------------------------------------------------
def test_gmk_slerp_argument_checks():
    from generative_models_amd._lib import PROTOS, lib
    assert PROTOS["gmk_slerp"][2] == ["a", "b", "t", "out", "cos_out", "B", "n", "K", "stream"]
    buf = ctypes.create_string_buffer(4096 + 16)
    p = (ctypes.addressof(buf) + 15) // 16 * 16

    def call(a=p, b=p + 256, t=p + 512, out=p + 1024, B=1, n=8, K=1):
        return lib.gmk_slerp(a, b, t, out, None, B, n, K, None)
    for kw in ({"a": None}, {"b": None}, {"t": None}, {"out": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"K": 0}, {"n": 0}, {"n": 3}, {"n": 6}, {"n": -4}):
        assert call(**kw) == -1 and b"shape" in lib.gmk_last_error()
    for kw in ({"a": p + 4}, {"b": p + 8}, {"out": p + 1028}):
        assert call(**kw) == -1 and b"aligned" in lib.gmk_last_error()


def test_ops_slerp_checks_before_any_launch():
    from generative_models_amd import ops
    a = torch.zeros((2, 8))
    with pytest.raises(ValueError, match="shape"):
        ops.slerp(a, torch.zeros((2, 12)), torch.zeros((1,)))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.slerp(torch.zeros((2, 6)), torch.zeros((2, 6)), torch.zeros((1,)))
    with pytest.raises(ValueError, match="dtype"):
        ops.slerp(a.double(), a.double(), torch.zeros((1,)))
    with pytest.raises(ValueError, match="t:"):
        ops.slerp(a, a, torch.zeros((1,), dtype=torch.float64))
    with pytest.raises(ValueError, match="t:"):
        ops.slerp(a, a, torch.zeros((2, 2)))
    with pytest.raises(ValueError, match="device tensor"):
        ops.slerp(a, a, torch.zeros((2,)))


def test_edit_and_interpolate_checks_before_any_launch():
    from functools import partial

    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    d = GaussianDiffusion(mean_type="v", num_steps=5)
    x = torch.zeros((2, 1, 8, 8))
    net = lambda *a, **k: None
    for bad in (0, 6, 2.5, True, None):
        with pytest.raises(ValueError, match="start"):
            d.edit(net=net, x=x, start=bad)
    with pytest.raises(ValueError, match="mask"):
        d.edit(net=net, x=x, start=2, mask=torch.full((1,), 2.0))
    with pytest.raises(ValueError, match="multiple of 4"):
        d.edit(net=net, x=torch.zeros((2, 1, 3, 3)), start=2, mask=torch.ones((1,)))
    for bad in (1, 0, 2.5, True):
        with pytest.raises(ValueError, match="frames"):
            d.interpolate(net=net, xa=x, xb=x, frames=bad, num_steps=3)
    with pytest.raises(ValueError, match="differs"):
        d.interpolate(net=net, xa=x, xb=torch.zeros((2, 1, 8, 4)), frames=3, num_steps=3)
    with pytest.raises(ValueError, match="cond_w"):
        d.interpolate(net=partial(net, cond_w=torch.ones((2,))), xa=x, xb=x, frames=3, num_steps=3)
    with pytest.raises(ValueError, match="num_steps"):
        d.interpolate(net=net, xa=x, xb=x, frames=3, num_steps=0)
    student = GaussianDiffusion(mean_type="v", num_steps=5, teacher_net=object(), teacher_mode="step1")
    with pytest.raises(ValueError, match="distilled"):
        student.interpolate(net=net, xa=x, xb=x, frames=3, num_steps=3)


# ---- the flags ---------------------------------------------------------------------------------------------------------------------------------
def test_flag_defaults_cli_and_hps(tmp_path):
    from generative_models_amd import common, main
    Model = common.discover_models()["diffusion_model"]
    assert Model.DG.edit_eval == 0.0 and isinstance(Model.DG.edit_eval, float)
    assert Model.DG.interp_eval == 0 and isinstance(Model.DG.interp_eval, int)
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G.edit_eval == 0.0 and G.interp_eval == 0
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--edit_eval", "0.5", "--interp_eval", "7"])
    assert G.edit_eval == 0.5 and G.interp_eval == 7
    G.logdir = str(tmp_path)

    class Writer:
        def add_scalar(self, *a):
            pass

        def flush(self):
            pass
    common.dump_logger({"loss": [1.0]}, Writer(), 0, G)
    with open(tmp_path / "hps.yaml") as f:
        hps = yaml.load(f, Loader=yaml.Loader)
    assert hps["edit_eval"] == 0.5 and hps["interp_eval"] == 7


@pytest.mark.parametrize("flags,name", [({"edit_eval": -0.1}, "edit_eval"), ({"edit_eval": 1.5}, "edit_eval"), ({"edit_eval": float("nan")}, "edit_eval"),
                                        ({"interp_eval": 1}, "interp_eval"), ({"interp_eval": -2}, "interp_eval")])
def test_model_flag_check(flags, name):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(hidden_size=32, **flags)
    with pytest.raises(ValueError, match=name):
        Model(G)


def test_model_takes_good_flags():
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(hidden_size=32, edit_eval=1.0, interp_eval=2)
    m = Model(G)
    assert m.edit_eval == 1.0 and m.interp_eval == 2
    assert Model.EDIT_EVAL_SEED not in (Model.INPAINT_EVAL_SEED, Model.INPAINT_EVAL_SEED + 1)
