"""CPU tests (no GPU) of the guided samplers' two options (`GaussianDiffusion(guidance_interval=(lo, hi), cfg_rescale=phi)`, gmk_cfg_rescale; an
extension): option validation, the per-row guidance mask and the forwarded-image count, the flags and the plugin's refusals, the C ABI and its
argument checks, and the restatement's (tests/guidance_ref.py) anchors to the chains of tests/sampler_ref.py."""
import ctypes
import math
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as G  # noqa: E402
import sampler_ref as S  # noqa: E402

INF = math.inf


# ---- guidance_check ----------------------------------------------------------------------------------------------------------------------------
def test_check_passes_through():
    from generative_models_amd.diffusion.gaussian_diffusion import guidance_check
    assert guidance_check(None, 0.0) == (None, 0.0)
    assert guidance_check((-3, 1.5), 0.7) == ((-3.0, 1.5), 0.7)
    assert guidance_check([-3.0, 1.5], 1, "dpmpp_2m") == ((-3.0, 1.5), 1.0)
    assert guidance_check((-INF, INF), 0) == (None, 0.0)                       # both infinite: off
    assert guidance_check((-INF, 2.0), 0) == ((-INF, 2.0), 0.0)
    assert guidance_check((1.0, 1.0), 0) == ((1.0, 1.0), 0.0)
    assert guidance_check((-3, 3), 0.0, "consistency") == ((-3.0, 3.0), 0.0)   # the interval is host logic: every sampler takes it
    assert guidance_check((-3, 3), 0.0, "ddim", 0.995) == ((-3.0, 3.0), 0.0)   # ... and so does dynamic thresholding
    pair, phi = guidance_check((-3, 3), 0.3)
    assert all(type(v) is float for v in pair) and type(phi) is float


@pytest.mark.parametrize("interval", [(1.0, -1.0), (float("nan"), 1.0), (0.0, float("nan")), (INF, -INF), (1.0,), (1.0, 2.0, 3.0), "ab", 3.0,
                                      ("x", 1.0)])
def test_check_refuses_intervals(interval):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, guidance_check
    with pytest.raises(ValueError, match="guidance_interval"):
        guidance_check(interval, 0.0)
    with pytest.raises(ValueError, match="guidance_interval"):
        GaussianDiffusion(mean_type="v", num_steps=4, guidance_interval=interval)


@pytest.mark.parametrize("phi", [-0.1, 1.0001, float("nan"), "x", None])
def test_check_refuses_phi(phi):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, guidance_check
    with pytest.raises(ValueError, match="cfg_rescale"):
        guidance_check(None, phi)
    with pytest.raises(ValueError, match="cfg_rescale"):
        GaussianDiffusion(mean_type="v", num_steps=4, cfg_rescale=phi)


def test_check_refuses_combinations():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, guidance_check
    with pytest.raises(ValueError, match="dyn_threshold"):
        guidance_check(None, 0.7, "ddim", 0.995)
    with pytest.raises(ValueError, match="consistency"):
        guidance_check(None, 0.7, "consistency")
    with pytest.raises(ValueError, match="dyn_threshold"):
        GaussianDiffusion(mean_type="v", num_steps=4, cfg_rescale=0.7, dyn_threshold=0.9)
    with pytest.raises(ValueError, match="consistency"):
        GaussianDiffusion(mean_type="v", num_steps=4, cfg_rescale=0.7, sampler="consistency")
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    assert d.guidance_interval is None and d.cfg_rescale == 0.0
    d = GaussianDiffusion(mean_type="v", num_steps=4, guidance_interval=(-3, 3), cfg_rescale=0.7, sampler="dpmpp_2m")
    assert d.guidance_interval == (-3.0, 3.0) and d.cfg_rescale == 0.7


def test_restore_refuses_rescale():
    """Restoration and the rescale are refused together, by an error that names both, before anything touches a device."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    d = GaussianDiffusion(mean_type="v", num_steps=4, cfg_rescale=0.7)
    x = torch.zeros((2, 1, 8, 8))
    with pytest.raises(ValueError, match=r"restor.*cfg_rescale|cfg_rescale.*restor"):
        d.restore(net=lambda *a, **k: None, obs=torch.zeros((2, 1, 4, 4)), factor=2, init_x=x)


# ---- guidance_mask / guidance_evals ---------------------------------------------------------------------------------------------------------------
def test_six_step_grid():
    """The grid the GPU chains run on: -20.001, -2.634, -1.099, -0.0, 1.099, 2.634 - the restatement's times are the plan's."""
    from generative_models_amd.diffusion.gaussian_diffusion import sampler_plan
    plan = sampler_plan(6)
    lts = [float(s.lt) for s in plan]
    assert lts == G.grid(6)
    assert [round(l, 3) for l in lts] == [-20.001, -2.634, -1.099, -0.0, 1.099, 2.634]
    assert lts[0] < -20.0


def test_mask():
    from generative_models_amd.diffusion.gaussian_diffusion import guidance_mask, sampler_plan
    F, T = False, True
    for sampler in ("ddim", "dpmpp_2m", "consistency"):
        plan = sampler_plan(6, sampler)
        assert guidance_mask(plan, (-3.0, 1.5)) == [F, T, T, T, T, F]
        assert guidance_mask(plan, None) == [T] * 6
        assert guidance_mask(plan, (-21.0, 21.0)) == [T] * 6
        assert guidance_mask(plan, (-20.0, 21.0)) == [F, T, T, T, T, T]       # the first time is below -20
        assert guidance_mask(plan, (-2.0, -1.5)) == [F] * 6                    # between two grid points
        assert guidance_mask(plan, (-INF, 0.0)) == [T, T, T, T, F, F]          # -0.0 <= 0.0
        assert guidance_mask(plan, (float(plan[2].lt), float(plan[2].lt))) == [F, F, T, F, F, F]      # the ends are included
    assert guidance_mask(sampler_plan(6, start=3), (-3.0, 1.5)) == [T, T, F]  # a chain that begins part-way: its own rows
    assert all(isinstance(g, bool) for g in guidance_mask(sampler_plan(6), (-3.0, 1.5)))


def test_plans_are_untouched():
    """`SamplerStep` keeps its fields: existing tests compare plans for equality."""
    from generative_models_amd.diffusion.gaussian_diffusion import SamplerStep
    assert SamplerStep._fields == ("i", "lt", "ls", "is_last", "passes", "dpm", "inp")


def test_evals():
    from generative_models_amd.diffusion.gaussian_diffusion import guidance_evals, guidance_mask, sampler_plan
    plan = sampler_plan(6)
    B = 3
    assert guidance_evals(plan, guidance_mask(plan, (-3.0, 1.5)), B) == B * (6 + 4)
    assert guidance_evals(plan, guidance_mask(plan, None), B) == 12 * B
    assert guidance_evals(plan, [False] * 6, B) == 6 * B
    plan = sampler_plan(6, resample=3)                                         # inpainting: 3 passes per step, the last step one
    assert [s.passes for s in plan] == [3, 3, 3, 3, 3, 1]
    assert guidance_evals(plan, guidance_mask(plan, (-3.0, 1.5)), B) == B * (16 + 12)


# ---- flags and the plugin ------------------------------------------------------------------------------------------------------------------------
def test_defaults_and_flags():
    from generative_models_amd import common, main
    Model = common.discover_models()["diffusion_model"]
    assert Model.DG.guidance_lo == -INF and Model.DG.guidance_hi == INF and Model.DG.cfg_rescale == 0.0
    G0, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G0.guidance_lo == -INF and G0.guidance_hi == INF and G0.cfg_rescale == 0.0
    G1, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--sample_cond_w", "2.0", "--guidance_lo", "-3", "--guidance_hi", "1.5",
                                             "--cfg_rescale", "0.7"])
    assert (G1.guidance_lo, G1.guidance_hi, G1.cfg_rescale, G1.sample_cond_w) == (-3.0, 1.5, 0.7, 2.0)
    G2, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--guidance_lo=-inf", "--guidance_hi=3"])
    assert G2.guidance_lo == -INF and G2.guidance_hi == 3.0


def test_yaml_round_trips_the_infinities():
    import yaml
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    text = yaml.dump({k: Model.DG[k] for k in ("guidance_lo", "guidance_hi", "cfg_rescale")})
    assert ".inf" in text
    back = yaml.load(text, Loader=yaml.Loader)
    assert back == {"guidance_lo": -INF, "guidance_hi": INF, "cfg_rescale": 0.0}


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    Gm = common.AttrDict(dict(Model.DG))
    Gm.update(lr=3e-4, pad32=0, device="cpu", **flags)
    return Model(Gm)


def test_plugin_passes_the_options_on():
    m = _model()
    assert m.diffusion.guidance_interval is None and m.diffusion.cfg_rescale == 0.0
    m = _model(guidance_lo=-3.0, guidance_hi=1.5, cfg_rescale=0.7, sample_cond_w=2.0)
    assert m.diffusion.guidance_interval == (-3.0, 1.5) and m.diffusion.cfg_rescale == 0.7
    m = _model(guidance_hi=1.5)
    assert m.diffusion.guidance_interval == (-INF, 1.5)
    m = _model(guidance_lo=-3.0, guidance_hi=3.0, sampler="consistency")
    assert m.diffusion.guidance_interval == (-3.0, 3.0)


@pytest.mark.parametrize("flags", [dict(guidance_lo=2.0, guidance_hi=-2.0), dict(guidance_lo=float("nan")), dict(cfg_rescale=1.5),
                                   dict(cfg_rescale=-0.1), dict(cfg_rescale=0.7, dyn_threshold=0.995),
                                   dict(cfg_rescale=0.7, sampler="consistency"), dict(cfg_rescale=0.7, restore_eval=2),
                                   dict(cfg_rescale=0.7, restore_gray=1, in_channels=3)])
def test_plugin_refuses(flags):
    with pytest.raises(ValueError):
        _model(**flags)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry():
    from generative_models_amd import _lib, ops
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    ret, argtypes, argnames = protos["gmk_cfg_rescale"]
    assert argnames == ["v", "v_uncond", "cond_w", "z", "logsnr_t", "phi", "thr_out", "ratio_out", "mean_type", "B", "n", "stream"]
    assert argtypes == [P] * 4 + [F, F, P, P, I, I, L, P] and ret is ctypes.c_int
    header = open(os.path.join(ROOT, "include", "gmk.h")).read()
    src = open(os.path.join(ROOT, "generative_models_amd", "csrc", "diffusion_ew.hip")).read()
    m = re.search(r"#define GMK_CFG_RESCALE_KEEP (\d+)\b", header)
    assert m and int(m.group(1)) == ops.CFG_RESCALE_KEEP == 12288 and "constexpr int kRescaleKeep = GMK_CFG_RESCALE_KEEP;" in src
    # no row in the kernel table, and the version stands
    assert "cfg_rescale" not in " ".join(name for _, _, name in _lib.parse_kernel_table()).lower() and _lib.lib.gmk_version() == 1
    assert "Lin et al. 2023" in src and "Kynkaanniemi et al. 2024" in src and "an extension, no reference call site" in src


def test_entry_rejects_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first

    def call(v=buf, vu=buf, w=buf, z=buf, thr=buf, ratio=None, lt=-1.0, phi=0.7, mt=0, B=2, n=64):
        return lib.gmk_cfg_rescale(v, vu, w, z, lt, phi, thr, ratio, mt, B, n, None)
    for kw in ({"v": None}, {"vu": None}, {"w": None}, {"z": None}, {"thr": None}):
        assert call(**kw) == -1 and b"null pointer" in lib.gmk_last_error(), kw
    for phi in (-0.1, 1.5, float("nan"), float("inf")):
        assert call(phi=phi) == -1 and b"phi" in lib.gmk_last_error()
    for mt in (-1, 3):
        assert call(mt=mt) == -1 and b"mean_type" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"n": 0}, {"B": -1}):
        assert call(**kw) == -1 and b"shape" in lib.gmk_last_error()
    assert call(lt=float("nan")) == -1 and b"non-finite" in lib.gmk_last_error()
    assert b"gmk_cfg_rescale" in lib.gmk_last_error()


def test_op_checks_on_the_host():
    from generative_models_amd import ops
    x = torch.zeros((2, 8))
    with pytest.raises(ValueError, match="required"):
        ops.cfg_rescale(x, x, -1.0, 0.7, None, None)
    with pytest.raises(ValueError, match="phi"):
        ops.cfg_rescale(x, x, -1.0, 1.5, x, torch.zeros((2,)))
    with pytest.raises(ValueError, match="device"):                            # the shared input checks: no CPU path
        ops.cfg_rescale(x, x, -1.0, 0.7, x, torch.zeros((2,)))


# ---- the restatement's anchors ----------------------------------------------------------------------------------------------------------------
def _small():
    from oracle import unet_ref as U
    params = U.reference_init_params(32, 1, zero_out_layers=False, seed=3)       # C = 32 keeps the CPU U-Net fast
    g = torch.Generator().manual_seed(4)
    return params, torch.randn((2, 1, 8, 8), generator=g), torch.tensor([2, 5]), torch.tensor([0.7, 2.4])


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_restatement_degenerates_to_the_sampler_refs_chains(sampler):
    """Every row guided and phi = 0: `sampler_ref`'s guided chain; no row guided: its unguided chain - up to the rounding of the fp32 update
    (the restatement carries z in float64)."""
    params, init, y, w = _small()
    T = 4
    with torch.no_grad():
        guided = S.chain(init, T, S.oracle_step(params, y, sampler, w))
        plain = S.chain(init, T, S.oracle_step(params, y, sampler, None))
        assert float((guided[0] - plain[0]).abs().max()) > 1e-3
        for interval in (None, (-21.0, 21.0)):
            got = G.sample(params, init, y, T, w, interval, 0.0, sampler)
            for a, b in zip(got, guided):
                assert float((a - b.double()).abs().max()) <= 1e-5 * float(b.abs().max())
        empty = (-1.0, -0.5)                                                   # between two points of the 4-step grid
        assert not any(G.inside(empty, l) for l in G.grid(T))
        got = G.sample(params, init, y, T, w, empty, 0.0, sampler)
        for a, b in zip(got, plain):
            assert float((a - b.double()).abs().max()) <= 1e-5 * float(b.abs().max())


def test_restatement_of_the_rescale():
    """f = 1 at phi = 0 and at w = 0; at phi = 1 the rescaled prediction has the conditional prediction's standard deviation."""
    g = torch.Generator().manual_seed(0)
    out, out_u, z = (torch.randn((3, 1, 8, 8), generator=g) for _ in range(3))
    lt = torch.full((3,), 0.5)
    w = torch.tensor([0.0, 2.0, 3.9])
    _, _, f0, r = G.predict(out, z, lt, 0.0, "v", out_u, w)
    assert torch.equal(f0, torch.ones_like(f0)) and float(r[0]) == 1.0 and float(r[1]) < 1.0 and float(r[2]) < float(r[1])
    _, _, f1, r1 = G.predict(out, z, lt, 1.0, "v", out_u, w)
    assert torch.allclose(f1, r1, rtol=0, atol=1e-15)
    import dyn_threshold_ref as R
    x_c, x_r = R.x_raw(out, z, lt, "v"), R.x_raw(out, z, lt, "v", out_u, w)
    scaled = f1[:, None, None, None] * x_r
    assert torch.allclose(scaled.flatten(1).std(dim=1), x_c.flatten(1).std(dim=1), rtol=1e-12, atol=0)
