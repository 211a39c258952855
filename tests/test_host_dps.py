"""Host tests of diffusion posterior sampling (DPS: Chung et al. 2023; `GaussianDiffusion.posterior_sample`, DG.dps_eval): the float64
restatement (tests/dps_ref.py) against its own definitions - the adjoint identity, the gradient formula against autograd through the oracle
U-Net, a closed form of the whole chain - the statement of the blur's fp32 arithmetic, the option checks, and the drift of the float32
restatement that the GPU chain bars (tests/test_gpu_dps.py) are derived from.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dps_ref as P  # noqa: E402
import restore_ref as R  # noqa: E402

from oracle import unet_ref as U  # noqa: E402

SHAPES = [(1, 8, 8), (3, 8, 8), (1, 12, 12), (1, 28, 28), (3, 32, 32), (3, 64, 64)]
B = 3


def operators(C, H, W):
    """Every operator of the issue's table that fits the shape: the blurs, and the box means whose side divides it (with and without gray)."""
    ops = [("blur", s) for s in P.BLUR_SIGMAS]
    for N in (2, 3, 4, 7):
        if H % N == 0 and W % N == 0:
            ops.append(("box", 1, N))
            if C > 1:
                ops.append(("box", C, N))
    if C > 1:
        ops.append(("box", C, 1))
    return ops


@pytest.mark.parametrize("C,H,W", SHAPES)
def test_adjoint_identity(C, H, W):
    """<A x, y> = <x, A^T y> in float64, to 1e-12 relative, for every operator and shape."""
    g = torch.Generator().manual_seed(C + H)
    x = torch.randn((B, C, H, W), generator=g, dtype=torch.float64)
    for op in operators(C, H, W):
        y = torch.randn(P.obs_shape(x.shape, op), generator=g, dtype=torch.float64)
        lhs, rhs = float((P.A(x, op) * y).sum()), float((x * P.AT(y, op)).sum())
        scale = float(P.A(x, op).norm() * y.norm())
        assert abs(lhs - rhs) <= 1e-12 * scale, (op, lhs, rhs)


def test_taps_are_the_package_s_and_sum_to_one():
    from generative_models_amd.diffusion.gaussian_diffusion import blur_taps
    for sigma, radius in zip(P.BLUR_SIGMAS + (5.0, 1.0), (2, 5, 9, 15, 3)):
        t = P.taps(sigma)
        assert len(t) == 2 * radius + 1 and t.dtype == np.float32
        assert blur_taps(sigma) == tuple(float(v) for v in t)
        assert abs(float(t.astype(np.float64).sum()) - 1.0) <= len(t) * 2.0 ** -25
        assert np.array_equal(t, t[::-1])


@pytest.mark.parametrize("C,H,W", [(1, 8, 8), (1, 12, 12), (3, 32, 32)])
def test_blur_fp32_statement_against_float64(C, H, W):
    """The numpy statement of the kernel's summation order stays within the bound the GPU test holds the kernel to: values in [-1, 1], taps
    summing to at most 1 per pass, at most 2 (2 R + 1) sequential additions of rounded products: (2 (2 R + 1) + 2) 2^-24."""
    g = torch.Generator().manual_seed(H)
    x = torch.rand((B, C, H, W), generator=g) * 2 - 1
    for sigma in P.BLUR_SIGMAS:
        err = float((torch.from_numpy(P.blur_fp32(x, sigma)).double() - P.A(x.double(), ("blur", sigma))).abs().max())
        assert err <= (2 * (2 * P.radius(sigma) + 1) + 2) * 2.0 ** -24, (sigma, err)


@pytest.mark.parametrize("mean_type", ["v", "x"])
def test_gradient_formula_against_autograd(mean_type):
    """c_z u + c_o J^T u = -1/2 grad_z |y - A x_hat(z)|^2, by torch.autograd through oracle.unet_ref.unet_forward: 8 x 8, B = 2, hidden 128,
    float64, to 1e-9 of the largest entry."""
    params = P.cast_params(U.reference_init_params(128, 1, seed=4, zero_out_layers=False), torch.float64)
    g = torch.Generator().manual_seed(3)
    z = torch.randn((2, 1, 8, 8), generator=g, dtype=torch.float64)
    y = torch.tensor([2, -1])
    for op in (("box", 1, 2), ("blur", 1.5)):
        obs = torch.randn(P.obs_shape(z.shape, op), generator=g, dtype=torch.float64)
        for lam in (-12.0, 1.0):
            _, d, s = P.guidance(params, z, lam, y, obs, op, mean_type)
            ref = P.autograd_direction(params, z, lam, y, obs, op, mean_type)
            err = float((d - ref).abs().max() / ref.abs().max())
            assert err <= 1e-9 and float(s.min()) > 0.1, (op, lam, err)


def test_chain_closed_form():
    """out.2 zeroed, mean type 'v': out = 0, J = 0, x_hat = alpha_t z, and the DDIM chain with a box operator is a scalar recurrence per box,
    written out independently in `box_recurrence`."""
    params = U.reference_init_params(128, 1, seed=0, zero_out_layers=False)
    params["out.2.weight"].zero_(); params["out.2.bias"].zero_()
    g = torch.Generator().manual_seed(5)
    init = torch.randn((2, 1, 8, 8), generator=g)
    obs = torch.rand((2, 1, 4, 4), generator=g) * 2 - 1
    for zeta in (0.0, 0.7):
        with torch.no_grad():
            z = P.sample(params, init, obs, ("box", 1, 2), torch.tensor([1, 2]), 4, "ddim", zeta, record=False)
        ref = P.box_recurrence(init, obs, 1, 2, 4, zeta)
        assert float((z - ref).abs().max()) <= 1e-12, zeta
    assert float((z - P.sample(params, init, obs, ("box", 1, 2), torch.tensor([1, 2]), 4, "ddim", 0.0, record=False)).abs().max()) > 1e-3


def test_noise_free_measurement_is_degrade():
    """The restatement's box operators are `restore`'s: A of 'box:N' / 'gray' / 'gray_box:N' is restore_ref.A with restore_operator's (cf, N),
    and the package's `measurement_op` names the same operator and observation shape."""
    from generative_models_amd.diffusion.gaussian_diffusion import measurement_op, restore_operator
    x = torch.rand((B, 3, 8, 8), generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for kind, factor, gray in (("box:2", 2, False), ("gray", 1, True), ("gray_box:4", 4, True)):
        op, low = measurement_op(kind, tuple(x.shape))
        cf, N, want = restore_operator(tuple(x.shape), factor, gray)
        assert (op.kind, op.cf, op.N, low) == ("box", cf, N, want) and op.taps == ()
        assert torch.equal(P.A(x, ("box", op.cf, op.N)), R.A(x, cf, N)) and P.A(x, ("box", cf, N)).shape == want
    op, low = measurement_op("blur:1.5", (B, 3, 8, 8))
    assert (op.kind, op.sigma, low, len(op.taps)) == ("blur", 1.5, (B, 3, 8, 8), 11)


def test_option_checks():
    from generative_models_amd.diffusion.gaussian_diffusion import (DPS_SAMPLERS, GaussianDiffusion, blur_taps, dps_check, dps_coefs, dps_zeta_check,
                                                                    measurement_op)
    shape = (2, 3, 8, 8)
    for kind in ("", "box", "box:", "box:x", "gray:2", "blur", "blur:wide", "sharpen:2", "box:2:2", 4, None):
        with pytest.raises(ValueError, match="measurement"):
            measurement_op(kind, shape)
    for kind, word in (("box:3", "does not divide"), ("box:1", "factor = 1"), ("box:0", "factor"), ("box:-2", "factor")):
        with pytest.raises(ValueError, match=word):
            measurement_op(kind, shape)
    with pytest.raises(ValueError, match="no colour"):
        measurement_op("gray", (2, 1, 8, 8))
    for sigma in (0.0, -1.0, 5.001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            blur_taps(sigma)
        with pytest.raises(ValueError, match="sigma"):
            measurement_op(f"blur:{sigma}", shape)
    with pytest.raises(ValueError, match="64 x 64"):
        measurement_op("blur:1.0", (1, 1, 128, 8))
    assert len(blur_taps(5.0)) == 31 and len(blur_taps(0.1)) == 3
    for zeta in (-0.5, float("nan"), float("inf"), "much", None):
        with pytest.raises(ValueError, match="zeta"):
            dps_zeta_check(zeta)
    assert dps_zeta_check(0) == 0.0 and dps_zeta_check(0.5) == 0.5
    # every refused combination names both sides
    for sampler in ("dpmpp_2m", "sde_dpmpp_2m", "consistency", "teacher_test"):
        with pytest.raises(ValueError, match=f"posterior_sample together with sampler '{sampler}'"):
            dps_check(sampler=sampler)
    for kw, word in ((dict(cond_w=True), "cond_w"), (dict(dyn_threshold=0.9), "dyn_threshold"), (dict(cfg_rescale=0.5), "cfg_rescale"),
                     (dict(learned_var=True), "learn_var"), (dict(student=True), "distilled student"), (dict(mean_type="eps"), "mean_type 'eps'")):
        with pytest.raises(ValueError, match="posterior_sample together with .*" + word):
            dps_check(sampler="ddim", **kw)
        with pytest.raises(ValueError, match="dps_eval together with"):
            dps_check(sampler="ancestral", what="dps_eval", **kw)
    for sampler in DPS_SAMPLERS:
        dps_check(sampler=sampler)
    dps_check(sampler="ddim", ddim_eta=0.5)
    assert dps_coefs(0.0, "x") == (0.0, 1.0) and dps_coefs(0.0, "v") == pytest.approx((0.5 ** 0.5, -(0.5 ** 0.5)))
    # the loop's own checks come before anything touches a device: the sampler, guidance, zeta, the operator, the observation's shape
    init, obs = torch.zeros(shape), torch.zeros((2, 3, 4, 4))
    op, _ = measurement_op("box:2", shape)
    net = lambda *a, **k: None
    call = lambda d, **kw: d.posterior_sample(**{**dict(net=net, obs=obs, op=op, init_x=init, zeta=1.0), **kw})
    with pytest.raises(ValueError, match="sampler 'dpmpp_2m'"):
        call(GaussianDiffusion(mean_type="v", num_steps=4, sampler="dpmpp_2m"))
    with pytest.raises(ValueError, match="cond_w"):
        call(GaussianDiffusion(mean_type="v", num_steps=4, sample_cond_w=2.0))
    with pytest.raises(ValueError, match="mean_type 'eps'"):
        call(GaussianDiffusion(mean_type="eps", num_steps=4))
    with pytest.raises(ValueError, match="dyn_threshold"):
        call(GaussianDiffusion(mean_type="v", num_steps=4, dyn_threshold=0.95))
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    with pytest.raises(ValueError, match="zeta"):
        call(d, zeta=-1.0)
    with pytest.raises(ValueError, match="MeasurementOp"):
        call(d, op=("box", 1, 2))
    for bad in (torch.zeros((2, 3, 8, 8)), torch.zeros((2, 1, 4, 4)), None):
        with pytest.raises(ValueError, match="obs shape"):
            call(d, obs=bad)
    with pytest.raises(ValueError, match="obs shape"):
        call(d, op=measurement_op("blur:1.0", shape)[0])
    assert d.rng.counter == 0


def test_plugin_flag_checks():
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    assert (Model.DG.dps_eval, Model.DG.dps_noise, Model.DG.dps_zeta) == ("", 0.05, 1.0)

    def build(**flags):
        G = common.AttrDict(dict(Model.DG))
        G.update(lr=3e-4, pad32=0, device="cpu", timesteps=4, bs=8, in_channels=3, image_size=8)
        G.update(flags)
        return Model(G)
    for flags, word in ((dict(dps_eval="box"), "measurement"), (dict(dps_eval="blur:9"), "sigma"), (dict(dps_eval="box:3"), "does not divide"),
                        (dict(dps_eval=2), "dps_eval"), (dict(dps_eval="box:2", dps_zeta=-1.0), "zeta"), (dict(dps_noise=-0.1), "dps_noise"),
                        (dict(dps_eval="box:2", sampler="dpmpp_2m"), "dps_eval together with sampler 'dpmpp_2m'"),
                        (dict(dps_eval="gray", mean_type="eps"), "dps_eval together with mean_type 'eps'"),
                        (dict(dps_eval="gray", sample_cond_w=1.5), "dps_eval together with .*cond_w"),
                        (dict(dps_eval="blur:1.5", dyn_threshold=0.9), "dps_eval together with dyn_threshold")):
        with pytest.raises(ValueError, match=word):
            build(**flags)
    model = build(dps_eval="gray_box:2", sampler="ancestral")
    assert (model.dps_eval, model.dps_noise, model.dps_zeta) == ("gray_box:2", 0.05, 1.0)


_DRIFT = {}


@pytest.mark.parametrize("kind", list(P.CHAIN_OPS))
def test_chain_drift_of_the_float32_restatement(kind):
    """The chain cases of tests/test_gpu_dps.py on the CPU: the float32 restatement against the float64 one.  The GPU bars are
    max(project bar, 4 x this drift); a case that needed more than 10 x the project's fp32 bar would have to be replaced by a
    better-conditioned one.  Prints the figures profiles/dps_probe.txt records."""
    params = U.reference_init_params(128, P.CHAIN_OPS[kind][0], seed=0, zero_out_layers=False)
    for sampler in P.CHAIN_SAMPLERS:
        drift, smin = P.chain_drift(params, kind, sampler)
        print(f"dps chain drift {kind} {sampler}: fp32 vs float64 {drift:.3e}, smallest |e| {smin:.3f}, fp32 bar {P.chain_bar(drift, 'fp32'):.3e}")
        assert 4.0 * max(drift, P.CHAIN_DRIFT[(kind, sampler)]) <= 10.0 * P.PROJECT_BAR["fp32"], (kind, sampler, drift)
