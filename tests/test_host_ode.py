"""CPU tests (no GPU) of the probability-flow ODE (`GaussianDiffusion.encode / decode / ode_nll`, `DiffusionModel.ode_nlogp`,
DG.ode_nlogp_steps): the float64 restatement (tests/ode_ref.py) on Gaussian data with the optimal predictor, where the ODE is linear and every
quantity has a closed form; the grid, trapezoid and divergence coefficients of the host against it; the documented draw order; the flag; and
the argument checks of the Python surface, the wrappers and the C entries."""
import ctypes
import math
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ode_ref  # noqa: E402

S = 0.5          # data N(0, S^2 I)


def _var(lam):
    a, s = ode_ref.coef(lam)
    return a * a * S * S + s * s


def _gauss_net(mean_type):
    """The optimal predictor for N(0, S^2 I) data, eps*(z, lambda) = sigma z / (alpha^2 S^2 + sigma^2), in each parametrisation, and its VJP."""
    def eps_coef(lam):
        a, s = ode_ref.coef(lam)
        return s / _var(lam)

    def out_coef(lam):            # out = k z: the mean type's output for that eps_hat
        a, s = ode_ref.coef(lam)
        e = eps_coef(lam)
        return {"eps": e, "v": (e - s) / a, "x": (1.0 - s * e) / a}[mean_type]
    return (lambda z, lam: out_coef(lam) * z), (lambda z, lam, r: out_coef(lam) * r)


def _y(B=4, D=16, seed=0):
    return torch.randn((B, D), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * S


def _exact_nlogp(y, lam0):
    """-log N(y; 0, (alpha_0^2 S^2 + sigma_0^2) I) / D"""
    v, D = _var(lam0), y.shape[1]
    return (0.5 * (y * y).sum(1) / v + 0.5 * D * math.log(2 * math.pi * v)) / D


@pytest.mark.parametrize("mean_type", ["eps", "v", "x"])
def test_gaussian_likelihood_converges_to_the_exact_density(mean_type):
    """Rademacher probes give the trace of the (diagonal) Jacobian exactly, so what is left is the discretisation.  The trapezoid sum of the
    divergence is second order: within 1e-3 of its exact value D/2 log(var_0 / var_N) per dimension at N = 256.  The DDIM update is first order
    in the angle theta = atan(sigma / alpha): every step contracts z by cos(d theta) against the exact flow, so z_N and with it the prior term
    carry an O(1/N) error (1.2e-2 nats/dim at N = 256 here).  With z_N replaced by the exact flow's value the estimate is within 1e-3 at N = 256;
    the full estimate's error halves with every doubling of N."""
    fwd, vjp = _gauss_net(mean_type)
    y = _y()
    B, D = y.shape
    half = torch.full_like(y, 0.5)                    # u = 1/2: no dequantisation offset, y is the point
    errs = []
    for N in (64, 128, 256, 512):
        g = torch.Generator().manual_seed(N)
        probes = [ode_ref.rademacher(torch.rand((B, D), generator=g)) for _ in range(N + 1)]
        r = ode_ref.ode_nll(fwd, vjp, y, N, half, probes, 1 / 255, mean_type)
        lam = ode_ref.logsnr_grid(N)
        exact = _exact_nlogp(y, lam[0])
        got = r["nlogp"] + math.log(2 / 255)          # -log p(y) / D
        errs.append(float((got - exact).abs().max()))
        exact_div = 0.5 * math.log(_var(lam[0]) / _var(lam[-1]))
        z_flow = y * math.sqrt(_var(lam[-1]) / _var(lam[0]))
        with_flow = -ode_ref.log_normal(z_flow) / D + r["divergence"]
        if N == 256:
            assert float((r["divergence"] - exact_div).abs().max()) < 1e-3
            assert float((with_flow - exact).abs().max()) < 1e-3
    assert errs[2] < 1.5e-2, errs
    assert all(b < 0.6 * a for a, b in zip(errs, errs[1:])), errs


@pytest.mark.parametrize("mean_type", ["eps", "v", "x"])
def test_gaussian_encode_and_decode(mean_type):
    """encode -> the continuous flow's z_N = y sqrt(var_N / var_0) and decode(encode(y)) -> y, both with relative errors O(1/N) (the first-order
    update: 1.5 / N and 3 / N here)."""
    fwd, _ = _gauss_net(mean_type)
    y = _y(seed=1)
    enc_err, rt_err = [], []
    for N in (32, 128, 512):
        lam = ode_ref.logsnr_grid(N)
        z = ode_ref.encode(fwd, y, N, mean_type)
        flow = y * math.sqrt(_var(lam[-1]) / _var(lam[0]))
        enc_err.append(float((z - flow).norm() / flow.norm()))
        back = ode_ref.decode(fwd, z, N, mean_type)
        rt_err.append(float((back - y).norm() / y.norm()))
    assert enc_err[-1] < 5e-3 and all(b < 0.3 * a for a, b in zip(enc_err, enc_err[1:])), enc_err
    assert rt_err[-1] < 1e-2 and all(b < 0.3 * a for a, b in zip(rt_err, rt_err[1:])), rt_err


def test_host_grid_weights_and_coefficients_match_the_restatement():
    from generative_models_amd.diffusion.gaussian_diffusion import ode_divergence_coefs, ode_logsnr_grid, ode_trapezoid_weights
    for N in (1, 4, 64, 512):
        lam = ode_logsnr_grid(N)
        ref = ode_ref.logsnr_grid(N)
        assert len(lam) == N + 1 and all(isinstance(v, float) for v in lam)
        assert max(abs(a - b) for a, b in zip(lam, ref)) < 2e-3      # the samplers' fp32 schedule (tan near pi / 2 at the prior end)
        assert all(a > b for a, b in zip(lam, lam[1:]))
        w = ode_trapezoid_weights(lam)
        assert w == ode_ref.trapezoid_weights(lam) and sum(w) == pytest.approx(lam[0] - lam[-1], rel=1e-12)
    g = torch.Generator().manual_seed(2)
    r = ode_ref.rademacher(torch.rand((3, 12), generator=g))
    gv = torch.randn((3, 12), generator=g, dtype=torch.float64)
    for mt in ("v", "eps", "x"):
        for lam in (20.0, 3.0, -0.5, -20.0):
            a, b = ode_divergence_coefs(lam, 12, mt)
            got = a + b * (r * gv).sum(1)
            ref = ode_ref.divergence(lam, r, gv, mt)
            assert torch.allclose(got, ref, rtol=1e-9, atol=1e-9 * 12), (mt, lam)


def test_draw_order_is_documented_and_replayable():
    """ode_nll draws from a fresh PhiloxStream(seed): the dequantisation u, then one probe per evaluation, each B D values."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, PhiloxStream
    B, D, N = 3, 5, 4                                  # B D = 15: not a multiple of 4, each draw reserves 4 counters
    rng = PhiloxStream(9)
    offs = [rng._take(B * D) for _ in range(N + 2)]
    assert GaussianDiffusion.ode_draw_counters(B, D, N) == offs == [4 * k for k in range(N + 2)]
    assert "u" in GaussianDiffusion.ode_nll.__doc__ and "ode_draw_counters" in GaussianDiffusion.ode_nll.__doc__


def test_flag_default_and_cli():
    from generative_models_amd import common, main
    Model = common.discover_models()["diffusion_model"]
    assert Model.DG.ode_nlogp_steps == 0 and isinstance(Model.DG.ode_nlogp_steps, int)
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--ode_nlogp_steps", "8"])
    assert G.ode_nlogp_steps == 8
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G.ode_nlogp_steps == 0


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(flags)
    return Model(G)


def test_model_flag_checks(tmp_path):
    assert _model(hidden_size=32).ode_nlogp_steps == 0
    with pytest.raises(ValueError, match="ode_nlogp_steps"):
        _model(hidden_size=32, ode_nlogp_steps=-1)
    path = tmp_path / "teacher.pt"
    torch.save(_model(hidden_size=32).state_dict(), path)
    with pytest.raises(ValueError, match="cond_w"):
        _model(hidden_size=32, teacher_path=path, ode_nlogp_steps=4)


def test_surface_refuses_bad_calls_before_any_device_work():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    net = SimpleUnet(32, 0.0)
    x = torch.zeros((2, 1, 8, 8))
    teach = GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=net, teacher_mode="step2")
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    calls = (lambda dd, n, **k: dd.encode(net=n, x=x, num_steps=k.get("N", 4)),
             lambda dd, n, **k: dd.decode(net=n, z=x, num_steps=k.get("N", 4)),
             lambda dd, n, **k: dd.ode_nll(net=n, x=k.get("x", x), num_steps=k.get("N", 4), delta=k.get("delta", 1 / 255)))
    for call in calls:
        with pytest.raises(ValueError, match="cond_w"):
            call(teach, net)
        with pytest.raises(ValueError, match="cond_w"):
            call(d, partial(net, cond_w=torch.ones(2)))
        for N in (0, -1, 1.5):
            with pytest.raises(ValueError, match="num_steps"):
                call(d, net, N=N)
    for delta in (0.0, -0.1, 0.75, float("nan")):
        with pytest.raises(ValueError, match="delta"):
            d.ode_nll(net=net, x=x, num_steps=4, delta=delta)
    for bad in (torch.zeros((2, 3, 8, 8)), torch.zeros((2, 64)), torch.zeros((0, 1, 8, 8))):
        with pytest.raises(ValueError, match="shape"):
            d.ode_nll(net=net, x=bad, num_steps=4)
        with pytest.raises(ValueError, match="shape"):
            d.encode(net=net, x=bad, num_steps=4)


def test_wrappers_reject_bad_arguments():
    from generative_models_amd import ops
    f = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt)
    x, v = f(3, 1, 5, 5), f(3)
    for mt in ("both", "V", None):
        with pytest.raises(ValueError, match="mean_type"):
            ops.pf_ode_step(x, x, 1.0, mean_type=mt)
    with pytest.raises(ValueError, match="probe"):
        ops.pf_ode_step(x, x, 1.0, acc=v, r=x)
    with pytest.raises(ValueError, match="prior"):
        ops.pf_ode_step(x, x, 1.0, 0.5, prior=v)
    with pytest.raises(ValueError, match="non-finite"):
        ops.pf_ode_step(x, x, float("nan"))
    with pytest.raises(ValueError, match="dtype"):
        ops.pf_ode_step(x, x.double(), 1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.pf_ode_step(x, f(3, 1, 5, 4), 1.0)
    with pytest.raises(ValueError, match="shape"):
        ops.pf_ode_step(x, x, 1.0, r=x, g=x, acc=f(2))
    with pytest.raises(ValueError, match="device tensor"):
        ops.pf_ode_step(x, x, 1.0, 0.5)
    for delta in (0.0, -1.0, 0.75, float("nan")):
        with pytest.raises(ValueError, match="delta"):
            ops.dequantize(x, delta, 0, 0)
    with pytest.raises(ValueError, match="dtype"):
        ops.dequantize(x.double(), 0.5, 0, 0)
    with pytest.raises(ValueError, match="device tensor"):
        ops.dequantize(x, 0.5, 0, 0)
    with pytest.raises(ValueError, match="shape"):
        ops.stem_dgrad(f(2, 4, 4, 128), f(128, 1, 2, 2))
    with pytest.raises(ValueError, match="shape"):
        ops.stem_dgrad(f(2, 4, 4, 128), f(256, 1, 3, 3))


def test_header_declares_the_entries():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L, U = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    assert protos["gmk_stem_dgrad"][1:] == ([P, P, P] + [I] * 6 + [P], ["dy", "w", "dx", "B", "cin", "H", "W", "C", "dtype", "stream"])
    assert protos["gmk_rng_rademacher"][1:] == ([P, L, U, U, P], ["out", "n", "seed", "offset", "stream"])
    assert protos["gmk_dequantize"][1:] == ([P, P, F, L, U, U, P], ["x", "y", "delta", "n", "seed", "offset", "stream"])
    assert protos["gmk_pf_ode_step"][1] == [P] * 7 + [F, F, I, F, F, F, I, I, L, P]
    assert all(protos[k][0] is ctypes.c_int for k in ("gmk_stem_dgrad", "gmk_rng_rademacher", "gmk_dequantize", "gmk_pf_ode_step"))


def test_entries_reject_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first
    step = lambda out=buf, acc=None, r=None, g=None, prior=None, upd=0, mt=0, B=2, n=64, li=1.0: lib.gmk_pf_ode_step(
        out, buf, r, g, acc, prior, None, li, 0.0, upd, 0.0, 0.0, 0.0, mt, B, n, None)
    assert step(out=None) == -1 and b"null pointer" in lib.gmk_last_error()
    for mt in (-1, 3):
        assert step(mt=mt) == -1 and b"mean_type" in lib.gmk_last_error()
    for B, n in ((0, 64), (70000, 64), (2, 0)):
        assert step(B=B, n=n) == -1 and b"shape" in lib.gmk_last_error()
    assert step(acc=buf, r=buf) == -1 and b"probe" in lib.gmk_last_error()
    assert step(prior=buf, upd=1) == -1 and b"prior" in lib.gmk_last_error()
    assert step(li=float("inf")) == -1 and b"non-finite" in lib.gmk_last_error()
    assert lib.gmk_rng_rademacher(None, 8, 0, 0, None) == -1
    assert lib.gmk_dequantize(buf, buf, 0.0, 8, 0, 0, None) == -1 and b"delta" in lib.gmk_last_error()
    assert lib.gmk_dequantize(None, buf, 0.5, 8, 0, 0, None) == -1
    assert lib.gmk_stem_dgrad(None, buf, buf, 2, 1, 8, 8, 128, 0, None) == -1 and b"null pointer" in lib.gmk_last_error()
    assert lib.gmk_stem_dgrad(buf, buf, buf, 2, 5, 8, 8, 128, 0, None) == -1 and b"shape" in lib.gmk_last_error()
    assert lib.gmk_stem_dgrad(buf, buf, buf, 2, 1, 8, 8, 96, 0, None) == -1 and b"shape" in lib.gmk_last_error()
