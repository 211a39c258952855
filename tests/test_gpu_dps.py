"""GPU tests of diffusion posterior sampling (DPS: Chung et al. 2023; `GaussianDiffusion.posterior_sample`, gmk_gauss_blur,
gmk_dps_backproject, gmk_dps_correct, `DiffusionModel.measure` / `posterior_sample`, DG.dps_eval; an extension): the operator and the two step
kernels against float64 and against the fp32 statement of their arithmetic, the assembled gradient through the HIP network against CPU autograd
through the oracle, whole chains against the CPU restatement (tests/dps_ref.py), zeta = 0 against `sample`, the plugin surface, and the
restoration of a learnt image from a noisy observation."""
import math
import os
import random
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dps_ref as P  # noqa: E402
import inpaint_ref  # noqa: E402
from test_gpu_ode import _cos_l2, _rel  # noqa: E402
from test_gpu_restore import _Frames, _close, _model, make_net, rel_err  # noqa: E402

U24 = 2.0 ** -24
SHAPES = [(1, 8, 8), (3, 8, 8), (1, 12, 12), (1, 28, 28), (3, 32, 32), (3, 64, 64)]
B = 3
TIMES = ((-20.0, -12.0), (1.0, 2.5))


def _op(spec):
    """tests/dps_ref.py's operator tuple -> the package's MeasurementOp"""
    from generative_models_amd.diffusion.gaussian_diffusion import MeasurementOp, blur_taps
    return MeasurementOp("box", spec[1], spec[2], 0.0, ()) if spec[0] == "box" else MeasurementOp("blur", 1, 1, spec[1], blur_taps(spec[1]))


def _operators(C, H, W):
    """The three blurs, a box mean (N = 3 at 12 x 12, 7 at 28 x 28, else 2) and, at three channels, its gray form and the channel mean alone"""
    N = 3 if H % 3 == 0 else 7 if H % 7 == 0 else 2
    return [("blur", s) for s in P.BLUR_SIGMAS] + [("box", 1, N)] + ([("box", C, N), ("box", C, 1)] if C > 1 else [])


def _blur_units(sigma):
    """Roundings on the path of one blurred value per unit of the largest input: per pass 2 R + 1 sequential additions, each relative to a
    partial sum no larger than the input's largest value (the taps sum to 1), and one unit for the rounded products (they sum to that too)."""
    return 2 * (2 * P.radius(sigma) + 1) + 2


def _rnd(shape, seed, uniform=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.rand(shape, device="cuda", generator=g) * 2 - 1 if uniform else torch.randn(shape, device="cuda", generator=g)


# ---- G1: the operator ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", P.BLUR_SIGMAS)
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_gauss_blur_against_float64(C, H, W, sigma):
    """Values in [-1, 1]: each output is two passes of at most 2 R + 1 sequential fp32 additions of rounded products whose magnitudes sum to at
    most 1, so the error stays within (2 (2 R + 1) + 2) 2^-24 (`_blur_units`).  The stated operation order bit for bit (numpy fp32), the same
    bits on a second call, and the adjoint identity <A x, y> = <x, A y> on the device outputs within that bound times |x|_1 + |y|_1."""
    from generative_models_amd import ops
    op = _op(("blur", sigma))
    x, y = _rnd((B, C, H, W), 5 + H, True), _rnd((B, C, H, W), 6 + H, True)
    ax = ops.gauss_blur(x, op.taps)
    bound = _blur_units(sigma) * U24
    err = float((ax.double().cpu() - P.A(x.double().cpu(), ("blur", sigma))).abs().max())
    print(f"gauss_blur {C}x{H}x{W} sigma {sigma}: err {err:.3e}, bound {bound:.3e}")
    assert ax.shape == x.shape and ax.dtype == torch.float32 and err <= bound
    assert torch.equal(ax.cpu(), torch.from_numpy(P.blur_fp32(x, sigma)))
    assert torch.equal(ax, ops.gauss_blur(x, op.taps)) and torch.equal(ax, ops.measure(x, op))
    ay = ops.gauss_blur(y, op.taps)
    lhs, rhs = float((ax.double() * y.double()).sum()), float((x.double() * ay.double()).sum())
    assert abs(lhs - rhs) <= bound * float(x.double().abs().sum() + y.double().abs().sum()), (lhs, rhs)


# ---- G2: gmk_dps_backproject ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_backproject_against_float64(C, H, W):
    """u = A^T (obs - A x_hat) and |e_b|^2 from the same fp32 (v, z, obs), mean types 'v' and 'x' at both times, 'eps' mid-chain.  With
    M = max(|c_z z| + |c_o out|) + max |obs| (the largest x_hat's terms and the observation), one unit = 2^-24 M:
      x_hat   8 units (the fp32 coefficients of logsnr_coef, two products, one sum);
      blur    A x_hat adds `_blur_units`, e = fsub(obs, .) one, u = A e `_blur_units` again:  u within (2 units_blur + 9) units;
      box     the sequential mean of k members k + 1, e one, u = fdiv(e, k) one:               u within (k + 11) units.
    |e_b|^2 (the tree order: per thread the sequential sum of its m elements' squares, then a 256-leaf binary tree, 8 levels): within
    (m + 9) 2^-24 |e_b|^2 + 2 |e_b|_1 de + n_e de^2, de the bound of e.  Then the kernel's own arithmetic bit for bit on the unclipped x_hat
    gmk_pf_ode_step returns (the same device function) - the blur inside the kernel is gmk_gauss_blur's - and a second call's bits."""
    from generative_models_amd import ops
    v, z, x0 = _rnd((B, C, H, W), 11 + H), _rnd((B, C, H, W), 12 + H), _rnd((B, C, H, W), 13 + H, True)
    for spec in _operators(C, H, W):
        op = _op(spec)
        obs = ops.measure(x0, op)
        k = spec[1] * spec[2] ** 2 if spec[0] == "box" else 1
        for mean_type, times in (("v", TIMES), ("x", TIMES), ("eps", TIMES[1:])):
            for lt, _ in times:
                u, en2 = ops.dps_backproject(v, z, obs, lt, op, mean_type=mean_type)
                assert u.shape == z.shape and en2.shape == (B,) and u.dtype == en2.dtype == torch.float32
                c_z, c_o = P.coefs(lt, mean_type)
                M = float((abs(c_z) * z.abs() + abs(c_o) * v.abs()).max() + obs.abs().max())
                if spec[0] == "blur":
                    units_e, units_u = _blur_units(spec[1]) + 9, 2 * _blur_units(spec[1]) + 9
                    m = C * math.ceil(H * W / 256)
                else:
                    units_e, units_u = k + 10, k + 11
                    m = math.ceil(obs[0].numel() / 256)
                u64, en64 = P.backproject(v.cpu(), z.cpu(), obs.cpu(), lt, spec, mean_type)
                err = float((u.double().cpu() - u64).abs().max())
                e64 = obs.double().cpu() - P.A(P.x_hat(v.double().cpu(), z.double().cpu(), lt, mean_type), spec)
                de = units_e * U24 * M
                bound2 = (m + 9) * U24 * en64 + 2 * e64.abs().flatten(1).sum(1) * de + e64[0].numel() * de * de
                err2 = (en2.double().cpu() - en64).abs()
                print(f"backproject {C}x{H}x{W} {spec} {mean_type} lt {lt}: u {err:.3e} (bound {units_u * U24 * M:.3e}), "
                      f"|e|^2 {float((err2 / bound2).max()):.3f} of its bound")
                assert err <= units_u * U24 * M and bool((err2 <= bound2).all())
                # the kernel's own arithmetic on the unclipped x_hat of the same device function
                xh = torch.empty_like(z)
                ops.pf_ode_step(v, z.clone(), lt, mean_type=mean_type, x_out=xh)
                e = obs - ops.measure(xh, op)
                # (fdiv(e, k) in numpy: a device tensor divided by a scalar is multiplied by its reciprocal)
                want = ops.gauss_blur(e, op.taps) if spec[0] == "blur" else P.R.A_pinv(
                    torch.from_numpy(e.cpu().numpy() / np.float32(k)), spec[1], spec[2]).cuda()
                assert torch.equal(u, want), (spec, mean_type, lt)
                u2, en2b = ops.dps_backproject(v, z, obs, lt, op, mean_type=mean_type)
                assert torch.equal(u, u2) and torch.equal(en2, en2b)


# ---- G3: gmk_dps_correct --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W", SHAPES)
def test_correct_against_float64(C, H, W):
    """The bar of the update kernels (test_gpu_restore.py's `_close`); zeta = 0 leaves z's bits; |e| = 0 - obs = A x_hat exactly, through
    v = z = 0 and obs = 0 - gives a finite z."""
    from generative_models_amd import ops
    z, u, g = _rnd((B, C, H, W), 21 + H), _rnd((B, C, H, W), 22 + H), _rnd((B, C, H, W), 23 + H)
    en2 = torch.tensor([0.37, 41.0, 3e-9], device="cuda")
    for lt, zeta in ((-20.0, 1.0), (1.0, 0.3), (1.0, 25.0)):
        for mean_type in ("v", "x"):
            c_z, c_o = P.coefs(lt, mean_type)
            got = ops.dps_correct(z.clone(), u, g, en2, c_z, c_o, zeta)
            assert _close(got, P.correct(z, u, g, en2, c_z, c_o, zeta)), (lt, zeta, mean_type)
    zc = z.clone()
    zc[0, 0, 0, 0] = -0.0
    keep = zc.clone()
    assert ops.dps_correct(zc, u, g, en2, 0.5, -0.5, 0.0) is zc and torch.equal(zc.view(torch.int32), keep.view(torch.int32))
    zero = torch.zeros_like(z)
    op = _op(("blur", 1.5))
    u0, e0 = ops.dps_backproject(zero, zero, zero, 1.0, op)
    assert float(e0.abs().max()) == 0.0 and float(u0.abs().max()) == 0.0
    out = ops.dps_correct(z.clone(), u0, zero, e0, 0.7, -0.7, 1.0)
    assert bool(torch.isfinite(out).all()) and torch.equal(out, z)
    with pytest.raises(ValueError, match="zeta"):
        ops.dps_correct(z.clone(), u, g, en2, 1.0, 1.0, -1.0)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.dps_correct(z[:, :, :1, :3].contiguous(), u[:, :, :1, :3].contiguous(), g[:, :, :1, :3].contiguous(), en2, 1.0, 1.0, 1.0)


# ---- G4: the gradient through the HIP network ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("spec", [("box", 1, 2), ("blur", 1.0)], ids=["box2", "blur1"])
def test_gradient_through_the_network(spec, dtype):
    """c_z u + c_o g assembled from forward_hip + dps_backproject + input_vjp_hip against the CPU autograd of tests/dps_ref.py through the
    oracle (float64), 8 x 8, B = 3, hidden 128, at the bars of test_gpu_ode.py's input-gradient test: fp32 mode 1e-3 of the largest entry,
    16-bit mode cosine >= 0.9999 and relative L2 <= 1.5e-2."""
    from generative_models_amd import ops
    net, params = make_net(dtype, 1)
    p64 = P.cast_params(params, torch.float64)
    g = torch.Generator().manual_seed(17)
    z = torch.randn((B, 1, 8, 8), generator=g)
    obs = (P.A(torch.rand((B, 1, 8, 8), generator=g, dtype=torch.float64) * 2 - 1, spec)).float()
    y = torch.tensor([2, -1, 9])
    op = _op(spec)
    for lt in (-12.0, 1.0):
        store = {}
        with torch.no_grad():
            out = net.forward_hip(z.cuda(), torch.full((B,), lt, device="cuda"), y.cuda(), None, ctx=store)
            u, en2 = ops.dps_backproject(out, z.cuda(), obs.cuda(), lt, op)
            gv = net.input_vjp_hip(store, u)
        c_z, c_o = P.coefs(lt, "v")
        got = c_z * u + c_o * gv
        _, ref, s = P.guidance(p64, z.double(), lt, y, obs.double(), spec, "v")
        if dtype == torch.float32:
            print(f"gradient {spec} lt {lt}: {_rel(got, ref):.3e}")
            assert _rel(got, ref) <= 1e-3 and _rel(en2.sqrt(), s) <= 1e-3
        else:
            cos, l2 = _cos_l2(got, ref)
            print(f"gradient {spec} lt {lt} 16-bit: cosine {cos:.6f}, relative L2 {l2:.2e}")
            assert cos >= 0.9999 and l2 <= 1.5e-2, (cos, l2)


# ---- G5: chains against the restatement ---------------------------------------------------------------------------------------------------
_REF = {}


def _diffusion(sampler):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion(mean_type="v", num_steps=P.CHAIN_T, sampler=sampler, seed=P.CHAIN_SEED)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("kind", list(P.CHAIN_OPS))
@pytest.mark.parametrize("sampler", P.CHAIN_SAMPLERS)
def test_chain_vs_restatement(sampler, kind, dtype):
    """T = 4, B = 3, 8 x 8, hidden 128, zeta = 1, a noisy observation (tests/dps_ref.py's `chain_case`); the draws of 'noisy' and 'ancestral'
    at the documented Philox counters (evaluation f at f ceil(B n / 4) of the diffusion's stream).  Bars per step, on z and on the update's
    x-hat: the larger of the project's (fp32 mode 1e-3, 16-bit mode 3e-2) and 4 x the drift of the float32 restatement from the float64 one
    on these exact cases.  That drift, measured on the CPU (tests/test_host_dps.py prints it; profiles/dps_probe.txt): 3.7e-7 ... 6.4e-7 for
    the nine cases (|e| >= 0.74 throughout), so every bar is the project's own."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import measurement_op
    init, obs, y = P.chain_case(kind)
    C, spec = P.CHAIN_OPS[kind]
    net, params = make_net(dtype, C)
    d = _diffusion(sampler)
    op, low = measurement_op(kind, tuple(init.shape))
    assert low == tuple(obs.shape)
    key = (sampler, kind)
    if key not in _REF:
        noises = None
        if sampler != "ddim":
            noises = [ops.rng_normal(tuple(init.shape), d.rng.seed, c, "cuda").cpu() for c in P.chain_noise_counters(tuple(init.shape))]
        with torch.no_grad():
            _REF[key] = P.sample(params, init, obs, spec, y, P.CHAIN_T, sampler, P.CHAIN_ZETA, noises)
    zs_ref, xs_ref, _, s_ref = _REF[key]
    zs, xs, es = d.posterior_sample(net=partial(net, guide=y.cuda()), obs=obs.cuda(), op=op, init_x=init.cuda(), zeta=P.CHAIN_ZETA, record=True)
    assert zs.shape == zs_ref.shape == xs.shape == es.shape and float(xs.abs().max()) <= 1.0
    bar = P.chain_bar(P.CHAIN_DRIFT[key[::-1]], "fp32" if dtype == torch.float32 else "16-bit")
    errs = [(rel_err(zs[k], zs_ref[k]), rel_err(xs[k], xs_ref[k])) for k in range(P.CHAIN_T)]
    print(f"dps chain {sampler} {kind} {dtype}: {errs}, bar {bar}, |e| per step {s_ref.min(1).values.tolist()}")
    assert all(ez < bar and ex < bar for ez, ex in errs), errs
    assert not torch.equal(zs[-1], xs[-1])                                     # the last step is corrected too
    last = _diffusion(sampler).posterior_sample(net=partial(net, guide=y.cuda()), obs=obs.cuda(), op=op, init_x=init.cuda(), zeta=P.CHAIN_ZETA)
    assert last[1] is None and torch.equal(last[0][-1], zs[-1])


@pytest.mark.parametrize("sampler,eta", [("ddim", 0.0), ("noisy", 0.0), ("ancestral", 0.0), ("ddim", 0.5)])
def test_zeta_zero_is_sample(sampler, eta):
    """The loop itself changes no bit: zeta = 0 gives `sample` with the same sampler, seed and labels (and consumes the stream alike)."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, measurement_op
    init, obs, y = P.chain_case("box:2")
    net, _ = make_net(torch.bfloat16, 1)
    op, _ = measurement_op("box:2", tuple(init.shape))
    outs, counters = [], []
    for dps in (False, True):
        d = GaussianDiffusion(mean_type="v", num_steps=P.CHAIN_T, sampler=sampler, seed=P.CHAIN_SEED, ddim_eta=eta)
        kw = dict(net=partial(net, guide=y.cuda()), init_x=init.cuda(), record=True)
        outs.append(d.posterior_sample(obs=obs.cuda(), op=op, zeta=0.0, **kw) if dps else d.sample(**kw))
        counters.append(d.rng.counter)
    for a, b_ in zip(*outs):
        assert torch.equal(a, b_)
    assert counters[0] == counters[1]


# ---- G6: what it is for -------------------------------------------------------------------------------------------------------------------
def test_restores_the_right_image_from_a_noisy_observation():
    """Trained on two images only, the net returns from measure(x_k, 'box:4', noise_std = 0.1) an image nearer to x_k than to the other one.
    tools/dps_probe.py measured the hit rate p over 512 draws (profiles/dps_probe.txt): 0.998.  The bar sits three binomial standard
    deviations sqrt(p (1 - p) / 64), at this test's 64 draws, below p: 0.998 - 3 x 0.0056 = 0.981.  On the same draws the mean |obs - A result| lies
    strictly below that of zeta = 0, and the unguided chain still draws both images.  The seeds are fixed."""
    model = inpaint_ref.train_two_mode(_model)
    right, s_dps, s_free, uncond = P.posterior_accuracy(model)
    print(f"dps: right image {right:.3f}, mean |e| {s_dps:.4f} (zeta = 0: {s_free:.4f}), unguided nearer mode 0 {uncond:.3f}")
    p = 0.998
    assert right >= p - 3.0 * math.sqrt(p * (1.0 - p) / 64), (right, uncond)
    assert s_dps < s_free, (s_dps, s_free)
    assert 0.2 <= uncond <= 0.8, uncond


# ---- G7: the plugin -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,kind", [({}, "box:7"), ({"in_channels": 3, "image_size": 8}, "gray_box:2"), ({"in_channels": 3, "image_size": 8}, "blur:1.5")])
def test_plugin_measure_and_posterior_sample(flags, kind):
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, PhiloxStream, measurement_op
    model = _model(ema_decay=0.999, **flags)
    model.eval()
    C, S = model.net.in_channels, model.size
    x = torch.rand(5, C, S, S, device="cuda") * 2 - 1
    y = torch.randint(0, 10, (5,), device="cuda")
    op, low = measurement_op(kind, tuple(x.shape))
    clean = model.measure(x, kind)
    assert clean.shape == low and torch.equal(clean, ops.measure(x, op))
    if op.kind == "box":
        assert torch.equal(clean, model.degrade(x, factor=op.N, gray=op.cf > 1))
    obs = model.measure(x, kind, noise_std=0.05, seed=4)
    assert torch.equal(obs, clean + 0.05 * ops.rng_normal(low, 4, 0, "cuda"))
    out = model.posterior_sample(obs, kind, y=y, seed=3, zeta=0.5)
    assert out.shape == x.shape and bool(torch.isfinite(out).all())
    # the EMA net, the initial noise from PhiloxStream(seed), labels without guidance
    assert model.optimizer.ema_seeded
    d = GaussianDiffusion(mean_type="v", num_steps=6, sample_cond_w=-1.0)
    ref = d.posterior_sample(net=partial(model.ema_net, guide=y), obs=obs, op=op, init_x=PhiloxStream(3).normal(tuple(x.shape), "cuda"), zeta=0.5)
    assert torch.equal(out, ref[0][-1])
    assert torch.equal(model.posterior_sample(obs, kind, y=y, seed=3), d.posterior_sample(
        net=partial(model.ema_net, guide=y), obs=obs, op=op, init_x=PhiloxStream(3).normal(tuple(x.shape), "cuda"), zeta=model.dps_zeta)[0][-1])


@pytest.mark.parametrize("flags,on", [({}, {"dps_eval": "box:2"}), ({"in_channels": 3, "image_size": 8}, {"dps_eval": "gray_box:2", "dps_noise": 0.0}),
                                      ({"in_channels": 3, "image_size": 8}, {"dps_eval": "blur:1.5", "dps_zeta": 0.5, "sampler": "ancestral"})])
def test_evaluate_dps_eval(flags, on):
    """test_gpu_restore.py::test_evaluate_restore_eval's pattern: with dps_eval everything evaluate() made before is bit-equal, the host RNG is
    consumed alike, and the new keys and frames are there with their shapes and definitions."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import measurement_op
    C, S = flags.get("in_channels", 1), flags.get("image_size", 28)
    x = torch.rand(8, C, S, S, device="cuda") * 2 - 1
    y = torch.randint(0, 10, (8,), device="cuda")
    base = {k: v for k, v in on.items() if k == "sampler"}
    evs, writers, host = [], [], []
    for extra in (base, on):
        torch.manual_seed(0)                                                    # the same initial weights
        model = _model(**flags, **extra)
        model.eval()
        random.seed(5)
        writers.append(_Frames())
        model.evaluate(writers[-1], x, y.clone(), 0)
        host.append(random.random())
        evs.append(model.last_eval)
    off, on_ = evs
    assert not any(k.startswith("dps") for k in off) and not any(k.startswith("dps") for k in writers[0].frames)
    assert host[0] == host[1]
    for k in ("samples", "sampling_process", "eps", "x"):
        assert torch.equal(off[k], on_[k]), k
    for k in writers[0].frames:
        assert torch.equal(writers[0].frames[k], writers[1].frames[k]), k
    assert on_["dps"].dtype == torch.uint8 and on_["dps"].shape == (8, C, S, S)
    z, z_in = writers[1].frames["dps"], writers[1].frames["dps_input"]
    assert z.shape == z_in.shape == x.shape
    op, low = measurement_op(on["dps_eval"], tuple(x.shape))
    obs = model.measure(x, on["dps_eval"], noise_std=model.dps_noise, seed=model.DPS_EVAL_SEED + 1)
    want_in = obs if op.kind == "blur" else P.R.A_pinv(obs, op.cf, op.N)
    assert torch.equal(z_in, want_in)
    psnr = lambda t: 10.0 * torch.log10(4.0 / (t.double() - x.double()).square().mean(dim=(1, 2, 3)))
    for key, t in (("dps_psnr", z), ("dps_input_psnr", z_in)):
        assert on_[key].shape == (8,) and torch.allclose(on_[key].double(), psnr(t).cpu(), rtol=1e-6, atol=0)
    resid = float(((obs - ops.measure(z, op)).double().flatten(1).norm(dim=1) / math.sqrt(math.prod(low[1:]))).mean())
    assert on_["dps_residual"] == pytest.approx(resid, rel=1e-6) and math.isfinite(resid)
