"""GPU tests of DDNM restoration (Wang, Yu & Zhang 2023; `GaussianDiffusion.restore`, gmk_box_mean, gmk_box_residual, gmk_sampler_step_ns,
gmk_dpm_solver_step_ns, `DiffusionModel.degrade` / `restore`, DG.restore_eval / DG.restore_gray; an extension): the box kernels against
float64 and the fp32 statement of their arithmetic, the _ns update kernels against the plain entries (r = 0, bit for bit) and a float64
restatement (random r), whole chains against the CPU restatement (tests/restore_ref.py) and the consistency A(result) = obs they exist for, on
the paths of the sampler loop - kernel by kernel, the captured-graph forward, two half-batch streams, the guided 2B batch - the plugin
surface, and the restoration of a learnt image."""
import math
import os
import random
import sys
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref  # noqa: E402
import restore_ref as R  # noqa: E402

U24 = 2.0 ** -24
# (C, H, W, cf, N): n under one workgroup; colourisation only; both degradations; a box side that is no power of two; 28 x 28 with N = 7;
# 768 boxes (more than one workgroup of the box kernels); a large spatial box
SHAPES = [(1, 8, 8, 1, 2), (3, 8, 8, 3, 1), (3, 8, 8, 3, 2), (1, 12, 12, 1, 3), (1, 28, 28, 1, 7), (3, 32, 32, 1, 2), (3, 32, 32, 1, 8)]
B = 3
MEAN_TYPES = ("v", "eps", "x")
# (logsnr_t, logsnr_s) of the kernel tests: the chain's first network time, -20, where x-hat's formulas cancel hardest, and a mid-chain pair
TIMES = ((-20.0, -12.0), (1.0, 2.5))
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def _ulp_err(a, b):
    """max |a - b| in units of b's fp32 spacing"""
    a, b = a.double(), b.double()
    spacing = torch.finfo(torch.float32).eps * torch.clamp(b.abs(), min=torch.finfo(torch.float32).tiny)
    return float(((a - b).abs() / spacing).max())


def _close(out, want):
    """The bar of test_gpu_inpaint.py::test_merge_kernel_against_torch: 4 fp32 spacings element by element, or 1e-6 of the largest value."""
    u, r = _ulp_err(out, want.to(out.device)), rel_err(out, want)
    print(f"      ulp {u:.2f} rel {r:.2e}")
    return u <= 4.0 or r < 1e-6


def _case(C, H, W, cf, N, guided, seed=3):
    from generative_models_amd import ops
    g = torch.Generator(device="cuda").manual_seed(seed + 7 * C + H + N)
    rnd = lambda: torch.randn((B, C, H, W), device="cuda", generator=g)
    v, z = rnd(), rnd()
    vu = rnd() if guided else None
    w = torch.tensor([0.5, 2.0, 3.1], device="cuda") if guided else None
    x0 = torch.rand((B, C, H, W), device="cuda", generator=g) * 2 - 1
    obs = ops.box_mean(x0, cf, N)
    return v, z, vu, w, x0, obs


# ---- G1: the box kernels -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,H,W,cf,N", SHAPES)
def test_box_mean_against_float64(C, H, W, cf, N):
    from generative_models_amd import ops
    k = cf * N * N
    _, _, _, _, x0, obs = _case(C, H, W, cf, N, False)
    assert obs.shape == (B, C // cf, H // N, W // N) and obs.dtype == torch.float32
    err = float((obs.double() - R.A(x0.double(), cf, N)).abs().max())
    print(f"box_mean k = {k}: err {err:.3e}, bound {(k + 1) * U24:.3e}")
    assert err <= (k + 1) * U24
    # the stated arithmetic, bit for bit, and the same bits on a second call
    assert torch.equal(obs.cpu(), torch.from_numpy(R.box_mean_fp32(x0, cf, N)))
    assert torch.equal(obs, ops.box_mean(x0, cf, N))


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C,H,W,cf,N", SHAPES)
def test_box_residual_against_float64(C, H, W, cf, N, guided):
    """r = obs - A x-hat on the x-hat gmk_sampler_step itself forms (its x_pred output: the same device function, so the same bits): the
    members of the sum lie in [-1, 1], which is what the bound (k + 1) 2^-24 rests on."""
    from generative_models_amd import ops
    k = cf * N * N
    v, z, vu, w, _, obs = _case(C, H, W, cf, N, guided)
    for mean_type in MEAN_TYPES:
        for lt, ls in TIMES:
            _, xh, _ = ops.sampler_step(v, z, lt, ls, False, v_uncond=vu, cond_w=w, want_pred=True, mean_type=mean_type)
            assert float(xh.abs().max()) <= 1.0
            r = ops.box_residual(v, z, obs, lt, cf, N, v_uncond=vu, cond_w=w, mean_type=mean_type)
            assert r.shape == obs.shape
            err = float((r.double() - R.residual(xh, obs, cf, N)).abs().max())
            print(f"box_residual {mean_type} lt = {lt} k = {k}: err {err:.3e}, bound {(k + 1) * U24:.3e}")
            assert err <= (k + 1) * U24
            want = obs.cpu().numpy() - R.box_mean_fp32(xh, cf, N)             # fsub(obs, fdiv(s, k)) in numpy fp32
            assert torch.equal(r.cpu(), torch.from_numpy(want))
            assert torch.equal(r, ops.box_residual(v, z, obs, lt, cf, N, v_uncond=vu, cond_w=w, mean_type=mean_type))
    # x-hat itself is the restatement's: checked where fp32 forms it without cancellation (mid-chain, unguided or guided alike)
    lt = TIMES[1][0]
    _, xh, _ = ops.sampler_step(v, z, lt, TIMES[1][1], False, v_uncond=vu, cond_w=w, want_pred=True)
    ref = R.x_hat(v.cpu(), z.cpu(), torch.full((B,), lt), "v", None if vu is None else vu.cpu(), None if w is None else w.cpu())
    assert float((xh.cpu().double() - ref).abs().max()) <= 1e-5


# ---- G2: the _ns update kernels ----------------------------------------------------------------------------------------------------------
def _dpm_coefs(lt, ls):
    """coef_z, coef_x of gmk_dpm_solver_step for one (logsnr_t, logsnr_s), in double (`dpm_solver_coefs`' formulas)."""
    sigma = lambda l: math.sqrt(1.0 / (1.0 + math.exp(l)))
    alpha = lambda l: math.sqrt(1.0 / (1.0 + math.exp(-l)))
    h = 0.5 * (ls - lt)
    return sigma(ls) / sigma(lt), -alpha(ls) * math.expm1(-h)


def _steps(v, z, vu, w, noise, hist, lt, ls, mean_type, is_last, dup, ns):
    """Every update the loop can launch, with or without `ns`: -> {name: (z_next, z_dup, x_pred, eps_pred, x_hist, logsnr_next)}"""
    from generative_models_amd import ops
    out = {}
    n_l = 2 * B if dup else B
    cz, cx = _dpm_coefs(lt, ls)
    for name in ("ddim", "noisy", "dpm1", "dpm2"):
        ln = torch.full((n_l,), float("nan"), device="cuda")
        kw = dict(v_uncond=vu, cond_w=w, want_pred=True, mean_type=mean_type, dup=dup, logsnr_next=ln, ns=ns)
        h = hist.clone()
        if name in ("ddim", "noisy"):
            zn, xp, ep = ops.sampler_step(v, z, lt, ls, is_last, noise=noise if name == "noisy" else None, **kw)
        else:
            zn, xp, ep = ops.dpm_solver_step(v, z, h, lt, ls, cz, cx, 0.0 if name == "dpm1" else 0.5, is_last, **kw)
        zn, z2 = zn if dup else (zn, None)
        out[name] = (zn, None if z2 is None else z2[B:], xp, ep, h, ln)
    return out


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C,H,W,cf,N", SHAPES)
def test_ns_steps_with_zero_residual_are_the_plain_entries(C, H, W, cf, N, guided):
    v, z, vu, w, _, obs = _case(C, H, W, cf, N, guided)
    g = torch.Generator(device="cuda").manual_seed(1)
    noise = torch.randn(z.shape, device="cuda", generator=g)
    hist = torch.rand(z.shape, device="cuda", generator=g) * 2 - 1
    zero = torch.zeros_like(obs)
    for mean_type in MEAN_TYPES:
        for (lt, ls), is_last, dup in ((TIMES[0], False, guided), (TIMES[1], False, False), (TIMES[1], True, guided)):
            plain = _steps(v, z, vu, w, noise, hist, lt, ls, mean_type, is_last, dup, None)
            ns = _steps(v, z, vu, w, noise, hist, lt, ls, mean_type, is_last, dup, (zero, cf, N))
            for name in plain:
                for a, b_ in zip(plain[name], ns[name]):
                    assert (a is None and b_ is None) or torch.equal(a, b_), (name, mean_type, lt, is_last, dup)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("C,H,W,cf,N", SHAPES)
def test_ns_steps_with_a_random_residual_against_float64(C, H, W, cf, N, guided):
    """x-hat' = fadd(x-hat, r[box]) on the plain entries' own x-hat (one rounding: the fp32 sum's bits), then eps-hat' and each update in
    float64 from x-hat'.  Nothing is clipped again: r in [-2, 2] takes x-hat' out to +-3."""
    v, z, vu, w, _, obs = _case(C, H, W, cf, N, guided)
    g = torch.Generator(device="cuda").manual_seed(2)
    noise = torch.randn(z.shape, device="cuda", generator=g)
    hist = torch.rand(z.shape, device="cuda", generator=g) * 2 - 1
    r = torch.rand(obs.shape, device="cuda", generator=g) * 4 - 2
    for mean_type in MEAN_TYPES:
        for (lt, ls), is_last, dup in ((TIMES[0], False, guided), (TIMES[1], False, False), (TIMES[1], True, guided)):
            plain = _steps(v, z, vu, w, noise, hist, lt, ls, mean_type, is_last, dup, None)
            ns = _steps(v, z, vu, w, noise, hist, lt, ls, mean_type, is_last, dup, (r, cf, N))
            xh = plain["ddim"][2]
            xp32 = xh + R.A_pinv(r, cf, N)
            assert float(xp32.abs().max()) > 1.0
            xp, ep = R.projected(xh, r, z, torch.full((B,), lt, device="cuda"), cf, N)
            cz, cx = _dpm_coefs(lt, ls)
            want = {"ddim": R.ddim_update(xp, ep, ls), "noisy": R.ancestral_update(xp, z, noise, lt, ls), "dpm1": cz * z.double() + cx * xp,
                    "dpm2": cz * z.double() + cx * (1.5 * xp - 0.5 * hist.double())}
            for name, (zn, z2, x_pred, eps_pred, h, ln) in ns.items():
                print(f"   {name} {mean_type} lt = {lt} is_last = {is_last}")
                assert torch.equal(x_pred, xp32), name
                assert _close(eps_pred, ep), name
                assert _close(zn, xp if is_last else want[name]), name
                if dup:
                    assert torch.equal(z2, zn)
                if name.startswith("dpm"):
                    assert torch.equal(h, x_pred)                              # the history holds x-hat', what the next step extrapolates from
                assert torch.equal(ln.cpu(), torch.full(ln.shape, ls, dtype=torch.float32))


def test_ns_and_thr_do_not_combine():
    from generative_models_amd import ops
    v, z, _, _, _, obs = _case(1, 8, 8, 1, 2, False)
    thr = torch.ones((B,), device="cuda")
    with pytest.raises(ValueError, match="not supported"):
        ops.sampler_step(v, z, -1.0, 1.0, False, thr=thr, ns=(obs, 1, 2))
    with pytest.raises(ValueError, match="not supported"):
        ops.dpm_solver_step(v, z, z.clone(), -1.0, 1.0, 0.5, 0.5, 0.0, False, thr=thr, ns=(obs, 1, 2))
    with pytest.raises(ValueError, match="ns residual"):
        ops.sampler_step(v, z, -1.0, 1.0, False, ns=(obs[:, :, :2], 1, 2))


# ---- G3: chains against the CPU restatement, and the consistency they exist for ----------------------------------------------------------
_NETS = {}


def make_net(dtype, in_channels=1, C=128, seed=0):
    """test_gpu_inpaint.make_net (default-init scale, the zero-initialised out_layers.3 convs made live), at 1 or 3 image channels."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    key = (dtype, in_channels, C, seed)
    if key not in _NETS:
        net = SimpleUnet(C, 0.0, in_channels=in_channels, compute_dtype=dtype)
        params = U.reference_init_params(C, in_channels, seed=seed, zero_out_layers=False)
        net.load_state_dict(params, strict=True)
        _NETS[key] = (net.cuda().eval(), params)
    return _NETS[key]


# (image channels, gray, N): super-resolution at 1 channel, colourisation + super-resolution at 3
OPERATORS = {"sr2": (1, False, 2), "gray_sr2": (3, True, 2)}


def _chain_case(op, Bn=3, S=8, seed=11):
    from generative_models_amd import ops
    C, gray, N = OPERATORS[op]
    g = torch.Generator().manual_seed(seed)
    init = torch.randn((Bn, C, S, S), generator=g).cuda()
    x0 = (torch.rand((Bn, C, S, S), generator=g) * 2 - 1).cuda()
    y = torch.tensor([1, 7, 3, 5, 2, 8][:Bn]).cuda()
    cf = C if gray else 1
    return init, ops.box_mean(x0, cf, N), y, cf, N, gray


def _draws(d, Bn, shape, T, guided):
    """The draws `restore` makes from d.rng: net_cond_w (guided), then one 'noisy' noise per network evaluation - at the counters the package
    documents, drawn with ops.rng_normal / ops.rng_uniform."""
    from generative_models_amd import ops
    n = Bn * math.prod(shape)
    c0, w = 0, None
    if guided:
        w = 4.0 * ops.rng_uniform((Bn,), d.rng.seed, 0, "cuda")
        c0 = (Bn + 3) // 4
    noises = [ops.rng_normal((Bn,) + shape, d.rng.seed, c0 + f * n // 4, "cuda").cpu() for f in range(T)]
    return (None if w is None else w.cpu()), noises


def _consistency(result, obs, cf, N):
    """max |float64 A(result) - obs| and its bound (k + 4) 2^-24"""
    err = float((R.A(result.double(), cf, N) - obs.double()).abs().max())
    return err, (cf * N * N + 4) * U24


_REF = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("op", list(OPERATORS))
@pytest.mark.parametrize("sampler", ["ddim", "noisy", "dpmpp_2m"])
def test_chain_vs_restatement(sampler, op, guided, dtype):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    Bn, S, T = 3, 8, 4
    init, obs, y, cf, N, gray = _chain_case(op, Bn, S)
    net, params = make_net(dtype, init.shape[1])
    d = GaussianDiffusion(mean_type="v", num_steps=T, sampler=sampler, sample_cond_w=-1.0, seed=9)
    assert not d._graph_path(net, 2 * Bn if guided else Bn, S, S)            # T < 16: kernel by kernel
    key = (sampler, op, guided)
    if key not in _REF:
        w, noises = _draws(d, Bn, tuple(init.shape[1:]), T, guided)
        with torch.no_grad():
            _REF[key] = R.sample(params, init.cpu(), obs.cpu(), cf, N, y.cpu(), T, sampler, cond_w=w, noises=noises)
    zs_ref, xs_ref, es_ref = _REF[key]
    zs, xs, es = d.restore(net=partial(net, guide=y), obs=obs, factor=N, gray=gray, init_x=init, cond_w=0.5 if guided else None, record=True)
    assert zs.shape == zs_ref.shape == xs.shape == es.shape
    # the consistency the feature exists for: the result, and every step's x-hat', agree with the observation
    err, bound = _consistency(zs[-1], obs, cf, N)
    errs_x = [_consistency(xs[k], obs, cf, N)[0] for k in range(T)]
    print(f"consistency {sampler} {op} guided = {guided} {dtype}: {err:.3e} (steps {max(errs_x):.3e}), bound {bound:.3e}")
    assert err <= bound and max(errs_x) <= bound
    assert float(xs.abs().max()) <= 3.0
    # the bars of test_gpu_inpaint.py::test_chain_vs_restatement, per step: fp32 1e-3 (5e-3 guided), 16-bit mode 3e-2
    tol = (5 if guided else 1) * TOL[dtype] if dtype == torch.float32 else 3 * TOL[dtype]
    errs = [(rel_err(zs[k], zs_ref[k]), rel_err(xs[k], xs_ref[k])) for k in range(T)]
    tols = [(tol, tol) for _ in range(T)]
    if guided and dtype != torch.float32:
        # The one exception that test holds, for its written reason: the first step's x-hat in 16-bit mode, guided.  At logsnr_t = -20,
        # x_hat = clip((z - sigma_t eps_w) / alpha_t) multiplies the guided eps_w = (1 + w) eps - w eps_u, and with it the 16-bit forward's
        # error, by (1 + 2 w) / alpha_t, 9 e^10 ~ 2e5 at the drawn w ~ 4; pixels inside the clip band then differ by up to 4.2e-2 of the largest
        # there (measured) and 3.3e-2 here (1 channel; 1.8e-2 at 3), against that test's 6e-2.  That x-hat is sample()'s own, bit for bit
        # (the same net, noise and weights), and the projection moves it along the range space only: the null-space part x - A+ A x of
        # xs[0] is sample()'s, up to the one rounding of x-hat' = fadd(x-hat, r) (|x-hat'| < 4: 2^-23 per element, twice that after A+ A).
        # Every later step and every z is held to the bar.
        tols[0] = (tol, 6e-2)
        ref_first = GaussianDiffusion(mean_type="v", num_steps=T, sampler=sampler, sample_cond_w=-1.0, seed=9).sample(
            net=partial(net, guide=y), init_x=init, cond_w=0.5)[1][0]
        null = lambda t: t.double() - R.A_pinv(R.A(t.double(), cf, N), cf, N)
        assert float((null(xs[0]) - null(ref_first)).abs().max()) <= 4 * U24
    print(f"chain {sampler} {op} guided = {guided} {dtype}: {errs}, bar {tol}")
    assert all(ez < tz and ex < tx for (ez, ex), (tz, tx) in zip(errs, tols)), errs


def test_graph_path_vs_restatement():
    """T = 16 at 8 x 8: the forward replays a captured graph."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    Bn, S, T = 3, 8, 16
    init, obs, y, cf, N, gray = _chain_case("sr2", Bn, S)
    net, params = make_net(torch.float32)
    d = GaussianDiffusion(mean_type="v", num_steps=T, sampler="ddim")
    assert d._graph_path(net, Bn, S, S)
    zs, xs, _ = d.restore(net=partial(net, guide=y), obs=obs, factor=N, init_x=init, record=True)
    assert len(d._graphs) == 1
    with torch.no_grad():
        zs_ref, xs_ref, _ = R.sample(params, init.cpu(), obs.cpu(), cf, N, y.cpu(), T, "ddim")
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    print(f"graph path: {ez:.3e} {ex:.3e}")
    assert ez < 1e-3 and ex < 1e-3, (ez, ex)
    err, bound = _consistency(zs[-1], obs, cf, N)
    assert err <= bound
    last = d.restore(net=partial(net, guide=y), obs=obs, factor=N, init_x=init)[0][-1]
    assert torch.equal(last, zs[-1])


# ---- G4: two streams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,cond_w", [("ddim", 0.5), ("noisy", None), ("dpmpp_2m", None)])
def test_two_streams_are_bit_identical(sampler, cond_w):
    """A batch above STREAM_MIN_PIXELS at hidden 128 runs as two half-batches on two streams, each with its rows of obs: every recorded
    tensor must be the same bits as on one stream (the residual and the projection are per image)."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    Bn, S, N = 8192, 8, 2
    torch.manual_seed(0)
    net = SimpleUnet(128, 0.0, compute_dtype=torch.bfloat16)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if ".out_layers.3.weight" in name:
                p.uniform_(-0.02, 0.02)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 10, (Bn,), generator=g).cuda()
    init = torch.randn((Bn, 1, S, S), generator=g).cuda()
    obs = ops.box_mean((torch.rand((Bn, 1, S, S), generator=g) * 2 - 1).cuda(), 1, N)
    outs = []
    for streams in (1, 2):
        d = GaussianDiffusion(mean_type="v", num_steps=3, sampler=sampler, seed=11)
        d.SAMPLER_STREAMS = streams
        assert (Bn // 2) * S * S >= d.STREAM_MIN_PIXELS
        outs.append(d.restore(net=partial(net, guide=y), obs=obs, factor=N, init_x=init, cond_w=cond_w, record=True))
    for a, b_ in zip(*outs):
        assert a.shape == b_.shape and torch.equal(a, b_)
    assert bool(torch.isfinite(outs[0][0]).all())
    err, bound = _consistency(outs[0][0][-1], obs, 1, N)
    assert err <= bound


# ---- G5: the plugin ----------------------------------------------------------------------------------------------------------------------
def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=6, bs=8)
    G.update(flags)
    return Model(G).to("cuda")


@pytest.mark.parametrize("flags,factor,gray", [({}, 7, False), ({"in_channels": 3, "image_size": 8}, 2, True)])
def test_plugin_degrade_and_restore(flags, factor, gray):
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, PhiloxStream
    model = _model(ema_decay=0.999, **flags)
    model.eval()
    C, S = model.net.in_channels, model.size
    x = torch.rand(5, C, S, S, device="cuda") * 2 - 1
    y = torch.randint(0, 10, (5,), device="cuda")
    cf = C if gray else 1
    obs = model.degrade(x, factor=factor, gray=gray)
    assert obs.shape == (5, C // cf, S // factor, S // factor) and torch.equal(obs, ops.box_mean(x, cf, factor))
    out = model.restore(obs, factor=factor, gray=gray, y=y, seed=3)
    assert out.shape == x.shape and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 3.0
    err, bound = _consistency(out, obs, cf, factor)
    assert err <= bound
    assert torch.equal(model.degrade(out, factor=factor, gray=gray), ops.box_mean(out, cf, factor))
    # the EMA net, the initial noise from PhiloxStream(seed), guidance with cond_w = 0.5 as in sample()
    assert model.optimizer.ema_seeded
    noise = PhiloxStream(3).normal(tuple(x.shape), "cuda")
    d = GaussianDiffusion(mean_type="v", num_steps=6, sample_cond_w=-1.0, seed=model.diffusion.rng.seed)
    d.rng.counter = model.diffusion.rng.counter - (5 + 3) // 4                # the guidance draw restore made
    ref = d.restore(net=partial(model.ema_net, guide=y), obs=obs, factor=factor, gray=gray, init_x=noise, cond_w=0.5)[0][-1]
    assert torch.equal(out, ref)
    free = model.restore(obs, factor=factor, gray=gray, seed=3)              # without labels: unguided
    assert not torch.equal(free, out) and _consistency(free, obs, cf, factor)[0] <= bound


class _Frames:
    """A writer with the device path (`write_frames`) that keeps what it is given."""

    def __init__(self):
        self.frames = {}

    def write_frames(self, tag, x, step, **kw):
        self.frames[tag] = x.detach().clone()


@pytest.mark.parametrize("flags,on,cf,N", [({}, {"restore_eval": 2}, 1, 2),
                                           ({"in_channels": 3, "image_size": 8}, {"restore_gray": 1}, 3, 1),
                                           ({"in_channels": 3, "image_size": 8}, {"restore_eval": 4, "restore_gray": 1}, 3, 4)])
def test_evaluate_restore_eval(flags, on, cf, N):
    C, S = flags.get("in_channels", 1), flags.get("image_size", 28)
    x = torch.rand(8, C, S, S, device="cuda") * 2 - 1
    y = torch.randint(0, 10, (8,), device="cuda")
    evs, writers, host = [], [], []
    for extra in ({}, on):
        torch.manual_seed(0)                                                    # the same initial weights
        model = _model(**flags, **extra)
        model.eval()
        random.seed(5)
        writers.append(_Frames())
        model.evaluate(writers[-1], x, y.clone(), 0)
        host.append(random.random())                                            # the host RNG has been consumed alike
        evs.append(model.last_eval)
    off, on_ = evs
    assert not any(k.startswith("restore") for k in off) and not any(k.startswith("restore") for k in writers[0].frames)
    assert host[0] == host[1]
    for k in ("samples", "sampling_process", "eps", "x"):
        assert torch.equal(off[k], on_[k]), k                                  # everything evaluate() made before is unchanged
    for k in writers[0].frames:
        assert torch.equal(writers[0].frames[k], writers[1].frames[k]), k
    img = on_["restore"]
    assert img.dtype == torch.uint8 and img.shape == (8, C, S, S)
    z, z_in = writers[1].frames["restore"], writers[1].frames["restore_input"]
    obs = R.A(x.double(), cf, N)
    assert z.shape == z_in.shape == x.shape
    assert float((z_in.double() - R.A_pinv(obs, cf, N)).abs().max()) <= (cf * N * N + 1) * U24      # the replicated observation
    assert _consistency(z, obs, cf, N)[0] <= (cf * N * N + 4) * U24 + (cf * N * N + 1) * U24           # ... which the restoration agrees with
    psnr = lambda t: 10.0 * torch.log10(4.0 / (t.double() - x.double()).square().mean(dim=(1, 2, 3)))
    for key, t in (("restore_psnr", z), ("restore_input_psnr", z_in)):
        assert on_[key].shape == (8,) and torch.allclose(on_[key].double(), psnr(t).cpu(), rtol=1e-6, atol=0)


# ---- G6: the restoration it is there for -------------------------------------------------------------------------------------------------
def test_restores_the_right_image():
    """Trained on two images only, the net returns from degrade(x_k) (4 x 4 box means) an image nearer to x_k than to the other one.
    tools/restore_probe.py measured the hit rate p over 512 draws (profiles/restore_probe.txt): 1.000.  The bar sits three binomial standard
    deviations sqrt(p (1 - p) / 64), at this test's 64 draws, below p: 1.0 - 3 x 0 = 1.0.  The seeds are fixed."""
    model = inpaint_ref.train_two_mode(_model)
    right, uncond = R.restore_accuracy(model)
    print(f"restore: right image {right:.3f}, unconditional nearer mode 0 {uncond:.3f}")
    assert right >= 1.0, (right, uncond)
    assert 0.2 <= uncond <= 0.8, uncond                                         # without the observation the net draws both images
