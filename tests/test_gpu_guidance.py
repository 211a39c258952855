"""GPU tests of the guided samplers' two options (`GaussianDiffusion(guidance_interval=(lo, hi), cfg_rescale=phi)`; extensions): the reduction
kernel gmk_cfg_rescale - its exact identities and its accuracy against float64 -, the thresholded update kernels driven by it against the
float64 restatement (tests/guidance_ref.py), whole chains that cross both mode changes on every path of the sampler loop - kernel by kernel,
two captured graphs, two half-batch streams, inpainting with resampling -, their bit-exact composition from all-guided and unguided chains,
the degenerate intervals (which show that nothing existing moved), the number of images forwarded, and the plugin surface."""
import math
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import guidance_ref as G  # noqa: E402
import sampler_ref as SR  # noqa: E402

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}      # tests/test_gpu_dyn_threshold.py's chain bars
INTERVAL = (-3.0, 1.5)      # on the 6-step grid (-20.001, -2.634, -1.099, -0.0, 1.099, 2.634): rows i = 4, 3, 2, 1 guided, i = 5 and i = 0 not
EMPTY = (-2.0, -1.5)        # between two points of that grid: no row guided
U = 2.0 ** -24


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


_NETS = {}


def make_net(dtype, C=128, seed=0):
    """Default-init scale with the zero-initialised out_layers.3 convs made live (the conditioning of test_gpu_dyn_threshold.py)."""
    if dtype not in _NETS:
        from generative_models_amd.diffusion.simple_unet import SimpleUnet
        from oracle import unet_ref
        net = SimpleUnet(C, 0.0, compute_dtype=dtype)
        params = unet_ref.reference_init_params(C, 1, seed=seed, zero_out_layers=False)
        net.load_state_dict(params, strict=True)
        _NETS[dtype] = (net.cuda().eval(), params)
    return _NETS[dtype]


def chain_inputs(B, S):
    """test_gpu_dyn_threshold.py's."""
    g = torch.Generator().manual_seed(11)
    init = torch.randn((B, 1, S, S), generator=g)
    y = torch.tensor([1, 7, 3, 5][:B])
    w = torch.tensor([0.3, 1.7, 3.2, 0.9][:B])
    return init, y, w


def diffusion(sampler="ddim", interval=None, phi=0.0, steps=6, **kw):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion(mean_type="v", num_steps=steps, sampler=sampler, sample_cond_w=-1.0, guidance_interval=interval, cfg_rescale=phi, **kw)


def run(d, net, init, y, w, **kw):
    """A guided call (w: the per-image weights) or, with w None, an unguided one with the same labels."""
    return d.sample(net=partial(net, guide=y.cuda()), init_x=init.cuda(), cond_w=None if w is None else 0.5,
                    net_cond_w=None if w is None else w.cuda(), **kw)


# ---- 1. the kernel's exact identities -------------------------------------------------------------------------------------------------------
def _sizes():
    from generative_models_amd import ops
    return [1, 4, 143, 256, 1027, 12288, ops.CFG_RESCALE_KEEP + 3]


def _kernel_inputs(n, B=3, shift=0.0):
    v = (rnd(B, n, seed=100 + n, scale=1.5) + shift).cuda()
    vu = (rnd(B, n, seed=200 + n, scale=1.5) + shift).cuda()
    z = rnd(B, n, seed=300 + n).cuda()
    return v, vu, z


@pytest.mark.parametrize("mean_type", ["x", "v", "eps"])
@pytest.mark.parametrize("k", range(7))
def test_kernel_identities(k, mean_type):
    """One element (n = 1: q_r = 0), one 16-byte group (4), a partial and a full pass (143, 256), the scalar path (1027), the largest resident
    image (12288) and the re-read path (capacity + 3): w_b = 0 gives thr = ratio = 1.0 and phi = 0 gives thr = 1.0, bit for bit; the same
    call gives the same bits; rows called alone equal the whole batch's."""
    from generative_models_amd import ops
    n = _sizes()[k]
    v, vu, z = _kernel_inputs(n)
    one = np.float32(1.0).view(np.uint32)
    zero_w = torch.zeros((3,), device="cuda")
    w = torch.tensor([0.0, 2.0, 3.9], device="cuda")
    lt = -0.7
    thr, ratio = ops.cfg_rescale(v, z, lt, 0.7, vu, zero_w, mean_type=mean_type, want_ratio=True)
    assert np.all(bits(thr) == one), (n, thr)
    if n > 1:
        assert np.all(bits(ratio) == one), (n, ratio)
    else:
        assert bool(torch.isnan(ratio).all())                                      # sqrt(0 / 0): one value has no spread
    thr0, ratio0 = ops.cfg_rescale(v, z, lt, 0.0, vu, w, mean_type=mean_type, want_ratio=True)
    assert np.all(bits(thr0) == one), (n, thr0)
    thr, ratio = ops.cfg_rescale(v, z, lt, 0.7, vu, w, mean_type=mean_type, want_ratio=True)
    assert bits(thr)[0] == one and bool(torch.isfinite(thr).all())                 # row 0 has w = 0
    if n == 1:
        assert np.all(bits(thr) == one)                                            # q_r = 0
    else:
        assert np.array_equal(bits(ratio), bits(ratio0))                           # the ratio does not depend on phi
        assert bool((thr[1:] != 1.0).all())
    thr2, ratio2 = ops.cfg_rescale(v, z, lt, 0.7, vu, w, mean_type=mean_type, want_ratio=True)
    assert np.array_equal(bits(thr), bits(thr2)) and np.array_equal(bits(ratio), bits(ratio2))
    assert np.array_equal(bits(ops.cfg_rescale(v, z, lt, 0.7, vu, w, mean_type=mean_type)), bits(thr))          # without ratio_out
    part = ops.cfg_rescale(ops.aligned(v[1:3]), ops.aligned(z[1:3]), lt, 0.7, ops.aligned(vu[1:3]), ops.aligned(w[1:3]), mean_type=mean_type,
                           want_ratio=True)
    assert np.array_equal(bits(part[0]), bits(thr)[1:3]) and np.array_equal(bits(part[1]), bits(ratio)[1:3])


def test_kernel_takes_image_shapes_and_checks_its_inputs():
    from generative_models_amd import ops
    v, vu, z = (rnd(2, 3, 8, 8, seed=s).cuda() for s in (1, 2, 3))
    w = torch.tensor([1.0, 3.0], device="cuda")
    thr = ops.cfg_rescale(v, z, 0.3, 0.7, vu, w)
    flat = ops.cfg_rescale(v.view(2, -1), z.view(2, -1), 0.3, 0.7, vu.view(2, -1), w)
    assert thr.shape == (2,) and torch.equal(thr, flat)
    with pytest.raises(ValueError):
        ops.cfg_rescale(v, z, 0.3, 1.5, vu, w)
    with pytest.raises(ValueError):
        ops.cfg_rescale(v, z, 0.3, 0.7, None, None)
    with pytest.raises(AssertionError):
        ops.cfg_rescale(v, z, 0.3, 0.7, vu[:, :2].contiguous(), w)


# ---- 2. accuracy against float64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0.0, 0.5])
@pytest.mark.parametrize("k", range(7))
def test_kernel_accuracy(k, shift):
    """Mean type 'x' (x_c is the input's bits), independent v and v_uncond = randn 1.5 (+ 0.5: |mean| <= std): thr and ratio against float64
    from the fp32 inputs, relative bound 2^-24 (ceil(n / 256) + 32 + 8 (1 + 2 w)): ceil(n / 256) + 8 additions per chain (the kernel's order:
    thread t adds t, t + 256, ... then the 6 + 2 of the workgroup's tree), a few roundings for the centring, the square, the square root, the
    division and f, and 3 u (1 + 2 w) per element for forming x_raw in fp32.  For w >= 2 the ratio is below 1 and thr above it: the effect
    the option exists for, on inputs where it is real.
    Worst measured error / bound over all 108 cases with n > 1: 0.042 (thr), 0.040 (ratio)."""
    from generative_models_amd import ops
    n = _sizes()[k]
    v, vu, z = _kernel_inputs(n, shift=shift)
    worst = 0.0
    for wv in (0.5, 2.0, 3.9):
        w = torch.full((3,), wv)
        w64 = w.double()[:, None]
        x_c = v.cpu().double()
        x_r = (1.0 + w64) * x_c + (-w64) * vu.cpu().double()
        ratio_ref = G.ratio(x_c, x_r)
        for phi in (0.3, 0.7, 1.0):
            thr, ratio = ops.cfg_rescale(v, z, 0.4, phi, vu, w.cuda(), mean_type="x", want_ratio=True)
            if n == 1:
                assert bool((thr == 1.0).all())
                continue
            thr_ref = 1.0 / (1.0 + float(np.float32(phi)) * (ratio_ref - 1.0))
            bound = U * (math.ceil(n / 256) + 32 + 8 * (1 + 2 * wv))
            e_r = float(((ratio.cpu().double() - ratio_ref).abs() / ratio_ref).max())
            e_t = float(((thr.cpu().double() - thr_ref).abs() / thr_ref).max())
            worst = max(worst, e_r / bound, e_t / bound)
            print(f"n={n} shift={shift} w={wv} phi={phi}: ratio err {e_r:.3e} thr err {e_t:.3e} bound {bound:.3e}")
            assert e_r <= bound and e_t <= bound, (n, wv, phi, e_r, e_t, bound)
            if wv >= 2.0:           # std(x_raw) ~ sqrt((1 + w)^2 + w^2) std(x_c): certain from 143 values on, the float64 ratio decides below
                assert n < 143 or bool((ratio_ref < 1.0).all())
                below = (ratio_ref < 1.0).cuda()
                assert torch.equal(ratio < 1.0, below) and torch.equal(thr > 1.0, below), (n, wv, phi, ratio, thr)
    print(f"n={n} shift={shift}: worst error / bound {worst:.3f}")


# ---- 3. the thresholded update kernels driven by the factor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "noisy", "dpmpp_2m"])
@pytest.mark.parametrize("mean_type", ["v", "eps"])
def test_step_against_restatement(mean_type, kind):
    """test_gpu_dyn_threshold.py's test_step_against_restatement with thr from `ops.cfg_rescale`: its shapes, times and bars - x-hat and thr 1e-4
    relative; eps-hat and z 1e-4, 2e-3 where logsnr_t <= -15."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import dpm_solver_coefs
    from oracle import diffusion_ref as D
    B, phi = 4, 0.7
    z = rnd(B, 1, 12, 12, seed=70) * 1.5
    v = rnd(B, 1, 12, 12, seed=71) * 1.5
    vu = rnd(B, 1, 12, 12, seed=72) * 1.5
    w = torch.tensor([0.0, 0.5, 2.0, 3.9])
    noise = rnd(B, 1, 12, 12, seed=73)
    x_prev = rnd(B, 1, 12, 12, seed=74).clamp(-1, 1)
    for (i, T) in [(7, 8), (3, 8), (0, 8), (199, 200)]:
        u_t, u_s = D.sampler_times(i, T)
        lt = D.logsnr_schedule_cosine(torch.tensor(u_t)); ls = D.logsnr_schedule_cosine(torch.tensor(u_s))
        xh, eh, f_ref, _ = G.predict(v, z, lt.expand(B), phi, mean_type, vu, w)
        thr_ref = 1.0 / f_ref
        assert abs(float(f_ref[0]) - 1.0) < 1e-12 and float(f_ref[1:].max()) < 1.0      # w = 0: no rescale; else the guided spread is larger
        lt64, ls64 = lt.double(), ls.double()
        if kind == "noisy":
            alpha_st = torch.sqrt((1 + torch.exp(-lt64)) / (1 + torch.exp(-ls64)))
            r = torch.exp(lt64 - ls64); omr = -torch.expm1(lt64 - ls64)
            zs = r * alpha_st * z.double() + omr * torch.sqrt(torch.sigmoid(ls64)) * xh + torch.sqrt(omr * torch.sigmoid(-lt64)) * noise.double()
        elif kind == "ddim":
            zs = torch.sqrt(torch.sigmoid(ls64)) * xh + torch.sqrt(torch.sigmoid(-ls64)) * eh
        else:
            c = dpm_solver_coefs(T)[T - 1 - i]
            assert c.i == i
            k = c.coef_prev if c.coef_prev else 0.37                   # a second-order step also where the table has a first-order one
            zs = c.coef_z * z.double() + c.coef_x * ((1 + k) * xh - k * x_prev.double())
        z_ref = xh if i == 0 else zs
        thr = ops.cfg_rescale(v.cuda(), z.cuda(), float(lt), phi, vu.cuda(), w.cuda(), mean_type=mean_type)
        kw = dict(v_uncond=vu.cuda(), cond_w=w.cuda(), want_pred=True, mean_type=mean_type, thr=thr)
        if kind == "dpmpp_2m":
            hist = x_prev.cuda()
            zn, xo, eo = ops.dpm_solver_step(v.cuda(), z.cuda(), hist, float(lt), float(ls), c.coef_z, c.coef_x, k, i == 0, **kw)
            assert torch.equal(hist, xo)
        else:
            zn, xo, eo = ops.sampler_step(v.cuda(), z.cuda(), float(lt), float(ls), i == 0, noise=noise.cuda() if kind == "noisy" else None, **kw)
        scale = 1e-4 if float(lt) > -15 else 2e-3
        et = float(((thr.double().cpu() - thr_ref).abs() / thr_ref).max())
        ex, ee, ez = rel_err(xo, xh), rel_err(eo, eh), rel_err(zn, z_ref)
        assert et < 1e-4 and ex < 1e-4 and ee < scale and ez < scale, (i, T, et, ex, ee, ez)
        assert float(xo.abs().max()) <= 1.0
        if i == 0:
            assert torch.equal(zn, xo)


# ---- 4. chains against the restatement -------------------------------------------------------------------------------------------------------
_REF = {}


def _chain_ref(params, sampler, phi, interval=INTERVAL, steps=6, B=3, S=8):
    key = (sampler, phi, interval, steps)
    if key not in _REF:
        init, y, w = chain_inputs(B, S)
        with torch.no_grad():
            _REF[key] = G.sample(params, init, y, steps, w, interval, phi, sampler)
    return _REF[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_chain_vs_restatement(sampler, phi, dtype):
    """B = 3, S = 8, 6 steps, interval [-3, 1.5]: unguided, four guided rows, unguided - both mode changes.  test_gpu_dyn_threshold.py's bars."""
    from generative_models_amd.diffusion.gaussian_diffusion import guidance_mask, sampler_plan
    B, S, steps = 3, 8, 6
    net, params = make_net(dtype)
    init, y, w = chain_inputs(B, S)
    assert guidance_mask(sampler_plan(steps, sampler), INTERVAL) == [False, True, True, True, True, False]
    zs_ref, xs_ref, _ = _chain_ref(params, sampler, phi)
    d = diffusion(sampler, INTERVAL, phi)
    assert not d._graph_path(net, 2 * B, S, S)                                     # T < 16: kernel by kernel
    zs, xs, es = run(d, net, init, y, w)
    assert zs.shape == zs_ref.shape == xs.shape == es.shape
    tol = (1 if dtype == torch.float32 else 3) * TOL[dtype]
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    assert ez < tol and ex < tol, (ez, ex)
    assert torch.equal(zs[-1], xs[-1]) and float(xs.abs().max()) <= 1.0
    last = run(d, net, init, y, w, record=False)[0][-1]
    assert torch.equal(last, zs[-1])


# ---- 5. a mixed chain is its parts, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_mixed_chain_composes_bitwise(dtype):
    """ddim, phi = 0: row 0 is the unguided chain's; an all-guided chain started from it reproduces rows 1 - 4; an unguided chain started from row 4
    gives row 5."""
    B, S = 3, 8
    net, _ = make_net(dtype)
    init, y, w = chain_inputs(B, S)
    zs, xs, es = run(diffusion("ddim", INTERVAL), net, init, y, w)
    plain = run(diffusion("ddim"), net, init, y, None)
    assert torch.equal(zs[0], plain[0][0]) and torch.equal(xs[0], plain[1][0]) and torch.equal(es[0], plain[2][0])
    mid = diffusion("ddim").sample(net=partial(net, guide=y.cuda()), init_x=zs[0], cond_w=0.5, net_cond_w=w.cuda(), start=5)
    for got, want in zip(mid, (zs, xs, es)):
        assert got.shape[0] == 5 and torch.equal(got[:4], want[1:5])
    assert not torch.equal(mid[0][4], zs[5])                                       # the last row is guided there, unguided here
    end = diffusion("ddim").sample(net=partial(net, guide=y.cuda()), init_x=zs[4], start=1)
    for got, want in zip(end, (zs, xs, es)):
        assert got.shape[0] == 1 and torch.equal(got[0], want[5])


# ---- 6. the degenerate intervals: nothing existing moved ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m", "noisy", "consistency"])
def test_degenerate_intervals_are_todays_chains(sampler):
    """[-21, 21] holds every row: the guided chain as it has always run; an interval without a grid point: the unguided chain with the same
    labels.  Bit for bit ('noisy' and 'consistency': with the same seed)."""
    B, S = 3, 8
    net, _ = make_net(torch.float32)
    init, y, w = chain_inputs(B, S)
    today = run(diffusion(sampler, seed=5), net, init, y, w)
    whole = run(diffusion(sampler, (-21.0, 21.0), seed=5), net, init, y, w)
    for a, b in zip(today, whole):
        assert torch.equal(a, b)
    plain = run(diffusion(sampler, seed=5), net, init, y, None)
    none = run(diffusion(sampler, EMPTY, seed=5), net, init, y, w)
    for a, b in zip(plain, none):
        assert torch.equal(a, b)
    assert not torch.equal(today[0], plain[0])
    mixed = run(diffusion(sampler, INTERVAL, seed=5), net, init, y, w)           # every sampler runs the mixed chain, and it is neither
    assert bool(torch.isfinite(mixed[0]).all()) and not torch.equal(mixed[0], today[0]) and not torch.equal(mixed[0], plain[0])
    assert torch.equal(mixed[0][0], plain[0][0])                                   # its first row is unguided


# ---- 7. the images forwarded --------------------------------------------------------------------------------------------------------------------
def test_forwarded_images():
    from generative_models_amd.diffusion.gaussian_diffusion import guidance_evals, guidance_mask, sampler_plan
    B, S = 3, 8
    net, _ = make_net(torch.float32)
    init, y, w = chain_inputs(B, S)
    plan = sampler_plan(6)
    seen = []
    orig = net.forward_hip
    net.forward_hip = lambda z, *a, **k: (seen.append(z.shape[0]), orig(z, *a, **k))[1]
    try:
        counts = {}
        for name, interval in (("mixed", INTERVAL), ("all", None), ("none", EMPTY)):
            del seen[:]
            run(diffusion("ddim", interval), net, init, y, w, record=False)
            counts[name] = sum(seen)
            if name == "mixed":
                assert seen == [B, 2 * B, 2 * B, 2 * B, 2 * B, B]
    finally:
        del net.forward_hip
    assert counts["mixed"] == guidance_evals(plan, guidance_mask(plan, INTERVAL), B) == B * (6 + 4)
    assert counts["all"] == guidance_evals(plan, guidance_mask(plan, None), B) == 12 * B
    assert counts["none"] == 6 * B


# ---- 8. the other paths of the loop -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,phi", [("ddim", 0.7), ("dpmpp_2m", 0.0), ("noisy", 0.0)])
def test_two_streams_are_bit_identical(sampler, phi):
    """The factor is per image and every launch writes its own half: two half-batches on two streams give the whole batch's bits."""
    B, S = 4, 8
    net, _ = make_net(torch.bfloat16)
    assert net.channels == 128
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 10, (B,), generator=g)
    init = torch.randn((B, 1, S, S), generator=g)
    w = torch.tensor([0.3, 1.7, 3.2, 0.9])
    outs = []
    for streams in (1, 2):
        d = diffusion(sampler, INTERVAL, phi, seed=11)
        d.SAMPLER_STREAMS = streams
        d.STREAM_MIN_PIXELS = 0
        outs.append(run(d, net, init, y, w))
        assert (getattr(d, "_streams", None) is not None) == (streams == 2)       # the split really ran
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all())


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_two_captured_graphs(phi):
    """20 steps, B = 3: both forwards (B and 2B images) replay a captured graph, and give the bits of the kernel-by-kernel path."""
    from generative_models_amd.diffusion.gaussian_diffusion import guidance_mask, sampler_plan
    B, S, steps = 3, 8, 20
    net, params = make_net(torch.float32)
    init, y, w = chain_inputs(B, S)
    mask = guidance_mask(sampler_plan(steps), INTERVAL)
    assert True in mask and False in mask and not mask[0] and not mask[-1]
    d = diffusion("ddim", INTERVAL, phi, steps=steps)
    assert d._graph_path(net, 2 * B, S, S)
    zs, xs, _ = run(d, net, init, y, w)
    assert len(d._graphs) == 2
    e = diffusion("ddim", INTERVAL, phi, steps=steps)
    e.GRAPH_MAX_PIXELS = 0
    zs2, xs2, _ = run(e, net, init, y, w)
    assert len(e._graphs) == 0 and torch.equal(zs, zs2) and torch.equal(xs, xs2)
    zs_ref, xs_ref, _ = _chain_ref(params, "ddim", phi, steps=steps)
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    assert ez < 1e-3 and ex < 1e-3, (ez, ex)
    assert torch.equal(run(d, net, init, y, w, record=False)[0][-1], zs[-1])      # a second call replays the same two graphs
    assert len(d._graphs) == 2


def test_inpainting_with_resampling():
    """resample = 2 on the mixed chain (a re-noising pass stays in its step's mode) against tests/inpaint_ref.py's merge (`sampler_ref.repaint`)
    composed with the restatement, at test_gpu_inpaint.py's guided fp32 bar (5e-3 per step); known pixels exactly."""
    import inpaint_ref
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, T, r, seed = 3, 8, 6, 2, 21
    net, params = make_net(torch.float32)
    init, y, _ = chain_inputs(B, S)
    g = torch.Generator().manual_seed(12)
    x0 = torch.rand((B, 1, S, S), generator=g) * 2 - 1
    mask = torch.zeros((1, 1, S, 1), dtype=torch.uint8)
    mask[:, :, : S // 2] = 1
    n = B * S * S
    F = inpaint_ref.forwards(T, r)
    eps1 = [ops.rng_normal((B, 1, S, S), seed, f * n // 2, "cuda").cpu() for f in range(F)]
    eps2 = [ops.rng_normal((B, 1, S, S), seed, f * n // 2 + n // 4, "cuda").cpu() for f in range(F)]
    w = torch.full((B,), 1.7)
    with torch.no_grad():
        zs_ref, xs_ref, _ = G.sample(params, init, y, T, w, INTERVAL, 0.7, "ddim", merge=SR.repaint(x0, mask.bool(), eps1, eps2), resample=r)
    d = GaussianDiffusion(mean_type="v", num_steps=T, sampler="ddim", sample_cond_w=1.7, guidance_interval=INTERVAL, cfg_rescale=0.7)
    seen = []
    orig = net.forward_hip
    net.forward_hip = lambda z, *a, **k: (seen.append(z.shape[0]), orig(z, *a, **k))[1]
    try:
        zs, xs, _ = d.inpaint(net=partial(net, guide=y.cuda()), x0=x0.cuda(), mask=mask.cuda(), init_x=init.cuda(), resample=r, seed=seed,
                              record=True)
    finally:
        del net.forward_hip
    assert seen == [B, B] + [2 * B] * 8 + [B]
    errs = [(rel_err(zs[k], zs_ref[k]), rel_err(xs[k], xs_ref[k])) for k in range(T)]
    assert all(ez < 5e-3 and ex < 5e-3 for ez, ex in errs), errs
    known = mask.cuda().bool().expand_as(zs[-1])
    assert torch.equal(zs[-1][known], x0.cuda()[known])


# ---- 9. the plugin surface ----------------------------------------------------------------------------------------------------------------------
def test_plugin_surface():
    from generative_models_amd import common, main
    G0, Model = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--sample_cond_w", "2.0", "--guidance_lo", "-3", "--guidance_hi", "1.5",
                                                 "--cfg_rescale", "0.7"])
    assert (G0.sample_cond_w, G0.guidance_lo, G0.guidance_hi, G0.cfg_rescale) == (2.0, -3.0, 1.5, 0.7)
    Gm = common.AttrDict(dict(Model.DG))
    Gm.update(lr=3e-4, pad32=0, device="cuda", timesteps=8, bs=8, sample_cond_w=G0.sample_cond_w, guidance_lo=G0.guidance_lo,
              guidance_hi=G0.guidance_hi, cfg_rescale=G0.cfg_rescale)
    model = Model(Gm).to("cuda")
    assert model.diffusion.guidance_interval == (-3.0, 1.5) and model.diffusion.cfg_rescale == 0.7
    model.eval()
    y = torch.randint(0, 10, (5,), device="cuda")
    s = model.sample(5, y=y)
    assert s.shape == (5, 1, 28, 28) and bool(torch.isfinite(s).all()) and float(s.abs().max()) <= 1.0
    x = torch.rand(8, 1, 28, 28, device="cuda") * 2 - 1
    model.evaluate(None, x, torch.randint(0, 10, (8,), device="cuda"), 0)
    ev = model.last_eval
    assert ev["samples"].shape == (25, 1, 28, 28) and ev["sampling_process"].shape == (8, 25, 1, 28, 28)
    mask = torch.zeros((1, 1, 28, 28), device="cuda")
    mask[..., :14, :] = 1
    out = model.inpaint(x[:5], mask, y=y)
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    m = mask.bool().expand_as(out)
    assert torch.equal(out[m], x[:5][m])                                           # known pixels exactly
    for flags in (dict(cfg_rescale=0.7, dyn_threshold=0.995), dict(cfg_rescale=0.7, sampler="consistency"), dict(cfg_rescale=0.7, restore_eval=2),
                  dict(guidance_lo=2.0, guidance_hi=-2.0)):
        bad = common.AttrDict(dict(Model.DG))
        bad.update(lr=3e-4, pad32=0, device="cuda", timesteps=8, bs=8, **flags)
        with pytest.raises(ValueError):
            Model(bad)
    with pytest.raises(ValueError, match="cfg_rescale"):
        model.diffusion.restore(net=partial(model._sampling_net(), guide=y), obs=torch.zeros((5, 1, 14, 14), device="cuda"), factor=2,
                                init_x=torch.zeros((5, 1, 28, 28), device="cuda"))
