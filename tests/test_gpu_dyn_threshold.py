"""GPU tests of dynamic thresholding (Saharia et al. 2022, section 2.3; an extension): the select kernel (gmk_dyn_threshold) bit for bit against
the fp32 restatement of its quantile rule, the thresholded update kernels (gmk_sampler_step_dt, gmk_dpm_solver_step_dt) against the float64
restatement (tests/dyn_threshold_ref.py) and, with thr = 1, against the kernels they are a second instantiation of, whole chains on every path
of the sampler loop - kernel by kernel, the captured-graph forward, two half-batch streams, the guided 2B batch - the effect it is there for
and the plugin surface."""
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyn_threshold_ref as R  # noqa: E402

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}      # tests/test_gpu_dpm_solver.py's chain bars


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def make_net(dtype, C=128, seed=0):
    """Default-init scale with the zero-initialised out_layers.3 convs made live (the conditioning of test_gpu_dpm_solver.py)."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    net = SimpleUnet(C, 0.0, compute_dtype=dtype)
    params = U.reference_init_params(C, 1, seed=seed, zero_out_layers=False)
    net.load_state_dict(params, strict=True)
    return net.cuda().eval(), params


def chain_inputs(B, S):
    g = torch.Generator().manual_seed(11)
    init = torch.randn((B, 1, S, S), generator=g)
    y = torch.tensor([1, 7, 3, 5][:B])
    w = torch.tensor([0.3, 1.7, 3.2, 0.9][:B])
    return init, y, w


# ---- the select kernel: exact order statistics ------------------------------------------------------------------------------------------------
def _select_inputs(n):
    """Four input sets of B = 3 images of n values (mean type 'x', unguided: x_raw is the input's bits)."""
    B = 3
    g = torch.Generator().manual_seed(1000 + n)
    sets = {"randn": torch.randn((B, n), generator=g) * 1.7}
    sets["equal"] = torch.tensor([0.75, -2.5, 0.0])[:, None].expand(B, n).contiguous()
    levels = torch.tensor([-2.0, -0.5, 0.5, 1.25, 3.0])
    sets["ties"] = levels[torch.randint(0, 5, (B, n), generator=g)]
    # the exponent range: image 0 spreads over every exponent (the top digits decide), image 1 packs 1 + k 2^-23 (only the last digit differs)
    # between the specials, image 2 packs 1.5 + k 2^-14 (the third digit); zeros, -0.0, 1e-30, 1e30 and denormals in all three
    sign = torch.randint(0, 2, (B, n), generator=g).float() * 2 - 1
    k = torch.randint(0, 200, (B, n), generator=g).float()
    spread = sign[0] * torch.pow(2.0, torch.randint(-140, 100, (n,), generator=g).float()) * (1 + torch.rand((n,), generator=g))
    x = torch.stack([spread, sign[1] * (1.0 + k[1] * 2.0 ** -23), sign[2] * (1.5 + k[2] * 2.0 ** -14)])
    special = torch.tensor([0.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, 1e-45, -3e-39, 1e-40, 1.1754944e-38])
    pick = torch.randint(0, 3 * len(special), (B, n), generator=g)
    sets["exponents"] = torch.where(pick < len(special), special[pick % len(special)], x)
    return sets


@pytest.mark.parametrize("n_extra", [(1, 0), (2, 0), (143, 0), (256, 0), (1027, 0), (12288, 0), (None, 3)])
def test_select_is_bit_exact(n_extra):
    """q and s bit-equal to the fp32 restatement of the quantile rule: one thread (n = 1, 2), a partial and a full pass (143, 256), the scalar
    path (1027), the largest LDS-resident image (12288) and the recompute-from-global path (capacity + 3)."""
    from generative_models_amd import ops
    n = n_extra[0] if n_extra[0] is not None else ops.DYN_THRESHOLD_KEYS + n_extra[1]
    z = rnd(3, n, seed=5).cuda()
    for name, x in _select_inputs(n).items():
        xd = x.cuda()
        assert np.array_equal(bits(xd), bits(x))
        for p in (1e-3, 0.5, 0.995, 1.0):
            q_ref, s_ref = R.quantile_fp32(x, p)
            s, q = ops.dyn_threshold(xd, z, 0.7, p, mean_type="x", want_q=True)
            s2, q2 = ops.dyn_threshold(xd, z, 0.7, p, mean_type="x", want_q=True)
            assert np.array_equal(bits(q), q_ref.view(np.uint32)), (name, n, p, q.cpu().numpy(), q_ref)
            assert np.array_equal(bits(s), s_ref.view(np.uint32)), (name, n, p, s.cpu().numpy(), s_ref)
            assert torch.equal(s, s2) and np.array_equal(bits(q), bits(q2))         # the same call gives the same bits
            assert torch.equal(ops.dyn_threshold(xd, z, 0.7, p, mean_type="x"), s)  # without q_out


# ---- the thresholded update kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ddim", "noisy", "dpmpp_2m"])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("mean_type", ["v", "eps"])
def test_step_against_restatement(mean_type, guided, kind):
    """test_sampler_step's shapes, times and bars, against the float64 restatement: x-hat 1e-4; eps-hat and z 1e-4, 2e-3 where logsnr_t <= -15;
    s 1e-4 relative.  p = 0.995; the inputs are scaled by 1.5 so that q > 1 for every image."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import dpm_solver_coefs
    from oracle import diffusion_ref as D
    B, p = 4, 0.995
    z = rnd(B, 1, 12, 12, seed=70) * 1.5
    v = rnd(B, 1, 12, 12, seed=71) * 1.5
    vu = rnd(B, 1, 12, 12, seed=72) * 1.5 if guided else None
    w = torch.tensor([0.0, 0.5, 2.0, 3.9]) if guided else None
    noise = rnd(B, 1, 12, 12, seed=73)
    x_prev = rnd(B, 1, 12, 12, seed=74).clamp(-1, 1)
    dev = lambda t: None if t is None else t.cuda()
    for (i, T) in [(7, 8), (3, 8), (0, 8), (199, 200)]:
        u_t, u_s = D.sampler_times(i, T)
        lt = D.logsnr_schedule_cosine(torch.tensor(u_t)); ls = D.logsnr_schedule_cosine(torch.tensor(u_s))
        xh, eh, s_ref, q_ref = R.predict(v, z, lt.expand(B), p, mean_type, vu, w)
        assert float(q_ref.min()) > 1.0
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
        s = ops.dyn_threshold(dev(v), dev(z), float(lt), p, v_uncond=dev(vu), cond_w=dev(w), mean_type=mean_type)
        kw = dict(v_uncond=dev(vu), cond_w=dev(w), want_pred=True, mean_type=mean_type, thr=s)
        if kind == "dpmpp_2m":
            hist = x_prev.cuda()
            zn, xo, eo = ops.dpm_solver_step(dev(v), dev(z), hist, float(lt), float(ls), c.coef_z, c.coef_x, k, i == 0, **kw)
            assert torch.equal(hist, xo)                               # the history holds this step's x-hat
        else:
            zn, xo, eo = ops.sampler_step(dev(v), dev(z), float(lt), float(ls), i == 0, noise=dev(noise) if kind == "noisy" else None, **kw)
        scale = 1e-4 if float(lt) > -15 else 2e-3
        es = float(((s.double().cpu() - s_ref).abs() / s_ref).max())
        ex, ee, ez = rel_err(xo, xh), rel_err(eo, eh), rel_err(zn, z_ref)
        assert es < 1e-4 and ex < 1e-4 and ee < scale and ez < scale, (i, T, es, ex, ee, ez)
        assert float(xo.abs().max()) <= 1.0
        if i == 0:
            assert torch.equal(zn, xo)


@pytest.mark.parametrize("mean_type", ["v", "eps", "x"])
def test_unit_threshold_is_the_static_kernels(mean_type):
    """thr = 1 and no guidance: clamp(x, -1, 1) / 1 is the static clip, so the _dt instantiations give the bits of the kernels they share
    their source with - z, x-hat, eps-hat, the history, the duplicate and the next log-SNR vector."""
    from generative_models_amd import ops
    B = 4
    z = rnd(B, 3, 12, 12, seed=70).cuda() * 1.5
    v = rnd(B, 3, 12, 12, seed=71).cuda() * 1.5
    noise = rnd(B, 3, 12, 12, seed=73).cuda()
    ones = torch.ones((B,), device="cuda")
    for is_last in (False, True):
        for nz in (None, noise):
            outs = []
            for thr in (None, ones):
                ln = torch.zeros((2 * B,), device="cuda")
                (zn, z2), xo, eo = ops.sampler_step(v, z, -1.3, 0.4, is_last, noise=nz, want_pred=True, mean_type=mean_type, dup=True,
                                                    logsnr_next=ln, thr=thr)
                outs.append((zn, z2, xo, eo, ln))
            assert all(torch.equal(a, b) for a, b in zip(*outs))
        outs = []
        for thr in (None, ones):
            hist = rnd(B, 3, 12, 12, seed=74).cuda()
            ln = torch.zeros((B,), device="cuda")
            zn, xo, eo = ops.dpm_solver_step(v, z, hist, -1.3, 0.4, 0.8, 0.3, 0.45, is_last, want_pred=True, mean_type=mean_type,
                                             logsnr_next=ln, thr=thr)
            outs.append((zn, xo, eo, hist, ln))
        assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_thr_is_checked():
    from generative_models_amd import ops
    z = rnd(4, 1, 8, 8, seed=1).cuda()
    with pytest.raises(ValueError):
        ops.sampler_step(z, z, -1.0, 1.0, False, thr=torch.ones((3,), device="cuda"))
    with pytest.raises(ValueError):
        ops.sampler_step(z, z, -1.0, 1.0, False, thr=torch.ones((4,), device="cuda", dtype=torch.float64))
    with pytest.raises(ValueError):
        ops.dyn_threshold(z, z, -1.0, 0.0)


# ---- chains -----------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _chain_ref(params, sampler, guided, steps=6, B=3, S=8, p=0.9):
    key = (sampler, guided, steps)
    if key not in _REF:
        init, y, w = chain_inputs(B, S)
        with torch.no_grad():
            _REF[key] = R.sample(params, init, y, steps, p, sampler, cond_w=w if guided else None)
    return _REF[key]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_chain_vs_restatement(sampler, guided, dtype):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, steps = 3, 8, 6
    net, params = make_net(dtype)
    init, y, w = chain_inputs(B, S)
    zs_ref, xs_ref, _ = _chain_ref(params, sampler, guided)
    diff = GaussianDiffusion(mean_type="v", num_steps=steps, sampler=sampler, sample_cond_w=-1.0, dyn_threshold=0.9)
    assert not diff._graph_path(net, 2 * B if guided else B, S, S)                 # T < 16: kernel by kernel
    kw = dict(net=partial(net, guide=y.cuda()), init_x=init.cuda(), cond_w=0.5 if guided else None, net_cond_w=w.cuda() if guided else None)
    zs, xs, es = diff.sample(**kw)
    assert zs.shape == zs_ref.shape == xs.shape == es.shape
    tol = (1 if dtype == torch.float32 else 3) * TOL[dtype]
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    assert ez < tol and ex < tol, (ez, ex)
    assert torch.equal(zs[-1], xs[-1]) and float(xs.abs().max()) <= 1.0
    last = diff.sample(**kw, record=False)[0][-1]
    assert torch.equal(last, zs[-1])


def test_graph_path_vs_restatement():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, steps = 3, 8, 20
    net, params = make_net(torch.float32)
    init, y, _ = chain_inputs(B, S)
    diff = GaussianDiffusion(mean_type="v", num_steps=steps, sampler="ddim", dyn_threshold=0.9)
    assert diff._graph_path(net, B, S, S)
    zs, xs, _ = diff.sample(net=partial(net, guide=y.cuda()), init_x=init.cuda())
    assert len(diff._graphs) == 1
    zs_ref, xs_ref, _ = _chain_ref(params, "ddim", False, steps=steps)
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    assert ez < 1e-3 and ex < 1e-3, (ez, ex)
    last = diff.sample(net=partial(net, guide=y.cuda()), init_x=init.cuda(), record=False)[0][-1]
    assert torch.equal(last, zs[-1])


@pytest.mark.parametrize("cond_w", [None, 0.5])
@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_two_streams_are_bit_identical(sampler, cond_w):
    """The select is per image, so two half-batches on two streams give the whole batch's bits."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S = 4, 8
    net, _ = make_net(torch.bfloat16)
    assert net.channels == 128
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    init = torch.randn((B, 1, S, S), generator=g).cuda()
    wv = None if cond_w is None else torch.tensor([0.3, 1.7, 3.2, 0.9]).cuda()
    outs = []
    for streams in (1, 2):
        d = GaussianDiffusion(mean_type="v", num_steps=4, sampler=sampler, seed=11, dyn_threshold=0.9)
        d.SAMPLER_STREAMS = streams
        d.STREAM_MIN_PIXELS = 0
        outs.append(d.sample(net=partial(net, guide=y), init_x=init, cond_w=cond_w, net_cond_w=wv))
        assert (getattr(d, "_streams", None) is not None) == (streams == 2)       # the split really ran
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all())


def test_it_reduces_saturation_under_strong_guidance():
    """Guidance 3.9 on the 6-step chain: the thresholded sample differs from the static one, and strictly fewer of its pixels sit at |x| = 1."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S = 3, 8
    net, _ = make_net(torch.float32)
    init, y, _ = chain_inputs(B, S)
    w = torch.full((B,), 3.9).cuda()
    final = {}
    for p in (0.0, 0.9):
        d = GaussianDiffusion(mean_type="v", num_steps=6, sampler="ddim", sample_cond_w=-1.0, dyn_threshold=p)
        final[p] = d.sample(net=partial(net, guide=y.cuda()), init_x=init.cuda(), cond_w=0.5, net_cond_w=w, record=False)[0][-1]
    assert not torch.equal(final[0.0], final[0.9])
    sat = {p: float((t.abs() == 1.0).float().mean()) for p, t in final.items()}
    assert sat[0.9] < sat[0.0], sat
    assert float(final[0.9].abs().max()) <= 1.0


def test_plugin_surface():
    from generative_models_amd import common, main
    G0, Model = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--dyn_threshold", "0.995"])
    assert G0.dyn_threshold == 0.995
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=8, bs=8, dyn_threshold=G0.dyn_threshold)
    model = Model(G).to("cuda")
    assert model.diffusion.dyn_threshold == 0.995
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
