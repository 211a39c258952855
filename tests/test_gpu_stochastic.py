"""GPU tests of gmk_stochastic_step and the samplers on it ('ancestral' with the reference's three posterior variances, 'ddim' with
ddim_eta > 0, 'sde_dpmpp_2m'): the kernel bit for bit against gmk_sampler_step's predictions and elementwise against the float64 restatement
(tests/stochastic_ref.py), the samplers step by step against the restatement and across their launch paths, and the model and command line.

The elementwise bound counts fp32 operations; u = 2^-24 is the unit roundoff:
  z_next   8 u (|c_z z| + |c_x| (|(1 + k) x_hat| + |k x_prev|) + |c_n xi|)
           each coefficient rounded once from double (u), each product once (u), 1 + k once, each of the three sums once: at most 7 u on the path
           of any term, relative to partial results that the sum of the terms' magnitudes bounds (`stochastic_ref.step_bound`)
  against gmk_sampler_step's ancestral update ('large', the same noise): twice that - the other kernel forms the same three coefficients on the
  device in fp32 (expf, expm1f, a quotient and a root each) where this one takes them from the host
"""
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stochastic_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
U = R.U24


def dev(a):
    from generative_models_amd import ops
    return ops.aligned(T(np.ascontiguousarray(a)).cuda())


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def rows_of(lt, ls):
    """One row of each kind for the step lt -> ls: (name, c_z, c_x, c_n, k)."""
    from generative_models_amd.diffusion.gaussian_diffusion import stochastic_row
    return [("ancestral large", *stochastic_row("ancestral", lt, ls, 1.0), 0.0),
            ("ancestral small", *stochastic_row("ancestral", lt, ls, 0.0), 0.0),
            ("ancestral medium:0.25", *stochastic_row("ancestral", lt, ls, 0.25), 0.0),
            ("ddim eta 0.5", *stochastic_row("ddim_eta", lt, ls, 1.0, 0.5), 0.0),
            ("sde first order", *stochastic_row("sde_dpmpp_2m", lt, ls), 0.0),
            ("sde second order", *stochastic_row("sde_dpmpp_2m", lt, ls), 0.37)]


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("mt", R.MEAN_TYPES)
@pytest.mark.parametrize("n,B", [(64, 1), (64, 5), (192, 5), (2052, 3)])          # 2052: three blocks of 1024 values, the last with 4
def test_step_kernel(n, B, mt, guided):
    from generative_models_amd import ops
    rng = np.random.default_rng(n + B)
    seed, offset = 77, 1000
    worst, thresholded = 0.0, False
    for lt, ls in ((-15.0, -2.5), (-2.5, 3.0), (3.0, 15.0)):
        v, z = dev(rng.standard_normal((B, n)).astype(np.float32)), dev(rng.standard_normal((B, n)).astype(np.float32))
        vu = dev(rng.standard_normal((B, n)).astype(np.float32)) if guided else None
        w = dev(rng.uniform(0.0, 4.0, (B,)).astype(np.float32)) if guided else None
        thr = dev(rng.uniform(1.0, 2.0, (B,)).astype(np.float32))
        prev = dev(rng.uniform(-1.0, 1.0, (B, n)).astype(np.float32))
        kw = dict(v_uncond=vu, cond_w=w, mean_type=mt)
        _, xp_s, ep_s = ops.sampler_step(v, z, lt, ls, False, want_pred=True, **kw)
        _, xp_t, ep_t = ops.sampler_step(v, z, lt, ls, False, want_pred=True, thr=thr, **kw)
        xi = ops.rng_normal((B, n), seed, offset, "cuda")                              # the fresh noise is gmk_rng_normal's at the same counters
        for name, c_z, c_x, c_n, k in rows_of(lt, ls):
            coef = (c_z, c_x, c_n, k)
            hist = prev.clone() if k else None
            z_next, xp, ep = ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=hist, want_pred=True, **kw)
            assert torch.equal(xp, xp_s) and torch.equal(ep, ep_s), name               # sampler_step's prediction, guidance included
            assert hist is None or torch.equal(hist, xp), name                         # x_hist takes this step's x-hat
            want = R.step(f64(z), f64(xp), f64(xi), *coef, x_prev=f64(prev))
            bound = R.step_bound(f64(z), f64(xp), f64(xi), *coef, x_prev=f64(prev))
            err = np.abs(f64(z_next) - want)
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), (n, B, mt, lt, ls, name, (err / bound).max())
            if k:       # the history is read: another one gives another z
                other = ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=torch.zeros_like(prev), **kw)[0]
                assert not torch.equal(other, z_next)
            else:       # and with k == 0 it is written but not read
                hist0 = torch.full_like(prev, float("nan"))
                assert torch.equal(ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=hist0, **kw)[0], z_next), name
                assert torch.equal(hist0, xp), name
            # the last step returns x-hat and draws nothing (any counter gives the same)
            hist = prev.clone() if k else None
            z_last, xp_l, _ = ops.stochastic_step(v, z, lt, ls, *coef, True, seed + 1, offset + 8, x_hist=hist, want_pred=True, **kw)
            assert torch.equal(z_last, xp_l) and torch.equal(xp_l, xp) and (hist is None or torch.equal(hist, xp)), name
            # with thr: the thresholded sampler_step's prediction
            hist = prev.clone() if k else None
            z_thr, xp2, ep2 = ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=hist, thr=thr, want_pred=True, **kw)
            assert torch.equal(xp2, xp_t) and torch.equal(ep2, ep_t), name
            thresholded |= not torch.equal(xp2, xp)          # (at logsnr -15 an eps net's x-hat saturates either way)
            bound_t = R.step_bound(f64(z), f64(xp2), f64(xi), *coef, x_prev=f64(prev))
            assert (np.abs(f64(z_thr) - R.step(f64(z), f64(xp2), f64(xi), *coef, x_prev=f64(prev))) <= bound_t).all(), name
            # a chunk of rows at its counter offset draws what the whole batch draws
            for a, b in ((0, B),) if B == 1 else ((0, 2), (2, B)):
                part = ops.stochastic_step(ops.aligned(v[a:b]), ops.aligned(z[a:b]), lt, ls, *coef, False, seed, offset, q0=a * n // 4,
                                           x_hist=ops.aligned(prev[a:b].clone()) if k else None,
                                           v_uncond=None if vu is None else ops.aligned(vu[a:b]), cond_w=None if w is None else ops.aligned(w[a:b]),
                                           mean_type=mt)[0]
                assert torch.equal(part, z_next[a:b]), (name, a, b)
            if name == "ancestral large":       # the existing, reference-checked ancestral update on the same noise
                z_old = ops.sampler_step(v, z, lt, ls, False, noise=xi, **kw)[0]
                err_old = np.abs(f64(z_next) - f64(z_old))
                assert (err_old <= 2 * bound).all(), (n, B, mt, lt, ls, (err_old / bound).max())
                assert not torch.equal(z_next, xp)
            if name == "ddim eta 0.5":          # noise reaches the result; with coef_noise = 0 nothing is drawn: any seed, the same bits
                quiet = ops.stochastic_step(v, z, lt, ls, c_z, c_x, 0.0, k, False, seed, offset, **kw)[0]
                assert torch.equal(quiet, ops.stochastic_step(v, z, lt, ls, c_z, c_x, 0.0, k, False, seed + 5, offset + 64, **kw)[0])
                assert not torch.equal(quiet, z_next)
                assert (np.abs(f64(quiet) - R.step(f64(z), f64(xp), None, c_z, c_x, 0.0)) <= bound).all()
        # z_dup and logsnr_next follow sampler_step's conventions
        name, *coef = rows_of(lt, ls)[-1]
        z_next = ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=prev.clone(), **kw)[0]
        lnext = torch.zeros((2 * B,), device="cuda")
        (zn, z2), _, _ = ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=prev.clone(), dup=True, logsnr_next=lnext, **kw)
        assert torch.equal(zn, z_next) and torch.equal(z2[:B], z_next) and torch.equal(z2[B:], z_next)
        assert torch.equal(lnext, torch.full((2 * B,), float(np.float32(ls)), device="cuda"))
        lnext1 = torch.zeros((B,), device="cuda")
        ops.stochastic_step(v, z, lt, ls, *coef, False, seed, offset, x_hist=prev.clone(), logsnr_next=lnext1, **kw)
        assert torch.equal(lnext1, lnext[:B])
        offset += 4096
    print(f"n = {n}, B = {B}, {mt}: largest z_next error over its bound {worst:.3f}")
    assert thresholded
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.stochastic_step(torch.zeros((B, 25), device="cuda"), torch.zeros((B, 25), device="cuda"), 0.0, 1.0, 0.5, 0.5, 0.1, 0.0, False, seed, 0)


# ---- the samplers -------------------------------------------------------------------------------------------------------------------------------
B4, S = 4, 8
SAMPLERS = {"ancestral": dict(sampler="ancestral"), "ancestral_small": dict(sampler="ancestral", posterior_var="small"),
            "ancestral_medium": dict(sampler="ancestral", posterior_var="medium:0.5"), "ddim_eta": dict(sampler="ddim", ddim_eta=0.5),
            "sde_dpmpp_2m": dict(sampler="sde_dpmpp_2m")}
OPTIONS = {"plain": ({}, False), "guided": ({}, True), "interval": (dict(guidance_interval=(-3.0, 30.0)), True),
           "cfg_rescale": (dict(cfg_rescale=0.7), True), "dyn_threshold": (dict(dyn_threshold=0.9), False)}


@pytest.fixture(scope="module")
def net():
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as UR
    net = SimpleUnet(32, 0.0, compute_dtype=torch.float32)
    net.load_state_dict(UR.reference_init_params(32, seed=1, zero_out_layers=False))
    return net.cuda().eval()


def _init(B=B4, C=1, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, C, S, S), generator=g).cuda(), torch.tensor([3, -1, 0, 9, 5, 1, 2, 7][:B]).cuda()


def _diffusion(num_steps=3, seed=11, **kw):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    return GaussianDiffusion(mean_type="v", num_steps=num_steps, seed=seed, **kw)


def _follows(plan, z0, zs, xs, seed, per, first=0):
    """Every recorded step against the restatement of ONE step on the recorded previous z and x-hats (nothing compounds); the noise is
    gmk_rng_normal's at the counter block the loop reserved for that evaluation."""
    from generative_models_amd import ops
    assert len(plan) == zs.shape[0]
    for k, step in enumerate(plan):
        c = step.sto
        z_in, x_prev = (z0 if k == 0 else zs[k - 1]), (None if k == 0 else f64(xs[k - 1]))
        assert (k > 0 or c.coef_prev == 0.0) and (c.lt, c.ls) == (float(step.lt), float(step.ls))
        xi = ops.rng_normal(tuple(z0.shape), seed, (first + k) * per, "cuda")
        args = (f64(z_in), f64(xs[k]), f64(xi), c.coef_z, c.coef_x, c.coef_noise, c.coef_prev)
        want = R.step(*args, x_prev=x_prev, is_last=step.is_last)
        err = np.abs(f64(zs[k]) - want)
        assert (err <= R.step_bound(*args, x_prev=x_prev)).all(), (k, (err / R.step_bound(*args, x_prev=x_prev)).max())
        assert float(xs[k].abs().max()) <= 1.0
    assert torch.equal(zs[-1], xs[-1]) and not torch.equal(zs[0], xs[0])


@pytest.mark.parametrize("option", sorted(OPTIONS))
@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_three_steps_follow_the_restatement(net, name, option):
    from generative_models_amd.diffusion.gaussian_diffusion import sampler_plan
    init, y = _init()
    extra, guided = OPTIONS[option]
    make = lambda: _diffusion(**SAMPLERS[name], **extra)
    kw = dict(cond_w=0.5, net_cond_w=torch.tensor([0.5, 1.0, 2.0, 3.5]).cuda()) if guided else {}
    d = make()
    zs, xs, es = d.sample(net=partial(net, guide=y), init_x=init, **kw)
    per = B4 * S * S // 4
    assert d.rng.counter == 3 * per and zs.shape == (3, B4, 1, S, S) and bool(torch.isfinite(es).all())
    plan = sampler_plan(3, SAMPLERS[name]["sampler"], posterior_var=SAMPLERS[name].get("posterior_var", "large"),
                        ddim_eta=SAMPLERS[name].get("ddim_eta", 0.0))
    assert (name != "sde_dpmpp_2m") == all(s.sto.coef_prev == 0.0 for s in plan)
    _follows(plan, init, zs, xs, d.rng.seed, per)
    # the same seed draws the same chain, another seed another one; record=False returns the last z
    assert torch.equal(make().sample(net=partial(net, guide=y), init_x=init, record=False, **kw)[0][-1], zs[-1])
    assert not torch.equal(_diffusion(**{**SAMPLERS[name], **extra, "seed": 12}).sample(net=partial(net, guide=y), init_x=init, **kw)[0][0], zs[0])


@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_edit_runs_the_tail_of_the_plan(net, name):
    """start = 2 (`edit` without a mask is the sampler from part-way): the rows i = 1, 0, the first of them without history."""
    from generative_models_amd.diffusion.gaussian_diffusion import sampler_plan
    init, y = _init()
    d = _diffusion(**SAMPLERS[name])
    zs, xs, _ = d.sample(net=partial(net, guide=y), init_x=init, start=2)
    per = B4 * S * S // 4
    assert zs.shape[0] == 2 and d.rng.counter == 2 * per
    plan = sampler_plan(3, SAMPLERS[name]["sampler"], start=2, posterior_var=SAMPLERS[name].get("posterior_var", "large"),
                        ddim_eta=SAMPLERS[name].get("ddim_eta", 0.0))
    _follows(plan, init, zs, xs, d.rng.seed, per)
    out = _diffusion(**SAMPLERS[name]).edit(net=partial(net, guide=y), x=init.clamp(-1, 1), start=2)[0][-1]
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0


def test_eta_zero_is_todays_ddim_and_one_step_is_ddim(net):
    init, y = _init()
    run = lambda d, **kw: d.sample(net=partial(net, guide=y), init_x=init, **kw)
    today = _diffusion(sampler="ddim")
    a, b = run(today), run(_diffusion(sampler="ddim", ddim_eta=0.0))
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and today.rng.counter == 0
    one = run(_diffusion(num_steps=1, sampler="ddim"))
    for name in sorted(SAMPLERS):
        d = _diffusion(num_steps=1, **SAMPLERS[name])
        got = run(d)
        assert all(torch.equal(s, t) for s, t in zip(got, one)) and got[0].shape == (1, B4, 1, S, S), name
    # eta = 1 is the ancestral sampler with the 'small' variance: the same counters, coefficients equal to a few float64 ulps
    a, b = run(_diffusion(sampler="ddim", ddim_eta=1.0))[0], run(_diffusion(sampler="ancestral", posterior_var="small"))[0]
    assert float((a[0] - b[0]).abs().max()) <= 1e-6 * float(b[0].abs().max())


@pytest.mark.parametrize("name", ["ancestral_medium", "ddim_eta", "sde_dpmpp_2m"])
def test_graph_path_and_chunks_give_the_whole_batchs_bits(net, name):
    init, y = _init()
    run = lambda d, i=init, yy=y: d.sample(net=partial(net, guide=yy), init_x=i, record=False)[0][-1]
    graphed, plain = (_diffusion(num_steps=16, seed=5, **SAMPLERS[name]) for _ in range(2))
    plain.GRAPH_MAX_PIXELS = 0
    assert graphed._graph_path(net, B4, S, S) and not plain._graph_path(net, B4, S, S)
    a, b = run(graphed), run(plain)
    assert torch.equal(a, b) and len(graphed._graphs) == 1 and not plain._graphs and bool(torch.isfinite(a).all())
    # two half-batches on two streams, each at its own Philox counter offset, against one batch on one stream
    init8, y8 = _init(B=8)
    two, one = (_diffusion(num_steps=3, seed=5, **SAMPLERS[name]) for _ in range(2))
    two.STREAM_MIN_PIXELS, one.SAMPLER_STREAMS = 0, 1
    seen = []
    chunk = two._sample_chunk
    two._sample_chunk = lambda *args, **kwargs: seen.append(args[9]) or chunk(*args, **kwargs)
    a, b = run(two, init8, y8), run(one, init8, y8)
    assert seen == [0, 4 * S * S // 4] and torch.equal(a, b)


def test_refused_combinations_raise(net):
    init, y = _init()
    ones = torch.ones((1, 1, S, S), device="cuda")
    for name, tag in (("ancestral_small", "ancestral"), ("sde_dpmpp_2m", "sde_dpmpp_2m"), ("ddim_eta", "ddim_eta")):
        d = _diffusion(**SAMPLERS[name])
        with pytest.raises(ValueError, match=tag + ".*inpainting"):
            d.inpaint(net=partial(net, guide=y), x0=init, mask=ones, init_x=init)
        with pytest.raises(ValueError, match=tag + ".*inpainting"):
            d.edit(net=partial(net, guide=y), x=init.clamp(-1, 1), start=2, mask=ones)
        with pytest.raises(ValueError, match=tag + ".*restoration"):
            d.restore(net=partial(net, guide=y), obs=torch.zeros((B4, 1, S // 2, S // 2), device="cuda"), factor=2, init_x=init)
        with pytest.raises(ValueError, match="noises"):
            d.sample(net=partial(net, guide=y), init_x=init, noises=torch.zeros((3,) + tuple(init.shape), device="cuda"))
        assert d.rng.counter == 0


# ---- the model and the command line ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SAMPLERS))
def test_model_samples_and_evaluates(name):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=4, seed=3, hidden_size=32, in_channels=1, timesteps=4, image_size=S, **SAMPLERS[name])
    torch.manual_seed(0)
    m = Model(G).to("cuda")
    d = m.diffusion
    assert (d.sampler, d.posterior_var, d.ddim_eta) == (G.sampler, G.posterior_var, G.ddim_eta)
    m.eval()
    out = m.sample(4, torch.tensor([1, 2, 3, 4]).cuda())
    assert out.shape == (4, 1, S, S) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    assert d.rng.counter > 0                                   # the chain drew its noise from the sampler's stream
    x = torch.rand(4, 1, S, S, device="cuda") * 2 - 1
    m.evaluate(None, x, torch.randint(0, 10, (4,), device="cuda"), 0)
    ev = m.last_eval
    assert ev["samples"].shape[1:] == (1, S, S) and ev["sampling_process"].shape[0] == 4


def test_cli_epoch(tmp_path):
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main", "--model=diffusion", "--epochs=1", "--hidden_size", "32", "--bs", "4",
                        "--train_batches", "2", "--test_batches", "1", "--sampler", "sde_dpmpp_2m", "--timesteps", "4", "--logdir",
                        str(tmp_path / "run")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "diffusion/train/loss" in r.stdout and "SAVED MODEL" in r.stdout
