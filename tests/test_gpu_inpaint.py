"""GPU tests of RePaint inpainting (`GaussianDiffusion.inpaint`, gmk_inpaint_merge, `DiffusionModel.inpaint`, DG.inpaint_eval; an extension):
the merge kernel against a torch restatement, the empty and the full mask, whole chains against the CPU restatement (tests/inpaint_ref.py) on
the paths of the sampler loop - kernel by kernel, the captured-graph forward, two half-batch streams, the guided 2B batch - the plugin
surface, and the completion it is there for."""
import os
import sys
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import inpaint_ref  # noqa: E402

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def make_net(dtype, C=128, seed=0):
    """Default-init scale with the zero-initialised out_layers.3 convs made live (the conditioning of test_gpu_dpm_solver.py)."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    net = SimpleUnet(C, 0.0, compute_dtype=dtype)
    params = U.reference_init_params(C, 1, seed=seed, zero_out_layers=False)
    net.load_state_dict(params, strict=True)
    return net.cuda().eval(), params


# ---- G1: the kernel ----------------------------------------------------------------------------------------------------------------------
def _merge_case(B=6, shape=(3, 8, 8), seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    z = torch.randn((B,) + shape, device="cuda", generator=g)
    x0 = torch.rand((B,) + shape, device="cuda", generator=g) * 2 - 1
    mask = (torch.rand((B,) + shape, device="cuda", generator=g) < 0.5).to(torch.uint8)
    mask[0] = 0                                                    # rows without / with only known pixels too
    mask[1] = 1
    return z, x0, mask


def _ulp_err(a, b):
    """max |a - b| in units of b's fp32 spacing"""
    a, b = a.double(), b.double()
    spacing = torch.finfo(torch.float32).eps * torch.clamp(b.abs(), min=torch.finfo(torch.float32).tiny)
    return float(((a - b).abs() / spacing).max())


@pytest.mark.parametrize("renoise,is_last", [(False, False), (True, False), (False, True)])
@pytest.mark.parametrize("dup", [False, True])
def test_merge_kernel_against_torch(renoise, is_last, dup):
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import inpaint_coefs
    B, shape = 6, (3, 8, 8)
    n = 3 * 8 * 8
    z, x0, mask = _merge_case(B, shape)
    rows = inpaint_coefs(10)
    c = rows[-1] if is_last else rows[3]
    seed, off = 1234567, 77
    eps1 = ops.rng_normal((B,) + shape, seed, off, "cuda")                       # the documented counters
    eps2 = ops.rng_normal((B,) + shape, seed, off + B * n // 4, "cuda")
    known = x0 if is_last else c.alpha_s * x0 + c.sigma_s * eps1
    sel = torch.where(mask.bool(), known, z)
    want = c.a * sel + c.b * eps2 if renoise else sel
    out = z.clone()
    z2 = torch.full((B,) + shape, float("nan"), device="cuda") if dup else None
    ln = torch.full((2 * B if dup else B,), float("nan"), device="cuda")
    ops.inpaint_merge(out, x0, mask.reshape(B, -1), c.alpha_s, c.sigma_s, c.a, c.b, is_last, renoise, c.lt, c.ls, seed, off, z_dup=z2,
                      logsnr_next=ln)
    m = mask.bool()
    if not renoise:
        assert torch.equal(out[~m], z[~m])                                      # unknown pixels keep z's bits
        if is_last:
            assert torch.equal(out[m], x0[m])                                   # the last step puts x0 itself
        else:
            assert _ulp_err(out[m], known[m]) <= 2.0
    else:
        assert _ulp_err(out, want) <= 4.0 or rel_err(out, want) < 1e-6
    if dup:
        assert torch.equal(z2, out)
    assert torch.equal(ln.cpu(), torch.full(ln.shape, float(c.lt if renoise else c.ls), dtype=torch.float32))


def test_merge_kernel_draws_match_rng_normal_exactly():
    """Known pixels at alpha_s = 0, sigma_s = 1 are eps1 itself; a jump with a = 0, b = 1 writes eps2: both bit for bit what gmk_rng_normal
    stores at the documented counters (the in-kernel Box-Muller is rng_kernel's)."""
    from generative_models_amd import ops
    B, shape, seed, off = 4, (1, 16, 16), 99, 1000
    n = 256
    x0 = torch.zeros((B,) + shape, device="cuda")
    z = torch.zeros_like(x0)
    ones = torch.ones((B, n), dtype=torch.uint8, device="cuda")
    ops.inpaint_merge(z, x0, ones, 0.0, 1.0, 1.0, 0.0, False, False, -1.0, 1.0, seed, off)
    assert torch.equal(z, ops.rng_normal((B,) + shape, seed, off, "cuda"))
    ops.inpaint_merge(z, x0, torch.zeros_like(ones), 0.0, 1.0, 0.0, 1.0, False, True, -1.0, 1.0, seed, off)
    assert torch.equal(z, ops.rng_normal((B,) + shape, seed, off + B * n // 4, "cuda"))


@pytest.mark.parametrize("renoise", [False, True])
def test_merge_kernel_half_batches_draw_what_the_batch_draws(renoise):
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import inpaint_coefs
    B, shape = 6, (3, 8, 8)
    n = 192
    z, x0, mask = _merge_case(B, shape, seed=8)
    c = inpaint_coefs(10)[4]
    args = (c.alpha_s, c.sigma_s, c.a, c.b, False, renoise, c.lt, c.ls, 4242, 31)
    whole = z.clone()
    ops.inpaint_merge(whole, x0, mask.reshape(B, -1), *args)
    parts = z.clone()
    for a, b in ((0, 2), (2, 6)):
        zz = parts[a:b]
        ops.inpaint_merge(zz, x0[a:b].contiguous(), mask[a:b].reshape(b - a, -1).contiguous(), *args, q0=a * n // 4, B_total=B)
    assert torch.equal(whole, parts)


# ---- G2 / G3: the empty and the full mask ------------------------------------------------------------------------------------------------
def _case(B=3, S=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    init = torch.randn((B, 1, S, S), generator=g)
    x0 = torch.rand((B, 1, S, S), generator=g) * 2 - 1
    y = torch.tensor([1, 7, 3, 5, 2, 8][:B])
    return init.cuda(), x0.cuda(), y.cuda()


@pytest.mark.parametrize("sampler", ["ddim", "noisy", "dpmpp_2m"])
@pytest.mark.parametrize("guided", [False, True])
def test_empty_mask_is_sample(sampler, guided):
    """Nothing known, r = 1: every merge is a select of z_gen - the trajectory is sample()'s, bit for bit (same draws from self.rng)."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = make_net(torch.float32)
    init, x0, y = _case()
    cw = 0.5 if guided else None
    mk = lambda: GaussianDiffusion(mean_type="v", num_steps=5, sampler=sampler, sample_cond_w=-1.0, seed=3)
    a = mk().sample(net=partial(net, guide=y), init_x=init, cond_w=cw)
    b = mk().inpaint(net=partial(net, guide=y), x0=x0, mask=torch.zeros((1,), dtype=torch.bool), init_x=init, cond_w=cw, record=True)
    for p, q in zip(a, b):
        assert p.shape == q.shape and torch.equal(p, q)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("resample", [1, 3])
def test_full_mask_ends_on_x0(dtype, resample):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = make_net(dtype)
    init, x0, y = _case()
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    out = d.inpaint(net=partial(net, guide=y), x0=x0, mask=torch.ones_like(x0), init_x=init, resample=resample)[0][-1]
    assert torch.equal(out, x0)


# ---- G4: chains against the CPU restatement ----------------------------------------------------------------------------------------------
def _draws(d, B, shape, T, r, seed, guided):
    """The draws `inpaint` makes: net_cond_w (guided) then one 'noisy' noise per evaluation from d.rng; eps1 / eps2 per merge from
    PhiloxStream(seed) - at the counters the package documents, drawn with ops.rng_normal / ops.rng_uniform."""
    from generative_models_amd import ops
    n = B * int(torch.tensor(shape).prod())
    F = inpaint_ref.forwards(T, r)
    c0 = 0
    w = None
    if guided:
        w = 4.0 * ops.rng_uniform((B,), d.rng.seed, 0, "cuda")
        c0 = (B + 3) // 4
    noises = [ops.rng_normal((B,) + shape, d.rng.seed, c0 + f * n // 4, "cuda").cpu() for f in range(F)]
    eps1 = [ops.rng_normal((B,) + shape, seed, f * n // 2, "cuda").cpu() for f in range(F)]
    eps2 = [ops.rng_normal((B,) + shape, seed, f * n // 2 + n // 4, "cuda").cpu() for f in range(F)]
    return (None if w is None else w.cpu()), noises, eps1, eps2


_REF = {}
CHAINS = [("ddim", 1), ("ddim", 3), ("noisy", 1), ("noisy", 3), ("dpmpp_2m", 1)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("mean_type", ["v", "eps"])
@pytest.mark.parametrize("sampler,resample", CHAINS)
def test_chain_vs_restatement(sampler, resample, mean_type, guided, dtype):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, T, seed = 3, 8, 4, 21
    net, params = make_net(dtype)
    init, x0, y = _case(B, S)
    mask = torch.zeros((1, 1, S, 1), dtype=torch.uint8)
    mask[:, :, : S // 2] = 1                                                  # the top half is known
    d = GaussianDiffusion(mean_type=mean_type, num_steps=T, sampler=sampler, sample_cond_w=-1.0, seed=9)
    assert not d._graph_path(net, 2 * B if guided else B, S, S)              # T < 16: kernel by kernel
    key = (sampler, resample, mean_type, guided)
    if key not in _REF:
        w, noises, eps1, eps2 = _draws(d, B, (1, S, S), T, resample, seed, guided)
        with torch.no_grad():
            _REF[key] = inpaint_ref.sample(params, init.cpu(), x0.cpu(), mask.bool(), y.cpu(), T, sampler, cond_w=w, resample=resample,
                                           eps1=eps1, eps2=eps2, noises=noises, mean_type=mean_type)
    zs_ref, xs_ref, es_ref = _REF[key]
    zs, xs, es = d.inpaint(net=partial(net, guide=y), x0=x0, mask=mask.cuda(), init_x=init, cond_w=0.5 if guided else None,
                           resample=resample, seed=seed, record=True)
    assert zs.shape == zs_ref.shape == xs.shape == es.shape
    # the bars of test_sampler_vs_oracle / test_gpu_dpm_solver.py's chain test, per step: fp32 1e-3 (5e-3 guided), 16-bit mode 3e-2
    tol = (5 if guided else 1) * TOL[dtype] if dtype == torch.float32 else 3 * TOL[dtype]
    errs = [(rel_err(zs[k], zs_ref[k]), rel_err(xs[k], xs_ref[k])) for k in range(T)]
    tols = [(tol, tol) for _ in range(T)]
    if guided and dtype != torch.float32 and resample == 1:
        # The first step's x_hat in 16-bit mode, guided: at logsnr_t = -20, x_hat = clip((z - sigma_t eps_w) / alpha_t) multiplies the guided
        # eps_w = (1 + w) eps - w eps_u, and with it the 16-bit forward's error, by (1 + 2 w) / alpha_t, 9 e^10 ~ 2e5 at the drawn w ~ 4 (the
        # sampler tests' weights stay below 3.2); pixels inside the clip band then differ by up to 4.2e-2 of the largest (measured).  No merge
        # has acted yet: with r = 1 that x_hat is sample()'s own, bit for bit, and every later step and every z is held to the bar (with r > 1
        # the step's last pass starts from a re-noised z and meets the bar).
        tols[0] = (tol, 6e-2)
        ref_first = GaussianDiffusion(mean_type=mean_type, num_steps=T, sampler=sampler, sample_cond_w=-1.0, seed=9).sample(
            net=partial(net, guide=y), init_x=init, cond_w=0.5)[1][0]
        assert torch.equal(xs[0], ref_first)
    assert all(ez < tz and ex < tx for (ez, ex), (tz, tx) in zip(errs, tols)), errs
    known = mask.cuda().bool().expand_as(x0)
    assert torch.equal(zs[-1][known], x0[known])


def test_graph_path_vs_restatement():
    """T = 16 at 8 x 8: the forward replays a captured graph; resample 2 (31 evaluations)."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, T, r, seed = 3, 8, 16, 2, 5
    net, params = make_net(torch.float32)
    init, x0, y = _case(B, S)
    mask = torch.zeros((1, 1, S, 1), dtype=torch.uint8)
    mask[:, :, : S // 2] = 1
    d = GaussianDiffusion(mean_type="v", num_steps=T, sampler="ddim")
    assert d._graph_path(net, B, S, S)
    zs, xs, _ = d.inpaint(net=partial(net, guide=y), x0=x0, mask=mask.cuda(), init_x=init, resample=r, seed=seed, record=True)
    assert len(d._graphs) == 1
    _, _, eps1, eps2 = _draws(d, B, (1, S, S), T, r, seed, False)
    with torch.no_grad():
        zs_ref, xs_ref, _ = inpaint_ref.sample(params, init.cpu(), x0.cpu(), mask.bool(), y.cpu(), T, "ddim", resample=r, eps1=eps1,
                                               eps2=eps2)
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    assert ez < 1e-3 and ex < 1e-3, (ez, ex)
    last = d.inpaint(net=partial(net, guide=y), x0=x0, mask=mask.cuda(), init_x=init, resample=r, seed=seed)[0][-1]
    assert torch.equal(last, zs[-1])


# ---- G5: two streams ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler,resample,cond_w", [("ddim", 1, None), ("ddim", 1, 0.5), ("noisy", 2, None)])
def test_two_streams_are_bit_identical(sampler, resample, cond_w):
    """A batch above STREAM_MIN_PIXELS at hidden 128 runs as two half-batches on two streams, each merging its rows at its own counter
    offset q0: every recorded tensor must be the same bits as on one stream."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    B, S = 8192, 8
    torch.manual_seed(0)
    net = SimpleUnet(128, 0.0, compute_dtype=torch.bfloat16)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if ".out_layers.3.weight" in name:
                p.uniform_(-0.02, 0.02)
    net = net.cuda().eval()
    g = torch.Generator().manual_seed(2)
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    init = torch.randn((B, 1, S, S), generator=g).cuda()
    x0 = (torch.rand((B, 1, S, S), generator=g) * 2 - 1).cuda()
    mask = (torch.rand((B, 1, S, S), generator=g) < 0.5).cuda()
    outs = []
    for streams in (1, 2):
        d = GaussianDiffusion(mean_type="v", num_steps=3, sampler=sampler, seed=11)
        d.SAMPLER_STREAMS = streams
        assert (B // 2) * S * S >= d.STREAM_MIN_PIXELS
        outs.append(d.inpaint(net=partial(net, guide=y), x0=x0, mask=mask, init_x=init, cond_w=cond_w, resample=resample, seed=4,
                              record=True))
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all())


# ---- G6: the plugin ----------------------------------------------------------------------------------------------------------------------
def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=6, bs=8)
    G.update(flags)
    return Model(G).to("cuda")


def test_plugin_inpaint():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    model = _model(ema_decay=0.999)
    model.eval()
    x = torch.rand(5, 1, 28, 28, device="cuda") * 2 - 1
    y = torch.randint(0, 10, (5,), device="cuda")
    mask = torch.zeros((1, 1, 28, 28), dtype=torch.bool, device="cuda")
    mask[..., :14, :] = True
    counter = model._aux_rng.counter
    out = model.inpaint(x, mask, y=y, resample=2, seed=3)
    assert out.shape == x.shape and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    known = mask.expand_as(x)
    assert torch.equal(out[known], x[known])
    assert not torch.equal(out[~known], x[~known])
    # the EMA net, the initial noise from _aux_rng, guidance with cond_w = 0.5 as in sample()
    assert model.optimizer.ema_seeded
    init = model._aux_rng.__class__(model._aux_rng.seed)
    init.counter = counter
    noise = init.normal(tuple(x.shape), "cuda")
    d = GaussianDiffusion(mean_type="v", num_steps=6, sample_cond_w=-1.0, seed=model.diffusion.rng.seed)
    d.rng.counter = model.diffusion.rng.counter - (5 + 3) // 4                # the guidance draw inpaint made
    ref = d.inpaint(net=partial(model.ema_net, guide=y), x0=x, mask=mask, init_x=noise, cond_w=0.5, resample=2, seed=3)[0][-1]
    assert torch.equal(out, ref)


def test_evaluate_inpaint_eval():
    x = torch.rand(8, 1, 28, 28, device="cuda") * 2 - 1
    y = torch.randint(0, 10, (8,), device="cuda")
    evs = []
    for flag in (0, 2):
        torch.manual_seed(0)                                                    # the same initial weights
        model = _model(inpaint_eval=flag)
        model.eval()
        model.evaluate(None, x, y.clone(), 0)
        evs.append(model.last_eval)
    off, on = evs
    assert "inpaint" not in off
    for k in ("samples", "sampling_process", "eps", "x"):
        assert torch.equal(off[k], on[k]), k                                   # everything evaluate() made before is unchanged
    img = on["inpaint"]
    assert img.dtype == torch.uint8 and img.shape == (8, 1, 28, 28)
    proc = ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8).cpu()
    assert torch.equal(img[..., :14, :], proc[..., :14, :])


# ---- G7: the completion it is there for --------------------------------------------------------------------------------------------------
def test_completes_the_right_mode():
    """Trained on two images only, the net completes each one's top half with its own bottom half.  The resample count and the bar come
    from tools/inpaint_probe.py (c) (profiles/inpaint_probe.txt); the seeds are fixed."""
    model = inpaint_ref.train_two_mode(_model)
    right, uncond = inpaint_ref.completion_accuracy(model, inpaint_ref.LEARNING_CHECK_R)
    assert right >= 0.9, (right, uncond)
    assert 0.2 <= uncond <= 0.8, uncond                                         # without the known half the net draws both modes
