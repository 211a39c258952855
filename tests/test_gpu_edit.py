"""GPU tests of SDEdit editing and latent interpolation (`GaussianDiffusion.edit` / `interpolate`, sampler chains that start part-way,
gmk_slerp, `DiffusionModel.edit` / `interpolate`, DG.edit_eval / DG.interp_eval; extensions): the slerp kernel against float64 and its
invariants, `start=T` against today's chain bit for bit, truncated chains and (masked) edits against the CPU restatement (tests/edit_ref.py)
on the paths of the sampler loop, the interpolation against the ODE restatement (tests/ode_ref.py), and the plugin surface."""
import os
import sys
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edit_ref  # noqa: E402
import ode_ref  # noqa: E402

TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def _ulp_err(a, b):
    """max |a - b| in units of b's fp32 spacing"""
    a, b = a.double().cpu(), b.double().cpu()
    spacing = torch.finfo(torch.float32).eps * torch.clamp(b.abs(), min=torch.finfo(torch.float32).tiny)
    return float(((a - b).abs() / spacing).max())


_NETS = {}


def make_net(dtype, C=128, seed=0):
    """Default-init scale with the zero-initialised out_layers.3 convs made live (the conditioning of test_gpu_inpaint.py); one per dtype."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    if (dtype, C, seed) not in _NETS:
        net = SimpleUnet(C, 0.0, compute_dtype=dtype)
        params = U.reference_init_params(C, 1, seed=seed, zero_out_layers=False)
        net.load_state_dict(params, strict=True)
        _NETS[(dtype, C, seed)] = (net.cuda().eval(), params)
    return _NETS[(dtype, C, seed)]


# ---- G1: the kernel against float64 ------------------------------------------------------------------------------------------------------
SLERP_SHAPES = [(5, 64, 3), (4, 784, 7), (3, 3072, 2), (2, 16384, 4), (1, 4, 1)]      # (B, n, K): fewer elements than threads, a row that is no
# multiple of the workgroup's 1024-value stride, an exact multiple, a row above the register-resident capacity, the minimum
T_POOL = [0.125, 1.0, 0.0, 0.5, 0.3, 0.77, 0.9]
COSINES = [-0.5, 0.0, 0.9, 0.9999]


def _slerp_rows(B, n, seed):
    """b = rho (c a + sqrt(1 - c^2) r), c cycling through COSINES from a row that depends on the seed, rho uniform in [0.5, 2]."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn((B, n), generator=g)
    r = torch.randn((B, n), generator=g)
    c = torch.tensor([COSINES[(seed + i) % 4] for i in range(B)])[:, None]
    rho = 0.5 + 1.5 * torch.rand((B, 1), generator=g)
    return a, (rho * (c * a + torch.sqrt(1 - c * c) * r)).float()


@pytest.mark.parametrize("shape", SLERP_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_slerp_kernel_against_float64(shape):
    from generative_models_amd import ops
    B, n, K = shape
    t = torch.tensor(T_POOL[:K])
    worst, worst_c = 0.0, 0.0
    for seed in range(4):                                          # every cosine in every row position
        a, b = _slerp_rows(B, n, seed)
        out, cos = ops.slerp(a.cuda(), b.cuda(), t.cuda(), want_cos=True)
        assert out.shape == (K, B, n) and cos.shape == (B,)
        ref, c_ref = edit_ref.slerp(a, b, t)
        worst = max(worst, float((out.cpu().double() - ref).abs().max() / ref.abs().max()))
        worst_c = max(worst_c, float((cos.cpu().double() - c_ref).abs().max()))
    print(f"slerp {shape}: max|out - ref| / max|ref| = {worst:.3e}, max|cos - c_ref| = {worst_c:.3e}")
    assert worst <= 2e-6 and worst_c <= 1e-6, (worst, worst_c)


def test_slerp_kernel_takes_image_shapes():
    from generative_models_amd import ops
    a, b = _slerp_rows(3, 3 * 8 * 8, 1)
    t = torch.tensor([0.25, 0.5]).cuda()
    flat = ops.slerp(a.cuda(), b.cuda(), t)
    img = ops.slerp(a.cuda().view(3, 3, 8, 8), b.cuda().view(3, 3, 8, 8), t)
    assert img.shape == (2, 3, 3, 8, 8) and torch.equal(img.view(2, 3, -1), flat)


# ---- G2: the kernel's invariants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 64), (3, 3072), (2, 12288), (2, 16384)], ids=lambda s: "x".join(map(str, s)))
def test_slerp_endpoints_are_exact_and_calls_repeat(shape):
    from generative_models_amd import ops
    B, n = shape
    a, b = _slerp_rows(B, n, 2)
    a, b = a.cuda(), b.cuda()
    t = torch.tensor([0.0, 1.0, 0.37]).cuda()
    out, cos = ops.slerp(a, b, t, want_cos=True)
    assert torch.equal(out[0], a) and torch.equal(out[1], b)
    again, cos2 = ops.slerp(a, b, t, want_cos=True)
    assert torch.equal(out, again) and torch.equal(cos, cos2)


def test_slerp_falls_back_to_lerp():
    """a == b, an all-zero a, b == -a: the lerp (1 - t) a + t b, finite everywhere; the first two within 2 ulps of it."""
    from generative_models_amd import ops
    g = torch.Generator().manual_seed(3)
    n = 784
    a = torch.randn((4, n), generator=g)
    b = torch.randn((4, n), generator=g)
    b[0] = a[0]                                                    # parallel (identical)
    a[1] = 0.0                                                     # the cosine is 0 / 0
    b[2] = -a[2]                                                   # antipodal
    t = torch.tensor([0.0, 0.125, 0.5, 0.75, 1.0])
    out, cos = ops.slerp(a.cuda(), b.cuda(), t.cuda(), want_cos=True)
    assert bool(torch.isfinite(out).all())
    want = edit_ref.lerp(a, b, t)
    for row in (0, 1):
        assert _ulp_err(out[:, row], want[:, row]) <= 2.0, (row, _ulp_err(out[:, row], want[:, row]))
    assert torch.equal(out[0], a.cuda()) and torch.equal(out[-1], b.cuda())
    assert float(cos[0]) == 1.0 and float(cos[2]) == -1.0 and bool(torch.isnan(cos[1]))
    assert _ulp_err(out[:, 2], want[:, 2]) <= 2.0 or float((out[:, 2].cpu().double() - want[:, 2]).abs().max()) <= 1e-6 * float(a[2].abs().max())
    ref, _ = edit_ref.slerp(a, b, t)                               # row 3 is an ordinary pair
    assert float((out[:, 3].cpu().double() - ref[:, 3]).abs().max()) <= 2e-6 * float(ref[:, 3].abs().max())


# ---- G3: start = T is today's chain ------------------------------------------------------------------------------------------------------
def _case(B=3, S=8, seed=11):
    g = torch.Generator().manual_seed(seed)
    init = torch.randn((B, 1, S, S), generator=g)
    x0 = torch.rand((B, 1, S, S), generator=g) * 2 - 1
    y = torch.tensor([1, 7, 3, 5, 2, 8][:B])
    return init.cuda(), x0.cuda(), y.cuda()


@pytest.mark.parametrize("sampler", ["ddim", "noisy", "dpmpp_2m"])
@pytest.mark.parametrize("guided", [False, True])
def test_start_T_is_sample(sampler, guided):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = make_net(torch.float32)
    init, _, y = _case()
    cw = 0.5 if guided else None
    mk = lambda: GaussianDiffusion(mean_type="v", num_steps=5, sampler=sampler, sample_cond_w=-1.0, seed=3)
    a = mk().sample(net=partial(net, guide=y), init_x=init, cond_w=cw)
    b = mk().sample(net=partial(net, guide=y), init_x=init, cond_w=cw, start=5)
    for p, q in zip(a, b):
        assert p.shape == q.shape and torch.equal(p, q)
    last = mk().sample(net=partial(net, guide=y), init_x=init, cond_w=cw, start=5, record=False)[0][-1]
    assert torch.equal(last, a[0][-1])


# ---- G4: truncated chains against the restatement ----------------------------------------------------------------------------------------
def _chain_draws(d, B, shape, k, guided, sampler):
    """The draws a chain of k evaluations makes from d.rng, at the documented counters: net_cond_w = 4 U[0, 1) [B] first when guided, then one
    normal tensor per evaluation ('noisy')."""
    from generative_models_amd import ops
    n = B * int(torch.tensor(shape).prod())
    c0, w = 0, None
    if guided:
        w = (4.0 * ops.rng_uniform((B,), d.rng.seed, 0, "cuda")).cpu()
        c0 = (B + 3) // 4
    noises = None
    if sampler == "noisy":
        noises = [ops.rng_normal((B,) + shape, d.rng.seed, c0 + f * n // 4, "cuda").cpu() for f in range(k)]
    return w, noises


def _step_tol(dtype, guided):
    """The per-step bars of test_gpu_inpaint.py: fp32 1e-3 (5e-3 guided), 16-bit mode 3e-2 (no exception: k < T never starts at logsnr -20)."""
    return (5 if guided else 1) * TOL[dtype] if dtype == torch.float32 else 3 * TOL[dtype]


_REF = {}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("mean_type", ["v", "eps"])
@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("sampler", ["ddim", "noisy", "dpmpp_2m"])
def test_truncated_chain_vs_restatement(sampler, k, mean_type, guided, dtype):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, T = 3, 8, 6
    net, params = make_net(dtype)
    eps, x0, y = _case(B, S)
    init = edit_ref.noised(x0.cpu(), eps.cpu(), k, T).float()                  # z at logsnr(k / T)
    d = GaussianDiffusion(mean_type=mean_type, num_steps=T, sampler=sampler, sample_cond_w=-1.0, seed=9)
    assert not d._graph_path(net, 2 * B if guided else B, S, S)
    key = (sampler, k, mean_type, guided)
    if key not in _REF:
        w, noises = _chain_draws(d, B, (1, S, S), k, guided, sampler)
        with torch.no_grad():
            _REF[key] = edit_ref.sample(params, init, y.cpu(), T, k, sampler, cond_w=w, noises=noises, mean_type=mean_type)
    zs_ref, xs_ref, _ = _REF[key]
    zs, xs, es = d.sample(net=partial(net, guide=y), init_x=init.cuda(), cond_w=0.5 if guided else None, start=k)
    assert zs.shape == zs_ref.shape == xs.shape == es.shape == (k, B, 1, S, S)
    tol = _step_tol(dtype, guided)
    errs = [(rel_err(zs[j], zs_ref[j]), rel_err(xs[j], xs_ref[j])) for j in range(k)]
    assert all(ez < tol and ex < tol for ez, ex in errs), errs
    assert torch.equal(zs[-1], xs[-1])                                          # the last step returns x_hat


# ---- G5: edit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "noisy", "dpmpp_2m"])
@pytest.mark.parametrize("guided", [False, True])
def test_edit_noises_then_samples(sampler, guided):
    """z_k = alpha x + sigma eps with eps the stream's first draw, then exactly sample(init_x=z_k, start=k); another seed, another result."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, sampler_plan
    B, S, T, k, seed = 3, 8, 5, 3, 17
    net, _ = make_net(torch.float32)
    _, x, y = _case(B, S)
    cw = 0.5 if guided else None
    mk = lambda: GaussianDiffusion(mean_type="v", num_steps=T, sampler=sampler, sample_cond_w=-1.0, seed=3)
    eps = ops.rng_normal(tuple(x.shape), seed, 0, "cuda")
    lt = sampler_plan(T, start=k)[0].lt
    z_k = ops.q_sample_logsnr(x, eps, torch.full((B,), float(lt), device="cuda"))
    assert rel_err(z_k, edit_ref.noised(x.cpu(), eps.cpu(), k, T)) <= 1e-6
    got = mk().edit(net=partial(net, guide=y), x=x, start=k, cond_w=cw, seed=seed, record=True)
    want = mk().sample(net=partial(net, guide=y), init_x=z_k, cond_w=cw, start=k)
    for p, q in zip(got, want):
        assert p.shape == q.shape and p.shape[0] == k and torch.equal(p, q)
    last = mk().edit(net=partial(net, guide=y), x=x, start=k, cond_w=cw, seed=seed)
    assert last[1] is None and torch.equal(last[0][-1], got[0][-1])
    other = mk().edit(net=partial(net, guide=y), x=x, start=k, cond_w=cw, seed=seed + 1)[0][-1]
    assert not torch.equal(other, got[0][-1])


def test_edit_on_the_graph_path_vs_restatement():
    """T = 16 at 8 x 8: the forward replays a captured graph; the chain starts at k = 8."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, T, k, seed = 3, 8, 16, 8, 5
    net, params = make_net(torch.float32)
    _, x, y = _case(B, S)
    d = GaussianDiffusion(mean_type="v", num_steps=T, sampler="ddim")
    assert d._graph_path(net, B, S, S)
    zs, xs, _ = d.edit(net=partial(net, guide=y), x=x, start=k, seed=seed, record=True)
    assert len(d._graphs) == 1 and zs.shape[0] == k
    eps = ops.rng_normal(tuple(x.shape), seed, 0, "cuda").cpu()
    with torch.no_grad():
        _, (zs_ref, xs_ref, _) = edit_ref.edit(params, x.cpu(), eps, y.cpu(), T, k, "ddim")
    ez, ex = rel_err(zs, zs_ref), rel_err(xs, xs_ref)
    assert ez < 1e-3 and ex < 1e-3, (ez, ex)


def test_edit_two_streams_are_bit_identical():
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
    x = (torch.rand((B, 1, S, S), generator=g) * 2 - 1).cuda()
    outs = []
    for streams in (1, 2):
        d = GaussianDiffusion(mean_type="v", num_steps=4, sampler="ddim", seed=11)
        d.SAMPLER_STREAMS = streams
        assert (B // 2) * S * S >= d.STREAM_MIN_PIXELS
        outs.append(d.edit(net=partial(net, guide=y), x=x, start=3, seed=4, record=True))
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.equal(a, b)
    assert bool(torch.isfinite(outs[0][0]).all())


# ---- G6: masked edit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sampler", ["ddim", "noisy"])
def test_masked_edit_vs_restatement(sampler):
    """The top half is known: it comes back as x itself, and the chain is the restatement's with the RePaint merge, its draws following eps
    on PhiloxStream(seed): merge f at counter ceil(B n / 4) + f B n / 2."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    B, S, T, k, seed = 3, 8, 6, 4, 21
    net, params = make_net(torch.float32)
    _, x, y = _case(B, S)
    mask = torch.zeros((1, 1, S, 1), dtype=torch.uint8)
    mask[:, :, : S // 2] = 1
    d = GaussianDiffusion(mean_type="v", num_steps=T, sampler=sampler, seed=9)
    zs, xs, _ = d.edit(net=partial(net, guide=y), x=x, start=k, mask=mask.cuda(), seed=seed, record=True)
    known = mask.cuda().bool().expand_as(x)
    assert zs.shape[0] == k and torch.equal(zs[-1][known], x[known])
    assert not torch.equal(zs[-1][~known], x[~known])
    n = B * S * S
    shape = (B, 1, S, S)
    eps = ops.rng_normal(shape, seed, 0, "cuda").cpu()
    q = (n + 3) // 4
    eps1 = [ops.rng_normal(shape, seed, q + f * n // 2, "cuda").cpu() for f in range(k)]
    _, noises = _chain_draws(d, B, (1, S, S), k, False, sampler)
    with torch.no_grad():
        _, (zs_ref, xs_ref, _) = edit_ref.edit(params, x.cpu(), eps, y.cpu(), T, k, sampler, noises=noises, mask=mask.bool(), eps1=eps1)
    errs = [(rel_err(zs[j], zs_ref[j]), rel_err(xs[j], xs_ref[j])) for j in range(k)]
    assert all(ez < 1e-3 and ex < 1e-3 for ez, ex in errs), errs


# ---- G7: interpolate ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_interpolate_against_the_oracle(dtype):
    """N = 4, B = 2, K = 3: the latents against ode_ref.encode followed by the float64 slerp, the frames against ode_ref.decode of the
    package's own latents (so that the encoder's error does not compound), at test_ode_against_the_oracle's bars."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, ode_logsnr_grid
    from oracle import unet_ref as U
    net, params = make_net(dtype, seed=2)
    B, N, K, S = 2, 4, 3, 8
    bar = 1e-3 if dtype == torch.float32 else 1e-2
    g = torch.Generator().manual_seed(8)
    xa = torch.rand((B, 1, S, S), generator=g) * 2 - 1
    xb = torch.rand((B, 1, S, S), generator=g) * 2 - 1
    y = torch.tensor([1, -1])
    d = GaussianDiffusion(mean_type="v", num_steps=N)
    frames, lat = d.interpolate(net=partial(net, guide=y.cuda()), xa=xa.cuda(), xb=xb.cuda(), frames=K, num_steps=N, return_latents=True)
    assert frames.shape == lat.shape == (K, B, 1, S, S) and frames.dtype == torch.float32
    only = d.interpolate(net=partial(net, guide=y.cuda()), xa=xa.cuda(), xb=xb.cuda(), frames=K, num_steps=N)
    assert torch.equal(only, frames)
    lam = ode_logsnr_grid(N)

    def fwd_for(labels):
        def fwd(zz, l):
            with torch.no_grad():
                return U.unet_forward(params, zz.float(), torch.full((zz.shape[0],), float(l)), guide=labels).double()
        return fwd
    za = ode_ref.encode(fwd_for(y), xa, N, "v", lam=lam)
    zb = ode_ref.encode(fwd_for(y), xb, N, "v", lam=lam)
    lat_ref, _ = edit_ref.slerp(za, zb, [k / (K - 1) for k in range(K)])
    e_lat = rel_err(lat, lat_ref)
    # the end frames are the codes themselves: one encode of cat([xa, xb]) with the guide repeated
    assert torch.equal(lat[0], d.encode(net=partial(net, guide=y.cuda().repeat(2)), x=torch.cat([xa, xb]).cuda(), num_steps=N)[:B])
    dec_ref = torch.stack([ode_ref.decode(fwd_for(y), lat[k].cpu(), N, "v", lam=lam) for k in range(K)])
    e_dec = rel_err(frames, dec_ref)
    print(f"interpolate {dtype}: latents {e_lat:.3e}, frames {e_dec:.3e}")
    assert e_lat <= bar and e_dec <= bar, (e_lat, e_dec)
    # chunks of whole frames (here one frame per decode, the guide tiled once) give the frames of one decode, up to the bar: a forward's
    # bits may depend on its batch size
    d.INTERP_MAX_BATCH = B
    chunked = d.interpolate(net=partial(net, guide=y.cuda()), xa=xa.cuda(), xb=xb.cuda(), frames=K, num_steps=N)
    assert chunked.shape == frames.shape and rel_err(chunked, frames) <= bar


def test_interpolate_raises():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = make_net(torch.float32)
    x = torch.zeros((2, 1, 8, 8), device="cuda")
    y = torch.tensor([1, -1]).cuda()
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    with pytest.raises(ValueError, match="frames"):
        d.interpolate(net=partial(net, guide=y), xa=x, xb=x, frames=1, num_steps=4)
    with pytest.raises(ValueError, match="differs"):
        d.interpolate(net=partial(net, guide=y), xa=x, xb=x[:1], frames=3, num_steps=4)
    with pytest.raises(ValueError, match="cond_w"):
        d.interpolate(net=partial(net, guide=y, cond_w=torch.ones((2,), device="cuda")), xa=x, xb=x, frames=3, num_steps=4)
    student = GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=net, teacher_mode="step1")
    with pytest.raises(ValueError, match="distilled"):
        student.interpolate(net=partial(net, guide=y), xa=x, xb=x, frames=3, num_steps=4)


# ---- G8: the plugin ----------------------------------------------------------------------------------------------------------------------
def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", timesteps=4, bs=8, hidden_size=128, image_size=8, seed=3)
    G.update(flags)
    torch.manual_seed(0)                                                        # the same initial weights
    return Model(G).to("cuda")


def _batch(B=12, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand((B, 1, 8, 8), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()


def test_evaluate_edit_and_interp_eval():
    x, y = _batch()
    runs = {}
    for name, flags in (("parent", {}), ("off", {"edit_eval": 0.0, "interp_eval": 0}), ("on", {"edit_eval": 0.5, "interp_eval": 3})):
        model = _model(**flags)
        model.eval()
        model.evaluate(None, x, y.clone(), 0)
        runs[name] = (model.last_eval, model._aux_rng.counter, model.diffusion.rng.counter)
    parent, off, on = runs["parent"], runs["off"], runs["on"]
    assert set(parent[0]) == set(off[0]) == {"samples", "sampling_process", "eps", "x"}
    assert parent[1:] == off[1:] == on[1:]                                      # the flags draw from streams of their own
    for k in parent[0]:
        assert torch.equal(parent[0][k], off[0][k]) and torch.equal(parent[0][k], on[0][k]), k
    assert set(on[0]) == set(parent[0]) | {"edit", "interp"}
    edit, interp = on[0]["edit"], on[0]["interp"]
    assert edit.dtype == torch.uint8 and edit.shape == (12, 1, 8, 8)
    assert interp.dtype == torch.uint8 and interp.shape == (3, 5, 1, 8, 8)
    few = _model(edit_eval=0.5, interp_eval=3)
    few.eval()
    few.evaluate(None, x[:8], y[:8].clone(), 0)                                # fewer than 10 test images: no interpolation
    assert few.last_eval["edit"].shape == (8, 1, 8, 8) and "interp" not in few.last_eval
    # the edit is the documented call on the documented stream
    model = _model(edit_eval=0.5)
    model.eval()
    model.evaluate(None, x, y.clone(), 0)
    from generative_models_amd import ops
    ref = model.diffusion.edit(net=partial(model.net, guide=y), x=x, start=2, seed=model.EDIT_EVAL_SEED)[0][-1]
    assert torch.equal(model.last_eval["edit"], ops.to_uint8(ref).cpu())


def test_edit_and_interpolate_use_the_ema_net():
    from generative_models_amd.diffusion.gaussian_diffusion import edit_start
    m = _model(ema_decay=0.9)
    m.train()
    for s in range(3):
        m.train_step(*_batch(8, seed=10 + s))
    m.eval()
    x, y = _batch(6)
    k = edit_start(0.6, 4)
    assert k == 2
    mask = torch.zeros((1, 1, 8, 8), dtype=torch.bool, device="cuda")
    mask[..., :4, :] = True
    for kw in ({}, {"mask": mask}):
        counter = m.diffusion.rng.counter
        got = m.edit(x, 0.6, y=y, seed=3, **kw)
        assert got.shape == x.shape and bool(torch.isfinite(got).all())
        assert m.diffusion.rng.counter == counter + (6 + 3) // 4                # the guidance draw, as in sample()
        m.diffusion.rng.counter = counter
        on_ema = m.diffusion.edit(net=partial(m.ema_net, guide=y), x=x, start=k, cond_w=0.5, seed=3, **kw)[0][-1]
        m.diffusion.rng.counter = counter
        on_raw = m.diffusion.edit(net=partial(m.net, guide=y), x=x, start=k, cond_w=0.5, seed=3, **kw)[0][-1]
        assert torch.equal(got, on_ema) and not torch.equal(got, on_raw)
        if kw:
            assert torch.equal(got[mask.expand_as(x)], x[mask.expand_as(x)])
    plain = m.edit(x, 0.6, seed=3)                                              # no labels: unguided, nothing drawn from diffusion.rng
    assert torch.equal(plain, m.diffusion.edit(net=partial(m.ema_net, guide=None), x=x, start=k, seed=3)[0][-1])
    xa, xb = x[:3], x[3:]
    guide = torch.full((3,), -1, dtype=torch.long, device="cuda")
    frames = m.interpolate(xa, xb, frames=3)
    assert frames.shape == (3, 3, 1, 8, 8)
    assert torch.equal(frames, m.diffusion.interpolate(net=partial(m.ema_net, guide=guide), xa=xa, xb=xb, frames=3, num_steps=4))
    assert not torch.equal(frames, m.diffusion.interpolate(net=partial(m.net, guide=guide), xa=xa, xb=xb, frames=3, num_steps=4))
    lab = m.interpolate(xa, xb, frames=2, y=y[:3], steps=3)
    assert torch.equal(lab, m.diffusion.interpolate(net=partial(m.ema_net, guide=y[:3]), xa=xa, xb=xb, frames=2, num_steps=3))
