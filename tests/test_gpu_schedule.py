"""GPU tests of the parametrised noise schedules: gmk_q_sample_sched and gmk_logsnr_schedule_sched against the reference's own fp32 output
(tests/golden/logsnr_schedules.npz) and the restatement of tests/schedule_ref.py, the default arguments against the original entries bit for
bit, the schedule through `GaussianDiffusion` (training pass, distillation, samplers, edit) and through `DiffusionModel`'s five flags.

Measured on an MI355X, gmk_q_sample_sched's log-SNR against the reference's (elementwise max |got - ref| / max(1, |ref|) over n, ranges and
shifts): cosine 1.0e-07, uniform 0, beta_const 9.5e-08, beta_linear 9.5e-08 - rounding of logf / tanf / expm1f, two orders under the bar."""
import os
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref  # noqa: E402
import schedule_ref as R  # noqa: E402

F = np.float32
T = torch.from_numpy
BAR = 1e-5                      # test_q_sample_and_loss's bar on rel_err
HOST_BAR = 2e-6                 # |got - ref| <= 2e-6 max(1, |ref|): two fp32 evaluations of the same steps (tests/test_host_schedule.py)
CHAIN_BAR = 1e-3                # the fp32 chain bar of test_sampler_vs_oracle


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t).tobytes()


def dev(a):
    from generative_models_amd import ops
    return ops.aligned(T(np.ascontiguousarray(a)).cuda())


def G():
    from generative_models_amd.diffusion import gaussian_diffusion
    return gaussian_diffusion


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


_NETS = {}


def make_net(C=32):
    """SimpleUnet(C) in the fp32 mode at default-init scale with the zero-initialised convolutions made live, and the same weights for the oracle."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    if C not in _NETS:
        net = SimpleUnet(C, 0.0, compute_dtype=torch.float32)
        params = U.reference_init_params(C, 1, zero_out_layers=False)
        net.load_state_dict(params, strict=True)
        _NETS[C] = (net.cuda(), params)
    return _NETS[C]


# ---- gmk_q_sample_sched ----------------------------------------------------------------------------------------------------------------------
Q_U = np.array([0.0, 0.03, 0.4, 0.999, 1.0], dtype=F)
Q_N = (25, 1026, 3072)          # a scalar tail with rows that are not 16-byte aligned; a tail inside the second workgroup; three workgroups per image


@pytest.mark.parametrize("kind", R.KINDS)
def test_q_sample_sched_against_the_reference(gold, kind):
    from generative_models_amd import ops
    g = G()
    gu = gold["u"]
    rows = [int(np.flatnonzero(gu == v)[0]) for v in Q_U]               # the golden's own u values: nothing is interpolated
    B = len(Q_U)
    gen = torch.Generator().manual_seed(7)
    worst = 0.0
    for n in Q_N:
        x = torch.rand((B, n), generator=gen) * 2 - 1
        eps = torch.randn((B, n), generator=gen)
        xd, ed, ud = dev(x.numpy()), dev(eps.numpy()), dev(Q_U)
        for lo, hi in ((-20.0, 20.0), (-10.0, 20.0)):
            base = gold[R.golden_key(kind, lo, hi)][rows]
            for shift in (0.0, -1.386):
                ref = (base + F(shift)).astype(F) if shift else base
                logsnr, z = ops.q_sample(xd, ed, ud, schedule=g.Schedule(kind, lo, hi, shift))
                assert logsnr.shape == (B,) and z.shape == (B, n)
                el = float(np.max(np.abs(logsnr.cpu().numpy().astype(np.float64) - ref) / np.maximum(1.0, np.abs(ref))))
                worst = max(worst, el)
                assert rel_err(logsnr, T(ref)) < BAR, (kind, n, lo, hi, shift, logsnr.cpu().numpy(), ref)
                assert rel_err(z, R.q_sample64(x, eps, ref)) < BAR, (kind, n, lo, hi, shift)
    print(f"gmk_q_sample_sched {kind}: max |logsnr - ref| / max(1, |ref|) = {worst:.3e}")
    assert worst <= BAR


@pytest.mark.parametrize("n", [100, 3072])
def test_default_arguments_give_the_old_kernels_bits(gold, n):
    from generative_models_amd import ops
    g = G()
    u = gold["u"][:64]                                                  # 0, 1 and both ends of the curve among them
    gen = torch.Generator().manual_seed(n)
    x, eps = dev((torch.rand((64, n), generator=gen) * 2 - 1).numpy()), dev(torch.randn((64, n), generator=gen).numpy())
    l0, z0 = ops.q_sample(x, eps, dev(u))
    l1, z1 = ops.q_sample(x, eps, dev(u), schedule=g.Schedule())
    assert bits(l0) == bits(l1) and bits(z0) == bits(z1)
    assert bool(torch.isfinite(l0).all()) and float(l0.max()) == 20.0


# ---- gmk_logsnr_schedule_sched ---------------------------------------------------------------------------------------------------------------
STEPS = 4
U_SHIFTS = (0.0, 1.0 / STEPS, 0.5 / STEPS)


def _schedule_inputs(gold):
    """(u, i_times, num_steps, u_shift) calls: every golden u unshifted, the part of it that stays in [0, 1] shifted, and the integer path."""
    gu = gold["u"]
    late = np.ascontiguousarray(gu[gu >= 0.25])
    i = np.array([0, 1, 2, 3, 3, 0, 2], dtype=np.int64)
    return [(gu, None, 1, 0.0)] + [(late, None, 1, s) for s in U_SHIFTS[1:]] + [(None, i, STEPS, s) for s in U_SHIFTS]


def test_schedule_entry_default_arguments_give_the_old_kernels_bits(gold):
    from generative_models_amd import ops
    g = G()
    for u, i, steps, s in _schedule_inputs(gold):
        B = len(u) if u is not None else len(i)
        kw = dict(u=None if u is None else dev(u), i_times=None if i is None else dev(i), num_steps=steps, shift=s, want_u=True)
        l0, u0 = ops.logsnr_schedule(B, "cuda", **kw)
        l1, u1 = ops.logsnr_schedule(B, "cuda", schedule=g.Schedule(), **kw)
        assert bits(l0) == bits(l1) and bits(u0) == bits(u1) and bool(torch.isfinite(l0).all())
        assert bits(ops.logsnr_schedule(B, "cuda", schedule=g.Schedule(), **dict(kw, want_u=False))) == bits(l0)


@pytest.mark.parametrize("kind", R.KINDS)
def test_schedule_entry_against_the_restatement(gold, kind):
    from generative_models_amd import ops
    g = G()
    for lo, hi, shift in ((-20.0, 20.0, 0.0), (-10.0, 20.0, -1.386)):
        S = g.Schedule(kind, lo, hi, shift)
        for u, i, steps, s in _schedule_inputs(gold):
            B = len(u) if u is not None else len(i)
            l, uo = ops.logsnr_schedule(B, "cuda", u=None if u is None else dev(u), i_times=None if i is None else dev(i), num_steps=steps, shift=s,
                                        want_u=True, schedule=S)
            uu = ((i + 1).astype(F) / F(steps) if u is None else u) - F(s)
            assert uu.dtype == F and bits(uo) == bits(uu)
            ref = R.logsnr32(kind, lo, hi, shift, uu).astype(np.float64)
            got = l.cpu().numpy().astype(np.float64)
            assert np.all(np.abs(got - ref) <= HOST_BAR * np.maximum(1.0, np.abs(ref))), (kind, lo, hi, shift, s, got, ref)
            if i is not None and s == 1.0 / STEPS:                      # i = 0 is u = 0, the top of the range
                assert uu[0] == 0.0 and abs(got[0] - (hi + shift)) <= HOST_BAR * 20


# ---- through GaussianDiffusion ---------------------------------------------------------------------------------------------------------------
def _train_inputs(B=4):
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand((B, 1, 8, 8), generator=gen) * 2 - 1).cuda()
    y = torch.tensor([3, -1, 7, 0][:B]).cuda()
    u = torch.tensor([0.02, 0.35, 0.71, 0.995][:B]).cuda()
    eps = torch.randn((B, 1, 8, 8), generator=gen).cuda()
    return x, y, u, eps


def test_training_pass_is_the_three_calls_by_hand():
    from generative_models_amd import ops
    g = G()
    net, _ = make_net()
    x, y, u, eps = _train_inputs()
    B = x.shape[0]
    side = ops.WGRAD_STREAM
    ops.WGRAD_STREAM = False
    try:
        S = g.Schedule("beta_linear", -15.0, 15.0, -0.5)
        out = g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=S).train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, u=u, eps=eps)
        logsnr, z = ops.q_sample(x, eps, u, schedule=S)
        v = net.forward_hip(z, logsnr, y, None)
        loss = ops.v_loss(v, z, x, eps, logsnr, grad_scale=1.0 / B, loss_type=0, mean_type="v")[0]
        assert bits(out["logsnr"]) == bits(logsnr) and bits(out["loss"]) == bits(loss)
        want = R.logsnr32("beta_linear", -15.0, 15.0, -0.5, u.cpu().numpy())
        assert np.all(np.abs(logsnr.cpu().numpy() - want) <= HOST_BAR * np.maximum(1.0, np.abs(want)))
        assert bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(net.flat_grads).all())
        # Schedule() is the run that passes no schedule at all
        plain = g.GaussianDiffusion(mean_type="v", num_steps=4).train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, u=u, eps=eps)
        grads = net.flat_grads.clone()
        dflt = g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=g.Schedule()).train_forward_backward(net=partial(net, guide=y), x=x,
                                                                                                            grad_scale=1.0 / B, u=u, eps=eps)
        assert bits(plain["logsnr"]) == bits(dflt["logsnr"]) and bits(plain["loss"]) == bits(dflt["loss"]) and bits(grads) == bits(net.flat_grads)
        assert bits(plain["logsnr"]) != bits(out["logsnr"])
    finally:
        ops.WGRAD_STREAM = side


def test_distillation_follows_the_training_schedule():
    from generative_models_amd import ops
    g = G()
    net, _ = make_net()
    teacher, _ = make_net()
    x, y, _, eps = _train_inputs()
    B = x.shape[0]
    S = g.Schedule("beta_const", -20.0, 20.0, 0.0)
    i_times = torch.tensor([0, 1, 2, 3]).cuda()
    w = torch.tensor([0.0, 1.0, 2.5, 3.9]).cuda()
    side = ops.WGRAD_STREAM
    ops.WGRAD_STREAM = False
    try:
        d = g.GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="step2", schedule=S)
        prep = d._prepare(partial(net, guide=y), x, None, eps, i_times=i_times, cond_w=w)
        logsnr = prep[4].cpu().numpy()
        want = np.array([S.host(g.sampler_times(i, 4)[0]) for i in range(4)])
        assert np.all(np.abs(logsnr - want) <= HOST_BAR * np.maximum(1.0, np.abs(want))), (logsnr, want)
        assert all(bool(torch.isfinite(t).all()) for t in prep[3:7])
        out = d.train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, eps=eps, i_times=i_times, cond_w=w)
        assert bits(out["logsnr"]) == bits(prep[4]) and bool(torch.isfinite(out["loss"]).all())
    finally:
        ops.WGRAD_STREAM = side


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp_2m"])
def test_sampler_walks_the_sampling_schedule(sampler):
    g = G()
    net, params = make_net()
    B, steps = 2, 4
    gen = torch.Generator().manual_seed(11)
    init = torch.randn((B, 1, 8, 8), generator=gen)
    y = torch.tensor([1, 7])
    sched = ("uniform", -20.0, 20.0, 0.0)
    d = g.GaussianDiffusion(mean_type="v", num_steps=steps, sampler=sampler, sample_schedule=g.Schedule(*sched))
    assert d.schedule is None
    zs, xs, es = d.sample(net=partial(net, guide=y.cuda()), init_x=init.cuda())
    with torch.no_grad():
        zs_ref, xs_ref, _ = R.chain(sched, init, steps, sampler_ref.oracle_step(params, y, sampler))
    assert zs.shape == zs_ref.shape
    print(f"{sampler} on the uniform grid: z {rel_err(zs, zs_ref):.3e}, x-hat {rel_err(xs, xs_ref):.3e}")
    assert rel_err(zs, zs_ref) < CHAIN_BAR and rel_err(xs, xs_ref) < CHAIN_BAR
    # the grid matters: the default curve gives another chain
    plain = g.GaussianDiffusion(mean_type="v", num_steps=steps, sampler=sampler).sample(net=partial(net, guide=y.cuda()), init_x=init.cuda())[0]
    assert rel_err(plain, zs_ref) > 10 * CHAIN_BAR


def test_edit_starts_on_the_sampling_schedule():
    from generative_models_amd import ops
    g = G()
    net, params = make_net()
    B, steps, k = 2, 4, 2
    sched = ("uniform", -20.0, 20.0, 0.0)
    S = g.Schedule(*sched)
    gen = torch.Generator().manual_seed(13)
    x = (torch.rand((B, 1, 8, 8), generator=gen) * 2 - 1).cuda()
    y = torch.tensor([1, 7])
    d = g.GaussianDiffusion(mean_type="v", num_steps=steps, sample_schedule=S)
    out = d.edit(net=partial(net, guide=y.cuda()), x=x, start=k, seed=3, record=True)
    lt = S.host(g.sampler_times(k - 1, steps)[0])
    assert float(lt) == 0.0                                              # uniform on [-20, 20] at u = 2 / 4
    eps = ops.rng_normal(tuple(x.shape), 3, 0, "cuda")
    z_k = ops.q_sample_logsnr(x, eps, torch.full((B,), float(lt), device="cuda"))
    by_hand = d.sample(net=partial(net, guide=y.cuda()), init_x=z_k, start=k)
    assert out[0].shape[0] == k and all(bits(a) == bits(b) for a, b in zip(out, by_hand))
    with torch.no_grad():
        zs_ref, _, _ = R.chain(sched, z_k.cpu(), steps, sampler_ref.oracle_step(params, y, "ddim"), start=k)
    assert rel_err(out[0], zs_ref) < CHAIN_BAR


# ---- through DiffusionModel ------------------------------------------------------------------------------------------------------------------
def _model(argv, **flags):
    from generative_models_amd import main
    Gf, Model = main.FlagSpace(main.DG).resolve(["--model=diffusion"] + argv)
    Gf.update(lr=1e-3, pad32=0, device="cuda", bs=8, seed=3, hidden_size=32, in_channels=1, image_size=8, compute_dtype="fp32", **flags)
    torch.manual_seed(0)
    return Model(Gf).to("cuda").train()


ARGV = ["--logsnr_schedule", "beta_linear", "--logsnr_shift", "-0.5", "--sample_logsnr_schedule", "uniform", "--timesteps", "4"]


@pytest.mark.parametrize("profiled", [0, 1], ids=["graphed-step", "loss-profile"])
def test_model_trains_and_samples_under_the_flags(tmp_path, profiled):
    from generative_models_amd import main
    g = G()
    m = _model(ARGV, loss_profile=profiled)
    S = g.Schedule("beta_linear", -20.0, 20.0, -0.5)
    assert m.diffusion.schedule == S and m.diffusion.sample_schedule == g.Schedule("uniform", -20.0, 20.0, -0.5) and m.diffusion.num_steps == 4
    gen = torch.Generator().manual_seed(5)
    x = (torch.rand((8, 1, 8, 8), generator=gen) * 2 - 1).cuda()
    y = torch.randint(0, 10, (8,), generator=gen).cuda()
    # the same images at the same times and noise before and after the two steps: the loss there must not rise (beyond the fp32 mode's 1e-3)
    u = ((torch.arange(8) + 0.5) / 8).cuda()
    eps = torch.randn((8, 1, 8, 8), generator=gen).cuda()
    probe = lambda: float(m.diffusion.training_losses(net=partial(m.net, guide=y), x=x, u=u, eps=eps)["loss"].mean())
    with torch.no_grad():
        before = probe()
    losses = [float(m.train_step(x, y.clone())["loss"]) for _ in range(2)]
    with torch.no_grad():
        after = probe()
    print(f"train losses {losses}, fixed-probe loss {before} -> {after}")
    assert all(np.isfinite(losses)) and np.isfinite(before) and np.isfinite(after)
    assert after <= before * (1.0 + 1e-3)
    m.eval()
    img = m.sample(2, torch.tensor([3, 4]).cuda())
    assert img.shape == (2, 1, 8, 8) and bool(torch.isfinite(img).all()) and float(img.abs().max()) <= 1.0
    if not profiled:
        assert m.diffusion.profile("train") is None
        return
    rows = m.diffusion.profile("train")
    assert 0.0 < rows["weight"].sum() <= 16.0                            # two steps of 8 images, the first decayed by importance_decay
    path = main.append_loss_profile(tmp_path, 1, "train", rows)
    lines = path.read_text().splitlines()
    table = [dict(zip(lines[0].split(","), ln.split(","))) for ln in lines[1:]]
    assert len(table) == 64
    u_lo, u_hi = np.arange(64, dtype=F) / F(64), np.arange(1, 65, dtype=F) / F(64)
    assert [F(r["logsnr_hi"]) for r in table] == list(S.host(u_lo)) and [F(r["logsnr_lo"]) for r in table] == list(S.host(u_hi))
    assert F(table[0]["logsnr_hi"]) == F(19.5) and abs(F(table[-1]["logsnr_lo"]) - F(-20.5)) < 1e-4
