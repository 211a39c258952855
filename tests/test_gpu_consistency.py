"""GPU tests of consistency distillation and the multistep consistency sampler (extensions; Song et al. 2023, "Consistency Models", Algorithms
2 and 1): gmk_consistency_target, gmk_x_loss_huber and gmk_consistency_step bit for bit against the entries whose device functions they share
and elementwise against the float64 restatement (tests/consistency_ref.py), the training mode composed by hand from public ops, the sampler
against the restatement and across its launch paths, and the model and command line.

The elementwise bounds count fp32 operations; u = 2^-24 is the unit roundoff.  alpha and sigma come from `logsnr_coef`-style expressions (expf
within one ulp, a sum, a correctly rounded quotient and root): at most 3 half-ulps each, i.e. 3 u relative.
  eps*     16 u (|z_t| + |x*|) / sigma_t     c2 = alpha at 3 u, the product x* c2 (u), the difference (u of at most |z_t| + |x*|), c1 = 1 / sigma at 3 u,
                                             the last product (u): under 9 u (|z_t| + |x*|) / sigma_t, rounded up to 16
  z_next   8 u (|x_hat| + |eps|)             alpha_s, sigma_s rounded once from double (u each), two products (u each), one sum (u): 3 u (|x_hat| + |eps|)
  Huber    2 n u relative on loss_b + c      the n-term fp32 sum of squares; dv: the same relative bound times |dv|, plus 4 u max|dv|
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
import consistency_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
U = R.U24
C_HUBER = 0.00054
SHAPES = [(64, 1), (64, 5), (192, 1), (192, 5), (25, 1), (25, 5)]          # 1 x 8 x 8, 3 x 8 x 8, and the scalar path


def dev(a):
    from generative_models_amd import ops
    return ops.aligned(T(np.ascontiguousarray(a)).cuda())


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def lams(B, lo=-15.0, hi=15.0):
    """B log-SNRs spread over [lo, hi] as the kernels see them (fp32); one image: `lo` (the tests call it with three in turn)."""
    return np.linspace(lo, hi, B).astype(np.float32) if B > 1 else np.array([lo], dtype=np.float32)


def off1(a):
    """The same values one float past a 16-byte boundary: the scalar path at any n."""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 5, device="cuda")
    view = buf[1:1 + a.size].view(*a.shape)
    view.copy_(T(a))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


# ---- gmk_consistency_target --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", R.MEAN_TYPES)
@pytest.mark.parametrize("n,B", SHAPES)
def test_target_kernel(n, B, mt):
    from generative_models_amd import ops
    for lo in ((-15.0,) if B > 1 else (-15.0, 1.5, 14.0)):
        lt = lams(B, lo, 14.0)
        ls = (lt + np.float32(1.0)).astype(np.float32)
        i_np = np.array([0, 3, 0, 1, 7][:B] if B > 1 else [0 if lo < 0 else 2], dtype=np.int64)
        v, z_s, xp, z_t = R.target_inputs(B, n, lt.astype(np.float64), ls.astype(np.float64), seed=n + B)
        v_d, zs_d, xp_d, zt_d, lt_d, ls_d, i_d = dev(v), dev(z_s), dev(xp), dev(z_t), dev(lt), dev(ls), dev(i_np)
        xs, es = ops.consistency_target(v_d, zs_d, xp_d, zt_d, lt_d, ls_d, i_d, mean_type=mt)
        first = T(i_np == 0).cuda()
        # x*: ddim_step_vec's x_pred for (v_tgt, z_s, logsnr_s) away from the boundary, the teacher's prediction on it - bit for bit
        x_ddim = ops.ddim_step_vec(v_d, zs_d, ls_d, ls_d, mean_type=mt)[1]
        assert torch.equal(xs[~first], x_ddim[~first]) and torch.equal(xs[first], xp_d[first])
        # eps*: distill_target's closing expression (its i == 0 rows hold the same x*)
        e_dist = ops.distill_target(zs_d, zt_d, xp_d, lt_d, ls_d, i_d)[1]
        assert torch.equal(es[first], e_dist[first])
        # eps* against the float64 formula on the kernel's own x*
        want = R.eps_from_x(z_t, f64(xs), lt.astype(np.float64))
        sigma = R.alpha_sigma(lt.astype(np.float64), 2)[1]
        bound = 16 * U * (np.abs(z_t.astype(np.float64)) + np.abs(f64(xs))) / sigma
        err = np.abs(f64(es) - want)
        print(f"n = {n}, B = {B}, {mt}: largest eps* error over its bound {(err / bound).max():.3f}")
        assert (err <= bound).all(), (n, B, mt, (err / bound).max())
        # x* itself against the restatement: away from a clip edge the two agree to the rounding of alpha z - sigma out
        xs_ref = R.consistency_target(v, z_s, xp, z_t, lt.astype(np.float64), ls.astype(np.float64), i_np, mt)[0]
        gain = {"v": 1.0, "eps": np.sqrt(1.0 + np.exp(-ls.astype(np.float64)))[:, None], "x": 1.0}[mt]
        assert (np.abs(f64(xs) - xs_ref) <= 16 * U * gain * (np.abs(z_s) + np.abs(v) + 1.0)).all()
        # the 16-byte and the scalar path give the same bits, and so does a second call
        xs2, es2 = ops.consistency_target(off1(v), zs_d, xp_d, zt_d, lt_d, ls_d, i_d, mean_type=mt)
        xs3, es3 = ops.consistency_target(v_d, zs_d, xp_d, zt_d, lt_d, ls_d, i_d, mean_type=mt)
        assert torch.equal(xs2, xs) and torch.equal(es2, es) and torch.equal(xs3, xs) and torch.equal(es3, es)


# ---- gmk_x_loss_huber ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mt", R.MEAN_TYPES)
@pytest.mark.parametrize("n,B", SHAPES + [(3072, 2), (16384, 2)])
def test_huber_kernel(n, B, mt):
    """Residuals of at least 0.1 and some clipped elements (tests/loss_weight_ref.loss_inputs); 16384 > GMK_X_LOSS_KEEP re-reads the image."""
    from generative_models_amd import ops
    assert ops.X_LOSS_KEEP == 12288
    gs = 0.37
    for lo in ((-15.0,) if B > 1 else (-15.0, 1.5, 15.0)):
        lam = lams(B, lo, 15.0)
        out, z, x, _ = R.loss_inputs(B, n, lam.astype(np.float64), mt, seed=n + B)
        v_d, z_d, x_d, l_d = dev(out), dev(z), dev(x), dev(lam)
        loss_b, x_mse, dv = ops.x_loss_huber(v_d, z_d, x_d, l_d, C_HUBER, grad_scale=gs, mean_type=mt)
        assert torch.equal(x_mse, ops.x_loss_w(v_d, z_d, x_d, l_d, "min_snr", 5.0, mean_type=mt)[1])          # x_loss_w's x_mse, bit for bit
        c32 = float(np.float32(C_HUBER))                                                                      # the c the kernel sees
        ref = R.x_loss_huber(out, z, x, lam.astype(np.float64), c32, grad_scale=gs, mean_type=mt)
        rel = 2 * n * U
        err_l = np.abs((f64(loss_b) + c32) - (ref["loss_b"] + c32)) / (ref["loss_b"] + c32)
        g, gr = f64(dv).reshape(B, -1), ref["dv"].reshape(B, -1)
        bound = rel * np.abs(gr) + 4 * U * np.abs(gr).max(1, keepdims=True)
        err_g = np.abs(g - gr)
        print(f"n = {n}, B = {B}, {mt}: loss_b + c relative error {err_l.max():.2e} of {rel:.2e} allowed, "
              f"largest dv error over its bound {np.where(bound > 0, err_g / np.maximum(bound, 1e-300), 0).max():.3f}")
        assert (err_l <= rel).all(), (n, B, mt, err_l)
        assert (err_g <= bound).all(), (n, B, mt)
        assert (g[ref["clipped"].reshape(B, -1)] == 0.0).all() and ref["clipped"].any()
        plain = ops.x_loss_huber(v_d, z_d, x_d, l_d, C_HUBER, mean_type=mt)                                   # without dv: the same bits
        assert plain[2] is None and torch.equal(plain[0], loss_b) and torch.equal(plain[1], x_mse)
        if n % 4 == 0:                                                                                        # scalar path: the same bits
            other = ops.x_loss_huber(off1(out), z_d, x_d, l_d, C_HUBER, grad_scale=gs, mean_type=mt)
            assert all(torch.equal(a, b) for a, b in zip(other, (loss_b, x_mse, dv)))


def test_huber_of_a_zero_residual_is_zero():
    from generative_models_amd import ops
    x = torch.rand((3, 64), device="cuda") * 1.8 - 0.9
    l = dev(lams(3))
    loss_b, x_mse, dv = ops.x_loss_huber(x.clone(), torch.randn_like(x), x, l, C_HUBER, grad_scale=1.0, mean_type="x")
    assert float(loss_b.abs().max()) == 0.0 and float(x_mse.abs().max()) == 0.0 and float(dv.abs().max()) == 0.0


# ---- gmk_consistency_step ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
@pytest.mark.parametrize("mt", R.MEAN_TYPES)
@pytest.mark.parametrize("n,B", [(64, 1), (64, 5), (192, 1), (192, 5)])
def test_step_kernel(n, B, mt, guided):
    from generative_models_amd import ops
    rng = np.random.default_rng(n + B)
    seed, offset = 77, 1000
    for lt, ls in ((-15.0, -2.5), (-2.5, 3.0), (3.0, 15.0)):
        v, z = dev(rng.standard_normal((B, n)).astype(np.float32)), dev(rng.standard_normal((B, n)).astype(np.float32))
        vu = dev(rng.standard_normal((B, n)).astype(np.float32)) if guided else None
        w = dev(rng.uniform(0.0, 4.0, (B,)).astype(np.float32)) if guided else None
        kw = dict(v_uncond=vu, cond_w=w, mean_type=mt)
        z_next, xp, ep = ops.consistency_step(v, z, lt, ls, False, seed, offset, want_pred=True, **kw)
        _, xp_s, ep_s = ops.sampler_step(v, z, lt, ls, False, want_pred=True, **kw)
        assert torch.equal(xp, xp_s) and torch.equal(ep, ep_s)                         # sampler_step's prediction, guidance included
        z_last, xp_l, _ = ops.consistency_step(v, z, lt, ls, True, seed, offset, want_pred=True, **kw)
        assert torch.equal(z_last, xp_l) and torch.equal(xp_l, xp)
        # the fresh noise is gmk_rng_normal's at the same counters
        eps = ops.rng_normal((B, n), seed, offset, "cuda")
        want = R.consistency_step(f64(xp), f64(eps), np.float32(ls), False)
        bound = 8 * U * (np.abs(f64(xp)) + np.abs(f64(eps)))
        err = np.abs(f64(z_next) - want)
        assert (err <= bound).all(), (n, B, mt, lt, ls, (err / bound).max())
        assert not torch.equal(z_next, xp) and (ls > 5.0 or float((z_next - xp).abs().max()) > 0.01)      # (sigma_s = 5.5e-4 at logsnr 15)
        # a chunk of rows at its counter offset draws what the whole batch draws
        for a, b in ((0, B),) if B == 1 else ((0, 2), (2, B)):
            rows = ops.consistency_step(ops.aligned(v[a:b]), ops.aligned(z[a:b]), lt, ls, False, seed, offset, q0=a * n // 4,
                                        v_uncond=None if vu is None else ops.aligned(vu[a:b]), cond_w=None if w is None else ops.aligned(w[a:b]),
                                        mean_type=mt)[0]
            assert torch.equal(rows, z_next[a:b]), (a, b)
        # z_dup and logsnr_next follow sampler_step's conventions
        lnext = torch.zeros((2 * B,), device="cuda")
        (zn, z2), _, _ = ops.consistency_step(v, z, lt, ls, False, seed, offset, dup=True, logsnr_next=lnext, **kw)
        assert torch.equal(zn, z_next) and torch.equal(z2[:B], z_next) and torch.equal(z2[B:], z_next)
        assert torch.equal(lnext, torch.full((2 * B,), float(np.float32(ls)), device="cuda"))
        lnext1 = torch.zeros((B,), device="cuda")
        ops.consistency_step(v, z, lt, ls, False, seed, offset, logsnr_next=lnext1, **kw)
        assert torch.equal(lnext1, lnext[:B])
        offset += 4096
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.consistency_step(torch.zeros((B, 25), device="cuda"), torch.zeros((B, 25), device="cuda"), 0.0, 1.0, False, seed, 0)


# ---- the training mode --------------------------------------------------------------------------------------------------------------------------
B4, S = 4, 8


def _net(seed, dropout=0.0, scale=1.0):
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as UR
    net = SimpleUnet(32, dropout, compute_dtype=torch.float32)
    net.load_state_dict({k: scale * v for k, v in UR.reference_init_params(32, seed=seed, zero_out_layers=False).items()})
    return net.cuda()


@pytest.fixture(scope="module")
def batch():
    g = torch.Generator().manual_seed(9)
    x = (torch.rand((B4, 1, S, S), generator=g) * 2 - 1).cuda()
    y = torch.tensor([3, -1, 0, 9]).cuda()
    eps = torch.randn((B4, 1, S, S), generator=g).cuda()
    cond_w = (4.0 * torch.rand((B4,), generator=g)).cuda()
    return x, y, eps, cond_w


def _composed(diff, student, teacher, target, batch, i_times, gs, huber):
    """A train_forward_backward under teacher_mode 'consistency', from public ops.  -> (loss_b, flat_grads)"""
    from generative_models_amd import ops
    x, y, eps, cond_w = batch
    N = diff.train_grid
    _, u = ops.logsnr_schedule(B4, x.device, i_times=i_times, num_steps=N, want_u=True)
    logsnr, z_t = ops.q_sample(x, eps, u)
    logsnr_s = ops.logsnr_schedule(B4, x.device, u=u, shift=1.0 / N)
    v_t = teacher.forward_hip(z_t, logsnr, y, cond_w)
    z_s, x_pred_t, _ = ops.ddim_step_vec(v_t, z_t, logsnr, logsnr_s)
    was, target.training = target.training, False
    v_tgt = target.forward_hip(z_s, logsnr_s, y, cond_w)
    target.training = was
    x_t, eps_t = ops.consistency_target(v_tgt, z_s, x_pred_t, z_t, logsnr, logsnr_s, i_times)
    ctx = {}
    v = student.forward_hip(z_t, logsnr, y, cond_w, ctx=ctx)
    if huber:
        loss_b, _, dv = ops.x_loss_huber(v, z_t, x_t, logsnr, C_HUBER, grad_scale=gs)
    else:
        loss_b, _, _, dv = ops.v_loss(v, z_t, x_t, eps_t, logsnr, grad_scale=gs, loss_type=0)
    student.backward_hip(ctx, dv)
    torch.cuda.synchronize()
    return loss_b.clone(), student.flat_grads.clone()


@pytest.mark.parametrize("loss", ["l2", "huber"])
@pytest.mark.parametrize("target", ["other", "self"])
def test_mode_is_the_composition_of_public_ops(batch, target, loss):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    x, y, eps, cond_w = batch
    teacher, student = _net(1).eval(), _net(2)
    tgt = _net(3).eval() if target == "other" else None
    diff = GaussianDiffusion(mean_type="v", num_steps=2, teacher_net=teacher, teacher_mode="consistency", target_net=tgt, consistency_grid=8,
                             consistency_loss=loss, consistency_huber_c=C_HUBER)
    i_times = torch.tensor([5, 0, 7, 2]).cuda()
    gs = 1.0 / B4
    frozen = [(n, n.flat_grads.clone()) for n in (teacher, tgt) if n is not None]
    want_loss, want_grads = _composed(diff, student, teacher, student if tgt is None else tgt, batch, i_times, gs, loss == "huber")
    student.flat_grads.zero_()
    out = diff.train_forward_backward(net=partial(student, guide=y), x=x, grad_scale=gs, eps=eps, i_times=i_times, cond_w=cond_w)
    torch.cuda.synchronize()
    assert torch.equal(out["loss"], want_loss) and torch.equal(student.flat_grads, want_grads)
    assert bool(torch.isfinite(want_loss).all()) and float(want_loss.min()) > 0.0 and float(want_grads.abs().max()) > 0.0
    assert all(torch.equal(n.flat_grads, g) for n, g in frozen)                        # teacher and target gradients stay untouched
    assert student.training and (tgt is None or not tgt.training)
    # the no-grad pass and the autograd bridge serve the mode too: the same loss
    kw = dict(net=partial(student, guide=y), x=x, eps=eps, i_times=i_times, cond_w=cond_w)
    with torch.no_grad():
        assert torch.equal(diff.training_losses(**kw)["loss"], want_loss)
    student.zero_grad_arena()
    l2 = diff.training_losses(**kw)["loss"]
    assert torch.equal(l2.detach(), want_loss)
    (gs * l2.sum()).backward()
    torch.cuda.synchronize()
    assert float((student.flat_grads - want_grads).abs().max()) <= 1e-5 * float(want_grads.abs().max())


@pytest.mark.parametrize("loss", ["l2", "huber"])
def test_boundary_rows_of_a_copy_of_the_teacher_cost_nothing(batch, loss):
    """Student = teacher weights and every i == 0: x* is the teacher's own prediction at (z_t, t), which the student repeats bit for bit."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    x, y, eps, cond_w = batch
    teacher, student = _net(1).eval(), _net(1)
    diff = GaussianDiffusion(mean_type="v", num_steps=8, teacher_net=teacher, teacher_mode="consistency", consistency_loss=loss)
    run = lambda i: diff.train_forward_backward(net=partial(student, guide=y), x=x, grad_scale=1.0 / B4, eps=eps, i_times=torch.tensor(i).cuda(),
                                                cond_w=cond_w)
    out = run([1, 2, 3, 4])                 # away from the boundary the arena holds a gradient, which the boundary pass has to overwrite
    torch.cuda.synchronize()
    assert float(out["loss"].min()) > 0.0 and int(torch.count_nonzero(student.flat_grads)) > 10000
    out = run([0, 0, 0, 0])
    torch.cuda.synchronize()
    assert float(out["loss"].abs().max()) == 0.0 and int(torch.count_nonzero(student.flat_grads)) == 0


def test_target_forward_leaves_the_dropout_counter_alone(batch):
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    x, y, eps, cond_w = batch
    teacher, student = _net(1, dropout=0.1).eval(), _net(2, dropout=0.1)
    assert student.training
    c0 = student._drop_counter
    student.forward_hip(x, torch.zeros(B4, device="cuda"), y, cond_w, ctx={})
    per_forward = student._drop_counter - c0
    assert per_forward > 0
    diff = GaussianDiffusion(mean_type="v", num_steps=8, teacher_net=teacher, teacher_mode="consistency")
    c1 = student._drop_counter
    out = diff.train_forward_backward(net=partial(student, guide=y), x=x, grad_scale=1.0 / B4, eps=eps, i_times=torch.tensor([1, 0, 7, 3]).cuda(),
                                      cond_w=cond_w)
    assert student._drop_counter - c1 == per_forward and student.training and bool(torch.isfinite(out["loss"]).all())


def test_draws_come_in_step2s_order(batch):
    """eps, then the integer time, then cond_w, from the same stream: a consistency step leaves the stream where a step2 step leaves it, and
    its drawn times lie on the training grid."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    x, y, _, _ = batch
    teacher, student = _net(1).eval(), _net(2)
    counters = {}
    for mode, grid in (("step2", 0), ("consistency", 0), ("consistency", 64)):
        diff = GaussianDiffusion(mean_type="v", num_steps=8, teacher_net=teacher, teacher_mode=mode, consistency_grid=grid, seed=4)
        out = diff.train_forward_backward(net=partial(student, guide=y), x=x, grad_scale=1.0 / B4)
        counters[(mode, grid)] = diff.rng.counter
        assert bool(torch.isfinite(out["loss"]).all())
    assert len(set(counters.values())) == 1 and counters[("step2", 0)] == B4 * S * S // 4 + 2


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
def _init(B=B4, C=1, seed=21):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((B, C, S, S), generator=g).cuda(), torch.tensor([3, -1, 0, 9, 5, 1, 2, 7][:B]).cuda()


def test_one_step_is_ddim_at_one_step():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net = _net(1).eval()
    init, y = _init()
    a = GaussianDiffusion(mean_type="v", num_steps=1, sampler="consistency").sample(net=partial(net, guide=y), init_x=init)
    b = GaussianDiffusion(mean_type="v", num_steps=1, sampler="ddim").sample(net=partial(net, guide=y), init_x=init)
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and a[0].shape == (1, B4, 1, S, S)


@pytest.mark.parametrize("guided", [False, True], ids=["unguided", "guided"])
def test_three_steps_follow_the_restatement(guided):
    """Step by step on the recorded trajectory: z_k = alpha_s x_hat_k + sigma_s eps_k within the z_next bound of ONE step (each step is checked
    on its own x_hat, so nothing compounds), eps_k the Philox normals at the counter block the loop reserved for evaluation k; the last z is x_hat."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, sampler_plan
    net = _net(1).eval()
    init, y = _init()
    d = GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency", seed=11)
    kw = dict(cond_w=0.5, net_cond_w=torch.tensor([0.5, 1.0, 2.0, 3.5]).cuda()) if guided else {}
    zs, xs, es = d.sample(net=partial(net, guide=y), init_x=init, **kw)
    per = B4 * S * S // 4
    assert d.rng.counter == 3 * per and zs.shape == (3, B4, 1, S, S)
    for k, step in enumerate(sampler_plan(3, "consistency")):
        eps = ops.rng_normal(tuple(init.shape), d.rng.seed, k * per, "cuda")
        want = R.consistency_step(f64(xs[k]), f64(eps), step.ls, step.is_last)
        bound = 8 * U * (np.abs(f64(xs[k])) + np.abs(f64(eps)))
        assert (np.abs(f64(zs[k]) - want) <= bound).all(), k
        assert float(xs[k].abs().max()) <= 1.0 and bool(torch.isfinite(es[k]).all())
    assert torch.equal(zs[2], xs[2]) and not torch.equal(zs[1], xs[1])
    # the same seed draws the same chain; record=False returns its last z
    d2 = GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency", seed=11)
    assert torch.equal(d2.sample(net=partial(net, guide=y), init_x=init, record=False, **kw)[0][-1], zs[-1])
    # start= (edit) runs the tail of the same plan
    d3 = GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency", seed=11)
    tail = d3.sample(net=partial(net, guide=y), init_x=init, start=2, **kw)[0]
    assert tail.shape[0] == 2 and d3.rng.counter == 2 * per and float(tail[-1].abs().max()) <= 1.0


def test_graph_path_and_chunks_give_the_whole_batchs_bits():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net = _net(1).eval()
    init, y = _init()
    run = lambda d, i=init, yy=y: d.sample(net=partial(net, guide=yy), init_x=i, record=False)[0][-1]
    graphed, plain = (GaussianDiffusion(mean_type="v", num_steps=16, sampler="consistency", seed=5) for _ in range(2))
    plain.GRAPH_MAX_PIXELS = 0
    assert graphed._graph_path(net, B4, S, S) and not plain._graph_path(net, B4, S, S)
    a, b = run(graphed), run(plain)
    assert torch.equal(a, b) and len(graphed._graphs) == 1 and not plain._graphs and bool(torch.isfinite(a).all())
    # two half-batches on two streams, each at its own Philox counter offset, against one batch on one stream
    init8, y8 = _init(B=8)
    two, one = (GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency", seed=5) for _ in range(2))
    two.STREAM_MIN_PIXELS, one.SAMPLER_STREAMS = 0, 1
    seen = []
    chunk = two._sample_chunk
    two._sample_chunk = lambda *args, **kwargs: seen.append(args[9]) or chunk(*args, **kwargs)
    a, b = run(two, init8, y8), run(one, init8, y8)
    assert seen == [0, 4 * S * S // 4] and torch.equal(a, b)


def test_refused_combinations_raise():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net = _net(1).eval()
    init, y = _init()
    d = GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency")
    with pytest.raises(ValueError, match="consistency.*inpainting"):
        d.inpaint(net=partial(net, guide=y), x0=init, mask=torch.ones((1, 1, S, S), device="cuda"), init_x=init)
    with pytest.raises(ValueError, match="consistency.*inpainting"):
        d.edit(net=partial(net, guide=y), x=init.clamp(-1, 1), start=2, mask=torch.ones((1, 1, S, S), device="cuda"))
    with pytest.raises(ValueError, match="consistency.*restoration"):
        d.restore(net=partial(net, guide=y), obs=torch.zeros((B4, 1, S // 2, S // 2), device="cuda"), factor=2, init_x=init)
    with pytest.raises(ValueError, match="consistency.*dyn_threshold"):
        GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency", dyn_threshold=0.995).sample(net=partial(net, guide=y), init_x=init)
    out = d.edit(net=partial(net, guide=y), x=init.clamp(-1, 1), start=2)[0][-1]          # editing without a mask is the sampler from part-way
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0


# ---- the model and the command line ----------------------------------------------------------------------------------------------------------
def _flags(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=4, seed=3, hidden_size=32, in_channels=1)
    G.update(flags)
    return Model, G


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """A w-conditioned net saved as model.pt (every SimpleUnet carries cond_w_embed)."""
    path = tmp_path_factory.mktemp("consistency") / "model.pt"
    Model, G = _flags()
    torch.manual_seed(0)
    m = Model(G)
    assert any(k.startswith("net.cond_w_embed") for k in m.state_dict())
    torch.save(m.state_dict(), path)
    return path


def test_model_trains_and_samples(checkpoint):
    Model, G = _flags(teacher_path=checkpoint, teacher_mode="consistency", ema_decay=0.95, consistency_grid=8, timesteps=2, sampler="consistency",
                      image_size=S)
    m = Model(G).to("cuda")
    assert m.diffusion.target_net is m.ema_net and m.diffusion.train_grid == 8 and not m.optimizer.ema_seeded
    seen = []
    forward = m.ema_net.forward_hip
    m.ema_net.forward_hip = lambda *a, **k: seen.append(m.arena_digests()) or forward(*a, **k)
    start = m.net.flat_params.clone()
    g = torch.Generator().manual_seed(5)
    losses = []
    for _ in range(3):
        x, y = (torch.rand((4, 1, S, S), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (4,), generator=g).cuda()
        losses.append(float(m.train_step(x, y)["loss"]))
    assert len(seen) == 3 and seen[0]["ema"] == seen[0]["params"] is not None          # seeded ahead of the first target forward
    assert seen[1]["ema"] != seen[1]["params"]                                         # and an average from then on
    assert all(np.isfinite(losses)) and not torch.equal(m.net.flat_params, start)
    assert not m.ema_net.training and m.net.training
    m.ema_net.forward_hip = forward
    m.eval()
    out = m.sample(4, torch.tensor([1, 2, 3, 4]).cuda())
    assert out.shape == (4, 1, S, S) and bool(torch.isfinite(out).all()) and float(out.abs().max()) <= 1.0
    with torch.no_grad():
        test_loss = m.loss(torch.zeros((4, 1, S, S), device="cuda"), torch.tensor([1, 2, 3, 4]).cuda())[0]
    assert bool(torch.isfinite(test_loss))


def test_cli_epoch(checkpoint, tmp_path):
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main", "--model=diffusion", "--epochs=1", "--hidden_size", "32", "--bs", "4",
                        "--train_batches", "2", "--test_batches", "1", "--teacher_path", str(checkpoint), "--teacher_mode", "consistency",
                        "--ema_decay", "0.95", "--consistency_grid", "8", "--timesteps", "2", "--sampler", "consistency", "--logdir",
                        str(tmp_path / "run")], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "Loading teacher model" in r.stdout and "diffusion/train/loss" in r.stdout and "SAVED MODEL" in r.stdout
