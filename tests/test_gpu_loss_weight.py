"""GPU tests of the loss weightings and the stratified times (extensions): gmk_x_loss_w against the float64 restatement
(tests/loss_weight_ref.py) and bit for bit against gmk_v_loss's x_mse, gmk_u_stratified bit for bit against the numpy rule, the default flags
against no flags, the whole gradient under min_snr against autograd through the CPU oracle, the stratified draw inside the step (kernel by
kernel and as a captured graph) and the command line."""
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_weight_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
LAM32 = np.array(R.LAMBDAS, dtype=np.float32)          # the six log-SNRs as the kernel sees them
GAMMA, GRAD_SCALE = 5.0, 0.37
CAP = 12288                                            # ops.X_LOSS_KEEP (asserted below): the LDS-resident limit
# tests/test_gpu_unet.py's bars, restated: the fp32 mode's 1e-3 and the 16-bit mode's whole-gradient statement (its GRAD16 constants)
TOL32 = 1e-3
GRAD16 = {"cosine": 0.9999, "rel_l2": 1.5e-2}


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def dev(a):
    from generative_models_amd import ops
    return ops.aligned(T(np.ascontiguousarray(a)).cuda())


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------------------
def _check_against_reference(got, ref, where, seen=None):
    """loss_b to 1e-5 relative, dv to 1e-5 of the image's largest entry and exactly 0 where the restatement clips.  seen: a two-element list
    that keeps the largest of the two figures."""
    loss_b, x_mse, dv = (t.cpu().numpy().astype(np.float64) for t in got)
    B = loss_b.shape[0]
    rel = np.abs(loss_b - ref["loss_b"]) / ref["loss_b"]
    dv, rdv = dv.reshape(B, -1), ref["dv"].reshape(B, -1)
    worst = np.abs(dv - rdv).max(1) / np.maximum(np.abs(rdv).max(1), 1e-300)
    if seen is not None:
        seen[0], seen[1] = max(seen[0], rel.max()), max(seen[1], np.where(np.abs(rdv).max(1) > 0, worst, 0).max())
    assert (rel <= 1e-5).all(), (where, rel)
    assert (np.abs(x_mse - ref["x_mse"]) <= 1e-5 * ref["x_mse"]).all(), where
    assert (np.abs(dv - rdv).max(1) <= 1e-5 * np.abs(rdv).max(1)).all(), (where, worst)
    assert (dv[ref["clipped"].reshape(B, -1)] == 0.0).all(), where


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 255, 256, 257, 1027, 3072, CAP, CAP + 3, CAP + 4])
def test_x_loss_w_against_the_reference_and_v_loss(n, B):
    """Both weightings, the three mean types, one image at each of the six log-SNRs (in launches of B images), gamma = 5, some elements
    clipped (tests/loss_weight_ref.loss_inputs).  n: one element, fewer than a wave, around one pass of the workgroup (255 / 256 / 257), odd
    (1027: the scalar path), 3 x 32 x 32, and the LDS capacity with the first sizes past it on the scalar (+ 3) and the 16-byte (+ 4) path."""
    from generative_models_amd import ops
    assert ops.X_LOSS_KEEP == CAP
    clipped = total = 0
    seen = [0.0, 0.0]
    for mt in R.MEAN_TYPES:
        out, z, x, eps = R.loss_inputs(6, n, LAM32.astype(np.float64), mt, seed=n)
        for a in range(0, 6, B):
            rows = slice(a, a + B)
            lam = LAM32[rows]
            v_d, z_d, x_d, e_d, l_d = dev(out[rows]), dev(z[rows]), dev(x[rows]), dev(eps[rows]), dev(lam)
            x_mse_v = ops.v_loss(v_d, z_d, x_d, e_d, l_d, grad_scale=1.0, mean_type=mt)[1]
            for weight in R.WEIGHTS:
                ref = R.x_loss_w(out[rows], z[rows], x[rows], lam, weight, GAMMA, grad_scale=GRAD_SCALE, mean_type=mt)
                got = ops.x_loss_w(v_d, z_d, x_d, l_d, weight, GAMMA, grad_scale=GRAD_SCALE, mean_type=mt)
                assert np.array_equal(bits(got[1]), bits(x_mse_v)), (mt, weight, a)          # v_loss's x_mse, bit for bit
                _check_against_reference(got, ref, f"n = {n}, B = {B}, {mt}, {weight}, images {a}..{a + B - 1}", seen)
                plain = ops.x_loss_w(v_d, z_d, x_d, l_d, weight, GAMMA, mean_type=mt)          # without dv: the same bits
                assert plain[2] is None
                assert np.array_equal(bits(plain[0]), bits(got[0])) and np.array_equal(bits(plain[1]), bits(got[1]))
                clipped += int(ref["clipped"].sum()); total += ref["clipped"].size
    print(f"n = {n}, B = {B}: largest loss_b relative error {seen[0]:.2e}, largest dv error over the image's largest entry {seen[1]:.2e}")
    assert 0 < clipped < total


@pytest.mark.parametrize("weight", R.WEIGHTS)
def test_x_loss_w_unaligned_views(weight):
    """Tensors that start one float past a 16-byte boundary (n = 1027): the scalar path, the same statements."""
    from generative_models_amd import ops
    n, B, mt = 1027, 3, "v"
    lam = LAM32[[1, 3, 5]]
    out, z, x, eps = R.loss_inputs(B, n, lam.astype(np.float64), mt, seed=7)

    def off1(a):
        buf = torch.empty(B * n + 5, device="cuda")
        assert buf.data_ptr() % 16 == 0
        view = buf[1:1 + B * n].view(B, n)
        view.copy_(T(a))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    l_d = dev(lam)
    got = ops.x_loss_w(off1(out), off1(z), off1(x), l_d, weight, GAMMA, grad_scale=GRAD_SCALE, mean_type=mt)
    ref = R.x_loss_w(out, z, x, lam, weight, GAMMA, grad_scale=GRAD_SCALE, mean_type=mt)
    _check_against_reference(got, ref, f"unaligned, {weight}")
    x_mse_v = ops.v_loss(dev(out), dev(z), dev(x), dev(eps), l_d, mean_type=mt)[1]
    assert np.array_equal(bits(got[1]), bits(x_mse_v))
    # mixed: only dv's alignment differs from the 16-byte case - n % 4 != 0 keeps it scalar anyway; aligned inputs with n = 1028 take 16 bytes
    n4 = 1028
    out, z, x, eps = R.loss_inputs(B, n4, lam.astype(np.float64), mt, seed=8)
    a = ops.x_loss_w(dev(out), dev(z), dev(x), l_d, weight, GAMMA, grad_scale=GRAD_SCALE, mean_type=mt)
    buf = torch.empty(B * n4 + 5, device="cuda")
    v1 = buf[1:1 + B * n4].view(B, n4)
    v1.copy_(T(out))
    b = ops.x_loss_w(v1, dev(z), dev(x), l_d, weight, GAMMA, grad_scale=GRAD_SCALE, mean_type=mt)      # one unaligned operand: scalar path
    for s, t in zip(a, b):
        assert np.array_equal(bits(s), bits(t))                   # the two paths agree bit for bit, dv included


@pytest.mark.parametrize("B", [1, 6, 8, 100, 256])
def test_u_stratified_is_the_numpy_rule(B):
    from generative_models_amd import ops
    offsets = [0.0, 1.0 - 2.0 ** -24, 0.5, 2.0 ** -24] + ops.rng_uniform((12,), 17, B, "cuda").cpu().tolist()
    for u0 in offsets:
        got = ops.u_stratified(torch.tensor([u0], device="cuda", dtype=torch.float32), B)
        want = R.u_stratified(np.float32(u0), B)
        assert np.array_equal(bits(got), want.view(np.uint32)), (u0, B)
        assert float(got.min()) >= 0.0 and float(got.max()) < 1.0


# ---- through the model -------------------------------------------------------------------------------------------------------------------------
def _model(graphed=True, **flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=4, seed=3, timesteps=8, hidden_size=32, in_channels=1, image_size=8)
    G.update(flags)
    torch.manual_seed(0)
    m = Model(G).to("cuda")
    if not graphed:
        m.TRAIN_GRAPH_MAX_PIXELS = 0
    return m


def _batches(steps, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((B, 1, 8, 8), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()) for _ in range(steps)]


def _train(m, batches):
    for x, y in batches:
        m.train_step(x, y.clone())
    torch.cuda.synchronize()
    return m.net.flat_params.clone()


@pytest.mark.parametrize("graphed", [True, False])
def test_default_flags_change_nothing(graphed):
    """Three steps with the three flags spelled out at their defaults against three steps without them: the same parameters, bit for bit."""
    batches = _batches(3, 4)
    runs = []
    for flags in ({}, dict(loss_weight="snr_trunc", loss_gamma=5.0, time_sampler="uniform")):
        m = _model(graphed, **flags)
        runs.append((_train(m, batches), m.diffusion.rng.counter))
        assert len(m.__dict__.get("_train_graphs", {})) == (1 if graphed else 0)
    assert torch.equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] == 3 * (4 * 64 // 4 + 1)


def _golden_setup(golden, dtype):
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import diffusion_ref as D
    from oracle import unet_ref as U
    g = golden("train_c32_s8.npz")
    net = SimpleUnet(32, 0.0, in_channels=1, compute_dtype=dtype)
    params = U.closed_form_params(32, 1)
    net.load_state_dict(params, strict=True)
    x0, y, u, eps = (T(g[k]) for k in ("x0", "y", "u", "eps"))
    logsnr = D.logsnr_schedule_cosine(u)
    ls = torch.sort(logsnr).values
    k = len(ls) // 2
    gamma = float(torch.exp(0.5 * (ls[k - 1] + ls[k])))            # ln gamma between the two middle log-SNRs of the batch
    lg = float(np.log(gamma))
    assert bool((logsnr < lg).any()) and bool((logsnr > lg).any()), (logsnr, lg)
    return net.cuda(), params, (x0, y, u, eps), logsnr, gamma


def _oracle_grads(params, inputs, logsnr, gamma):
    """Autograd through the CPU oracle: model_x of run_model -> w x_mse -> mean over the batch."""
    from oracle import diffusion_ref as D
    x0, y, u, eps = inputs
    pr = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    z_t = D.q_sample(x0, logsnr, eps)
    model_x = D.run_model(pr, z_t, logsnr, guide=y)["model_x"]
    loss_b = torch.clamp(torch.exp(logsnr), max=gamma) * torch.square(model_x - x0).flatten(1).mean(1)
    loss_b.mean().backward()
    return pr, loss_b.detach()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_min_snr_gradient_against_the_oracle(golden, dtype):
    """The inputs of tests/golden/train_c32_s8.npz under min_snr, gamma between the batch's log-SNRs: train_forward_backward's gradient against
    autograd through the oracle.  fp32 mode: test_training_step_vs_golden's bar on the same vectors (every tensor's gradient norm to
    1e-3 of itself plus 1e-6 of the largest norm, loss to 1e-3), and training_losses under autograd leaves the fused pass's gradient to 1e-6
    of its norm.  16-bit mode: that test's whole-gradient statement, cosine >= 0.9999 and relative L2 <= 1.5e-2 (its GRAD16 constants)."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, params, inputs, logsnr, gamma = _golden_setup(golden, dtype)
    x0, y, u, eps = (t.cuda() for t in inputs)
    B = x0.shape[0]
    pr, loss_ref = _oracle_grads(params, inputs, logsnr, gamma)
    diff = GaussianDiffusion(mean_type="v", num_steps=250, loss_weight="min_snr", loss_gamma=gamma)
    out = diff.train_forward_backward(net=partial(net, guide=y), x=x0, grad_scale=1.0 / B, u=u, eps=eps)
    assert set(out) == {"loss", "x_mse", "logsnr"}
    names = [n for n in pr if pr[n].grad is not None]
    gh = torch.cat([net.grad(n).float().cpu().reshape(-1) for n in names])
    gr = torch.cat([pr[n].grad.reshape(-1) for n in names])
    cos, rl2 = float(F.cosine_similarity(gh, gr, dim=0)), float((gh - gr).norm() / gr.norm())
    loss_err = float((out["loss"].cpu() - loss_ref).abs().max() / loss_ref.abs().max())
    print(f"min_snr gradient vs oracle [{dtype}]: gamma {gamma:.4f}, loss error {loss_err:.3e}, cosine {cos:.6f}, relative L2 {rl2:.3e}")
    if dtype == torch.float32:
        assert loss_err < TOL32
        norms = torch.stack([net.grad(n).norm().cpu() for n in names])
        ref = torch.stack([pr[n].grad.norm() for n in names])
        ok = (norms - ref).abs() <= TOL32 * ref.abs() + 1e-3 * TOL32 * ref.abs().max()
        assert bool(ok.all()), [(names[i], float(norms[i]), float(ref[i])) for i in (~ok).nonzero().flatten()[:8]]
        fused = net.flat_grads.clone()
        net.zero_grad_arena()
        with torch.enable_grad():
            res = diff.training_losses(net=partial(net, guide=y), x=x0, u=u, eps=eps)
            res["loss"].mean().backward()
        assert set(res) == {"loss", "x_mse"} and not res["x_mse"].requires_grad
        assert torch.allclose(res["loss"].detach(), out["loss"], rtol=1e-6, atol=0) and torch.allclose(res["x_mse"], out["x_mse"], rtol=1e-6, atol=0)
        gap = float((net.flat_grads - fused).norm() / fused.norm())
        print(f"autograd bridge against the fused pass: {gap:.3e} of the norm")
        assert gap <= 1e-6
    else:
        assert cos >= GRAD16["cosine"] and rl2 <= GRAD16["rel_l2"], (cos, rl2)


def test_stratified_times_in_the_step():
    """time_sampler = 'stratified', B = 8: the step's log-SNRs are the schedule of u_stratified(u0) for the u0 the stream holds at the counter
    after the eps draw, and the stream advances by the eps draw plus one."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    B, n = 8, 64
    net = SimpleUnet(32, 0.0, in_channels=1, compute_dtype=torch.float32).cuda()
    diff = GaussianDiffusion(mean_type="v", num_steps=8, loss_weight="min_snr", time_sampler="stratified", seed=11)
    (x, y), = _batches(1, B)
    diff.rng.normal((3,), "cuda")                               # not at counter 0
    c0 = diff.rng.counter
    out = diff.train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B)
    eps_counters = B * n // 4
    assert diff.rng.counter == c0 + eps_counters + 1
    u0 = ops.rng_uniform((1,), diff.rng.seed, c0 + eps_counters, "cuda")
    u = T(R.u_stratified(np.float32(u0.item()), B)).cuda()
    assert torch.equal(ops.u_stratified(u0, B), u)
    cells = torch.floor(u.double() * B).long().sort().values
    assert cells.tolist() == list(range(B))
    eps = ops.rng_normal((B, 1, 8, 8), diff.rng.seed, c0, "cuda")
    want = ops.q_sample(x, eps, u)[0]
    assert torch.equal(out["logsnr"], want)


def test_stratified_min_snr_graphed_equals_ungraphed():
    """Three steps under min_snr with stratified times: the captured step (the new loss kernel inside the graph, the u0 draw and
    gmk_u_stratified outside) leaves the parameters of the kernel-by-kernel step, bit for bit - and not those of the default objective."""
    batches = _batches(3, 8)
    flags = dict(loss_weight="min_snr", loss_gamma=5.0, time_sampler="stratified")
    a, b = _model(True, **flags), _model(False, **flags)
    pa, pb = _train(a, batches), _train(b, batches)
    assert len(a.__dict__.get("_train_graphs", {})) == 1 and not b.__dict__.get("_train_graphs")
    assert torch.equal(pa, pb)
    assert a.diffusion.rng.counter == b.diffusion.rng.counter == 3 * (8 * 64 // 4 + 1)
    assert not torch.equal(pa, _train(_model(True), batches))
    with torch.no_grad():
        loss, metrics = a.eval().loss(*batches[0])
    assert set(metrics) == {"loss", "x_mse"} and metrics["x_mse"].dim() == 0 and torch.equal(loss, metrics["loss"])
    with torch.no_grad():
        assert set(_model(True).eval().loss(*batches[0])[1]) == {"loss"}
        assert set(_model(True, loss_weight="snr").eval().loss(*batches[0])[1]) == {"loss", "x_mse"}


def test_snr_weighting_is_v_loss_type_1():
    """loss_weight = 'snr' in ordinary training: the eps-MSE through the unchanged gmk_v_loss(loss_type = 1)."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    B = 4
    net = SimpleUnet(32, 0.0, in_channels=1, compute_dtype=torch.float32).cuda()
    (x, y), = _batches(1, B)
    g = torch.Generator().manual_seed(1)
    u, eps = torch.rand((B,), generator=g).cuda(), torch.randn((B, 1, 8, 8), generator=g).cuda()
    out = GaussianDiffusion(mean_type="v", num_steps=8, loss_weight="snr").train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, u=u, eps=eps)
    assert set(out) == {"loss", "x_mse", "eps_mse", "logsnr"} and torch.equal(out["loss"], out["eps_mse"])
    grads = net.flat_grads.clone()
    logsnr, z_t = ops.q_sample(x, eps, u)
    v = net.forward_hip(z_t, logsnr, y, None)
    loss_b, _, eps_mse, _ = ops.v_loss(v, z_t, x, eps, logsnr, loss_type=1)
    assert torch.equal(loss_b, out["loss"]) and torch.equal(eps_mse, out["eps_mse"])
    ref = GaussianDiffusion(mean_type="v", num_steps=8).train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, u=u, eps=eps)
    assert torch.equal(ref["eps_mse"], out["eps_mse"]) and torch.equal(ref["loss"], torch.maximum(ref["x_mse"], ref["eps_mse"]))
    assert bool(torch.isfinite(grads).all()) and float(grads.abs().max()) > 0


def test_cli(tmp_path):
    """The three flags on the command line: one epoch runs, hps.yaml records them, the test pass logs x_mse; with a teacher they are refused."""
    import yaml
    run = tmp_path / "run"
    cmd = [sys.executable, "-m", "generative_models_amd.main", "--model=diffusion", "--loss_weight", "min_snr", "--loss_gamma", "5",
           "--time_sampler", "stratified", "--epochs", "1", "--bs", "8", "--timesteps", "4", "--train_batches", "3", "--test_batches", "1",
           "--eval_heavy", "0"]
    r = subprocess.run(cmd + ["--logdir", str(run)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    hps = yaml.load((run / "hps.yaml").read_text(), Loader=yaml.Loader)
    assert (hps["loss_weight"], hps["loss_gamma"], hps["time_sampler"]) == ("min_snr", 5.0, "stratified")
    assert "diffusion/test/x_mse" in r.stdout and "diffusion/test/loss" in r.stdout and "diffusion/train/loss" in r.stdout
    assert (run / "model.pt").exists()
    r = subprocess.run(cmd + ["--logdir", str(tmp_path / "student"), "--teacher_path", str(run / "model.pt")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode != 0 and "loss_weight" in r.stderr and "teacher" in r.stderr, r.stdout[-1000:] + r.stderr[-2000:]
    assert not (tmp_path / "student" / "model.pt").exists()
