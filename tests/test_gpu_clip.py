"""GPU tests of the steered optimiser step (DG.grad_clip, DG.skip_nonfinite, the learning-rate schedule): the gradient-norm kernel against a
float64 norm within the a-priori bound of its summation tree, its determinism, the steered Adam kernel against the plain Adam kernels bit for
bit, the non-finite guard, and all of it through the train step (graphed and kernel by kernel, 16-bit and fp32 modes) and the CLI."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clip_ref  # noqa: E402

ADAM = (3e-4, 0.9, 0.999, 1e-8)      # lr, beta1, beta2, eps


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=8, seed=3, timesteps=8)
    G.update(flags)
    torch.manual_seed(0)
    return Model(G).to("cuda")


def _batches(n, B=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((B, 1, 28, 28), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()) for _ in range(n)]


def _state():
    return torch.zeros(4, device="cuda")


def _check_norm(got, g, n, grad_scale=1.0):
    """|got - float64 norm| <= bound(n) * norm: clip_ref.norm_rel_bound, from the kernel's summation tree (d additions + the square)."""
    want = clip_ref.norm64(g, grad_scale)
    rel = abs(float(got) - want) / want
    print(f"n = {n}: norm {float(got)!r} against {want!r}, relative error {rel:.3e}, bound {clip_ref.norm_rel_bound(n):.3e} "
          f"(d = {clip_ref.norm_chain(n)})")
    assert rel <= clip_ref.norm_rel_bound(n)


# ---- the norm kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1003, 6033665])
def test_norm_against_float64_within_the_summation_bound(n):
    """n = 1003: the n & 3 tail; n = 6,033,665: the configs[2] arena.  The tolerance is clip_ref.norm_rel_bound(n) = (d + 1) 2^-25 with d the
    longest chain of fp32 additions behind the sum (d = 28 and 30 here), not a fitted number."""
    from generative_models_amd import ops
    gen = torch.Generator(device="cuda").manual_seed(n)
    for scale, grad_scale in ((1.0, 1.0), (8.0, 0.125), (1e-3, 1.0 / 3)):
        g = torch.randn(n, device="cuda", generator=gen) * scale
        st = ops.grad_norm(g, _state(), grad_scale=grad_scale, max_norm=1.0)
        _check_norm(st[ops.GRAD_NORM], g, n, grad_scale)
        assert float(st[ops.APPLY]) == 1.0 and float(st[ops.SKIPPED]) == 0.0
    # the tail elements count: a large value in the very last slot shows in the norm
    g = torch.zeros(n, device="cuda")
    g[-1] = 3.0
    g[0] = 4.0
    assert float(ops.grad_norm(g, _state())[ops.GRAD_NORM]) == 5.0


@pytest.mark.parametrize("n", [1003, 6033665])
def test_norm_bits_repeat_and_do_not_follow_the_cu_limit(n):
    from generative_models_amd import ops
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(7)) * 3
    ws = ops.grad_norm_workspace(n, g.device)
    assert ws.numel() == clip_ref.norm_parts(n)
    a = ops.grad_norm(g, _state(), 0.5, 1.0, ws).clone()
    b = ops.grad_norm(g, _state(), 0.5, 1.0).clone()          # a workspace of its own
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    limit = ops.get_cu_limit()
    ops.set_cu_limit(64 if limit > 64 else 8)
    try:
        c = ops.grad_norm(g, _state(), 0.5, 1.0, ws).clone()
    finally:
        ops.set_cu_limit(limit)
    assert torch.equal(a.view(torch.int32), c.view(torch.int32))


def test_coefficient_on_both_sides_of_max_norm():
    from generative_models_amd import ops
    n = 1003
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    norm = float(ops.grad_norm(g, _state())[ops.GRAD_NORM])
    for max_norm in (0.25 * norm, 0.999 * norm, norm, 1.001 * norm, 4 * norm, 1e-30, 1e30):
        st = ops.grad_norm(g, _state(), 1.0, max_norm).cpu().numpy()
        want = clip_ref.clip_coef(st[ops.GRAD_NORM], np.float32(max_norm))
        assert st[ops.CLIP_COEF] == want, (max_norm, st, want)
    assert float(ops.grad_norm(g, _state(), 1.0, 0.25 * norm)[ops.CLIP_COEF]) < 0.2500001
    assert float(ops.grad_norm(g, _state(), 1.0, 4 * norm)[ops.CLIP_COEF]) == 1.0
    for off in (0.0, -1.0):
        assert float(ops.grad_norm(g, _state(), 1.0, off)[ops.CLIP_COEF]) == 1.0


def test_nonfinite_values_and_overflow_clear_apply():
    from generative_models_amd import ops
    n = 6033665
    g = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    st = _state()
    for i, bad in enumerate((float("nan"), float("inf"), -float("inf"))):
        h = g.clone()
        h[n // 3 + i] = bad
        ops.grad_norm(h, st, 1.0, 1.0)
        assert float(st[ops.APPLY]) == 0.0 and float(st[ops.SKIPPED]) == i + 1 and not np.isfinite(float(st[ops.GRAD_NORM]))
    h = g.clone()
    h[5] = 3e19                                  # finite, its square is not: counts as non-finite
    ops.grad_norm(h, st, 1.0, 0.0)
    assert float(st[ops.APPLY]) == 0.0 and float(st[ops.SKIPPED]) == 4.0
    ops.grad_norm(g, st, 1.0, 1.0)               # a finite gradient: apply again, the count stays
    assert float(st[ops.APPLY]) == 1.0 and float(st[ops.SKIPPED]) == 4.0


# ---- the steered Adam kernel --------------------------------------------------------------------------------------------------------
def _arenas(n, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda: torch.randn(n, device="cuda", generator=gen)
    return r, (r(), r() * 0.01, r().abs() * 1e-4, r())


@pytest.mark.parametrize("n", [1003, 6033665])
def test_steered_adam_with_coefficient_one_is_todays_kernels(n):
    from generative_models_amd import ops
    r, (p, m, v, ema) = _arenas(n, n)
    st = _state()
    for step, decay in ((1, 0.1), (2, 0.75), (3, 0.999)):
        g = r() * 8
        ops.grad_norm(g, st, 0.125, 0.0)
        assert float(st[ops.CLIP_COEF]) == 1.0
        pa, ma, va = p.clone(), m.clone(), v.clone()
        ops.adam_step(pa, g, ma, va, *ADAM, step, grad_scale=0.125)
        pe, me, ve, ee = p.clone(), m.clone(), v.clone(), ema.clone()
        ops.adam_ema_step(pe, g, me, ve, ee, *ADAM, step, decay, grad_scale=0.125)
        pc, mc, vc = p.clone(), m.clone(), v.clone()
        ops.adam_step_ctl(pc, g, mc, vc, st, *ADAM, step, grad_scale=0.125)
        assert torch.equal(pc, pa) and torch.equal(mc, ma) and torch.equal(vc, va)
        ops.adam_step_ctl(p, g, m, v, st, *ADAM, step, grad_scale=0.125, ema=ema, decay_t=decay)
        assert torch.equal(p, pe) and torch.equal(m, me) and torch.equal(v, ve) and torch.equal(ema, ee)


@pytest.mark.parametrize("n", [1003, 6033665])
def test_steered_adam_clips_like_a_prescaled_gradient(n):
    """coef < 1: the bits of ops.adam_step(grad_scale=1.0) on (g * grad_scale) * coef formed by torch in fp32."""
    from generative_models_amd import ops
    r, (p, m, v, _) = _arenas(n, n + 1)
    st = _state()
    for step, grad_scale in ((1, 0.125), (2, 1.0), (3, 1.0 / 3)):
        g = r() * 8
        ops.grad_norm(g, st, grad_scale, 0.5)
        coef = st[ops.CLIP_COEF].clone()
        assert 0.0 < float(coef) < 1.0
        pre = (g * grad_scale) * coef
        pa, ma, va = p.clone(), m.clone(), v.clone()
        ops.adam_step(pa, pre, ma, va, *ADAM, step, grad_scale=1.0)
        ops.adam_step_ctl(p, g, m, v, st, *ADAM, step, grad_scale=grad_scale)
        assert torch.equal(p, pa) and torch.equal(m, ma) and torch.equal(v, va)
        assert clip_ref.norm64(pre) <= 0.5 * (1 + 1e-5)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
@pytest.mark.parametrize("n", [1003, 6033665])
def test_one_nonfinite_value_skips_the_whole_step(n, bad):
    """A NaN (or an inf) is a value written into the gradient tensor: p, m, v and ema keep their bits, `skipped` goes up by one, and the next
    call with a finite gradient updates as usual."""
    from generative_models_amd import ops
    r, (p, m, v, ema) = _arenas(n, n + 2)
    st = _state()
    g = r()
    ops.grad_norm(g, st, 1.0, 1.0)
    ops.adam_step_ctl(p, g, m, v, st, *ADAM, 1, ema=ema, decay_t=0.5)
    keep = [t.clone() for t in (p, m, v, ema)]
    gb = r()
    gb[n - 1] = bad
    ops.grad_norm(gb, st, 1.0, 1.0)
    ops.adam_step_ctl(p, gb, m, v, st, *ADAM, 2, ema=ema, decay_t=0.5)
    ops.adam_step_ctl(p, gb, m, v, st, *ADAM, 2)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip((p, m, v, ema), keep))
    assert float(st[ops.SKIPPED]) == 1.0 and float(st[ops.APPLY]) == 0.0
    g2 = r()
    ops.grad_norm(g2, st, 1.0, 1.0)
    coef = st[ops.CLIP_COEF].clone()
    pa, ma, va, ea = [t.clone() for t in keep]
    ops.adam_ema_step(pa, (g2 * 1.0) * coef, ma, va, ea, *ADAM, 3, 0.5)
    ops.adam_step_ctl(p, g2, m, v, st, *ADAM, 3, ema=ema, decay_t=0.5)
    assert torch.equal(p, pa) and torch.equal(m, ma) and torch.equal(v, va) and torch.equal(ema, ea)
    assert float(st[ops.SKIPPED]) == 1.0 and bool(torch.isfinite(p).all())


# ---- through the train step ---------------------------------------------------------------------------------------------------------
MODES = [("bf16", True), ("bf16", False), ("fp32", True), ("fp32", False)]


def _ungraph(m, graphed):
    if not graphed:
        m.TRAIN_GRAPH_MAX_PIXELS = 0
    return m


@pytest.mark.parametrize("dtype,graphed", MODES)
def test_a_clip_that_never_clips_leaves_training_alone(dtype, graphed):
    """grad_clip = 1e30 and skip_nonfinite = 1: after 5 steps the weights equal a default model's bit for bit."""
    batches = _batches(5)
    arenas = []
    for flags in ({}, dict(grad_clip=1e30, skip_nonfinite=1)):
        m = _ungraph(_model(compute_dtype=dtype, **flags), graphed)
        outs = [m.train_step(x, y.clone()) for x, y in batches]
        assert len(m.__dict__.get("_train_graphs", {})) == (1 if graphed else 0)
        assert ("grad_norm" in outs[-1]) == bool(flags) and ("skipped_steps" in outs[-1]) == bool(flags) and "lr" not in outs[-1]
        arenas.append(m.net.flat_params.clone())
    assert torch.equal(arenas[0], arenas[1])
    assert outs[-1]["grad_norm"].is_cuda and float(outs[-1]["grad_norm"]) > 0 and float(outs[-1]["skipped_steps"]) == 0.0
    assert m.optimizer.state_dict()["skipped"] == 0


@pytest.mark.parametrize("dtype,graphed", MODES)
def test_every_clipped_step_equals_a_replay_on_the_prescaled_gradient(dtype, graphed):
    """grad_clip a quarter of the first step's norm, so every step clips: the reported norm matches the float64 norm of flat_grads within
    the kernel's bound, the coefficient is the formula on it, and the weights after each step equal ops.adam_step on (g * 1) * coef."""
    from generative_models_amd import ops
    batches = _batches(5)
    probe = _ungraph(_model(compute_dtype=dtype, grad_clip=1e30), graphed)
    clip = 0.25 * float(probe.train_step(batches[0][0], batches[0][1].clone())["grad_norm"])
    m = _ungraph(_model(compute_dtype=dtype, grad_clip=clip), graphed)
    n = m.net.flat_params.numel()
    p = m.net.flat_params.clone()
    mm, vv = torch.zeros_like(p), torch.zeros_like(p)
    for t, (x, y) in enumerate(batches):
        out = m.train_step(x, y.clone())
        g = m.net.flat_grads.clone()
        st = m.optimizer.ctl_state.clone()
        assert torch.equal(out["grad_norm"], st[ops.GRAD_NORM])
        _check_norm(out["grad_norm"], g, n)
        coef = st[ops.CLIP_COEF]
        assert float(coef) == float(clip_ref.clip_coef(st[ops.GRAD_NORM].cpu().numpy(), np.float32(clip))) and float(coef) < 1.0
        ops.adam_step(p, (g * 1.0) * coef, mm, vv, 1e-3, 0.9, 0.999, 1e-8, t + 1, grad_scale=1.0)
        assert torch.equal(p, m.net.flat_params), t
    assert float(out["skipped_steps"]) == 0.0


@pytest.mark.parametrize("C", [128, 96])
def test_norm_equals_clip_grad_norm_on_the_parameter_gradients(C):
    """torch.nn.utils.clip_grad_norm_ on CPU double copies of the per-parameter gradients, in the reference's shapes.  At the zero-padded
    width 96 the arena is wider than the parameters: the padding's gradients are zero and must not show in the norm."""
    m = _model(hidden_size=C, grad_clip=1.0)
    x, y = _batches(1)[0]
    out = m.train_step(x, y.clone())
    net = m.net
    want = clip_ref.clip_grad_norm_double([net.grad(name) for name, _ in net._inventory], 1.0)
    n = net.flat_grads.numel()
    rel = abs(float(out["grad_norm"]) - want) / want
    print(f"C = {C}: norm {float(out['grad_norm'])!r} against clip_grad_norm_ {want!r}, relative error {rel:.3e}")
    assert rel <= clip_ref.norm_rel_bound(n)
    if C == 96:
        assert sum(net.grad(name).numel() for name, _ in net._inventory) < n


@pytest.mark.parametrize("dtype,graphed", MODES)
def test_a_planted_nan_skips_the_step_and_the_average(dtype, graphed):
    """ema_decay > 0: a NaN written into flat_grads just before the optimiser runs leaves net, the Adam moments and ema_net bit-unchanged and
    counts one skipped step; the next step trains as usual.  The host counters advance all the same."""
    batches = _batches(4)
    m = _ungraph(_model(compute_dtype=dtype, ema_decay=0.999, skip_nonfinite=1), graphed)
    for x, y in batches[:2]:
        m.train_step(x, y.clone())
    opt = m.optimizer
    keep = [t.clone() for t in (m.net.flat_params, opt.m, opt.v, m.ema_net.flat_params)]
    step = opt.step

    def poisoned(grad_scale=1.0):
        m.net.flat_grads[12345] = float("nan")
        return step(grad_scale=grad_scale)

    opt.step = poisoned
    out = m.train_step(*batches[2])
    opt.step = step
    now = (m.net.flat_params, opt.m, opt.v, m.ema_net.flat_params)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(now, keep))
    assert float(out["skipped_steps"]) == 1.0 and not np.isfinite(float(out["grad_norm"])) and opt.step_count == 3
    assert opt.state_dict()["skipped"] == 1
    out = m.train_step(*batches[3])
    assert float(out["skipped_steps"]) == 1.0 and np.isfinite(float(out["grad_norm"])) and opt.step_count == 4
    assert not torch.equal(m.net.flat_params, keep[0]) and not torch.equal(m.ema_net.flat_params, keep[3])
    assert bool(torch.isfinite(m.net.flat_params).all()) and bool(torch.isfinite(m.ema_net.flat_params).all())


@pytest.mark.parametrize("dtype,graphed", MODES)
def test_cosine_schedule_with_warmup_equals_a_replay(dtype, graphed):
    """lr_scheduler = 'cosine', 2 warm-up steps, 3 decay steps, 5 train steps: the weights equal ops.adam_step called with lr_at(t); the
    schedule alone goes through today's kernels and reports `lr`."""
    from generative_models_amd import ops
    batches = _batches(5)
    m = _ungraph(_model(compute_dtype=dtype, lr_scheduler="cosine", lr_warmup=2, lr_decay_steps=3, lr_min_ratio=0.1), graphed)
    assert not m.optimizer.steered
    p = m.net.flat_params.clone()
    mm, vv = torch.zeros_like(p), torch.zeros_like(p)
    lrs = []
    for t, (x, y) in enumerate(batches):
        out = m.train_step(x, y.clone())
        lr = clip_ref.lr_at(1e-3, t, "cosine", 2, 3, 0.1)
        assert float(out["lr"]) == pytest.approx(lr, rel=1e-15) and m.optimizer.lr_at(t) == float(out["lr"]) and "grad_norm" not in out
        ops.adam_step(p, m.net.flat_grads, mm, vv, m.optimizer.lr_at(t), 0.9, 0.999, 1e-8, t + 1, grad_scale=1.0)
        assert torch.equal(p, m.net.flat_params), t
        lrs.append(lr)
    assert lrs[0] == pytest.approx(5e-4) and lrs[1] == 1e-3 and lrs[2] == 1e-3 and lrs[4] < lrs[3] < lrs[2]


# ---- the driver -----------------------------------------------------------------------------------------------------------------------
def test_cli_with_clip_guard_and_schedule(tmp_path):
    import yaml
    run = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main", "--model=diffusion", "--epochs=1", "--bs", "8", "--timesteps", "4",
                        "--grad_clip", "1.0", "--skip_nonfinite", "1", "--lr_scheduler", "cosine", "--lr_warmup", "2", "--lr_decay_steps", "3",
                        "--train_batches", "3", "--test_batches", "1", "--eval_heavy", "0", "--logdir", str(run)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(run / "hps.yaml") as f:
        hps = yaml.load(f, Loader=yaml.Loader)
    assert (hps["grad_clip"], hps["skip_nonfinite"], hps["lr_scheduler"], hps["lr_warmup"], hps["lr_decay_steps"], hps["lr_min_ratio"]) == \
        (1.0, 1, "cosine", 2, 3, 0.1)
    for key in ("diffusion/train/grad_norm", "diffusion/train/skipped_steps", "diffusion/train/lr"):
        assert key in r.stdout, r.stdout[-3000:]
