"""GPU tests of the loss profile and the loss-aware time sampler (extensions): gmk_loss_profile and gmk_u_importance bit for bit against the
numpy float32 restatement (tests/time_importance_ref.py), a run inside the sampler's warm-up against the run without the flag, the weighted
gradient against single-image passes of a model without the flag, resume, and the command line."""
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_importance_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
T = torch.from_numpy
TOL32 = 1e-3                                               # the fp32 mode's bar (tests/test_gpu_unet.py)


def bits(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().contiguous().numpy()
    return np.ascontiguousarray(t, dtype=F).view(np.uint32)


def dev(a):
    from generative_models_amd import ops
    return ops.aligned(T(np.ascontiguousarray(a, dtype=F)).cuda())


# ---- gmk_loss_profile ---------------------------------------------------------------------------------------------------------------------------
def _profile_inputs(B, seed):
    """u: every edge k / 64 that fits, 0 and 1 - 2^-24 first, the rest uniform over a part of [0, 1) that leaves bins 20 ... 39 empty; a few
    samples carry a NaN or an infinite value or u = 1 (skipped).  v0 of both signs over four decades, v1 positive."""
    rng = np.random.default_rng(seed)
    edges = np.concatenate([[0.0, 1.0 - 2.0 ** -24], np.delete(np.arange(64) / 64.0, np.arange(20, 40))])
    u = rng.random(B)
    u = np.where(u < 0.5, u * (20.0 / 64 / 0.5), 40.0 / 64 + (u - 0.5) * (24.0 / 64 / 0.5))
    m = min(B, len(edges))
    u[:m] = edges[:m]
    u = u.astype(F)
    v0 = (rng.standard_normal(B) * 10.0 ** rng.uniform(-2, 2, B)).astype(F)
    v1 = rng.uniform(0.01, 3.0, B).astype(F)
    if B >= 63:
        u[50], v0[51], v0[52], v1[53], u[54], u[55] = 1.0, np.nan, np.inf, -np.inf, np.nan, -0.5
    return u, v0, v1


@pytest.mark.parametrize("decay", [1.0, 0.9])
@pytest.mark.parametrize("with_v1", [True, False])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257, 2051])
def test_loss_profile_is_the_restatement(B, with_v1, decay):
    """Two consecutive updates from a state with odd contents, bit for bit; bins no sample reaches keep their bits (a NaN payload among them); the
    same call from the same state gives the same bits.  B: one sample, around a wavefront, more than one pass of the workgroup, and more than
    two LDS tiles with a tail that is no multiple of four."""
    from generative_models_amd import ops
    rng = np.random.default_rng(B)
    start = np.abs(rng.standard_normal((5, 64))).astype(F)
    start[:, 25] = np.array([3.0, np.nan, np.inf, -0.0, 1e-40], dtype=F)        # bin 25 stays empty: these bits must survive
    ref = start
    state = dev(start)
    for step in range(2):
        u, v0, v1 = _profile_inputs(B, 100 * B + step)
        if not with_v1:
            v1 = None
        before = state.clone()
        again = ops.loss_profile(dev(u), dev(v0), None if v1 is None else dev(v1), before.clone(), decay)
        out = ops.loss_profile(dev(u), dev(v0), None if v1 is None else dev(v1), state, decay)
        assert out is state
        ref_next = R.loss_profile(ref, u, v0, v1, decay)
        assert np.array_equal(bits(state), bits(ref_next)), (B, with_v1, decay, step, np.argwhere(bits(state) != bits(ref_next))[:8])
        assert np.array_equal(bits(again), bits(state))
        same = bits(ref_next) == bits(ref)
        assert same[:, 20:40].all() and not same[:3, 0].any()
        if v1 is None:
            assert same[3:].all()
        ref = ref_next
    assert np.array_equal(bits(state[:, 25]), bits(start[:, 25]))


# ---- gmk_u_importance ---------------------------------------------------------------------------------------------------------------------------
def _states():
    flat = R.steep_state(0.0)
    short = R.steep_state(14.0)
    short[0, 40] = F(4.5)                                   # one bin below warm = 5
    zero_s2 = R.steep_state(14.0)
    zero_s2[2] = 0
    rough = R.steep_state(-9.0)
    rough[2] *= np.random.default_rng(9).uniform(0.2, 5.0, 64).astype(F)
    return {"empty": np.zeros((5, 64), dtype=F), "short": short, "flat": flat, "steep": R.steep_state(28.0), "steep_down": R.steep_state(-14.0),
            "rough": rough, "zero_s2": zero_s2}


@pytest.mark.parametrize("B", [1, 64, 1000])
@pytest.mark.parametrize("name", list(_states()))
def test_u_importance_is_the_restatement(name, B):
    """u, w and the table (p_out, w_out) bit for bit, at floor 0.01 and 0.05; not ready / no mass: u's bits are u0's and w == 1; every draw
    carries the weight of the bin it lies in.  u0: the device RNG's values plus 0, 1 - 2^-24 and 2^-30."""
    from generative_models_amd import ops
    state = _states()[name]
    u0 = ops.rng_uniform((B,), 23, 5 * B, "cuda").cpu().numpy()
    for i, edge in enumerate((0.0, 1.0 - 2.0 ** -24, 2.0 ** -30)[:max(0, B - 1)]):
        u0[i] = edge
    for floor in (0.01, 0.05):
        u, w, p, wt = ops.u_importance(dev(state), dev(u0), 5.0, floor, want_table=True)
        ru, rw, rp, rwt = R.u_importance(state, u0, 5.0, floor)
        for got, want, what in ((u, ru, "u"), (w, rw, "w"), (p, rp, "p_out"), (wt, rwt, "w_out")):
            assert np.array_equal(bits(got), bits(want)), (name, B, floor, what)
        plain = ops.u_importance(dev(state), dev(u0), 5.0, floor)
        assert len(plain) == 2 and torch.equal(plain[0], u) and torch.equal(plain[1], w)
        un = u.cpu().numpy()
        assert (un >= 0).all() and (un < 1).all()
        kb = np.floor(un.astype(np.float64) * 64).astype(np.int64)
        assert np.array_equal(bits(w), bits(wt.cpu().numpy()[kb]))
        if name in ("empty", "short", "zero_s2"):
            assert np.array_equal(bits(u), bits(u0)) and bool((w == 1.0).all()) and bool((p == 2.0 ** -6).all())
        elif name == "flat":
            assert bool(((p - 2.0 ** -6).abs() < 1e-8).all())
        else:
            assert float(p.max()) > 4.0 * float(p.min())


# ---- through the model ----------------------------------------------------------------------------------------------------------------------
def _model(bs=8, dtype="fp32", **flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=bs, seed=3, timesteps=8, hidden_size=32, in_channels=1, image_size=8, compute_dtype=dtype)
    G.update(flags)
    torch.manual_seed(0)
    return Model(G).to("cuda").train()


def _batches(steps, B, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((B, 1, 8, 8), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()) for _ in range(steps)]


def _train(m, batches):
    losses = []
    for x, y in batches:
        losses.append(m.train_step(x, y.clone())["loss"])
    torch.cuda.synchronize()
    return torch.stack(losses).cpu()


@pytest.mark.parametrize("time_sampler", ["uniform", "stratified"])
def test_warm_up_is_the_run_without_the_flag(time_sampler):
    """Three train steps with time_importance 1 and a warm-up count that cannot be reached against three steps without the flag: the same
    parameters, losses and Philox counters, bit for bit - while the profile fills."""
    batches = _batches(3, 8)
    off = _model(time_sampler=time_sampler)
    on = _model(time_sampler=time_sampler, time_importance=1, importance_decay=1.0, importance_warmup=1e9)
    l_off, l_on = _train(off, batches), _train(on, batches)
    assert torch.equal(on.net.flat_params, off.net.flat_params)
    assert torch.equal(l_on, l_off)
    assert on.diffusion.rng.counter == off.diffusion.rng.counter and on._aux_rng.counter == off._aux_rng.counter
    assert off.diffusion.time_profile is None and "time_profile" not in off.train_state()
    prof = on.diffusion.time_profile
    assert float(prof[0].sum()) == 24.0 and float(prof[1].sum()) > 0
    assert not on.__dict__.get("_train_graphs")             # the profiled step runs kernel by kernel
    if time_sampler == "stratified":
        assert float(prof[0].max()) <= 3.0                  # B = 8 evenly spaced times: no bin takes two of one batch


def test_weighted_gradient_is_the_sum_of_weighted_single_image_passes():
    """B = 4, fp32 mode, a hand-set steep ready profile: flat_grads of one pass with time_importance against the sum of four single-image passes
    of a GaussianDiffusion without the flag at the returned u[b], the same eps[b] and grad_scale = time_w[b] / B, to 1e-3 of the largest
    entry; loss = time_w loss_b; the times come from the profile (not u0) and the profile took the unweighted losses."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    B = 4
    net = SimpleUnet(32, 0.0, in_channels=1, compute_dtype=torch.float32).cuda()
    (x, y), = _batches(1, B)
    eps = torch.randn((B, 1, 8, 8), generator=torch.Generator().manual_seed(2)).cuda()
    steep = R.steep_state(14.0)
    diff = GaussianDiffusion(mean_type="v", num_steps=8, seed=13, time_importance=1, importance_floor=0.5)
    diff.time_profile = dev(steep)
    u0 = ops.rng_uniform((B,), diff.rng.seed, 0, "cuda")
    out = diff.train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, eps=eps)
    assert set(out) == {"loss", "x_mse", "eps_mse", "logsnr", "u", "time_w", "loss_b"}
    assert diff.rng.counter == 1                            # eps was given: one uniform draw of four
    grads = net.flat_grads.clone()
    ru, rw, _, _ = R.u_importance(steep, u0.cpu().numpy(), 5.0, 0.5)
    assert np.array_equal(bits(out["u"]), bits(ru)) and np.array_equal(bits(out["time_w"]), bits(rw))
    assert not torch.equal(out["u"], u0) and not bool((out["time_w"] == 1.0).any())
    print("u0", u0.tolist(), "u", out["u"].tolist(), "time_w", out["time_w"].tolist())
    assert torch.equal(out["loss"], out["time_w"] * out["loss_b"])
    want_state = R.loss_profile(steep, ru, out["loss_b"].cpu().numpy(), out["x_mse"].cpu().numpy(), 0.9)
    assert np.array_equal(bits(diff.time_profile), bits(want_state))
    plain = GaussianDiffusion(mean_type="v", num_steps=8)
    total = torch.zeros_like(grads)
    for b in range(B):
        one = plain.train_forward_backward(net=partial(net, guide=y[b:b + 1].clone()), x=x[b:b + 1], grad_scale=float(out["time_w"][b]) / B,
                                           u=out["u"][b:b + 1], eps=eps[b:b + 1])
        assert set(one) == {"loss", "x_mse", "eps_mse", "logsnr"}
        assert torch.allclose(one["loss"], out["loss_b"][b:b + 1], rtol=TOL32, atol=0)
        total += net.flat_grads
    err = float((grads - total).abs().max() / total.abs().max())
    print(f"weighted gradient against four single-image passes: {err:.3e} of the largest entry")
    assert float(total.abs().max()) > 0 and err <= TOL32


def test_profile_alone_samples_nothing_and_fills_both_states():
    """loss_profile 1 without time_importance: the parameters of the run without flags, the train profile filled at importance_decay, the test
    pass summed at decay 1 into a state of its own and reset on read."""
    batches = _batches(2, 8)
    off, on = _model(), _model(loss_profile=1)
    _train(off, batches), _train(on, batches)
    assert torch.equal(on.net.flat_params, off.net.flat_params) and on.diffusion.rng.counter == off.diffusion.rng.counter
    rows = on.diffusion.profile("train")
    assert rows["p"] is None and 0 < rows["weight"].sum() <= 16.0
    with torch.no_grad():
        on.eval()
        l_on = [on.loss(x, y)[1] for x, y in batches]
        off.eval()
        l_off = [off.loss(x, y)[1] for x, y in batches]
    assert all(torch.equal(a["loss"], b["loss"]) for a, b in zip(l_on, l_off))
    test_rows = on.diffusion.profile("test", reset=True)
    assert test_rows["weight"].sum() == 16.0
    total = float(np.nansum(test_rows["loss_mean"] * test_rows["weight"])) / 16.0
    assert total == pytest.approx(float(sum(m["loss"] for m in l_on)) / 2, rel=1e-5)
    assert on.diffusion.profile("test")["weight"].sum() == 0.0
    assert on.diffusion.profile("train")["weight"].sum() == rows["weight"].sum()          # the test pass leaves the train profile alone


def test_resume_reaches_the_bits_of_the_straight_run(tmp_path):
    """Four steps straight against two steps, train_state() + state_dict() into a fresh model, two more: the same bits in the parameters and
    in time_profile.  B = 64 stratified puts one time into every bin per step, so with warm-up 1 the sampler is live from the second step."""
    flags = dict(bs=64, dtype="bf16", time_sampler="stratified", time_importance=1, importance_warmup=1, importance_floor=0.05)
    batches = _batches(4, 64)
    A = _model(**flags)
    _train(A, batches)
    Bm = _model(**flags)
    _train(Bm, batches[:2])
    assert float(Bm.diffusion.time_profile[0].min()) >= 1.0
    torch.save(Bm.state_dict(), tmp_path / "model.pt")
    torch.save(Bm.train_state(), tmp_path / "state.pt")
    C = _model(**flags)
    C.load_state_dict(torch.load(tmp_path / "model.pt", map_location="cuda"))
    state = torch.load(tmp_path / "state.pt", map_location="cpu")
    assert not state["time_profile"].is_cuda and torch.equal(state["time_profile"], Bm.diffusion.time_profile.cpu())
    C.load_train_state(state)
    _train(C, batches[2:])
    assert torch.equal(A.net.flat_params, C.net.flat_params)
    assert np.array_equal(bits(A.diffusion.time_profile), bits(C.diffusion.time_profile))
    assert A.diffusion.rng.counter == C.diffusion.rng.counter
    p = A.diffusion.profile("train")["p"]
    assert p is not None and p.max() > p.min() and abs(p.sum() - 1.0) < 1e-5          # the sampler has left uniform
    # the control: without the saved profile the continued run differs
    D = _model(**flags)
    D.load_state_dict(torch.load(tmp_path / "model.pt", map_location="cuda"))
    del state["time_profile"]
    D.load_train_state(state)
    _train(D, batches[2:])
    assert not torch.equal(A.net.flat_params, D.net.flat_params)


# ---- the command line ----------------------------------------------------------------------------------------------------------------------
def _driver(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR", "GMK_FORCE_EXCHANGE")}
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main"] + [str(a) for a in argv], capture_output=True, text=True, timeout=600,
                       cwd=ROOT, env=dict(env, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def _csv(path):
    lines = path.read_text().splitlines()
    return [dict(zip(lines[0].split(","), ln.split(","))) for ln in lines[1:]]


def test_cli(tmp_path):
    """One tiny epoch with --time_importance 1 --loss_profile 1 --save_state 1 writes loss_profile.csv: 64 test rows per evaluation whose weights
    sum to the test images, 64 train rows once the train pass ran (with p); --resume continues the run and the file; the default command line
    writes no such file."""
    import yaml
    base = ["--model=diffusion", "--bs", "8", "--timesteps", "4", "--train_batches", "2", "--test_batches", "2", "--eval_heavy", "0", "--save_n", "1"]
    run = tmp_path / "run"
    _driver(base + ["--time_importance", "1", "--loss_profile", "1", "--save_state", "1", "--epochs", "1", "--logdir", run])
    hps = yaml.load((run / "hps.yaml").read_text(), Loader=yaml.Loader)
    assert (hps["time_importance"], hps["loss_profile"], hps["importance_decay"]) == (1, 1, 0.9)
    rows = _csv(run / "loss_profile.csv")
    groups = {}
    for r in rows:
        groups.setdefault((int(r["epoch"]), r["split"]), []).append(r)
    assert set(groups) == {(0, "test"), (1, "test"), (1, "train")} and all(len(g) == 64 for g in groups.values())
    for epoch in (0, 1):
        assert sum(float(r["weight"]) for r in groups[(epoch, "test")]) == 16.0
        assert all(r["p"] == "" for r in groups[(epoch, "test")])
    train = groups[(1, "train")]
    assert 0 < sum(float(r["weight"]) for r in train) <= 16.0 and all(float(r["p"]) == 2.0 ** -6 for r in train)      # inside the warm-up
    assert (float(train[0]["logsnr_hi"]), [r["bin"] for r in train]) == (20.0, [str(k) for k in range(64)])
    state = torch.load(run / "train_state.pt", map_location="cpu")
    assert state["version"] == 1
    assert float(state["model"]["time_profile"][0].double().sum()) == pytest.approx(sum(float(r["weight"]) for r in train), rel=1e-7)
    out = _driver(["--resume", run, "--epochs", "2"])
    assert "RESUMED" in out
    rows = _csv(run / "loss_profile.csv")
    assert {(int(r["epoch"]), r["split"]) for r in rows} == {(0, "test"), (1, "test"), (1, "train"), (2, "test"), (2, "train")}
    later = [r for r in rows if (r["epoch"], r["split"]) == ("2", "train")]
    assert sum(float(r["weight"]) for r in later) > sum(float(r["weight"]) for r in train)
    plain = tmp_path / "plain"
    _driver(base + ["--epochs", "1", "--logdir", plain])
    assert (plain / "model.pt").exists() and not (plain / "loss_profile.csv").exists()
