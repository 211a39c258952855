"""GPU tests of the weight EMA extension (DG.ema_decay > 0): the fused Adam + EMA kernel against the plain Adam kernel and torch.lerp, the
average through the train step (graphed and kernel by kernel, 16-bit and fp32 modes), sampling from it (captured-graph and two-stream sampler
paths), checkpoints and the CLI."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECAY = 0.999


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=8, seed=3)
    G.update(flags)
    torch.manual_seed(0)
    return Model(G).to("cuda")


def _batches(n, B=8, seed=5):
    g = torch.Generator().manual_seed(seed)
    return [((torch.rand((B, 1, 28, 28), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (B,), generator=g).cuda()) for _ in range(n)]


def _within_one_ulp(got, ref):
    ulp = torch.nextafter(ref.abs(), torch.full_like(ref, float("inf"))) - ref.abs()
    return bool(((got - ref).abs() <= ulp).all())


@pytest.mark.parametrize("n", [1003, 6033665])
def test_fused_kernel_matches_adam_and_lerp(n):
    """p, m, v the same bits as ops.adam_step; ema within 1 ulp of torch's lerp_ on the new weights, on both sides of torch.lerp's w = 0.5
    switch; decay 0 copies p_new exactly, ema_w = 0 leaves ema untouched.  Odd lengths exercise the n & 3 tail (n = 6,033,665: the
    configs[2] arena)."""
    from generative_models_amd import ops
    g = torch.Generator(device="cuda").manual_seed(n)
    r = lambda: torch.randn(n, device="cuda", generator=g)
    p, m, v, ema = r(), r() * 0.01, r().abs() * 1e-4, r()
    for step, decay in ((1, 0.1), (2, 0.75), (3, 0.999)):
        grad = r() * 8
        pa, ma, va = p.clone(), m.clone(), v.clone()
        ops.adam_step(pa, grad, ma, va, 3e-4, 0.9, 0.999, 1e-8, step, grad_scale=0.125)
        ema0 = ema.clone()
        ops.adam_ema_step(p, grad, m, v, ema, 3e-4, 0.9, 0.999, 1e-8, step, decay, grad_scale=0.125)
        assert torch.equal(p, pa) and torch.equal(m, ma) and torch.equal(v, va)
        ref = ema0.lerp_(p, 1.0 - decay)
        assert _within_one_ulp(ema, ref), float((ema - ref).abs().max())
    grad = r()
    ops.adam_ema_step(p, grad, m, v, ema, 3e-4, 0.9, 0.999, 1e-8, 4, 0.0)
    assert torch.equal(ema, p)
    keep = ema.clone()
    ops.adam_ema_step(p, grad, m, v, ema, 3e-4, 0.9, 0.999, 1e-8, 5, 1.0)
    assert torch.equal(ema, keep) and not torch.equal(ema, p)
    from generative_models_amd._lib import GmkError
    with pytest.raises(GmkError):
        ops.adam_ema_step(p, grad, m, v, ema, 3e-4, 0.9, 0.999, 1e-8, 6, -0.5)


@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("graphed", [True, False])
def test_train_steps_leave_training_alone_and_follow_the_recurrence(dtype, graphed):
    """EMA on must not move training by one bit: after 5 steps the net arenas of decay 0 and decay 0.999 are equal.  The average equals a
    float64 recomputation of the warm-up recurrence over snapshots of the weights after every step (seeded from the weights before the
    first)."""
    from generative_models_amd.diffusion.optim import ema_decay_at
    batches = _batches(5)
    runs = []
    for decay in (0.0, DECAY):
        m = _model(compute_dtype=dtype, timesteps=8, ema_decay=decay)
        if not graphed:
            m.TRAIN_GRAPH_MAX_PIXELS = 0
        snaps = [m.net.flat_params.double()]
        for x, y in batches:
            m.train_step(x, y.clone())
            snaps.append(m.net.flat_params.double())
        assert len(m.__dict__.get("_train_graphs", {})) == (1 if graphed else 0)
        runs.append((m, snaps))
    (plain, _), (m, snaps) = runs
    assert torch.equal(plain.net.flat_params, m.net.flat_params)
    e = snaps[0]
    for t, p in enumerate(snaps[1:]):
        d = ema_decay_at(DECAY, t)
        e = d * e + (1.0 - d) * p
    got = m.ema_net.flat_params.double()
    assert torch.allclose(got, e, rtol=1e-6, atol=1e-6 * float(e.abs().max())), float((got - e).abs().max())
    assert not torch.equal(m.ema_net.flat_params, m.net.flat_params)


@pytest.mark.parametrize("path", ["graph", "two_stream"])
def test_sample_runs_on_the_average(path):
    """model.sample with EMA on equals, bit for bit, the sample of a plain model whose net holds the ema_net.* weights (same Philox streams),
    and differs from the online net's.  'graph': 8 images at T = 16 replay a captured forward of the EMA net; 'two_stream': 672 images take
    the sampler's two half-batches on two streams, whose re-pack before the fork must hold for the EMA net too."""
    T, n = (16, 8) if path == "graph" else (4, 672)
    m = _model(timesteps=T, ema_decay=DECAY)
    for x, y in _batches(3):
        m.train_step(x, y)
    sd = m.state_dict()
    forks = []
    m.diffusion._chunk_streams = (lambda orig: lambda dev, K: forks.append(K) or orig(dev, K))(m.diffusion._chunk_streams)
    y = torch.arange(n, device="cuda") % 10

    def plain_with(prefix):
        p = _model(timesteps=T)
        p.load_state_dict({"net." + k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)})
        p._aux_rng.counter, p.diffusion.rng.counter = m._aux_rng.counter, m.diffusion.rng.counter
        return p.sample(n, y)

    want, online = plain_with("ema_net."), plain_with("net.")
    got = m.sample(n, y)
    assert torch.equal(got, want) and not torch.equal(got, online)
    if path == "graph":
        assert forks == [] and any(key[0] == id(m.ema_net) for key in m.diffusion._graphs)
    else:
        assert forks == [2] and not m.diffusion._graphs


@pytest.mark.parametrize("C", [128, 96])
def test_checkpoint_round_trip(C, tmp_path):
    """save -> load into a fresh model: 320 keys, both arenas restored bit for bit (also at the zero-padded width 96, whose padding stays zero
    in the average); a 160-key checkpoint seeds the average from the loaded weights; EMA off saves exactly today's 160 keys."""
    m = _model(hidden_size=C, timesteps=8, ema_decay=DECAY)
    for x, y in _batches(2):
        m.train_step(x, y)
    m.save(tmp_path)
    sd = torch.load(tmp_path / "model.pt", map_location="cpu")
    assert len(sd) == 320 and sum(k.startswith("ema_net.") for k in sd) == 160
    fresh = _model(hidden_size=C, timesteps=8, ema_decay=DECAY)
    fresh.load_state_dict(sd)
    assert torch.equal(fresh.ema_net.flat_params, m.ema_net.flat_params) and torch.equal(fresh.net.flat_params, m.net.flat_params)
    if C == 96:
        pad = m.net.flat_params == 0
        assert bool((m.ema_net.flat_params[pad & (m.net.flat_grads == 0)] == 0).all())
    seeded = _model(hidden_size=C, timesteps=8, ema_decay=DECAY)
    seeded.load_state_dict({k: v for k, v in sd.items() if k.startswith("net.")})
    assert torch.equal(seeded.ema_net.flat_params, seeded.net.flat_params)
    off = _model(hidden_size=C, timesteps=8)
    off.train_step(*_batches(1)[0])
    assert len(off.state_dict()) == 160


def test_cli_with_ema(tmp_path):
    import yaml
    run = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main", "--model=diffusion", "--epochs=1", "--bs", "8", "--timesteps", "4",
                        "--ema_decay", "0.999", "--train_batches", "3", "--test_batches", "1", "--eval_heavy", "0", "--save_n", "1",
                        "--logdir", str(run)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    with open(run / "hps.yaml") as f:
        assert yaml.load(f, Loader=yaml.Loader)["ema_decay"] == 0.999
    sd = torch.load(run / "model.pt", map_location="cpu")
    assert len(sd) == 320 and not all(torch.equal(sd[k], sd["ema_net." + k[4:]]) for k in sd if k.startswith("net."))
