"""GPU tests of post-hoc EMA (DG.ema_sigma_rel): gmk_adam_pema_step against the existing Adam entries bit for bit, gmk_arena_combine against
the float64 loop of tests/posthoc_ema_ref.py bit for bit, the power-function averages through the train step (graphed and kernel by kernel,
16-bit and fp32 modes), snapshots and reconstruction, resume, and the command line."""
import csv
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posthoc_ema_ref as R  # noqa: E402

ADAM = (3e-4, 0.9, 0.999, 1e-8)
# (ema_w, pw) per step: a weight of exactly 1 on step 1, then both sides of lerp_to's 0.5 switch
STEP_WEIGHTS = ((1.0, (1.0, 1.0, 1.0)), (0.45, (0.9, 0.6, 0.5)), (0.001, (3e-5, 0.49, 0.51)))


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


def _decay(w):
    """The decay_t under which the existing ops hand the kernel the fp32 weight the new op gets from w."""
    d = 1.0 - w
    assert np.float32(1.0 - d) == np.float32(w)
    return d


# ---- the fused kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["tight", "padded"])
@pytest.mark.parametrize("n_pema", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 3, 1003, 262147])
def test_pema_step_carries_the_bits_of_the_existing_entries(n, n_pema, layout):
    """Three steps (then, steered, a fourth the guard skips) of ops.adam_pema_step with the classic average on and off, steered and
    unsteered: p, m, v torch.equal to adam_step / adam_step_ctl on clones, `ema` and every row to adam_ema_step on clones (steered: on the
    gradient pre-scaled by the clipping coefficient, whose p is checked too).  'tight': rows of stride n (16-byte row accesses only when n % 4
    == 0, never here past n = 3); 'padded': an aligned stride beyond n, whose padding must keep its bits."""
    from generative_models_amd import ops
    stride = n if layout == "tight" else (n + 3) // 4 * 4 + 4
    gen = torch.Generator(device="cuda").manual_seed(n * 8 + n_pema)
    r = lambda: torch.randn(n, device="cuda", generator=gen)
    for with_ema in (False, True):
        for steered in (False, True):
            p, m, v, ema = r(), r() * 0.01, r().abs() * 1e-4, r()
            store = torch.randn((n_pema, stride), device="cuda", generator=gen)          # garbage: step 1 (w = 1) must overwrite it
            pema = store[:, :n]
            pad = store[:, n:].clone()
            state = torch.tensor([0.0, 1.0, 1.0, 0.0], device="cuda") if steered else None
            for step, (ema_w, pws) in enumerate(STEP_WEIGHTS, start=1):
                grad = r() * 8
                if steered:
                    ops.grad_norm(grad, state, 0.125, 1e-4 * math.sqrt(n))               # norm ~ sqrt(n): clips, with a coefficient near 1e-4
                    assert float(state[ops.APPLY]) == 1.0 and float(state[ops.CLIP_COEF]) < 1.0
                pa, ma, va = p.clone(), m.clone(), v.clone()
                if steered:
                    ops.adam_step_ctl(pa, grad, ma, va, state, *ADAM, step, grad_scale=0.125)
                    g_ref, gs_ref = (grad * 0.125) * state[ops.CLIP_COEF], 1.0           # what the steered kernel feeds adam_elem
                else:
                    ops.adam_step(pa, grad, ma, va, *ADAM, step, grad_scale=0.125)
                    g_ref, gs_ref = grad, 0.125
                rows_ref = []
                for w, start in [(pw, pema[k]) for k, pw in enumerate(pws[:n_pema])] + ([(ema_w, ema)] if with_ema else []):
                    pb, mb, vb, eb = p.clone(), m.clone(), v.clone(), start.clone()
                    ops.adam_ema_step(pb, g_ref, mb, vb, eb, *ADAM, step, _decay(w), grad_scale=gs_ref)
                    assert torch.equal(pb, pa) and torch.equal(mb, ma) and torch.equal(vb, va)
                    rows_ref.append(eb)
                ops.adam_pema_step(p, grad, m, v, pema, pws[:n_pema], *ADAM, step, grad_scale=0.125, ema=ema if with_ema else None,
                                   decay_t=_decay(ema_w), state=state)
                assert torch.equal(p, pa) and torch.equal(m, ma) and torch.equal(v, va), (with_ema, steered, step)
                for k in range(n_pema):
                    assert torch.equal(pema[k], rows_ref[k]), (with_ema, steered, step, k)
                    if step == 1:
                        assert torch.equal(pema[k], p)
                if with_ema:
                    assert torch.equal(ema, rows_ref[-1])
                    if step == 1:
                        assert torch.equal(ema, p)
                assert torch.equal(store[:, n:], pad)
            if steered:                                                                  # apply = 0: nothing changes, `skipped` counts
                grad = r()
                grad[0] = float("inf")
                ops.grad_norm(grad, state, 0.125, 0.5)
                assert float(state[ops.APPLY]) == 0.0 and float(state[ops.SKIPPED]) == 1.0
                keep = [t.clone() for t in (p, m, v, ema, store)]
                ops.adam_pema_step(p, grad, m, v, pema, (0.5, 0.5, 0.5)[:n_pema], *ADAM, 4, grad_scale=0.125, ema=ema if with_ema else None,
                                   decay_t=0.5, state=state)
                assert all(torch.equal(a, b) for a, b in zip((p, m, v, ema, store), keep))
                assert float(state[ops.SKIPPED]) == 1.0


def test_pema_step_refuses_bad_arguments():
    from generative_models_amd import ops
    from generative_models_amd._lib import GmkError
    n = 64
    p, g, m, v = (torch.zeros(n, device="cuda") for _ in range(4))
    call = lambda pema, w: ops.adam_pema_step(p, g, m, v, pema, w, *ADAM, 1)
    rows = lambda k, width=n: torch.zeros((k, width), device="cuda")
    with pytest.raises(GmkError, match="n_pema"):
        call(rows(4), (0.5,) * 4)
    with pytest.raises(GmkError, match="n_pema"):
        call(rows(0), ())
    for bad in (-0.25, 1.5, float("nan")):
        with pytest.raises(GmkError, match="pw1"):
            call(rows(2), (0.5, bad))
    with pytest.raises(GmkError, match="pema_stride"):
        call(rows(2, n - 1), (0.5, 0.5))
    with pytest.raises(GmkError, match="ema_w"):
        ops.adam_pema_step(p, g, m, v, rows(1), (0.5,), *ADAM, 1, ema=torch.zeros(n, device="cuda"), decay_t=1.5)
    assert not p.any() and not m.any()                                                   # refused before any launch
    call(rows(3), (1.0, 0.0, 0.5))


# ---- the combine kernel ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 1003])
@pytest.mark.parametrize("K", [1, 2, 5, 64])
def test_arena_combine_equals_the_float64_loop(K, n):
    """torch.equal to the sequential float64 loop, on an aligned row stride (16-byte loads and the n & 3 tail) and on one that breaks the
    alignment (scalar loads); rows 0 and 1 are nearly equal under the cancelling pair (1e3, -1e3 + 1e-3)."""
    from generative_models_amd import ops
    rng = np.random.default_rng(K * 4096 + n)
    rows = rng.standard_normal((K, n)).astype(np.float32)
    coef = rng.standard_normal(K)
    if K >= 2:
        rows[1] = np.nextafter(rows[0], np.float32(np.inf)) if n < 5 else rows[0] * np.float32(1.0 + 2.0 ** -20)
        coef[0], coef[1] = 1e3, -1e3 + 1e-3
    want = torch.from_numpy(R.combine(rows, coef))
    for stride in ((n + 3) // 4 * 4, (n + 3) // 4 * 4 + 1):
        store = torch.full((K, stride), float("nan"), device="cuda")
        store[:, :n] = torch.from_numpy(rows)
        got = ops.arena_combine(store[:, :n] if K > 1 else store, coef, n=n)
        assert got.dtype == torch.float32 and tuple(got.shape) == (n,)
        assert torch.equal(got.cpu(), want), (stride, float((got.cpu() - want).abs().max()))
    if K == 1:                                                                           # coefficient 1.0: a copy
        src = torch.from_numpy(rows).cuda()
        assert torch.equal(ops.arena_combine(src, [1.0]), src[0])


def test_arena_combine_refuses_bad_arguments():
    from generative_models_amd import ops
    from generative_models_amd._lib import GmkError
    n = 40
    with pytest.raises(GmkError, match="K = 0"):
        ops.arena_combine(torch.zeros((0, n), device="cuda"), [], n=n)
    with pytest.raises(GmkError, match="K = 65"):
        ops.arena_combine(torch.zeros((65, n), device="cuda"), [1.0] * 65)
    src = torch.zeros((3, n), device="cuda")
    for out in (src[0], src[2], src.view(-1)[n - 1:2 * n - 1]):
        with pytest.raises(GmkError, match="aliases"):
            ops.arena_combine(src, [1.0, 2.0, 3.0], out=out)
    with pytest.raises(ValueError):
        ops.arena_combine(src, [1.0, 2.0])
    with pytest.raises(GmkError, match="src_stride"):
        ops.arena_combine(src, [1.0, 2.0, 3.0], n=n + 1)


# ---- the train step --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp32"])
@pytest.mark.parametrize("graphed", [True, False])
def test_training_is_untouched_and_the_recurrence_holds(dtype, graphed):
    """Five steps with ema_sigma_rel = '0.05,0.1': the net arena is torch.equal to a run without the flag, with ema_decay added the classic
    average is torch.equal to ema_decay alone, and each power-function arena follows the float64 recurrence over per-step weight snapshots
    (the tolerance of test_gpu_ema.py's chain of the same kind)."""
    batches = _batches(5)
    sigma = "0.05,0.1"
    runs = {}
    for name, flags in (("plain", {}), ("pema", dict(ema_sigma_rel=sigma)), ("ema", dict(ema_decay=0.999)),
                        ("both", dict(ema_decay=0.999, ema_sigma_rel=sigma))):
        m = _model(compute_dtype=dtype, timesteps=8, **flags)
        if not graphed:
            m.TRAIN_GRAPH_MAX_PIXELS = 0
        snaps = []
        for x, y in batches:
            m.train_step(x, y.clone())
            snaps.append(m.net.flat_params.double())
        assert len(m.__dict__.get("_train_graphs", {})) == (1 if graphed else 0)
        runs[name] = (m, snaps)
    plain, pema, ema, both = (runs[k][0] for k in ("plain", "pema", "ema", "both"))
    assert plain.optimizer.pema is None and ema.optimizer.pema is None
    for m in (pema, ema, both):
        assert torch.equal(m.net.flat_params, plain.net.flat_params)
    assert torch.equal(both.ema_net.flat_params, ema.ema_net.flat_params)
    assert torch.equal(both.optimizer.pema, pema.optimizer.pema)
    m, snaps = runs["pema"]
    assert tuple(m.optimizer.pema.shape) == (2, m.net.flat_params.numel()) and m.optimizer.step_count == 5
    for k, s in enumerate((0.05, 0.1)):
        gamma = R.gamma_root(s)
        e = torch.zeros_like(snaps[0])
        for t, p in enumerate(snaps, start=1):
            w = float(R.weight(gamma, t))
            e = (1.0 - w) * e + w * p
        got = m.optimizer.pema[k].double()
        assert torch.allclose(got, e, rtol=1e-6, atol=1e-6 * float(e.abs().max())), (k, float((got - e).abs().max()))
        assert not torch.equal(m.optimizer.pema[k], m.net.flat_params)
    assert not torch.equal(m.optimizer.pema[0], m.optimizer.pema[1])


def test_snapshot_reconstruct_compare(tmp_path):
    """24 steps tracking 0.05, 0.07 and 0.1 with a snapshot every 2: a tracked width at the last snapshot comes back to 1 ulp, and 0.07 rebuilt
    from the other two lies within 2.5e-3 M (the trajectory-free bound of tests/test_host_posthoc_ema.py, M = max |theta|) + 1e-5 M (the fp32
    rounding of 24 lerps) of the tracked 0.07 arena."""
    from generative_models_amd import posthoc_ema as P
    m = _model(timesteps=8, ema_sigma_rel="0.05,0.07,0.1", ema_snapshot_every=2, logdir=tmp_path)
    M = 0.0
    for x, y in _batches(24):
        m.train_step(x, y)
        M = max(M, float(m.net.flat_params.abs().max()))
    files = P.list_snapshots(tmp_path)
    assert [s for s, _ in files] == list(range(2, 25, 2))
    last = torch.load(files[-1][1], map_location="cpu")
    assert last["step"] == 24 and last["sigma_rel"] == [0.05, 0.07, 0.1] and last["layout"] == P.layout_digest(m.net.flat_params.numel())
    assert torch.equal(last["arenas"], m.optimizer.pema.cpu())
    got = P.reconstruct(tmp_path, 0.1)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == m.net.flat_params.shape
    assert _within_one_ulp(got, m.optimizer.pema[2]), float((got - m.optimizer.pema[2]).abs().max())
    got = P.reconstruct(tmp_path, 0.07, profiles=(0.05, 0.1))
    err = float((got - m.optimizer.pema[1]).abs().max())
    print(f"M = {M:.4f}, max |reconstructed - tracked| = {err:.3e} = {err / M:.3e} M")
    assert err <= 2.5e-3 * M + 1e-5 * M
    assert not torch.equal(got, m.net.flat_params)                                       # an average, not the online weights
    early = P.reconstruct(tmp_path, 0.07, at_step=12)
    assert not torch.equal(early, got)


def test_resume_reaches_the_bits_of_the_uninterrupted_run(tmp_path):
    from generative_models_amd import posthoc_ema as P
    flags = dict(timesteps=8, ema_sigma_rel="0.05,0.1", grad_clip=1.0)
    batches = _batches(12)
    A = _model(**flags)
    for x, y in batches:
        A.train_step(x, y.clone())
    B = _model(**flags)
    for x, y in batches[:6]:
        B.train_step(x, y.clone())
    B.save(tmp_path)
    torch.save(B.train_state(), tmp_path / "state.pt")
    assert [s for s, _ in P.list_snapshots(tmp_path)] == [6]                             # save() snapshots the averages
    state = torch.load(tmp_path / "state.pt", map_location="cpu")
    assert tuple(state["optimizer"]["pema"].shape) == (2, A.net.flat_params.numel())
    assert set(state["digests"]) == {"params", "ema", "m", "v", "pema0", "pema1"} and state["digests"]["pema1"] is not None
    C = _model(**flags)
    C.load_state_dict(torch.load(tmp_path / "model.pt", map_location="cuda"))
    C.load_train_state(state)
    assert C.optimizer.pema.is_cuda and torch.equal(C.optimizer.pema, B.optimizer.pema)
    for x, y in batches[6:]:
        C.train_step(x, y.clone())
    assert torch.equal(C.net.flat_params, A.net.flat_params)
    for k in range(2):
        assert torch.equal(C.optimizer.pema[k], A.optimizer.pema[k]), k
    assert C.arena_digests() == A.arena_digests()
    # a power-function arena that does not carry its digest is refused by name
    state = torch.load(tmp_path / "state.pt", map_location="cpu")
    state["digests"]["pema1"] ^= 1
    D = _model(**flags)
    D.load_state_dict(torch.load(tmp_path / "model.pt", map_location="cuda"))
    with pytest.raises(RuntimeError, match="pema1"):
        D.load_train_state(state)
    # and a state saved without the averages by a run that tracks them
    E = _model(timesteps=8, grad_clip=1.0)
    E.train_step(*batches[0])
    with pytest.raises(ValueError, match="ema_sigma_rel"):
        D.optimizer.load_state_dict(E.optimizer.state_dict())


# ---- the command line ------------------------------------------------------------------------------------------------------------------
def _run(module, argv):
    r = subprocess.run([sys.executable, "-m", module] + [str(a) for a in argv], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_train_reconstruct_sweep_and_load(tmp_path):
    run = tmp_path / "run"
    _run("generative_models_amd.main", ["--model=diffusion", "--epochs=1", "--bs", "8", "--timesteps", "4", "--data", "synthetic",
                                        "--ema_sigma_rel", "0.05,0.1", "--ema_snapshot_every", "2", "--train_batches", "6", "--test_batches", "1",
                                        "--eval_heavy", "0", "--save_n", "1", "--logdir", run])
    steps = sorted(p.name for p in (run / "ema_snapshots").iterdir())
    assert steps == [f"step_{t:09d}.pt" for t in (2, 4, 6)]
    out = _run("generative_models_amd.posthoc_ema", ["--run", run, "--sigma_rel", "0.07", "--sweep", "0.05,0.07,0.1", "--sweep_batches", "1"])
    weights = run / "model_ema_0.07.pt"
    assert weights.exists() and f"WROTE {weights}" in out
    sd, online = torch.load(weights, map_location="cpu"), torch.load(run / "model.pt", map_location="cpu")
    assert list(sd) == list(online) and len(sd) == 160 and not all(torch.equal(sd[k], online[k]) for k in sd)
    with open(run / "ema_sweep.csv") as f:
        rows = list(csv.DictReader(f))
    assert [r["sigma_rel"] for r in rows] == ["0.05", "0.07", "0.1", "online"]
    assert list(rows[0])[:4] == ["sigma_rel", "at_step", "n_arenas", "fit_residual"] and "loss" in rows[0]
    for r in rows:
        assert math.isfinite(float(r["loss"]))
        if r["sigma_rel"] != "online":
            assert r["at_step"] == "6" and r["n_arenas"] == "6"
    for r in (rows[0], rows[2]):                                                          # tracked widths at the snapshot step
        assert float(r["fit_residual"]) <= 1e-6
    assert len({r["loss"] for r in rows}) > 1                                             # same images, times and noise: the rows differ by the weights
    out = _run("generative_models_amd.main", ["--weights_from", weights, "--skip_training", "1", "--epochs", "0", "--eval_heavy", "0",
                                              "--logdir", tmp_path / "eval"])
    assert "diffusion/test/loss" in out
