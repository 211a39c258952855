"""Host tests of the training objective's table (no GPU): `LOSS_TABLE` against the `ops` wrappers it names, what the two training passes return
for every row and grad mode, the order of a step's first two draws at every place that makes them, and the one autograd bridge.  The passes run
on the CPU with the `ops` functions they call and the network's forward / backward replaced by stand-ins."""
import inspect
from functools import partial
from types import SimpleNamespace

import pytest
import torch

from generative_models_amd import ops
from generative_models_amd.diffusion import gaussian_diffusion as gd
from generative_models_amd.diffusion.gaussian_diffusion import LOSS_TABLE, GaussianDiffusion, loss_row

B, S = 4, 8
ROWS = {            # row name -> the options that select it (a teacher: the stand-in network below)
    "snr_trunc": dict(), "snr": dict(loss_weight="snr"), "snr_plus1": dict(loss_weight="snr_plus1"), "min_snr": dict(loss_weight="min_snr"),
    "huber": dict(teacher_mode="consistency", consistency_loss="huber"), "hybrid": dict(learn_var=1)}
N_OUT = {"v_loss": 3, "x_loss_w": 2, "x_loss_huber": 2, "hybrid_loss": 5}       # per-image outputs ahead of the gradients


class Net(torch.nn.Module):
    """What the passes ask of a network, without kernels: v = w x (so autograd reaches a parameter), nu = v / 4."""

    def __init__(self, learn_var=False):
        super().__init__()
        self.learn_var, self.w = learn_var, torch.nn.Parameter(torch.tensor(0.5))
        self.backward_calls = []

    def forward_hip(self, x, logsnr, guide=None, cond_w=None, ctx=None, want_nu=False):
        v = x * self.w.detach() if ctx is not None or not torch.is_grad_enabled() else x * self.w
        return (v, v * 0.25) if want_nu else v

    def forward(self, x, logsnr, guide=None, cond_w=None, want_nu=False):
        return self.forward_hip(x, logsnr, guide, cond_w, want_nu=want_nu)

    def backward_hip(self, ctx, dout, on_grads_ready=None, join_side_before_ready=True, dnu=None):
        self.backward_calls.append((dout, dnu))


@pytest.fixture
def calls(monkeypatch):
    """The `ops` functions of a training pass as CPU stand-ins; -> the list of (name, arguments by parameter name) they were called with."""
    log = []

    def standin(name, fake):
        sig = inspect.signature(getattr(ops, name))

        def f(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            log.append((name, dict(bound.arguments)))
            return fake(**bound.arguments)
        monkeypatch.setattr(ops, name, f)

    def loss(name, wrt):
        def fake(**kw):
            base = kw["v"].reshape(B, -1).sum(1)
            return tuple(base * (i + 1) for i in range(N_OUT[name])) + tuple(torch.ones_like(kw[w]) if kw["grad_scale"] is not None else None for w in wrt)
        standin(name, fake)
    for name, wrt in (("v_loss", ("v",)), ("x_loss_w", ("v",)), ("x_loss_huber", ("v",)), ("hybrid_loss", ("v", "nu"))):
        loss(name, wrt)
    standin("scale_rows", lambda x, rowscale: x * rowscale[:, None])
    standin("loss_profile", lambda u, v0, v1, state, decay: state)
    standin("u_importance", lambda state, u0, warm, floor, want_table: (u0, u0 + 1.0))
    standin("q_sample", lambda x, eps, u, schedule: (10.0 - 20.0 * u, x + eps))
    standin("logsnr_schedule", lambda B, device, u, i_times, num_steps, shift, want_u, schedule:
            (torch.zeros(B), torch.full((B,), 0.5)) if want_u else torch.zeros(B))
    standin("ddim_step_vec", lambda v, z, logsnr_t, logsnr_s, v_uncond, cond_w, mean_type: (z, v, v))
    standin("consistency_target", lambda v_tgt, z_s, x_pred_teacher, z_t, logsnr_t, logsnr_s, i_times, mean_type: (v_tgt, z_t))
    standin("rng_normal", lambda shape, seed, offset, device: torch.ones(shape))
    standin("rng_uniform", lambda shape, seed, offset, device: torch.full(shape, 0.25))
    standin("u_stratified", lambda u0, B: torch.full((B,), 0.25))
    return log


def _diffusion(row, **kw):
    opts = dict(ROWS[row], **kw)
    if "teacher_mode" in opts:
        opts["teacher_net"] = Net()
    return GaussianDiffusion(mean_type="v", num_steps=4, seed=5, **opts)


def _x():
    return torch.linspace(-1, 1, B * S * S).view(B, 1, S, S)


# ---- the table ---------------------------------------------------------------------------------------------------------------------------------
def test_every_objective_resolves_to_one_row():
    """Every value `loss_weight_type` can take (the caller's four, 'snr' through distillation step 1, 'huber' through consistency distillation),
    with learn_var on and off where the option checks allow it, is the key of exactly one row; learn_var selects the hybrid row."""
    seen = set()
    for weight in gd.LOSS_WEIGHTS:
        for learn_var in (0, 1):
            if learn_var and weight not in ("snr_trunc", "snr"):
                with pytest.raises(ValueError, match="learn_var.*loss_weight"):
                    GaussianDiffusion(mean_type="v", num_steps=4, loss_weight=weight, learn_var=1)
                continue
            d = GaussianDiffusion(mean_type="v", num_steps=4, loss_weight=weight, learn_var=learn_var)
            assert d.loss_weight_type == weight and loss_row(d) is LOSS_TABLE["hybrid" if learn_var else weight]
            seen.add("hybrid" if learn_var else weight)
    for opts, weight in ((dict(teacher_mode="step1"), "snr"), (dict(teacher_mode="step2"), "snr_trunc"), (dict(teacher_mode="consistency"), "snr_trunc"),
                         (dict(teacher_mode="consistency", consistency_loss="huber"), "huber")):
        d = GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=Net(), **opts)
        assert d.loss_weight_type == weight and loss_row(d) is LOSS_TABLE[weight]
        seen.add(weight)
    assert seen == set(LOSS_TABLE) == set(ROWS)
    assert LOSS_TABLE["snr_trunc"] is LOSS_TABLE["snr"] and LOSS_TABLE["snr_plus1"] is LOSS_TABLE["min_snr"]      # one wrapper, told apart by a scalar


@pytest.mark.parametrize("name", sorted(LOSS_TABLE))
def test_rows_describe_their_wrappers(name):
    """The wrapper exists, its signature is what `_loss` calls - the tensors the row says it reads, in order, then the row's scalars, grad_scale and
    mean_type - and `outs` names its return tuple, gradients last."""
    row = LOSS_TABLE[name]
    params = list(inspect.signature(getattr(ops, row.op)).parameters)
    tensors = ["v"] + ["nu"] * row.nu + ["z", "x"] + ["eps"] * row.eps + ["logsnr"] + ["logsnr_s"] * row.nu
    assert params[:len(tensors)] == tensors
    assert sorted(params[len(tensors):]) == sorted([kw for kw, _ in row.scalars] + ["grad_scale", "mean_type"])
    assert row.outs[0] == "loss" and "x_mse" in row.outs and row.outs[-len(row.grads):] == row.grads
    assert row.grads == (("dv", "dnu") if row.nu else ("dv",)) and len(row.outs) == N_OUT[row.op] + len(row.grads)
    d = SimpleNamespace(loss_weight_type=name, loss_gamma=5.0, consistency_huber_c=0.001, vlb_lambda=0.001)
    assert all(attr is None or hasattr(d, attr) for _, attr in row.scalars)


def test_wrappers_return_what_the_rows_name(monkeypatch):
    """The real wrappers' return tuples, with the library behind them replaced: len(outs), the gradients None without grad_scale."""
    class Lib:
        def __getattr__(self, entry):
            return lambda *args: 0
    monkeypatch.setattr(ops, "lib", Lib())
    monkeypatch.setattr(ops, "_s", lambda: None)
    monkeypatch.setattr(ops, "_images", lambda tensors, vectors=(), what="": (B, S * S))
    t, l = _x(), torch.zeros(B)
    for name, row in LOSS_TABLE.items():
        tensors = (t,) * (3 + row.nu + row.eps) + (l,) * (1 + row.nu)
        kw = {kw: {"loss_type": 0, "weight": "min_snr", "gamma": 5.0, "c": 0.001, "vlb_lambda": 0.001}[kw] for kw, _ in row.scalars}
        for gs in (None, 0.25):
            ret = getattr(ops, row.op)(*tensors, grad_scale=gs, **kw)
            assert len(ret) == len(row.outs)
            for out_name, val in zip(row.outs, ret):
                assert (val is None) == (out_name in row.grads and gs is None), (name, out_name)


# ---- what the passes return -------------------------------------------------------------------------------------------------------------------
TL_KEYS = {"hybrid": {"loss", "vlb", "var_frac"}, "huber": {"loss", "x_mse"}, "snr_plus1": {"loss", "x_mse"}, "min_snr": {"loss", "x_mse"}}
TFB_KEYS = {"hybrid": ["loss", "x_mse", "eps_mse", "logsnr", "vlb", "var_frac"], "snr_trunc": ["loss", "x_mse", "eps_mse", "logsnr"],
            "snr": ["loss", "x_mse", "eps_mse", "logsnr"]}


@pytest.mark.parametrize("row", sorted(ROWS))
def test_what_training_losses_returns(calls, row):
    """hybrid: loss, vlb, var_frac; huber and the x-weightings: loss, x_mse; the v-loss rows: loss under autograd, and without it loss plus
    x_mse only when the caller chose a weighting other than 'snr_trunc'.  The v-loss rows under autograd hand the profile no x_mse."""
    for grad in (True, False):
        d = _diffusion(row, **({} if "teacher_mode" in ROWS[row] else {"loss_profile": 1}))
        net = Net(learn_var=row == "hybrid")
        del calls[:]
        with torch.set_grad_enabled(grad):
            out = d.training_losses(net=partial(net, guide=None), x=_x())
        want = TL_KEYS.get(row, {"loss"} if grad or row == "snr_trunc" else {"loss", "x_mse"})
        assert set(out) == want and all(v.shape == (B,) for v in out.values()), (row, grad)
        assert out["loss"].requires_grad == grad
        assert [name for name, _ in calls if name in N_OUT] == [LOSS_TABLE[row].op]
        noted = [a for name, a in calls if name == "loss_profile"]
        if d.loss_profile:
            assert len(noted) == 1 and (noted[0]["v1"] is None) == (grad and row in ("snr_trunc", "snr")) and not noted[0]["v0"].requires_grad


@pytest.mark.parametrize("row", sorted(ROWS))
def test_what_train_forward_backward_returns(calls, row):
    """hybrid: loss, x_mse, eps_mse, logsnr, vlb, var_frac; the v-loss rows: loss, x_mse, eps_mse, logsnr; the rest: loss, x_mse, logsnr; u when
    profiled; loss / loss_b / time_w under importance sampling.  The gradients go to backward_hip, dnu only from the hybrid row."""
    base = TFB_KEYS.get(row, ["loss", "x_mse", "logsnr"])
    modes = [({}, [])] if "teacher_mode" in ROWS[row] else [({}, []), ({"loss_profile": 1}, ["u"]), ({"time_importance": 1}, ["u", "loss_b", "time_w"])]
    for opts, extra in modes:
        d = _diffusion(row, **opts)
        net = Net(learn_var=row == "hybrid")
        del calls[:]
        out = d.train_forward_backward(net=partial(net, guide=None), x=_x(), grad_scale=0.25)
        assert list(out) == base + extra, (row, opts)
        (call,) = [a for name, a in calls if name in N_OUT]
        assert call["grad_scale"] == 0.25 and call["mean_type"] == "v"
        ((dv, dnu),) = net.backward_calls
        assert dv.shape == (B, 1, S, S) and (dnu is not None) == (row == "hybrid")
        assert sum(name == "scale_rows" for name, _ in calls) == (len(LOSS_TABLE[row].grads) if "time_w" in out else 0)
    with pytest.raises(ValueError, match="no variance head"):
        _diffusion("hybrid").train_forward_backward(net=partial(Net(), guide=None), x=_x(), grad_scale=0.25)
    with pytest.raises(ValueError, match="no variance head"):
        _diffusion("hybrid").training_losses(net=partial(Net(), guide=None), x=_x())


# ---- the draws ---------------------------------------------------------------------------------------------------------------------------------
def _draws(calls):
    return [(name, tuple(a["shape"]), a["offset"]) for name, a in calls if name in ("rng_normal", "rng_uniform")]


def test_every_entry_point_draws_eps_then_u(calls, monkeypatch):
    """`_prepare`, `training_losses`, `train_forward_backward` and the graphed train step: eps (B S S / 4 counters), then u (B / 4 counters, one
    under 'stratified'), then nothing else; what the caller passes in is not drawn, and the other draw keeps its place on the stream."""
    n_eps = B * S * S // 4
    want = [("rng_normal", (B, 1, S, S), 0), ("rng_uniform", (B,), n_eps)]
    net = partial(Net(learn_var=True), guide=None)
    entries = {
        "_prepare": lambda d, **kw: d._prepare(net, _x(), kw.get("u"), kw.get("eps")),
        "training_losses, learn_var": lambda d, **kw: d.training_losses(net=net, x=_x(), **kw),
        "train_forward_backward, learn_var": lambda d, **kw: d.train_forward_backward(net=net, x=_x(), grad_scale=0.25, **kw),
    }
    for what, run in entries.items():
        for opts in (dict(learn_var=1), dict(learn_var=1, loss_profile=1), dict(learn_var=1, time_sampler="stratified")):
            d = GaussianDiffusion(mean_type="v", num_steps=4, seed=5, **opts)
            del calls[:]
            run(d)
            one = opts.get("time_sampler") == "stratified"
            assert _draws(calls) == [want[0], ("rng_uniform", (1,) if one else (B,), n_eps)], (what, opts)
            assert d.rng.counter == n_eps + 1, (what, opts)
        d = GaussianDiffusion(mean_type="v", num_steps=4, seed=5, learn_var=1)
        del calls[:]
        run(d, u=torch.full((B,), 0.5))
        assert _draws(calls) == want[:1] and d.rng.counter == n_eps, what
        run(d, eps=torch.zeros(B, 1, S, S))
        assert _draws(calls)[1:] == [("rng_uniform", (B,), n_eps)] and d.rng.counter == n_eps + 1, what
    # a teacher's discrete times: eps, then i_times, then cond_w - no u
    d = _diffusion("huber")
    del calls[:]
    d._prepare(partial(Net(), guide=None), _x(), None, None)
    assert _draws(calls) == [want[0], ("rng_uniform", (B,), n_eps), ("rng_uniform", (B,), n_eps + 1)]
    # the graphed train step draws through the same function, outside its captured graph (here: a graph that is already captured)
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cpu", hidden_size=32, timesteps=4)
    model = Model(G)
    x, y = _x(), torch.zeros(B, dtype=torch.int64)
    static = (SimpleNamespace(replay=lambda: None), torch.zeros_like(x), y.clone(), torch.zeros_like(x), torch.zeros(B), torch.zeros(()))
    model.__dict__["_train_graphs"] = {(tuple(x.shape), y.dtype): static}
    monkeypatch.setattr(model.optimizer, "step", lambda **kw: None)
    monkeypatch.setattr(model, "_after_step", lambda: None)
    monkeypatch.setattr(model, "_step_metrics", lambda loss: {"loss": loss})
    monkeypatch.setattr(ops, "throttle", lambda: None)
    shared = []
    real = model.diffusion.draw_eps_u
    monkeypatch.setattr(model.diffusion, "draw_eps_u", lambda *a, **k: shared.append(1) or real(*a, **k))
    del calls[:]
    model._train_step_graphed(x, y)
    assert shared == [1] and _draws(calls) == want and model.diffusion.rng.counter == n_eps + 1
    assert torch.equal(static[3], torch.ones_like(x)) and torch.equal(static[4], torch.full((B,), 0.25))      # eps and u reached the static inputs


# ---- the bridge --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LOSS_TABLE))
def test_the_bridge_differentiates_the_rows_inputs_only(calls, name):
    """`_LossBridge`: the wrapper runs once with grad_scale 1, `loss` is the one differentiable output, and backward hands back the saved
    gradients with their rows scaled by g (fp32, contiguous) - to v, to nu on the hybrid row, None to everything else."""
    row = LOSS_TABLE[name]
    d = _diffusion(name)
    leaf = lambda: (_x() * 0.5).requires_grad_(True)
    v, nu, z, x, eps = leaf(), leaf() if row.nu else None, leaf(), leaf(), leaf()
    logsnr, u = torch.zeros(B, requires_grad=True), torch.full((B,), 0.5)
    out = d._loss(row, v, nu, z, x, eps, logsnr, u, 0, None)
    assert list(out) == [n for n in row.outs if n not in row.grads]
    assert [k for k, val in out.items() if val.requires_grad] == ["loss"]
    (call,) = [a for n, a in calls if n == row.op]
    assert call["grad_scale"] == 1.0
    g = torch.arange(1, B + 1, dtype=torch.float64)
    del calls[:]
    (out["loss"].double() * g).sum().backward()
    scaled = [a for n, a in calls if n == "scale_rows"]
    assert len(scaled) == len(row.grads) and all(a["rowscale"].dtype == torch.float32 and a["x"].shape == (B, S * S) for a in scaled)
    want = torch.ones_like(v) * g.float().view(B, 1, 1, 1)          # the stand-ins' gradients are ones
    assert torch.equal(v.grad, want) and (nu is None or torch.equal(nu.grad, want))
    assert z.grad is None and x.grad is None and eps.grad is None and logsnr.grad is None
    # and by the Function's own return: one entry per input, gradients exactly where v (and nu) stand
    ctx = SimpleNamespace(saved_tensors=tuple(torch.ones(B, 1, S, S) for _ in row.grads), constants=3 + row.eps + row.nu)
    ret = gd._LossBridge.backward(ctx, torch.ones(B))
    assert len(ret) == 2 + len(row.grads) + ctx.constants
    assert [r is not None for r in ret] == [False, False] + [True] * len(row.grads) + [False] * ctx.constants
