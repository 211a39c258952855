"""Host tests (no GPU) of consistency distillation and the multistep consistency sampler (extensions; Song et al. 2023): the flags and their
refusals, the C prototypes, the sampler's plan, and the float64 restatement (tests/consistency_ref.py) against autograd and its own limits."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import consistency_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_flags(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cpu", hidden_size=32, **flags)
    return Model, G


# ---- flags ---------------------------------------------------------------------------------------------------------------------------------------
def test_defaults_and_types_of_the_flags():
    from generative_models_amd import main
    Model, _ = _model_flags()
    DG = Model.DG
    assert (DG.consistency_grid, DG.consistency_loss, DG.consistency_huber_c) == (0, "l2", 0.00054)
    assert type(DG.consistency_grid) is int and type(DG.consistency_loss) is str and type(DG.consistency_huber_c) is float
    assert (DG.teacher_mode, DG.sampler) == ("step1", "ddim")                      # the reference's defaults, untouched
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert (G.consistency_grid, G.consistency_loss, G.consistency_huber_c, G.teacher_mode, G.sampler) == (0, "l2", 0.00054, "step1", "ddim")
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--teacher_mode", "consistency", "--consistency_grid", "256", "--consistency_loss",
                                            "huber", "--consistency_huber_c", "0.001", "--sampler", "consistency", "--timesteps", "2"])
    assert (G.consistency_grid, G.consistency_loss, G.consistency_huber_c) == (256, "huber", 0.001)
    assert (G.teacher_mode, G.sampler, G.timesteps) == ("consistency", "consistency", 2)


def test_gaussian_diffusion_takes_the_mode():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    teacher, target = object(), object()
    d = GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="consistency")
    assert d.consistency and d.teacher_mode == "consistency" and d.target_net is None and d.train_grid == 4
    assert (d.consistency_loss, d.consistency_huber_c, d.loss_weight, d.loss_weight_type) == ("l2", 0.00054, "snr_trunc", "snr_trunc")
    d = GaussianDiffusion(mean_type="v", num_steps=2, teacher_net=teacher, teacher_mode="consistency", target_net=target, consistency_grid=256,
                          consistency_loss="huber", consistency_huber_c="0.002", sampler="consistency")
    assert d.target_net is target and d.train_grid == 256 and d.num_steps == 2 and d.loss_weight_type == "huber" and d.consistency_huber_c == 0.002
    # the other modes are as they were, and never hold a target net
    d = GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="step2", target_net=target)
    assert not d.consistency and d.target_net is None and d.train_grid == 4 and d.loss_weight_type == "snr_trunc"
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    assert not d.consistency and d.target_net is None


def test_refusals_name_the_flags():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, consistency_check
    assert consistency_check("consistency", True, 8, "huber", 0.001) == (True, 8, "huber", 0.001)
    assert consistency_check("step1", False) == (False, 0, "l2", 0.00054)
    teacher = object()
    with pytest.raises(ValueError, match="teacher_mode.*teacher_path"):
        consistency_check("consistency", False)
    with pytest.raises(ValueError, match="teacher_mode.*teacher_path"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_mode="consistency")
    for mode, has in (("step1", True), ("step2", True), ("step1", False)):
        with pytest.raises(ValueError, match="consistency_loss.*teacher_mode"):
            consistency_check(mode, has, 0, "huber")
        with pytest.raises(ValueError, match="consistency_grid.*teacher_mode"):
            consistency_check(mode, has, 16)
    with pytest.raises(ValueError, match="consistency_loss"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="step2", consistency_loss="huber")
    with pytest.raises(ValueError, match="consistency_grid"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="step1", consistency_grid=8)
    for bad in (-1, -256, 1.5, "many", None, True):
        with pytest.raises(ValueError, match="consistency_grid"):
            consistency_check("consistency", True, bad)
    with pytest.raises(ValueError, match="consistency_loss"):
        consistency_check("consistency", True, 0, "lpips")
    for bad in (0.0, -1.0, float("nan"), float("inf"), "c", None, True):
        with pytest.raises(ValueError, match="consistency_huber_c"):
            consistency_check("consistency", True, 0, "huber", bad)
    # what a teacher refuses stays refused
    with pytest.raises(ValueError, match="loss_weight.*teacher"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="consistency", loss_weight="min_snr")
    with pytest.raises(ValueError, match="time_sampler.*teacher"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="consistency", time_sampler="stratified")
    for flag in ("time_importance", "loss_profile"):
        with pytest.raises(ValueError, match=f"{flag}.*teacher"):
            GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="consistency", **{flag: 1})


def test_model_refuses_at_construction():
    for flags, match in ((dict(teacher_mode="consistency"), "teacher_mode.*teacher_path"),
                         (dict(consistency_loss="huber"), "consistency_loss"),
                         (dict(consistency_grid=8), "consistency_grid"),
                         (dict(teacher_mode="step2", consistency_grid=-2), "consistency_grid"),
                         (dict(sampler="consistency", dyn_threshold=0.995), "consistency.*dyn_threshold"),
                         (dict(sampler="consistency", inpaint_eval=1), "consistency.*inpaint_eval"),
                         (dict(sampler="consistency", restore_eval=2), "consistency.*restore_eval")):
        Model, G = _model_flags(**flags)
        with pytest.raises(ValueError, match=match):
            Model(G)
    Model, G = _model_flags(sampler="consistency", timesteps=2)
    assert Model(G).diffusion.sampler == "consistency"


def test_model_hands_the_weight_average_over_as_target(tmp_path):
    Model, G = _model_flags()
    torch.save(Model(G).state_dict(), tmp_path / "model.pt")
    Model, G = _model_flags(teacher_path=tmp_path / "model.pt", teacher_mode="consistency", ema_decay=0.95, consistency_grid=8, timesteps=2,
                            sampler="consistency")
    m = Model(G)
    assert m.diffusion.target_net is m.ema_net and m.ema_net is not None and m.diffusion.train_grid == 8 and m.diffusion.num_steps == 2
    assert not m.optimizer.ema_seeded
    m.net.flat_params.add_(0.25)                       # what a later weights_from load or broadcast would do
    m._seed_target()
    assert m.optimizer.ema_seeded and torch.equal(m.ema_net.flat_params, m.net.flat_params)
    Model, G = _model_flags(teacher_path=tmp_path / "model.pt", teacher_mode="consistency")
    m = Model(G)
    assert m.diffusion.target_net is None and m.ema_net is None
    m._seed_target()                                   # nothing to seed: the student is its own target
    Model, G = _model_flags(teacher_path=tmp_path / "model.pt", teacher_mode="step2", ema_decay=0.95)
    m = Model(G)
    assert m.diffusion.target_net is None
    m._seed_target()
    assert not m.optimizer.ema_seeded                  # the other modes seed at the first optimiser step, as before


# ---- the C surface and the plan ---------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L, U = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    assert protos["gmk_consistency_target"] == (I, [P] * 9 + [I, I, L, P], [
        "v_tgt", "z_s", "x_pred_teacher", "z_t", "logsnr_t", "logsnr_s", "i_times", "x_target", "eps_target", "mean_type", "B", "n", "stream"])
    assert protos["gmk_x_loss_huber"] == (I, [P] * 7 + [F, F, I, I, L, P], [
        "v", "z", "x", "logsnr", "loss_b", "x_mse", "dv", "grad_scale", "c", "mean_type", "B", "n", "stream"])
    assert protos["gmk_consistency_step"] == (I, [P] * 4 + [F, F, I, U, U, U] + [P] * 5 + [I, I, L, P], [
        "v", "v_uncond", "cond_w", "z", "logsnr_t", "logsnr_s", "is_last", "seed", "offset", "q0", "z_next", "x_pred", "eps_pred", "z_dup",
        "logsnr_next", "mean_type", "B", "n", "stream"])
    for name in ("gmk_consistency_target", "gmk_x_loss_huber", "gmk_consistency_step"):
        assert _lib.PROTOS[name] == protos[name]
    text = open(os.path.join(ROOT, "include", "gmk.h")).read()
    assert "Consistency Models" in text and "Improved Techniques for Training Consistency Models" in text
    assert _lib.lib.gmk_version() == 1
    assert not any("consistency" in name.lower() or "huber" in name.lower() for _, _, name in _lib.parse_kernel_table())      # no profile label


def test_entries_reject_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first

    def target(mt=0, B=2, n=64, **null):
        a = {k: buf for k in ("v", "zs", "xp", "zt", "lt", "ls", "it", "xt", "et")}
        a.update(null)
        return lib.gmk_consistency_target(a["v"], a["zs"], a["xp"], a["zt"], a["lt"], a["ls"], a["it"], a["xt"], a["et"], mt, B, n, None)
    for k in ("v", "zs", "xp", "zt", "lt", "ls", "it", "xt", "et"):
        assert target(**{k: None}) == -1 and b"gmk_consistency_target: null pointer" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"n": 0}, {"B": 65536}):
        assert target(**kw) == -1 and b"gmk_consistency_target: bad shape" in lib.gmk_last_error()
    for mt in (-1, 3):
        assert target(mt=mt) == -1 and b"gmk_consistency_target: mean_type" in lib.gmk_last_error()

    def huber(v=buf, z=buf, x=buf, l=buf, loss=buf, xm=buf, c=0.00054, mt=0, B=2, n=64):
        return lib.gmk_x_loss_huber(v, z, x, l, loss, xm, None, 1.0, c, mt, B, n, None)
    for kw in ({"v": None}, {"z": None}, {"x": None}, {"l": None}, {"loss": None}, {"xm": None}):
        assert huber(**kw) == -1 and b"gmk_x_loss_huber: null pointer" in lib.gmk_last_error()
    for c in (0.0, -1.0, float("nan"), float("inf")):
        assert huber(c=c) == -1 and b"gmk_x_loss_huber: c" in lib.gmk_last_error()
    for mt in (-1, 3):
        assert huber(mt=mt) == -1 and b"gmk_x_loss_huber: mean_type" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"n": 0}):
        assert huber(**kw) == -1 and b"gmk_x_loss_huber: bad shape" in lib.gmk_last_error()

    def step(v=buf, vu=None, w=None, z=buf, lt=1.0, ls=2.0, zn=buf, mt=0, B=2, n=64):
        return lib.gmk_consistency_step(v, vu, w, z, lt, ls, 0, 1, 0, 0, zn, None, None, None, None, mt, B, n, None)
    for kw in ({"v": None}, {"z": None}, {"zn": None}):
        assert step(**kw) == -1 and b"gmk_consistency_step: null pointer" in lib.gmk_last_error()
    assert step(vu=buf) == -1 and b"go together" in lib.gmk_last_error()
    assert step(n=66) == -1 and b"gmk_consistency_step: n = 66" in lib.gmk_last_error()
    for kw in ({"lt": float("nan")}, {"ls": float("inf")}):
        assert step(**kw) == -1 and b"gmk_consistency_step: non-finite time" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"B": 65536}, {"mt": 3}):
        assert step(**kw) == -1 and b"gmk_consistency_step" in lib.gmk_last_error()


def test_wrappers_check_before_asking_for_a_device():
    from generative_models_amd import ops
    t, l, i = torch.zeros(2, 8), torch.zeros(2), torch.zeros(2, dtype=torch.int64)
    with pytest.raises(ValueError, match="mean_type"):
        ops.consistency_target(t, t, t, t, l, l, i, mean_type="both")
    with pytest.raises(ValueError, match="v_tgt: shape"):
        ops.consistency_target(t[:, :4], t, t, t, l, l, i)
    with pytest.raises(ValueError, match="device"):
        ops.consistency_target(t, t, t, t, l, l, i)
    with pytest.raises(ValueError, match="c = "):
        ops.x_loss_huber(t, t, t, l, float("nan"))
    with pytest.raises(ValueError, match="c = "):
        ops.x_loss_huber(t, t, t, l, 0.0)
    with pytest.raises(ValueError, match="logsnr: shape"):
        ops.x_loss_huber(t, t, t, torch.zeros(3), 0.001)
    with pytest.raises(ValueError, match="device"):
        ops.x_loss_huber(t, t, t, l, 0.001)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.consistency_step(torch.zeros(2, 6), torch.zeros(2, 6), 0.0, 1.0, False, 0, 0)
    with pytest.raises(ValueError, match="unsigned 64-bit"):
        ops.consistency_step(t, t, 0.0, 1.0, False, -1, 0)
    with pytest.raises(ValueError, match="q0"):
        ops.consistency_step(t, t, 0.0, 1.0, False, 0, 0, q0=-4)
    with pytest.raises(ValueError, match="non-finite"):
        ops.consistency_step(t, t, float("nan"), 1.0, False, 0, 0)
    with pytest.raises(ValueError, match="go together"):
        ops.consistency_step(t, t, 0.0, 1.0, False, 0, 0, v_uncond=t)
    with pytest.raises(ValueError, match="device"):
        ops.consistency_step(t, t, 0.0, 1.0, False, 0, 0)


def test_sampler_plan_rows():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, sampler_grid, sampler_plan
    plan = sampler_plan(3, "consistency")
    assert plan == sampler_plan(3, "ddim")
    assert [(s.i, s.is_last, s.passes, s.dpm, s.inp) for s in plan] == [(2, False, 1, None, None), (1, False, 1, None, None), (0, True, 1, None, None)]
    assert [(s.i, s.lt, s.ls) for s in plan] == sampler_grid(3)
    assert abs(float(plan[0].lt) + 20.0) < 2e-3 and abs(float(plan[-1].ls) - 20.0) < 1e-4 and all(a.ls == b.lt for a, b in zip(plan, plan[1:]))
    assert [s.i for s in sampler_plan(3, "consistency", start=2)] == [1, 0]
    # the loop knows the name; an unknown one stays unknown
    d = GaussianDiffusion(mean_type="v", num_steps=3, sampler="dpmpp_3m")
    with pytest.raises(NotImplementedError):
        d.sample(net=lambda *a, **k: None, init_x=torch.zeros(2, 1, 4, 4))


def test_sampler_refuses_the_three_combinations_and_injected_noise():
    """Before anything touches a device: inpainting, restoration, dynamic thresholding, injected noise, n % 4 != 0."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net = lambda *a, **k: None
    z = torch.zeros(2, 1, 4, 4)
    d = GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency")
    with pytest.raises(ValueError, match="consistency.*inpainting"):
        d.inpaint(net=net, x0=z, mask=torch.ones(1, 1, 4, 4), init_x=z)
    with pytest.raises(ValueError, match="consistency.*restoration"):
        d.restore(net=net, obs=torch.zeros(2, 1, 2, 2), factor=2, init_x=z)
    with pytest.raises(ValueError, match="consistency.*dyn_threshold"):
        GaussianDiffusion(mean_type="v", num_steps=3, sampler="consistency", dyn_threshold=0.99).sample(net=net, init_x=z)
    with pytest.raises(ValueError, match="noises"):
        d.sample(net=net, init_x=z, noises=torch.zeros(3, 2, 1, 4, 4))
    with pytest.raises(ValueError, match="multiple of 4"):
        d.sample(net=net, init_x=torch.zeros(2, 1, 3, 3))


# ---- the restatement ----------------------------------------------------------------------------------------------------------------------------
LAM = np.linspace(-15.0, 15.0, 5)


@pytest.mark.parametrize("mt", R.MEAN_TYPES)
def test_huber_gradient_is_autograds(mt):
    B, n, c, gs = 5, 48, 0.00054, 0.37
    out, z, x, _ = R.loss_inputs(B, n, LAM, mt, seed=11)
    ref = R.x_loss_huber(out, z, x, LAM, c, grad_scale=gs, mean_type=mt)
    o = torch.tensor(out, dtype=torch.float64, requires_grad=True)
    zz, xx, l = torch.tensor(z, dtype=torch.float64), torch.tensor(x, dtype=torch.float64), torch.tensor(LAM)[:, None]
    alpha, sigma = torch.sqrt(torch.sigmoid(l)), torch.sqrt(torch.sigmoid(-l))
    raw = {"v": alpha * zz - sigma * o, "eps": (zz - sigma * o) / alpha, "x": o}[mt]
    m = (torch.clip(raw, -1.0, 1.0) - xx).square().mean(1)
    loss = torch.sqrt(m + c * c) - c
    (gs * loss.sum()).backward()
    assert np.allclose(ref["loss_b"], loss.detach().numpy(), rtol=1e-12, atol=0) and np.allclose(ref["x_mse"], m.detach().numpy(), rtol=1e-12, atol=0)
    g = o.grad.numpy()
    assert np.abs(ref["dv"] - g).max() <= 1e-12 * np.abs(g).max()
    assert (ref["dv"][ref["clipped"]] == 0.0).all() and 0 < ref["clipped"].sum()
    if mt != "eps":                                     # ('eps' at logsnr -15: loss_inputs clips every element of that image)
        assert ref["clipped"].sum() < ref["clipped"].size


def test_huber_tends_to_the_scaled_l2():
    """sqrt(m + c^2) - c = m / 2c - m^2 / 8c^3 + ...: the relative distance to m / 2c is at most m / 4c^2, the series' next term."""
    for m in (1e-6, 0.01, 0.3, 4.0):
        for k in (10.0, 1e3, 1e5):                      # c^2 = k m; the 1e-9 covers float64's rounding of c^2 + m (1.1e-16 k, relative to m)
            c = float(np.sqrt(k * m))
            want = m / (2.0 * c)
            rel = abs(R.huber(m, c) - want) / want
            assert rel <= m / (4.0 * c * c) + 1e-9, (m, c, rel)
            assert rel >= 0.5 * m / (4.0 * c * c), (m, c, rel)        # and it is that term, not something smaller by luck
    assert R.huber(0.0, 0.00054) == 0.0
    # and for m >> c^2 it is the root of the mean square, less c
    assert abs(R.huber(4.0, 0.00054) - (2.0 - 0.00054)) < 1e-7


@pytest.mark.parametrize("mt", R.MEAN_TYPES)
def test_target_rows_at_the_boundary_return_the_teachers_prediction(mt):
    B, n = 5, 24
    lt, ls = LAM, LAM + 0.7
    v, z_s, xp, z_t = R.target_inputs(B, n, lt, ls, seed=3)
    i = np.array([0, 3, 0, 1, 7])
    xs, es = R.consistency_target(v, z_s, xp, z_t, lt, ls, i, mt)
    assert np.array_equal(xs[i == 0], xp[i == 0].astype(np.float64))
    assert np.array_equal(xs[i != 0], R.x_hat(v, z_s, ls, mt)[i != 0]) and np.abs(xs).max() <= 1.0
    alpha, sigma = R.alpha_sigma(lt, 2)
    assert np.allclose(alpha * xs + sigma * es, z_t, rtol=0, atol=1e-12)         # eps* is the noise that carries x* to z_t
    # the i == 0 rows do not depend on the target net's output at all
    xs2, es2 = R.consistency_target(v + 1.0, z_s - 1.0, xp, z_t, lt, ls, i, mt)
    assert np.array_equal(xs2[i == 0], xs[i == 0]) and np.array_equal(es2[i == 0], es[i == 0])


def test_step_restated():
    x, e = np.array([[0.5, -1.0]]), np.array([[2.0, 0.25]])
    assert np.array_equal(R.consistency_step(x, e, 3.0, True), x)
    a, s = (float(t[0]) for t in R.alpha_sigma(3.0, 1))
    assert np.allclose(R.consistency_step(x, e, 3.0, False), a * x + s * e, rtol=1e-15) and abs(a * a + s * s - 1.0) < 1e-15
