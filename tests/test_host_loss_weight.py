"""Host tests of the loss weightings and the stratified time rule (extensions; no GPU): the float64 restatement (tests/loss_weight_ref.py)
against its own finite differences and against the oracle's x_mse / eps_mse, the fp32 stratified rule, the option checks, the Philox
counter a stratified draw takes, the C entries' argument checks and the capacity constant."""
import ctypes
import math
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_weight_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inputs(mean_type, seed=0, n=96):
    lam = np.array(R.LAMBDAS)
    out, z, x, eps = R.loss_inputs(len(lam), n, lam, mean_type, seed)
    return lam, out.astype(np.float64), z.astype(np.float64), x.astype(np.float64), eps.astype(np.float64)


# ---- the restatement's gradient is the gradient of its loss ---------------------------------------------------------------------------------
@pytest.mark.parametrize("weight", R.WEIGHTS)
@pytest.mark.parametrize("mean_type", R.MEAN_TYPES)
def test_reference_gradient_is_a_finite_difference(mean_type, weight):
    """dv against a central difference of grad_scale sum_b loss_b, one image at each of the six log-SNRs, some elements clipped; only elements
    at least 1e-3 away from the clip are perturbed (the loss has a kink there).  The loss is quadratic in an unclipped element, so the central
    difference is exact up to rounding: h = 1e-4 of an element's reach in x_raw, tolerance 1e-6 of the image's largest |dv|."""
    lam, out, z, x, _ = _inputs(mean_type)
    gs, gamma = 0.37, 5.0
    ref = R.x_loss_w(out, z, x, lam, weight, gamma, grad_scale=gs, mean_type=mean_type)
    assert ref["clipped"].any() and not ref["clipped"].all()
    # grad_scale sum_b loss_b as a function of image b's output: the other images' terms do not move (and would drown the difference)
    total = lambda o, b: gs * R.x_loss_w(o[b:b + 1], z[b:b + 1], x[b:b + 1], lam[b:b + 1], weight, gamma, mean_type=mean_type)["loss_b"][0]
    _, dxo = R.x_raw(out, z, lam, mean_type)
    checked = 0
    for b in range(len(lam)):
        scale = np.abs(ref["dv"][b]).max()
        for i in range(0, out.shape[1], 5):
            if abs(abs(ref["x_raw"][b, i]) - 1.0) < 1e-3:
                continue
            h = 1e-4 / abs(dxo[b, i])                   # moves x_raw by 1e-4: stays on its side of the clip
            op, om = out.copy(), out.copy()
            op[b, i] += h; om[b, i] -= h
            fd = (total(op, b) - total(om, b)) / (2.0 * h)
            if ref["clipped"][b, i]:
                assert ref["dv"][b, i] == 0.0 and fd == 0.0
            else:
                assert abs(fd - ref["dv"][b, i]) <= 1e-6 * scale, (b, i, fd, ref["dv"][b, i])
            checked += 1
    assert checked > 60


# ---- identities against the oracle's two MSEs -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mean_type", R.MEAN_TYPES)
def test_reference_identities_against_the_oracle(mean_type):
    """With z = alpha x + sigma eps, eps_hat - eps = -e^(lambda / 2) (x_hat - x), so eps_mse = e^lambda x_mse and
      snr_plus1 = x_mse + eps_mse (checked for |lambda| <= 5, where neither term drowns the other),
      min_snr with gamma = 1e30 = eps_mse,  min_snr with gamma = 1 and lambda >= 0 = x_mse.
    x_mse and eps_mse from oracle.diffusion_ref.model_outputs in float64 (z formed in float64 here: the identity is about the exact z)."""
    from oracle import diffusion_ref as D
    lam, out, _, x, eps = _inputs(mean_type, seed=3)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    z = D.q_sample(T(x), T(lam), T(eps))
    # the perturbed output against the exact z: re-derive it so that some elements clip
    mo = D.model_outputs(T(out), z, T(lam), mean_type)
    x_mse = torch.square(mo["model_x"] - T(x)).mean(1).numpy()
    eps_mse = torch.square(mo["model_eps"] - T(eps)).mean(1).numpy()
    clipped = (mo["model_x"].abs() == 1.0).numpy()
    assert clipped.any() and not clipped.all()
    ref = lambda w, g: R.x_loss_w(out, z.numpy(), x, lam, w, g, mean_type=mean_type)
    np.testing.assert_allclose(ref("min_snr", 5.0)["x_mse"], x_mse, rtol=1e-12)
    mid = np.abs(lam) <= 5.0
    assert mid.sum() == 4
    np.testing.assert_allclose(ref("snr_plus1", 5.0)["loss_b"][mid], (x_mse + eps_mse)[mid], rtol=1e-9)
    np.testing.assert_allclose(ref("min_snr", 1e30)["loss_b"], eps_mse, rtol=1e-8)
    pos = lam >= 0.0
    np.testing.assert_allclose(ref("min_snr", 1.0)["loss_b"][pos], x_mse[pos], rtol=1e-12)
    # and the weights themselves at the six log-SNRs
    np.testing.assert_allclose(R.weight(lam, "min_snr", 5.0), [math.exp(-20), math.exp(-3), 1.0, 5.0, 5.0, 5.0], rtol=1e-12)
    np.testing.assert_allclose(R.weight(lam, "snr_plus1", 5.0), 1.0 + np.exp(lam), rtol=0)


# ---- the stratified rule -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 8, 256])
def test_stratified_rule_puts_one_time_in_every_interval(B):
    """Powers of two: b / B and the sums are exact in fp32, so every [k / B, (k + 1) / B) holds exactly one u and all lie in [0, 1)."""
    rng = np.random.default_rng(B)
    offsets = [np.float32(0.0), np.float32(1.0 - 2.0 ** -24)] + list(rng.random(16, dtype=np.float32))
    for u0 in offsets:
        u = R.u_stratified(u0, B)
        assert u.dtype == np.float32 and u.shape == (B,)
        assert (u >= 0).all() and (u < 1).all()
        cells = np.floor(u.astype(np.float64) * B).astype(np.int64)
        assert sorted(cells.tolist()) == list(range(B)), (float(u0), B)
    assert R.u_stratified(np.float32(0.0), B)[0] == 0.0
    assert R.u_stratified(np.float32(0.25), 8).tolist() == [0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 0.0, 0.125]


# ---- options ---------------------------------------------------------------------------------------------------------------------------------
def test_loss_weight_check_names_the_flag():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, loss_weight_check
    assert loss_weight_check("snr_trunc", 5.0, "uniform") == ("snr_trunc", 5.0, "uniform")
    assert loss_weight_check("min_snr", "2.5", "stratified") == ("min_snr", 2.5, "stratified")
    for name in ("snr", "snr_plus1"):
        assert loss_weight_check(name, 5, "uniform")[0] == name
    with pytest.raises(ValueError, match="loss_weight"):
        loss_weight_check("sigmoid", 5.0, "uniform")
    with pytest.raises(ValueError, match="time_sampler"):
        loss_weight_check("min_snr", 5.0, "importance")
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match="loss_gamma"):
            loss_weight_check("min_snr", bad, "uniform")
    # with a teacher only the defaults
    assert loss_weight_check("snr_trunc", 5.0, "uniform", has_teacher=True)[0] == "snr_trunc"
    for name in ("snr", "snr_plus1", "min_snr"):
        with pytest.raises(ValueError, match="loss_weight.*teacher"):
            loss_weight_check(name, 5.0, "uniform", has_teacher=True)
    with pytest.raises(ValueError, match="time_sampler.*teacher"):
        loss_weight_check("snr_trunc", 5.0, "stratified", has_teacher=True)
    # the constructor runs the same check
    teacher = object()
    with pytest.raises(ValueError, match="loss_weight"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="step1", loss_weight="min_snr")
    with pytest.raises(ValueError, match="time_sampler"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=teacher, teacher_mode="step2", time_sampler="stratified")
    with pytest.raises(ValueError, match="loss_gamma"):
        GaussianDiffusion(mean_type="v", num_steps=4, loss_weight="min_snr", loss_gamma=0)


def test_defaults_flags_and_weighting_in_use():
    from generative_models_amd import common, main
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    Model = common.discover_models()["diffusion_model"]
    assert (Model.DG.loss_weight, Model.DG.loss_gamma, Model.DG.time_sampler) == ("snr_trunc", 5.0, "uniform")
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    assert (d.loss_weight, d.loss_weight_type, d.loss_gamma, d.time_sampler) == ("snr_trunc", "snr_trunc", 5.0, "uniform")
    d = GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=object(), teacher_mode="step1")
    assert (d.loss_weight, d.loss_weight_type) == ("snr_trunc", "snr")           # distillation's own weighting, as before
    d = GaussianDiffusion(mean_type="v", num_steps=4, loss_weight="min_snr", loss_gamma=3, time_sampler="stratified")
    assert (d.loss_weight_type, d.loss_gamma, d.time_sampler) == ("min_snr", 3.0, "stratified")
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--loss_weight", "min_snr", "--loss_gamma", "4", "--time_sampler", "stratified"])
    assert (G.loss_weight, G.loss_gamma, G.time_sampler) == ("min_snr", 4.0, "stratified")
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert (G.loss_weight, G.loss_gamma, G.time_sampler) == ("snr_trunc", 5.0, "uniform")
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cpu", loss_weight="snr_plus1", time_sampler="stratified")
    m = Model(G)
    assert (m.diffusion.loss_weight_type, m.diffusion.time_sampler) == ("snr_plus1", "stratified")
    for key, bad in (("loss_weight", "sigmoid"), ("time_sampler", "importance"), ("loss_gamma", -2.0)):
        G = common.AttrDict(dict(Model.DG))
        G.update(lr=3e-4, pad32=0, device="cpu", **{key: bad})
        with pytest.raises(ValueError, match=key):
            Model(G)


def test_stratified_draw_takes_one_philox_counter(monkeypatch):
    """`draw_u`: 'stratified' reserves one Philox counter (one uniform) per batch, 'uniform' ceil(B / 4); eps first, then u, as before."""
    from generative_models_amd import ops
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, PhiloxStream
    calls = []
    monkeypatch.setattr(ops, "rng_uniform", lambda shape, seed, off, dev: calls.append(("uniform", tuple(shape), off)) or torch.zeros(shape))
    monkeypatch.setattr(ops, "rng_normal", lambda shape, seed, off, dev: calls.append(("normal", tuple(shape), off)) or torch.zeros(shape))
    monkeypatch.setattr(ops, "u_stratified", lambda u0, B: calls.append(("expand", tuple(u0.shape), B)) or torch.zeros(B))
    s = PhiloxStream(3)
    s.uniform((1,), "cpu")
    assert s.counter == 1
    d = GaussianDiffusion(mean_type="v", num_steps=4, time_sampler="stratified", seed=5)
    for k in range(3):
        assert d.draw_u(8, "cpu").shape == (8,)
        assert d.rng.counter == k + 1
    assert calls[-2:] == [("uniform", (1,), 2), ("expand", (1,), 8)]
    d.rng.normal((8, 1, 8, 8), "cpu")                    # a step's draws: eps (128 counters), then u (one)
    d.draw_u(8, "cpu")
    assert d.rng.counter == 3 + 128 + 1
    d = GaussianDiffusion(mean_type="v", num_steps=4, seed=5)
    del calls[:]
    d.draw_u(10, "cpu")
    assert d.rng.counter == 3 and calls == [("uniform", (10,), 0)]


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    ret, argtypes, argnames = protos["gmk_x_loss_w"]
    assert argnames == ["v", "z", "x", "logsnr", "loss_b", "x_mse", "dv", "grad_scale", "weight_type", "gamma", "mean_type", "B", "n", "stream"]
    assert argtypes == [P] * 7 + [F, I, F, I, I, L, P] and ret is ctypes.c_int
    assert protos["gmk_u_stratified"] == (ctypes.c_int, [P, P, I, P], ["u0", "u", "B", "stream"])
    assert _lib.PROTOS["gmk_x_loss_w"] == protos["gmk_x_loss_w"]
    # gmk_v_loss as it was
    assert protos["gmk_v_loss"][2] == ["v", "z", "x", "eps", "logsnr", "loss_b", "x_mse", "eps_mse", "dv", "grad_scale", "loss_type", "mean_type",
                                       "B", "n", "stream"]
    text = open(os.path.join(ROOT, "include", "gmk.h")).read()
    assert "Hang et al. 2023" in text and "Salimans & Ho 2022" in text and "Kingma et al. 2021" in text


def test_entries_reject_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first

    def call(v=buf, z=buf, x=buf, l=buf, loss=buf, xm=buf, dv=None, wt=1, gamma=5.0, mt=0, B=2, n=64):
        return lib.gmk_x_loss_w(v, z, x, l, loss, xm, dv, 1.0, wt, gamma, mt, B, n, None)
    for kw in ({"v": None}, {"z": None}, {"x": None}, {"l": None}, {"loss": None}, {"xm": None}):
        assert call(**kw) == -1 and b"gmk_x_loss_w: null pointer" in lib.gmk_last_error()
    for wt in (-1, 2):
        assert call(wt=wt) == -1 and b"gmk_x_loss_w: weight_type" in lib.gmk_last_error()
    for gamma in (0.0, -1.0, float("nan"), float("inf")):
        for wt in (0, 1):
            assert call(gamma=gamma, wt=wt) == -1 and b"gmk_x_loss_w: gamma" in lib.gmk_last_error()
    for mt in (-1, 3):
        assert call(mt=mt) == -1 and b"gmk_x_loss_w: mean_type" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"n": 0}):
        assert call(**kw) == -1 and b"gmk_x_loss_w: bad shape" in lib.gmk_last_error()
    for kw in ({"u0": None}, {"u": None}):
        a = {"u0": buf, "u": buf, **kw}
        assert lib.gmk_u_stratified(a["u0"], a["u"], 8, None) == -1 and b"gmk_u_stratified: null pointer" in lib.gmk_last_error()
    for B in (0, -3, (1 << 24) + 1):
        assert lib.gmk_u_stratified(buf, buf, B, None) == -1 and b"gmk_u_stratified: B" in lib.gmk_last_error()


def test_constants_match_the_kernel_and_wrappers_check_first():
    from generative_models_amd import ops
    src = open(os.path.join(ROOT, "generative_models_amd", "csrc", "diffusion_ew.hip")).read()
    hdr = open(os.path.join(ROOT, "include", "gmk.h")).read()
    m = re.search(r"#define GMK_X_LOSS_KEEP (\d+)\b", hdr)      # the kernel's constant is the header's
    assert "constexpr int kXLossKeep = GMK_X_LOSS_KEEP;" in src and m and int(m.group(1)) == ops.X_LOSS_KEEP == ops.DYN_THRESHOLD_KEYS and ops.X_LOSS_KEEP % 256 == 0
    for name, code in ops.X_LOSS_WEIGHTS.items():
        assert re.search(rf"#define GMK_LOSS_W_{name.upper()} {code}\b", hdr)
    t = torch.zeros(2, 8)
    with pytest.raises(ValueError, match="weight"):
        ops.x_loss_w(t, t, t, t[:, 0], "snr_trunc", 5.0)
    with pytest.raises(ValueError, match="gamma"):
        ops.x_loss_w(t, t, t, t[:, 0], "min_snr", float("nan"))
    with pytest.raises(ValueError, match="device"):
        ops.x_loss_w(t, t, t, t[:, 0].contiguous(), "min_snr", 5.0)
