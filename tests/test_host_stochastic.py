"""Host tests (no GPU) of the stochastic samplers ('ancestral' with the reference's three posterior variances, 'ddim' with ddim_eta > 0,
'sde_dpmpp_2m'): `stochastic_coefs` against the reference's own float64 posterior (tests/golden/posterior_var.npz, written by
tools/make_posterior_golden.py) and against the identities that tie the three families together, the plan, the options and their refusals,
the C prototype and its argument checks."""
import ctypes
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import stochastic_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = (1, 2, 3, 4, 8, 20, 250)
X_LOGVARS = ("small", "large", "medium:0.25", "medium:0.5", "medium:0.75")


def rel(a, b):
    """Largest |a - b| / |b| over two arrays; entries where both are exactly 0 count as 0."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where((a == 0) & (b == 0), 0.0, np.abs(a - b) / np.abs(b))
    return float(q.max())


@pytest.fixture(scope="module")
def golden():
    g = np.load(os.path.join(ROOT, "tests", "golden", "posterior_var.npz"))
    assert tuple(int(t) for t in g["steps"]) == STEPS and tuple(str(c) for c in g["x_logvars"]) == X_LOGVARS
    return g


def _key(T, case):
    return f"T{T}_" + case.replace(":", "_").replace(".", "p")


# ---- coefficients against the reference ------------------------------------------------------------------------------------------------------
def test_ancestral_coefficients_match_the_references_float64_posterior(golden):
    """The reference's diffusion_reverse, run in float64 on its own fp32 grid log-SNRs: mean at (z, x) = (1, 0) is coef_z, at (0, 1) coef_x,
    std is coef_noise; 1e-13 relative (measured: 6.9e-16 for the means and the 'small' / 'large' std, 1.2e-15 for 'medium').

    Two things the fixture shows.  (a) The host's grid (numpy) and the reference's (torch) differ by an fp32 ulp at some points for T >= 8, so
    the closed forms are compared AT the fixture's log-SNRs (`stochastic_row`, the function every row of `stochastic_coefs` comes from), and
    `stochastic_coefs` itself wherever the two grids agree bit for bit, which includes every T <= 4.  (b) The reference's 'medium:<frac>' std
    is NaN at every step: it is exp(logvar) and its logvar goes through log1mexp with a positive argument (diffusion_utils.py:40).  Their
    yardstick is the formula those lines state, var = var_large^frac var_small^(1 - frac), formed from the fixture's own finite 'large' and
    'small' std in float64 (two pow and a product on values in [1e-5, 1]: under 1e-15 relative)."""
    from generative_models_amd.diffusion.gaussian_diffusion import posterior_var_frac, sampler_grid, stochastic_coefs, stochastic_row
    worst, direct = 0.0, 0
    for T in STEPS:
        pairs = golden[f"T{T}_logsnr"]
        assert pairs.dtype == np.float32 and pairs.shape == (T, 2)
        ours_grid = np.array([(lt, ls) for _, lt, ls in sampler_grid(T)], dtype=np.float32)
        assert np.abs(ours_grid.astype(np.float64) - pairs).max() <= 4e-6           # the same grid to a few fp32 ulps
        same = (ours_grid.view(np.uint32) == pairs.view(np.uint32)).all(1)
        assert T > 4 or same.all()
        small, large = golden[_key(T, "small")], golden[_key(T, "large")]
        for case in X_LOGVARS:
            ref = golden[_key(T, case)].copy()
            assert ref.dtype == np.float64 and ref.shape == (T, 3) and np.isfinite(ref[:, :2]).all()
            f = posterior_var_frac(case)
            if case.startswith("medium:"):
                want = large[:, 2] ** f * small[:, 2] ** (1.0 - f)
                ref[:, 2] = np.where(np.isfinite(ref[:, 2]), ref[:, 2], want)
                assert rel(ref[:, 2], want) <= 1e-13
            assert np.isfinite(ref).all()
            at_ref = np.array([stochastic_row("ancestral", lt, ls, f) for lt, ls in pairs])
            worst = max(worst, rel(at_ref, ref))
            assert rel(at_ref, ref) <= 1e-13, (T, case, rel(at_ref, ref))
            rows = stochastic_coefs(T, "ancestral", case)
            assert [r.i for r in rows] == list(range(T))[::-1] and all(r.coef_prev == 0.0 for r in rows)
            mine = np.array([(r.coef_z, r.coef_x, r.coef_noise) for r in rows])
            assert rel(mine[same], ref[same]) <= 1e-13, (T, case)
            direct += int(same.sum())
            # and every row is the closed form at the host grid's own log-SNRs
            assert all((r.coef_z, r.coef_x, r.coef_noise) == stochastic_row("ancestral", r.lt, r.ls, f) for r in rows)
            assert [(r.lt, r.ls) for r in rows] == [(float(lt), float(ls)) for _, lt, ls in sampler_grid(T)]
    print(f"largest relative distance to the reference's float64 posterior: {worst:.2e}; {direct} rows compared through stochastic_coefs itself")
    assert direct >= 5 * (1 + 2 + 3 + 4)


@pytest.mark.parametrize("T", STEPS)
def test_coefficients_match_the_restatement(T):
    from generative_models_amd.diffusion.gaussian_diffusion import sampler_grid, stochastic_coefs
    grid = sampler_grid(T)
    for kind, pv, eta in [("ancestral", c, 0.0) for c in X_LOGVARS] + [("ddim_eta", "large", e) for e in (0.3, 1.0)] + [("sde_dpmpp_2m", "large", 0.0)]:
        rows = stochastic_coefs(T, kind, pv, eta)
        ks = R.second_order_k(grid) if kind == "sde_dpmpp_2m" else [0.0] * T
        for row, (i, lt, ls), k in zip(rows, grid, ks):
            want = R.coefs(kind, lt, ls, R.frac_of(pv), eta)
            assert rel(row[3:6], want) <= 1e-12, (kind, pv, eta, i)
            assert (row.i, row.lt, row.ls) == (i, float(lt), float(ls)) and rel([row.coef_prev], [k]) <= 1e-12


# ---- identities: 1e-12 relative (measured at or below 8e-16) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", STEPS)
def test_identities_between_the_families(T):
    from generative_models_amd.diffusion.gaussian_diffusion import stochastic_coefs
    cut = lambda rows: np.array([r[3:6] for r in rows])
    small = stochastic_coefs(T, "ancestral", "small")
    assert rel(cut(stochastic_coefs(T, "ddim_eta", ddim_eta=1.0)), cut(small)) <= 1e-12        # eta = 1 is the ancestral sampler, 'small'
    assert rel(cut(stochastic_coefs(T, "sde_dpmpp_2m")), cut(small)) <= 1e-12                  # and so is the first-order SDE solver
    for row in stochastic_coefs(T, "ddim_eta", ddim_eta=1e-200):                               # eta -> 0: DDIM's deterministic update
        (a_t, s_t), (a_s, s_s) = R.alpha_sigma(row.lt), R.alpha_sigma(row.ls)
        assert rel([row.coef_z, row.coef_x], [s_s / s_t, a_s - a_t * (s_s / s_t)]) <= 1e-12 and 0.0 <= row.coef_noise <= 1e-199
    for row in stochastic_coefs(T, "ddim_eta", ddim_eta=0.0):
        (a_t, s_t), (a_s, s_s) = R.alpha_sigma(row.lt), R.alpha_sigma(row.ls)
        assert rel([row.coef_z, row.coef_x], [s_s / s_t, a_s - a_t * (s_s / s_t)]) <= 1e-12 and row.coef_noise == 0.0
    for eta in (0.3, 1.0):                                                                      # the marginal N(alpha_s x, sigma_s^2) is preserved
        for row in stochastic_coefs(T, "ddim_eta", ddim_eta=eta):
            (a_t, s_t), (a_s, s_s) = R.alpha_sigma(row.lt), R.alpha_sigma(row.ls)
            assert rel([row.coef_z * a_t + row.coef_x], [a_s]) <= 1e-12
            assert rel([row.coef_z ** 2 * s_t ** 2 + row.coef_noise ** 2], [s_s ** 2]) <= 1e-12
    for row in stochastic_coefs(T, "ancestral", "large"):                                       # the kernel's `stdv` of the 'noisy' sampler
        omr = -math.expm1(row.lt - row.ls)
        assert rel([row.coef_noise], [math.sqrt(omr / (1.0 + math.exp(row.lt)))]) <= 1e-12
    for case in X_LOGVARS[2:]:                                                                  # 'medium' lies between the two, in order
        f = float(case.split(":")[1])
        m, lg = stochastic_coefs(T, "ancestral", case), stochastic_coefs(T, "ancestral", "large")
        assert all(s.coef_noise < x.coef_noise < l.coef_noise for s, x, l in zip(small, m, lg))
        assert rel([x.coef_noise for x in m], [l.coef_noise ** f * s.coef_noise ** (1 - f) for s, l in zip(small, lg)]) <= 1e-12


def test_eta_one_on_the_one_step_grid_keeps_its_digits():
    """The form sqrt(1 - eta^2 omr) is 0 there (omr rounds to 1); the one in use gives r's own root."""
    from generative_models_amd.diffusion.gaussian_diffusion import stochastic_coefs
    (row,) = stochastic_coefs(1, "ddim_eta", ddim_eta=1.0)
    assert -math.expm1(row.lt - row.ls) == 1.0 and row.coef_z > 0.0
    s_t, s_s = R.alpha_sigma(row.lt)[1], R.alpha_sigma(row.ls)[1]
    assert rel([row.coef_z], [s_s / s_t * math.exp(0.5 * (row.lt - row.ls))]) <= 1e-12


def test_zero_length_step_is_the_identity():
    from generative_models_amd.diffusion.gaussian_diffusion import stochastic_row
    for kind in R.KINDS:
        for l in (-20.0, 0.0, 3.5):
            assert stochastic_row(kind, l, l, 0.5, 0.7) == (1.0, 0.0, 0.0)
            assert R.coefs(kind, l, l, 0.5, 0.7) == (1.0, 0.0, 0.0)
    # the nearest fp32 neighbours: finite, a tiny noise share, no log(0)
    lt = np.float32(3.5)
    ls = np.nextafter(lt, np.float32(4.0))
    for kind in R.KINDS:
        c_z, c_x, c_n = stochastic_row(kind, lt, ls, 0.5, 0.7)
        assert all(math.isfinite(c) for c in (c_z, c_x, c_n)) and abs(c_z - 1.0) < 1e-6 and 0.0 < c_x < 1e-6 and 0.0 < c_n < 1e-3


# ---- the plan -----------------------------------------------------------------------------------------------------------------------------------
def test_coef_prev_follows_dpm_solver_coefs():
    from generative_models_amd.diffusion.gaussian_diffusion import dpm_solver_coefs, stochastic_coefs
    for T in STEPS:
        for start in (None, 1, max(1, T // 2), T):
            dpm, sde = dpm_solver_coefs(T, start), stochastic_coefs(T, "sde_dpmpp_2m", start=start)
            assert [(r.i, r.lt, r.ls, r.coef_prev) for r in sde] == [(d.i, d.lt, d.ls, d.coef_prev) for d in dpm]
            assert sde[0].coef_prev == 0.0 and sde[-1].coef_prev == 0.0 and sde[-1].i == 0
            whole = stochastic_coefs(T, "sde_dpmpp_2m")[T - len(sde):]           # a chain from part-way: its first row has no history
            assert len(sde) == (T if start is None else start) and sde[1:] == whole[1:] and sde[0] == whole[0]._replace(coef_prev=0.0)
            for kind in ("ancestral", "ddim_eta"):
                rows = stochastic_coefs(T, kind, ddim_eta=0.5, start=start)
                assert rows == stochastic_coefs(T, kind, ddim_eta=0.5)[T - len(rows):] and all(r.coef_prev == 0.0 for r in rows)
    assert any(r.coef_prev > 0.0 for r in stochastic_coefs(4, "sde_dpmpp_2m"))
    with pytest.raises(ValueError, match="start"):
        stochastic_coefs(4, "ancestral", start=5)
    with pytest.raises(ValueError, match="kind"):
        stochastic_coefs(4, "noisy")
    with pytest.raises(ValueError, match="ddim_eta"):
        stochastic_coefs(4, "ddim_eta", ddim_eta=1.5)
    with pytest.raises(ValueError, match="posterior_var"):
        stochastic_coefs(4, "ancestral", "medium:2")


def test_sampler_plan_carries_the_rows():
    from generative_models_amd.diffusion.gaussian_diffusion import SamplerStep, sampler_plan, stochastic_coefs
    # the row trails the seven tuple fields and defaults to None: an old-style row is the tuple it always was
    import copy
    import pickle
    old = SamplerStep(0, 0.0, 1.0, True, 1, None, None)
    assert SamplerStep._fields == ("i", "lt", "ls", "is_last", "passes", "dpm", "inp") and old.sto is None and len(old) == 7
    assert old == (0, 0.0, 1.0, True, 1, None, None) and old == SamplerStep(0, 0.0, 1.0, True, 1, None, None, None)
    new = SamplerStep(0, 0.0, 1.0, True, 1, None, None, "row")
    assert new.sto == "row" and tuple(new) == tuple(old) and new != old and not new == old and hash(new) != hash(old)
    assert new._replace(passes=3).sto == "row" and new._replace(passes=3).passes == 3 and new._replace(sto=None) == old
    assert copy.deepcopy(new) == new and pickle.loads(pickle.dumps(new)) == new and "sto='row'" in repr(new)
    for sampler, kw, kind in (("ancestral", dict(posterior_var="medium:0.5"), "ancestral"), ("sde_dpmpp_2m", {}, "sde_dpmpp_2m"),
                              ("ddim", dict(ddim_eta=0.5), "ddim_eta")):
        for start in (None, 2):
            plan = sampler_plan(4, sampler, start=start, **kw)
            assert [s.sto for s in plan] == stochastic_coefs(4, kind, kw.get("posterior_var", "large"), kw.get("ddim_eta", 0.0), start=start)
            assert [s[:7] for s in plan] == [s[:7] for s in sampler_plan(4, "ddim", start=start)]        # DDIM's rows otherwise
            assert plan[-1].is_last and plan[-1].sto.i == 0 and all(s.passes == 1 and s.dpm is None for s in plan)
    for sampler in ("ddim", "noisy", "dpmpp_2m", "consistency", "teacher_test"):                        # the old loops carry none
        assert all(s.sto is None for s in sampler_plan(4, sampler))
    assert sampler_plan(4, "ddim", ddim_eta=0.0) == sampler_plan(4, "ddim")
    with pytest.raises(ValueError, match="ddim_eta"):
        sampler_plan(4, "noisy", ddim_eta=0.5)


# ---- options ------------------------------------------------------------------------------------------------------------------------------------
def _model_flags(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cpu", hidden_size=32, **flags)
    return Model, G


BAD = ((dict(sampler="ddim", posterior_var="small"), "posterior_var.*'ddim'"),
       (dict(sampler="noisy", posterior_var="medium:0.5"), "posterior_var.*'noisy'"),
       (dict(sampler="sde_dpmpp_2m", posterior_var="small"), "posterior_var.*'sde_dpmpp_2m'"),
       (dict(sampler="dpmpp_2m", posterior_var="small"), "posterior_var.*'dpmpp_2m'"),
       (dict(sampler="consistency", posterior_var="small"), "posterior_var.*'consistency'"),
       (dict(sampler="ancestral", ddim_eta=0.5), "ddim_eta.*'ancestral'"),
       (dict(sampler="noisy", ddim_eta=0.5), "ddim_eta.*'noisy'"),
       (dict(sampler="sde_dpmpp_2m", ddim_eta=1.0), "ddim_eta.*'sde_dpmpp_2m'"),
       (dict(sampler="dpmpp_2m", ddim_eta=0.1), "ddim_eta.*'dpmpp_2m'"),
       (dict(sampler="consistency", ddim_eta=0.1), "ddim_eta.*'consistency'"),
       (dict(sampler="ddim", ddim_eta=1.5), "ddim_eta"),
       (dict(sampler="ddim", ddim_eta=-0.1), "ddim_eta"),
       (dict(sampler="ddim", ddim_eta=float("nan")), "ddim_eta"),
       (dict(sampler="ddim", ddim_eta="much"), "ddim_eta"),
       (dict(sampler="ancestral", posterior_var="medium:1.5"), "posterior_var"),
       (dict(sampler="ancestral", posterior_var="medium:-0.1"), "posterior_var"),
       (dict(sampler="ancestral", posterior_var="medium:x"), "posterior_var"),
       (dict(sampler="ancestral", posterior_var="medium:nan"), "posterior_var"),
       (dict(sampler="ancestral", posterior_var="medium"), "posterior_var"),
       (dict(sampler="ancestral", posterior_var="huge"), "posterior_var"),
       (dict(sampler="ancestral", posterior_var=0.5), "posterior_var"))


def test_stochastic_check():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, stochastic_check
    assert stochastic_check("ddim") == (None, "large", 0.0) and stochastic_check("noisy", "large", 0) == (None, "large", 0.0)
    assert stochastic_check("ddim", "large", 0.5) == ("ddim_eta", "large", 0.5) and stochastic_check("ddim", ddim_eta=1) == ("ddim_eta", "large", 1.0)
    assert stochastic_check("ancestral") == ("ancestral", "large", 0.0)
    assert stochastic_check("ancestral", "medium:0.25") == ("ancestral", "medium:0.25", 0.0)
    assert stochastic_check("ancestral", "medium:0") == ("ancestral", "medium:0", 0.0) and stochastic_check("ancestral", "medium:1")[0] == "ancestral"
    assert stochastic_check("sde_dpmpp_2m") == ("sde_dpmpp_2m", "large", 0.0)
    for kw, match in BAD:
        with pytest.raises(ValueError, match=match):
            stochastic_check(**kw)
        with pytest.raises(ValueError, match=match):
            GaussianDiffusion(mean_type="v", num_steps=4, **kw)
    d = GaussianDiffusion(mean_type="v", num_steps=4, sampler="ancestral", posterior_var="medium:0.5")
    assert (d.sampler, d.posterior_var, d.ddim_eta) == ("ancestral", "medium:0.5", 0.0)
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    assert (d.sampler, d.posterior_var, d.ddim_eta) == ("ddim", "large", 0.0)


def test_model_takes_the_flags_and_refuses_at_construction():
    from generative_models_amd import main
    Model, _ = _model_flags()
    DG = Model.DG
    assert (DG.sampler, DG.posterior_var, DG.ddim_eta) == ("ddim", "large", 0.0) and type(DG.posterior_var) is str and type(DG.ddim_eta) is float
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--sampler", "ancestral", "--posterior_var", "medium:0.5"])
    assert (G.sampler, G.posterior_var, G.ddim_eta) == ("ancestral", "medium:0.5", 0.0)
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--ddim_eta", "0.5"])
    assert (G.sampler, G.posterior_var, G.ddim_eta) == ("ddim", "large", 0.5)
    for kw, match in BAD + ((dict(sampler="ancestral", inpaint_eval=1), "ancestral.*inpaint_eval"),
                            (dict(sampler="sde_dpmpp_2m", restore_eval=2), "sde_dpmpp_2m.*restore_eval"),
                            (dict(sampler="ddim", ddim_eta=0.5, inpaint_eval=1), "ddim_eta.*inpaint_eval"),
                            (dict(sampler="ddim", ddim_eta=0.5, restore_gray=1, in_channels=3), "ddim_eta.*restore_gray")):
        Model, G = _model_flags(**kw)
        with pytest.raises(ValueError, match=match):
            Model(G)
    for kw in (dict(sampler="ancestral", posterior_var="small"), dict(sampler="sde_dpmpp_2m", dyn_threshold=0.995), dict(sampler="ddim", ddim_eta=0.5),
               dict(sampler="ancestral", cfg_rescale=0.7), dict(sampler="ddim", inpaint_eval=1)):
        Model, G = _model_flags(timesteps=4, **kw)
        d = Model(G).diffusion
        assert (d.sampler, d.posterior_var, d.ddim_eta) == (kw["sampler"], kw.get("posterior_var", "large"), kw.get("ddim_eta", 0.0))


def test_sampler_refuses_before_anything_touches_a_device():
    """Inpainting, restoration, injected noise and n % 4 != 0, as sampler 'consistency' refuses them; 'ddim' at eta = 0 refuses none of it."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net = lambda *a, **k: None
    z = torch.zeros(2, 1, 4, 4)
    for kw, name in ((dict(sampler="ancestral", posterior_var="small"), "ancestral"), (dict(sampler="sde_dpmpp_2m"), "sde_dpmpp_2m"),
                     (dict(sampler="ddim", ddim_eta=0.5), "ddim_eta")):
        d = GaussianDiffusion(mean_type="v", num_steps=3, **kw)
        with pytest.raises(ValueError, match=name + ".*inpainting"):
            d.inpaint(net=net, x0=z, mask=torch.ones(1, 1, 4, 4), init_x=z)
        with pytest.raises(ValueError, match=name + ".*restoration"):
            d.restore(net=net, obs=torch.zeros(2, 1, 2, 2), factor=2, init_x=z)
        with pytest.raises(ValueError, match="noises"):
            d.sample(net=net, init_x=z, noises=torch.zeros(3, 2, 1, 4, 4))
        with pytest.raises(ValueError, match="multiple of 4"):
            d.sample(net=net, init_x=torch.zeros(2, 1, 3, 3))
    d = GaussianDiffusion(mean_type="v", num_steps=3)
    d.ddim_eta = 0.5                        # set after construction: the loop checks again
    with pytest.raises(ValueError, match="ddim_eta.*inpainting"):
        d.inpaint(net=net, x0=z, mask=torch.ones(1, 1, 4, 4), init_x=z)
    d.sampler = "noisy"
    with pytest.raises(ValueError, match="ddim_eta.*'noisy'"):
        d.sample(net=net, init_x=z)


# ---- the C surface --------------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry():
    from generative_models_amd import _lib
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, F, I, L, U = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64, ctypes.c_uint64
    assert protos["gmk_stochastic_step"] == (I, [P] * 6 + [F] * 6 + [I, U, U, U] + [P] * 5 + [I, I, L, P], [
        "v", "v_uncond", "cond_w", "z", "x_hist", "thr", "logsnr_t", "logsnr_s", "coef_z", "coef_x", "coef_noise", "coef_prev", "is_last", "seed",
        "offset", "q0", "z_next", "x_pred", "eps_pred", "z_dup", "logsnr_next", "mean_type", "B", "n", "stream"])
    assert _lib.PROTOS["gmk_stochastic_step"] == protos["gmk_stochastic_step"]
    text = open(os.path.join(ROOT, "include", "gmk.h")).read()
    assert "diffusion_utils.py:34-62" in text
    assert not any("stochastic" in name.lower() for _, _, name in _lib.parse_kernel_table())      # no profile label


def test_entry_rejects_bad_arguments_before_any_launch():
    from generative_models_amd import _lib
    lib = _lib.lib
    buf = ctypes.c_void_p(16)        # never dereferenced: argument checks come first

    def step(v=buf, vu=None, w=None, z=buf, xh=None, thr=None, lt=1.0, ls=2.0, cz=0.5, cx=0.5, cn=0.1, k=0.0, zn=buf, mt=0, B=2, n=64):
        return lib.gmk_stochastic_step(v, vu, w, z, xh, thr, lt, ls, cz, cx, cn, k, 0, 1, 0, 0, zn, None, None, None, None, mt, B, n, None)
    for kw in ({"v": None}, {"z": None}, {"zn": None}):
        assert step(**kw) == -1 and b"gmk_stochastic_step: null pointer" in lib.gmk_last_error()
    assert step(vu=buf) == -1 and b"go together" in lib.gmk_last_error()
    assert step(w=buf) == -1 and b"go together" in lib.gmk_last_error()
    assert step(n=66) == -1 and b"gmk_stochastic_step: n = 66" in lib.gmk_last_error()
    for name in ("lt", "ls", "cz", "cx", "cn", "k"):
        for bad in (float("nan"), float("inf"), -float("inf")):
            assert step(**{name: bad}) == -1 and b"gmk_stochastic_step: non-finite time or coefficient" in lib.gmk_last_error(), (name, bad)
    assert step(cn=-0.1) == -1 and b"gmk_stochastic_step: coef_noise = -0.1" in lib.gmk_last_error()
    assert step(k=0.5) == -1 and b"gmk_stochastic_step: coef_prev = 0.5 without x_hist" in lib.gmk_last_error()
    for kw in ({"B": 0}, {"B": 65536}, {"n": 0}, {"mt": 3}, {"mt": -1}):
        assert step(**kw) == -1 and b"gmk_stochastic_step" in lib.gmk_last_error()


def test_wrapper_checks_before_asking_for_a_device():
    from generative_models_amd import ops
    t = torch.zeros(2, 8)
    ok = (0.0, 1.0, 0.5, 0.5, 0.1, 0.0, False, 0, 0)
    with pytest.raises(ValueError, match="mean_type"):
        ops.stochastic_step(t, t, *ok, mean_type="both")
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.stochastic_step(torch.zeros(2, 6), torch.zeros(2, 6), *ok)
    with pytest.raises(ValueError, match="unsigned 64-bit"):
        ops.stochastic_step(t, t, 0.0, 1.0, 0.5, 0.5, 0.1, 0.0, False, -1, 0)
    with pytest.raises(ValueError, match="q0"):
        ops.stochastic_step(t, t, *ok, q0=-4)
    for at in range(6):
        bad = list(ok)
        bad[at] = float("nan")
        with pytest.raises(ValueError, match="non-finite"):
            ops.stochastic_step(t, t, *bad)
    with pytest.raises(ValueError, match="coef_noise"):
        ops.stochastic_step(t, t, 0.0, 1.0, 0.5, 0.5, -0.1, 0.0, False, 0, 0)
    with pytest.raises(ValueError, match="coef_prev.*x_hist"):
        ops.stochastic_step(t, t, 0.0, 1.0, 0.5, 0.5, 0.1, 0.5, False, 0, 0)
    with pytest.raises(ValueError, match="go together"):
        ops.stochastic_step(t, t, *ok, v_uncond=t)
    with pytest.raises(ValueError, match="device"):
        ops.stochastic_step(t, t, *ok)


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def test_step_restated():
    z, x, xp, xi = np.array([[0.5, -1.0]]), np.array([[0.25, 1.0]]), np.array([[1.0, -0.5]]), np.array([[2.0, -4.0]])
    assert np.array_equal(R.step(z, x, xi, 0.5, 2.0, 0.25, is_last=True), x)
    assert np.array_equal(R.step(z, x, xi, 0.5, 2.0, 0.25), 0.5 * z + 2.0 * x + 0.25 * xi)
    assert np.array_equal(R.step(z, x, None, 0.5, 2.0, 0.0), 0.5 * z + 2.0 * x)
    assert np.array_equal(R.step(z, x, xi, 0.5, 2.0, 0.25, k=0.5, x_prev=xp), 0.5 * z + 2.0 * (1.5 * x - 0.5 * xp) + 0.25 * xi)
    assert np.array_equal(R.step_bound(z, x, xi, 0.5, -2.0, 0.25, k=0.5, x_prev=xp),
                          8 * R.U24 * (0.5 * np.abs(z) + 2.0 * (1.5 * np.abs(x) + 0.5 * np.abs(xp)) + 0.25 * np.abs(xi)))
    assert R.second_order_k([(2, -20.0, -1.0), (1, -1.0, 1.0), (0, 1.0, 20.0)]) == [0.0, 1.0 / (2.0 * 9.5), 0.0]
    assert R.second_order_k([(3, -2.0, -2.0), (2, -2.0, 0.0), (1, 0.0, 1.0), (0, 1.0, 2.0)]) == [0.0, 0.0, 0.25, 0.0]
