"""Host tests of the parametrised noise schedules (`Schedule`, `schedule_check`, the `schedule=` keyword of the sampler grids, the five
flags): `Schedule.host` against the reference's own fp32 output (tests/golden/logsnr_schedules.npz, written by tools/make_schedule_golden.py)
and against the restatement of tests/schedule_ref.py, the grids bit for bit, the coefficient tables against their float64 formulas, and the
refusals by flag name.  Bar of the golden comparison: |got - ref| <= 2e-6 max(1, |ref|), the bar of test_sampler_index_arithmetic_bit_exact."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedule_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(k, lo, hi) for k in R.KINDS for lo, hi in R.RANGES]
IDS = [R.golden_key(*c) for c in CASES]
SHIFTS = (-1.386, 0.5, 10.0)
HOST_BAR = 2e-6


@pytest.fixture(scope="module")
def gold():
    return R.load_golden()


def G():
    from generative_models_amd.diffusion import gaussian_diffusion
    return gaussian_diffusion


def bits(a):
    return np.asarray(a).tobytes()


# ---- Schedule.host -------------------------------------------------------------------------------------------------------------------------
def test_golden_file_covers_the_cases(gold):
    u = gold["u"]
    assert u.dtype == np.float32 and tuple(gold["kinds"]) == R.KINDS and [tuple(r) for r in gold["ranges"]] == list(R.RANGES)
    for v in (0.0, 1.0, 1.0 / 64, 63.0 / 64, 0.999, 1e-4, 0.03, 0.4):
        assert np.float32(v) in u
    for T in (4, 250):
        a, b = gold[f"grid_T{T}"]
        assert bits(u[a:b]) == bits(np.arange(T + 1, dtype=np.float32) / np.float32(T))
    assert len(u) > 500 and os.path.getsize(R.GOLDEN) < 100 * 1024
    for c in CASES:
        assert gold[R.golden_key(*c)].dtype == np.float32 and gold[R.golden_key(*c)].shape == u.shape


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_against_the_reference_output(gold, case):
    kind, lo, hi = case
    S = G().Schedule(kind, lo, hi, 0.0)
    u, ref = gold["u"], gold[R.golden_key(*case)].astype(np.float64)
    got = S.host(u)
    assert got.dtype == np.float32 and got.shape == u.shape
    one = np.array([S.host(v) for v in u])
    assert all(type(S.host(v)) is np.float32 for v in u[:4]) and bits(one) == bits(got)          # a scalar is the array's element
    err = float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))))
    mine = float(np.max(np.abs(R.logsnr32(kind, lo, hi, 0.0, u) - ref) / np.maximum(1.0, np.abs(ref))))
    print(f"{R.golden_key(*case)}: Schedule.host {err:.3e}, schedule_ref.logsnr32 {mine:.3e} of max(1, |ref|)")
    assert err <= HOST_BAR and mine <= HOST_BAR
    if kind == "uniform":
        assert bits(got) == bits(gold[R.golden_key(*case)])
    assert bits(got) == bits(R.logsnr32(kind, lo, hi, 0.0, u))                                   # two restatements of the same steps
    # and the float64 formula, as far as fp32 can follow it: 10 ulps of 20 (2e-5) for the rounding of the log-SNR and of the argument where the
    # function is tame; the cosine form's argument t nears pi / 2 at its bottom end, where d logsnr / d t = 2 / (sin t cos t) ~ 2 exp(-lmin / 2)
    # multiplies t's rounding (up to an ulp of pi / 2, 2^-23, over the product and the sum): 5e-3 at lmin = -20, 2e-4 at -15
    f64 = R.logsnr64(kind, lo, hi, 0.0, u.astype(np.float64))
    slack = 2.0 * np.exp(-0.5 * lo) * 2.0 ** -23 if kind == "cosine" else 0.0
    assert float(np.max(np.abs(got - f64))) <= 2e-5 + slack


def test_default_schedule_is_the_cosine_host_function(gold):
    g = G()
    S = g.Schedule()
    assert S == g.Schedule("cosine", -20.0, 20.0, 0.0) and S.full_range
    assert bits(S.a) == bits(g.SCHED_A) and bits(S.b) == bits(g.SCHED_B)
    u = gold["u"]
    assert bits(S.host(u)) == bits(g.logsnr_schedule_cosine_host(u))
    for v in u:
        a, b = S.host(v), g.logsnr_schedule_cosine_host(v)
        assert type(a) is type(b) is np.float32 and bits(a) == bits(b)
    with pytest.raises(AttributeError):
        S.kind = "uniform"                                                                        # immutable


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_shift_is_one_fp32_add(gold, case):
    g = G()
    u = gold["u"]
    base = g.Schedule(*case, 0.0).host(u)
    for s in SHIFTS:
        got = g.Schedule(*case, s).host(u)
        assert got.dtype == np.float32 and bits(got) == bits((base + np.float32(s)).astype(np.float32))
        assert bits(got) == bits(R.logsnr32(*case, s, u))
    assert bits(g.Schedule(*case, 0).host(u)) == bits(base) == bits(g.Schedule(*case, -0.0).host(u))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_monotone_and_finite(gold, case):
    S = G().Schedule(*case, -1.386)
    u = np.sort(np.concatenate([gold["u"], np.linspace(0, 1, 4097, dtype=np.float32)]))
    l = S.host(u)
    assert np.all(np.isfinite(l)) and np.all(np.diff(l) <= 0)
    top, bottom = S.host(0.0), S.host(1.0)
    assert np.isfinite(top) and np.isfinite(bottom) and top > bottom
    lo, hi = case[1] - 1.386, case[2] - 1.386
    assert abs(top - hi) <= 1e-5 * abs(hi) and abs(bottom - lo) <= 2e-3            # (the cosine form's bottom end is 1e-3 off at -20)


# ---- the grids -----------------------------------------------------------------------------------------------------------------------------
GRID_SCHEDULES = [("uniform", -20.0, 20.0, 0.0), ("beta_linear", -15.0, 15.0, -0.5), ("beta_const", -10.0, 20.0, 0.0), ("cosine", -15.0, 15.0, -1.386)]


@pytest.mark.parametrize("sched", GRID_SCHEDULES, ids=lambda s: s[0])
@pytest.mark.parametrize("T", [1, 4, 250])
def test_grids_carry_the_schedule_bit_for_bit(sched, T):
    g = G()
    S = g.Schedule(*sched)
    rows = g.sampler_grid(T, schedule=S)
    assert [r[0] for r in rows] == list(range(T))[::-1]
    for (i, lt, ls), (i2, lt2, ls2) in zip(rows, R.grid(*sched, T)):
        u_t, u_s = g.sampler_times(i, T)
        assert type(lt) is type(ls) is np.float32
        assert bits(lt) == bits(S.host(u_t)) == bits(lt2) and bits(ls) == bits(S.host(u_s)) == bits(ls2) and i == i2
    for sampler in ("ddim", "dpmpp_2m"):
        for start in (None, 1, T):
            plan = g.sampler_plan(T, sampler, None, start, schedule=S)
            want = rows if start is None else rows[T - start:]
            assert [(p.i, bits(p.lt), bits(p.ls)) for p in plan] == [(i, bits(lt), bits(ls)) for i, lt, ls in want]
            assert plan[-1].is_last and all((p.dpm is not None) == (sampler == "dpmpp_2m") for p in plan)
    plan = g.sampler_plan(T, "ddim", 2, None, schedule=S)
    assert [(float(p.inp.lt), float(p.inp.ls)) for p in plan] == [(float(lt), float(ls)) for _, lt, ls in rows]
    lam = g.ode_logsnr_grid(T, schedule=S)
    assert lam == [float(S.host(np.float32(np.float32(i) / np.float32(T)))) for i in range(T + 1)]
    assert lam[:-1] == [float(ls) for _, _, ls in rows][::-1] and lam[-1] == float(rows[0][1])


@pytest.mark.parametrize("sched", GRID_SCHEDULES, ids=lambda s: s[0])
def test_coefficient_tables_follow_the_schedule(sched):
    g = G()
    S = g.Schedule(*sched)
    for T in (4, 20):
        rows = R.grid(*sched, T)
        for start in (None, 3):
            got = g.dpm_solver_coefs(T, start, schedule=S)
            part = rows if start is None else rows[T - start:]
            assert len(got) == len(part)
            for r, (i, lt, ls), (h, cz, cx, cp) in zip(got, part, R.dpm_rows(part)):
                assert (r.i, r.lt, r.ls) == (i, float(lt), float(ls))
                assert r.h == pytest.approx(h, rel=1e-12) and r.coef_z == pytest.approx(cz, rel=1e-12)
                assert r.coef_x == pytest.approx(cx, rel=1e-12) and r.coef_prev == pytest.approx(cp, rel=1e-12, abs=1e-300)
        got = g.inpaint_coefs(T, schedule=S)
        for r, (i, lt, ls), (a_s, s_s, a, b) in zip(got, rows, R.inpaint_rows(rows)):
            assert (r.i, r.lt, r.ls, r.is_last) == (i, float(lt), float(ls), i == 0)
            assert r.alpha_s == pytest.approx(a_s, rel=1e-12) and r.sigma_s == pytest.approx(s_s, rel=1e-12)
            assert r.a == pytest.approx(a, rel=1e-12) and r.b == pytest.approx(b, rel=1e-6, abs=1e-9)          # 1 - a^2 cancels; the table's form does not


def test_without_a_schedule_every_grid_is_todays():
    g = G()
    for T in (1, 4, 250):
        assert g.sampler_grid(T, schedule=None) == g.sampler_grid(T) == g.sampler_grid(T, g.Schedule())
        assert all(bits(a) == bits(b) for r, q in zip(g.sampler_grid(T), g.sampler_grid(T, schedule=g.Schedule())) for a, b in zip(r, q))
        assert g.dpm_solver_coefs(T, None, schedule=None) == g.dpm_solver_coefs(T) == g.dpm_solver_coefs(T, schedule=g.Schedule())
        assert g.dpm_solver_coefs(T, 1, schedule=None) == g.dpm_solver_coefs(T, 1)
        assert g.inpaint_coefs(T, schedule=None) == g.inpaint_coefs(T) == g.inpaint_coefs(T, g.Schedule())
        for sampler in ("ddim", "dpmpp_2m"):
            assert g.sampler_plan(T, sampler, None, None, schedule=None) == g.sampler_plan(T, sampler) == g.sampler_plan(T, sampler, schedule=g.Schedule())
        assert g.sampler_plan(T, "ddim", 2, 1, schedule=None) == g.sampler_plan(T, "ddim", 2, 1)
        assert g.ode_logsnr_grid(T, schedule=None) == g.ode_logsnr_grid(T) == g.ode_logsnr_grid(T, g.Schedule())
    for a, b, c in zip(g.profile_bin_edges(), g.profile_bin_edges(schedule=None), g.profile_bin_edges(schedule=g.Schedule())):
        assert bits(a) == bits(b) == bits(c)
    d = g.GaussianDiffusion(mean_type="v", num_steps=4)
    assert d.schedule is None and d.sample_schedule is None


def test_profile_edges_and_rows_follow_the_training_schedule():
    g = G()
    S = g.Schedule("beta_linear", -15.0, 15.0, -0.5)
    u_lo, u_hi, l_hi, l_lo = g.profile_bin_edges(schedule=S)
    assert bits(u_lo) == bits(g.profile_bin_edges()[0]) and bits(u_hi) == bits(g.profile_bin_edges()[1])
    assert bits(l_hi) == bits(S.host(u_lo)) == bits(R.logsnr32("beta_linear", -15.0, 15.0, -0.5, u_lo)) and bits(l_lo) == bits(S.host(u_hi))
    rows = g.profile_rows(np.ones((5, 64), np.float32), schedule=S)
    assert bits(rows["logsnr_hi"]) == bits(l_hi) and bits(rows["logsnr_lo"]) == bits(l_lo)
    d = g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=S, loss_profile=1)
    d.time_profile = torch.ones((5, 64))
    assert bits(d.profile("train")["logsnr_lo"]) == bits(l_lo)


# ---- validation and flags ------------------------------------------------------------------------------------------------------------------
def test_schedule_check_names_the_flag():
    g = G()
    tr, sa = g.schedule_check("cosine", -20.0, 20.0, 0.0, "")
    assert tr == sa == g.Schedule()
    tr, sa = g.schedule_check("beta_linear", "-15", 15, -0.5, "uniform")
    assert tr == g.Schedule("beta_linear", -15.0, 15.0, -0.5) and sa == g.Schedule("uniform", -15.0, 15.0, -0.5)
    assert g.schedule_check("uniform", -20, 20, 10.0, None)[1].kind == "uniform"
    for bad in ("linear", "beta_interp", "iddpm_cosine_interp", "", None, 3):
        with pytest.raises(ValueError, match="^logsnr_schedule"):
            g.schedule_check(bad, -20.0, 20.0, 0.0, "")
    for bad in ("linear", "beta_interp", 3):
        with pytest.raises(ValueError, match="^sample_logsnr_schedule"):
            g.schedule_check("cosine", -20.0, 20.0, 0.0, bad)
    for name, args in (("logsnr_min", (float("nan"), 20.0, 0.0)), ("logsnr_min", (float("-inf"), 20.0, 0.0)), ("logsnr_min", ("x", 20.0, 0.0)),
                       ("logsnr_min", (None, 20.0, 0.0)), ("logsnr_max", (-20.0, float("inf"), 0.0)), ("logsnr_max", (-20.0, float("nan"), 0.0)),
                       ("logsnr_shift", (-20.0, 20.0, float("nan"))), ("logsnr_shift", (-20.0, 20.0, float("inf"))), ("logsnr_shift", (-20.0, 20.0, "s")),
                       ("logsnr_min", (-20.5, 20.0, 0.0)), ("logsnr_max", (-20.0, 20.001, 0.0)), ("logsnr_min.*logsnr_max", (5.0, 5.0, 0.0)),
                       ("logsnr_min.*logsnr_max", (6.0, 5.0, 0.0)), ("logsnr_shift", (-20.0, 20.0, 10.5)), ("logsnr_shift", (-20.0, 20.0, -10.001))):
        with pytest.raises(ValueError, match="^" + name):
            g.schedule_check("cosine", *args, "")
    # the constructor runs the same check on a Schedule built by hand
    with pytest.raises(ValueError, match="logsnr_max"):
        g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=g.Schedule("cosine", -20.0, 30.0, 0.0))
    with pytest.raises(ValueError, match="logsnr_schedule"):
        g.GaussianDiffusion(mean_type="v", num_steps=4, sample_schedule=g.Schedule("linear"))
    with pytest.raises(ValueError, match="Schedule"):
        g.GaussianDiffusion(mean_type="v", num_steps=4, schedule="cosine")
    d = g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=g.Schedule("beta_const"))
    assert d.sample_schedule == d.schedule == g.Schedule("beta_const")
    d = g.GaussianDiffusion(mean_type="v", num_steps=4, sample_schedule=g.Schedule("uniform"))
    assert d.schedule is None and d.sample_schedule.kind == "uniform"


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    Gf = common.AttrDict(dict(Model.DG))
    Gf.update(lr=3e-4, pad32=0, device="cpu", hidden_size=32, **flags)
    return Model(Gf)


def test_flag_defaults_cli_and_model():
    from generative_models_amd import common, main
    g = G()
    DG = common.discover_models()["diffusion_model"].DG
    want = {"logsnr_schedule": "cosine", "logsnr_min": -20.0, "logsnr_max": 20.0, "logsnr_shift": 0.0, "sample_logsnr_schedule": ""}
    for k, v in want.items():
        assert DG[k] == v and type(DG[k]) is type(v), k
    Gf, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert all(Gf[k] == v for k, v in want.items())
    Gf, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--logsnr_schedule", "beta_linear", "--logsnr_min", "-15", "--logsnr_max", "15",
                                             "--logsnr_shift", "-1.386", "--sample_logsnr_schedule", "uniform"])
    assert (Gf.logsnr_schedule, Gf.logsnr_min, Gf.logsnr_max, Gf.logsnr_shift, Gf.sample_logsnr_schedule) == ("beta_linear", -15.0, 15.0, -1.386, "uniform")
    m = _model()
    assert m.diffusion.schedule is None and m.diffusion.sample_schedule is None                  # a default run stays on the original entries
    m = _model(logsnr_schedule="beta_linear", logsnr_min=-15.0, logsnr_max=15.0, logsnr_shift=-0.5, sample_logsnr_schedule="uniform")
    assert m.diffusion.schedule == g.Schedule("beta_linear", -15.0, 15.0, -0.5) and m.diffusion.sample_schedule == g.Schedule("uniform", -15.0, 15.0, -0.5)
    m = _model(sample_logsnr_schedule="uniform")
    assert m.diffusion.schedule is None and m.diffusion.sample_schedule == g.Schedule("uniform")
    m = _model(logsnr_schedule="beta_const", sample_logsnr_schedule="cosine")                     # the samplers on the default curve, the training not
    assert m.diffusion.schedule == g.Schedule("beta_const") and m.diffusion.sample_schedule == g.Schedule()
    m = _model(logsnr_shift=-1.386)
    assert m.diffusion.schedule == m.diffusion.sample_schedule == g.Schedule("cosine", -20.0, 20.0, -1.386)
    for key, bad in (("logsnr_schedule", "linear"), ("sample_logsnr_schedule", "beta_interp"), ("logsnr_min", -25.0), ("logsnr_max", float("nan")),
                     ("logsnr_shift", 11.0), ("logsnr_max", -20.0)):
        with pytest.raises(ValueError, match=key):
            _model(**{key: bad})


def test_likelihoods_take_the_full_range_only():
    from functools import partial

    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    g = G()
    net = SimpleUnet(32, 0.0)
    x = torch.zeros((2, 1, 8, 8))
    for S in (g.Schedule("cosine", -15.0, 15.0, 0.0), g.Schedule("uniform", -20.0, 20.0, -1.386), g.Schedule("beta_linear", -10.0, 20.0, 0.0)):
        d = g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=S)
        for call in (partial(d.nll, net=net, x=x, num_samples=2), partial(d.ode_nll, net=net, x=x, num_steps=4)):
            with pytest.raises(ValueError, match="logsnr_min.*logsnr_max.*logsnr_shift"):
                call()
    # any kind over exactly [-20, 20] passes the check: the calls go on to the next one (a host tensor is no device tensor)
    for kind in R.KINDS:
        d = g.GaussianDiffusion(mean_type="v", num_steps=4, schedule=g.Schedule(kind))
        assert d.schedule.full_range
        d._full_range("nll", d.schedule); d._full_range("ode_nll", d.sample_schedule)
        with pytest.raises(ValueError, match="num_samples"):
            d.nll(net=net, x=x, num_samples=0)
        with pytest.raises(ValueError, match="delta"):
            d.ode_nll(net=net, x=x, num_steps=4, delta=0.0)
    # the training range guards nll, the samplers' range ode_nll
    d = g.GaussianDiffusion(mean_type="v", num_steps=4, sample_schedule=g.Schedule("uniform", -10.0, 10.0, 0.0))
    with pytest.raises(ValueError, match="num_samples"):
        d.nll(net=net, x=x, num_samples=0)
    with pytest.raises(ValueError, match="logsnr_min"):
        d.ode_nll(net=net, x=x, num_steps=4)
    assert _model(logsnr_schedule="beta_linear", nlogp_samples=2, ode_nlogp_steps=4).diffusion.schedule.kind == "beta_linear"
    for flags in (dict(nlogp_samples=2, logsnr_shift=-1.0), dict(ode_nlogp_steps=4, logsnr_min=-15.0)):
        with pytest.raises(ValueError, match="logsnr_min.*logsnr_max.*logsnr_shift"):
            _model(**flags)


# ---- the C surface and the wrappers ----------------------------------------------------------------------------------------------------------
def test_header_declares_the_entries_and_the_old_ones_keep_their_prototypes():
    from generative_models_amd import _lib, ops
    protos = _lib.parse_header(os.path.join(ROOT, "include", "gmk.h"))
    P, Fl, I, L = ctypes.c_void_p, ctypes.c_float, ctypes.c_int, ctypes.c_int64
    assert protos["gmk_q_sample_sched"] == (I, [P] * 5 + [I, L, I] + [Fl] * 5 + [P],
                                            ["x", "eps", "u", "logsnr", "z", "B", "n", "kind", "a", "b", "lmin", "lmax", "shift", "stream"])
    assert protos["gmk_logsnr_schedule_sched"] == (I, [P, P, I, Fl, I] + [Fl] * 5 + [P, P, I, P],
                                                   ["u", "i_times", "num_steps", "u_shift", "kind", "a", "b", "lmin", "lmax", "shift", "u_out", "logsnr", "B", "stream"])
    assert protos["gmk_q_sample"] == (I, [P] * 5 + [I, L, P], ["x", "eps", "u", "logsnr", "z", "B", "n", "stream"])
    assert protos["gmk_logsnr_schedule"] == (I, [P, P, I, Fl, P, P, I, P], ["u", "i_times", "num_steps", "shift", "u_out", "logsnr", "B", "stream"])
    for name in ("gmk_q_sample_sched", "gmk_logsnr_schedule_sched"):
        assert _lib.PROTOS[name] == protos[name]
    C = _lib.parse_constants()
    assert [C[f"GMK_SCHED_{k.upper()}"] for k in R.KINDS] == [0, 1, 2, 3] and ops.SCHEDULES == dict(zip(R.KINDS, range(4)))
    text = open(os.path.join(ROOT, "include", "gmk.h")).read()
    assert text.count("diffusion_utils.py:169-201") >= 2


def test_entries_refuse_bad_arguments_without_a_device():
    from generative_models_amd._lib import lib
    buf = ctypes.c_void_p(16)
    ok = (0, 1.0, 0.0, -20.0, 20.0, 0.0)
    assert lib.gmk_q_sample_sched(buf, buf, buf, buf, None, 2, 64, *ok, None) == -1 and b"null pointer" in lib.gmk_last_error()
    assert lib.gmk_q_sample_sched(buf, buf, buf, buf, buf, 0, 64, *ok, None) == -1 and b"shape" in lib.gmk_last_error()
    assert lib.gmk_q_sample_sched(buf, buf, buf, buf, buf, 70000, 64, *ok, None) == -1 and b"shape" in lib.gmk_last_error()
    assert lib.gmk_q_sample_sched(buf, buf, buf, buf, buf, 2, 0, *ok, None) == -1 and b"shape" in lib.gmk_last_error()
    for kind in (-1, 4, 17):
        assert lib.gmk_q_sample_sched(buf, buf, buf, buf, buf, 2, 64, kind, *ok[1:], None) == -1 and b"kind" in lib.gmk_last_error()
        assert lib.gmk_logsnr_schedule_sched(buf, None, 1, 0.0, kind, *ok[1:], None, buf, 2, None) == -1 and b"kind" in lib.gmk_last_error()
    assert lib.gmk_q_sample_sched(buf, buf, buf, buf, buf, 2, 64, 0, float("nan"), 0.0, -20.0, 20.0, 0.0, None) == -1 and b"non-finite" in lib.gmk_last_error()
    assert lib.gmk_logsnr_schedule_sched(buf, None, 1, 0.0, 1, 0.0, 0.0, -20.0, 20.0, float("inf"), None, buf, 2, None) == -1 and b"non-finite" in lib.gmk_last_error()
    assert lib.gmk_logsnr_schedule_sched(buf, buf, 1, 0.0, *ok, None, buf, 2, None) == -1 and b"exactly one" in lib.gmk_last_error()
    assert lib.gmk_logsnr_schedule_sched(None, buf, 0, 0.0, *ok, None, buf, 2, None) == -1 and b"num_steps" in lib.gmk_last_error()


def test_wrappers_check_before_they_launch():
    from generative_models_amd import ops
    g = G()
    x, u = torch.zeros((3, 1, 5, 5)), torch.zeros(3)
    with pytest.raises(ValueError, match="device tensor"):
        ops.q_sample(x, x, u, schedule=g.Schedule("uniform"))
    with pytest.raises(ValueError, match="device tensor"):
        ops.logsnr_schedule(3, "cpu", u=u, schedule=g.Schedule("uniform"))
    with pytest.raises(ValueError, match="kind"):
        ops._sched_args(g.Schedule("linear"))
    assert ops._sched_args(g.Schedule("beta_linear", -15.0, 15.0, -0.5)) == (3, float(g.Schedule("beta_linear", -15.0, 15.0).a),
                                                                               float(g.Schedule("beta_linear", -15.0, 15.0).b), -15.0, 15.0, -0.5)
