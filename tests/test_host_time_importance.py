"""Host tests of the loss profile and the loss-aware time sampler (extensions; no GPU): the properties of the numpy float32 restatement
(tests/time_importance_ref.py) that the kernels inherit bit for bit, the option checks, the train state's keys and the CSV writer."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import time_importance_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
ZERO_STATE = np.zeros((5, R.BINS), dtype=F)


def bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


def uniform_like_rng(n, seed):
    """Values of gmk_rng_uniform's kind: multiples of 2^-24 in [0, 1)."""
    return (np.random.default_rng(seed).integers(0, 1 << 24, n).astype(np.float64) * 2.0 ** -24).astype(F)


# ---- the restatement's properties --------------------------------------------------------------------------------------------------------------
def test_warm_up_is_the_identity():
    """Not ready (p_k = 2^-6): u == u0 bit for bit and w == 1 for 10^5 rng-style values, the edge values and stratified draws with B = 7 (whose
    values are not multiples of 2^-24) - on the zero state and on a state one bin short of the warm-up count."""
    short = R.steep_state(6.0, count=8.0)
    short[0, 17] = F(4.0)
    draws = [uniform_like_rng(100000, 1), np.array([0.0, 1.0 - 2.0 ** -24, 1.0 / 3.0, 2.0 ** -30], dtype=F)]
    draws += [R.stratified(o, 7) for o in (0.0, 0.3, 1.0 - 2.0 ** -24, 1.0 / 7.0)]
    for state, warm in ((ZERO_STATE, 5.0), (short, 5.0)):
        assert not R.table(state, warm, 0.01)[3]
        for u0 in draws:
            u, w, p, wt = R.u_importance(state, u0, warm, 0.01)
            assert np.array_equal(bits(u), bits(u0))
            assert (w == F(1.0)).all() and (p == F(2.0 ** -6)).all() and (wt == F(1.0)).all()


@pytest.mark.parametrize("floor", [0.001, 0.05])
def test_steep_profiles_stay_in_range_in_their_bin_and_near_the_float64_inverse(floor):
    """Steep profiles, rising and falling: u in [0, 1), u inside the bin whose weight it carries (r_k across e^14 and across e^28), and each
    draw within 16 * 2^-24 / (64 p_k) of the float64 inverse CDF of the same fp32 table (r_k across e^14).

    Where the bound comes from, in units of 2^-24 / (64 p_k) (u moves by 1 / (64 p_k) per unit of t): t = u0 C is rounded once (half an ulp
    below 1: 1/2 unit), t - c_k is exact or nearly so, the quotient f < 1 is rounded once (p_k / 2 units).  The sum k + f lies below 64 and keeps
    multiples of 2^-18 from k = 32 on: half of that, times 2^-6, is 32 p_k units - the fp32 grid of u itself near 1, whatever the code does.
    The clamp onto the float below (k + 1) / 64 can cost a whole ulp of u at the top: 64 p_k units.  So 16 units can hold only for tables
    whose upper bins keep p_k below 1/4; the profile across e^14 has p_63 = 0.2 (worst possible 64 p + 1 = 13.7, worst seen on the CPU 12.7
    at u0 = 1 - 2^-24 and 6.6 elsewhere), the one across e^28 has p_63 = 0.36 and is held to the range, bin and weight statements only."""
    u0 = np.concatenate([uniform_like_rng(200000, 2), np.array([0.0, 1.0 - 2.0 ** -24, 2.0 ** -30, 0.5], dtype=F)])
    worst = 0.0
    for rate in (14.0, -14.0, 28.0, -28.0):
        state = R.steep_state(rate)
        u, w, p, wt = R.u_importance(state, u0, 5.0, floor)
        _, c, _, ready = R.table(state, 5.0, floor)
        assert ready
        assert (u >= 0).all() and (u < 1).all()
        kb = np.floor(u.astype(np.float64) * 64).astype(np.int64)
        assert np.array_equal(bits(w), bits(wt[kb]))                    # w[b] == w_out[floor(64 u[b])]
        u64, k64 = R.inverse_cdf64(p, c, u0)
        assert np.array_equal(kb, k64)
        assert p.min() >= F(floor) / F(64) and abs(float(p.astype(np.float64).sum()) - 1.0) < 1e-5
        if abs(rate) == 14.0:
            assert p[32:].max() < 0.25
            err = np.abs(u.astype(np.float64) - u64) / (2.0 ** -24 / (64.0 * p[k64].astype(np.float64)))
            worst = max(worst, float(err.max()))
    print(f"floor {floor}: worst distance from the float64 inverse CDF {worst:.2f} units of 2^-24 / (64 p_k)")
    assert worst <= 16.0


def test_weighted_mean_reproduces_the_integral():
    """E[w g(u)] over uniform u0 is the integral of g: 2^20 stratified u0 through a steep profile at floor 0.05, g smooth with a known
    integral, to 1e-3 relative (the midpoint-like rule's own error is far below; what is tested is that w is 1 / (64 p) of u's bin)."""
    B = 1 << 20
    u0 = R.stratified(F(0.37), B)
    g = lambda t: 1.0 + np.sin(2.0 * np.pi * t) ** 2 + t ** 3             # integral over [0, 1] = 1 + 1/2 + 1/4
    for rate in (28.0, -12.0):
        u, w, _, _ = R.u_importance(R.steep_state(rate), u0, 5.0, 0.05)
        est = float(np.mean(w.astype(np.float64) * g(u.astype(np.float64))))
        assert abs(est - 1.75) <= 1e-3 * 1.75, (rate, est)
        assert abs(float(np.mean(w.astype(np.float64))) - 1.0) <= 1e-3


def test_degenerate_profiles_fall_back_to_uniform():
    """Every S2 = 0 (R = 0), warm = 0 on the zero state (0 / 0), an infinite S2: p_k = 2^-6, u == u0, w == 1."""
    u0 = uniform_like_rng(1000, 3)
    zero_s2 = R.steep_state(3.0)
    zero_s2[2] = 0
    inf_s2 = R.steep_state(3.0)
    inf_s2[2, 5] = np.inf
    for state, warm in ((zero_s2, 5.0), (ZERO_STATE, 0.0), (inf_s2, 5.0)):
        assert R.table(state, warm, 0.01)[3]                            # ready - and still uniform
        u, w, p, _ = R.u_importance(state, u0, warm, 0.01)
        assert np.array_equal(bits(u), bits(u0)) and (w == F(1.0)).all() and (p == F(2.0 ** -6)).all()


def test_profile_update_rules():
    """Bins, sequential sums, decay, skipped samples and untouched rows, on values small enough to check by hand."""
    u = np.array([0.0, 1.0 / 64, 1.0 / 64 + 2.0 ** -20, 1.0 - 2.0 ** -24, 0.5, 1.0, -0.25, np.nan, 0.5, 0.5], dtype=F)
    v0 = np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0, np.nan, 0.25], dtype=F)
    v1 = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, np.inf], dtype=F)
    s = R.loss_profile(ZERO_STATE, u, v0, None, 0.9)
    assert s[0, 0] == 1 and s[0, 1] == 2 and s[0, 63] == 1 and s[0, 32] == 2 and s[0].sum() == 6     # u = 1, u < 0, NaN u, NaN v0 are skipped
    assert s[1, 1] == 5 and s[2, 1] == 13 and s[1, 32] == 5.25 and s[2, 63] == 16
    assert not s[3:].any()                                              # no v1: rows 3, 4 keep their bits
    s1 = R.loss_profile(ZERO_STATE, u, v0, v1, 1.0)
    assert s1[0, 32] == 1 and s1[1, 32] == 5 and s1[3, 32] == 1       # the sample with an infinite v1 is skipped entirely
    s2 = R.loss_profile(s1, u, v0, v1, 0.5)
    assert s2[0, 1] == F(0.5) * 2 + 2 and s2[2, 1] == F(0.5) * 13 + 13 and s2[4, 1] == 3
    # a batch of skipped samples leaves every bit where it was, NaN payloads included
    odd = s2.copy()
    odd[1, 40] = np.nan
    bad = R.loss_profile(odd, np.array([1.0, 2.0, np.nan, 0.3], dtype=F), np.array([1.0, 1.0, 1.0, np.inf], dtype=F), None, 0.9)
    assert np.array_equal(bits(bad), bits(odd))
    # bins a batch does not reach do not decay
    one = R.loss_profile(s2, np.array([0.25], dtype=F), np.array([2.0], dtype=F), np.array([3.0], dtype=F), 0.9)
    changed = bits(one) != bits(s2)
    assert changed[:, 16].all() and not np.delete(changed, 16, axis=1).any()


def test_warmed_bin_never_drops_below_the_warm_up_count():
    """decay 0.9, warmup 5 (the defaults, at the bound 0.5 / (1 - decay)): over 10^5 single-sample updates a bin that has reached 5 stays there."""
    rng = np.random.default_rng(4)
    ks = rng.integers(0, R.BINS, 100000)
    state = ZERO_STATE.copy()
    reached = np.zeros(R.BINS, dtype=bool)
    one = np.array([1.0], dtype=F)
    for k in ks[:2000]:                                                  # through the restatement itself
        state = R.loss_profile(state, np.array([(k + 0.5) / 64], dtype=F), one, None, 0.9)
        reached |= state[0] >= 5
        assert (state[0][reached] >= 5).all()
    W = state[0].copy()
    for k in ks[2000:]:                                                  # the same rule on W alone
        W[k] = F(0.9) * W[k] + F(1.0)
        reached[k] |= W[k] >= 5
        assert W[k] >= 5 or not reached[k]
    assert reached.all() and (W <= F(10.0)).all()


# ---- options ---------------------------------------------------------------------------------------------------------------------------------
def test_check_names_the_flag():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, time_importance_check as chk
    assert chk(0, 0.9, 5, 0.01, 0) == (0, 0.9, 5.0, 0.01, 0)
    assert chk(1, "0.99", 50, 1.0, 1) == (1, 0.99, 50.0, 1.0, 1)
    assert chk(1, 1.0, 1e6, 0.5, 0)[2] == 1e6                            # decay 1: no bound on the warm-up
    for name, pos in (("time_importance", 0), ("loss_profile", 4)):
        for bad in (2, -1, 0.5, "on", None, True):
            args = [0, 0.9, 5, 0.01, 0]
            args[pos] = bad
            with pytest.raises(ValueError, match=name):
                chk(*args)
    for bad in (0.0, -0.1, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError, match="importance_decay"):
            chk(1, bad, 5, 0.01, 0)
        with pytest.raises(ValueError, match="importance_floor"):
            chk(1, 0.9, 5, bad, 0)
    for bad in (-1, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="importance_warmup"):
            chk(1, 0.9, bad, 0.01, 0)
    with pytest.raises(ValueError, match="importance_warmup.*importance_decay"):
        chk(1, 0.9, 5.5, 0.01, 0)                                        # above 0.5 / (1 - 0.9)
    with pytest.raises(ValueError, match="importance_warmup"):
        chk(0, 0.5, 2, 0.01, 1)
    for args, name in (((1, 0.9, 5, 0.01, 0), "time_importance"), ((0, 0.9, 5, 0.01, 1), "loss_profile")):
        with pytest.raises(ValueError, match=f"{name}.*teacher"):
            chk(*args, has_teacher=True)
    with pytest.raises(ValueError, match="time_importance.*2 ranks.*per-step collective"):
        chk(1, 0.9, 5, 0.01, 0, world=2)
    assert chk(0, 0.9, 5, 0.01, 1, world=8)[4] == 1                      # the profile alone runs data-parallel
    with pytest.raises(ValueError, match="time_importance"):
        GaussianDiffusion(mean_type="v", num_steps=4, teacher_net=object(), teacher_mode="step2", time_importance=1)
    with pytest.raises(ValueError, match="importance_floor"):
        GaussianDiffusion(mean_type="v", num_steps=4, importance_floor=0)
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    assert (d.time_importance, d.importance_decay, d.importance_warmup, d.importance_floor, d.loss_profile) == (0, 0.9, 5.0, 0.01, 0)
    assert d.time_profile is None and d.profile("train") is None and d.profile("test") is None


def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cpu", **flags)
    return Model(G)


def test_defaults_flags_and_model_checks(monkeypatch):
    from generative_models_amd import common, main, parallel
    Model = common.discover_models()["diffusion_model"]
    DG = Model.DG
    assert (DG.time_importance, DG.importance_decay, DG.importance_warmup, DG.importance_floor, DG.loss_profile) == (0, 0.9, 5, 0.01, 0)
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert (G.time_importance, G.importance_decay, G.importance_warmup, G.importance_floor, G.loss_profile) == (0, 0.9, 5, 0.01, 0)
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--time_importance", "1", "--importance_decay", "0.95", "--importance_warmup", "8",
                                           "--importance_floor", "0.02", "--loss_profile", "1"])
    assert (G.time_importance, G.importance_decay, G.importance_warmup, G.importance_floor, G.loss_profile) == (1, 0.95, 8, 0.02, 1)
    m = _model(time_importance=1, loss_profile=1, importance_decay=0.95, importance_warmup=8)
    d = m.diffusion
    assert (d.time_importance, d.importance_decay, d.importance_warmup, d.loss_profile, m.loss_profile) == (1, 0.95, 8.0, 1, 1)
    for key, bad in (("time_importance", 2), ("loss_profile", -1), ("importance_decay", 0.0), ("importance_decay", 1.01), ("importance_floor", 0.0),
                     ("importance_floor", 2.0), ("importance_warmup", -1), ("importance_warmup", 6)):
        with pytest.raises(ValueError, match=key):
            _model(**{key: bad})
    monkeypatch.setattr(parallel, "world", lambda: 2)
    with pytest.raises(ValueError, match="time_importance.*ranks"):
        _model(time_importance=1)
    assert _model(loss_profile=1).diffusion.loss_profile == 1


def test_graph_path_is_left_when_a_flag_is_on(monkeypatch):
    x = torch.zeros((8, 1, 8, 8))
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    assert _model()._graphable(x, 1)
    assert not _model(time_importance=1)._graphable(x, 1)
    assert not _model(loss_profile=1)._graphable(x, 1)


# ---- the train state ---------------------------------------------------------------------------------------------------------------------------
def test_train_state_key_only_with_a_flag():
    keys = {"optimizer", "rng", "aux_rng", "dropout", "digests"}
    assert set(_model().train_state()) == keys
    for flags in (dict(time_importance=1), dict(loss_profile=1)):
        m = _model(**flags)
        state = m.train_state()
        assert set(state) == keys | {"time_profile"}
        prof = state["time_profile"]
        assert prof.dtype == torch.float32 and tuple(prof.shape) == (5, 64) and not prof.is_cuda and not prof.any()
        # back in: the saved profile, and zeros from a state written without the flags
        state["time_profile"] = torch.arange(320, dtype=torch.float32).reshape(5, 64)
        m.load_train_state(state)
        assert torch.equal(m.diffusion.time_profile, state["time_profile"]) and m.diffusion.time_profile is not state["time_profile"]
        assert torch.equal(m.train_state()["time_profile"], state["time_profile"])
        del state["time_profile"]
        m.load_train_state(state)
        assert tuple(m.diffusion.time_profile.shape) == (5, 64) and not m.diffusion.time_profile.any()
    from generative_models_amd import checkpoint
    assert checkpoint.FORMAT_VERSION == 1


# ---- the CSV writer ----------------------------------------------------------------------------------------------------------------------------
def test_csv_writer(tmp_path):
    from generative_models_amd import main
    from generative_models_amd.diffusion.gaussian_diffusion import logsnr_schedule_cosine_host, profile_rows
    state = np.zeros((5, 64), dtype=F)
    state[:, 0] = [2, 1, 8, 1, 1]
    state[:, 63] = [4, 3, 16, 1, 1]
    path = main.append_loss_profile(tmp_path, 0, "test", profile_rows(state))
    p = np.full(64, 1.0 / 64)
    assert main.append_loss_profile(tmp_path, 3, "train", profile_rows(state, p)) == path == tmp_path / "loss_profile.csv"
    lines = path.read_text().splitlines()
    assert lines[0] == "epoch,split,bin,u_lo,u_hi,logsnr_hi,logsnr_lo,weight,loss_mean,loss_rms,x_mse_mean,p"
    assert len(lines) == 1 + 64 + 64
    rows = [dict(zip(lines[0].split(","), ln.split(","))) for ln in lines[1:]]
    assert [r["bin"] for r in rows[:64]] == [str(k) for k in range(64)] and {r["split"] for r in rows[:64]} == {"test"}
    assert {r["epoch"] for r in rows[64:]} == {"3"} and {r["split"] for r in rows[64:]} == {"train"}
    first, last, empty = rows[0], rows[63], rows[5]
    assert (float(first["u_lo"]), float(first["u_hi"]), float(first["logsnr_hi"])) == (0.0, 1.0 / 64, 20.0)
    assert float(first["logsnr_lo"]) == pytest.approx(float(logsnr_schedule_cosine_host(1.0 / 64)), rel=1e-7)
    assert float(rows[1]["logsnr_hi"]) == float(first["logsnr_lo"])
    # (the fp32 schedule at u = 1: d logsnr / d t = 4 / sin(2 t) = 4.4e4 at t = atan(e^10), times half an ulp of t, 6e-8: a few 1e-3)
    assert (float(last["u_hi"]), float(last["logsnr_lo"])) == (1.0, pytest.approx(-20.0, abs=1e-2))
    assert F(last["logsnr_lo"]) == logsnr_schedule_cosine_host(1.0)          # nine digits carry an fp32 value
    assert (float(first["weight"]), float(first["loss_mean"]), float(first["loss_rms"]), float(first["x_mse_mean"]), first["p"]) == (2, 0.5, 2, 0.5, "")
    assert (float(last["weight"]), float(last["loss_mean"]), float(last["loss_rms"]), float(last["x_mse_mean"])) == (4, 0.75, 2, 0.25)
    assert (empty["weight"], empty["loss_mean"], empty["loss_rms"], empty["x_mse_mean"]) == ("0", "", "", "")
    assert all(float(r["p"]) == 1.0 / 64 for r in rows[64:])


# ---- the C surface -----------------------------------------------------------------------------------------------------------------------------
def test_header_and_argument_checks():
    from generative_models_amd import _lib, ops
    P, Fl, I = ctypes.c_void_p, ctypes.c_float, ctypes.c_int
    assert _lib.PROTOS["gmk_loss_profile"] == (I, [P, P, P, I, Fl, P, P], ["u", "v0", "v1", "B", "decay", "state", "stream"])
    assert _lib.PROTOS["gmk_u_importance"] == (I, [P, P, P, P, I, Fl, Fl, P, P, P],
                                               ["state", "u0", "u", "w", "B", "warm", "floor", "p_out", "w_out", "stream"])
    hdr = open(os.path.join(ROOT, "include", "gmk.h")).read()
    assert "#define GMK_PROFILE_BINS 64" in hdr and ops.PROFILE_BINS == R.BINS == 64 and "Nichol & Dhariwal 2021" in hdr
    lib = _lib.lib
    buf = ctypes.c_void_p(16)            # never dereferenced: argument checks come first
    for args in ((None, buf, None, 4, 0.9, buf), (buf, None, None, 4, 0.9, buf), (buf, buf, None, 4, 0.9, None)):
        assert lib.gmk_loss_profile(*args, None) == -1 and b"gmk_loss_profile: null pointer" in lib.gmk_last_error()
    for B in (0, -1, (1 << 24) + 1):
        assert lib.gmk_loss_profile(buf, buf, None, B, 0.9, buf, None) == -1 and b"gmk_loss_profile: B" in lib.gmk_last_error()
    for decay in (0.0, -0.5, 1.5, float("nan")):
        assert lib.gmk_loss_profile(buf, buf, None, 4, decay, buf, None) == -1 and b"gmk_loss_profile: decay" in lib.gmk_last_error()
    for args in ((None, buf, buf, buf), (buf, None, buf, buf), (buf, buf, None, buf), (buf, buf, buf, None)):
        assert lib.gmk_u_importance(*args, 4, 5.0, 0.01, None, None, None) == -1 and b"gmk_u_importance: null pointer" in lib.gmk_last_error()
    for B in (0, (1 << 24) + 1):
        assert lib.gmk_u_importance(buf, buf, buf, buf, B, 5.0, 0.01, None, None, None) == -1 and b"gmk_u_importance: B" in lib.gmk_last_error()
    for warm in (-1.0, float("nan")):
        assert lib.gmk_u_importance(buf, buf, buf, buf, 4, warm, 0.01, None, None, None) == -1 and b"gmk_u_importance: warm" in lib.gmk_last_error()
    for floor in (0.0, 1.5, float("nan")):
        assert lib.gmk_u_importance(buf, buf, buf, buf, 4, 5.0, floor, None, None, None) == -1 and b"gmk_u_importance: floor" in lib.gmk_last_error()
    # the wrappers check first, by name
    state, t = torch.zeros(5, 64), torch.zeros(8)
    with pytest.raises(ValueError, match="device"):
        ops.loss_profile(t, t, None, state, 0.9)
    with pytest.raises(ValueError, match="device"):
        ops.u_importance(state, t, 5.0, 0.01)
