"""CPU tests (no GPU) of post-hoc EMA (DG.ema_sigma_rel, generative_models_amd/posthoc_ema.py): the gamma root, the closed-form inner products
against a quadrature, the step weights, the least-squares reconstruction against the discrete weight vectors of tests/posthoc_ema_ref.py,
flag parsing and every refusal that needs no device."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import posthoc_ema_ref as R  # noqa: E402

from generative_models_amd import posthoc_ema as P  # noqa: E402

GAMMA_TABLE = {0.05: 16.972199, 0.07: 11.244939, 0.10: 6.937204, 0.15: 3.557869}


def test_gamma_table_and_round_trip():
    for s, g in GAMMA_TABLE.items():
        assert abs(P.gamma_from_sigma_rel(s) - g) <= 1e-6
        assert abs(R.gamma_root(s) - g) <= 1e-6
    for s in np.linspace(0.01, 0.25, 97):
        g = P.gamma_from_sigma_rel(float(s))
        assert abs(P.sigma_rel_from_gamma(g) - s) <= 1e-12, (s, g)
        assert abs(R.sigma_rel(g) - s) <= 1e-12
    for bad in (0.0, -0.1, 0.2887, 1.0, float("nan")):
        with pytest.raises(ValueError, match="sigma_rel"):
            P.gamma_from_sigma_rel(bad)


@pytest.mark.parametrize("ga,ta,gb,tb", [(16.97, 96, 6.94, 40), (6.94, 4000, 11.24, 4000), (30.3, 7, 3.56, 24)])
def test_profile_dot_against_quadrature(ga, ta, gb, tb):
    want = R.quadrature_dot(ga, ta, gb, tb, points=10 ** 6)
    got = P.profile_dot(ga, ta, gb, tb)
    rel = abs(got - want) / abs(want)
    print(f"profile_dot({ga}, {ta}, {gb}, {tb}) = {got:.15e}, quadrature {want:.15e}, relative {rel:.2e}")
    assert rel <= 1e-9
    assert P.profile_dot(gb, tb, ga, ta) == got                      # symmetric, bit for bit


def test_profile_dot_does_not_overflow():
    v = P.profile_dot(17.0, 1e7, 17.0, 1e7)
    assert math.isfinite(v) and v > 0.0
    assert abs(v - 18.0 * 18.0 / 35.0 / 1e7) <= 1e-12 * v
    assert math.isfinite(P.profile_dot(17.0, 1e7, 3.5, 3.0)) and P.profile_dot(17.0, 1e7, 3.5, 3.0) >= 0.0


def test_power_weight():
    try:
        import mpmath
    except ImportError:
        mpmath = None
    for gamma in (0.0, 3.557869, 16.972199, 9406.0):
        assert P.power_weight(gamma, 1) == 1.0
        last = 1.0
        for t in (2, 3, 7, 100, 4000, 10 ** 7):
            w = P.power_weight(gamma, t)
            if mpmath is not None:
                mpmath.mp.dps = 50
                want = float(1 - (1 - mpmath.mpf(1) / t) ** (mpmath.mpf(gamma) + 1))
            else:
                want = float(R.weight(gamma, t))
            # 1/t, gamma + 1, log1p, their product and expm1 each round once (<= 1 ulp for the two library calls), and w's condition
            # number in the exponent, |a e^a / (1 - e^a)|, is at most 1: below 8 ulp of 1.1e-16 in all
            assert abs(w - want) <= 1e-15 * want, (gamma, t, w, want)
            assert 0.0 < w <= last
            assert w < last or w == 1.0                              # strictly decreasing until it saturates at 1 in double (huge gamma)
            last = w
    with pytest.raises(ValueError):
        P.power_weight(1.0, 0)


def _snapshots(widths, every, total):
    return [(P.gamma_from_sigma_rel(s), t) for t in range(every, total + 1, every) for s in widths]


def test_target_equal_to_a_snapshot_gives_the_unit_vector():
    for every, total in ((32, 512), (2, 24)):
        snaps = _snapshots((0.05, 0.10), every, total)
        for pick in (0, len(snaps) // 2, len(snaps) - 1):
            x = P.solve_weights(snaps, *snaps[pick])
            unit = np.zeros(len(snaps))
            unit[pick] = 1.0
            err = float(np.abs(x - unit).max())
            print(f"every {every} of {total}, snapshot {pick}: max |x - e| = {err:.2e}")
            assert x.dtype == np.float64 and x.shape == (len(snaps),)
            assert err <= 1e-10
            assert P.fit_residual(snaps, *snaps[pick], x) <= 1e-6
    # duplicates make the Gram matrix singular: the two copies share the weight
    x = P.solve_weights([snaps[0], snaps[0], snaps[1]], *snaps[0])
    assert abs(x[0] + x[1] - 1.0) <= 1e-10 and abs(x[2]) <= 1e-10


@pytest.mark.parametrize("every,total,target,bound", [(32, 512, 0.07, 4.0e-3), (32, 512, 0.15, 1.1e-2), (2, 24, 0.07, 2.5e-3)])
def test_reconstructed_profile_is_close_to_the_tracked_one(every, total, target, bound):
    """L1 distance between sum_i x_i (discrete weights of snapshot i) and the discrete weights of the directly tracked target: a bound on
    |reconstruction - tracked average| / max|theta| for ANY trajectory.  Measured by an independent script: 3.59e-3, 9.59e-3, 2.24e-3."""
    snaps = _snapshots((0.05, 0.10), every, total)
    gamma = P.gamma_from_sigma_rel(target)
    x = P.solve_weights(snaps, gamma, total)
    mix = sum(xi * R.discrete_weights(g, t, length=total) for xi, (g, t) in zip(x, snaps))
    want = R.discrete_weights(gamma, total)
    assert abs(want.sum() - 1.0) <= 1e-12                            # the discrete weights of an average sum to 1
    dist = float(np.abs(mix - want).sum())
    print(f"every {every} of {total}, target {target}: L1 = {dist:.3e}, sum x - 1 = {x.sum() - 1.0:.2e}, "
          f"fit residual {P.fit_residual(snaps, gamma, total, x):.3e}")
    assert dist <= bound
    assert abs(x.sum() - 1.0) <= 1e-3


def test_flag_parsing():
    from generative_models_amd import main
    assert P.parse_sigma_rel("") == () and P.parse_sigma_rel("0.05") == (0.05,) and P.parse_sigma_rel("0.05, 0.1,0.25") == (0.05, 0.1, 0.25)
    for bad in ("0.1,0.05", "0.05,0.05", "0.005", "0.26", "0.05,0.06,0.07,0.08", "a,b", "0.05,,0.1"):
        with pytest.raises(ValueError, match="ema_sigma_rel"):
            P.parse_sigma_rel(bad)
    for every in (-1, 2.5, "x"):
        with pytest.raises(ValueError, match="ema_snapshot_every"):
            P.check_flags("0.05", every)
    with pytest.raises(ValueError, match="ema_snapshot_every"):
        P.check_flags("", 4)
    G, Model = main.FlagSpace(main.DG).resolve(["--model=diffusion"])
    assert G.ema_sigma_rel == "" and G.ema_snapshot_every == 0
    G, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--ema_sigma_rel", "0.05,0.1", "--ema_snapshot_every", "16"])
    assert G.ema_sigma_rel == "0.05,0.1" and G.ema_snapshot_every == 16
    main._check_posthoc_flags(G)
    G.ema_sigma_rel = "0.1,0.05"
    with pytest.raises(ValueError, match="ema_sigma_rel"):            # by name, before a model is built
        main._check_posthoc_flags(G)
    with pytest.raises(ValueError, match="ema_sigma_rel"):
        Model(G)


def _write(logdir, step, widths, n, fill=0.0):
    arenas = torch.full((len(widths), n), float(fill))
    return P.write_snapshot(logdir, step, widths, [P.gamma_from_sigma_rel(s) for s in widths], arenas)


def test_snapshot_files_and_refusals(tmp_path):
    path = _write(tmp_path, 7, (0.05, 0.1), 12, fill=2.0)
    assert path == tmp_path / "ema_snapshots" / "step_000000007.pt" and [p.name for p in path.parent.iterdir()] == [path.name]
    rec = torch.load(path, map_location="cpu")
    assert set(rec) == {"step", "sigma_rel", "gamma", "arenas", "layout"}
    assert rec["step"] == 7 and rec["sigma_rel"] == [0.05, 0.1] and rec["arenas"].dtype == torch.float32 and tuple(rec["arenas"].shape) == (2, 12)
    assert rec["layout"] == P.layout_digest(12) != P.layout_digest(13) and 0 <= rec["layout"] < 1 << 64
    _write(tmp_path, 14, (0.05, 0.1), 12, fill=2.0)
    found = P.gather(tmp_path, 0.07)
    assert found["at_step"] == 14 and len(found["rows"]) == 4 and found["snapshots"][-1][1] == 14
    assert len(P.gather(tmp_path, 0.07, at_step=7)["rows"]) == 2 and len(P.gather(tmp_path, 0.07, profiles=(0.1,))["rows"]) == 2
    # a target outside the tracked range widened by 1.5 on each side
    for target in (0.05 / 1.5 - 1e-3, 0.1 * 1.5 + 1e-3):
        with pytest.raises(ValueError, match="sigma_rel"):
            P.gather(tmp_path, target)
    P.gather(tmp_path, 0.1 * 1.5 - 1e-3)
    with pytest.raises(ValueError, match="sigma_rel"):
        P.gather(tmp_path, 0.1, profiles=(0.05,), at_step=7)          # 0.1 > 0.05 * 1.5
    # a snapshot of another arena length
    with pytest.raises(ValueError, match="another shape"):
        P.gather(tmp_path, 0.07, n=13)
    _write(tmp_path, 21, (0.05, 0.1), 16)
    with pytest.raises(ValueError, match="step_000000021.pt.*another shape"):
        P.gather(tmp_path, 0.07)
    assert len(P.gather(tmp_path, 0.07, at_step=14)["rows"]) == 4
    with pytest.raises(ValueError, match="no snapshot"):
        P.gather(tmp_path, 0.07, at_step=3)
    with pytest.raises(ValueError, match="no snapshots"):
        P.gather(tmp_path / "elsewhere", 0.07)


def test_more_than_64_arenas_are_refused(tmp_path):
    for t in range(1, 34):
        _write(tmp_path, t, (0.05, 0.1), 4)
    with pytest.raises(ValueError, match="at_step.*profiles.*stride"):
        P.gather(tmp_path, 0.07)                                      # 66 arenas
    assert len(P.gather(tmp_path, 0.07, at_step=32)["rows"]) == 64
    assert len(P.gather(tmp_path, 0.06, profiles=(0.05,))["rows"]) == 33


def test_flag_unset_changes_nothing_in_the_optimiser():
    from generative_models_amd.diffusion.optim import FusedAdam
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    opt = FusedAdam(SimpleUnet(32))
    assert opt.sigma_rel == () and opt.gamma == () and opt.pema is None
    assert set(opt.state_dict()) == {"step", "m", "v", "lr", "skipped", "ema_seeded"}
    on = FusedAdam(SimpleUnet(32), ema_sigma_rel="0.05,0.1")
    assert on.sigma_rel == (0.05, 0.1) and on.pema is None            # the arena appears with the first step, on the parameters' device
    assert abs(on.gamma[0] - GAMMA_TABLE[0.05]) <= 1e-6 and on.power_weights(1) == [1.0, 1.0]
    sd = on.state_dict()
    assert set(sd) == {"step", "m", "v", "lr", "skipped", "ema_seeded", "pema", "pema_sigma_rel"} and sd["pema"] is None
    with pytest.raises(ValueError, match="ema_sigma_rel"):
        on.load_state_dict(opt.state_dict())                          # a state saved without the averages
    with pytest.raises(ValueError, match="ema_sigma_rel"):
        FusedAdam(SimpleUnet(32), ema_sigma_rel="0.1,0.05")
