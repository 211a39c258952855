"""Host checks of tests/gn_ref.py: the float64 GroupNorm + SiLU reference against torch's own group_norm in double and against central
differences; the bars of tests/test_gpu_gn_conformance.py on an fp32 restatement of the kernels' arithmetic - they pass it as it is and
fail it with the faults they are there for; and the case tables against the host dispatch of csrc/gn_silu.hip: every kernel instantiation the
file holds is launched by some case, and each case reports the kernel id the table says."""
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_ref as R  # noqa: E402
import philox_ref  # noqa: E402


def _tiny(seed=0, B=2, S=3, C=8):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.randn(shape, generator=g, dtype=torch.float64)
    return dict(x=rnd(B, S, S, C) * 1.5 + 0.3, gamma=1 + 0.2 * rnd(C), beta=0.1 * rnd(C), xadd=0.5 * rnd(B, C), dy=rnd(B, S, S, C),
                dadd1=rnd(B, S, S, C), dadd2=rnd(B, S, S, C))


def _torch_gn(t, groups, xadd, eps=R.eps32(R.EPS)):
    """silu(group_norm(x + xadd)) by torch in double with autograd -> (y NHWC, leaves x, gamma, beta)"""
    x, gamma, beta = (t[k].clone().requires_grad_(True) for k in ("x", "gamma", "beta"))
    xin = x if xadd is None else x + xadd[:, None, None, :]
    y = F.silu(F.group_norm(xin.permute(0, 3, 1, 2), groups, gamma, beta, eps)).permute(0, 2, 3, 1)
    return y, x, gamma, beta


@pytest.mark.parametrize("with_xadd", [False, True])
@pytest.mark.parametrize("groups", [2, 4, 8])
def test_reference_equals_torch_in_double(groups, with_xadd):
    t = _tiny(groups)
    xadd = t["xadd"] if with_xadd else None
    y, x, gamma, beta = _torch_gn(t, groups, xadd)
    y.backward(t["dy"])
    y64, mean, rstd = R.forward64(t["x"], t["gamma"], t["beta"], groups, xadd=xadd)
    assert float((y64 - y.detach()).abs().max()) < 1e-12
    xin = (t["x"] if xadd is None else t["x"] + xadd[:, None, None, :]).reshape(2, 9, groups, 8 // groups)
    assert float((mean - xin.mean((1, 3))).abs().max()) < 1e-12
    assert float((rstd - 1 / torch.sqrt(xin.var((1, 3), unbiased=False) + R.eps32(R.EPS))).abs().max()) < 1e-12
    dx, dgp, dbp, dxsum = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], groups, xadd=xadd, dadd1=t["dadd1"], dadd2=t["dadd2"])
    assert float((dx - (x.grad + t["dadd1"] + t["dadd2"])).abs().max()) < 1e-12
    assert dgp.shape == dbp.shape == (2, 8)
    assert float((dgp.sum(0) - gamma.grad).abs().max()) < 1e-12 and float((dbp.sum(0) - beta.grad).abs().max()) < 1e-12      # the partials sum to the gradient
    assert float((dxsum - dx.sum((1, 2))).abs().max()) < 1e-12
    only = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], groups, xadd=xadd, dadd1=t["dadd1"])[0]
    assert float((only - (x.grad + t["dadd1"])).abs().max()) < 1e-12
    # the tables are the affine form of the same normalisation
    scale, shift = R.tables64(t["x"], t["gamma"], t["beta"], groups, xadd=xadd)
    gq = t["x"] * scale[:, None, None, :] + shift[:, None, None, :]
    assert float((gq * torch.sigmoid(gq) - y64).abs().max()) < 1e-12


def test_dx_equals_central_differences():
    t = _tiny(5, B=2, S=2, C=8)
    groups, xadd = 2, t["xadd"]
    L = lambda x: float((R.forward64(x, t["gamma"], t["beta"], groups, xadd=xadd)[0] * t["dy"]).sum())
    dx = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], groups, xadd=xadd)[0]
    h = 1e-5
    fd = torch.empty_like(dx)
    for i in range(dx.numel()):
        e = torch.zeros(dx.numel(), dtype=torch.float64); e[i] = h
        e = e.view_as(dx)
        fd.view(-1)[i] = (L(t["x"] + e) - L(t["x"] - e)) / (2 * h)
    assert float((fd - dx).abs().max()) < 1e-8 * float(dx.abs().max())


def test_dropout_factors_are_the_philox_stream():
    shape, p = (2, 3, 3, 8), 0.2
    f = R.dropout_factor(shape, p, R.SEED, R.OFFSET)
    u = philox_ref.uniform(R.SEED, R.OFFSET, 144).reshape(shape)
    keep = u >= np.float32(p)
    assert 0 < keep.sum() < keep.size and np.array_equal(keep, philox_ref.keep_mask(R.SEED, R.OFFSET, 144, p).reshape(shape))
    assert np.array_equal(f.numpy() != 0, keep) and np.allclose(f.numpy()[keep], 1 / (1 - float(np.float32(p))), rtol=0, atol=1e-15)
    assert torch.equal(R.dropout_factor(shape, 0.0, 1, 2), torch.ones(shape, dtype=torch.float64))
    t = _tiny(2)
    plain = R.forward64(t["x"], t["gamma"], t["beta"], 2)[0]
    assert torch.equal(R.forward64(t["x"], t["gamma"], t["beta"], 2, dropout=(p, R.SEED, R.OFFSET))[0], plain * f)
    # the backward masks dy with the same factors
    a = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], 2, dropout=(p, R.SEED, R.OFFSET))
    b = R.backward64(t["dy"] * f, t["x"], t["gamma"], t["beta"], 2)
    assert all(torch.equal(u_, v_) for u_, v_ in zip(a, b))


def test_explicit_group_size_is_group_norm_on_the_real_channels():
    """groups = -3 at 16 channels: GroupNorm(4, 12) on the 12 real channels, two padding groups (one whole, one partial) that stay zero"""
    t = _tiny(3, B=2, S=3, C=16)
    live = torch.zeros(16, dtype=torch.float64); live[:12] = 1
    for k in ("x", "gamma", "beta", "xadd", "dy"):
        t[k] = t[k] * live
    real = {k: v[..., :12] for k, v in t.items()}
    y, x, gamma, beta = _torch_gn(real, 4, real["xadd"])
    y.backward(real["dy"])
    y64, mean, rstd = R.forward64(t["x"], t["gamma"], t["beta"], -3, xadd=t["xadd"])
    assert mean.shape == (2, 6) and float((y64[..., :12] - y.detach()).abs().max()) < 1e-12 and float(y64[..., 12:].abs().max()) == 0
    assert float(mean[:, 4:].abs().max()) == 0 and float((rstd[:, 4:] - R.eps32(R.EPS) ** -0.5).abs().max()) < 1e-9
    dx, dgp, dbp, _ = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], -3, xadd=t["xadd"])
    assert float((dx[..., :12] - x.grad).abs().max()) < 1e-12 and float(dx[..., 12:].abs().max()) == 0
    assert float((dgp.sum(0)[:12] - gamma.grad).abs().max()) < 1e-12 and float((dbp.sum(0)[:12] - beta.grad).abs().max()) < 1e-12


def test_pair_reference_is_the_documented_composite():
    t, u = _tiny(7), _tiny(8)
    up = (u["dy"].bfloat16(), u["dadd1"].bfloat16(), u["gamma"], u["beta"], 2)
    dn = (t["dy"].bfloat16(), t["dadd1"].bfloat16(), t["gamma"], t["beta"], 4)
    dx, dxsum, (dgu, dbu), (dgd, dbd) = R.pair_backward64(t["x"], up, dn, xadd=t["xadd"])
    ds = R.backward64(up[0], t["x"], up[2], up[3], 2, xadd=t["xadd"], dadd1=up[1])
    down = R.backward64(dn[0], t["x"], dn[2], dn[3], 4, xadd=t["xadd"], dadd1=dn[1])
    assert torch.equal(dx, down[0] + ds[0].bfloat16().double()) and torch.equal(dxsum, dx.sum((1, 2)))
    assert torch.equal(dgu, ds[1]) and torch.equal(dbu, ds[2]) and torch.equal(dgd, down[1]) and torch.equal(dbd, down[2])


def test_worst_names_sample_slab_group_pixel_and_plane():
    ref = torch.ones((3, 15, 15, 128), dtype=torch.float64)
    got = ref.clone()
    got[1, 13, 2, 70] += 0.25                     # pixel 197 of 225: at 4 pixels per thread, 57 planes -> plane 26, iteration 3
    got[2, 0, 0, 3] += 0.125
    w = R.worst(got, ref, it=4, groups=32)
    assert w["err"].shape == (3, 4) and float(w["err"][1, 2]) == 0.25 and float(w["err"][2, 0]) == 0.125 and float(w["err"].sum()) == 0.375
    assert w["at"] == (1, 2, 70, 197)
    for part in ("sample 1", "slab 2", "group 17", "pixel 197 of 225", "plane 26 of 57", "iteration 3 of 4"):
        assert part in w["text"], (part, w["text"])
    assert "plane 5 of 64, iteration 3" in R.worst(got, ref, it=4, groups=32, planes=64)["text"]
    got[0, 0, 0, 0] = float("nan")                # a NaN is the worst element, not an ignored one
    assert float(R.worst(got, ref)["err"][0, 0]) == float("inf")
    x = torch.randn((2, 4, 4, 64), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert torch.equal(R.rms_ratio(x.bfloat16(), x, torch.bfloat16), torch.ones(2, 2, dtype=torch.float64))
    z = torch.zeros((1, 2, 2, 32), dtype=torch.float64)
    assert float(R.rms_ratio(z, z, torch.bfloat16)) == 0 and float(R.rms_ratio(z + 1, z, torch.bfloat16)) == float("inf")
    assert R.rows_err(torch.tensor([[1.0, 2.0], [3.0, float("nan")]]), torch.tensor([[1.0, 4.0], [3.0, 3.0]])).tolist() == [0.5, float("inf")]


# ---- what the bars see ---------------------------------------------------------------------------------------------------------------
def _problem(S, dtype, C=128, G=32, B=3):
    c = R._c("gn_silu_bwd", S, C, G, R.BF16, R.K_BWD, x_dtype=dtype, B=B)
    return c, R.make_inputs(c, seed=S)


@pytest.mark.parametrize("S", [14, 28, 32])
@pytest.mark.parametrize("dtype", [R.BF16, R.F16])
def test_rstd_fault_passes_the_global_bar_and_breaks_the_slab_bound(S, dtype):
    """One group's rstd wrong by 2^-9 in y: inside the whole-tensor 1e-2 max-norm bar of test_gn_silu_fwd_bwd, outside A.2 on its (sample,
    slab) - and only there; the unmodified chain measures 1.000."""
    c, t = _problem(S, dtype, B=2 if S > 14 else 3)
    dt = R.TORCH[dtype]
    y64 = R.forward64(t["x"], t["gamma"], t["beta"], c.G)[0]
    good = R.restate32(t["x"], t["gamma"], t["beta"], c.G)["y"].to(dt)
    bad = R.restate32(t["x"], t["gamma"], t["beta"], c.G, rstd_fault=(1, 9, 1 + 2.0 ** -9))["y"].to(dt)      # group 9: channels 36..39, slab 1
    assert float((bad.double() - y64).abs().max() / y64.abs().max()) < 1e-2
    ratios = R.rms_ratio(bad, y64, dt)
    assert float(ratios[1, 1]) > R.SHARP, ratios
    ratios[1, 1] = 0
    assert float(ratios.max()) < 1.001 and float(R.rms_ratio(good, y64, dt).max()) < 1.001
    with pytest.raises(AssertionError, match="sample 1 slab 1"):
        R.check_a(bad, y64, dt, "planted", True, groups=c.G)


@pytest.mark.parametrize("S", [14, 28, 32])
def test_dropped_pixel_breaks_the_partials_bar(S):
    """One pixel missing from one channel's dgamma partial: the largest such term of the sample moves its entry by more than 1e-4 of the
    sample's largest partial (and by less than the 1e-2 that was asked of the batch sum)."""
    c, t = _problem(S, R.F16, B=2 if S > 14 else 3)
    ref = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], c.G)
    good = R.restate32(t["x"], t["gamma"], t["beta"], c.G, dy=t["dy"])
    assert R.check_rows(good["dgp"], ref[1], "dgamma_part") < 2e-6
    hit = 0
    for p in range(0, S * S, max(1, S * S // 16)):
        bad = R.restate32(t["x"], t["gamma"], t["beta"], c.G, dy=t["dy"], drop_pixel=(1, 40, p))
        e = R.rows_err(bad["dgp"], ref[1])
        assert float(e[0]) < 2e-6 and float(e[1]) < 1e-1
        hit += float(e[1]) >= R.PART_BAR
    assert hit >= 12, hit                  # (a pixel whose term happens to be tiny is no fault the sums can show)
    with pytest.raises(AssertionError, match="sample 1, channel 40"):
        R.check_rows(bad["dgp"], ref[1], "planted")


_CPU_CASES = [c for c in R.FORWARD + R.BACKWARD if not c.stats]          # (the producer-statistics row needs the convolution that emits them)
_STATS_IDS = {R.ident(c) for c in R.STATS}


def test_unmodified_restatement_passes_every_bar():
    """The fp32 chain as the kernels state it, stored by one rounding: A.1, A.2 (centred 16-bit cases) and B on every case of the tables, the
    gmk_gn_stats tables and the pairs included.  The figures printed are the floor the kernels are measured against."""
    top = {}
    note = lambda k, v: top.__setitem__(k, max(top.get(k, 0.0), v))
    for c in _CPU_CASES:
        t = R.make_inputs(c)
        what = R.ident(c)
        drop = (c.p, R.SEED, R.OFFSET) if c.p else None
        dt, gdt = R.TORCH[c.x_dtype], R.TORCH[c.dtype]
        if c.entry == "gn_silu_fwd":
            got = R.restate32(t["x"], t["gamma"], t["beta"], c.G, xadd=t["xadd"], dropout=drop)
            y64 = R.forward64(t["x"], t["gamma"], t["beta"], c.G, xadd=t["xadd"], dropout=drop)[0]
            a1, a2 = R.check_a(got["y"].to(dt), y64, dt, what + " y", not c.offset, groups=c.G)
            qm, qr = R.check_stats(got["mean"], got["rstd"], t["x"], c.G, what, xadd=t["xadd"])
            note("stats / bound", max(qm, qr))
            if what in _STATS_IDS:          # the gmk_gn_stats tables of the same chain
                sc = got["rstd"].repeat_interleave(c.C // c.G, 1) * t["gamma"]
                add = t["xadd"] if t["xadd"] is not None else torch.zeros(c.B, c.C)
                sh = t["beta"] + (add - got["mean"].repeat_interleave(c.C // c.G, 1)) * sc
                note("tables / bound", max(R.check_tables(sc, sh, t["x"], t["gamma"], t["beta"], c.G, what + " table", xadd=t["xadd"])))
        else:
            adds = [t["dadd"], t["dadd2"]][:c.dadd]
            kw = dict(xadd=t["xadd"], dropout=drop, dadd1=adds[0] if adds else None, dadd2=adds[1] if len(adds) > 1 else None)
            got = R.restate32(t["x"], t["gamma"], t["beta"], c.G, dy=t["dy"], **kw)
            dx, dgp, dbp, dxsum = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], c.G, **kw)
            a1, a2 = R.check_a(got["dx"].to(gdt), dx, gdt, what + " dx", not c.offset, groups=c.G)
            for name, g_, r_ in (("dgamma_part", got["dgp"], dgp), ("dbeta_part", got["dbp"], dbp), ("dxsum", got["dxsum"], dxsum)):
                note("partials", R.check_rows(g_, r_, f"{what} {name}"))
        note("A.1", a1)
        if a2 is not None:
            note("A.2", a2)
    for c in R.PAIRS:
        t = R.make_inputs(c)
        what, dt = R.ident(c), R.TORCH[c.x_dtype]
        if c.entry == "gn_silu_fwd_pair":
            for k, G in (("", c.G), ("2", c.G2)):
                got = R.restate32(t["x"], t["gamma" + k], t["beta" + k], G, xadd=t["xadd"])
                y64 = R.forward64(t["x"], t["gamma" + k], t["beta" + k], G, xadd=t["xadd"])[0]
                note("A.2", R.check_a(got["y"].to(dt), y64, dt, f"{what} y{k}", True, groups=G)[1])
                note("stats / bound", max(R.check_stats(got["mean"], got["rstd"], t["x"], G, what, xadd=t["xadd"])))
        else:                               # the composite: the up consumer's input gradient stored in bf16 on the way
            up = R.restate32(t["x"], t["gamma"], t["beta"], c.G, xadd=t["xadd"], dy=t["dy"], dadd1=t["dadd"])
            dn = R.restate32(t["x"], t["gamma2"], t["beta2"], c.G2, xadd=t["xadd"], dy=t["dy2"], dadd1=t["dadd2"], dadd2=up["dx"].bfloat16())
            dx, dxsum, (gu, bu), (gd, bd) = R.pair_backward64(t["x"], (t["dy"], t["dadd"], t["gamma"], t["beta"], c.G),
                                                              (t["dy2"], t["dadd2"], t["gamma2"], t["beta2"], c.G2), xadd=t["xadd"])
            note("A.2", R.check_a(dn["dx"].bfloat16(), dx, torch.bfloat16, what + " dx", True, groups=c.G2)[1])
            for name, g_, r_ in (("dgamma_part up", up["dgp"], gu), ("dbeta_part up", up["dbp"], bu), ("dgamma_part", dn["dgp"], gd), ("dbeta_part", dn["dbp"], bd)):
                note("partials", R.check_rows(g_, r_, f"{what} {name}"))
            # (5e-5 at 32 x 32, two hundred times the single backward's: bf16(ds) of an fp32 and of a float64 chain part ways at a few ties of
            # the rounding, and one such step of 2^-7 is 5e-5 of the largest channel sum - the kernels measure the same figure)
            note("pair dxsum", R.check_rows(dn["dxsum"], dxsum, what + " dxsum"))
    print("restatement:", {k: f"{v:.3e}" for k, v in top.items()})
    assert top["A.2"] < 1.01 and top["partials"] < 2e-5 and top["stats / bound"] < 0.5 and top["tables / bound"] < 0.5, top


# ---- the case tables against the dispatch ------------------------------------------------------------------------------------------------
def test_case_tables_reach_every_instantiation():
    """The case tables through the host dispatch of csrc/gn_silu.hip (tools/gn_launch_trace.cpp `cases`, no GPU): each call succeeds, launches
    exactly one kernel and reports the id its row stores; and the kernels launched are ALL the gn_silu_* kernels of the code object - a
    new instantiation without a conformance case fails here."""
    import launch_trace
    run = launch_trace.build("gn_launch_trace", ("gn_silu", "gmk_common"))
    symbols = set(re.findall(r"\.name:\s+(\S*gn_silu_\S+)", open(run.notes).read()))
    assert len(symbols) >= 49 and all(s.startswith("_Z") for s in symbols), sorted(symbols)[:3]
    ids = [R.ident(c) + c.entry for c in R.CASES]
    assert len(set(ids)) == len(ids)
    lines = run("cases", stdin="".join(R.trace_line(c) + "\n" for c in R.CASES))
    assert len(lines) == len(R.CASES)
    launched = {}
    for c, line in zip(R.CASES, lines):
        head, _, tail = line.partition(" -> ")
        assert head.startswith(c.entry + " ") and f" HW={c.S * c.S} C={c.C} G={c.G},{c.G2} " in head, (R.ident(c), line[:300])
        names = re.findall(r" launch=(\S+)", tail)
        kid = int(re.findall(r'" kernel=(-?\d+)', tail)[-1])
        assert tail.startswith('rc=0 err="" ') and len(names) == 1, (R.ident(c), line[:400])
        assert kid == c.kernel, (R.ident(c), c.kernel, line[:400])
        launched.setdefault(names[0], R.ident(c))
        form = R.pixel_form(c)              # the mirror the error texts use: <type, pixels per thread, vectors | threads, vectors>
        m = re.search(r"(?:fwd_reg|fwd_pair|bwd_hybrid|bwd_pair)_kernelIDF16[_b]Li(\d+)ELi(\d+)E(?:Li(\d+)E)?", names[0])
        assert (form is None) == (m is None), (R.ident(c), names[0])
        if m and "fwd" in m.group(0):
            assert form == (int(m.group(1)), -(-c.S * c.S // int(m.group(1)))), (R.ident(c), form, names[0])
        elif m:
            nvec = 4 if "pair" in m.group(0) else int(m.group(3))
            assert form == (int(m.group(1)), int(m.group(2)) // nvec), (R.ident(c), form, names[0])
    assert set(launched) <= symbols
    assert not symbols - set(launched), f"kernel instantiations no conformance case reaches: {sorted(symbols - set(launched))}"
    # what the issue's table promises of single rows
    first = lambda frag: next((v for k, v in launched.items() if frag in k), None)
    assert "m6" in first("fwd_reg_kernelIDF16_Li1ELi8E") and "m5" in first("fwd_reg_kernelIDF16_Li8ELi4E") and first("fwd_reg_kernelIDF16_Li16ELi4E").startswith("48x48")
    assert first("bwd_hybrid_kernelIDF16_Li8ELi1024ELi2E") and first("bwd_hybrid_kernelIDF16bLi32ELi512ELi4ELi28ELi13E")


def test_trace_tool_keeps_its_other_modes():
    """`cases` is an addition: an empty table prints nothing, the landmark rows are still there"""
    import launch_trace
    run = launch_trace.build("gn_launch_trace", ("gn_silu", "gmk_common"))
    assert run("cases", stdin="") == []
    assert len(run("landmarks")) > 20
