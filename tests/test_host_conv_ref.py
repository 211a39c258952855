"""Host checks of tests/conv_ref.py: the float64 convolution reference against itself (finite differences, the adjoint identity, the
nearest-x2 identity), the planner mirrors against the library's own planners, and the case tables of
tests/test_gpu_conv_wide.py against the branches those planners have - the tables may not quietly lose one."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [R.NORMAL, R.STRIDE2, R.UPSAMPLE2, R.TRANSPOSED2]


def _problem(mode, seed=0):
    """2 x 4 x 6 x 5 sources in two halves, 3 output channels (for TRANSPOSED2: the gradient of a 3-channel 12 x 10 stride-2 convolution's output)"""
    g = torch.Generator().manual_seed(seed)
    B, C, H, W, Co = 2, 4, 6, 5, 3
    srcs = [torch.randn((B, C // 2, H, W), generator=g, dtype=torch.float64) for _ in range(2)]
    w = torch.randn((C, Co, 3, 3) if mode == R.TRANSPOSED2 else (Co, C, 3, 3), generator=g, dtype=torch.float64)
    y = R.conv_ref64(mode, srcs, w)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    return srcs, w, y, dy


@pytest.mark.parametrize("mode", MODES)
def test_output_sizes_and_epilogue(mode):
    srcs, w, y, _ = _problem(mode)
    want = {R.NORMAL: (6, 5), R.STRIDE2: (3, 3), R.UPSAMPLE2: (12, 10), R.TRANSPOSED2: (12, 10)}[mode]
    assert y.shape == (2, 3, *want) and y.dtype == torch.float64
    g = torch.Generator().manual_seed(9)
    bias, emb = torch.randn(3, generator=g), torch.randn((2, 3), generator=g)
    res = torch.randn(y.shape, generator=g)
    full = R.conv_ref64(mode, srcs, w, bias=bias, emb=emb, residual=res)
    assert torch.equal(full, y + bias.double()[None, :, None, None] + emb.double()[:, :, None, None] + res.double())


@pytest.mark.parametrize("mode", MODES)
def test_grads64_equal_finite_differences_of_conv_ref64(mode):
    """Every element of every gradient: central differences of L = sum(conv_ref64 * dy) in double (L is linear in each operand, so the
    quotient is exact up to rounding: 1e-9 of the gradient's scale)."""
    srcs, w, _, dy = _problem(mode, seed=mode + 1)
    dsrcs, dw = R.grads64(mode, srcs, w, dy)
    L = lambda s, ww: float((R.conv_ref64(mode, s, ww) * dy).sum())
    h = 0.5
    for k, (s, ds) in enumerate(zip(srcs, dsrcs)):
        fd = torch.empty_like(s)
        for i in range(s.numel()):
            e = torch.zeros(s.numel(), dtype=torch.float64); e[i] = h
            e = e.view_as(s)
            up = [t + e if j == k else t for j, t in enumerate(srcs)]
            dn = [t - e if j == k else t for j, t in enumerate(srcs)]
            fd.view(-1)[i] = (L(up, w) - L(dn, w)) / (2 * h)
        assert float((fd - ds).abs().max()) < 1e-9 * float(ds.abs().max()), f"source {k}"
    fd = torch.empty_like(w)
    for i in range(w.numel()):
        e = torch.zeros(w.numel(), dtype=torch.float64); e[i] = h
        e = e.view_as(w)
        fd.view(-1)[i] = (L(srcs, w + e) - L(srcs, w - e)) / (2 * h)
    assert float((fd - dw).abs().max()) < 1e-9 * float(dw.abs().max())


def test_transposed_is_the_data_gradient_of_stride2():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 4, 12, 10), generator=g, dtype=torch.float64)
    w = torch.randn((3, 4, 3, 3), generator=g, dtype=torch.float64)
    dy = torch.randn((2, 3, 6, 5), generator=g, dtype=torch.float64)
    (dx,), _ = R.grads64(R.STRIDE2, [x], w, dy)
    t = R.conv_ref64(R.TRANSPOSED2, [dy], w)
    assert t.shape == dx.shape and float((t - dx).abs().max()) < 1e-12 * float(dx.abs().max())
    # and its own gradients close the circle: d/d(dy) of <transposed(dy), x> is the stride-2 convolution of x
    (ddy,), _ = R.grads64(R.TRANSPOSED2, [dy], w, x)
    assert float((ddy - R.conv_ref64(R.STRIDE2, [x], w)).abs().max()) < 1e-12 * float(ddy.abs().max())


def test_upsample_is_conv_of_interpolate_and_pools_its_gradient():
    g = torch.Generator().manual_seed(6)
    x = torch.randn((2, 4, 6, 5), generator=g, dtype=torch.float64)
    w = torch.randn((3, 4, 3, 3), generator=g, dtype=torch.float64)
    up = F.interpolate(x, scale_factor=2, mode="nearest")
    assert torch.equal(up[:, :, 1::2, 0::2], x)
    assert torch.equal(R.conv_ref64(R.UPSAMPLE2, [x], w), F.conv2d(up, w, None, padding=1))
    dy = torch.randn((2, 3, 12, 10), generator=g, dtype=torch.float64)
    (dx,), dw = R.grads64(R.UPSAMPLE2, [x], w, dy)
    (dup,), dwn = R.grads64(R.NORMAL, [up], w, dy)
    assert float((dx - F.avg_pool2d(dup, 2) * 4).abs().max()) < 1e-12 * float(dx.abs().max())
    assert float((dw - dwn).abs().max()) < 1e-12 * float(dw.abs().max())


def test_worst_names_block_tile_and_row():
    ref = torch.ones((3, 256, 28, 28), dtype=torch.float64)
    got = ref.clone()
    got[1, 200, 5, 7] += 0.25                       # global row 33 of 84, R = 9: tile 3, row 6
    got[2, 3, 0, 0] += 0.125
    r = R.worst(got, ref, cu_limit=8)
    assert r["err"] == [0.125, 0.25] and r["at"] == (1, 5, 7, 200) and (r["tile"], r["row"]) == (3, 6)
    assert "channel block 1" in r["text"] and "tile 3 of 10 row 6 of R=9" in r["text"] and "half_tail" in r["text"]
    got[0, 0, 0, 0] = float("nan")                  # a NaN is the worst element, not an ignored one
    assert R.worst(got, ref)["err"][0] == float("inf")
    x = torch.randn((2, 256, 4, 4), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    assert R.rms_ratio(x.bfloat16(), x, torch.bfloat16) == [1.0, 1.0]
    errs, text = R.worst_w(torch.ones(256, 512, 3, 3), torch.ones(256, 512, 3, 3))
    assert errs == [[0.0] * 4, [0.0] * 4]


def test_rms_ratio_separates_one_rounding_from_two():
    """What the sharp bound of test_gpu_conv_wide.py (rms error <= 1.05 x the rms error of rounding the float64 result) can see, on a
    512 -> 128 3x3 (K = 4608) in bf16: one rounding of an fp32-accumulated sum passes at 1.00; a second rounding on the way (the sum stored
    in bf16 before the residual is added) and one missing term of the 4608 both fail it - the first of them far inside the 1e-2 max-norm bar."""
    g = torch.Generator().manual_seed(11)
    bf = torch.bfloat16
    x = torch.randn((2, 512, 8, 8), generator=g).to(bf).double()
    w = (torch.randn((128, 512, 3, 3), generator=g) / 4608 ** 0.5).to(bf).double()
    res = torch.randn((2, 128, 8, 8), generator=g).to(bf).double()
    conv = R.conv_ref64(R.NORMAL, [x], w)
    ref = conv + res
    once = (conv.float() + res.float()).to(bf)                              # fp32 sum, one rounding
    twice = (conv.float().to(bf).float() + res.float()).to(bf)
    w1 = w.clone(); w1[:, 300, 1, 2] = 0
    dropped = (R.conv_ref64(R.NORMAL, [x], w1).float() + res.float()).to(bf)
    (r1,), (r2,), (r3,) = (R.rms_ratio(t, ref, bf) for t in (once, twice, dropped))
    assert 0.999 < r1 < 1.001, r1
    assert r2 > 1.05 and max(R.worst(twice, ref)["err"]) < 1e-2, (r2, R.worst(twice, ref)["err"])
    assert r3 > 1.05, r3


# ---- the planners ------------------------------------------------------------------------------------------------------------------
# (variant, fold) -> (no half-job tail, no all-half form): variant 4 counts for the plain launch only, 6 switches both off, 8 the all-half form
_NO_HALF = {(0, 0): (False, False), (4, 0): (True, True), (6, 0): (True, True), (8, 0): (False, True),
            (0, 1): (False, False), (4, 1): (False, False), (6, 1): (True, True), (8, 1): (False, True)}


def _planner_cases():
    """(halo cases (B, H, W, limit, variant, fold), slot cases (B, H, W, cout, ktot, stride2, limit, forced)): the case tables at their limits, every
    small grid and the widest ones at four batch sizes under the three CU limits, one small problem under every CU limit; the variants that
    switch half jobs off, for the plain launch and the fold, and the automatic choice's work floor over the case tables"""
    grids = [(B, H, W, lim) for H in range(2, 67) for W in list(range(2, 67)) + [126, 127, 128, 254, 255] for B in (1, 3, 9, 37) for lim in (8, 248, 256)]
    table = [(B, H, W, lim) for (H, W, B, lim) in R.TABLE]
    halo = [c + (0, 0) for c in table + grids] + [c + vf for c in table + [(3, 32, 32, 8)] for vf in _NO_HALF if vf != (0, 0)]
    stable = [(B, H, W, lim) for (H, W, B, lim) in R.SLOT_TABLE]
    slot = [(B, H, W, 256, ktot, s2, lim, 1) for (B, H, W, lim) in stable + grids for ktot in (256, 512) for s2 in (0, 1)]
    # the XCD rounding over every split count a CU limit can give (128 x 64: up to 128 splits; `& ~7` and `& ~3` part ways from 68 on)
    slot += [(9, 16, 16, 128, 64, s2, lim, 1) for lim in range(8, 257) for s2 in (0, 1)]
    slot += [(B, H, W, 256, ktot, s2, lim, 0) for (B, H, W, lim) in stable for ktot in (256, 512) for s2 in (0, 1)]
    return halo, slot


def test_planner_mirrors_restate_the_library():
    """halo_plan / slot_plan against the planners of csrc/conv_plan.h themselves (tools/conv_launch_trace.cpp `plans`, the host objects of the
    tree without a GPU): every field both sides have, over a set that holds both sides of every rule the mirrors restate."""
    halo, slot = _planner_cases()
    # the set itself, on the mirror alone: both sides of the halo-slot capacity edge (ner * (W + 2) = 448 at 7 x 6, 496 at 5 x 6), the
    # `2 rem == G` edge of the tail rule, all four schedules; both windows, both answers of the automatic choice, the XCD rounding
    assert (1, 7, 6, 8, 0, 0) in halo and (1, 5, 6, 8, 0, 0) in halo
    assert R.halo_plan(1, 7, 6, 8)["eligible"] and not R.halo_plan(1, 5, 6, 8)["eligible"]
    assert 256 // 6 + 2 + 2 * R.halo_plan(1, 7, 6, 8)["crossings"] == R.HALO_SLOTS // 8 and (256 // 6 + 2 + 2 * R.halo_plan(1, 5, 6, 8)["crossings"]) * 8 == 496
    mirrors = [R.halo_plan(*c[:4], *_NO_HALF[c[4:]]) for c in halo]
    ok = [p for p in mirrors if p["eligible"]]
    for vf, flags in _NO_HALF.items():          # every exclusion changes some schedule of the set
        assert not any(flags) or any(R.halo_plan(*c[:4], *flags) != R.halo_plan(*c[:4]) for c in halo if c[4:] == vf), vf
    assert {p["schedule"] for p in ok} == {"all_half", "whole_rounds", "half_tail", "whole_partial"}
    assert any(p["schedule"] == "half_tail" and 2 * (p["ntiles"] % p["grid"]) == p["grid"] for p in ok)
    assert any(2 * p["ntiles"] == lim for p, (_, _, _, lim, _, _) in zip(mirrors, halo) if p["eligible"])          # the `<=` of the all-half rule
    assert any(not p["eligible"] and "R" in p for p in mirrors) and any("R" not in p for p in mirrors)
    smirrors = [R.slot_plan(B, H, W, cout, ktot, stride2=bool(s2), cu_limit=lim) for (B, H, W, cout, ktot, s2, lim, _) in slot]
    sok = [p for p in smirrors if p["eligible"]]
    assert {p["wide"] for p in sok} == {False, True} and {p["auto"] for p in sok} == {False, True}
    assert {1, 7, 8, 12, 16, 64, 68, 72} <= {p["ns3_plan"] for p in sok} and any(p["ns3"] < p["ns3_plan"] for p in sok)
    assert any(p["nchunks"] == 8 * (248 // 8) for p in sok)                                                # the `<` of the automatic choice, at 31 splits

    import launch_trace
    run = launch_trace.build("conv_launch_trace", launch_trace.CONV_SOURCES)
    text = "".join("halo %d %d %d %d %d %d\n" % c for c in halo) + "".join("slot %d %d %d %d %d %d %d %d\n" % c for c in slot)
    lines = run("plans", stdin=text)
    assert len(lines) == len(halo) + len(slot)
    fields = lambda line: {k: v for k, v in (kv.split("=", 1) for kv in line.split()[1:])}
    for case, want, line in zip(halo, mirrors, lines):
        got = fields(line)
        assert line.startswith("halo ") and tuple(int(got[k]) for k in ("B", "H", "W", "cu", "variant", "fold")) == case
        assert bool(int(got["eligible"])) == want["eligible"], (case, line)
        if want["eligible"]:
            mine = (want["R"], want["ntiles"], want["rows"], want["nfull"], want["nhalf"], want["grid"])
            assert tuple(int(got[k]) for k in ("R", "ntiles", "rows", "nfull", "nhalf", "grid")) == mine, (case, want, line)
    for case, want, line in zip(slot, smirrors, lines[len(halo):]):
        got = fields(line)
        assert line.startswith("slot ") and tuple(int(got[k]) for k in ("B", "H", "W", "cout", "ktot", "stride2", "cu", "forced")) == case
        assert bool(int(got["eligible"])) == (want["eligible"] and (case[-1] != 0 or want["auto"])), (case, line)      # forced 0: the work floor decides too
        if int(got["eligible"]):
            mine = (want["wide"], want["nchunks"], want["auto"], want["ns3_plan"], want["ns3"], want["grid"])
            theirs = (bool(int(got["wide"])), int(got["nchunks"]), bool(int(got["auto"])), int(got["ns_cu"]), int(got["ns"]), tuple(int(v) for v in got["grid"].split(",")))
            assert theirs == mine, (case, want, line)


def test_halo_plan_by_hand():
    """The schedules of the issue's shape table, worked by hand from the rule (limit 8 unless stated)."""
    want = {(16, 16, 3, 8): (16, 3, False, "all_half"), (16, 16, 8, 8): (16, 8, False, "whole_rounds"), (16, 16, 9, 8): (16, 9, False, "half_tail"),
            (16, 16, 13, 8): (16, 13, False, "whole_partial"), (28, 28, 3, 8): (9, 10, True, "half_tail"), (14, 14, 12, 8): (18, 10, True, "half_tail"),
            (8, 8, 37, 8): (32, 10, True, "half_tail"), (32, 32, 3, 8): (8, 12, False, "half_tail"), (64, 64, 1, 8): (4, 16, False, "whole_rounds"),
            (12, 20, 9, 8): (12, 9, False, "half_tail"), (10, 24, 9, 8): (10, 9, False, "half_tail"), (20, 12, 5, 8): (21, 5, True, "whole_rounds"),
            (16, 16, 5, 256): (16, 5, False, "all_half"), (28, 28, 2, 256): (9, 7, True, "all_half"), (16, 16, 9, 248): (16, 9, False, "all_half")}
    assert set(want) == set(R.TABLE)
    for (H, W, B, lim), (r, nt, cross, sched) in want.items():
        p = R.halo_plan(B, H, W, lim)
        assert p["eligible"] and (p["R"], p["ntiles"], p["crosses"], p["schedule"]) == (r, nt, cross, sched), (H, W, B, lim, p)
    p = R.halo_plan(3, 32, 32, 8)                        # the tail of 4 on 8 workgroups: 2 rem == G, the rule's own edge
    assert (p["nfull"], p["nhalf"], p["grid"]) == (8, 8, 8)
    assert R.halo_plan(12, 14, 14, 8)["crossings"] == 2 and R.halo_plan(37, 8, 8, 8)["crossings"] == 4       # a tile spans two / four images' borders
    assert R.halo_plan(400, 14, 14, 256)["schedule"] == "half_tail" and R.halo_plan(90, 28, 28, 256)["schedule"] == "half_tail"     # test_halo_tail_runs_as_half_jobs' shapes
    assert not R.halo_plan(2, 7, 2, 8)["eligible"] and not R.halo_plan(40, 4, 4, 8)["eligible"]          # too narrow; 64-row tiles over 4-row images: no room


def test_slot_plan_by_hand():
    assert R.slot_plan(1, 64, 64, 256, 512, cu_limit=256)["ns3_plan"] == 8
    assert R.slot_plan(1, 64, 64, 256, 512, cu_limit=248)["ns3_plan"] == 7
    assert R.slot_plan(1, 64, 64, 256, 256, cu_limit=248)["ns3_plan"] == 12            # 15 -> a multiple of 4 (two XCDs), not 8
    assert R.slot_plan(1, 64, 64, 256, 256, cu_limit=256)["ns3_plan"] == 16
    assert R.slot_plan(1, 64, 64, 256, 512, cu_limit=8)["ns3_plan"] == 1
    p = R.slot_plan(1, 64, 64, 256, 512, cu_limit=256)
    assert p["wide"] and p["nchunks"] == 67 and p["ns3"] == 8 and p["grid"] == (8, 8, 4) and not p["auto"]
    p = R.slot_plan(9, 16, 16, 256, 512, cu_limit=8)
    assert not p["wide"] and p["nchunks"] == 41 and p["ns3"] == 1 and p["auto"]
    p = R.slot_plan(9, 8, 8, 256, 256, stride2=True, cu_limit=8)                         # Downsample's weight gradient of 9 x 16 x 16 inputs
    assert p["grid"] == (1, 16, 4) and p["auto"]
    assert not R.slot_plan(1, 64, 64, 256, 256, stride2=True)["eligible"]


def test_case_tables_reach_every_planner_branch():
    """The cap on the case tables of test_gpu_conv_wide.py: every halo family meets all four schedules, tiles aligned to images and
    tiles that cross them, and a tile over more than two images; the slot family meets both windows, split counts on both sides of 8 as the
    CU limit sets them, and both answers of the automatic choice - at 256 outputs and both input widths."""
    for fam in ("halo_forward", "halo_dgrad", "halo_resample"):
        plans = [R.halo_plan(B, H, W, lim) for (H, W, B, lim) in R.CASES[fam]]
        assert all(p["eligible"] for p in plans), fam
        assert {p["schedule"] for p in plans} == {"all_half", "whole_rounds", "half_tail", "whole_partial"}, fam
        assert {p["crosses"] for p in plans} == {False, True}, fam
        assert max(p["crossings"] for p in plans) >= 4 and any(p["R"] > H for p, (H, W, B, lim) in zip(plans, R.CASES[fam])), fam
        assert any(p["schedule"] == "half_tail" and 2 * (p["ntiles"] % p["grid"]) == p["grid"] for p in plans), fam     # the `<=` of the tail rule
        assert any(p["schedule"] == "half_tail" and p["crosses"] for p in plans), fam
        assert {lim for (_, _, _, lim) in R.CASES[fam]} >= {8, 248, 256}, fam
        assert all(H % 2 == 0 and W % 2 == 0 for (H, W, _, _) in R.CASES[fam]), fam                                  # the resampling forms halve them
    for ktot in (256, 512):
        plans = [R.slot_plan(B, H, W, 256, ktot, cu_limit=lim) for (H, W, B, lim) in R.CASES["slot_wgrad"]]
        assert all(p["eligible"] for p in plans)
        assert {p["wide"] for p in plans} == {False, True}, ktot
        assert {p["auto"] for p in plans} == {False, True}, ktot
        assert min(p["ns3_plan"] for p in plans) < 8 <= max(p["ns3_plan"] for p in plans), ktot
        assert min(p["ns3"] for p in plans) == 1 and max(p["ns3"] for p in plans) >= 8, ktot
    assert {lim for (_, _, _, lim) in R.CASES["slot_wgrad"]} == {8, 248, 256}
    both = [R.slot_plan(B, H, W, 256, k, cu_limit=lim)["ns3_plan"] for (H, W, B, lim) in R.CASES["slot_wgrad"] for k in (256, 512)]
    assert {1, 7, 8, 12, 16} <= set(both)                     # 8 / 32, 248 / 32, 256 / 32, 248 / 16 on two XCDs, 256 / 16
