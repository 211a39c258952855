"""Every kernel instantiation of csrc/gn_silu.hip against a float64 reference of the same operation on the same rounded operands
(tests/gn_ref.py, written from the contract in include/gmk.h).  The case tables live in gn_ref; tests/test_host_gn_ref.py holds them to
the dispatch: each of the 49 gn_silu_* kernels of the code object is launched by some case here, and each case launches the kernel id its
row names (asserted here through gmk_last_kernel).

What is asserted, per (sample, 32-channel slab) unless stated, nothing excluded:
  A.1  max|got - ref64| / max|ref64| < 1e-2 for results stored in 16 bits, < 1e-3 for fp32 results (the project's bars, per slab instead of
       over the whole tensor);
  A.2  16-bit y and dx of the centred cases: rms(got - ref64) <= 1.05 rms(round(ref64) - ref64).  Derived, not measured: the fp32 chain,
       hardware exp and reciprocal at a few ulp included, adds about 1e-6 relative beside the 2^-9 (bf16) / 2^-12 (fp16) of the one final
       rounding, and a double rounding flips a result with probability of order 1e-3.  One group's rstd wrong by 2^-9 passes the whole-tensor
       1e-2 bar and measures 1.1 (bf16) / 4 (fp16) here (tests/test_host_gn_ref.py);
  B    fp32 results.  rstd: relative error <= 4 2^-24 log2(n) (1 + m^2 / sigma^2) per group (n values per group, m and sigma from the
       reference: the error model of one-pass fp32 statistics); mean: absolute error <= 4 2^-24 log2(n) sqrt(m^2 + sigma^2);
       dgamma_part, dbeta_part, dxsum: per sample max|err| / max|ref64| < 1e-4; the gmk_gn_stats tables: per sample, relative to the table's
       maximum, within the rstd bound + 2^-22; gmk_gn_stats and gmk_gn_silu_fwd return the same mean / rstd bits.
  The cases 8 sigma off centre get A.1 and B only: there the rstd bound (1.7e-4) is of the size of the fp16 rounding.
Every assertion message carries gn_ref.worst(): sample, slab, group, pixel and - for the register / LDS kernels - pixel plane and iteration.

Measured on an MI355X, smallest .. largest over the cases of a family of each case's worst (sample, slab); no kernel needed a change:
  family                        A.1 (y / dx)          A.2               mean, rstd error / bound    partials, dxsum (B)
  forward register  bf16        2.0e-3 .. 3.6e-3      1.000000          0.007 .. 0.038, 0.017 .. 0.082
  forward register  fp16        2.6e-4 .. 4.7e-4      1.000000 .. 1.000001   0.004 .. 0.048, 0.020 .. 0.085
  forward streaming bf16        2.1e-3 .. 3.8e-3      1.000000          0.007 .. 0.20,  0.045 .. 0.14
  forward streaming fp16        2.9e-4 .. 4.6e-4      1.000000 .. 1.000004   0.010 .. 0.22,  0.055 .. 0.12
  forward streaming fp32        1.7e-7 .. 2.8e-7      -                 0.010 .. 0.072, 0.046 .. 0.14
  forward pair      bf16 / fp16 2.2e-3 .. 3.7e-3 / 2.7e-4 .. 4.7e-4   1.000000 .. 1.000001   0.005 .. 0.025, 0.036 .. 0.073
  forward, 8 sigma off centre   bf16 3.2e-3, fp16 4.6e-4, fp32 1.4e-5   -          0.089 .. 0.14,  0.085 .. 0.14
  gmk_gn_stats tables           scale 0.018 .. 0.085 of the bound, shift 0.016 .. 0.22 of it; statistics bits equal everywhere
  producer statistics           3.5e-3                -                 mean 9.3e-8, rstd 1.2e-7 (max-norm)
  backward hybrid    (both x)   2.3e-3 .. 3.5e-3      1.000000          -                           9.7e-8 .. 3.0e-7
  backward streaming (both x)   2.5e-3 .. 3.6e-3      1.000000          -                           9.0e-8 .. 4.9e-7
  backward streaming fp32       1.2e-7 .. 2.4e-7      -                 -                           1.4e-7 .. 4.4e-7
  backward, 8 sigma off centre  3.1e-3 .. 3.7e-3 (fp32 1.2e-5)   -      -                           1.6e-6 .. 1.5e-5
  backward pair      (both x)   2.4e-3 .. 2.8e-3      1.000000 .. 1.000243   -                      partials 1.1e-7 .. 2.5e-7; dxsum 1.2e-6 .. 5.3e-5
  sumpool2x2                    bf16 2.9e-3, fp32 9.1e-8   1.000000
The paired backward's dxsum is the one figure near its bar, and the reference explains it: bf16(ds) of the fp32 chain and of the float64 chain
differ in 2 - 15 elements per tensor (ties of the rounding, 4e-5 of the elements), one such step of 2^-7 moves a channel sum by 5e-5 of the
largest; with the kernel's own ds (the two-call form's, whose bits the pair shares) in the composite the dxsum error is 1.0e-7 .. 1.5e-7.
Wall time of the module: 3.7 s (205 cases, the slowest 0.45 s - the first, which loads the library).
"""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_ref as R  # noqa: E402

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
RANGES = {}                 # family -> figure -> [min, max] over the cases that ran
T0 = time.time()


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from generative_models_amd import ops as o
    yield o
    for fam in sorted(RANGES):          # (shown with -s: the figures the module docstring quotes)
        print(f"\nRANGE {fam}: " + "; ".join(f"{k} {lo:.6f} .. {hi:.6f}" if k.startswith("A.2") else f"{k} {lo:.2e} .. {hi:.2e}" for k, (lo, hi) in sorted(RANGES[fam].items())), end="")
    print(f"\nRANGE module wall time {time.time() - T0:.1f} s")


@pytest.fixture
def lib(ops):
    """The library with the kernel choice put back afterwards"""
    from generative_models_amd._lib import lib as l
    try:
        yield l
    finally:
        l.gmk_set_kernel_choice(-1, -1, -1)
        ops.GN_STATS = False


def note(fam, log):
    for k, v in log:
        lo, hi = RANGES.setdefault(fam, {}).get(k, (v, v))
        RANGES[fam][k] = (min(lo, v), max(hi, v))


def family(c):
    t = {R.F32: "fp32", R.BF16: "bf16", R.F16: "fp16"}[c.x_dtype]
    name = {R.K_FWD_REG: "forward register", R.K_FWD: "forward streaming", R.K_BWD_HYBRID: "backward hybrid", R.K_BWD: "backward streaming",
            R.K_FWD_PAIR: "forward pair", R.K_BWD_PAIR: "backward pair"}[c.kernel]
    return f"{name} {t}" + (" offset" if c.offset else "")


def device_inputs(c):
    t = R.make_inputs(c)
    d = {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in t.items()}
    d["xadd"] = d["xadd_table"][:, c.C:2 * c.C] if c.xadd else None          # a column view of a wider table, as the model passes it
    return t, d


def run_forward(ops, lib, c, d):
    drop = (c.p, R.SEED, R.OFFSET) if c.p else None
    lib.gmk_set_kernel_choice(-1, -1, c.mode)
    y, mean, rstd = ops.gn_silu_fwd(d["x"], d["gamma"], d["beta"], c.G, dropout=drop, xadd=d["xadd"])
    kid = lib.gmk_last_kernel()
    lib.gmk_set_kernel_choice(-1, -1, -1)
    torch.cuda.synchronize()
    assert kid == c.kernel, f"{R.ident(c)}: kernel {kid}, the table says {c.kernel}"
    return y, mean, rstd


_STATS_IDS = {R.ident(c) for c in R.STATS}


@pytest.mark.parametrize("c", [c for c in R.FORWARD if not c.stats], ids=R.ident)
def test_forward(ops, lib, c):
    """gmk_gn_silu_fwd: y under A.1 (and A.2 where centred), mean and rstd under B; on the automatic 16-bit shapes gmk_gn_stats as well - its
    tables under B, its statistics the forward's bits."""
    t, d = device_inputs(c)
    what, dt, log = R.ident(c), R.TORCH[c.x_dtype], []
    y, mean, rstd = run_forward(ops, lib, c, d)
    drop = (c.p, R.SEED, R.OFFSET) if c.p else None
    y64 = R.forward64(t["x"], t["gamma"], t["beta"], c.G, xadd=t["xadd"], dropout=drop)[0]
    form = R.pixel_form(c) or (None, None)
    R.check_stats(mean.cpu(), rstd.cpu(), t["x"], c.G, what, xadd=t["xadd"], log=log)
    R.check_a(y, y64, dt, what + " y", not c.offset, it=form[0], groups=c.G, planes=form[1], log=log)
    if what in _STATS_IDS and c.mode == -1:
        B, C = c.B, c.C
        tabs = torch.full((2, B, 3 * C), float("nan"), device="cuda")
        sc, sh = tabs[0, :, C:2 * C], tabs[1, :, C:2 * C]
        m2, r2 = ops.gn_stats(d["x"], d["gamma"], d["beta"], c.G, sc, sh, xadd=d["xadd"])
        assert lib.gmk_last_kernel() == c.kernel
        torch.cuda.synchronize()
        assert torch.equal(m2, mean) and torch.equal(r2, rstd), f"{what}: gn_stats and gn_silu_fwd disagree on the statistics bits"
        assert bool(torch.isnan(tabs[:, :, :C]).all()) and bool(torch.isnan(tabs[:, :, 2 * C:]).all()), f"{what}: gn_stats wrote outside its columns"
        R.check_tables(sc.cpu(), sh.cpu(), t["x"], t["gamma"], t["beta"], c.G, what + " table", xadd=t["xadd"], log=log)
    note(family(c), log)


def test_forward_with_producer_statistics(ops, lib):
    """Statistics emitted by the producing convolution (ops.conv_igemm(..., gn_stats=True), as test_conv_emits_groupnorm_statistics obtains
    them): y under A.1 against the float64 GroupNorm of the convolution's STORED output, the statistics at that test's 1e-4 (they are those of
    the unrounded sums, so no A.2 and no bound B)."""
    c = next(c for c in R.FORWARD if c.stats)
    B, S, C = c.B, c.S, c.C
    g = torch.Generator().manual_seed(90)
    rnd = lambda *shape: torch.randn(shape, generator=g)
    x = rnd(B, S, S, C).bfloat16().cuda()
    w = (rnd(C, C, 3, 3) / (9 * C) ** 0.5).bfloat16().float()
    wf = torch.empty(w.numel(), device="cuda", dtype=BF16)
    ops.pack_conv_weight(w.cuda(), wf, None)
    res = (rnd(B, S, S, C) * 3).bfloat16().cuda()
    lib.gmk_set_kernel_choice(3, -1, -1)
    ops.GN_STATS = True
    out = ops.conv_igemm([x], wf, C, 3, 0, (S, S), bias=(0.5 * rnd(C)).cuda(), residual=res, gn_stats=True)
    lib.gmk_set_kernel_choice(-1, -1, -1)
    ops.GN_STATS = False
    assert getattr(out, "_gn_stats", None) is not None
    gamma, beta = 1 + 0.2 * rnd(C), 0.1 * rnd(C)
    y, mean, rstd = ops.gn_silu_fwd(out, gamma.cuda(), beta.cuda(), c.G)
    assert lib.gmk_last_kernel() == c.kernel
    torch.cuda.synchronize()
    y64, m64, r64 = R.forward64(out.cpu(), gamma, beta, c.G)
    log = []
    R.check_a(y, y64, BF16, "producer-statistics y", False, groups=c.G, log=log)
    em = float((mean.cpu().double() - m64).abs().max() / m64.abs().max())
    er = float((rstd.cpu().double() - r64).abs().max() / r64.abs().max())
    log += [("mean, max-norm", em), ("rstd, max-norm", er)]
    note("forward producer statistics", log)
    assert em < 1e-4 and er < 1e-4, (em, er)


def dxsum_buffer(c):
    """-> (the [B][C] view handed to the kernel or None, the whole buffer): absent, contiguous, or columns 8 .. 8 + C of a wider table"""
    if not c.dxsum:
        return None, None
    whole = torch.full((c.B, c.C if c.dxsum == 1 else 2 * c.C + 24), float("nan"), device="cuda")
    return (whole if c.dxsum == 1 else whole[:, 8:8 + c.C]), whole


@pytest.mark.parametrize("c", R.BACKWARD, ids=R.ident)
def test_backward(ops, lib, c):
    """gmk_gn_silu_bwd with the statistics its own forward wrote: dx (addends included) under A.1 / A.2 against the gradient of the float64
    forward, the per-sample dgamma / dbeta partials and dxsum (the sums of the unrounded dx) under B."""
    t, d = device_inputs(c)
    what, gdt, log = R.ident(c), R.TORCH[c.dtype], []
    drop = (c.p, R.SEED, R.OFFSET) if c.p else None
    _, mean, rstd = ops.gn_silu_fwd(d["x"], d["gamma"], d["beta"], c.G, xadd=d["xadd"])
    adds = [("dadd", "dadd2")[i] for i in range(c.dadd)]
    a1, a2 = (d[adds[0]] if adds else None), (d[adds[1]] if len(adds) > 1 else None)
    dxsum, whole = dxsum_buffer(c)
    lib.gmk_set_kernel_choice(-1, -1, c.mode)
    dx, dgp, dbp = ops.gn_silu_bwd(d["dy"], d["x"], d["gamma"], d["beta"], mean, rstd, dadd1=a1, dadd2=a2, dxsum=dxsum, dropout=drop, xadd=d["xadd"])
    kid = lib.gmk_last_kernel()
    lib.gmk_set_kernel_choice(-1, -1, -1)
    torch.cuda.synchronize()
    assert kid == c.kernel, f"{what}: kernel {kid}, the table says {c.kernel}"
    r_dx, r_dgp, r_dbp, r_sum = R.backward64(t["dy"], t["x"], t["gamma"], t["beta"], c.G, xadd=t["xadd"], dropout=drop,
                                             dadd1=t[adds[0]] if adds else None, dadd2=t[adds[1]] if len(adds) > 1 else None)
    form = R.pixel_form(c) or (None, None)
    R.check_rows(dgp.cpu(), r_dgp, what + " dgamma_part", log=log)
    R.check_rows(dbp.cpu(), r_dbp, what + " dbeta_part", log=log)
    if dxsum is not None:
        R.check_rows(dxsum.cpu(), r_sum, what + " dxsum", log=log)
        if c.dxsum == 2:
            assert bool(torch.isnan(whole[:, :8]).all()) and bool(torch.isnan(whole[:, 8 + c.C:]).all()), f"{what}: dxsum written outside its columns"
    R.check_a(dx, r_dx, gdt, what + " dx", not c.offset, it=form[0], groups=c.G, planes=form[1], log=log)
    note(family(c), log)


@pytest.mark.parametrize("c", [c for c in R.PAIRS if c.entry == "gn_silu_fwd_pair"], ids=R.ident)
def test_forward_pair(ops, lib, c):
    """gmk_gn_silu_fwd_pair: both consumers' y, mean and rstd against float64 (the existing tests compare them with the single kernel only)."""
    t, d = device_inputs(c)
    what, dt, log = R.ident(c), R.TORCH[c.x_dtype], []
    assert ops.gn_pair_fwd_ok(d["x"], c.G, c.G2)
    sides = ops.gn_silu_fwd_pair(d["x"], (d["gamma"], d["beta"], c.G), (d["gamma2"], d["beta2"], c.G2), xadd=d["xadd"])
    assert lib.gmk_last_kernel() == c.kernel
    torch.cuda.synchronize()
    it, planes = R.pixel_form(c)
    for side, (k, G) in enumerate((("", c.G), ("2", c.G2))):
        y, mean, rstd = sides[side]
        y64 = R.forward64(t["x"], t["gamma" + k], t["beta" + k], G, xadd=t["xadd"])[0]
        R.check_stats(mean.cpu(), rstd.cpu(), t["x"], G, f"{what} side{side}", xadd=t["xadd"], log=log)
        R.check_a(y, y64, dt, f"{what} side{side}-y", True, it=it, groups=G, planes=planes, log=log)
    note(family(c), log)


@pytest.mark.parametrize("c", [c for c in R.PAIRS if c.entry == "gn_silu_bwd_pair"], ids=R.ident)
def test_backward_pair(ops, lib, c):
    """gmk_gn_silu_bwd_pair against the documented composite in float64 (the up consumer's input gradient rounded to bf16 inside, as the
    header states): dx under A.1 / A.2, dxsum and the four partial tables under B."""
    t, d = device_inputs(c)
    what, log = R.ident(c), []
    assert ops.gn_pair_ok(d["x"], c.G, c.G2)
    stats = [ops.gn_silu_fwd(d["x"], d["gamma" + k], d["beta" + k], G, xadd=d["xadd"])[1:] for k, G in (("", c.G), ("2", c.G2))]
    dxsum, whole = dxsum_buffer(c)
    dx, (dgu, dbu), (dgd, dbd) = ops.gn_silu_bwd_pair(d["x"], (d["dy"], d["dadd"], d["gamma"], d["beta"], *stats[0]),
                                                      (d["dy2"], d["dadd2"], d["gamma2"], d["beta2"], *stats[1]), dxsum=dxsum, xadd=d["xadd"])
    assert lib.gmk_last_kernel() == c.kernel
    torch.cuda.synchronize()
    r_dx, r_sum, (r_gu, r_bu), (r_gd, r_bd) = R.pair_backward64(t["x"], (t["dy"], t["dadd"], t["gamma"], t["beta"], c.G),
                                                                (t["dy2"], t["dadd2"], t["gamma2"], t["beta2"], c.G2), xadd=t["xadd"])
    for name, got, ref in (("dgamma_part up", dgu, r_gu), ("dbeta_part up", dbu, r_bu), ("dgamma_part", dgd, r_gd), ("dbeta_part", dbd, r_bd)):
        R.check_rows(got.cpu(), ref, f"{what} {name}", log=log)
    if dxsum is not None:
        R.check_rows(dxsum.cpu(), r_sum, what + " dxsum", log=log)
        if c.dxsum == 2:
            assert bool(torch.isnan(whole[:, :8]).all()) and bool(torch.isnan(whole[:, 8 + c.C:]).all()), f"{what}: dxsum written outside its columns"
    it, planes = R.pixel_form(c)
    R.check_a(dx, r_dx, BF16, what + " dx", True, it=it, groups=c.G2, planes=planes, log=log)
    note(family(c), log)


# ---- the small kernels of the same file ----------------------------------------------------------------------------------------------------
def differ(got, want):
    """elementwise: another value, or another sign of zero (NaN equals NaN, whatever its sign and payload)"""
    g, w = got.float(), want.float()
    return ~(torch.isnan(g) & torch.isnan(w)) & ((g != w) | (torch.signbit(g) != torch.signbit(w)))


def test_cast16_edges(ops):
    """gmk_cast16 against torch's conversion.  bf16 -> fp16: round to nearest even, finite values beyond the fp16 range saturate at +-65504 (as
    include/gmk.h says), infinities and NaN pass, results below 2^-14 are fp16 subnormals.  fp16 -> bf16: round to nearest even."""
    inf, nan = float("inf"), float("nan")
    g = torch.Generator().manual_seed(3)
    edge = [65280.0, -65280.0, 65536.0, -65536.0, 1e5, -7e4, 3e38, -3e38, inf, -inf, nan, 0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25,
            5 * 2.0 ** -25, 2.0 ** -26, 2.0 ** -14, 2.0 ** -15, 1e-7, -3e-6, 6e-5, 1.0, -1.0009765625]
    src = torch.cat([torch.tensor(edge), torch.randn(1024 - len(edge), generator=g) * 100]).bfloat16()
    want = src.float().to(F16)
    over = torch.isinf(want) & torch.isfinite(src.float())
    assert int(over.sum()) == 6
    want = torch.where(over, (torch.sign(src.float()) * 65504).to(F16), want)
    got = ops.cast16(src.cuda(), F16).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and int(torch.isnan(got).sum()) == 1
    bad = differ(got, want)
    assert not bool(bad.any()), [(float(s), float(a), float(b)) for s, a, b in zip(src[bad], got[bad], want[bad])][:8]
    edge = [65504.0, -65504.0, 65472.0, inf, -inf, nan, 0.0, -0.0, 2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 257 * 2.0 ** -24, 259 * 2.0 ** -24,
            2.0 ** -14, 1.00390625, 1.005859375, 1.001953125, -1.00390625]
    src = torch.cat([torch.tensor(edge, dtype=torch.float64).to(F16), (torch.randn(1024 - len(edge), generator=g) * 100).to(F16)])
    want = src.float().to(BF16)
    got = ops.cast16(src.cuda(), BF16).cpu()
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and float(want[0]) == 65536.0
    bad = differ(got, want)
    assert not bool(bad.any()), [(float(s), float(a), float(b)) for s, a, b in zip(src[bad], got[bad], want[bad])][:8]


@pytest.mark.parametrize("S", [7, 30, 64])
def test_chansum_and_colsum(ops, S):
    """gmk_chansum (bf16 and fp32, strided result) and gmk_colsum (plain, accumulating, strided rows; R = S^2 rows: the tail loop alone, both
    loops, the unrolled loop alone) against float64 at 1e-5 of the maximum."""
    g = torch.Generator().manual_seed(S)
    B, C = 2, 128 if S < 64 else 32
    for dt in (BF16, F32):
        x = (torch.randn((B, S, S, C), generator=g) * 1.5 + 0.3).to(dt)
        wide = torch.full((B, C + 40), float("nan"), device="cuda")
        ops.chansum(x.cuda(), out=wide[:, 8:8 + C])
        ref = x.double().sum((1, 2))
        e = R.rows_err(wide[:, 8:8 + C].cpu(), ref)
        assert float(e.max()) < 1e-5, (dt, e)
        assert bool(torch.isnan(wide[:, :8]).all()) and bool(torch.isnan(wide[:, 8 + C:]).all())
    rows, cols = S * S, 136                                  # 136 columns: four full blocks of 32 and one of 8
    table = torch.randn((rows, cols + 24), generator=g) + 0.5
    part = table.cuda()[:, 16:16 + cols]
    ref = table[:, 16:16 + cols].double().sum(0)
    out = torch.full((cols,), float("nan"), device="cuda")
    ops.colsum(part, out)
    assert float((out.cpu().double() - ref).abs().max() / ref.abs().max()) < 1e-5
    before = torch.randn(cols, generator=g)
    out = before.cuda()
    ops.colsum(part, out, accumulate=True)
    assert float((out.cpu().double() - (ref + before.double())).abs().max() / (ref + before.double()).abs().max()) < 1e-5


@pytest.mark.parametrize("dt", [BF16, F32], ids=["bf16", "fp32"])
def test_sumpool2x2(ops, dt):
    """gmk_sumpool2x2 against float64 under A.1 / A.2 (a sum of four stored values, rounded once): odd output sizes, several blocks."""
    g = torch.Generator().manual_seed(17)
    x = (torch.randn((3, 14, 18, 64), generator=g) * 1.5 + 0.3).to(dt)
    y = ops.sumpool2x2(x.cuda())
    xd = x.double()
    ref = xd[:, 0::2, 0::2] + xd[:, 0::2, 1::2] + xd[:, 1::2, 0::2] + xd[:, 1::2, 1::2]
    assert y.shape == (3, 7, 9, 64)
    log = []
    R.check_a(y, ref, dt, f"sumpool2x2-{dt} y", True, log=log)
    note("sumpool2x2", log)
