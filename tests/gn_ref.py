"""Float64 restatement of the GroupNorm + SiLU entry points of include/gmk.h (gmk_gn_silu_fwd, gmk_gn_stats, gmk_gn_silu_bwd and the two paired
forms), written from the header's contract and not from the kernels; the bars tests/test_gpu_gn_conformance.py holds the kernels to; an fp32
restatement of the kernels' one-pass arithmetic, on which tests/test_host_gn_ref.py shows what those bars see; and the case tables both
test modules read.  Host code only (torch on the CPU, NumPy for the Philox streams).

Tensors are NHWC [B][H][W][C] (or [B][HW][C]) as the library takes them.  Every function converts the operands it is given - the 16-bit or
fp32 tensors the kernel gets - to double and rounds nothing on the way."""
import math
import os
import sys
import zlib
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import philox_ref  # noqa: E402

F32, BF16, F16 = 0, 1, 2                                        # GMK_F32 / GMK_BF16 / GMK_F16 of include/gmk.h
TORCH = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
K_FWD_REG, K_FWD, K_BWD_HYBRID, K_BWD, K_BWD_PAIR, K_FWD_PAIR = 21, 22, 23, 24, 25, 26      # GMK_KERNEL_TABLE ids
EPS = 1e-5
SLAB = 32                                                       # channels of the slabs errors are localised to
SEED, OFFSET = 0x5EED5EED5EED, (1 << 40) + 12345                # the dropout stream of the cases that have one


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _d(t):
    return None if t is None else t.detach().double().cpu()


def channels_per_group(C, groups):
    """groups > 0: that many groups of C / groups channels; groups < 0: -groups channels per group, ceil(C / -groups) groups, the last one
    partial (it lies in the zero padding of the width)."""
    return -groups if groups < 0 else C // groups


def _grouped(t, cpg):
    """[B][HW][C] -> [B][HW][ng][cpg], a partial last group filled up with zeros (the padding it lies in, continued)"""
    B, HW, C = t.shape
    ng = (C + cpg - 1) // cpg
    if ng * cpg != C:
        t = torch.cat([t, t.new_zeros(B, HW, ng * cpg - C)], 2)
    return t.reshape(B, HW, ng, cpg)


def _per_channel(stat, cpg, C):
    """[B][ng] -> [B][1][C]"""
    return stat.repeat_interleave(cpg, 1)[:, None, :C]


def _xin(x, xadd):
    x = _d(x)
    B, C = x.shape[0], x.shape[-1]
    x = x.reshape(B, -1, C)
    return x if xadd is None else x + _d(xadd)[:, None, :]


def eps32(eps):
    """eps as the library receives it: a C float"""
    return float(np.float32(eps))


def stats64(x, groups, eps=EPS, xadd=None):
    """-> (mean, rstd) [B][ng] of x + xadd over each group's pixels x channels: two-pass, biased variance, eps inside the root."""
    xin = _xin(x, xadd)
    cpg = channels_per_group(xin.shape[-1], groups)
    g = _grouped(xin, cpg)
    mean = g.mean((1, 3))
    var = (g - mean[:, None, :, None]).square().mean((1, 3))
    return mean, 1.0 / torch.sqrt(var + eps32(eps))


def dropout_factor(shape, p, seed, offset):
    """The factor nn.Dropout(p) applies to element e (NHWC order) of a tensor of `shape`: 1 / (1 - p) iff the uniform e of stream
    (seed, offset) is >= p, else 0 (tests/philox_ref.py; p as the C float the library receives).  p = 0: ones."""
    n = int(np.prod(shape))
    if not p:
        return torch.ones(shape, dtype=torch.float64)
    p32 = np.float32(p)
    keep = philox_ref.uniform(seed, offset, n) >= p32
    return (torch.from_numpy(keep.astype(np.float64)) / (1.0 - float(p32))).reshape(shape)


def forward64(x, gamma, beta, groups, eps=EPS, xadd=None, dropout=None):
    """-> (y like x, mean, rstd): y = dropout(silu(gn(x + xadd))).  dropout = (p, seed, offset)."""
    shape = x.shape
    xin = _xin(x, xadd)
    C = xin.shape[-1]
    cpg = channels_per_group(C, groups)
    mean, rstd = stats64(x, groups, eps, xadd)
    g = (xin - _per_channel(mean, cpg, C)) * _per_channel(rstd, cpg, C) * _d(gamma)[None, None, :] + _d(beta)[None, None, :]
    y = g * torch.sigmoid(g)
    if dropout is not None and dropout[0]:
        y = y * dropout_factor(y.shape, *dropout)
    return y.reshape(shape), mean, rstd


def tables64(x, gamma, beta, groups, eps=EPS, xadd=None):
    """gmk_gn_stats: -> (scale, shift) [B][C] with y = silu(x * scale + shift): scale = rstd gamma, shift = beta + (xadd - mean) scale."""
    B, C = x.shape[0], x.shape[-1]
    cpg = channels_per_group(C, groups)
    mean, rstd = stats64(x, groups, eps, xadd)
    scale = _per_channel(rstd, cpg, C)[:, 0] * _d(gamma)[None, :]
    add = _d(xadd) if xadd is not None else torch.zeros((B, C), dtype=torch.float64)
    return scale, _d(beta)[None, :] + (add - _per_channel(mean, cpg, C)[:, 0]) * scale


def backward64(dy, x, gamma, beta, groups, eps=EPS, xadd=None, dadd1=None, dadd2=None, dropout=None, stats=None):
    """The gradient of sum(dy * forward64(x, ...)[0]) -> (dx like x, including dadd1 + dadd2 and not rounded; dgamma_part [B][C];
    dbeta_part [B][C]; dxsum [B][C], the per-sample channel sums of that dx).  stats: (mean, rstd) to use instead of the float64 ones."""
    shape = x.shape
    xin = _xin(x, xadd)
    B, HW, C = xin.shape
    cpg = channels_per_group(C, groups)
    mean, rstd = stats if stats is not None else stats64(x, groups, eps, xadd)
    mean, rstd = _d(mean), _d(rstd)
    gam = _d(gamma)[None, None, :]
    rs = _per_channel(rstd, cpg, C)
    xhat = (xin - _per_channel(mean, cpg, C)) * rs
    g = xhat * gam + _d(beta)[None, None, :]
    s = torch.sigmoid(g)
    dyd = _d(dy).reshape(B, HW, C)
    if dropout is not None and dropout[0]:
        dyd = dyd * dropout_factor(dyd.shape, *dropout)
    dg = dyd * s * (1.0 + g * (1.0 - s))
    dgp, dbp = (dg * xhat).sum(1), dg.sum(1)
    n = float(cpg * HW)
    a = _grouped((dbp * gam[0])[:, None, :], cpg).sum((1, 3)) / n            # per group: mean of d/dxhat, and of d/dxhat * xhat
    bq = _grouped((dgp * gam[0])[:, None, :], cpg).sum((1, 3)) / n
    dx = rs * (dg * gam - _per_channel(a, cpg, C) - xhat * _per_channel(bq, cpg, C))
    for t in (dadd1, dadd2):
        if t is not None:
            dx = dx + _d(t).reshape(B, HW, C)
    return dx.reshape(shape), dgp, dbp, dx.sum(1)


def pair_backward64(x, up, dn, eps=EPS, xadd=None):
    """gmk_gn_silu_bwd_pair's documented composite.  up / dn = (dy, dadd, gamma, beta, groups).
    dx = GNbwd_dn(dy_dn) + dadd_dn + bf16(GNbwd_up(dy_up) + dadd_up): the inner term is rounded to bf16 here as there, so dx is still one
    final rounding away from a float64 value.  -> (dx, dxsum, (dgp_up, dbp_up), (dgp_dn, dbp_dn))"""
    dy_u, dadd_u, gam_u, bet_u, g_u = up
    dy_d, dadd_d, gam_d, bet_d, g_d = dn
    ds, dgp_u, dbp_u, _ = backward64(dy_u, x, gam_u, bet_u, g_u, eps, xadd, dadd1=dadd_u)
    dx, dgp_d, dbp_d, dxsum = backward64(dy_d, x, gam_d, bet_d, g_d, eps, xadd, dadd1=dadd_d, dadd2=ds.to(torch.bfloat16))
    return dx, dxsum, (dgp_u, dbp_u), (dgp_d, dbp_d)


# ---- where a result is worst -------------------------------------------------------------------------------------------------------
def _slabs(C):
    return [(c0, min(c0 + SLAB, C)) for c0 in range(0, C, SLAB)]


def worst(got, ref, it=None, groups=None, planes=None):
    """got, ref: NHWC.  Per (sample, 32-channel slab): max|got - ref| / max|ref| of that slab (a NaN counts as infinite) -> dict(err = [B][slabs]
    tensor, at = (sample, slab, channel, pixel), text).  The text names the sample, slab, group (given `groups`), pixel and - given the
    plan's pixels per thread `it` (planes = ceil(HW / it) unless given: pixel p = plane + i * planes) - the pixel plane and iteration."""
    got, ref = _d(got), _d(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B, C = ref.shape[0], ref.shape[-1]
    got, ref = got.reshape(B, -1, C), ref.reshape(B, -1, C)
    HW = ref.shape[1]
    d = (got - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    slabs = _slabs(C)
    err = torch.stack([d[:, :, a:b].amax((1, 2)) / ref[:, :, a:b].abs().amax((1, 2)).clamp_min(1e-30) for a, b in slabs], 1)
    b, s = divmod(int(err.argmax()), len(slabs))
    a0, a1 = slabs[s]
    p, c = divmod(int(d[b, :, a0:a1].argmax()), a1 - a0)
    c += a0
    where = f"worst at sample {b}, slab {s} (channels {a0}..{a1 - 1}), channel {c}"
    if groups is not None:
        where += f", group {c // channels_per_group(C, groups)}"
    where += f", pixel {p} of {HW}"
    if it:
        pl = planes or (HW + it - 1) // it
        where += f" = plane {p % pl} of {pl}, iteration {p // pl} of {it}"
    where += f": got {float(got[b, p, c]):.6g}, reference {float(ref[b, p, c]):.6g}"
    return dict(err=err, at=(b, s, c, p), text=f"max-norm error per (sample, slab) up to {float(err.max()):.3e}; " + where)


def rms_ratio(got, ref, dtype):
    """Per (sample, 32-channel slab) -> [B][slabs] tensor: rms(got - ref) / rms(ref.to(dtype) - ref), the distance of a result stored in
    `dtype` from the float64 reference in units of the error of rounding the reference itself (1.0: nothing but that rounding).  A slab the
    rounding leaves exact (all zero: the padding of a zero-padded width) counts 0 if the result is exact too, else infinite."""
    got, ref = _d(got), _d(ref)
    B, C = ref.shape[0], ref.shape[-1]
    got, ref = got.reshape(B, -1, C), ref.reshape(B, -1, C)
    e = got - ref
    e = torch.where(torch.isnan(e), torch.full_like(e, float("inf")), e)
    r = ref.to(dtype).double() - ref
    out = []
    for a, b in _slabs(C):
        num, den = e[:, :, a:b].square().mean((1, 2)).sqrt(), r[:, :, a:b].square().mean((1, 2)).sqrt()
        ratio = num / den.clamp_min(1e-300)
        out.append(torch.where(den == 0, torch.where(num == 0, torch.zeros_like(num), torch.full_like(num, float("inf"))), ratio))
    return torch.stack(out, 1)


def rows_err(got, ref):
    """[B][C] fp32 results: per sample max|got - ref| / max|ref| -> [B] tensor (NaN counts as infinite)"""
    got, ref = _d(got), _d(ref)
    d = (got - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    return d.amax(1) / ref.abs().amax(1).clamp_min(1e-30)


# ---- the bars ------------------------------------------------------------------------------------------------------------------------
BAR = {torch.bfloat16: 1e-2, torch.float16: 1e-2, torch.float32: 1e-3}          # A.1, per (sample, slab)
SHARP = 1.05                                                                    # A.2 (the SHARP of test_gpu_conv_wide.py)
PART_BAR = 1e-4                                                                 # B: dgamma / dbeta partials and dxsum, per sample


def _tag(what):
    """'<case> <result name>' -> the result name: the key the measured figures are collected under"""
    return what.partition(" ")[2]


def check_a(got, ref, dtype, what, sharp, it=None, groups=None, planes=None, log=None):
    """A.1 on every (sample, 32-channel slab), and with `sharp` (16-bit results of the centred cases) A.2.  -> (largest A.1 error, largest
    A.2 ratio or None); log: a list the two figures are appended to."""
    w = worst(got, ref, it, groups, planes)
    ratios = rms_ratio(got, ref, dtype) if sharp and dtype != torch.float32 else None
    msg = f"{what}: {w['text']}"
    if ratios is not None:
        b, s = divmod(int(ratios.argmax()), ratios.shape[1])
        msg += f"; rms / rounding rms per (sample, slab) {float(ratios.min()):.6f} .. {float(ratios.max()):.6f}, largest at sample {b} slab {s}"
    a1, a2 = float(w["err"].max()), (float(ratios.max()) if ratios is not None else None)
    if log is not None:
        log += [(f"A.1 {_tag(what)}", a1)] + ([(f"A.2 {_tag(what)}", a2)] if a2 is not None else [])
    assert a1 < BAR[dtype], msg
    if ratios is not None:
        assert a2 <= SHARP, msg
    return a1, a2


def stat_bounds(x, groups, eps=EPS, xadd=None):
    """The error model of one-pass fp32 statistics (sum and sum of squares of n = pixels x channels-per-group values, var = E x^2 - mean^2):
    -> (mean64, rstd64, bound on |mean - mean64|, bound on |rstd - rstd64| / rstd64), per (sample, group):
        rstd  4 2^-24 log2(n) (1 + m^2 / sigma^2)          mean  4 2^-24 log2(n) sqrt(m^2 + sigma^2)
    (m, sigma: the float64 mean and standard deviation; a group of zeros, m = sigma = 0, has the ratio 0)."""
    xin = _xin(x, xadd)
    cpg = channels_per_group(xin.shape[-1], groups)
    n = cpg * xin.shape[1]
    mean, rstd = stats64(x, groups, eps, xadd)
    var = _grouped(xin, cpg).var((1, 3), unbiased=False)
    ratio = torch.where(var > 0, mean.square() / var.clamp_min(1e-300), torch.where(mean == 0, torch.zeros_like(var), torch.full_like(var, float("inf"))))
    k = 4.0 * 2.0 ** -24 * math.log2(n)
    return mean, rstd, k * torch.sqrt(mean.square() + var), k * (1.0 + ratio)


def check_stats(mean, rstd, x, groups, what, eps=EPS, xadd=None, log=None):
    """B on the statistics -> (largest mean error / bound, largest rstd error / bound)"""
    m64, r64, mb, rb = stat_bounds(x, groups, eps, xadd)
    em = (_d(mean) - m64).abs()
    er = (_d(rstd) - r64).abs() / r64
    em = torch.where(torch.isnan(em), torch.full_like(em, float("inf")), em)
    er = torch.where(torch.isnan(er), torch.full_like(er, float("inf")), er)
    qm, qr = em / mb.clamp_min(1e-300), er / rb
    qm = torch.where((mb == 0) & (em == 0), torch.zeros_like(qm), qm)
    G = m64.shape[1]
    bm, gm = divmod(int(qm.argmax()), G)
    br, gr = divmod(int(qr.argmax()), G)
    msg = (f"{what}: mean error up to {float(em.max()):.3e} ({float(qm.max()):.3f} of its bound, sample {bm} group {gm}: got {float(mean[bm, gm]):.8g}, "
           f"reference {float(m64[bm, gm]):.8g}); rstd relative error up to {float(er.max()):.3e} ({float(qr.max()):.3f} of its bound "
           f"{float(rb[br, gr]):.3e}, sample {br} group {gr}: got {float(rstd[br, gr]):.8g}, reference {float(r64[br, gr]):.8g})")
    if log is not None:
        log += [(f"B {_tag(what)} mean error / bound".replace("  ", " "), float(qm.max())), (f"B {_tag(what)} rstd error / bound".replace("  ", " "), float(qr.max()))]
    assert float(qm.max()) <= 1.0 and float(qr.max()) <= 1.0, msg
    return float(qm.max()), float(qr.max())


def check_rows(got, ref, what, bar=PART_BAR, log=None):
    """B on an fp32 [B][C] result: per sample max|err| / max|ref| < bar"""
    e = rows_err(got, ref)
    b = int(e.argmax())
    c = int((_d(got)[b] - _d(ref)[b]).abs().nan_to_num(float("inf")).argmax())
    msg = f"{what}: per-sample errors {[f'{v:.2e}' for v in e.tolist()]}; worst at sample {b}, channel {c} (slab {c // SLAB}): got {float(got[b, c]):.8g}, reference {float(ref[b, c]):.8g}"
    if log is not None:
        log.append((f"B {_tag(what)}", float(e.max())))
    assert float(e.max()) < bar, msg
    return float(e.max())


def check_tables(scale, shift, x, gamma, beta, groups, what, eps=EPS, xadd=None, log=None):
    """B on the gmk_gn_stats tables: per sample, relative to the table's maximum, within the sample's largest rstd bound + 2^-22"""
    s64, h64 = tables64(x, gamma, beta, groups, eps, xadd)
    bound = stat_bounds(x, groups, eps, xadd)[3].amax(1) + 2.0 ** -22
    out = []
    for name, got, ref in (("scale", scale, s64), ("shift", shift, h64)):
        e = rows_err(got, ref)
        q = e / bound
        b = int(q.argmax())
        if log is not None:
            log.append((f"B {_tag(what)} {name} error / bound", float(q.max())))
        assert float(q.max()) <= 1.0, f"{what}: {name} table errors per sample {[f'{v:.2e}' for v in e.tolist()]} against {[f'{v:.2e}' for v in bound.tolist()]}, worst sample {b}"
        out.append(float(q.max()))
    return out


# ---- the kernels' arithmetic in fp32 (what the bars are shown on without a GPU) ----------------------------------------------------------------
def restate32(x, gamma, beta, groups, eps=EPS, xadd=None, dropout=None, dy=None, dadd1=None, dadd2=None, rstd_fault=None, drop_pixel=None):
    """fp32 restatement of the kernels' chain: one-pass statistics (sum and sum of squares, var = q / n - m^2), y = silu(x * sc + sh) with
    sc = rstd gamma, and with dy the backward from fp32 sums.  Results are fp32, not yet rounded to the storage type.
    rstd_fault = (sample, group, factor): that group's rstd wrong by the factor, in y only.  drop_pixel = (sample, channel, pixel): that pixel
    missing from that channel's dgamma partial.  -> dict(y, mean, rstd[, dx, dgp, dbp, dxsum])"""
    f = lambda t: None if t is None else t.detach().float().cpu()
    shape = x.shape
    B, C = shape[0], shape[-1]
    xin = f(x).reshape(B, -1, C)
    if xadd is not None:
        xin = xin + f(xadd)[:, None, :]
    HW = xin.shape[1]
    cpg = channels_per_group(C, groups)
    n = float(cpg * HW)
    # sums as the kernels form them - short per-thread chains, then trees - not as one long chain: torch's pairwise sum over a contiguous last axis
    over_group = lambda t: _grouped(t, cpg).permute(0, 2, 1, 3).reshape(B, -1, HW * cpg).sum(-1)
    over_pixels = lambda t: t.transpose(1, 2).contiguous().sum(-1)
    m = over_group(xin) / n
    var = (over_group(xin * xin) / n - m * m).clamp_min(0)
    r = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=torch.float32))
    gam, bet = f(gamma)[None, None, :], f(beta)[None, None, :]
    r_y = r.clone()
    if rstd_fault is not None:
        r_y[rstd_fault[0], rstd_fault[1]] *= rstd_fault[2]
    sc = _per_channel(r_y, cpg, C) * gam
    g = xin * sc + (bet - _per_channel(m, cpg, C) * sc)
    y = g * torch.sigmoid(g)
    if dropout is not None and dropout[0]:
        y = y * dropout_factor(y.shape, *dropout).float()
    out = dict(y=y.reshape(shape), mean=m, rstd=r)
    if dy is None:
        return out
    rs = _per_channel(r, cpg, C)
    xhat = (xin - _per_channel(m, cpg, C)) * rs
    g = xhat * gam + bet
    s = torch.sigmoid(g)
    dyf = f(dy).reshape(B, HW, C)
    if dropout is not None and dropout[0]:
        dyf = dyf * dropout_factor(dyf.shape, *dropout).float()
    dg = dyf * s * (1.0 + g * (1.0 - s))
    dgp, dbp = over_pixels(dg * xhat), over_pixels(dg)
    a = _grouped((dbp * gam[0])[:, None, :], cpg).sum((1, 3)) / n
    bq = _grouped((dgp * gam[0])[:, None, :], cpg).sum((1, 3)) / n
    dx = rs * (dg * gam - _per_channel(a, cpg, C) - xhat * _per_channel(bq, cpg, C))
    for t in (dadd1, dadd2):
        if t is not None:
            dx = dx + f(t).reshape(B, HW, C)
    if drop_pixel is not None:
        b, c, p = drop_pixel
        dgp = dgp.clone()
        dgp[b, c] -= (dg * xhat)[b, p, c]
    out.update(dx=dx.reshape(shape), dgp=dgp, dbp=dbp, dxsum=over_pixels(dx))
    return out


# ---- the case tables -------------------------------------------------------------------------------------------------------------------
# entry: the entry point.  mode: the forced GMK_GN_KERNEL mode, -1 unset.  dtype / x_dtype: type codes of the gradients (forward: of x) and of
# the saved x.  S: image side (HW = S^2).  G, G2: group counts (the pair entries: the two consumers - forward a, b; backward up, down).
# p: dropout probability.  xadd: 0 / 1.  dxsum: 0 absent, 1 contiguous, 2 a strided view.  stats: producer statistics.  kernel: the
# gmk_last_kernel id the call must report (checked against the host trace in tests/test_host_gn_ref.py).  dadd: how many gradient addends
# (backward).  offset: data at 8 sigma from zero instead of centred.
Case = namedtuple("Case", "entry mode dtype x_dtype S C G G2 p xadd dxsum stats B kernel dadd offset")


def _c(entry, S, C, G, dtype, kernel, mode=-1, x_dtype=None, G2=0, p=0.0, xadd=0, dxsum=0, stats=0, B=3, dadd=0, offset=0):
    return Case(entry, mode, dtype, dtype if x_dtype is None else x_dtype, S, C, G, G2, p, xadd, dxsum, stats, B, kernel, dadd, offset)


def _forward_cases():
    out = []
    fwd = lambda *a, **k: out.append(_c("gn_silu_fwd", *a, **k))
    for dt in (F16, BF16):
        # automatic: 64-channel slabs in registers at 2 (odd pixel count), 4 (masked last plane), 8, 14, 16 (masked), 16 pixels per thread;
        # the whole-sample streaming kernel at 7 x 7 and 8 x 8; groups of 4 and 8 channels at both widths, xadd with the wider groups
        for S in (9, 15, 20, 28, 30, 32, 7, 8):
            for C, G in ((64, 16), (64, 8), (128, 32), (128, 16)):
                fwd(S, C, G, dt, K_FWD_REG if S > 8 else K_FWD, xadd=int(C // G == 8))
        for S in (48, 64):                                                   # one 1024-thread workgroup per 32-channel slab, 16 pixels per thread
            fwd(S, 32, 8, dt, K_FWD_REG, B=2, xadd=int(S == 48))
            fwd(S, 32, 4, dt, K_FWD_REG, B=2, xadd=int(S == 64))
        fwd(9, 64, 16, dt, K_FWD_REG, B=8, xadd=1)                           # a batch of 8: the workgroup -> (sample, slab) map by XCD
        fwd(16, 32, 8, dt, K_FWD, xadd=1)                                    # 32 channels: the register form declines
        for S in (7, 15, 20, 30):                                            # mode 5: 32-channel slabs at 1, 2, 4, 8 pixels per thread
            fwd(S, 64 if S % 2 else 128, 16, dt, K_FWD_REG, mode=5, xadd=int(S > 15))
        fwd(7, 128, 32, dt, K_FWD_REG, mode=6, xadd=1)                       # mode 6: 1 pixel per thread, and 16 (masked) at 28 x 28
        fwd(28, 64, 8, dt, K_FWD_REG, mode=6)
        fwd(14, 128, 32, dt, K_FWD, mode=3, xadd=1)                          # the streaming kernel on 32- and 64-channel slabs, and on whole
        fwd(14, 128, 16, dt, K_FWD, mode=4)                                  # samples where the automatic plan takes the registers
        fwd(16, 128, 32, dt, K_FWD, mode=1, xadd=1)
        # narrow groups: one and two channels, and the explicit group sizes of the zero-padded widths 96 (in 128) and 192 (in 256)
        fwd(9, 64, 64, dt, K_FWD, xadd=1)
        fwd(14, 128, 64, dt, K_FWD)
        fwd(9, 128, -3, dt, K_FWD, xadd=1)
        fwd(7, 256, -6, dt, K_FWD, B=2)
        fwd(8, 128, 32, dt, K_FWD, p=0.2, xadd=1)                            # dropout: streaming, register, narrow
        fwd(20, 128, 16, dt, K_FWD_REG, p=0.2)
        fwd(9, 64, 64, dt, K_FWD, p=0.2)
        fwd(8, 128, 32, dt, K_FWD, xadd=1, offset=1)                         # 8 sigma off centre: streaming, register
        fwd(16, 128, 16, dt, K_FWD_REG, xadd=1, offset=1)
    for S in (7, 15, 32):
        fwd(S, 128, 32 if S != 15 else 16, F32, K_FWD, xadd=int(S == 15))
    fwd(14, 128, 32, F32, K_FWD, mode=3, xadd=1)
    fwd(9, 64, 64, F32, K_FWD, xadd=1)
    fwd(9, 128, -3, F32, K_FWD)
    fwd(8, 128, 32, F32, K_FWD, p=0.2)
    fwd(8, 128, 32, F32, K_FWD, xadd=1, offset=1)
    fwd(16, 128, 16, F32, K_FWD, xadd=1, offset=1)
    fwd(28, 128, 32, BF16, K_FWD, stats=1)                                   # statistics from the producing convolution
    return out


def _backward_cases():
    out = []
    i = [0]

    def bwd(S, C, G, kernel, dtype=BF16, both=True, **k):
        # every row with fp16 and with bf16 activations beside bf16 gradients: the fp16 call with both addends, a strided dxsum and xadd, the
        # bf16 call with none or one addend and no or a contiguous dxsum in turn
        for xdt in ((F16, BF16) if both and dtype == BF16 else (dtype,)):
            i[0] += 1
            opt = dict(dadd=2, dxsum=2, xadd=1) if xdt == F16 else dict(dadd=i[0] % 4 // 2, dxsum=(i[0] // 4) % 2, xadd=0) if dtype == BF16 else \
                dict(dadd=i[0] % 3, dxsum=i[0] % 3, xadd=i[0] % 2)
            opt.update(k)
            out.append(_c("gn_silu_bwd", S, C, G, dtype, kernel, x_dtype=xdt, **opt))
    for S in (9, 14, 16):                                                    # kHyb4
        bwd(S, 128 if S != 14 else 64, 32 if S != 14 else 8, K_BWD_HYBRID)
    bwd(20, 64, 16, K_BWD_HYBRID)                                            # kHyb13
    bwd(28, 128, 16, K_BWD_HYBRID)
    bwd(30, 64, 8, K_BWD_HYBRID)                                             # kHyb8, masked
    bwd(31, 128, 32, K_BWD_HYBRID)
    bwd(32, 128, 32, K_BWD_HYBRID)                                           # kHyb8Exact
    bwd(32, 64, 4, K_BWD_HYBRID)
    bwd(64, 32, 8, K_BWD_HYBRID, B=2)                                        # 64 x 64 on 32-channel slabs
    bwd(48, 32, 4, K_BWD_HYBRID, B=2)                                        # 16-channel slabs: 48 x 48; 16 channels; mode 7
    bwd(64, 16, 4, K_BWD_HYBRID, B=2)
    bwd(64, 32, 8, K_BWD_HYBRID, B=2, mode=7)
    bwd(9, 64, 16, K_BWD_HYBRID, B=8)                                        # a batch of 8
    bwd(7, 128, 32, K_BWD)                                                   # streaming: small images; dropout (32-channel slabs at 32 x 32)
    bwd(8, 64, 8, K_BWD)
    bwd(32, 128, 32, K_BWD, p=0.2)
    bwd(8, 128, 16, K_BWD, p=0.2)
    bwd(16, 128, 32, K_BWD, mode=1)                                          # forced: whole samples, 32- and 64-channel slabs
    bwd(16, 128, 16, K_BWD, mode=3)
    bwd(14, 128, 32, K_BWD, mode=4)
    bwd(9, 64, 64, K_BWD, dadd=1)                                            # narrow groups (of one channel: dx sums to zero over a channel but for the addend)
    bwd(14, 128, 64, K_BWD)
    bwd(9, 128, -3, K_BWD)
    bwd(7, 256, -6, K_BWD, B=2)
    bwd(8, 128, 32, K_BWD, offset=1)                                         # 8 sigma off centre
    bwd(16, 128, 16, K_BWD_HYBRID, offset=1)
    for S, G in ((7, 32), (15, 16), (32, 32)):
        bwd(S, 128, G, K_BWD, dtype=F32)
    bwd(14, 128, 32, K_BWD, dtype=F32, mode=3)
    bwd(9, 64, 64, K_BWD, dtype=F32, dadd=1)
    bwd(8, 128, 32, K_BWD, dtype=F32, p=0.2)
    bwd(16, 128, 16, K_BWD, dtype=F32, offset=1, xadd=1)
    return out


def _pair_cases():
    out = []
    for dt in (F16, BF16):
        for C, ga, gb, xa in ((128, 32, 16, 1), (128, 8, 32, 0), (64, 16, 8, 0), (64, 4, 16, 1)):
            out.append(_c("gn_silu_fwd_pair", 16, C, ga, dt, K_FWD_PAIR, G2=gb, xadd=xa))
        for S in (16, 32):
            out.append(_c("gn_silu_bwd_pair", S, 128, 16, BF16, K_BWD_PAIR, x_dtype=dt, G2=32, xadd=1, dxsum=2, dadd=2))
            out.append(_c("gn_silu_bwd_pair", S, 64, 16, BF16, K_BWD_PAIR, x_dtype=dt, G2=4, xadd=0, dxsum=int(S == 16), dadd=2))
    return out


FORWARD, BACKWARD, PAIRS = _forward_cases(), _backward_cases(), _pair_cases()
# gmk_gn_stats runs on every automatic 16-bit forward shape (its plan is the forward's automatic one)
STATS = [c._replace(entry="gn_stats") for c in FORWARD if c.mode == -1 and c.dtype != F32 and not c.p and not c.stats and not c.offset
         and channels_per_group(c.C, c.G) >= 4 and c.G > 0]
CASES = FORWARD + STATS + BACKWARD + PAIRS


def ident(c):
    t = {F32: "fp32", BF16: "bf16", F16: "fp16"}
    s = f"{c.S}x{c.S}-c{c.C}-g{c.G}" + (f"+{c.G2}" if c.G2 else "") + f"-{t[c.x_dtype]}"
    s += ("" if c.x_dtype == c.dtype else f"+{t[c.dtype]}") + (f"-m{c.mode}" if c.mode >= 0 else "") + (f"-B{c.B}" if c.B != 3 else "")
    s += ("-drop" if c.p else "") + ("-xadd" if c.xadd else "") + (f"-dxsum{c.dxsum}" if c.dxsum else "") + (f"-dadd{c.dadd}" if c.dadd else "")
    return s + ("-stats" if c.stats else "") + ("-offset" if c.offset else "")


def trace_line(c):
    """The case as tools/gn_launch_trace.cpp `cases` reads it"""
    return f"{c.entry} {c.mode} {c.dtype} {c.x_dtype} {c.S * c.S} {c.C} {c.G} {c.G2} {c.p:g} {c.xadd} {int(c.dxsum > 0)} {c.stats} {c.B}"


def pixel_form(c):
    """-> (pixels per thread, pixel planes) of the register forward and the LDS / register backward (pixel p = plane + i * planes), None for the
    streaming kernels: for the text of worst().  Restated from gn_fwd_plan / gn_reg_iter / gn_bwd_plan; tests/test_host_gn_ref.py holds it
    to the instantiation each case launches."""
    HW = c.S * c.S
    if c.kernel in (K_FWD_REG, K_FWD_PAIR):
        nvec = 4 if c.mode == 5 or HW > 1024 else 8
        it = 16 if HW > 1024 else 14 if nvec == 8 and HW == 784 and c.mode != 6 else next(i for i in (1, 2, 4, 8, 16) if -(-HW // i) * nvec <= 512)
        return it, -(-HW // it)
    if c.kernel in (K_BWD_HYBRID, K_BWD_PAIR):
        if HW > 1024:
            return (32, 128) if HW == 4096 and c.C % 32 == 0 and c.mode != 7 else (8, 512)
        return (8, 128) if HW > 832 else (4, 64) if HW <= 256 else (13, 64)
    return None


def real_channels(c):
    """Channels outside the zero padding: groups < 0 stands for GroupNorm(32, 32 cpg) padded to C (simple_unet.py: 96 in 128, 192 in 256)"""
    return 32 * -c.G if c.G < 0 else c.C


def make_inputs(c, seed=None):
    """The operands of a case, on the CPU in the types the library takes: x (sample b scaled by 1 + b / 2: a cross-sample mix-up shows),
    per-channel gamma = 1 + 0.2 randn, beta = 0.1 randn, xadd = 0.5 randn as the middle column block of a three times wider table (or
    None), dy and two addends in the gradient type, a second (gamma, beta, dy, dadd) set for the pair entries.  Centred data is
    1.5 randn + 0.3, offset data 1.5 randn + 12 (8 sigma).  Channels in the zero padding of a width (groups < 0) are zero throughout."""
    g = torch.Generator().manual_seed(1000 + (zlib.crc32((ident(c) + c.entry).encode()) if seed is None else seed) % 100000)
    rnd = lambda *shape: torch.randn(shape, generator=g)
    B, S, C = c.B, c.S, c.C
    live = torch.zeros(C)
    live[:real_channels(c)] = 1.0
    by_sample = (1.0 + 0.5 * torch.arange(B, dtype=torch.float32))[:, None, None, None]
    x = ((rnd(B, S, S, C) * 1.5 + (12.0 if c.offset else 0.3)) * by_sample * live).to(TORCH[c.x_dtype])
    out = dict(x=x, live=live)
    table = 0.5 * rnd(B, 3 * C)
    table[:, C:2 * C] *= live
    out["xadd_table"] = table
    out["xadd"] = table[:, C:2 * C] if c.xadd else None
    gdt = TORCH[c.dtype]
    for k in ("", "2"):
        out["gamma" + k] = (1.0 + 0.2 * rnd(C)) * live
        out["beta" + k] = 0.1 * rnd(C) * live
        out["dy" + k] = (rnd(B, S, S, C) * by_sample * live).to(gdt)
        out["dadd" + k] = (rnd(B, S, S, C) * live).to(gdt)
    return out
