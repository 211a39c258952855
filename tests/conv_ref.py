"""Float64 restatement of the four convolution modes of gmk_conv_igemm / gmk_conv_wgrad, a host mirror of the two planners that
schedule the persistent kernels (gmk_halo_geometry + the nfull / nhalf rule of gmk_halo_schedule; the ns3 rule of
gmk_wgrad_slot_plan: csrc/conv_plan.h), and the case tables of tests/test_gpu_conv_wide.py.  Host code only: tests/test_host_conv_ref.py checks the
reference against itself and the case tables against the planners' branches."""
import torch
import torch.nn.functional as F

NORMAL, STRIDE2, UPSAMPLE2, TRANSPOSED2 = 0, 1, 2, 3          # GMK_CONV_* of include/gmk.h
HALO_SLOTS = 448                                              # kHaloSlots of csrc/conv_halo.hip


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def _conv64(mode, x, w):
    if mode == NORMAL:
        return F.conv2d(x, w, None, padding=w.shape[-1] // 2)
    if mode == STRIDE2:
        return F.conv2d(x, w, None, stride=2, padding=1)
    if mode == UPSAMPLE2:
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w, None, padding=1)
    if mode == TRANSPOSED2:
        # the adjoint of y = conv2d(x, w, stride 2, padding 1) for an input of twice the output's size, written as such (no zero-stuffing,
        # no flipped taps): w is the stride-2 convolution's own weight [its cout][its cin][3][3], the source is a gradient of its output
        return F.conv_transpose2d(x, w, None, stride=2, padding=1, output_padding=1)
    raise ValueError(mode)


def conv_ref64(mode, srcs, w, bias=None, emb=None, residual=None):
    """NCHW in, NCHW out, float64 on the CPU.  srcs: one or two tensors (concatenated along channels); w: [cout][cin][k][k] - for
    TRANSPOSED2 the weight of the stride-2 convolution whose data gradient this is; bias [cout], emb [B][cout], residual like the output."""
    x = torch.cat([s.detach().double().cpu() for s in srcs], 1)
    y = _conv64(mode, x, w.detach().double().cpu())
    if bias is not None:
        y = y + bias.detach().double().cpu()[None, :, None, None]
    if emb is not None:
        y = y + emb.detach().double().cpu()[:, :, None, None]
    if residual is not None:
        y = y + residual.detach().double().cpu()
    return y


def grads64(mode, srcs, w, dy, want="both"):
    """-> ([d src_i], dw) of sum(conv(mode, cat(srcs), w) * dy) by autograd in float64.  want = "src" / "w": only that side is computed
    (the other is returned as None)."""
    xs = [s.detach().double().cpu().requires_grad_(want != "w") for s in srcs]
    wd = w.detach().double().cpu().requires_grad_(want != "src")
    y = _conv64(mode, torch.cat(xs, 1), wd)
    wrt = (xs if want != "w" else []) + ([wd] if want != "src" else [])
    g = list(torch.autograd.grad(y, wrt, dy.detach().double().cpu()))
    dw = g.pop() if want != "src" else None
    return (g if want != "w" else None), dw


# ---- the planners ----------------------------------------------------------------------------------------------------------------
def halo_plan(B, H, W, cu_limit=256, no_tail=False, no_all_half=False):
    """Tiling and schedule of a halo launch over the B x H x W OUTPUT grid: R rows of the global row list per tile, ntiles, whether a tile
    can span an image boundary, and how the wave-specialised kernel spreads the tiles over G = min(ntiles, cu_limit) workgroups:
      all_half       2 ntiles <= cu_limit: every tile as two half-channel jobs (grid 2 ntiles)
      whole_rounds   whole jobs, every round full (ntiles a multiple of G)
      half_tail      whole jobs, then a last round of rem <= G / 2 tiles as 2 rem half jobs
      whole_partial  whole jobs, the last round (rem > G / 2 tiles) partly filled
    no_tail / no_all_half: the GMK_DEV_VARIANT values that switch the half-job tail / the all-half form off (gmk_halo_schedule)"""
    R = 256 // W if W else 0
    ok = 4 <= W <= 254 and H >= 2 and R >= 1
    if not ok:
        return dict(eligible=False)
    crossings = 0 if H % R == 0 else (R - 1 + H - 1) // H
    ner = R + 2 + 2 * crossings
    rows = B * H
    ntiles = (rows + R - 1) // R
    G = min(ntiles, cu_limit)
    rem = ntiles % G
    nfull, nhalf, grid = ntiles, 0, G
    if ntiles > G and rem > 0 and 2 * rem <= G and not no_tail:
        nfull, nhalf, schedule = ntiles - rem, 2 * rem, "half_tail"
    elif 2 * ntiles <= cu_limit and not no_all_half:
        nfull, nhalf, grid, schedule = 0, 2 * ntiles, 2 * ntiles, "all_half"
    else:
        schedule = "whole_rounds" if rem == 0 else "whole_partial"
    return dict(eligible=ner * (W + 2) <= HALO_SLOTS, R=R, ntiles=ntiles, crosses=H % R != 0, crossings=crossings, schedule=schedule,
                nfull=nfull, nhalf=nhalf, grid=grid, rows=rows)


def slot_plan(B, H, W, cout, ktot, stride2=False, cu_limit=256):
    """The slot weight-gradient kernels over the B x (H + 1) x (W + 1) slot grid of the OUTPUT gradient (gmk_wgrad_slot_plan):
    `wide` the 128-slot window of rows beyond 62 pixels, `auto` whether the automatic choice takes the slot kernel, `ns3_plan` the
    wave-specialised kernel's split count as the CU limit sets it (the value the planner compares with 8), `ns3` after the work clamps."""
    WE, RE = W + 1, H + 1
    if WE + 1 > 128 or W < 4 or H < 2 or (stride2 and W + 2 > 64):
        return dict(eligible=False)
    total = B * RE * WE
    nchunks = (total + 63) // 64
    ns = max(1, cu_limit // ((cout // 128) * (ktot // 64)))
    ytiles = (4 if stride2 else 1) * (ktot // 64)
    ns3 = cu_limit // ((cout // 64) * ytiles)
    if ns3 >= 8:
        all8, two = ns3 & ~7, ns3 & ~3
        ns3 = two if all8 * 16 < ns3 * 15 else all8
    ns3 = max(ns3, 1)
    plan = ns3
    if nchunks < 8 * ns3:
        ns3 = max(nchunks // 8, 1)
    cps = (nchunks + ns3 - 1) // ns3
    ns3 = (nchunks + cps - 1) // cps
    return dict(eligible=True, wide=WE + 1 > 64, nchunks=nchunks, auto=nchunks >= 8 * ns, ns3_plan=plan, ns3=ns3,
                grid=(ns3, ytiles, cout // 64))


# ---- where a result is worst -------------------------------------------------------------------------------------------------------
def worst(got, ref, block=128, cu_limit=256):
    """got, ref: NCHW.  Per `block`-channel block max|got - ref| / max|ref| over that block, and the (b, y, x, c) of the worst element of the
    worst block with its halo tile and row within the tile (halo_plan of the tensor's own grid).  -> dict(err=[per block], at, tile, row, text)"""
    got = got.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    B, C, H, W = ref.shape
    errs, at, top = [], None, -1.0
    for c0 in range(0, C, block):
        d = (got[:, c0:c0 + block] - ref[:, c0:c0 + block]).abs()
        d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
        e = float(d.max()) / max(1e-30, float(ref[:, c0:c0 + block].abs().max()))
        errs.append(e)
        if e > top:
            i = int(d.argmax())
            b, r = divmod(i, d.shape[1] * H * W)
            c, r = divmod(r, H * W)
            y, x = divmod(r, W)
            top, at = e, (b, y, x, c0 + c)
    plan = halo_plan(B, H, W, cu_limit)
    b, y, x, c = at
    where = f"worst at (b={b}, y={y}, x={x}, c={c}) channel block {c // block}"
    tile = row = None
    if plan.get("eligible"):
        tile, row = divmod(b * H + y, plan["R"])
        where += f", tile {tile} of {plan['ntiles']} row {row} of R={plan['R']} ({plan['schedule']}, nfull={plan['nfull']} nhalf={plan['nhalf']})"
    return dict(err=errs, at=at, tile=tile, row=row, text=f"per-block max-norm errors {[f'{e:.3e}' for e in errs]}; " + where)


def rms_ratio(got, ref, dtype, block=128):
    """Per channel block: rms(got - ref) / rms(ref.to(dtype) - ref): how far a 16-bit result stored by one rounding lies from the float64
    reference, in units of the error of rounding the reference itself (1.0 = nothing but that rounding)."""
    got = got.detach().double().cpu(); ref = ref.detach().double().cpu()
    out = []
    for c0 in range(0, ref.shape[1], block):
        r = ref[:, c0:c0 + block]
        e_round = (r.to(dtype).double() - r).square().mean().sqrt()
        out.append(float((got[:, c0:c0 + block] - r).square().mean().sqrt() / e_round))
    return out


def worst_w(dw, ref, block=128):
    """Weight gradients [cout][cin][k][k]: max|dw - ref| / max|ref| per block x block tile of [cout][cin] -> (errors as a nested list, text)."""
    dw = dw.detach().double().cpu(); ref = ref.detach().double().cpu()
    assert dw.shape == ref.shape, (dw.shape, ref.shape)
    errs, top, at = [], -1.0, None
    for o in range(0, ref.shape[0], block):
        row = []
        for i in range(0, ref.shape[1], block):
            d = (dw[o:o + block, i:i + block] - ref[o:o + block, i:i + block]).abs()
            d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
            e = float(d.max()) / max(1e-30, float(ref[o:o + block, i:i + block].abs().max()))
            row.append(e)
            if e > top:
                j = int(d.argmax())
                shp = d.shape
                co, r = divmod(j, shp[1] * shp[2] * shp[3])
                ci, t = divmod(r, shp[2] * shp[3])
                top, at = e, (o + co, i + ci, t)
        errs.append(row)
    text = f"per-block errors {[[f'{e:.2e}' for e in r] for r in errs]}; worst at (co={at[0]}, ci={at[1]}, tap={at[2]})"
    return errs, text


# ---- the case tables of tests/test_gpu_conv_wide.py: (H, W, B, cu_limit) over the OUTPUT grid ------------------------------------------
TABLE = [(16, 16, 3, 8), (16, 16, 8, 8), (16, 16, 9, 8), (16, 16, 13, 8), (28, 28, 3, 8), (14, 14, 12, 8), (8, 8, 37, 8), (32, 32, 3, 8),
         (64, 64, 1, 8), (12, 20, 9, 8), (10, 24, 9, 8), (20, 12, 5, 8),
         (16, 16, 5, 256), (28, 28, 2, 256), (16, 16, 9, 248)]
# (every size is even: the nearest-x2 and transposed forms run on the same table with half-size sources)
SLOT_TABLE = [(16, 16, 9, 8), (64, 64, 1, 8), (64, 64, 1, 248), (28, 28, 3, 8), (14, 14, 12, 8), (8, 8, 37, 8), (32, 32, 3, 8), (12, 20, 9, 8),
              (20, 12, 5, 8), (64, 64, 1, 256), (16, 16, 9, 248), (32, 32, 3, 256), (28, 28, 2, 256)]
CASES = {
    "halo_forward": TABLE,
    "halo_dgrad": TABLE,
    "halo_resample": TABLE,
    "slot_wgrad": SLOT_TABLE,
}
