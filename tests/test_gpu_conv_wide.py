"""Convolution kernels at 256 channels (hidden_size's default in the reference's training script) and under a CU limit, against a float64
reference on the same rounded operands (tests/conv_ref.py).  At this width the sub-pixel, skip-fold and 1x1 streaming kernels decline and
every 3x3 runs on the generic halo, slot and im2col kernels with a second output-channel block, 4 or 8 K-phases and weight-row offsets of 256
in 512; `ops.set_cu_limit(8)` brings the whole-job rounds, the half-job tail and the partly filled last round of the persistent grids to
problems of 9 - 16 tiles; a few of those run at 128 channels too, where no test lowers the limit either.  tests/test_host_conv_ref.py
holds the case tables to those branches.

What is asserted (per 128-channel block, nothing excluded):
  A.1  max|got - ref64| / max|ref64| < 1e-2 for outputs stored in 16 bits, < 1e-3 for fp32 outputs (the bar of test_gpu_ops.py);
  A.2  outputs stored in 16 bits by ONE rounding of an fp32 sum: rms(got - ref64) <= 1.05 rms(round(ref64) - ref64).  Derived, not measured:
       fp32 accumulation of K <= 4608 exact products adds about sqrt(K) 2^-24 relative beside the 2^-9 (bf16) / 2^-12 (fp16) of the rounding,
       and a double rounding flips a result with probability of order 1e-3.  A dropped or doubled K-phase moves this ratio to the tens;
  B    weight gradients: max|dw - dw64| / max|dw64| < 1e-4 per 128 x 128 block of [cout][cin] (the same products, fp32 sums in another order).
Each assertion message carries conv_ref.worst(): the channel block, tile and row within the tile that broke."""
import math
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_ref as R  # noqa: E402

C = 256
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
BAR = {BF16: 1e-2, F16: 1e-2, F32: 1e-3}
SHARP = 1.05


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from generative_models_amd import ops as o
    return o


@pytest.fixture
def lib(ops):
    """The library with its global switches put back afterwards: CU limit, kernel choice, code variant, fp32 mode."""
    from generative_models_amd._lib import lib as l
    before = ops.get_cu_limit()
    try:
        yield l
    finally:
        ops.set_cu_limit(before)
        l.gmk_set_kernel_choice(-1, -1, -1)
        l.gmk_set_dev_variant(0)
        l.gmk_set_fp32_exact(1)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def q(x, dtype):
    return x.to(dtype).float()


def nhwc(x, dtype):
    return x.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def nchw(y):
    return y.detach().double().cpu().permute(0, 3, 1, 2)


def pack(ops, w, dtype):
    wf = torch.empty(w.numel(), device="cuda", dtype=dtype); wd = torch.empty_like(wf)
    ops.pack_conv_weight(w.detach().float().cuda().contiguous(), wf, wd)
    return wf, wd


def ident(case):
    return "x".join(str(v) for v in case[:2]) + f"-B{case[2]}-cu{case[3]}"


# the CU limit is not exercised at 128 channels either: a half-job tail, a partly filled last round, tiles across images, the tail rule's edge
NARROW = [(16, 16, 9, 8), (16, 16, 13, 8), (28, 28, 3, 8), (32, 32, 3, 8)]


def widths(table):
    """-> pytest parameters (channels, case): every case of `table` at 256 channels, the NARROW ones (those the table has) at 128"""
    both = [(C, c) for c in table] + [(128, c) for c in NARROW if c in table]
    return [pytest.param(cw, c, id=f"c{cw}-{ident(c)}") for cw, c in both]


def check_a(got, ref, dtype, lim, what):
    """Assertions A.1 and (16-bit outputs of one rounding) A.2 on an NHWC device result against an NCHW float64 reference."""
    got = nchw(got)
    w = R.worst(got, ref, cu_limit=lim)
    ratios = R.rms_ratio(got, ref, dtype) if dtype != F32 else []
    msg = f"{what}: {w['text']}; rms / rounding rms per block {[round(r, 6) for r in ratios]}"
    print("A", msg)
    assert max(w["err"]) < BAR[dtype], msg
    if ratios:
        assert max(ratios) <= SHARP, msg


def check_b(dw, ref, what):
    errs, text = R.worst_w(dw, ref)
    print("B", what, text)
    assert max(max(r) for r in errs) < 1e-4, f"{what}: {text}"


# -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,case", widths(R.CASES["halo_forward"]))
@pytest.mark.parametrize("two", [False, True], ids=["one", "two"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "fp16"])
def test_halo_forward_wide(ops, lib, dtype, two, C, case):
    """3x3, 256 -> 256 and 512 -> 256, bias + residual: the wave-specialised halo kernel (id 4), the 8-compute-wave kernel (id 3), the
    automatic choice, and the `emb` addend that routes to the 8-compute-wave kernel.  The kernels are bit-identical (same products, same
    order), A.1 and A.2 per channel block.  Measured over all cases: A.1 2.1e-4 - 3.5e-3; A.2 ratio 1.000000 (bf16), 1.000000 - 1.000002 (fp16)."""
    H, W, B, lim = case
    plan = R.halo_plan(B, H, W, lim)
    n = 2 if two else 1
    srcs = [q(rnd(B, C, H, W, seed=10 + i), dtype) for i in range(n)]
    w = q(rnd(C, n * C, 3, 3, seed=20) / math.sqrt(n * C * 9), dtype)
    bias = 0.1 * rnd(C, seed=21)
    emb = rnd(B, C, seed=22)
    res = q(rnd(B, C, H, W, seed=23), dtype)
    ref = R.conv_ref64(R.NORMAL, srcs, w, bias=bias, residual=res)
    wf, _ = pack(ops, w, dtype)
    sd = [nhwc(s, dtype) for s in srcs]
    rd, bd = nhwc(res, dtype), bias.cuda()
    ops.set_cu_limit(lim)
    outs = {}
    for name, force, variant, kid in (("ws", 3, 0, ops.K.CONV_HALO_WS), ("8wave", 3, 3, ops.K.CONV_HALO), ("auto", -1, 0, ops.K.CONV_HALO_WS)):
        lib.gmk_set_kernel_choice(force, -1, -1)
        lib.gmk_set_dev_variant(variant)
        outs[name] = ops.conv_igemm(sd, wf, C, 3, ops.NORMAL, (H, W), cout=C, bias=bd, residual=rd)
        assert lib.gmk_last_kernel() == kid, (name, lib.gmk_last_kernel())
    lib.gmk_set_kernel_choice(-1, -1, -1)
    lib.gmk_set_dev_variant(0)
    embd = torch.zeros((B, 3 * C), device="cuda")
    embd[:, C:2 * C] = emb.cuda()
    out_e = ops.conv_igemm(sd, wf, C, 3, ops.NORMAL, (H, W), cout=C, bias=bd, emb=embd[:, C:2 * C], residual=rd)
    assert lib.gmk_last_kernel() == ops.K.CONV_HALO
    tag = f"{plan['schedule']} c{C} {ident(case)} {dtype} srcs={n}"
    check_a(outs["ws"], ref, dtype, lim, f"wave-specialised {tag}")
    assert torch.equal(outs["ws"], outs["8wave"]), "8-compute-wave kernel differs: " + R.worst(nchw(outs["8wave"]), nchw(outs["ws"]), cu_limit=lim)["text"]
    assert torch.equal(outs["ws"], outs["auto"])
    check_a(out_e, ref + emb.double()[:, :, None, None], dtype, lim, f"emb {tag}")


@pytest.mark.parametrize("C,case", widths(R.CASES["halo_dgrad"]))
def test_halo_dgrad_offset_rows(ops, lib, C, case):
    """Data gradient of the two-source 3x3 (the up path's conv1 at width 256): 256 gradient channels against rows n0 = 0 / 256 of the 512
    packed rows, each against float64 autograd's gradient of that source; both halo kernels bit-identical.  A row offset that lands in the
    other source's rows fails here.  Measured: A.1 1.8e-3 - 3.8e-3; A.2 ratio 1.000000 to six decimals in every case."""
    H, W, B, lim = case
    dtype = BF16
    srcs = [q(rnd(B, C, H, W, seed=30 + i), dtype) for i in range(2)]
    w = q(rnd(C, 2 * C, 3, 3, seed=32) / math.sqrt(C * 9), dtype)
    dy = q(rnd(B, C, H, W, seed=33), dtype)
    dsrcs, _ = R.grads64(R.NORMAL, srcs, w, dy, want="src")
    _, wd = pack(ops, w, dtype)
    dyd = nhwc(dy, dtype)
    ops.set_cu_limit(lim)
    for i in range(2):
        outs = {}
        for name, force, variant, kid in (("ws", 3, 0, ops.K.CONV_HALO_WS), ("8wave", 3, 3, ops.K.CONV_HALO), ("auto", -1, 0, ops.K.CONV_HALO_WS)):
            lib.gmk_set_kernel_choice(force, -1, -1)
            lib.gmk_set_dev_variant(variant)
            outs[name] = ops.conv_igemm([dyd], wd, 2 * C, 3, ops.NORMAL, (H, W), n0=i * C, cout=C)
            assert lib.gmk_last_kernel() == kid, (name, lib.gmk_last_kernel())
        check_a(outs["ws"], dsrcs[i], dtype, lim, f"dgrad of source {i} (n0={i * C} of {2 * C}) {ident(case)}")
        assert torch.equal(outs["ws"], outs["8wave"]) and torch.equal(outs["ws"], outs["auto"]), f"source {i}"


@pytest.mark.parametrize("case", R.CASES["halo_resample"], ids=ident)
@pytest.mark.parametrize("res", [False, True], ids=["plain", "res"])
def test_halo_upsample_and_transposed_wide(ops, lib, res, case):
    """The x2 forms over the same output grids.  Nearest-x2 forward (bf16 and fp16): the sub-pixel kernel declines at 256 channels, the halo
    kernel (id 4) takes it.  Transposed (data gradient of the stride-2 3x3): the zero-stuffed halo form (id 5, forced, both kernels
    bit-identical) and the four parity phases on the LDS-DMA kernel (id 6: the automatic choice below 32 tiles, and fp32), against the
    explicit adjoint F.conv_transpose2d in float64.  Measured: A.1 2.6e-4 - 3.6e-3 (16-bit), 5.4e-7 - 1.7e-6 (fp32); A.2 ratio 1.000000 (bf16),
    1.000000 - 1.000002 (fp16)."""
    H, W, B, lim = case
    hs, ws = H // 2, W // 2
    ops.set_cu_limit(lim)
    for dtype in (BF16, F16):
        x = q(rnd(B, C, hs, ws, seed=40), dtype)
        w = q(rnd(C, C, 3, 3, seed=41) / math.sqrt(C * 9), dtype)
        r = q(rnd(B, C, H, W, seed=42), dtype) if res else None
        rd = nhwc(r, dtype) if res else None
        assert not ops.conv_subpixel_ok(B, hs, ws, C, dtype, cout=C)
        wf, _ = pack(ops, w, dtype)
        ref = R.conv_ref64(R.UPSAMPLE2, [x], w, residual=r)
        xd = nhwc(x, dtype)
        outs = []
        for force, variant in ((3, 0), (-1, 0)):
            lib.gmk_set_kernel_choice(force, -1, -1)
            lib.gmk_set_dev_variant(variant)
            outs.append(ops.conv_igemm([xd], wf, C, 3, ops.UPSAMPLE2, (H, W), cout=C, residual=rd))
            assert lib.gmk_last_kernel() == ops.K.CONV_HALO_WS
        check_a(outs[0], ref, dtype, lim, f"nearest-x2 forward {ident(case)} {dtype}")
        assert torch.equal(outs[0], outs[1])
    # transposed: dy is the gradient of a stride-2 convolution's (hs x ws) output, w that convolution's weight
    for dtype in (BF16, F32):
        dy = q(rnd(B, C, hs, ws, seed=43), dtype)
        w = q(rnd(C, C, 3, 3, seed=44) / math.sqrt(C * 9), dtype)
        r = q(rnd(B, C, H, W, seed=45), dtype) if res else None
        rd = nhwc(r, dtype) if res else None
        ref = R.conv_ref64(R.TRANSPOSED2, [dy], w, residual=r)
        _, wd = pack(ops, w, dtype)
        dyd = nhwc(dy, dtype)
        lib.gmk_set_kernel_choice(-1, -1, -1)
        lib.gmk_set_dev_variant(0)
        dx = ops.conv_igemm([dyd], wd, C, 3, ops.TRANSPOSED2, (H, W), cout=C, residual=rd)
        assert lib.gmk_last_kernel() == ops.K.CONV_DMA_PHASES                      # fewer than 32 tiles, or fp32: four phases
        check_a(dx, ref, dtype, lim, f"transposed, four phases {ident(case)} {dtype}")
        if dtype == BF16:
            outs = []
            for variant in (0, 3):
                lib.gmk_set_kernel_choice(3, -1, -1)
                lib.gmk_set_dev_variant(variant)
                outs.append(ops.conv_igemm([dyd], wd, C, 3, ops.TRANSPOSED2, (H, W), cout=C, residual=rd))
                assert lib.gmk_last_kernel() == ops.K.CONV_HALO_STUFFED
            check_a(outs[0], ref, dtype, lim, f"transposed, zero-stuffed halo {ident(case)}")
            assert torch.equal(outs[0], outs[1])


# (H, W, B, cu_limit) of the OUTPUT: 9 tiles of 256 pixels on 8 workgroups; 2352 pixels = 9 tiles and a partial one; one round at the default limit
IM2COL_GEOM = [(16, 16, 9, 8), (14, 14, 12, 8), (16, 16, 9, 256)]


@pytest.mark.parametrize("geom", IM2COL_GEOM, ids=ident)
@pytest.mark.parametrize("what", ["stride2", "1x1", "1x1_dgrad"])
@pytest.mark.parametrize("mode", ["bf16", "fp32", "fp32_split"])
def test_im2col_kernels_wide(ops, lib, mode, what, geom):
    """The register-staged (id 1) and LDS-DMA (id 2) im2col kernels, forced, at 256 channels: the 3x3 stride-2 forward (even and odd input
    sizes), the 1x1 over a concatenated 512-channel input, and the 1x1 data gradient against rows 0 / 256 of 512.  Under a CU limit of 8 the
    LDS-DMA kernel's persistent loop runs two rounds.  fp32 in both forms (exact MFMA chains; products as bf16 hi / lo halves, weights
    re-packed after the switch).  Measured: A.1 2.5e-3 - 3.4e-3 (bf16), 5.6e-7 - 6.2e-6 (fp32, both forms); A.2 ratio 1.000000 (bf16)."""
    H, W, B, lim = geom
    dtype = BF16 if mode == "bf16" else F32
    lib.gmk_set_fp32_exact(0 if mode == "fp32_split" else 1)
    ops.set_cu_limit(lim)
    runs = []             # (name, srcs, packed weight, w_rows, ksize, conv mode, n0, reference)
    if what == "stride2":
        hs, ws = (2 * H, 2 * W) if H % 4 == 0 else (2 * H - 1, 2 * W - 1)
        x = q(rnd(B, C, hs, ws, seed=50), dtype)
        w = q(rnd(C, C, 3, 3, seed=51) / math.sqrt(C * 9), dtype)
        runs.append((f"{hs}x{ws}", [x], pack(ops, w, dtype)[0], C, 3, ops.STRIDE2, 0, R.conv_ref64(R.STRIDE2, [x], w)))
    elif what == "1x1":
        srcs = [q(rnd(B, C, H, W, seed=52 + i), dtype) for i in range(2)]
        w = q(rnd(C, 2 * C, 1, 1, seed=54) / math.sqrt(2 * C), dtype)
        runs.append(("ktot=512", srcs, pack(ops, w, dtype)[0], C, 1, ops.NORMAL, 0, R.conv_ref64(R.NORMAL, srcs, w)))
    else:
        srcs = [q(rnd(B, C, H, W, seed=55 + i), dtype) for i in range(2)]
        w = q(rnd(C, 2 * C, 1, 1, seed=57) / math.sqrt(C), dtype)
        dy = q(rnd(B, C, H, W, seed=58), dtype)
        dsrcs, _ = R.grads64(R.NORMAL, srcs, w, dy, want="src")
        wd = pack(ops, w, dtype)[1]
        for i in range(2):
            runs.append((f"n0={i * C}", [dy], wd, 2 * C, 1, ops.NORMAL, i * C, dsrcs[i]))
    for name, srcs, wp, w_rows, ks, cmode, n0, ref in runs:
        sd = [nhwc(s, dtype) for s in srcs]
        for force, kid in ((1, ops.K.CONV_IGEMM), (2, ops.K.CONV_IGEMM_DMA)):
            lib.gmk_set_kernel_choice(force, -1, -1)
            out = ops.conv_igemm(sd, wp, w_rows, ks, cmode, (H, W), n0=n0, cout=C)
            assert lib.gmk_last_kernel() == kid
            check_a(out, ref, dtype, lim, f"kernel {kid} {what} {name} {mode} {ident(geom)}")


# (conv mode, sources, activation type, (H, W, B, cu_limit) of the output gradient): every combination on three core shapes (narrow and wide
# window under limit 8, the wide window at 248), two each on the others
def _slot_cases():
    combos = [(m, n, t) for m in (R.NORMAL, R.UPSAMPLE2) for n in (1, 2) for t in (BF16, F16)]
    out = []
    for i, case in enumerate(R.CASES["slot_wgrad"]):
        picks = combos if i < 3 else [combos[(2 * i) % 8], combos[(2 * i + 5) % 8]]
        out += [(m, n, t, case) for (m, n, t) in picks]
    out += [(R.STRIDE2, 1, t, case) for t in (BF16, F16) for case in ((8, 8, 9, 8), (16, 16, 3, 8), (14, 14, 3, 8))]
    out = [(C,) + o for o in out]
    out += [(128, m, 2, F16, case) for m in (R.NORMAL, R.UPSAMPLE2) for case in NARROW]          # ns3 = 8 / (2 x 4) = 1 at 128 channels
    return out


def _slot_id(v):
    if isinstance(v, tuple):
        return ident(v)
    if isinstance(v, torch.dtype):
        return str(v).split(".")[1]
    return f"c{v}" if v in (128, C) else None


@pytest.mark.parametrize("C,cmode,n,xdt,case", _slot_cases(), ids=_slot_id)
def test_slot_wgrad_wide(ops, lib, C, cmode, n, xdt, case):
    """Weight gradient [256][256 n][3][3] of bf16 gradients and bf16 / fp16 activations on the slot kernels: the 8-compute-wave kernel (id 12,
    bf16 activations), the wave-specialised kernel (id 13; its stride-2 four-plane form id 17), forced and as the automatic choice takes
    them, at CU limits 8 / 248 / 256 (ns3 = 1 ... 16, both windows).  Every run twice (the same bits), against the im2col kernel (id 11:
    the same products in another order, 1e-4) and against float64 autograd on the rounded operands (assertion B; fp16 activations enter as
    bf16(x), as in the kernels).  Measured B error: 1.2e-7 - 1.1e-6 on the slot kernels (ids 12, 13), 2.5e-7 - 4.9e-7 on the four-plane form
    (id 17), 8.9e-8 - 1.7e-7 on the im2col kernel; torch's own fp32 CPU autograd on the same operands lies 4.1e-7 - 2.0e-6 from float64
    (printed, not asserted)."""
    H, W, B, lim = case
    s2 = cmode == R.STRIDE2
    hs, ws = (H // 2, W // 2) if cmode == R.UPSAMPLE2 else (2 * H, 2 * W) if s2 else (H, W)
    plan = R.slot_plan(B, H, W, C, n * C, stride2=s2, cu_limit=lim)
    xs = [q(rnd(B, C, hs, ws, seed=60 + i), xdt) for i in range(n)]
    dy = q(rnd(B, C, H, W, seed=62), BF16)
    xb = [q(x, BF16) for x in xs]                                  # what the MFMA multiplies
    w0 = torch.zeros(C, n * C, 3, 3)
    _, ref = R.grads64(cmode, xb, w0, dy, want="w")
    w32 = w0.clone().requires_grad_(True)
    y32 = R._conv64(cmode, torch.cat(xb, 1), w32)
    (dw32,) = torch.autograd.grad(y32, [w32], dy)
    print("B torch fp32 CPU autograd vs float64:", R.worst_w(dw32, ref)[1])
    xd, dyd = [nhwc(x, xdt) for x in xs], nhwc(dy, BF16)
    ops.set_cu_limit(lim)

    def run(force):
        lib.gmk_set_kernel_choice(-1, force, -1)
        a = torch.empty((C, n * C, 3, 3), device="cuda"); b = torch.full_like(a, float("nan"))
        ops.conv_wgrad(dyd, xd, 3, cmode, a)
        kid = lib.gmk_last_kernel()
        ops.conv_wgrad(dyd, xd, 3, cmode, b)
        assert torch.equal(a, b), f"kernel {kid} is not reproducible"
        return a, kid

    base, kid = run(1)
    assert kid == ops.K.CONV_WGRAD
    tag = f"c{C} mode {cmode} srcs={n} x={xdt} {ident(case)} plan={plan}"
    check_b(base, ref, f"im2col {tag}")
    slot = ops.K.CONV_WGRAD_SLOTS_S2 if s2 else ops.K.CONV_WGRAD_SLOTS_WS
    todo = [(3, slot), (-1, slot if plan["auto"] else ops.K.CONV_WGRAD)]
    if xdt == BF16 and not s2:
        todo.insert(0, (2, ops.K.CONV_WGRAD_SLOTS))
    for force, want in todo:
        dw, kid = run(force)
        assert kid == want, (force, kid, want, plan)
        check_b(dw, ref, f"kernel {kid} (choice {force}) {tag}")
        errs, text = R.worst_w(dw, base)
        assert max(max(r) for r in errs) < 1e-4, f"kernel {kid} against the im2col kernel: {text}"


@pytest.mark.parametrize("xdt", [BF16, F16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("case", [(16, 16, 9, 8), (14, 14, 12, 256)], ids=ident)
def test_skip_wgrad_wide(ops, lib, xdt, case):
    """Weight gradient of the 1x1 over a concatenated 512-channel input, 256 outputs: the streaming kernel (128 channels only) declines,
    the im2col kernel (id 11) takes it; assertion B.  Measured: 8.9e-8 - 1.3e-7."""
    H, W, B, lim = case
    xs = [q(rnd(B, C, H, W, seed=70 + i), xdt) for i in range(2)]
    dy = q(rnd(B, C, H, W, seed=72), BF16)
    _, ref = R.grads64(R.NORMAL, [q(x, BF16) for x in xs], torch.zeros(C, 2 * C, 1, 1), dy, want="w")
    ops.set_cu_limit(lim)
    dw = torch.empty((C, 2 * C, 1, 1), device="cuda"); dw2 = torch.empty_like(dw)
    ops.conv_wgrad(nhwc(dy, BF16), [nhwc(x, xdt) for x in xs], 1, ops.NORMAL, dw)
    assert lib.gmk_last_kernel() == ops.K.CONV_WGRAD
    ops.conv_wgrad(nhwc(dy, BF16), [nhwc(x, xdt) for x in xs], 1, ops.NORMAL, dw2)
    assert torch.equal(dw, dw2)
    check_b(dw, ref, f"1x1 ktot=512 {xdt} {ident(case)}")


def test_conv_stress_at_256():
    """tools/conv_stress.py at 256 channels: 10 random (B, H, W, cin, upsample, epilogue) problems through both halo kernels, the slot
    weight-gradient kernel and the im2col kernels (the 128-channel run of 30 is test_gpu_ops.py's)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "conv_stress.py"), "2", "10", "256"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "failures: 0" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
