"""Every kernel of csrc/attention.hip against a float64 reference of the same operation on the same rounded operands (tests/attn_ref.py,
written from the contract in include/gmk.h), held PER ELEMENT to bounds derived there from the number formats - nothing excluded, no
whole-tensor norm.  The checks of families a - c are attn_ref.check_case, the very functions tests/test_host_attn_ref.py runs on the fp32
restatement of the kernels and on its mutants: what is caught there is caught here.

  a  bounds      gmk_attention_fwd (bf16 and fp8, P stored) and gmk_attention_bwd (on the bf16 forward's o and on the fp8 forward's, the
                 `--attention 2` training route) at N in {64, 128, 256} x B in {1, 3, 7} x randn * {0.5, 1.5, 3, 6}, and k 8 sigma off centre;
                 want_p=False and a second call give the same bits; the three-kernel chain against its own bound
  b  gather      Hadamard keys, q = 16 k[pi]: P is exactly 0 / 1, so o, the stored P and dv are compared with ==; every index map of the file,
                 and the max subtraction (the raw logit is 2048)
  c  uniform     q = 0, integer v: P == 1 / N and o == bf16(mean) bit for bit
  d  isolation   a sample's bits do not depend on its neighbours (NaN neighbours included); guard regions behind o, P, dqkv and stats
  e  rejections  N = 96, N = 512, C = 64, B = 0: the wrappers raise, nothing is written
  f  blocks      gmk_bgemm_nt (exact small-integer products, ragged M / N / K, strided operands, guarded output block), gmk_transpose,
                 gmk_softmax_fwd / gmk_softmax_bwd (ragged rows, every register slot count, N = 1 .. 1024, scores of +-1e4)
  g  dispatch    SimpleUnet._attn_core_fwd / _attn_core_bwd on the ragged three-kernel path (144 tokens, bf16 and fp32), the GMK_ATTN_BWD=gemm
                 route, the 7 x 7 rejection
  fp8 operands above 448 saturate (include/gmk.h): held to the fp8 bound against the saturating reference.

Measured on an MI355X: per family the smallest .. largest over its cases of each case's worst error / bound (the RANGE lines printed with -s):
  a  bf16 forward        o 0.130 .. 0.818       stored P 0.950 .. 0.996
     fp8 forward         o 0.133 .. 0.518       stored P 0.034 .. 0.730
     backward            dq 0.149 .. 0.860      dk 0.154 .. 0.895      dv 0.000 .. 0.924     (either forward's o)
     three-kernel chain  o 0.114 .. 0.871       P 0.896 .. 0.995       dq 0.095 .. 0.662     dk 0.091 .. 0.714     dv 0.085 .. 0.618
  b  gather backward     dq 0.008 .. 0.016      dk 0.005 .. 0.016 (bf16 mode: the fp32 terms alone)     dv 0 (exact) .. 0.475 (many-to-one)
     o, stored P and dv of the permutations: equal, bit for bit, in both modes; c, d and e likewise
  f  bgemm_nt random     bf16 -> bf16 0.958     bf16 -> fp32 0.007     fp32 0.021            (the integer cases: exact)
     softmax_fwd         fp32 up to 0.435       bf16 up to 0.996       softmax_bwd  fp32 up to 0.341, bf16 up to 0.996
  g  144 tokens          bf16: y 7.5e-3, da 7.9e-3, parameter gradients 2.2e-3 .. 6.6e-3 (bar 1e-2); fp32: 1.4e-7 .. 8.5e-7 (bar 1e-3)
     GMK_ATTN_BWD=gemm   fused route dq 0.506, dk 0.460, dv 0.378 of its bound; gemm route dq 0.284, dk 0.237, dv 0.252 of its own
  fp8 operands above 448 o 0.612, stored P 0.821
What the module found.  (1) The e4m3 conversion returns NaN above 448 and the whole sample's output went NaN with it: q, k and v are now
clamped before it (test_fp8_operands_above_448_saturate is the regression test).  (2) Two derivations were short and were corrected in
attn_ref, none scaled: the fp8 form's stored P measured up to 2.0 of U + relP because the e4m3 matrix core adds a lane's 8 products in
fixed point and drops what lies below 2^-13 of the largest (term and probe: attn_ref.Quantities, tools/fp8_mfma_probe.py); softmax_fwd in
fp32 measured 1.09 and 1.12 at N = 1023 and 1024 against 2^-21 (1 + |x|) alone, which leaves out the 22 roundings of the row sum.
Wall time of the module: 3.1 s (175 cases; the slowest 0.9 s, the first model case).
"""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_ref as R  # noqa: E402

BF16, F32 = torch.bfloat16, torch.float32
C = R.C
RANGES = {}                 # figure -> [min, max] of the cases' worst ratio to the bound
T0 = time.time()
GUARD = -7.0


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from generative_models_amd import ops as o
    yield o
    for k in sorted(RANGES):          # (shown with -s: the figures the module docstring quotes)
        print(f"\nRANGE {k}: {RANGES[k][0]:.3f} .. {RANGES[k][1]:.3f}", end="")
    print(f"\nRANGE module wall time {time.time() - T0:.1f} s")


@pytest.fixture(scope="module")
def lib(ops):
    from generative_models_amd._lib import lib as l
    return l


def note(log):
    for k, v in log:
        lo, hi = RANGES.get(k, (v, v))
        RANGES[k] = (min(lo, v), max(hi, v))


class Gpu:
    """attn_ref's `impl` on the kernels: host tensors in, host tensors out"""

    def __init__(self, ops):
        self.ops = ops

    def fwd(self, qkv, fp8=False, want_p=True):
        o, P = self.ops.attention_fwd(qkv.cuda().contiguous(), R.SCALE, want_p=want_p, fp8=fp8)
        return o.cpu(), None if P is None else P.cpu()

    def bwd(self, qkv, o, do):
        return self.ops.attention_bwd(qkv.cuda().contiguous(), o.cuda().contiguous(), do.cuda().contiguous()).cpu()

    def fwd3(self, qkv):
        ops, t = self.ops, qkv.cuda()
        q, k, v = R.split(t)
        Pm = ops.softmax_fwd(ops.bgemm_nt(q, k, out_dtype=F32), R.SCALE, t.dtype)
        return ops.bgemm_nt(Pm, ops.transpose_last2(v)), Pm

    def bwd3(self, qkv, do, Pm=None):
        """the three-kernel backward of SimpleUnet._attn_core_bwd on a stored P"""
        ops, t, do = self.ops, qkv.cuda(), do.cuda()
        q, k, v = R.split(t)
        Pm = self.fwd3(qkv)[1] if Pm is None else Pm.cuda()
        dS = ops.softmax_bwd(Pm, ops.bgemm_nt(do, v, out_dtype=F32), R.SCALE)
        d = torch.empty_like(t)
        ops.bgemm_nt(ops.transpose_last2(Pm), ops.transpose_last2(do), out=d[:, :, 2 * C:])
        ops.bgemm_nt(dS, ops.transpose_last2(k), out=d[:, :, :C])
        ops.bgemm_nt(ops.transpose_last2(dS), ops.transpose_last2(q), out=d[:, :, C:2 * C])
        return d.cpu()


# ---- a, b, c ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", R.BOUNDS, ids=R.ident)
def test_bounds(ops, c):
    log = []
    R.check_bounds_case(Gpu(ops), c, log)
    note(log)


@pytest.mark.parametrize("c", [c for c in R.BOUNDS if c.B <= 3], ids=R.ident)
def test_three_kernel_chain(ops, c):
    """bgemm_nt -> softmax_fwd -> bgemm_nt and the backward on the stored bf16 P, as the model runs them where the fused kernels do not apply"""
    log, impl = [], Gpu(ops)
    qkv, do = R.make_inputs(c)
    o3, Pm = impl.fwd3(qkv)
    Q = R.Quantities(qkv)
    R.hold(o3, Q.o, Q.bound_o(), f"{R.ident(c)} three-kernel: o", ("sample", "query", "channel"), log, "three-kernel o")
    R.hold(Pm, Q.P, Q.bound_P(), f"{R.ident(c)} three-kernel: P", ("sample", "query", "key"), log, "three-kernel P")
    R.check_backward(impl, c, None, log, " three-kernel", qkv=qkv, do=do, three=True)
    note(log)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("c", R.GATHER, ids=R.ident)
def test_exact_gather(ops, c, fp8):
    log = []
    R.check_gather_case(Gpu(ops), c, fp8, log)
    note(log)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("c", R.UNIFORM, ids=R.ident)
def test_exact_uniform(ops, c, fp8):
    R.check_uniform_case(Gpu(ops), c, fp8)


def test_fp8_operands_above_448_saturate(ops):
    """q, k and v elements of 480, 1024 and -2048 (bf16-exact): the contract says they enter as +-448"""
    c = R.Case("saturate", 2, 64, ("randn", 1.5), 448)
    qkv, _ = R.make_inputs(c)
    big = (480.0, 1024.0, -2048.0)
    for part in range(3):                         # q, k, v
        for n, val in enumerate(big):
            qkv[n % 2, 5 + 17 * part + 3 * n, part * C + 11 * n + part] = val
            qkv[1, 40 + n, part * C + 64 + n] = val
    assert int((qkv.float().abs() > 448).sum()) == 18
    log = []
    o, P, _ = R.check_forward(Gpu(ops), c, True, log, qkv=qkv)
    assert bool(torch.isfinite(o.float()).all()) and bool(torch.isfinite(P.float()).all())
    note([("fp8 saturation " + k.split()[-1], v) for k, v in log])


# ---- d: isolation ---------------------------------------------------------------------------------------------------------------------
ISO = R.Case("isolation", 7, 128, ("randn", 1.5), 77)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
def test_sample_is_independent_of_its_neighbours(ops, fp8):
    impl = Gpu(ops)
    qkv, do = R.make_inputs(ISO)
    o, P = impl.fwd(qkv, fp8, True)
    d = impl.bwd(qkv, o, do)
    nan = float("nan")
    for b in (0, 3, 6):
        o1, P1 = impl.fwd(qkv[b:b + 1], fp8, True)
        assert torch.equal(o1[0], o[b]) and torch.equal(P1[0], P[b]), f"sample {b} alone: other forward bits"
        assert torch.equal(impl.bwd(qkv[b:b + 1], o[b:b + 1], do[b:b + 1])[0], d[b]), f"sample {b} alone: other backward bits"
        qn, on, dn = (torch.full_like(t, nan) for t in (qkv, o, do))
        qn[b], on[b], dn[b] = qkv[b], o[b], do[b]
        o2, P2 = impl.fwd(qn, fp8, True)
        assert torch.equal(o2[b], o[b]) and torch.equal(P2[b], P[b]), f"sample {b} among NaN samples: other forward bits"
        assert torch.equal(impl.bwd(qn, on, dn)[b], d[b]), f"sample {b} among NaN samples: other backward bits"


@pytest.mark.parametrize("N", [64, 128, 256])
def test_guard_regions(ops, lib, N):
    B, G = 3, 4096
    qkv, do = (t.cuda() for t in R.make_inputs(R.Case("guard", B, N, ("randn", 1.5), N + 5)))

    def guarded(n, dtype):
        buf = torch.full((n + G,), GUARD, device="cuda", dtype=dtype)
        return buf, buf[:n]
    for fp8 in (0, 1):
        ob, o = guarded(B * N * C, BF16)
        pb, P = guarded(B * N * N, BF16)
        assert lib.gmk_attention_fwd(qkv.data_ptr(), o.data_ptr(), P.data_ptr(), B, N, C, R.SCALE, fp8, ops._s()) == 0
        db, d = guarded(B * N * 3 * C, BF16)
        sb, st = guarded(B * N * 2, F32)
        assert lib.gmk_attention_bwd(qkv.data_ptr(), o.data_ptr(), do.data_ptr(), d.data_ptr(), st.data_ptr(), B, N, C, R.SCALE, ops._s()) == 0
        torch.cuda.synchronize()
        for name, buf, n in (("o", ob, o.numel()), ("P", pb, P.numel()), ("dqkv", db, d.numel()), ("stats", sb, st.numel())):
            assert bool((buf[n:] == GUARD).all()), f"N={N} fp8={fp8}: wrote behind {name}"
            assert bool(torch.isfinite(buf[:n].float()).all()) and not bool((buf[:n] == GUARD).all())
        o2, P2 = ops.attention_fwd(qkv, R.SCALE, want_p=True, fp8=bool(fp8))
        assert torch.equal(o2.reshape(-1), o) and torch.equal(P2.reshape(-1), P)
        assert torch.equal(ops.attention_bwd(qkv, o2, do).reshape(-1), d)


# ---- e: rejections ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,N,Cc", [(2, 96, 128), (1, 512, 128), (2, 64, 64), (0, 64, 128)])
def test_rejections(ops, lib, B, N, Cc):
    from generative_models_amd._lib import GmkError
    qkv = torch.zeros((B, N, 3 * Cc), device="cuda", dtype=BF16)
    o = torch.zeros((B, N, Cc), device="cuda", dtype=BF16)
    for fp8 in (False, True):
        with pytest.raises(GmkError):
            ops.attention_fwd(qkv, Cc ** -0.5, want_p=True, fp8=fp8)
    with pytest.raises(GmkError):
        ops.attention_bwd(qkv, o, o)
    # the entry points themselves, on buffers that must stay as they are (host-side GMK_REQUIRE failures: nothing is launched)
    n = max(B, 1) * N * max(N, 3 * Cc)
    out = [torch.full((n,), GUARD, device="cuda", dtype=BF16) for _ in range(3)]
    st = torch.full((n,), GUARD, device="cuda", dtype=F32)
    src = torch.zeros((n,), device="cuda", dtype=BF16)
    assert lib.gmk_attention_fwd(src.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, N, Cc, 0.1, 0, ops._s()) != 0
    assert lib.gmk_attention_fwd(src.data_ptr(), out[0].data_ptr(), out[1].data_ptr(), B, N, Cc, 0.1, 1, ops._s()) != 0
    assert lib.gmk_attention_bwd(src.data_ptr(), src.data_ptr(), src.data_ptr(), out[2].data_ptr(), st.data_ptr(), B, N, Cc, 0.1, ops._s()) != 0
    torch.cuda.synchronize()
    assert all(bool((t == GUARD).all()) for t in out + [st])


# ---- f: building blocks --------------------------------------------------------------------------------------------------------------
MNK = [(1, 1, 8), (63, 65, 72), (64, 64, 64), (130, 33, 200), (144, 144, 128)]


def _wide(t, pad=8):
    """t [batch, rows, cols] as a column view of a wider tensor (leading dimension cols + 2 pad)"""
    w = torch.full((t.shape[0], t.shape[1], t.shape[2] + 2 * pad), 3.0, device="cuda", dtype=t.dtype)
    w[:, :, pad:pad + t.shape[2]] = t
    return w[:, :, pad:pad + t.shape[2]]


@pytest.mark.parametrize("alpha", [1.0, 0.5])
@pytest.mark.parametrize("M,N,K", MNK)
@pytest.mark.parametrize("types", [(BF16, BF16), (BF16, F32), (F32, F32)], ids=["bf16-bf16", "bf16-fp32", "fp32"])
def test_bgemm_nt_exact(ops, types, M, N, K, alpha):
    """operands in {-1, 0, 1}: every result is an integer (or half of one) of magnitude <= 200, exact in fp32 and in bf16"""
    tin, tout = types
    g = torch.Generator().manual_seed(M * N + K)
    A = torch.randint(-1, 2, (2, M, K), generator=g).to(tin)
    Bm = torch.randint(-1, 2, (2, N, K), generator=g).to(tin)
    want = R.bgemm_nt(A, Bm, alpha)
    assert float(want.abs().max()) <= 200 and torch.equal(want.to(tout).double(), want)
    wide = torch.full((2, M, N + 16), GUARD, device="cuda", dtype=tout)
    out = wide[:, :, 8:8 + N]
    ops.bgemm_nt(_wide(A.cuda()), _wide(Bm.cuda()), out=out, alpha=alpha)
    bad = (out.cpu().double() != want).nonzero()
    assert bad.numel() == 0, f"{len(bad)} wrong; first at (batch, m, n) = {bad[0].tolist()}: {float(out[tuple(bad[0])])} for {float(want[tuple(bad[0])])}"
    assert bool((wide[:, :, :8] == GUARD).all()) and bool((wide[:, :, 8 + N:] == GUARD).all()), "wrote outside the output's column block"
    assert torch.equal(ops.bgemm_nt(A.cuda(), Bm.cuda(), alpha=alpha, out_dtype=tout), out)


@pytest.mark.parametrize("types", [(BF16, BF16), (BF16, F32), (F32, F32)], ids=["bf16-bf16", "bf16-fp32", "fp32"])
def test_bgemm_nt_random(ops, types):
    tin, tout = types
    g = torch.Generator().manual_seed(5)
    A, Bm = torch.randn((3, 130, 200), generator=g).to(tin), torch.randn((3, 33, 200), generator=g).to(tin)
    out = ops.bgemm_nt(A.cuda(), Bm.cuda(), alpha=0.7, out_dtype=tout)
    a = float(torch.tensor(0.7, dtype=F32))
    log = []
    R.hold(out, R.bgemm_nt(A, Bm, a), R.bound_bgemm(A, Bm, a, tout == BF16), f"bgemm_nt {tin} -> {tout}", ("batch", "m", "n"), log,
           f"bgemm_nt {'bf16' if tin == BF16 else 'fp32'} -> {'bf16' if tout == BF16 else 'fp32'}")
    note(log)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("Rr,Cc", [(1, 8), (33, 65), (32, 32), (200, 128), (144, 144)])
def test_transpose_last2(ops, dtype, Rr, Cc):
    g = torch.Generator().manual_seed(Rr + Cc)
    x = torch.randn((3, Rr, Cc), generator=g).to(dtype)
    for src in (x.cuda(), _wide(x.cuda())):
        assert torch.equal(ops.transpose_last2(src).cpu(), R.transpose(x))
    wide = torch.full((3, Cc, Rr + 16), GUARD, device="cuda", dtype=dtype)
    ops.transpose_last2(_wide(x.cuda()), out=wide[:, :, 8:8 + Rr])
    assert torch.equal(wide[:, :, 8:8 + Rr].cpu(), R.transpose(x))
    assert bool((wide[:, :, :8] == GUARD).all()) and bool((wide[:, :, 8 + Rr:] == GUARD).all())


def _scores(rows, N, sig, g):
    S = torch.randn((rows, N), generator=g) * sig
    if rows >= 5:
        S[1] = 3.0                                                     # a row of equal scores
        S[rows - 2] = 1e4 * (1 - 2 * (torch.arange(N) % 2).float())     # a row of +-1e4: overflows exp without the max subtraction
    return S


@pytest.mark.parametrize("N", [1, 8, 63, 64, 65, 200, 1023, 1024])
@pytest.mark.parametrize("rows", [1, 5, 7, 600])
def test_softmax_fwd_bwd(ops, lib, rows, N):
    g = torch.Generator().manual_seed(rows * 2000 + N)
    K = {F32: 0, BF16: 1}
    scale = float(torch.tensor(R.SCALE, dtype=F32))
    log = []
    for sig in (1.0, 30.0):
        S = _scores(rows, N, sig, g)
        dP = torch.randn((rows, N), generator=g)
        ref = R.softmax_fwd(S, scale)
        for dt in (F32, BF16):
            tag = f"rows={rows} N={N} sigma={sig} {dt}"
            name = "fp32" if dt == F32 else "bf16"
            buf = torch.full((rows + 1, N), GUARD, device="cuda", dtype=dt)
            assert lib.gmk_softmax_fwd(S.cuda().data_ptr(), buf.data_ptr(), rows, N, scale, K[dt], ops._s()) == 0
            torch.cuda.synchronize()
            assert bool((buf[rows] == GUARD).all()), f"{tag}: softmax_fwd wrote behind its last row"
            P = buf[:rows].cpu()
            R.hold(P, ref, R.bound_softmax_fwd(S, scale, dt == BF16), f"{tag}: softmax_fwd", ("row", "column"), log, f"softmax_fwd {name}")
            assert torch.equal(ops.softmax_fwd(S.cuda(), scale, dt).cpu(), P)
            if dt == F32:
                assert float((P.double().sum(-1) - 1).abs().max()) <= 2.0 ** -20, f"{tag}: row sums"
            if rows >= 5:
                assert bool((P[1].double() - 1.0 / N).abs().max() <= (2.0 ** -22 + (R.U if dt == BF16 else 0)) / N)
            # the backward on the P the forward stored
            buf = torch.full((rows + 1, N), GUARD, device="cuda", dtype=dt)
            assert lib.gmk_softmax_bwd(P.cuda().data_ptr(), dP.cuda().data_ptr(), buf.data_ptr(), rows, N, scale, K[dt], ops._s()) == 0
            torch.cuda.synchronize()
            assert bool((buf[rows] == GUARD).all()), f"{tag}: softmax_bwd wrote behind its last row"
            R.hold(buf[:rows], R.softmax_bwd(P, dP, scale), R.bound_softmax_bwd(P, dP, scale, dt == BF16), f"{tag}: softmax_bwd", ("row", "column"),
                   log, f"softmax_bwd {name}")
            assert torch.equal(ops.softmax_bwd(P.cuda(), dP.cuda(), scale), buf[:rows])
    note(log)


# ---- g: the model's dispatch ---------------------------------------------------------------------------------------------------------
def rel_err(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max())


def _core_net(mode, N, B=2):
    """the net, inputs and float64 reference results of test_attention_core_vs_the_references_own_attention, at any token count"""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    dtype = F32 if mode == "fp32" else BF16
    x, dy, lin = U.attn_core_case(N, C, B)
    params = U.closed_form_params(C, attention=True)
    params["attn.qkv.weight"] = torch.cat([lin[k][0] for k in ("query", "key", "value")]).reshape(3 * C, C, 1, 1)
    params["attn.qkv.bias"] = torch.cat([lin[k][1] for k in ("query", "key", "value")])
    params["attn.proj.weight"], params["attn.proj.bias"] = lin["proj"][0].reshape(C, C, 1, 1), lin["proj"][1]
    net = SimpleUnet(C, 0.0, compute_dtype=dtype, attention=1); net.load_state_dict(params); net = net.cuda()
    net.prepare_forward()
    S = int(round(N ** 0.5))
    names = ("attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias")
    p64 = {k: params[k].double().requires_grad_(True) for k in names}
    a64 = x.reshape(B, S, S, C).permute(0, 3, 1, 2).double().requires_grad_(True)            # NCHW for the oracle
    y64 = U.attention_core(p64, a64)
    k = 256.0                                                                                # headroom for the 16-bit gradient, as in that test
    y64.backward(dy.reshape(B, S, S, C).permute(0, 3, 1, 2).double() * k)
    ref = {"y": y64.detach().permute(0, 2, 3, 1), "da": a64.grad.permute(0, 2, 3, 1), **{n: p64[n].grad for n in names}}
    a = x.reshape(B, S, S, C).cuda().to(dtype).contiguous()
    dout = (dy * k).reshape(B, S, S, C).cuda().to(dtype).contiguous()
    return net, a, dout, ref


def _run_core(net, a, dout, ops, spy=None):
    out, saved = net._attn_core_fwd(a, keep=True)
    if spy is not None:
        ow, oc = net._wgrad, net._conv

        def wgrad(dy, *args):
            spy.setdefault("wgrad dy", []).append(dy)
            return ow(dy, *args)

        def conv(*args, **kw):
            r = oc(*args, **kw)
            spy.setdefault("conv out", []).append(r)
            return r
        net._wgrad, net._conv = wgrad, conv
    try:
        da = net._attn_core_bwd(saved, dout)
    finally:
        if spy is not None:
            del net._wgrad, net._conv
    ops.flush_colsums(); net._join_side(); torch.cuda.synchronize()
    return out, saved, da


def _core_errors(net, out, da, ref):
    errs = {"y": rel_err(out, ref["y"]), "da": rel_err(da, ref["da"])}
    gb, rb = net.grad("attn.qkv.bias").reshape(3, C), ref["attn.qkv.bias"].reshape(3, C)
    errs["dqkv_w"] = rel_err(net.grad("attn.qkv.weight").reshape(3 * C, C), ref["attn.qkv.weight"].reshape(3 * C, C))
    for i, name in enumerate(("query", "key", "value")):
        # (the key bias shifts every logit of a row alike: its true gradient is zero - measured against the query bias gradient's scale)
        errs[f"d{name}_b"] = rel_err(gb[i], rb[i]) if name != "key" else float((gb[i].double().cpu() - rb[i]).abs().max() / rb[0].abs().max())
    errs["dproj_w"] = rel_err(net.grad("attn.proj.weight").reshape(C, C), ref["attn.proj.weight"].reshape(C, C))
    errs["dproj_b"] = rel_err(net.grad("attn.proj.bias"), ref["attn.proj.bias"])
    return errs


@pytest.mark.parametrize("mode", ["bf16", "fp32"])
def test_model_ragged_level_takes_the_three_kernel_path(ops, mode):
    """12 x 12 = 144 tokens (a 48 x 48 input): no fused kernel applies, in either type.  Output, da and the four parameter gradients against
    oracle.unet_ref.attention_core in double, at the bars of test_attention_core_vs_the_references_own_attention (fp32 1e-3, bf16 1e-2)."""
    net, a, dout, ref = _core_net(mode, 144)
    out, saved, da = _run_core(net, a, dout, ops)
    assert saved[2] is not None and saved[2].shape == (2, 144, 144) and saved[2].dtype == a.dtype, "the ragged level keeps P"
    errs = _core_errors(net, out, da, ref)
    print("attention core 144", mode, errs)
    assert max(errs.values()) < {"fp32": 1e-3, "bf16": 1e-2}[mode], errs


def test_model_gemm_backward_route(ops, monkeypatch):
    """GMK_ATTN_BWD=gemm at 8 x 8 tokens in bf16: the fused forward keeps P and the three-kernel backward runs on it.  Each route's dqkv is held
    to its own per-element bound against its own reference (so the two agree within the sum of the bounds and the difference of the
    references, which is D of the rounded o against D of P v); the conv-wrapped results keep the bf16 bar 1e-2."""
    res = {}
    for route in ("fused", "gemm"):
        monkeypatch.setenv("GMK_ATTN_BWD", route)
        net, a, dout, ref = _core_net("bf16", 64)
        spy = {}
        out, saved, da = _run_core(net, a, dout, ops, spy)
        assert (saved[2] is None) == (route == "fused"), f"{route}: P kept: {saved[2] is not None}"
        errs = _core_errors(net, out, da, ref)
        assert max(errs.values()) < 1e-2, (route, errs)
        qkv, o = saved[1].reshape(2, 64, 3 * C).cpu(), saved[3].reshape(2, 64, C).cpu()
        do, dqkv = spy["conv out"][0].reshape(2, 64, C).cpu(), spy["wgrad dy"][1].reshape(2, 64, 3 * C).cpu()
        res[route] = (qkv, o, do, dqkv, saved[2])
    monkeypatch.delenv("GMK_ATTN_BWD")
    (qkv, o, do, df, _), (qkv2, o2, do2, dg, Pm) = res["fused"], res["gemm"]
    assert torch.equal(qkv, qkv2) and torch.equal(o, o2) and torch.equal(do, do2)

    class Fixed:            # attn_ref's impl over the results the model produced
        def bwd(self, *_):
            return df

        def bwd3(self, *_):
            return dg
    c, log = R.Case("model", 2, 64, ("core", 1.0), 0), []
    R.check_backward(Fixed(), c, o, log, " fused route", qkv=qkv, do=do)
    R.check_backward(Fixed(), c, None, log, " gemm route", qkv=qkv, do=do, three=True)
    Q = R.Quantities(qkv)
    R.hold(Pm, Q.P, Q.bound_P(), "gemm route: stored P", ("sample", "query", "key"))
    note([("model gemm route " + k, v) for k, v in log])


def test_model_rejects_a_7x7_level(ops):
    net, _, _, _ = _core_net("bf16", 64)
    with pytest.raises(ValueError, match="49 tokens"):
        net._attn_core_fwd(torch.zeros((2, 7, 7, C), device="cuda", dtype=BF16))
