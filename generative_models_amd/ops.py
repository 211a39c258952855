"""Thin torch-tensor wrappers over the C ABI (include/gmk.h).  torch supplies device memory and streams only.

Every wrapper checks shapes/dtypes/contiguity on the host before launching (a kernel fault on this hardware can
take the whole node down) and enqueues on torch's current HIP stream.
"""
import functools
import math

import os

import torch

from ._lib import C, K, check, kernel_name, lib

F32, BF16, F16 = C["GMK_F32"], C["GMK_BF16"], C["GMK_F16"]      # these and every other GMK_* integer below: read from include/gmk.h
# fp16 = forward activations / forward weight packs of the 16-bit mode; bf16 = gradients (and the all-bf16 A/B mode)
_DT = {torch.float32: F32, torch.bfloat16: BF16, torch.float16: F16}
_HALF = (torch.bfloat16, torch.float16)
NORMAL, STRIDE2, UPSAMPLE2, TRANSPOSED2 = C["GMK_CONV_NORMAL"], C["GMK_CONV_STRIDE2"], C["GMK_CONV_UPSAMPLE2"], C["GMK_CONV_TRANSPOSED2"]

# bench.py sets this to a list to collect (kernel name, start event, end event, algorithmic FLOPs, algorithmic HBM bytes, multiplied FLOPs) per
# launch of the convolution, weight-gradient, GroupNorm and stem / head kernels; events are recorded on the stream the kernel is launched on.
# "Algorithmic" FLOPs are the REFERENCE op's (9 taps per output pixel); "multiplied" are the products the kernel's MFMAs actually form - they
# differ for the sub-pixel forms (16 tap-products per low-resolution pixel where the reference op counts 36), and only the multiplied
# count may be set against the MFMA peak.
PROFILE = None


def instantiation_key(name, dtype):
    """The template instantiation a profiled launch ran as, spelled like the keys of the counter records (tools/kernel_names.py:
    `conv3x3_halo_ws_kernel<f16>`, `<bf16>`, `<f16,+skip>`, `conv_subpixel_ws_kernel<bf16,upsample dgrad>` ...), so that a launch's own
    algorithmic bytes can stand beside its own counter bytes; None for kernels that have one instantiation per name."""
    if dtype not in _HALF:
        return None
    t = "f16" if dtype == torch.float16 else "bf16"
    if name == "conv3x3_halo_ws_kernel":
        return f"{name}<{t}>"
    if name == "conv3x3_halo_ws_kernel[+1x1 skip]":
        return f"conv3x3_halo_ws_kernel<{t},+skip>"
    if name == "conv_wgrad_slots_ws_kernel[stride-2 planes]":
        return "conv_wgrad_slots_ws_kernel<stride-2 planes>"
    if name.startswith("conv_subpixel_ws_kernel["):
        return f"conv_subpixel_ws_kernel<{t},{name[len('conv_subpixel_ws_kernel['):-1]}>"
    return None


def _nbytes(*tensors):
    """Algorithmic bytes of a launch - only evaluated when a profile is being collected (it sits on every launch's path)."""
    if PROFILE is None:
        return 0.0
    return float(sum(t.numel() * t.element_size() for t in tensors if t is not None))


class _Timed:
    """flops / nbytes: ALGORITHMIC work of the launch (each operand tensor read once, each result written once);
    fixed=True: `name` is the kernel's own name; otherwise the launcher's report is asked (gmk_last_kernel: every C entry point behind such
    a block notes an id of include/gmk.h's kernel table on every path that launches) and `name` only labels a call that has reported nothing."""

    def __init__(self, name, flops, nbytes=0.0, fixed=False, multiplied=None, dtype=None):
        self.on = PROFILE is not None
        if self.on:
            self.name, self.flops, self.nbytes, self.fixed = name, flops, nbytes, fixed
            self.multiplied = flops if multiplied is None else multiplied
            self.dtype = dtype
            self.s = torch.cuda.Event(enable_timing=True)
            self.e = torch.cuda.Event(enable_timing=True)

    def __enter__(self):
        if self.on:
            self.s.record()

    def __exit__(self, *exc):
        if self.on:
            self.e.record()
            name = self.name if self.fixed else kernel_name(lib.gmk_last_kernel()) or self.name
            PROFILE.append((name, self.s, self.e, self.flops, self.nbytes, self.multiplied, instantiation_key(name, self.dtype)))


_IN_FLIGHT = {}


def throttle(max_in_flight=2):
    """Call once per step (train step, sampler iteration): records an event and waits for the one `max_in_flight` steps back.
    A step's host work (~4 ms of launches) is far shorter than its GPU work, so an unthrottled loop queues dozens of steps
    ahead; every tensor that crossed streams (`record_stream`: the side-stream weight gradients and skip convolutions) then
    stays unavailable to the caching allocator until the GPU catches up, the pool grows by those bytes PER QUEUED STEP, hits the
    device limit and falls into free-and-retry (measured at 3x64x64, B=1024: 305 instead of 117 ms per step, and 5 instead of
    28 sampler steps/s).  Two steps in flight keep the GPU fed and the pool at its steady size."""
    q = _IN_FLIGHT.setdefault(torch.cuda.current_device(), [])
    ev = torch.cuda.Event()
    ev.record()
    q.append(ev)
    if len(q) >= max_in_flight:
        q.pop(0).synchronize()


def dt_code(dtype):
    return _DT[dtype]


# The current HIP stream's raw handle.  torch.cuda.current_stream() builds a Stream object and walks torch's device-index helpers (an
# os.environ lookup among them) on every call - a quarter of the host time of a small-batch step with ~ 350 launches (a host profile of round 3 (docs/EXPERIMENTS.md));
# the raw getter is the same value through one C call.
_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_GET_DEVICE = getattr(torch._C, "_cuda_getDevice", None)


def _s():
    if _RAW_STREAM is not None and _GET_DEVICE is not None:
        return _RAW_STREAM(_GET_DEVICE())
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _chk(t, dtype=None, name="tensor"):
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if dtype is not None and t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name}: data pointer not 16-byte aligned")
    return t


def get_cu_limit():
    return lib.gmk_get_cu_limit()


def set_cu_limit(n):
    """CUs the persistent grids launched from here on may occupy (read by the host at launch time)."""
    check(lib.gmk_set_cu_limit(int(n)), "set_cu_limit")


def aligned(t):
    """Contiguous, 16-byte aligned version of a caller-supplied tensor (a slice of a batch may start anywhere)."""
    if t is None:
        return None
    t = t.contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _f32(t, name):
    return _chk(t, torch.float32, name)


def check_stream(seed, offset):
    """-> (seed, offset) as ints.  A Philox stream is named by an unsigned 64-bit seed and counter; ctypes would wrap any other int into
    c_uint64 silently, which selects a different stream from the one asked for."""
    seed, offset = int(seed), int(offset)
    if not (0 <= seed < 1 << 64 and 0 <= offset < 1 << 64):
        raise ValueError(f"offset = {offset}, seed = {seed}: Philox counters and seeds are unsigned 64-bit")
    return seed, offset


# ---- packing ---------------------------------------------------------------------------------------------
def pack_conv_weight(w, w_fwd, w_dgrad):
    _f32(w, "w")
    cout, cin, k, _ = w.shape
    ref = w_fwd if w_fwd is not None else w_dgrad
    for t in (w_fwd, w_dgrad):
        if t is not None:
            _chk(t, name="pack")
            assert t.numel() == w.numel()
    if w_fwd is not None and w_dgrad is not None and w_fwd.dtype != w_dgrad.dtype:      # fp16 forward pack + bf16 data-gradient pack
        pack_conv_weight(w, w_fwd, None)
        pack_conv_weight(w, None, w_dgrad)
        return
    check(lib.gmk_pack_conv_weight(_p(w), _p(w_fwd), _p(w_dgrad), cout, cin, k, _DT[ref.dtype], _s()), "pack_conv_weight")


def pack_conv_weights_multi(arena, packs, table, fwd_f16=None):
    """One launch for every convolution of the net.  table = (w_off, pack_off, cout, cin, ksize) host int lists: tensor e is
    arena[w_off[e]:...] (fp32 [cout][cin][k][k]) -> packs[pack_off[e]:...] = [w_fwd | w_dgrad]; fwd_f16[e] != 0: that entry's
    w_fwd half is written as fp16 (bf16 packs only)."""
    import ctypes
    _f32(arena, "arena"); _chk(packs, name="packs")
    n = len(table[0])
    arrs = [(ctypes.c_int * n)(*[int(v) for v in col]) for col in table]
    flags = (ctypes.c_int * n)(*[int(v) for v in fwd_f16]) if fwd_f16 is not None else None
    check(lib.gmk_pack_conv_weights_multi(_p(arena), _p(packs), n, *arrs, flags, _DT[packs.dtype], _s()), "pack_conv_weights_multi")


# ---- GroupNorm + SiLU ------------------------------------------------------------------------------------
# Let producing convolutions emit GroupNorm statistics from their epilogue (gmk_conv_igemm gn_stats).  OFF by default:
# measured on MI355X the DPP reductions in the conv epilogue cost as much as the statistics pass they save (27.25 vs
# 27.19 ms/step), and with it a sample's result depends (in the last bits) on which tile neighbours it had.
GN_STATS = False
GN_FUSE = os.environ.get("GMK_GN_FUSE", "1") != "0"            # inference: GroupNorm-apply + SiLU inside the consuming convolution (simple_unet._res_fwd)
# ... where it pays (round 3's fused-GroupNorm A/B, docs/EXPERIMENTS.md 7b.7, B x HW = 1 M pixels): at 64 x 64 the statistics-only launch + fused convolution take 1,497 us against
# 1,658 us for GroupNorm + convolution (-10 %); at 32 x 32 / 28 x 28 the producer waves' transform (224 VALU issue slots per K-step
# against the ~190 the consumer's MFMA stream leaves free on the shared SIMD) costs what the normalised tensor's round trip saved
# (758 vs 747 us, 351 vs 341 us), at 16 x 16 more.  GMK_GN_FUSE_MIN_HW overrides the threshold.
GN_FUSE_MIN_HW = int(os.environ.get("GMK_GN_FUSE_MIN_HW", "2048"))
# `skip_connection(x) + h` of the up-path ResBlocks as one launch (gmk_conv3x3_skipfold; GMK_SKIP_FOLD=0: the 1x1 convolution as its own
# launch + residual epilogue, the path of rounds 1-3, kept for A/B).  GMK_SKIP_FOLD_FUSE=fuse: where inference could instead apply conv2's
# GroupNorm inside the convolution (64-pixel rows), prefer that to the fold (the two do not combine yet)
SKIP_FOLD = os.environ.get("GMK_SKIP_FOLD", "1") != "0"
SKIP_FOLD_OVER_FUSE = os.environ.get("GMK_SKIP_FOLD_FUSE", "fold") != "fuse"
EMB_SIDE = os.environ.get("GMK_EMB_SIDE", "1") == "1"          # the embedding path of a forward on the side stream (simple_unet.forward_hip; round 5: +0.7 % DDIM steps/s, +0.2 % train)
FWD_SIDE = os.environ.get("GMK_FWD_SIDE", "0") == "1"          # forward 1x1 skip convolutions on the side stream (simple_unet._res_fwd)
WGRAD_CUS = int(os.environ.get("GMK_WGRAD_CUS", "0"))           # > 0: the side stream's persistent grids take this many CUs, the data-gradient chain's the rest
WGRAD_STREAM = os.environ.get("GMK_WGRAD_STREAM", "1") != "0"    # weight gradients on a side stream beside the data-gradient chain (simple_unet._wgrad)
# GMK_GN_PAIR also gates the paired forward (gmk_gn_silu_fwd_pair, 16 x 16 only; simple_unet._res_fwd).
# The two GroupNorm backward passes over a down-path tensor (the down ResBlock's and the skip half of the matching up ResBlock's) as ONE launch
# (gmk_gn_silu_bwd_pair; simple_unet._res_bwd).  GMK_GN_PAIR=0: the two launches with the up block's input gradient handed over through HBM (A/B).
GN_PAIR = os.environ.get("GMK_GN_PAIR", "1") != "0"


def _xadd_stride(xadd, B, C):
    """xadd: optional fp32 [B, C] view (unit column stride, any row stride) added to x per (sample, channel) on load."""
    if xadd is None:
        return 0
    assert xadd.dtype == torch.float32 and xadd.shape == (B, C) and xadd.stride(1) == 1 and xadd.is_cuda
    return xadd.stride(0)


def gn_silu_fwd(x, gamma, beta, groups, eps=1e-5, dropout=None, xadd=None):
    """x NHWC [B,H,W,C] -> (y, mean[B,G], rstd[B,G]).  If the convolution that produced x attached its partial
    GroupNorm statistics (x._gn_stats), the statistics pass over x is skipped.  dropout = (p, seed, offset): nn.Dropout(p)
    behind the SiLU with the mask `rng_uniform(x.shape, seed, offset) >= p` (pass the same triple to gn_silu_bwd)."""
    _chk(x, name="x"); _f32(gamma, "gamma"); _f32(beta, "beta")
    B, H, W, C = x.shape
    assert gamma.numel() == C and beta.numel() == C
    y = torch.empty_like(x)
    # groups < 0: -groups channels per group (any size up to 16: the zero-padded widths 96, 160, 192, 224), ceil(C / -groups) groups
    ncol = groups if groups > 0 else (C - groups - 1) // -groups
    mean = torch.empty((B, ncol), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    mean._gn_groups = groups                    # gn_silu_bwd reads the group layout from the statistics it is handed
    st = getattr(x, "_gn_stats", None)
    part, tp, nt = st if st is not None else (None, 0, 0)
    dp, dseed, doff = dropout if dropout is not None else (0.0, 0, 0)
    xs = _xadd_stride(xadd, B, C)
    with _Timed("gn_silu_fwd", 0.0, _nbytes(x, y)):
        check(lib.gmk_gn_silu_fwd(_p(x), _p(y), _p(gamma), _p(beta), _p(mean), _p(rstd), B, H * W, C, groups, eps, _p(part), tp, nt,
                                  float(dp), int(dseed), int(doff), _p(xadd), xs, _DT[x.dtype], _s()), "gn_silu_fwd")
    return y, mean, rstd


def gn_stats(x, gamma, beta, groups, tab_scale, tab_shift, eps=1e-5, xadd=None):
    """Statistics-only GroupNorm of x NHWC [B,H,W,C]: fills columns [0, C) of the fp32 table views tab_scale / tab_shift
    ([B, C] slices of a [B, Ctot] table: unit column stride, row stride Ctot) with the affine form of the normalisation,
    y = silu(x * scale + shift), for a convolution that applies it itself (conv_igemm gn=).  -> (mean, rstd)"""
    _chk(x, name="x"); _f32(gamma, "gamma"); _f32(beta, "beta")
    assert x.dtype in _HALF
    B, H, W, C = x.shape
    for t in (tab_scale, tab_shift):
        assert t.dtype == torch.float32 and t.shape == (B, C) and t.stride(1) == 1 and t.is_cuda and t.data_ptr() % 16 == 0
    assert tab_scale.stride(0) == tab_shift.stride(0)
    mean = torch.empty((B, groups), device=x.device, dtype=torch.float32)
    rstd = torch.empty_like(mean)
    xs = _xadd_stride(xadd, B, C)
    with _Timed("gn_stats", 0.0, _nbytes(x)):
        check(lib.gmk_gn_stats(_p(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(tab_scale), _p(tab_shift), tab_scale.stride(0), B, H * W, C,
                               groups, eps, _p(xadd), xs, _DT[x.dtype], _s()), "gn_stats")
    return mean, rstd


def conv_gn_fusable(srcs, cout=128):
    """Can conv_igemm(srcs, ..., 3, NORMAL, gn=...) apply the GroupNorm of its (16-bit) sources itself?"""
    s0 = srcs[0]
    c1 = srcs[1].shape[3] if len(srcs) > 1 else 0
    B, H, W, c0 = s0.shape
    return s0.dtype in _HALF and H * W >= GN_FUSE_MIN_HW and bool(lib.gmk_conv_gn_fusable(B, H, W, c0, c1, cout))


def gn_silu_bwd(dy, x, gamma, beta, mean, rstd, dadd1=None, dadd2=None, dxsum=None, dropout=None, xadd=None):
    """-> (dx, dgamma_part[B,C], dbeta_part[B,C]); dxsum (optional fp32 [B, >=C] view with row stride) is filled.
    x (the saved forward input) may be fp16 next to bf16 gradients (dy, addends, dx)."""
    _chk(x, name="x"); _chk(dy, name="dy")
    assert dy.shape == x.shape and (x.dtype == dy.dtype or (x.dtype == torch.float16 and dy.dtype == torch.bfloat16)), (x.dtype, dy.dtype)
    for t in (dadd1, dadd2):
        if t is not None:
            _chk(t, dy.dtype, "dadd"); assert t.shape == x.shape
    B, H, W, C = x.shape
    G = getattr(mean, "_gn_groups", mean.shape[1])
    dx = torch.empty_like(dy)
    dgp = torch.empty((B, C), device=x.device, dtype=torch.float32)
    dbp = torch.empty_like(dgp)
    stride = 0
    if dxsum is not None:
        assert dxsum.dtype == torch.float32 and dxsum.shape == (B, C) and dxsum.stride(1) == 1
        stride = dxsum.stride(0)
    dp, dseed, doff = dropout if dropout is not None else (0.0, 0, 0)
    xs = _xadd_stride(xadd, B, C)
    with _Timed("gn_silu_bwd", 0.0, _nbytes(dy, x, dadd1, dadd2, dx)):
        check(lib.gmk_gn_silu_bwd(_p(dy), _p(x), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dadd1), _p(dadd2), _p(dx),
                                  _p(dgp), _p(dbp), _p(dxsum), stride, B, H * W, C, G, float(dp), int(dseed), int(doff),
                                  _p(xadd), xs, _DT[dy.dtype], _DT[x.dtype], _s()), "gn_silu_bwd")
    return dx, dgp, dbp


def gn_pair_fwd_ok(x, groups_a, groups_b):
    """True if the GroupNorm + SiLU forward of x's two consumers runs as one launch (gn_silu_fwd_pair)."""
    if not GN_PAIR or groups_a <= 0 or groups_b <= 0 or x.dtype not in _HALF or getattr(x, "_gn_stats", None) is not None:
        return False
    B, H, W, C = x.shape
    return bool(lib.gmk_gn_pair_fwd_ok(H * W, C, groups_a, groups_b, _DT[x.dtype]))


def gn_silu_fwd_pair(x, a, b, eps=1e-5, xadd=None):
    """GroupNorm + SiLU of one x for two consumers, a / b = (gamma, beta, groups): -> ((y_a, mean_a, rstd_a), (y_b, mean_b, rstd_b)), each
    bit-identical to gn_silu_fwd(x, gamma, beta, groups, xadd=xadd) of its own, with x read once.  Shapes: gn_pair_fwd_ok."""
    _chk(x, name="x")
    B, H, W, C = x.shape
    outs, args = [], []
    for gamma, beta, groups in (a, b):
        _f32(gamma, "gamma"); _f32(beta, "beta")
        assert gamma.numel() == C and beta.numel() == C and groups > 0
        y = torch.empty_like(x)
        mean = torch.empty((B, groups), device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        mean._gn_groups = groups
        outs.append((y, mean, rstd))
    xs = _xadd_stride(xadd, B, C)
    (ya, ma, ra), (yb, mb, rb) = outs
    with _Timed("gn_silu_fwd_pair", 0.0, _nbytes(x, ya, yb)):
        check(lib.gmk_gn_silu_fwd_pair(_p(x), _p(ya), _p(yb), _p(a[0]), _p(a[1]), _p(b[0]), _p(b[1]), _p(ma), _p(ra), _p(mb), _p(rb), B, H * W, C,
                                       a[2], b[2], eps, _p(xadd), xs, _DT[x.dtype], _s()), "gn_silu_fwd_pair")
    return outs[0], outs[1]


def gn_pair_ok(x, groups_up, groups_dn, grad_dtype=torch.bfloat16):
    """True if the GroupNorm backward of x's two consumers (groups_up / groups_dn groups) runs as one launch (gn_silu_bwd_pair)."""
    if not GN_PAIR or groups_up <= 0 or groups_dn <= 0 or x.dtype not in _HALF or grad_dtype not in _DT:
        return False
    B, H, W, C = x.shape
    return bool(lib.gmk_gn_pair_ok(H * W, C, groups_up, groups_dn, _DT[x.dtype], _DT[grad_dtype]))


def gn_silu_bwd_pair(x, up, dn, dxsum=None, xadd=None):
    """The backward of x's two GroupNorm + SiLU consumers in one launch.  up / dn = (dy, dadd, gamma, beta, mean, rstd) of the up block's skip
    half and of the down block; -> (dx, (dgp_up, dbp_up), (dgp_dn, dbp_dn)), bit-identical to
        ds, dgp_up, dbp_up = gn_silu_bwd(dy_up, x, ..., dadd1=dadd_up)
        dx, dgp_dn, dbp_dn = gn_silu_bwd(dy_dn, x, ..., dadd1=dadd_dn, dadd2=ds, dxsum=dxsum)
    without ds in HBM and with x read once.  Shapes: gn_pair_ok."""
    _chk(x, name="x")
    B, H, W, C = x.shape
    sides = []
    for dy, dadd, gamma, beta, mean, rstd in (up, dn):
        _chk(dy, torch.bfloat16, "dy"); _chk(dadd, torch.bfloat16, "dadd"); _f32(gamma, "gamma"); _f32(beta, "beta")
        assert dy.shape == x.shape and dadd.shape == x.shape and gamma.numel() == C and beta.numel() == C
        G = getattr(mean, "_gn_groups", mean.shape[1])
        dgp = torch.empty((B, C), device=x.device, dtype=torch.float32)
        sides.append((dy, dadd, gamma, beta, mean, rstd, dgp, torch.empty_like(dgp), G))
    dx = torch.empty_like(sides[1][0])
    stride = 0
    if dxsum is not None:
        assert dxsum.dtype == torch.float32 and dxsum.shape == (B, C) and dxsum.stride(1) == 1
        stride = dxsum.stride(0)
    xs = _xadd_stride(xadd, B, C)
    args = []
    for dy, dadd, gamma, beta, mean, rstd, dgp, dbp, G in sides:
        args += [_p(dy), _p(dadd), _p(gamma), _p(beta), _p(mean), _p(rstd), _p(dgp), _p(dbp), G]
    # (the 32 x 32 instantiation reads dy_dn twice: 7 tensor passes; 6 at 16 x 16)
    with _Timed("gn_silu_bwd_pair", 0.0, _nbytes(x, sides[0][0], sides[0][1], sides[1][0], sides[1][1], dx, sides[1][0] if H * W == 1024 else None)):
        check(lib.gmk_gn_silu_bwd_pair(_p(x), *args, _p(dx), _p(dxsum), stride, B, H * W, C, _p(xadd), xs, _DT[x.dtype], _s()),
              "gn_silu_bwd_pair")
    return dx, (sides[0][6], sides[0][7]), (sides[1][6], sides[1][7])


def cast16(x, dtype):
    """fp16 <-> bf16 copy of a contiguous tensor (numel a multiple of 8)."""
    _chk(x, name="x")
    assert x.dtype in _HALF and dtype in _HALF
    if x.dtype == dtype:
        return x
    out = torch.empty_like(x, dtype=dtype)
    check(lib.gmk_cast16(_p(x), _p(out), x.numel(), _DT[x.dtype], _DT[dtype], _s()), "cast16")
    return out


def chansum(x, out=None):
    _chk(x, name="x")
    B, H, W, C = x.shape
    if out is None:
        out = torch.empty((B, C), device=x.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (B, C) and out.stride(1) == 1
    with _Timed("chansum_kernel", 0.0, _nbytes(x), fixed=True):
        check(lib.gmk_chansum(_p(x), _p(out), out.stride(0), B, H * W, C, _DT[x.dtype], _s()), "chansum")
    return out


_PENDING_COLSUMS = []      # (part, out) pairs deferred into gmk_colsum_multi launches of up to 16


def colsum(part, out, accumulate=False, defer=False):
    """out[c] (+)= sum_r part[r, c]; part fp32 [R, C] with unit column stride, out fp32 [C] (any contiguous view).
    defer=True queues the reduction (same stream order) until flush_colsums(); `part` is kept alive until then."""
    assert part.dtype == torch.float32 and part.dim() == 2 and part.stride(1) == 1 and part.is_cuda
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() == part.shape[1]
    if defer and not accumulate:
        _PENDING_COLSUMS.append((part, out))
        if len(_PENDING_COLSUMS) >= 16:
            flush_colsums()
        return out
    check(lib.gmk_colsum(_p(part), part.stride(0), _p(out), part.shape[0], part.shape[1], int(accumulate), _s()), "colsum")
    return out


def flush_colsums():
    import ctypes
    while _PENDING_COLSUMS:
        batch = _PENDING_COLSUMS[:16]
        del _PENDING_COLSUMS[:16]
        n = len(batch)
        parts = (ctypes.c_void_p * n)(*[b[0].data_ptr() for b in batch])
        outs = (ctypes.c_void_p * n)(*[b[1].data_ptr() for b in batch])
        strides = (ctypes.c_int64 * n)(*[b[0].stride(0) for b in batch])
        Rs = (ctypes.c_int * n)(*[b[0].shape[0] for b in batch])
        Cs = (ctypes.c_int * n)(*[b[0].shape[1] for b in batch])
        check(lib.gmk_colsum_multi(n, ctypes.cast(parts, ctypes.c_void_p), ctypes.cast(strides, ctypes.c_void_p),
                                   ctypes.cast(outs, ctypes.c_void_p), ctypes.cast(Rs, ctypes.c_void_p),
                                   ctypes.cast(Cs, ctypes.c_void_p), _s()), "colsum_multi")


def sumpool2x2(x):
    _chk(x, name="x")
    B, H2, W2, C = x.shape
    assert H2 % 2 == 0 and W2 % 2 == 0
    y = torch.empty((B, H2 // 2, W2 // 2, C), device=x.device, dtype=x.dtype)
    with _Timed("sumpool2x2_kernel", 0.0, _nbytes(x, y), fixed=True):
        check(lib.gmk_sumpool2x2(_p(x), _p(y), B, H2 // 2, W2 // 2, C, _DT[x.dtype], _s()), "sumpool2x2")
    return y


# ---- convolutions ----------------------------------------------------------------------------------------
def out_size(mode, hs, ws):
    if mode == NORMAL:
        return hs, ws
    if mode == STRIDE2:
        return (hs - 1) // 2 + 1, (ws - 1) // 2 + 1
    if mode == UPSAMPLE2:
        return 2 * hs, 2 * ws
    raise ValueError(mode)


def conv_igemm(srcs, w, w_rows, ksize, mode, out_hw, n0=0, cout=128, bias=None, emb=None, residual=None, gn_stats=False, gn=None):
    """srcs: list of 1-2 NHWC tensors (same B,H,W); w: packed weights [taps][w_rows][sum C]; -> out NHWC [B,ho,wo,cout]."""
    s0 = _chk(srcs[0], name="src0")
    s1 = _chk(srcs[1], s0.dtype, "src1") if len(srcs) > 1 else None
    B, hs, ws, c0 = s0.shape
    c1 = 0
    if s1 is not None:
        assert s1.shape[:3] == s0.shape[:3]
        c1 = s1.shape[3]
    _chk(w, s0.dtype, "w")
    assert w.numel() == ksize * ksize * w_rows * (c0 + c1), (w.numel(), ksize, w_rows, c0, c1)
    ho, wo = out_hw
    out = torch.empty((B, ho, wo, cout), device=s0.device, dtype=s0.dtype)
    emb_stride = 0
    if emb is not None:
        assert emb.dtype == torch.float32 and emb.shape == (B, cout) and emb.stride(1) == 1 and emb.data_ptr() % 16 == 0
        emb_stride = emb.stride(0)
        assert emb_stride % 4 == 0
    if bias is not None:
        _f32(bias, "bias"); assert bias.numel() == cout
    if residual is not None:
        _chk(residual, s0.dtype, "residual"); assert residual.shape == out.shape
    gsc = gsh = None
    gstride = 0
    if gn is not None:          # (scale, shift) fp32 [B, c0 + c1] tables of gn_stats: the sources are raw, the kernel normalises them
        gsc, gsh = gn
        for t in (gsc, gsh):
            _f32(t, "gn table"); assert t.shape == (B, c0 + c1)
        gstride = c0 + c1
    mpix = B * hs * ws if mode == TRANSPOSED2 else B * ho * wo     # algorithmic work: that of the stride-2 conv
    part, tp, nt = None, 0, 0
    if gn_stats and GN_STATS and ksize == 3 and mode in (NORMAL, UPSAMPLE2) and s0.dtype == torch.bfloat16 and 4 <= wo <= 254:      # (bf16 only)
        r = 256 // wo
        tp, nt = r * wo, (B * ho + r - 1) // r
        part = torch.empty(nt * 8 * 2 * (cout // 4) * 2, device=s0.device, dtype=torch.float32)
    with _Timed("conv_igemm", 2.0 * mpix * cout * (c0 + c1) * ksize * ksize, _nbytes(s0, s1, residual, out), dtype=s0.dtype):
        check(lib.gmk_conv_igemm(_p(s0), _p(s1), c0, c1, B, hs, ws, ho, wo, ksize, mode, _p(w), w_rows, n0, cout,
                                 _p(bias), _p(emb), emb_stride, _p(residual), _p(out), cout, _p(part),
                                 part.numel() * 4 if part is not None else 0, _p(gsc), _p(gsh), gstride, _DT[s0.dtype], _s()),
              "conv_igemm")
    if part is not None and lib.gmk_last_kernel() == K.CONV_HALO and ho * wo >= 32:      # only the 8-compute-wave halo kernel emits statistics
        out._gn_stats = (part, tp, nt)     # consumed by gn_silu_fwd(out, ...)
    return out


SUBPIXEL_UPSAMPLE, SUBPIXEL_TRANSPOSED, SUBPIXEL_UPSAMPLE_DGRAD = C["GMK_SUBPIXEL_UPSAMPLE"], C["GMK_SUBPIXEL_TRANSPOSED"], C["GMK_SUBPIXEL_UPSAMPLE_DGRAD"]


def conv_subpixel_ok(B, H, W, c, dtype, cout=128):
    """True if the x2 resampling convolutions over the LOW-resolution grid B x H x W run in their sub-pixel form (gmk_conv_subpixel)."""
    return dtype in _HALF and bool(lib.gmk_conv_subpixel_ok(B, H, W, c, cout, _DT[dtype]))


def pack_upsample_weight(w, out, out_dgrad=None):
    """w: fp32 [Cout][Cin][3][3] (a contiguous arena view) -> out: 16 x Cout x Cin elements, the pre-summed 2x2-tap matrices of the sub-pixel
    `Upsample` (reference simple_unet.py:112-122); out_dgrad: their transposes [16][Cin][Cout] for its data gradient.  Either may be None."""
    _f32(w, "w")
    cout, cin = w.shape[0], w.shape[1]
    assert w.shape[2:] == (3, 3) and w.is_contiguous()
    for t in (out, out_dgrad):
        if t is not None:
            _chk(t, name="pack"); assert t.numel() == 16 * cout * cin and t.dtype in _HALF
    ref = out if out is not None else out_dgrad
    check(lib.gmk_pack_upsample_weight(_p(w), _p(out), _p(out_dgrad), cout, cin, _DT[ref.dtype],
                                       _DT[(out_dgrad if out_dgrad is not None else ref).dtype], _s()), "pack_upsample_weight")
    return out


def conv_subpixel(src, w, w_rows, mode, bias=None, residual=None, n0=0, cout=128):
    """SUBPIXEL_UPSAMPLE: low-resolution NHWC src [B,H,W,128] -> conv3x3(nearest x2 (src)) [B,2H,2W,cout], w = the forward pack of
    pack_upsample_weight.  SUBPIXEL_TRANSPOSED: the data gradient of a 3x3 stride-2 convolution (src = its output gradient, w = its ordinary
    data-gradient pack) -> [B,2H,2W,cout].  SUBPIXEL_UPSAMPLE_DGRAD: src = the HIGH-resolution output gradient [B,2H,2W,128] of the upsampled
    convolution -> its input gradient [B,H,W,cout] (w = the out_dgrad pack): sumpool2x2(dgrad3x3(src)) in one launch."""
    s0 = _chk(src, name="src")
    B, H, W, c = s0.shape
    down = mode == SUBPIXEL_UPSAMPLE_DGRAD
    if down:
        assert H % 2 == 0 and W % 2 == 0
        H, W = H // 2, W // 2                  # the C ABI takes the LOW-resolution grid in every mode
    _chk(w, s0.dtype, "w")
    taps = 9 if mode == SUBPIXEL_TRANSPOSED else 16
    assert w.numel() == taps * w_rows * c, (w.numel(), taps, w_rows, c)
    out = torch.empty((B, H, W, cout) if down else (B, 2 * H, 2 * W, cout), device=s0.device, dtype=s0.dtype)
    if bias is not None:
        _f32(bias, "bias"); assert bias.numel() == cout
    if residual is not None:
        _chk(residual, s0.dtype, "residual"); assert residual.shape == out.shape
    # algorithmic work: that of the reference's op (9 taps per HIGH-resolution pixel for the upsampled convolution and its data gradient,
    # 9 per LOW-resolution pixel for the transposed one)
    mpix = B * H * W if mode == SUBPIXEL_TRANSPOSED else B * 4 * H * W
    with _Timed("conv_subpixel", 2.0 * mpix * cout * c * 9, _nbytes(s0, residual, out), multiplied=2.0 * B * H * W * cout * c * taps, dtype=s0.dtype):
        check(lib.gmk_conv_subpixel(_p(s0), B, H, W, c, _p(w), w_rows, n0, cout, mode, _p(bias), _p(residual), _p(out), cout,
                                    _DT[s0.dtype], _s()), "conv_subpixel")
    return out


def conv_skipfold_ok(src, skips):
    """True if conv3x3(src) + conv1x1(cat(skips)) of these shapes runs as one launch (gmk_conv3x3_skipfold)."""
    if not SKIP_FOLD or len(skips) != 2 or src.dtype not in (torch.bfloat16, torch.float16):
        return False
    B, H, W, c0 = src.shape
    return skips[0].shape[3] == skips[1].shape[3] and bool(lib.gmk_conv3x3_skipfold_ok(B, H, W, c0, skips[0].shape[3], 128))


def conv3x3_skipfold(src, w, bias, skips, wsk, bias_sk, cout=128):
    """out = conv3x3(src; w) + bias + conv1x1(cat(skips); wsk) + bias_sk in one launch: the `skip_connection(x) + h` of the up-path
    ResBlocks (reference simple_unet.py:174-186) without the skip output ever reaching HBM."""
    s0 = _chk(src, name="src")
    k0, k1 = _chk(skips[0], s0.dtype, "skip0"), _chk(skips[1], s0.dtype, "skip1")
    B, H, W, c0 = s0.shape
    cs = k0.shape[3]
    assert k0.shape == k1.shape == (B, H, W, cs)
    _chk(w, s0.dtype, "w"); _chk(wsk, s0.dtype, "wsk")
    assert w.numel() == 9 * cout * c0 and wsk.numel() == cout * 2 * cs, (w.numel(), wsk.numel())
    _f32(bias, "bias"); _f32(bias_sk, "bias_sk")
    assert bias.numel() == cout and bias_sk.numel() == cout
    out = torch.empty((B, H, W, cout), device=s0.device, dtype=s0.dtype)
    with _Timed("conv_igemm", 2.0 * B * H * W * cout * (9 * c0 + 2 * cs), _nbytes(s0, k0, k1, out), dtype=s0.dtype):
        check(lib.gmk_conv3x3_skipfold(_p(s0), c0, B, H, W, _p(w), cout, 0, cout, _p(bias), _p(k0), _p(k1), cs, _p(wsk), cout, 0,
                                       _p(bias_sk), _p(out), cout, _DT[s0.dtype], _s()), "conv3x3_skipfold")
    return out


def conv1x1_pair(src, w, w_rows, n0=0):
    """Two 128-channel 1x1 convolutions of one source (packed weight rows n0.. and n0+128..) from one pass over it: the skip
    connection's data gradient for both halves of a concatenated input.  -> (out_a, out_b), NHWC [B,H,W,128] each."""
    s0 = _chk(src, name="src")
    B, H, W, c = s0.shape
    _chk(w, s0.dtype, "w")
    assert w.numel() == w_rows * c and n0 + 256 <= w_rows
    oa = torch.empty((B, H, W, 128), device=s0.device, dtype=s0.dtype)
    ob = torch.empty_like(oa)
    with _Timed("conv_igemm", 2.0 * B * H * W * 256 * c, _nbytes(s0, oa, ob)):
        check(lib.gmk_conv1x1_pair(_p(s0), c, B, H, W, _p(w), w_rows, n0, _p(oa), _p(ob), _DT[s0.dtype], _s()), "conv1x1_pair")
    return oa, ob


_WS = {}


def _workspace(nbytes, device, tag="conv"):
    key = (tag, device.index, _s())
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(int(nbytes), device=device, dtype=torch.uint8)
        _WS[key] = ws
    return ws


def conv_wgrad(dy, srcs, ksize, mode, dw):
    """dw (fp32 [cout][sum C][k][k], a contiguous view into the gradient arena) = weight gradient."""
    _chk(dy, name="dy")
    s0 = _chk(srcs[0], name="src0")
    s1 = _chk(srcs[1], s0.dtype, "src1") if len(srcs) > 1 else None
    assert s0.dtype == dy.dtype or (s0.dtype == torch.float16 and dy.dtype == torch.bfloat16), (s0.dtype, dy.dtype)
    B, hs, ws_, c0 = s0.shape
    c1 = s1.shape[3] if s1 is not None else 0
    _, ho, wo, cout = dy.shape
    assert dy.shape[0] == B
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == cout * (c0 + c1) * ksize * ksize
    need = lib.gmk_conv_wgrad_workspace_bytes(B * ho * wo, ksize * ksize, cout, c0 + c1)
    assert need > 0
    wsbuf = _workspace(need, dy.device)
    with _Timed("conv_wgrad", 2.0 * B * ho * wo * cout * (c0 + c1) * ksize * ksize, _nbytes(dy, s0, s1)):
        check(lib.gmk_conv_wgrad(_p(dy), cout, _p(s0), _p(s1), c0, c1, B, hs, ws_, ho, wo, ksize, mode, _p(dw), cout,
                                 _p(wsbuf), wsbuf.numel(), _DT[dy.dtype], _DT[s0.dtype], _s()), "conv_wgrad")
    return dw


def conv_wgrad_subpixel_ok(B, H, W, c, dy_dtype, cout=128):
    """True if the weight gradient of `Upsample` over the LOW-resolution grid B x H x W runs in its sub-pixel form (gmk_conv_wgrad_subpixel)."""
    return dy_dtype == torch.bfloat16 and bool(lib.gmk_conv_wgrad_subpixel_ok(B, H, W, c, cout))


def conv_wgrad_subpixel(dy, x, dw):
    """dw (fp32 [cout][cin][3][3], a contiguous arena view) = weight gradient of conv3x3(nearest x2 (x)) given the high-resolution output
    gradient dy [B,2H,2W,cout] (bf16) and the saved low-resolution input x [B,H,W,cin] (bf16 / fp16)."""
    _chk(dy, torch.bfloat16, "dy")
    _chk(x, name="x")
    assert x.dtype in _HALF
    B, H, W, cin = x.shape
    cout = dy.shape[3]
    assert dy.shape == (B, 2 * H, 2 * W, cout)
    assert dw.dtype == torch.float32 and dw.is_contiguous() and dw.numel() == cout * cin * 9
    need = lib.gmk_conv_wgrad_subpixel_workspace_bytes(B, H, W, cin, cout)
    assert need > 0
    wsbuf = _workspace(need, dy.device)
    with _Timed("conv_wgrad", 2.0 * B * 4 * H * W * cout * cin * 9, _nbytes(dy, x), multiplied=2.0 * B * H * W * cout * cin * 16):
        check(lib.gmk_conv_wgrad_subpixel(_p(dy), cout, _p(x), B, H, W, cin, cout, _p(dw), _p(wsbuf), wsbuf.numel(), _DT[dy.dtype],
                                          _DT[x.dtype], _s()), "conv_wgrad_subpixel")
    return dw


def stem_fwd(x, w, bias, C, dtype):
    _f32(x, "x"); _f32(w, "w"); _f32(bias, "bias")
    B, cin, H, W = x.shape
    assert w.shape == (C, cin, 3, 3)
    y = torch.empty((B, H, W, C), device=x.device, dtype=dtype)
    with _Timed("stem_fwd", 2.0 * B * H * W * C * cin * 9, _nbytes(x, y)):
        check(lib.gmk_stem_fwd(_p(x), _p(w), _p(bias), _p(y), B, cin, H, W, C, _DT[dtype], _s()), "stem_fwd")
    return y


def stem_wgrad(x, dy, dw):
    _f32(x, "x"); _chk(dy, name="dy")
    B, cin, H, W = x.shape
    C = dy.shape[3]
    nb = lib.gmk_stem_wgrad_blocks(B * H * W)
    part = torch.empty((nb, C * cin * 9), device=x.device, dtype=torch.float32)
    with _Timed("stem_wgrad", 2.0 * B * H * W * C * cin * 9, _nbytes(x, dy)):
        check(lib.gmk_stem_wgrad(_p(x), _p(dy), _p(part), B, cin, H, W, C, _DT[dy.dtype], _s()), "stem_wgrad")
    return colsum(part, dw)


def head_fwd(a, w, bias):
    _chk(a, name="a"); _f32(w, "w"); _f32(bias, "bias")
    B, H, W, C = a.shape
    cout = w.shape[0]
    assert w.shape == (cout, C, 3, 3)
    out = torch.empty((B, cout, H, W), device=a.device, dtype=torch.float32)
    with _Timed("head_fwd", 2.0 * B * H * W * C * cout * 9, _nbytes(a, out)):
        check(lib.gmk_head_fwd(_p(a), _p(w), _p(bias), _p(out), B, cout, H, W, C, _DT[a.dtype], _s()), "head_fwd")
    return out


def head_dgrad(dout, w, dtype):
    _f32(dout, "dout"); _f32(w, "w")
    B, cout, H, W = dout.shape
    C = w.shape[1]
    da = torch.empty((B, H, W, C), device=dout.device, dtype=dtype)
    with _Timed("head_dgrad", 2.0 * B * H * W * C * cout * 9, _nbytes(dout, da)):
        check(lib.gmk_head_dgrad(_p(dout), _p(w), _p(da), B, cout, H, W, C, _DT[dtype], _s()), "head_dgrad")
    return da


def head_wgrad(dout, a, dwb):
    """dwb: contiguous fp32 view of [weight (cout*C*9) | bias (cout)] in the gradient arena."""
    _f32(dout, "dout"); _chk(a, name="a")
    B, cout, H, W = dout.shape
    C = a.shape[3]
    n = cout * C * 9 + cout
    assert dwb.numel() == n
    nb = lib.gmk_head_wgrad_blocks(B * H * W)
    part = torch.empty((nb, n), device=a.device, dtype=torch.float32)
    with _Timed("head_wgrad", 2.0 * B * H * W * C * cout * 9, _nbytes(dout, a)):
        check(lib.gmk_head_wgrad(_p(dout), _p(a), _p(part), B, cout, H, W, C, _DT[a.dtype], _s()), "head_wgrad")
    return colsum(part, dwb)


def add_into(a, b):
    """a += b in place (gmk_add_into): two gradient tensors of one shape and type (fp32 or bf16), a multiple of 8 elements.  -> a"""
    _chk(a, name="a"); _chk(b, a.dtype, "b")
    if a.shape != b.shape or a.numel() % 8 or a.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"add_into: shapes {tuple(a.shape)} and {tuple(b.shape)} of {a.dtype}: one shape, a multiple of 8 elements, fp32 or bf16")
    check(lib.gmk_add_into(_p(a), _p(b), a.numel(), _DT[a.dtype], _s()), "add_into")
    return a


def stem_dgrad(dy, w):
    """The network's input gradient through the stem: dy NHWC [B, H, W, C] (compute dtype) -> dx NCHW fp32 [B, cin, H, W], the transposed 3x3
    convolution with the stem weight w [C, cin, 3, 3] (gmk_stem_dgrad; an extension)."""
    if dy.dim() != 4 or w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] != dy.shape[3]:
        raise ValueError(f"stem_dgrad: bad shapes dy {tuple(dy.shape)} and w {tuple(w.shape)}: expected [B, H, W, C] and [C, cin, 3, 3]")
    if dy.dtype not in _DT:
        raise ValueError(f"stem_dgrad: dy dtype {dy.dtype}")
    _f32(w, "w"); _chk(dy, name="dy")
    B, H, W, C = dy.shape
    cin = w.shape[1]
    dx = torch.empty((B, cin, H, W), device=dy.device, dtype=torch.float32)
    with _Timed("stem_dgrad", 2.0 * B * H * W * C * cin * 9, _nbytes(dy, dx)):
        check(lib.gmk_stem_dgrad(_p(dy), _p(w), _p(dx), B, cin, H, W, C, _DT[dy.dtype], _s()), "stem_dgrad")
    return dx


# ---- embedding path --------------------------------------------------------------------------------------
def timestep_freqs(max_period, device):
    """simple_unet.py:215-219 evaluated with the same torch fp32 ops (host), as a 32-entry table."""
    half = 32
    return torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half).to(device)


def timestep_embedding(t, freqs):
    _f32(t, "t"); _f32(freqs, "freqs")
    B = t.numel()
    out = torch.empty((B, 64), device=t.device, dtype=torch.float32)
    check(lib.gmk_timestep_embedding(_p(t), _p(freqs), _p(out), B, _s()), "timestep_embedding")
    return out


def guide_onehot(guide):
    _chk(guide, torch.int64, "guide")
    B = guide.numel()
    onehot = torch.empty((B, 10), device=guide.device, dtype=torch.float32)
    keep = torch.empty((B,), device=guide.device, dtype=torch.float32)
    check(lib.gmk_guide_onehot(_p(guide), _p(onehot), _p(keep), B, _s()), "guide_onehot")
    return onehot, keep


def label_drop(y, p, seed, offset):
    """In place: y[b] = -1 where rng_uniform((B,), seed, offset)[b] < p (diffusion_model.py:67)."""
    seed, offset = check_stream(seed, offset)
    _chk(y, torch.int64, "y")
    check(lib.gmk_label_drop(_p(y), y.numel(), float(p), seed, offset, _s()), "label_drop")
    return y


def batch_gather(images, labels, index, *, pad, binarize, flip_p=0.0, seed=0, offset=0, trusted=False):
    """-> (x fp32 [B, C, H + 2 pad, W + 2 pad], y int64 [B]), both FRESH on every call (train_step overwrites y in place): the transform chain
    of data.transform on images[index] (uint8 [N, C, H, W] on the device), a zero border of `pad` pixels, and a mirror along W of the images
    whose element of rng_uniform((B,), seed, offset) is below flip_p; y = labels[index] (uint8 [N]).  Unless `trusted`, 0 <= index < N is
    checked with one host sync and a violation raises before anything is launched."""
    seed, offset = check_stream(seed, offset)
    for t, dtype, name in ((images, torch.uint8, "images"), (labels, torch.uint8, "labels"), (index, torch.int64, "index")):
        if not t.is_cuda:
            raise ValueError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
        if t.dtype != dtype:
            raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
        if not t.is_contiguous():
            raise ValueError(f"{name}: must be contiguous")
        if t.device != images.device:
            raise ValueError(f"{name}: on {t.device}, images on {images.device}")
    if images.dim() != 4 or labels.dim() != 1 or index.dim() != 1 or labels.shape[0] != images.shape[0] or index.numel() == 0 or images.numel() == 0:
        raise ValueError(f"batch_gather: images {tuple(images.shape)} (want [N, C, H, W]), labels {tuple(labels.shape)} (want [N]), "
                         f"index {tuple(index.shape)} (want [B], B > 0)")
    pad, binarize, flip_p = int(pad), int(binarize), float(flip_p)
    if pad < 0 or binarize not in (0, 1) or not 0.0 <= flip_p <= 1.0:
        raise ValueError(f"batch_gather: pad = {pad} (>= 0), binarize = {binarize} (0 or 1), flip_p = {flip_p} (in [0, 1])")
    N, C, H, W = images.shape
    B = index.numel()
    if not trusted:
        lo, hi = (int(v) for v in torch.stack((index.min(), index.max())).tolist())      # one sync
        if lo < 0 or hi >= N:
            raise ValueError(f"batch_gather: index values span [{lo}, {hi}], the dataset has {N} images")
    x = torch.empty((B, C, H + 2 * pad, W + 2 * pad), device=images.device, dtype=torch.float32)
    y = torch.empty((B,), device=images.device, dtype=torch.int64)
    with _Timed("batch_gather_kernel", 0.0, _nbytes(x, y) + float(B * C * H * W + B), fixed=True):
        check(lib.gmk_batch_gather(_p(images), _p(labels), _p(index), B, N, C, H, W, pad, binarize, flip_p, seed, offset, _p(x), _p(y), _s()),
              "batch_gather")
    return x, y


def _image_source(x, ranks, crop, what):
    """The checks ops.to_uint8 and ops.image_grid share -> (x contiguous and 16-byte aligned, crop).  A slice or a misaligned view is copied,
    not rejected."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError(f"{what}: x dtype {getattr(x, 'dtype', type(x))}, expected {torch.float32}")
    if not x.is_cuda:
        raise ValueError(f"{what}: x: expected a device tensor (the HIP path has no CPU fallback)")
    if x.dim() not in ranks:
        raise ValueError(f"{what}: x of rank {x.dim()}, shape {tuple(x.shape)} (want {' or '.join(ranks.values())})")
    if x.numel() == 0:
        raise ValueError(f"{what}: x of shape {tuple(x.shape)} is empty")
    H, W = x.shape[-2:]
    if isinstance(crop, bool) or crop != int(crop) or int(crop) < 0 or 2 * int(crop) >= min(H, W):
        raise ValueError(f"{what}: crop = {crop} of {H} x {W} images (want 0 <= 2 crop < min(H, W))")
    return aligned(x), int(crop)


def to_uint8(x, crop=0):
    """-> uint8 x.shape[:-2] + (H - 2 crop, W - 2 crop), FRESH on every call: ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8) of
    x[..., crop:H - crop, crop:W - crop] (fp32 [..., H, W] on the device, rank >= 2) in one pass - the bits of that torch chain, NaN -> 0."""
    x, crop = _image_source(x, {r: f"rank {r}" for r in range(2, 9)}, crop, "to_uint8")
    H, W = x.shape[-2:]
    planes = x.numel() // (H * W)
    out = torch.empty(tuple(x.shape[:-2]) + (H - 2 * crop, W - 2 * crop), device=x.device, dtype=torch.uint8)
    with _Timed("to_uint8_kernel", 0.0, _nbytes(out) + 4.0 * out.numel(), fixed=True):
        check(lib.gmk_to_uint8(_p(x), _p(out), planes, 1, H, W, crop, _s()), "to_uint8")
    return out


def image_grid(x, *, ncol, crop=0, gap=2, fill=0, out_channels=None, row_prefix=0):
    """x fp32 [N, C, H, W] -> uint8 [GH, row], or [T, N, C, H, W] -> [T, GH, row], FRESH on every call: the images quantised as in to_uint8,
    cropped and tiled `ncol` to a line with `gap` pixels of the byte `fill` around and between them (include/gmk.h: gmk_image_grid).
    C 1 or 3; out_channels: C (default), or 3 with C = 1.  row = row_prefix + GW out_channels bytes, channels interleaved; row_prefix 1 puts
    PNG's filter byte 0 in front of every line (pngio.encode_png takes that buffer as it is)."""
    x, crop = _image_source(x, {4: "[N, C, H, W]", 5: "[T, N, C, H, W]"}, crop, "image_grid")
    single = x.dim() == 4
    T, (N, C, H, W) = (1 if single else x.shape[0]), x.shape[-4:]
    if C not in (1, 3):
        raise ValueError(f"image_grid: C = {C} channels (1 or 3)")
    out_channels = C if out_channels is None else out_channels
    if out_channels not in (1, 3) or (out_channels != C and C != 1):
        raise ValueError(f"image_grid: out_channels = {out_channels} with C = {C} (C, or 3 with C = 1)")
    for name, val, lo, hi in (("ncol", ncol, 1, 1 << 20), ("gap", gap, 0, 1024), ("fill", fill, 0, 255), ("row_prefix", row_prefix, 0, 1)):
        if isinstance(val, bool) or not isinstance(val, int) or not lo <= val <= hi:
            raise ValueError(f"image_grid: {name} = {val!r}: an integer in [{lo}, {hi}]")
    nrow = -(-N // ncol)
    GH, GW = gap + nrow * (H - 2 * crop + gap), gap + ncol * (W - 2 * crop + gap)
    out = torch.empty((T, GH, row_prefix + GW * out_channels), device=x.device, dtype=torch.uint8)
    with _Timed("image_grid_kernel", 0.0, _nbytes(out) + 4.0 * T * N * C * (H - 2 * crop) * (W - 2 * crop), fixed=True):
        check(lib.gmk_image_grid(_p(x), _p(out), T, N, C, H, W, crop, ncol, gap, fill, out_channels, row_prefix, _s()), "image_grid")
    return out[0] if single else out


def mean(x):
    """0-dim fp32 mean of a contiguous fp32 vector (fixed summation order)."""
    _f32(x, "x")
    out = torch.empty((), device=x.device, dtype=torch.float32)
    check(lib.gmk_mean(_p(x), x.numel(), _p(out), _s()), "mean")
    return out


def gemm(A, B, out=None, bias=None, rowscale=None, silu_a=False, silu_b=False, accumulate=False, bias2=None):
    """out[M,N] (+)= rowscale * (bias + bias2 + fa(A) @ fb(B)) for 2-D fp32 views A [M,K], B [K,N] with arbitrary strides."""
    assert A.dtype == torch.float32 and B.dtype == torch.float32 and A.is_cuda and B.is_cuda
    M, K = A.shape
    K2, N = B.shape
    assert K == K2
    if out is None:
        assert not accumulate
        out = torch.empty((M, N), device=A.device, dtype=torch.float32)
    assert out.dtype == torch.float32 and out.shape == (M, N) and out.stride(1) == 1
    for bv in (bias, bias2):
        if bv is not None:
            assert bv.dtype == torch.float32 and bv.numel() == N and bv.is_contiguous()
    if rowscale is not None:
        assert rowscale.dtype == torch.float32 and rowscale.numel() == M and rowscale.is_contiguous()
    need = lib.gmk_gemm_f32_workspace_bytes(M, N, K)
    wsb = _workspace(need, A.device, "gemm") if need else None
    check(lib.gmk_gemm_f32(_p(A), A.stride(0), A.stride(1), _p(B), B.stride(0), B.stride(1), _p(out), out.stride(0), M, N, K,
                           _p(bias), _p(bias2), _p(rowscale), int(silu_a) | (int(silu_b) << 1), int(accumulate), _p(wsb), need, _s()),
          "gemm_f32")
    return out


def silu_bwd(dpost, pre, rowscale=None):
    _f32(dpost, "dpost"); _f32(pre, "pre")
    assert dpost.shape == pre.shape
    out = torch.empty_like(pre)
    check(lib.gmk_silu_bwd(_p(dpost), _p(pre), _p(rowscale), _p(out), pre.numel(), pre.shape[-1], _s()), "silu_bwd")
    return out


def scale_rows(x, rowscale):
    _f32(x, "x"); _f32(rowscale, "rowscale")
    out = torch.empty_like(x)
    check(lib.gmk_scale_rows(_p(x), _p(rowscale), _p(out), x.numel(), x.shape[-1], _s()), "scale_rows")
    return out


# ---- diffusion algebra -----------------------------------------------------------------------------------
def rng_normal(shape, seed, offset, device):
    seed, offset = check_stream(seed, offset)
    out = torch.empty(shape, device=device, dtype=torch.float32)
    check(lib.gmk_rng_normal(_p(out), out.numel(), seed, offset, _s()), "rng_normal")
    return out


def rng_uniform(shape, seed, offset, device):
    seed, offset = check_stream(seed, offset)
    out = torch.empty(shape, device=device, dtype=torch.float32)
    check(lib.gmk_rng_uniform(_p(out), out.numel(), seed, offset, _s()), "rng_uniform")
    return out


SCHEDULES = {"cosine": C["GMK_SCHED_COSINE"], "uniform": C["GMK_SCHED_UNIFORM"], "beta_const": C["GMK_SCHED_BETA_CONST"],
             "beta_linear": C["GMK_SCHED_BETA_LINEAR"]}       # the closed-form log-SNR schedules (diffusion_utils.py:169-201)


@functools.lru_cache(maxsize=64)
def _sched_args(schedule):
    """The (kind, a, b, lmin, lmax, shift) arguments of the gmk_*_sched entries from a `gaussian_diffusion.Schedule` (its kind, the fp32
    coefficients a, b it derived, its range and shift); kept per schedule (an immutable tuple): this sits on every training launch's path."""
    if schedule.kind not in SCHEDULES:
        raise ValueError(f"schedule kind {schedule.kind!r}: one of {', '.join(SCHEDULES)}")
    return (SCHEDULES[schedule.kind], float(schedule.a), float(schedule.b), float(schedule.logsnr_min), float(schedule.logsnr_max),
            float(schedule.shift))


def q_sample(x, eps, u, schedule=None):
    """-> (logsnr, z): logsnr = schedule(u), z = alpha x + sigma eps.  schedule: a `gaussian_diffusion.Schedule` (gmk_q_sample_sched, any
    image size), None: the reference's cosine schedule on [-20, 20] (gmk_q_sample, as ever)."""
    _f32(x, "x"); _f32(eps, "eps"); _f32(u, "u")
    B = x.shape[0]
    n = x.numel() // B
    assert eps.shape == x.shape and u.numel() == B
    logsnr = torch.empty((B,), device=x.device, dtype=torch.float32)
    z = torch.empty_like(x)
    if schedule is None:
        check(lib.gmk_q_sample(_p(x), _p(eps), _p(u), _p(logsnr), _p(z), B, n, _s()), "q_sample")
    else:
        check(lib.gmk_q_sample_sched(_p(x), _p(eps), _p(u), _p(logsnr), _p(z), B, n, *_sched_args(schedule), _s()), "q_sample_sched")
    return logsnr, z


MEAN_TYPES = {"v": C["GMK_MEAN_V"], "eps": C["GMK_MEAN_EPS"], "x": C["GMK_MEAN_X"]}      # what the network output parametrises (gaussian_diffusion.py:58-73)


def _loss_front(what, images, vectors, mean_type, aligned16=False):
    """What the four loss wrappers ask of their tensors, after their own scalars: a known mean type, then `_images` - images: (tensor, name)
    pairs of one fp32 shape [B, ...], vectors: (tensor, name) pairs of fp32 [B], all contiguous device tensors; aligned16: also 16-byte
    aligned (`v_loss`, as ever; its siblings take other tensors on their scalar path).  -> (B, values per image)"""
    if mean_type not in MEAN_TYPES:
        raise ValueError(f"mean_type {mean_type!r}: expected one of {sorted(MEAN_TYPES)}")
    B, n = _images(images, tuple((t, nm, torch.float32) for t, nm in vectors), what)
    for t, nm in (images + vectors) if aligned16 else ():
        if t.data_ptr() % 16:
            raise ValueError(f"{nm}: data pointer not 16-byte aligned")
    return B, n


def _loss_call(what, inputs, n_out, wrt, grad_scale, scalars, mean_type, B, n):
    """The four loss wrappers' tail: n_out per-image fp32 [B] outputs, a gradient like each tensor of `wrt` iff grad_scale is given, and the call
    gmk_<what>(inputs, outputs, gradients, grad_scale, scalars, mean type, B, n, stream).  -> (outputs ..., gradients or Nones ...)"""
    outs = tuple(torch.empty((B,), device=inputs[0].device, dtype=torch.float32) for _ in range(n_out))
    grads = tuple(torch.empty_like(t) if grad_scale is not None else None for t in wrt)
    check(getattr(lib, "gmk_" + what)(*map(_p, inputs + outs + grads), float(grad_scale or 0.0), *scalars, MEAN_TYPES[mean_type], B, n, _s()), what)
    return outs + grads


def v_loss(v, z, x, eps, logsnr, grad_scale=None, loss_type=0, mean_type="v"):
    """-> (loss_b, x_mse, eps_mse, dv or None).  loss_type 0 'snr_trunc', 1 'snr'."""
    B, n = _loss_front("v_loss", ((x, "x"), (v, "v"), (z, "z"), (eps, "eps")), ((logsnr, "logsnr"),), mean_type, aligned16=True)
    return _loss_call("v_loss", (v, z, x, eps, logsnr), 3, (v,), grad_scale, (loss_type,), mean_type, B, n)


def hybrid_loss(v, nu, z, x, eps, logsnr, logsnr_s, vlb_lambda, grad_scale=None, loss_type=0, mean_type="v"):
    """The hybrid loss of a learned reverse-process variance (gmk_hybrid_loss; Nichol & Dhariwal 2021, section 3.1; an extension): `v_loss`'s simple
    loss (its x_mse, eps_mse and dv bits) plus vlb_lambda times the bound term vlb_b = mean_i KL(q(z_s | z_t, x) || p(z_s | z_t)) in nats per
    dimension, p with the per-element 'medium' fraction f = (nu + 1) / 2 and the mean held constant.  v, nu, z, x, eps: fp32 [B, ...], contiguous
    (16-byte aligned tensors with n % 4 == 0 take the 16-byte path, anything else the scalar one); logsnr, logsnr_s: fp32 [B], logsnr_s >= logsnr
    the log-SNR one step of the bound's grid earlier.  -> (loss_b, vlb_b, frac_b, x_mse, eps_mse, dv or None, dnu or None), the gradients of
    grad_scale sum_b loss_b when grad_scale is given."""
    if loss_type not in (0, 1):
        raise ValueError(f"loss_type {loss_type!r}: 0 (snr_trunc) or 1 (snr)")
    lam = float(vlb_lambda)
    if not (math.isfinite(lam) and lam >= 0.0):
        raise ValueError(f"vlb_lambda = {lam}: need a finite value >= 0")
    B, n = _loss_front("hybrid_loss", ((x, "x"), (v, "v"), (nu, "nu"), (z, "z"), (eps, "eps")), ((logsnr, "logsnr"), (logsnr_s, "logsnr_s")), mean_type)
    return _loss_call("hybrid_loss", (v, nu, z, x, eps, logsnr, logsnr_s), 5, (v, nu), grad_scale, (lam, loss_type), mean_type, B, n)


X_LOSS_WEIGHTS = {"snr_plus1": C["GMK_LOSS_W_SNR_PLUS1"], "min_snr": C["GMK_LOSS_W_MIN_SNR"]}      # the weightings gmk_x_loss_w evaluates
X_LOSS_KEEP = C["GMK_X_LOSS_KEEP"]      # images of up to this many values keep their residuals in LDS, larger ones are re-read


def x_loss_w(v, z, x, logsnr, weight, gamma, grad_scale=None, mean_type="v"):
    """Weighted x-space loss (gmk_x_loss_w; an extension): loss_b = w(logsnr) x_mse with weight 'snr_plus1' (w = 1 + e^logsnr, Salimans & Ho
    2022) or 'min_snr' (w = min(e^logsnr, gamma), Hang et al. 2023), x_mse = mean (x_hat - x)^2 of the clipped prediction - the bits of
    `v_loss`'s x_mse.  v, z, x: fp32 [B, ...], contiguous (16-byte aligned tensors with n % 4 == 0 take the 16-byte path, anything else the
    scalar one); logsnr: fp32 [B].  -> (loss_b, x_mse, dv or None), dv = d(grad_scale sum_b loss_b)/dv when grad_scale is given."""
    if weight not in X_LOSS_WEIGHTS:
        raise ValueError(f"weight {weight!r}: expected one of {sorted(X_LOSS_WEIGHTS)}")
    gamma = float(gamma)
    if not (math.isfinite(gamma) and gamma > 0.0):
        raise ValueError(f"gamma = {gamma}: need a finite value > 0")
    B, n = _loss_front("x_loss_w", ((x, "x"), (v, "v"), (z, "z")), ((logsnr, "logsnr"),), mean_type)
    return _loss_call("x_loss_w", (v, z, x, logsnr), 2, (v,), grad_scale, (X_LOSS_WEIGHTS[weight], gamma), mean_type, B, n)


def u_stratified(u0, B):
    """Low-discrepancy times (gmk_u_stratified; Kingma et al. 2021, VDM, App. I.1): u[b] = frac(u0 + b / B) in fp32 from ONE uniform draw u0
    (fp32, one element, on the device); exactly one u in every [k / B, (k + 1) / B) when B is a power of two and u0 a multiple of 2^-24
    (`rng_uniform`'s values), in [0, 1) for every B.  -> fp32 [B]"""
    _f32(u0, "u0")
    B = int(B)
    if u0.numel() != 1 or not 1 <= B <= 1 << 24:
        raise ValueError(f"u_stratified: u0 of {u0.numel()} values, B = {B}: one offset and 1 <= B <= 2^24")
    u = torch.empty((B,), device=u0.device, dtype=torch.float32)
    check(lib.gmk_u_stratified(_p(u0), _p(u), B, _s()), "u_stratified")
    return u


PROFILE_BINS = C["GMK_PROFILE_BINS"]      # bins of equal width in u, one per lane of a wavefront


def _profile_state(state):
    _f32(state, "state")
    if tuple(state.shape) != (5, PROFILE_BINS):
        raise ValueError(f"state: shape {tuple(state.shape)}, expected (5, {PROFILE_BINS}) (W, then S1 and S2 of two value channels)")
    return state


def loss_profile(u, v0, v1, state, decay):
    """Add one batch to a per-time loss profile (gmk_loss_profile; an extension), in place: sample b falls into bin min(int(64 u[b]), 63) and is
    skipped when u[b] is outside [0, 1) or a value is not finite; a bin that received n samples takes W = decay W + n, S1 = decay S1 + sum v,
    S2 = decay S2 + sum v^2 per value channel (v0 -> rows 1, 2; v1 -> rows 3, 4, untouched when v1 is None), every other bin keeps its bits.
    u, v0, v1: fp32 [B], 1 <= B <= 2^24; state: fp32 [5, 64]; 0 < decay <= 1.  Sequential fp32 sums in ascending b, no atomics: the same
    inputs give the same bits.  -> state"""
    _profile_state(state)
    _f32(u, "u"); _f32(v0, "v0")
    B = u.numel()
    if not 1 <= B <= 1 << 24:
        raise ValueError(f"loss_profile: {B} samples, 1 <= B <= 2^24")
    for t, nm in ((u, "u"), (v0, "v0"), (v1, "v1")):
        if t is not None and (_f32(t, nm).numel() != B or t.device != state.device):
            raise ValueError(f"loss_profile: {nm} of {t.numel()} values on {t.device}, u has {B} and the state is on {state.device}")
    decay = float(decay)
    if not 0.0 < decay <= 1.0:
        raise ValueError(f"loss_profile: decay = {decay} outside (0, 1]")
    check(lib.gmk_loss_profile(_p(u), _p(v0), _p(v1), B, decay, _p(state), _s()), "loss_profile")
    return state


def u_importance(state, u0, warm, floor, want_table=False):
    """Loss-aware times (gmk_u_importance; Nichol & Dhariwal 2021, section 3.3): the uniform draws u0 (fp32 [B] in [0, 1)) through the inverse
    CDF of p_k = (1 - floor) r_k / sum r + floor / 64, r_k = sqrt(S2_k / W_k) of the profile `state`'s channel 0, and the importance weights
    w = C / (64 p_k) of the bins they land in.  While a bin holds fewer than `warm` samples (or the profile has no finite positive mass) the
    table is uniform: u == u0 bit for bit and w == 1.  warm >= 0, 0 < floor <= 1.
    -> (u, w), fp32 [B]; with want_table also the table's (p, w), fp32 [64] each."""
    _profile_state(state)
    _f32(u0, "u0")
    B = u0.numel()
    if u0.dim() != 1 or not 1 <= B <= 1 << 24 or u0.device != state.device:
        raise ValueError(f"u_importance: u0 of shape {tuple(u0.shape)} on {u0.device}: a vector of 1 <= B <= 2^24 draws on the state's device")
    warm, floor = float(warm), float(floor)
    if not warm >= 0.0:
        raise ValueError(f"u_importance: warm = {warm}, need a sample count >= 0")
    if not 0.0 < floor <= 1.0:
        raise ValueError(f"u_importance: floor = {floor} outside (0, 1]")
    u, w = torch.empty_like(u0), torch.empty_like(u0)
    p_t = torch.empty((PROFILE_BINS,), device=u0.device, dtype=torch.float32) if want_table else None
    w_t = torch.empty_like(p_t) if want_table else None
    check(lib.gmk_u_importance(_p(state), _p(u0), _p(u), _p(w), B, warm, floor, _p(p_t), _p(w_t), _s()), "u_importance")
    return (u, w, p_t, w_t) if want_table else (u, w)


def _sampler_check(v, z, same_shape, cond_w):
    """The input checks `sampler_step`, `dpm_solver_step` and `dyn_threshold` share.  same_shape: (tensor or None, name) pairs of z's shape.
    -> (B, n)"""
    _f32(v, "v"); _f32(z, "z")
    B = z.shape[0]
    n = z.numel() // B
    assert v.shape == z.shape
    for t, nm in same_shape:
        if t is not None:
            _f32(t, nm); assert t.shape == z.shape
    if cond_w is not None:
        _f32(cond_w, "cond_w"); assert cond_w.numel() == B
    return B, n


def _sampler_io(v, z, same_shape, cond_w, want_pred, dup, logsnr_next):
    """The checks and outputs `sampler_step` and `dpm_solver_step` share.  same_shape: as in `_sampler_check`.
    -> (B, n, z_next, z2 (None without dup), x_pred, eps_pred)"""
    B, n = _sampler_check(v, z, same_shape, cond_w)
    z2 = torch.empty((2 * B,) + tuple(z.shape[1:]), device=z.device, dtype=z.dtype) if dup else None
    z_next = z2[:B] if dup else torch.empty_like(z)
    xp = torch.empty_like(z) if want_pred else None
    ep = torch.empty_like(z) if want_pred else None
    if logsnr_next is not None:
        _f32(logsnr_next, "logsnr_next"); assert logsnr_next.numel() == (2 * B if dup else B)
    return B, n, z_next, z2, xp, ep


def _sampler_ret(z_next, z2, xp, ep):
    """What every update wrapper returns from `_sampler_io`'s outputs: (z_next, or (z_next, z2) with dup), x_pred, eps_pred."""
    return (z_next if z2 is None else (z_next, z2)), xp, ep


def _drawn_scalars(name, z, mean_type, scalars):
    """The first checks of the updates that draw their noise in the kernel (`consistency_step`, `stochastic_step`, `stochastic_step_lv`), ahead
    of each wrapper's own sign rules: mean_type, z's shape [B, ...], n % 4, the scalars (times and coefficients) finite.  -> scalars as floats"""
    if mean_type not in MEAN_TYPES:
        raise ValueError(f"mean_type {mean_type!r}: expected one of {sorted(MEAN_TYPES)}")
    shape = tuple(z.shape)
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f"z: bad shape {shape}, expected [B, ...] with B and every image dimension > 0")
    if math.prod(shape[1:]) % 4:
        raise ValueError(f"z: {math.prod(shape[1:])} values per image, a multiple of 4 is required")
    scalars = tuple(float(s) for s in scalars)
    if not all(math.isfinite(s) for s in scalars):
        raise ValueError(f"{name}: non-finite time or coefficient {scalars}")
    return scalars


def _drawn_stream(name, seed, offset, q0, v_uncond, cond_w):
    """Their checks after the sign rules, before any device tensor is asked for: the Philox stream, q0, v_uncond with cond_w.  -> (seed, offset, q0)"""
    seed, offset = check_stream(seed, offset)
    q0 = int(q0)
    if not 0 <= q0 < 1 << 64:
        raise ValueError(f"q0 = {q0}: an unsigned 64-bit Philox counter offset")
    if (v_uncond is None) != (cond_w is None):
        raise ValueError(f"{name}: v_uncond and cond_w go together")
    return seed, offset, q0


def _thr_check(thr, B):
    """`thr` of the *_dt entries: fp32 [B], the per-image threshold `dyn_threshold` returns."""
    _f32(thr, "thr")
    if thr.dim() != 1 or thr.numel() != B:
        raise ValueError(f"thr: shape {tuple(thr.shape)}, expected ({B},)")
    return thr


def box_geometry(shape, cf, N):
    """The box-mean operator A of DDNM restoration (gmk_box_mean) on images of `shape` = [B, C, H, W]: cf in {1, C} channels averaged together,
    an N x N spatial box.  -> (B, C, H, W, cf, N, low-resolution shape [B, C / cf, H / N, W / N]), or ValueError."""
    if len(shape) != 4 or 0 in shape:
        raise ValueError(f"box operator: shape {tuple(shape)}, expected [B, C, H, W] with every dimension > 0")
    B, C, H, W = (int(d) for d in shape)
    if isinstance(cf, bool) or isinstance(N, bool) or int(cf) != cf or int(N) != N:
        raise ValueError(f"box operator: cf = {cf!r}, N = {N!r}: integers")
    cf, N = int(cf), int(N)
    if cf not in (1, C):
        raise ValueError(f"box operator: cf = {cf}, the channels averaged together: 1 or C = {C}")
    if N < 1 or H % N or W % N:
        raise ValueError(f"box operator: N = {N} does not divide H = {H} and W = {W}")
    low = (B, C // cf, H // N, W // N)
    if C * H * W >= 1 << 31 or math.prod(low) >= 1 << 31:
        raise ValueError(f"box operator: shape {tuple(shape)} has 2^31 or more values per image, or boxes per batch")
    return B, C, H, W, cf, N, low


def box_mean(x, cf, N):
    """A x of DDNM restoration (gmk_box_mean; an extension): x fp32 [B, C, H, W] -> fp32 [B, C / cf, H / N, W / N], each value the mean of a
    box of cf channels x N x N pixels: the sequential fp32 sum of the members in (dc, dy, dx) order, divided by k = cf N^2."""
    _f32(x, "x")
    B, C, H, W, cf, N, low = box_geometry(tuple(x.shape), cf, N)
    out = torch.empty(low, device=x.device, dtype=torch.float32)
    check(lib.gmk_box_mean(_p(x), _p(out), B, C, H, W, cf, N, _s()), "box_mean")
    return out


def _ns_check(ns, z):
    """`ns` of the *_ns entries: (r, cf, N) with r fp32 [B, C / cf, H / N, W / N] (`box_residual`'s output) -> (r, C, H, W, cf, N)"""
    r, cf, N = ns
    _, C, H, W, cf, N, low = box_geometry(tuple(z.shape), cf, N)
    _f32(r, "ns residual")
    if tuple(r.shape) != low:
        raise ValueError(f"ns residual: shape {tuple(r.shape)}, expected {low}")
    return r, C, H, W, cf, N


def box_residual(v, z, obs, logsnr_t, cf, N, v_uncond=None, cond_w=None, mean_type="v"):
    """DDNM's residual obs - A x-hat (gmk_box_residual; Wang, Yu & Zhang 2023; an extension): x-hat the clipped (guided, when v_uncond /
    cond_w are given) data prediction `sampler_step` forms for the network output v at (z, logsnr_t), bit for bit.  v, z, v_uncond: fp32
    [B, C, H, W]; obs: fp32 [B, C / cf, H / N, W / N].  -> r of obs's shape: the `ns=(r, cf, N)` of `sampler_step` / `dpm_solver_step`."""
    _sampler_check(v, z, ((v_uncond, "v_uncond"),), cond_w)
    B, C, H, W, cf, N, low = box_geometry(tuple(z.shape), cf, N)
    _f32(obs, "obs")
    if tuple(obs.shape) != low:
        raise ValueError(f"obs: shape {tuple(obs.shape)}, expected {low}")
    r = torch.empty_like(obs)
    check(lib.gmk_box_residual(_p(v), _p(v_uncond), _p(cond_w), _p(z), _p(obs), float(logsnr_t), _p(r), MEAN_TYPES[mean_type], B, C, H, W,
                               cf, N, _s()), "box_residual")
    return r


# ---- diffusion posterior sampling (Chung et al. 2023, Algorithm 1; an extension; gaussian_diffusion.GaussianDiffusion.posterior_sample) ----
DPS_OPS = {"box": C["GMK_DPS_BOX"], "blur": C["GMK_DPS_BLUR"]}
BLUR_MAX_R, BLUR_MAX_SIDE = C["GMK_BLUR_MAX_R"], C["GMK_BLUR_MAX_SIDE"]


@functools.lru_cache(maxsize=32)
def _device_taps(taps, device):
    """The fp32 taps of a blur (a tuple of 2 R + 1 floats) on `device`: made once per operator, not once per sampler step."""
    return torch.tensor(taps, dtype=torch.float32).to(device)


def _blur_check(shape, taps):
    """-> (B, C, H, W, R) of a blur with `taps` (2 R + 1 floats) on images of `shape`, or ValueError."""
    if len(shape) != 4 or 0 in shape:
        raise ValueError(f"blur operator: shape {tuple(shape)}, expected [B, C, H, W] with every dimension > 0")
    B, C, H, W = (int(d) for d in shape)
    R = (len(taps) - 1) // 2
    if len(taps) != 2 * R + 1 or not 1 <= R <= BLUR_MAX_R:
        raise ValueError(f"blur operator: {len(taps)} taps, expected 2 R + 1 with 1 <= R <= {BLUR_MAX_R}")
    if H > BLUR_MAX_SIDE or W > BLUR_MAX_SIDE:
        raise ValueError(f"blur operator: H = {H}, W = {W}, at most {BLUR_MAX_SIDE} (the plane is staged in LDS)")
    return B, C, H, W, R


def gauss_blur(x, taps):
    """A x of the blur operator (gmk_gauss_blur; an extension): x fp32 [B, C, H, W] with H, W <= 64 -> x's shape, every channel convolved with
    `taps` (a tuple of 2 R + 1 fp32 values, `gaussian_diffusion.blur_taps`) along its rows, then along its columns, with zero padding: each
    value a sequential fp32 sum of fmul(tap, value) in tap order."""
    _f32(x, "x")
    taps = tuple(float(t) for t in taps)
    B, C, H, W, R = _blur_check(tuple(x.shape), taps)
    out = torch.empty_like(x)
    with _Timed("gauss_blur_kernel", 0.0, _nbytes(x, out), fixed=True):
        check(lib.gmk_gauss_blur(_p(x), _p(out), _p(_device_taps(taps, x.device)), R, B, C, H, W, _s()), "gauss_blur")
    return out


def measure(x, op):
    """A x of a `gaussian_diffusion.MeasurementOp`: `box_mean` (kind 'box') or `gauss_blur` (kind 'blur')."""
    if op.kind == "box":
        return box_mean(x, op.cf, op.N)
    if op.kind == "blur":
        return gauss_blur(x, op.taps)
    raise ValueError(f"measurement operator of kind {op.kind!r}: expected 'box' or 'blur'")


def dps_backproject(v, z, obs, logsnr_t, op, mean_type="v"):
    """The data term of one DPS step (gmk_dps_backproject): x-hat the UNCLIPPED, unguided data prediction of the network output v at
    (z, logsnr_t), e = obs - A x-hat, -> (u, enorm2) = (A^T e, fp32 of z's shape; |e_b|^2, fp32 [B]).  v, z: fp32 [B, C, H, W]; obs: what
    `measure(x, op)` returns for an x of z's shape; op: a `gaussian_diffusion.MeasurementOp`."""
    if mean_type not in MEAN_TYPES:
        raise ValueError(f"mean_type {mean_type!r}: expected one of {sorted(MEAN_TYPES)}")
    if not math.isfinite(float(logsnr_t)):
        raise ValueError(f"dps_backproject: non-finite time {logsnr_t}")
    if op.kind not in DPS_OPS:
        raise ValueError(f"measurement operator of kind {op.kind!r}: expected 'box' or 'blur'")
    shape = tuple(z.shape)
    if tuple(v.shape) != shape:
        raise ValueError(f"v: shape {tuple(v.shape)}, expected z's {shape}")
    if op.kind == "box":
        B, C, H, W, cf, N, low = box_geometry(shape, op.cf, op.N)
        taps, R = None, 0
    else:
        B, C, H, W, R = _blur_check(shape, op.taps)
        cf, N, low = 1, 1, shape
    if tuple(obs.shape) != tuple(low):
        raise ValueError(f"obs: shape {tuple(obs.shape)}, expected {tuple(low)}")
    _f32(v, "v"); _f32(z, "z"); _f32(obs, "obs")
    if op.kind == "blur":
        taps = _device_taps(tuple(float(t) for t in op.taps), z.device)
    u = torch.empty_like(z)
    enorm2 = torch.empty((B,), device=z.device, dtype=torch.float32)
    with _Timed("dps_backproject_kernel", 0.0, _nbytes(v, z, obs, u), fixed=True):
        check(lib.gmk_dps_backproject(_p(v), _p(z), _p(obs), float(logsnr_t), DPS_OPS[op.kind], cf, N, _p(taps), R, _p(u), _p(enorm2),
                                      MEAN_TYPES[mean_type], B, C, H, W, _s()), "dps_backproject")
    return u, enorm2


def dps_correct(z, u, g, enorm2, c_z, c_o, zeta):
    """The guidance of one DPS step, in place on z (gmk_dps_correct): z += 2 zeta / max(sqrt(enorm2[b]), FLT_MIN) (c_z u + c_o g) - u, enorm2
    from `dps_backproject`, g the network's input VJP of u, (c_z, c_o) = d x-hat / d (z, out).  z, u, g: fp32 [B, ...] of one shape with a
    multiple of 4 values per image; zeta finite, >= 0; zeta = 0 launches nothing.  -> z"""
    shape = tuple(z.shape)
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f"z: bad shape {shape}, expected [B, ...] with B and every image dimension > 0")
    B, n = shape[0], math.prod(shape[1:])
    if n % 4:
        raise ValueError(f"z: {n} values per image, a multiple of 4 is required")
    for t, nm in ((u, "u"), (g, "g")):
        if tuple(t.shape) != shape:
            raise ValueError(f"{nm}: shape {tuple(t.shape)}, expected {shape}")
    if tuple(enorm2.shape) != (B,):
        raise ValueError(f"enorm2: shape {tuple(enorm2.shape)}, expected ({B},)")
    c_z, c_o, zeta = float(c_z), float(c_o), float(zeta)
    if not (math.isfinite(c_z) and math.isfinite(c_o)):
        raise ValueError(f"dps_correct: non-finite coefficient c_z = {c_z}, c_o = {c_o}")
    if not (math.isfinite(zeta) and 0.0 <= zeta < 1e38):
        raise ValueError(f"dps_correct: zeta = {zeta}, need a finite step size >= 0")
    _f32(z, "z"); _f32(u, "u"); _f32(g, "g"); _f32(enorm2, "enorm2")
    if zeta == 0.0:                         # (the entry launches nothing either: a profile records no launch)
        return z
    with _Timed("dps_correct_kernel", 0.0, _nbytes(z, u, g, z), fixed=True):
        check(lib.gmk_dps_correct(_p(z), _p(u), _p(g), _p(enorm2), c_z, c_o, zeta, B, n, _s()), "dps_correct")
    return z


def _step_forms(name, plain, dt, with_ns, head, rest, z, B, thr, ns):
    """One launch of an update that has a thresholded and a restoring form: the entry `plain`, with thr (fp32 [B], dynamic thresholding) `dt`,
    with ns ((r, cf, N), restoration) `with_ns`, never both.  The extra pointer follows `head`, the box geometry `rest`."""
    if ns is not None:
        if thr is not None:
            raise ValueError(f"{name}: ns (restoration) together with thr (dynamic thresholding) is not supported")
        r, *geom = _ns_check(ns, z)
        check(with_ns(*head, _p(r), *rest, *geom, _s()), name + "_ns")
    elif thr is not None:
        check(dt(*head, _p(_thr_check(thr, B)), *rest, _s()), name + "_dt")
    else:
        check(plain(*head, *rest, _s()), name)


def sampler_step(v, z, logsnr_t, logsnr_s, is_last, v_uncond=None, cond_w=None, noise=None, want_pred=False, mean_type="v",
                 dup=False, logsnr_next=None, thr=None, ns=None):
    """dup: z_next is returned as the first half of a [2B, ...] tensor whose second half holds the same values (z2 = returned[1]);
    logsnr_next: fp32 [B] (or [2B] with dup) filled with logsnr_s.  thr: None, or fp32 [B] - dynamic thresholding (gmk_sampler_step_dt):
    x-hat is the unclipped (guided) prediction clamped to +-thr[b] and divided by thr[b] (`dyn_threshold` gives thr).  ns: None, or
    (r, cf, N) - DDNM's null-space projection (gmk_sampler_step_ns): x-hat + A+ r with r = `box_residual`'s output; not together with thr."""
    B, n, z_next, z2, xp, ep = _sampler_io(v, z, ((v_uncond, "v_uncond"), (noise, "noise")), cond_w, want_pred, dup, logsnr_next)
    rest = (_p(z), _p(noise), float(logsnr_t), float(logsnr_s), int(is_last), _p(z_next), _p(xp), _p(ep), _p(z2[B:]) if dup else None,
            _p(logsnr_next), MEAN_TYPES[mean_type], B, n)
    _step_forms("sampler_step", lib.gmk_sampler_step, lib.gmk_sampler_step_dt, lib.gmk_sampler_step_ns, (_p(v), _p(v_uncond), _p(cond_w)), rest,
                z, B, thr, ns)
    return _sampler_ret(z_next, z2, xp, ep)


def dpm_solver_step(v, z, x_hist, logsnr_t, logsnr_s, coef_z, coef_x, coef_prev, is_last, v_uncond=None, cond_w=None, want_pred=False,
                    mean_type="v", dup=False, logsnr_next=None, thr=None, ns=None):
    """One DPM-Solver++(2M) step (gmk_dpm_solver_step).  x_hist: fp32 [B, ...], the previous x-hat, overwritten with this step's (not read
    when coef_prev == 0).  Arguments and returns otherwise as `sampler_step` (no noise: the solver is deterministic); thr as there
    (gmk_dpm_solver_step_dt), ns as there (gmk_dpm_solver_step_ns)."""
    B, n, z_next, z2, xp, ep = _sampler_io(v, z, ((x_hist, "x_hist"), (v_uncond, "v_uncond")), cond_w, want_pred, dup, logsnr_next)
    rest = (_p(z), _p(x_hist), float(logsnr_t), float(logsnr_s), float(coef_z), float(coef_x), float(coef_prev), int(is_last), _p(z_next), _p(xp),
            _p(ep), _p(z2[B:]) if dup else None, _p(logsnr_next), MEAN_TYPES[mean_type], B, n)
    _step_forms("dpm_solver_step", lib.gmk_dpm_solver_step, lib.gmk_dpm_solver_step_dt, lib.gmk_dpm_solver_step_ns,
                (_p(v), _p(v_uncond), _p(cond_w)), rest, z, B, thr, ns)
    return _sampler_ret(z_next, z2, xp, ep)


DYN_THRESHOLD_KEYS = C["GMK_DYN_THRESHOLD_KEYS"]      # images of up to this many values are selected from LDS, larger ones re-read


def dyn_threshold(v, z, logsnr_t, p, v_uncond=None, cond_w=None, mean_type="v", want_q=False):
    """The per-image threshold of dynamic thresholding (Saharia et al. 2022, section 2.3; gmk_dyn_threshold; an extension): s[b] = max(1, q[b]),
    q[b] the p-quantile (0 < p <= 1, torch.quantile's linear rule, exact order statistics) of |x_raw[b]|, x_raw the UNCLIPPED (guided, when
    v_uncond / cond_w are given) data prediction of the network output v at (z, logsnr_t).  v, z, v_uncond: fp32 [B, ...]; cond_w: fp32 [B].
    -> s (fp32 [B]: the `thr=` of `sampler_step` / `dpm_solver_step`), or (s, q) with want_q."""
    from .diffusion.gaussian_diffusion import dyn_threshold_rank
    B, n = _sampler_check(v, z, ((v_uncond, "v_uncond"),), cond_w)
    k_lo, frac = dyn_threshold_rank(p, n)
    s = torch.empty((B,), device=z.device, dtype=torch.float32)
    q = torch.empty_like(s) if want_q else None
    check(lib.gmk_dyn_threshold(_p(v), _p(v_uncond), _p(cond_w), _p(z), float(logsnr_t), k_lo, frac, _p(s), _p(q), MEAN_TYPES[mean_type],
                                B, n, _s()), "dyn_threshold")
    return (s, q) if want_q else s


CFG_RESCALE_KEEP = C["GMK_CFG_RESCALE_KEEP"]      # images of up to this many values are read once and kept in registers, larger ones re-read


def cfg_rescale(v, z, logsnr_t, phi, v_uncond, cond_w, mean_type="v", want_ratio=False):
    """The rescale factor of classifier-free guidance as a threshold (Lin et al. 2023, section 3.4; gmk_cfg_rescale; an extension):
    thr[b] = 1 / f[b], f = 1 + phi (ratio - 1), ratio[b] = std(x_c[b]) / std(x_raw[b]) - x_c the conditional data prediction of the network
    output v at (z, logsnr_t), x_raw the guided one, both UNCLIPPED as `dyn_threshold` forms them.  clamp(x, -thr, thr) / thr = clip(f x, -1, 1),
    so thr is the `thr=` of `sampler_step` / `dpm_solver_step`.  v, z, v_uncond: fp32 [B, ...]; cond_w: fp32 [B]; 0 <= phi <= 1.
    -> thr (fp32 [B]), or (thr, ratio) with want_ratio."""
    if v_uncond is None or cond_w is None:
        raise ValueError("cfg_rescale: v_uncond and cond_w are required (the factor compares the guided prediction with the conditional one)")
    phi = float(phi)
    if not 0.0 <= phi <= 1.0:
        raise ValueError(f"cfg_rescale: phi = {phi} outside [0, 1]")
    B, n = _sampler_check(v, z, ((v_uncond, "v_uncond"),), cond_w)
    thr = torch.empty((B,), device=z.device, dtype=torch.float32)
    ratio = torch.empty_like(thr) if want_ratio else None
    check(lib.gmk_cfg_rescale(_p(v), _p(v_uncond), _p(cond_w), _p(z), float(logsnr_t), phi, _p(thr), _p(ratio), MEAN_TYPES[mean_type], B, n,
                              _s()), "cfg_rescale")
    return (thr, ratio) if want_ratio else thr


def inpaint_merge(z, x0, mask, alpha_s, sigma_s, a, b, is_last, renoise, logsnr_t, logsnr_s, seed, offset, q0=0, B_total=None, z_dup=None,
                  logsnr_next=None):
    """RePaint's merge of the known region (gmk_inpaint_merge), in place on z (fp32 [B, ...], the sampler update's output):
    z = mask ? (is_last ? x0 : alpha_s x0 + sigma_s eps1) : z, then z = a z + b eps2 when `renoise`.  mask: uint8 with B x n elements in z's
    element order (nonzero = known); x0: z's shape.  eps1 / eps2 are the Philox normals of gmk_rng_normal(seed, offset + q0) and
    gmk_rng_normal(seed, offset + B_total n / 4 + q0): q0 places this chunk's rows inside a batch of B_total rows (default: the chunk is
    the batch).  z_dup: a second tensor of z's shape that receives the same values; logsnr_next: fp32 [B] ([2B] with z_dup), filled with
    logsnr_t when renoise, else logsnr_s.  -> z"""
    for t, nm in ((z, "z"), (x0, "x0"), (z_dup, "z_dup"), (logsnr_next, "logsnr_next")):
        if t is not None and t.dtype != torch.float32:
            raise ValueError(f"{nm}: dtype {t.dtype}, expected torch.float32")
    if mask.dtype != torch.uint8:
        raise ValueError(f"mask: dtype {mask.dtype}, expected torch.uint8")
    shape = tuple(z.shape)
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f"z: bad shape {shape}, expected [B, ...] with B and every image dimension > 0")
    B, n = shape[0], math.prod(shape[1:])
    if n % 4:
        raise ValueError(f"z: {n} values per image, a multiple of 4 is required")
    if tuple(x0.shape) != shape:
        raise ValueError(f"x0: shape {tuple(x0.shape)}, expected {shape}")
    if mask.dim() < 1 or mask.shape[0] != B or mask.numel() != B * n:
        raise ValueError(f"mask: shape {tuple(mask.shape)}, expected {B} rows of {n} values")
    if z_dup is not None and tuple(z_dup.shape) != shape:
        raise ValueError(f"z_dup: shape {tuple(z_dup.shape)}, expected {shape}")
    if logsnr_next is not None and (logsnr_next.dim() != 1 or logsnr_next.numel() != (2 * B if z_dup is not None else B)):
        raise ValueError(f"logsnr_next: shape {tuple(logsnr_next.shape)}, expected ({2 * B if z_dup is not None else B},)")
    B_total = B if B_total is None else int(B_total)
    q0 = int(q0)
    if B_total < B or q0 < 0 or q0 > (B_total - B) * (n // 4):
        raise ValueError(f"q0 = {q0}, B_total = {B_total}: a chunk of {B} rows must lie inside the batch")
    seed, offset = check_stream(seed, offset)
    if is_last and renoise:
        raise ValueError("inpaint_merge: the last step does not re-noise")
    coefs = (alpha_s, sigma_s, a, b, logsnr_t, logsnr_s)
    if not all(math.isfinite(float(c)) for c in coefs):
        raise ValueError(f"inpaint_merge: non-finite time or coefficient {coefs}")
    _f32(z, "z"); _f32(x0, "x0"); _chk(mask, torch.uint8, "mask")
    if z_dup is not None:
        _f32(z_dup, "z_dup")
    if logsnr_next is not None:
        _f32(logsnr_next, "logsnr_next")
    check(lib.gmk_inpaint_merge(_p(z), _p(x0), _p(mask), float(alpha_s), float(sigma_s), float(a), float(b), int(bool(is_last)),
                                int(bool(renoise)), float(logsnr_t), float(logsnr_s), seed, offset, q0, B_total, _p(z_dup), _p(logsnr_next),
                                B, n, _s()), "inpaint_merge")
    return z


# ---- continuous-time variational bound (an extension; gaussian_diffusion.GaussianDiffusion.nll) ----------------------------------------
# Shapes, dtypes and the mean type are checked before `_f32` asks for a device tensor, so that a bad call is named for what is wrong with it.
def _vlb_check(tensors, vectors=()):
    """tensors: (tensor, name) pairs of one image shape [B, ...]; vectors: (tensor, name) pairs of B floats each.  -> (B, floats per image)"""
    for t, nm in tuple(tensors) + tuple(vectors):
        if t.dtype != torch.float32:
            raise ValueError(f"{nm}: dtype {t.dtype}, expected torch.float32")
    shape = tuple(tensors[0][0].shape)
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f"{tensors[0][1]}: bad shape {shape}, expected [B, ...] with B and every image dimension > 0")
    for t, nm in tensors:
        if tuple(t.shape) != shape:
            raise ValueError(f"{nm}: shape {tuple(t.shape)}, expected {shape}")
    for t, nm in vectors:
        if t.dim() != 1 or t.numel() != shape[0]:
            raise ValueError(f"{nm}: shape {tuple(t.shape)}, expected ({shape[0]},)")
    for t, nm in tuple(tensors) + tuple(vectors):
        _f32(t, nm)
    return shape[0], math.prod(shape[1:])


def q_sample_logsnr(x, eps, logsnr):
    """z = alpha x + sigma eps at the per-sample log-SNR `logsnr` (fp32 [B]).  -> z"""
    B, n = _vlb_check(((x, "x"), (eps, "eps")), vectors=((logsnr, "logsnr"),))
    z = torch.empty_like(x)
    check(lib.gmk_q_sample_logsnr(_p(x), _p(eps), _p(logsnr), _p(z), B, n, _s()), "q_sample_logsnr")
    return z


def vlb_term(out, z, eps, logsnr, weight, acc, mean_type="v"):
    """acc += weight * sum over each image of (eps - eps_hat)^2, eps_hat the unclipped noise prediction of the net output `out` (gmk_vlb_term).
    logsnr, weight, acc: fp32 [B]; acc is updated in place and returned."""
    if mean_type not in MEAN_TYPES:
        raise ValueError(f"mean_type {mean_type!r}: expected one of {sorted(MEAN_TYPES)}")
    B, n = _vlb_check(((out, "out"), (z, "z"), (eps, "eps")), vectors=((logsnr, "logsnr"), (weight, "weight"), (acc, "acc")))
    check(lib.gmk_vlb_term(_p(out), _p(z), _p(eps), _p(logsnr), _p(weight), _p(acc), MEAN_TYPES[mean_type], B, n, _s()), "vlb_term")
    return acc


def vlb_endpoints(x, eps0, delta):
    """Prior (KL at logsnr -20) and decoder (discretised Gaussian at logsnr 20, bin half-width `delta`) terms per image, in nats.
    -> (prior, decoder), fp32 [B] each."""
    delta = float(delta)
    if not 0.0 < delta <= 0.5:
        raise ValueError(f"delta = {delta}: the bin half-width must lie in (0, 0.5]")
    B, n = _vlb_check(((x, "x"), (eps0, "eps0")))
    prior = torch.empty((B,), device=x.device, dtype=torch.float32)
    dec = torch.empty_like(prior)
    check(lib.gmk_vlb_endpoints(_p(x), _p(eps0), delta, _p(prior), _p(dec), B, n, _s()), "vlb_endpoints")
    return prior, dec


# ---- probability-flow ODE (an extension; gaussian_diffusion.GaussianDiffusion.encode / decode / ode_nll) ----------------------------------
def rng_rademacher(shape, seed, offset, device):
    """+1 where rng_uniform(shape, seed, offset) >= 1/2, else -1 (Hutchinson probes)."""
    seed, offset = check_stream(seed, offset)
    out = torch.empty(shape, device=device, dtype=torch.float32)
    with _Timed("rng_rademacher_kernel", 0.0, _nbytes(out), fixed=True):
        check(lib.gmk_rng_rademacher(_p(out), out.numel(), seed, offset, _s()), "rng_rademacher")
    return out


def dequantize(x, delta, seed, offset):
    """y = x + delta (2 u - 1), u = rng_uniform(x.shape, seed, offset) (drawn in the kernel).  -> y"""
    delta = float(delta)
    if not 0.0 < delta <= 0.5:
        raise ValueError(f"delta = {delta}: the bin half-width must lie in (0, 0.5]")
    seed, offset = check_stream(seed, offset)
    if x.dtype != torch.float32:
        raise ValueError(f"x: dtype {x.dtype}, expected torch.float32")
    if x.numel() == 0:
        raise ValueError("x: empty")
    _f32(x, "x")
    y = torch.empty_like(x)
    with _Timed("dequantize_kernel", 0.0, _nbytes(x, y), fixed=True):
        check(lib.gmk_dequantize(_p(x), _p(y), delta, x.numel(), seed, offset, _s()), "dequantize")
    return y


def pf_ode_step(out, z, logsnr_i, logsnr_j=None, mean_type="v", r=None, g=None, acc=None, div_a=0.0, div_b=0.0, prior=None, x_out=None):
    """One probability-flow ODE step after the network evaluation `out` at (z, logsnr_i) (gmk_pf_ode_step), fp32 [B, ...] tensors:
    logsnr_j given: z = alpha_j x_hat + sigma_j eps_hat in place (x_hat, eps_hat unclipped); x_out: receives x_hat;
    acc (fp32 [B]): acc += div_a + div_b sum r g per image (needs the probe r and its input VJP g); prior (fp32 [B], only without an
    update): -log N(z; 0, I) per image.  -> z"""
    if mean_type not in MEAN_TYPES:
        raise ValueError(f"mean_type {mean_type!r}: expected one of {sorted(MEAN_TYPES)}")
    if acc is not None and (r is None or g is None):
        raise ValueError("pf_ode_step: the divergence needs the probe r and the VJP g")
    if prior is not None and logsnr_j is not None:
        raise ValueError("pf_ode_step: the prior is taken at the last point, which has no update")
    coefs = (logsnr_i, 0.0 if logsnr_j is None else logsnr_j, div_a, div_b)
    if not all(math.isfinite(float(c)) for c in coefs):
        raise ValueError(f"pf_ode_step: non-finite time or coefficient {coefs}")
    tensors = [(out, "out"), (z, "z")] + [(t, nm) for t, nm in ((r, "r"), (g, "g"), (x_out, "x_out")) if t is not None]
    vectors = [(t, nm) for t, nm in ((acc, "acc"), (prior, "prior")) if t is not None]
    B, n = _vlb_check(tensors, vectors=vectors)
    prior_c = 0.5 * n * math.log(2.0 * math.pi)
    with _Timed("pf_ode_step_kernel", 0.0, _nbytes(out, z, r, g, x_out) + (_nbytes(z) if logsnr_j is not None else 0.0), fixed=True):
        check(lib.gmk_pf_ode_step(_p(out), _p(z), _p(r), _p(g), _p(acc), _p(prior), _p(x_out), float(logsnr_i),
                                  float(0.0 if logsnr_j is None else logsnr_j), int(logsnr_j is not None), float(div_a), float(div_b),
                                  float(prior_c), MEAN_TYPES[mean_type], B, n, _s()), "pf_ode_step")
    return z


SLERP_KEEP = C["GMK_SLERP_KEEP"]      # images of up to this many values are read once, larger ones again for every t


def slerp(a, b, t, want_cos=False):
    """Spherical interpolation between the latent codes a and b (gmk_slerp; an extension): per image, out[k] = (sin((1 - t_k) theta) a +
    sin(t_k theta) b) / sin(theta) with cos(theta) = a.b / (|a| |b|), the lerp (1 - t_k) a + t_k b where sin(theta) < 1e-6 or the cosine is
    not finite.  a, b: fp32 [B, ...] of one shape with a multiple of 4 values per image; t: fp32 [K] on the device.
    -> out, fp32 [K, B, ...]; or (out, cos) with want_cos, cos fp32 [B]."""
    for x, nm in ((a, "a"), (b, "b"), (t, "t")):
        if x.dtype != torch.float32:
            raise ValueError(f"{nm}: dtype {x.dtype}, expected torch.float32")
    shape = tuple(a.shape)
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f"a: bad shape {shape}, expected [B, ...] with B and every image dimension > 0")
    if tuple(b.shape) != shape:
        raise ValueError(f"b: shape {tuple(b.shape)}, expected {shape}")
    B, n = shape[0], math.prod(shape[1:])
    if n % 4:
        raise ValueError(f"a: {n} values per image, a multiple of 4 is required")
    if t.dim() != 1 or t.numel() < 1:
        raise ValueError(f"t: shape {tuple(t.shape)}, expected (K,) with K >= 1")
    _f32(a, "a"); _f32(b, "b"); _f32(t, "t")
    K = t.numel()
    out = torch.empty((K,) + tuple(a.shape), device=a.device, dtype=torch.float32)
    cos = torch.empty((B,), device=a.device, dtype=torch.float32) if want_cos else None
    with _Timed("slerp_kernel", 0.0, _nbytes(a, b, out), fixed=True):
        check(lib.gmk_slerp(_p(a), _p(b), _p(t), _p(out), _p(cos), B, n, K, _s()), "slerp")
    return (out, cos) if want_cos else out


def logsnr_schedule(B, device, u=None, i_times=None, num_steps=1, shift=0.0, want_u=False, schedule=None):
    """logsnr = schedule(u - shift), u given or (i_times + 1) / num_steps.  schedule: as in `q_sample` (`shift` here moves u, the schedule's
    own shift the log-SNR).  -> logsnr (, u_shifted)"""
    if u is not None:
        _f32(u, "u")
        assert u.numel() == B
    if i_times is not None:
        _chk(i_times, torch.int64, "i_times")
        assert i_times.numel() == B
    logsnr = torch.empty((B,), device=device, dtype=torch.float32)
    uo = torch.empty((B,), device=device, dtype=torch.float32) if want_u else None
    if schedule is None:
        check(lib.gmk_logsnr_schedule(_p(u), _p(i_times), int(num_steps), float(shift), _p(uo), _p(logsnr), B, _s()),
              "logsnr_schedule")
    else:
        check(lib.gmk_logsnr_schedule_sched(_p(u), _p(i_times), int(num_steps), float(shift), *_sched_args(schedule), _p(uo), _p(logsnr), B,
                                            _s()), "logsnr_schedule_sched")
    return (logsnr, uo) if want_u else logsnr


def ddim_step_vec(v, z, logsnr_t, logsnr_s, v_uncond=None, cond_w=None, mean_type="v"):
    """Teacher DDIM step with per-sample times.  -> (z_s, x_pred, eps_pred)"""
    for t, nm in ((v, "v"), (z, "z"), (logsnr_t, "logsnr_t"), (logsnr_s, "logsnr_s")):
        _f32(t, nm)
    B = z.shape[0]
    n = z.numel() // B
    zs, xp, ep = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    check(lib.gmk_ddim_step_vec(_p(v), _p(v_uncond), _p(cond_w), _p(z), _p(logsnr_t), _p(logsnr_s), _p(zs), _p(xp), _p(ep),
                                MEAN_TYPES[mean_type], B, n, _s()), "ddim_step_vec")
    return zs, xp, ep


def distill_target(z_teacher, z_t, x_pred_teacher, logsnr, logsnr_s, i_times):
    for t, nm in ((z_teacher, "z_teacher"), (z_t, "z_t"), (x_pred_teacher, "x_pred"), (logsnr, "logsnr"), (logsnr_s, "logsnr_s")):
        _f32(t, nm)
    _chk(i_times, torch.int64, "i_times")
    B = z_t.shape[0]
    n = z_t.numel() // B
    xt, et = torch.empty_like(z_t), torch.empty_like(z_t)
    check(lib.gmk_distill_target(_p(z_teacher), _p(z_t), _p(x_pred_teacher), _p(logsnr), _p(logsnr_s), _p(i_times), _p(xt), _p(et),
                                 B, n, _s()), "distill_target")
    return xt, et


# ---- consistency distillation and multistep consistency sampling (extensions; Song et al. 2023, "Consistency Models") ------------------
def _images(tensors, vectors=(), what="consistency"):
    """tensors: (tensor, name) pairs of one fp32 image shape [B, ...]; vectors: (tensor, name, dtype) triples of B values each; all contiguous
    device tensors (named for what is wrong before anything is launched).  -> (B, values per image)"""
    shape = tuple(tensors[0][0].shape)
    if len(shape) < 2 or 0 in shape:
        raise ValueError(f"{what}: {tensors[0][1]} has shape {shape}, expected [B, ...] with B and every image dimension > 0")
    for t, nm in tensors:
        if tuple(t.shape) != shape:
            raise ValueError(f"{nm}: shape {tuple(t.shape)}, expected {shape}")
    for t, nm, dtype in vectors:
        if t.dim() != 1 or t.numel() != shape[0]:
            raise ValueError(f"{nm}: shape {tuple(t.shape)}, expected ({shape[0]},)")
    for t, nm, dtype in tuple((t, nm, torch.float32) for t, nm in tensors) + tuple(vectors):
        if not (t.is_cuda and t.is_contiguous() and t.dtype == dtype):
            raise ValueError(f"{nm}: expected a contiguous {dtype} device tensor")
    return shape[0], math.prod(shape[1:])


def consistency_target(v_tgt, z_s, x_pred_teacher, z_t, logsnr_t, logsnr_s, i_times, mean_type="v"):
    """The target of consistency distillation (gmk_consistency_target; Song et al. 2023, Algorithm 2): x_target = the clipped data prediction
    of the target network's output v_tgt at (z_s, logsnr_s) - `ddim_step_vec`'s x_pred, bit for bit - with the i_times == 0 rows taking
    x_pred_teacher (the boundary condition), and eps_target = eps_from_x(z_t, x_target, logsnr_t), `distill_target`'s closing expression.
    Images: fp32 [B, ...], contiguous (16-byte aligned tensors with n % 4 == 0 take the 16-byte path, anything else the scalar one);
    logsnr_t, logsnr_s: fp32 [B]; i_times: int64 [B].  -> (x_target, eps_target)"""
    if mean_type not in MEAN_TYPES:
        raise ValueError(f"mean_type {mean_type!r}: expected one of {sorted(MEAN_TYPES)}")
    B, n = _images(((z_t, "z_t"), (v_tgt, "v_tgt"), (z_s, "z_s"), (x_pred_teacher, "x_pred_teacher")),
                   ((logsnr_t, "logsnr_t", torch.float32), (logsnr_s, "logsnr_s", torch.float32), (i_times, "i_times", torch.int64)),
                   "consistency_target")
    if B >= 65536:
        raise ValueError(f"consistency_target: B = {B}, need < 65536")
    xt, et = torch.empty_like(z_t), torch.empty_like(z_t)
    check(lib.gmk_consistency_target(_p(v_tgt), _p(z_s), _p(x_pred_teacher), _p(z_t), _p(logsnr_t), _p(logsnr_s), _p(i_times), _p(xt), _p(et),
                                     MEAN_TYPES[mean_type], B, n, _s()), "consistency_target")
    return xt, et


def x_loss_huber(v, z, x, logsnr, c, grad_scale=None, mean_type="v"):
    """Pseudo-Huber x-space loss (gmk_x_loss_huber; Song & Dhariwal 2023; an extension): loss_b = sqrt(x_mse + c^2) - c, x_mse = mean (x_hat - x)^2
    of the clipped prediction - the bits of `x_loss_w`'s x_mse.  c = c_paper / sqrt(n), finite and > 0.  Tensors as in `x_loss_w`.
    -> (loss_b, x_mse, dv or None), dv = d(grad_scale sum_b loss_b)/dv when grad_scale is given."""
    c = float(c)
    if not (math.isfinite(c) and c > 0.0):
        raise ValueError(f"c = {c}: need a finite value > 0")
    B, n = _loss_front("x_loss_huber", ((x, "x"), (v, "v"), (z, "z")), ((logsnr, "logsnr"),), mean_type)
    return _loss_call("x_loss_huber", (v, z, x, logsnr), 2, (v,), grad_scale, (c,), mean_type, B, n)


def consistency_step(v, z, logsnr_t, logsnr_s, is_last, seed, offset, q0=0, v_uncond=None, cond_w=None, want_pred=False, mean_type="v",
                     dup=False, logsnr_next=None):
    """One step of multistep consistency sampling (gmk_consistency_step; Song et al. 2023, Algorithm 1): x-hat as `sampler_step` forms it
    (guidance included), z_next = x-hat when is_last, else alpha_s x-hat + sigma_s eps with eps the Philox normals of
    gmk_rng_normal(seed, offset + q0), drawn in the kernel: q0 = a n / 4 places a chunk that starts at row a of a batch.  n % 4 == 0.
    Arguments and returns otherwise as `sampler_step`."""
    scalars = _drawn_scalars("consistency_step", z, mean_type, (logsnr_t, logsnr_s))
    seed, offset, q0 = _drawn_stream("consistency_step", seed, offset, q0, v_uncond, cond_w)
    B, n, z_next, z2, xp, ep = _sampler_io(v, z, ((v_uncond, "v_uncond"),), cond_w, want_pred, dup, logsnr_next)
    check(lib.gmk_consistency_step(_p(v), _p(v_uncond), _p(cond_w), _p(z), *scalars, int(bool(is_last)), seed, offset, q0,
                                   _p(z_next), _p(xp), _p(ep), _p(z2[B:]) if dup else None, _p(logsnr_next), MEAN_TYPES[mean_type], B, n, _s()),
          "consistency_step")
    return _sampler_ret(z_next, z2, xp, ep)


def stochastic_step(v, z, logsnr_t, logsnr_s, coef_z, coef_x, coef_noise, coef_prev, is_last, seed, offset, q0=0, x_hist=None, thr=None,
                    v_uncond=None, cond_w=None, want_pred=False, mean_type="v", dup=False, logsnr_next=None):
    """One step of a stochastic sampler (gmk_stochastic_step): x-hat as `sampler_step` forms it (guidance included; with thr, fp32 [B], as its
    thresholded form), D = (1 + coef_prev) x-hat - coef_prev x_hist when coef_prev != 0, else x-hat, and z_next = x-hat when is_last, else
    coef_z z + coef_x D + coef_noise xi with xi the Philox normals of gmk_rng_normal(seed, offset + q0), drawn in the kernel (none when
    coef_noise == 0): q0 = a n / 4 places a chunk that starts at row a of a batch.  The coefficients are a row of
    `gaussian_diffusion.stochastic_coefs` ('ancestral', 'ddim_eta', 'sde_dpmpp_2m').  x_hist: None, or fp32 [B, ...] - the previous x-hat,
    overwritten with this step's; required when coef_prev != 0.  n % 4 == 0.  Arguments and returns otherwise as `sampler_step`."""
    scalars = _drawn_scalars("stochastic_step", z, mean_type, (logsnr_t, logsnr_s, coef_z, coef_x, coef_noise, coef_prev))
    if scalars[4] < 0.0:
        raise ValueError(f"coef_noise = {scalars[4]}: a standard deviation, need >= 0")
    if scalars[5] != 0.0 and x_hist is None:
        raise ValueError(f"coef_prev = {scalars[5]} without x_hist: the second-order step needs the previous x-hat")
    seed, offset, q0 = _drawn_stream("stochastic_step", seed, offset, q0, v_uncond, cond_w)
    B, n, z_next, z2, xp, ep = _sampler_io(v, z, ((x_hist, "x_hist"), (v_uncond, "v_uncond")), cond_w, want_pred, dup, logsnr_next)
    check(lib.gmk_stochastic_step(_p(v), _p(v_uncond), _p(cond_w), _p(z), _p(x_hist), None if thr is None else _p(_thr_check(thr, B)), *scalars,
                                  int(bool(is_last)), seed, offset, q0, _p(z_next), _p(xp), _p(ep), _p(z2[B:]) if dup else None,
                                  _p(logsnr_next), MEAN_TYPES[mean_type], B, n, _s()), "stochastic_step")
    return _sampler_ret(z_next, z2, xp, ep)


def stochastic_step_lv(v, z, nu, logsnr_t, logsnr_s, coef_z, coef_x, coef_noise_small, half_delta, is_last, seed, offset, q0=0, thr=None,
                       v_uncond=None, cond_w=None, want_pred=False, mean_type="v", dup=False, logsnr_next=None):
    """One 'ancestral' step under a learned variance (gmk_stochastic_step_lv; Nichol & Dhariwal 2021): `stochastic_step` with coef_prev = 0 and the
    noise multiplier coef_noise_small exp(f half_delta) per element, f = (nu + 1) / 2 - nu: fp32 of z's shape, the network's second output (the
    conditional half's under guidance); coef_noise_small: the 'small' row of `gaussian_diffusion.stochastic_row`; half_delta =
    (softplus(logsnr_s) - softplus(logsnr_t)) / 2 >= 0.  nu = -1 everywhere gives the bits of `stochastic_step` under 'small'.  Arguments and
    returns otherwise as `stochastic_step`."""
    scalars = _drawn_scalars("stochastic_step_lv", z, mean_type, (logsnr_t, logsnr_s, coef_z, coef_x, coef_noise_small, half_delta))
    if scalars[4] < 0.0:
        raise ValueError(f"coef_noise_small = {scalars[4]}: a standard deviation, need >= 0")
    if scalars[5] < 0.0:
        raise ValueError(f"half_delta = {scalars[5]}: half of logvar_large - logvar_small, need >= 0")
    seed, offset, q0 = _drawn_stream("stochastic_step_lv", seed, offset, q0, v_uncond, cond_w)
    if nu is None:
        raise ValueError("stochastic_step_lv: nu is required (the network's variance output)")
    B, n, z_next, z2, xp, ep = _sampler_io(v, z, ((nu, "nu"), (v_uncond, "v_uncond")), cond_w, want_pred, dup, logsnr_next)
    check(lib.gmk_stochastic_step_lv(_p(v), _p(v_uncond), _p(cond_w), _p(z), _p(nu), None if thr is None else _p(_thr_check(thr, B)), *scalars,
                                     int(bool(is_last)), seed, offset, q0, _p(z_next), _p(xp), _p(ep), _p(z2[B:]) if dup else None,
                                     _p(logsnr_next), MEAN_TYPES[mean_type], B, n, _s()), "stochastic_step_lv")
    return _sampler_ret(z_next, z2, xp, ep)


def _adam_arenas(p, g, m, v, ema=None):
    """The tensor checks of the three Adam ops: fp32 device arenas of one size (ema when given)."""
    arenas = ((p, "p"), (g, "g"), (m, "m"), (v, "v")) + (() if ema is None else ((ema, "ema"),))
    for t, nm in arenas:
        _f32(t, nm)
    assert all(t.numel() == p.numel() for t, _ in arenas)


def adam_step(p, g, m, v, lr, beta1, beta2, eps, step, grad_scale=1.0):
    _adam_arenas(p, g, m, v)
    check(lib.gmk_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), lr, beta1, beta2, eps, step, grad_scale, _s()), "adam_step")


def adam_ema_step(p, g, m, v, ema, lr, beta1, beta2, eps, step, decay_t, grad_scale=1.0):
    """adam_step, then ema.lerp_(p_new, 1 - decay_t) in the same pass over the arenas (gmk_adam_ema_step).  p, m, v come out the same bits as
    adam_step's."""
    _adam_arenas(p, g, m, v, ema)
    check(lib.gmk_adam_ema_step(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), lr, beta1, beta2, eps, step, grad_scale,
                                1.0 - float(decay_t), _s()), "adam_ema_step")


GRAD_NORM, CLIP_COEF, APPLY, SKIPPED = C["GMK_GRAD_NORM"], C["GMK_CLIP_COEF"], C["GMK_APPLY"], C["GMK_SKIPPED"]       # slots of the 4-float state gmk_grad_norm writes


def grad_norm_workspace(n, device):
    """The workspace gmk_grad_norm needs for an arena of n floats (one partial sum of squares per workgroup)."""
    return torch.empty((max(1, lib.gmk_grad_norm_workspace_bytes(int(n)) // 4),), dtype=torch.float32, device=device)


def grad_norm(g, state, grad_scale=1.0, max_norm=0.0, workspace=None):
    """state[GRAD_NORM] = grad_scale * ||g||_2, state[CLIP_COEF] = clip_grad_norm_'s coefficient for max_norm (1 when max_norm <= 0),
    state[APPLY] = 1 if the norm is finite else 0, state[SKIPPED] += 1 - apply; no host sync (gmk_grad_norm).  `state`: 4 fp32 on the device,
    zeroed by the caller before the first call; `workspace`: grad_norm_workspace(g.numel()), allocated here if not given.  -> state"""
    _f32(g, "g")
    _f32(state, "state")
    assert state.numel() == 4
    if workspace is None:
        workspace = grad_norm_workspace(g.numel(), g.device)
    _f32(workspace, "workspace")
    check(lib.gmk_grad_norm(_p(g), g.numel(), grad_scale, max_norm, _p(workspace), workspace.numel() * 4, _p(state), _s()), "grad_norm")
    return state


def adam_step_ctl(p, g, m, v, state, lr, beta1, beta2, eps, step, grad_scale=1.0, ema=None, decay_t=0.0):
    """adam_step (ema None) or adam_ema_step on the gradient (g * grad_scale) * state[CLIP_COEF]; does nothing at all when state[APPLY] is 0
    (gmk_adam_step_ctl).  With a coefficient of 1 the bits of those two ops."""
    _adam_arenas(p, g, m, v, ema)
    _f32(state, "state")
    assert state.numel() == 4
    check(lib.gmk_adam_step_ctl(_p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), lr, beta1, beta2, eps, step, grad_scale,
                                1.0 - float(decay_t), _p(state), _s()), "adam_step_ctl")


def _row_arena(t, n, name):
    """-> (tensor, row stride) of an fp32 [K][>= n] device arena whose rows are contiguous (a [:, :n] view of padded storage is one).  Rows
    narrower than n are reported as that width, which the library refuses by name."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{name}: expected an fp32 device tensor [K][stride] with contiguous rows, got {t.dtype} {tuple(t.shape)} strides "
                         f"{tuple(t.stride())}")
    if t.shape[1] < n or t.shape[0] < 2:
        return t, t.shape[1]
    if t.stride(0) < t.shape[1]:
        raise ValueError(f"{name}: rows overlap (strides {tuple(t.stride())})")
    return t, t.stride(0)


def adam_pema_step(p, g, m, v, pema, weights, lr, beta1, beta2, eps, step, grad_scale=1.0, ema=None, decay_t=0.0, state=None):
    """adam_step (state None) or adam_step_ctl (state: grad_norm's record), then the classic average when `ema` is given (adam_ema_step's bits),
    then row k of `pema` (fp32 [K][stride >= n], K = 1 .. 3) = lerp(row k, p_new, weights[k]) - one launch, every arena read and written once
    (gmk_adam_pema_step).  weights: K floats in [0, 1]."""
    _adam_arenas(p, g, m, v, ema)
    n = p.numel()
    pema, stride = _row_arena(pema, n, "pema")
    weights = [float(w) for w in weights]
    if len(weights) != pema.shape[0]:
        raise ValueError(f"pema has {pema.shape[0]} rows, {len(weights)} weights given")
    if state is not None:
        _f32(state, "state")
        assert state.numel() == 4
    pw = (weights + [0.0, 0.0, 0.0])[:3]
    check(lib.gmk_adam_pema_step(_p(p), _p(g), _p(m), _p(v), _p(ema), _p(pema), stride, pema.shape[0], n, lr, beta1, beta2, eps, step,
                                 grad_scale, 1.0 - float(decay_t), *pw, _p(state), _s()), "adam_pema_step")


def arena_combine(src, coef, out=None, n=None):
    """out[i] = fp32(sum_k coef[k] src[k][i]) accumulated in double in index order, each product and sum rounded on its own (gmk_arena_combine):
    src fp32 [K][stride >= n] on the device with contiguous rows, K = 1 .. 64; coef: K float64 values (any sequence, or a device tensor); n:
    columns combined (default: all of them).  -> out, fp32 [n] (must not overlap src)"""
    n = src.shape[1] if n is None else int(n)
    src, stride = _row_arena(src, n, "src")
    if not (isinstance(coef, torch.Tensor) and coef.is_cuda):
        coef = torch.as_tensor(coef, dtype=torch.float64).to(src.device)
    if coef.dtype != torch.float64 or not coef.is_contiguous() or coef.dim() != 1 or coef.numel() != src.shape[0]:
        raise ValueError(f"coef: expected {src.shape[0]} contiguous float64 values, got {coef.dtype} {tuple(coef.shape)}")
    if out is None:
        out = torch.empty((n,), dtype=torch.float32, device=src.device)
    if not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() != n:
        raise ValueError(f"out: expected {n} contiguous fp32 values on the device, got {out.dtype} {tuple(out.shape)}")
    check(lib.gmk_arena_combine(_p(src), stride, _p(coef), src.shape[0], _p(out), n, _s()), "arena_combine")
    return out


def arena_digest(t):
    """64-bit digest of a tensor's bytes read as 4-byte words (gmk_arena_digest; checkpoint.digest_host is the same function in numpy):
    any contiguous CUDA tensor whose byte size is a positive multiple of 4.  -> an unsigned Python int (reads the device: a host sync)"""
    nbytes = t.numel() * t.element_size()
    assert t.is_cuda and t.is_contiguous() and nbytes > 0 and nbytes % 4 == 0, (t.device, tuple(t.shape), tuple(t.stride()), t.dtype)
    out = torch.empty((1,), dtype=torch.int64, device=t.device)
    check(lib.gmk_arena_digest(_p(t), nbytes // 4, _p(out), _s()), "arena_digest")
    return int(out.item()) & 0xFFFFFFFFFFFFFFFF


# ---- exact nearest neighbours of byte rows (an extension; no reference call site) --------------------------------
NN_SLAB, NN_MAX_K, NN_MAX_D = C["GMK_NN_SLAB"], C["GMK_NN_MAX_K"], C["GMK_NN_MAX_D"]
NN_WORKSPACE_CAP = 64 << 20          # bytes of partial lists one launch may leave: nn_search_u8 takes the queries in blocks that stay below it


def _byte_rows(t, name):
    """uint8 device tensor of rank >= 2 -> its contiguous [rows, D] view (everything behind dimension 0 flattened; a copy only of a
    non-contiguous view), with the ranges of include/gmk.h checked."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
        raise ValueError(f"{name}: dtype {getattr(t, 'dtype', type(t))}, expected {torch.uint8}")
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if t.dim() < 2 or t.shape[0] < 1:
        raise ValueError(f"{name}: shape {tuple(t.shape)} (want [rows, ...] of rank >= 2 with at least one row)")
    rows = t.reshape(t.shape[0], -1).contiguous()
    if not 1 <= rows.shape[1] <= NN_MAX_D:
        raise ValueError(f"{name}: rows of D = {rows.shape[1]} bytes (1 .. {NN_MAX_D}: beyond it a squared distance leaves int32)")
    if rows.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: {rows.shape[0]} rows (below 2^31)")
    return rows


def u8_sqnorm(rows):
    """-> int32 [N]: sum_i (rows[j][i] - 128)^2 of a uint8 device tensor [N, ...] (gmk_u8_sqnorm): the norms nn_search_u8 wants of its database."""
    rows = _byte_rows(rows, "u8_sqnorm: rows")
    out = torch.empty((rows.shape[0],), device=rows.device, dtype=torch.int32)
    with _Timed("u8_sqnorm_kernel", 0.0, _nbytes(rows, out), fixed=True):
        check(lib.gmk_u8_sqnorm(_p(rows), rows.shape[0], rows.shape[1], _p(out), _s()), "u8_sqnorm")
    return out


def nn_search_u8(queries, database, k=1, db_sqnorm=None):
    """-> (dist2 int32 [Q, k], index int64 [Q, k]): per query the k smallest pairs (d2, j) in lexicographic order, d2 the exact squared
    Euclidean distance between the bytes of queries[q] and database[j] (include/gmk.h: gmk_nn_search_u8).  queries [Q, ...] and database
    [N, ...]: uint8 device tensors of rank >= 2 with the same number of bytes per row; db_sqnorm: u8_sqnorm(database), computed here when
    None.  The queries are taken in blocks whose workspace stays under NN_WORKSPACE_CAP."""
    queries, database = _byte_rows(queries, "nn_search_u8: queries"), _byte_rows(database, "nn_search_u8: database")
    if queries.device != database.device:
        raise ValueError(f"nn_search_u8: queries on {queries.device}, database on {database.device}")
    (Q, D), N = queries.shape, database.shape[0]
    if database.shape[1] != D:
        raise ValueError(f"nn_search_u8: queries of D = {D} bytes, database rows of D = {database.shape[1]}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= NN_MAX_K or k > N:
        raise ValueError(f"nn_search_u8: k = {k!r} with N = {N} (an integer in 1 .. {NN_MAX_K}, at most N)")
    if db_sqnorm is None:
        db_sqnorm = u8_sqnorm(database)
    elif (not isinstance(db_sqnorm, torch.Tensor) or db_sqnorm.dtype != torch.int32 or db_sqnorm.device != database.device
          or tuple(db_sqnorm.shape) != (N,) or not db_sqnorm.is_contiguous()):
        raise ValueError(f"nn_search_u8: db_sqnorm {getattr(db_sqnorm, 'dtype', type(db_sqnorm))} {tuple(getattr(db_sqnorm, 'shape', ()))}, "
                         f"expected contiguous {torch.int32} [{N}] on {database.device} (u8_sqnorm(database))")
    per_query = lib.gmk_nn_search_workspace(2, N, k) - lib.gmk_nn_search_workspace(1, N, k)      # the partial lists of one query
    block = max(1, NN_WORKSPACE_CAP // per_query)
    block = Q if block >= Q else max(block // 16 * 16, 1)          # whole 16-row groups: a later block starts 16-byte aligned when the first does
    need = lib.gmk_nn_search_workspace(block, N, k)
    workspace = torch.empty((need,), device=queries.device, dtype=torch.uint8)
    dist2 = torch.empty((Q, k), device=queries.device, dtype=torch.int32)
    index = torch.empty((Q, k), device=queries.device, dtype=torch.int32)
    for lo in range(0, Q, block):
        n = min(block, Q - lo)
        with _Timed("nn_search_kernel", 2.0 * n * N * D, _nbytes(database, queries[lo:lo + n], db_sqnorm) + 8.0 * n * k, fixed=True,
                    multiplied=2.0 * n * N * D):
            check(lib.gmk_nn_search_u8(_p(queries[lo:lo + n]), n, _p(database), N, D, _p(db_sqnorm), k, _p(workspace), need,
                                       _p(dist2[lo:lo + n]), _p(index[lo:lo + n]), _s()), "nn_search_u8")
    return dist2, index.long()


# ---- k-NN radii and ball counts of fp32 rows (an extension; no reference call site: metrics.manifold_metrics) -----
KNN_TILE, KNN_SLAB, KNN_MAX_D = C["GMK_KNN_TILE"], C["GMK_KNN_SLAB"], C["GMK_KNN_MAX_D"]


def _f32_rows(t, name):
    """fp32 device tensor [rows, D] -> itself when contiguous (4-byte alignment is enough: a view that starts off a 16-byte boundary takes the
    kernels' scalar staging path), else a contiguous copy; the ranges of include/gmk.h checked."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise ValueError(f"{name}: dtype {getattr(t, 'dtype', type(t))}, expected {torch.float32}")
    if not t.is_cuda:
        raise ValueError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if t.dim() != 2 or t.shape[0] < 1 or t.shape[0] >= 1 << 31:
        raise ValueError(f"{name}: shape {tuple(t.shape)} (want [rows, D] with 1 .. 2^31 - 1 rows)")
    if not 1 <= t.shape[1] <= KNN_MAX_D:
        raise ValueError(f"{name}: rows of D = {t.shape[1]} floats (1 .. {KNN_MAX_D})")
    return t.contiguous()


def knn_radius2(pts, k=3):
    """-> fp32 [N]: per row the (k + 1)-th smallest value of {d2(pts[i], pts[j]) : all j, j = i included}, the SQUARED distance to the k-th
    nearest other point (include/gmk.h: gmk_knn_radius_f32; d2 is the ascending fmaf chain of the direct differences)."""
    pts = _f32_rows(pts, "knn_radius2: pts")
    N, D = pts.shape
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= NN_MAX_K or k + 1 > N:
        raise ValueError(f"knn_radius2: k = {k!r} with N = {N} (an integer in 1 .. {NN_MAX_K}, k + 1 at most N)")
    need = lib.gmk_knn_radius_workspace(N, k)
    workspace = torch.empty((need // 4,), device=pts.device, dtype=torch.float32)
    r2 = torch.empty((N,), device=pts.device, dtype=torch.float32)
    with _Timed("knn_tile_kernel[radius]", 3.0 * N * N * D, _nbytes(pts, r2), fixed=True):
        check(lib.gmk_knn_radius_f32(_p(pts), N, D, k, _p(workspace), need, _p(r2), _s()), "knn_radius2")
    return r2


def ball_counts(balls, r2, queries, want_q=True, want_m=True):
    """-> (q_count int32 [Q] or None, m_count int32 [M] or None): q_count[q] = #{j : d2(queries[q], balls[j]) < r2[j]}, m_count[j] = #{q : the
    same predicate}, strict (include/gmk.h: gmk_ball_counts_f32).  balls [M, D], r2 [M], queries [Q, D]: fp32 device tensors."""
    balls, queries = _f32_rows(balls, "ball_counts: balls"), _f32_rows(queries, "ball_counts: queries")
    (M, D), Q = balls.shape, queries.shape[0]
    if queries.device != balls.device or queries.shape[1] != D:
        raise ValueError(f"ball_counts: balls {tuple(balls.shape)} on {balls.device}, queries {tuple(queries.shape)} on {queries.device}")
    if (not isinstance(r2, torch.Tensor) or r2.dtype != torch.float32 or r2.device != balls.device or tuple(r2.shape) != (M,)
            or not r2.is_contiguous()):
        raise ValueError(f"ball_counts: r2 {getattr(r2, 'dtype', type(r2))} {tuple(getattr(r2, 'shape', ()))}, expected contiguous "
                         f"{torch.float32} [{M}] on {balls.device}")
    q_count = torch.empty((Q,), device=balls.device, dtype=torch.int32) if want_q else None
    m_count = torch.empty((M,), device=balls.device, dtype=torch.int32) if want_m else None
    with _Timed("knn_tile_kernel[counts]", 3.0 * M * Q * D, _nbytes(balls, queries, r2, q_count, m_count), fixed=True):
        check(lib.gmk_ball_counts_f32(_p(balls), _p(r2), M, _p(queries), Q, D, _p(q_count), _p(m_count), _s()), "ball_counts")
    return q_count, m_count


# ---- self-attention core (north_star extension; no reference call site) -----------------------------------------
def bgemm_nt(A, B, out=None, alpha=1.0, out_dtype=None):
    """C[b] = alpha * A[b] @ B[b]^T for batches of K-contiguous matrices (row / batch strides free): A [batch, M, K],
    B [batch, N, K] -> C [batch, M, N].  bf16 operands run on the matrix cores (fp32 accumulation), fp32 operands on FMAs."""
    assert A.dim() == 3 and B.dim() == 3 and A.shape[0] == B.shape[0] and A.shape[2] == B.shape[2] and A.dtype == B.dtype
    assert A.stride(2) == 1 and B.stride(2) == 1 and A.is_cuda and A.dtype in _DT
    batch, M, K = A.shape
    N = B.shape[1]
    od = out_dtype or (out.dtype if out is not None else A.dtype)
    if out is None:
        out = torch.empty((batch, M, N), device=A.device, dtype=od)
    assert out.shape == (batch, M, N) and out.stride(2) == 1 and out.dtype == od
    check(lib.gmk_bgemm_nt(_p(A), A.stride(0), A.stride(1), _p(B), B.stride(0), B.stride(1), _p(out), out.stride(0), out.stride(1),
                           batch, M, N, K, float(alpha), _DT[A.dtype], _DT[od], _s()), "bgemm_nt")
    return out


def attention_fwd(qkv, scale, want_p=False, fp8=False):
    """Fused softmax(scale * q k^T) v for qkv [B, N, 3C] (bf16, C = 128, N in {64, 128, 256}) -> (o [B, N, C], P [B, N, N] or None).
    fp8: both contractions on the fp8 (e4m3) matrix cores; q, k and v saturate to +-448, the largest e4m3 magnitude, before the e4m3
    rounding (round to nearest even; NaN stays NaN)."""
    _chk(qkv, torch.bfloat16, "qkv")
    B, N, C3 = qkv.shape
    C = C3 // 3
    o = torch.empty((B, N, C), device=qkv.device, dtype=qkv.dtype)
    P = torch.empty((B, N, N), device=qkv.device, dtype=qkv.dtype) if want_p else None
    check(lib.gmk_attention_fwd(_p(qkv), _p(o), _p(P), B, N, C, float(scale), int(bool(fp8)), _s()), "attention_fwd")
    return o, P


def transpose_last2(x, out=None):
    """[batch, R, C] (unit last stride, free row / batch strides) -> contiguous [batch, C, R]."""
    assert x.dim() == 3 and x.stride(2) == 1 and x.is_cuda and x.dtype in _DT
    batch, R, C = x.shape
    if out is None:
        out = torch.empty((batch, C, R), device=x.device, dtype=x.dtype)
    check(lib.gmk_transpose(_p(x), x.stride(0), x.stride(1), _p(out), out.stride(0), out.stride(1), batch, R, C, _DT[x.dtype], _s()),
          "transpose")
    return out


def attention_bwd_fused_ok(qkv):
    """True if the fused backward of the attention core takes this shape (bf16, C = 128, N in {64, 128, 256}): the forward then need not keep P."""
    return qkv.dtype == torch.bfloat16 and qkv.dim() == 3 and qkv.shape[2] == 384 and qkv.shape[1] in (64, 128, 256) and \
        os.environ.get("GMK_ATTN_BWD", "fused") != "gemm"


def attention_bwd(qkv, o, do):
    """(dq | dk | dv) [B, N, 3C] of o = softmax(scale q k^T) v given do, with P recomputed in registers (gmk_attention_bwd): no N x N matrix in HBM."""
    _chk(qkv, torch.bfloat16, "qkv"); _chk(o, torch.bfloat16, "o"); _chk(do, torch.bfloat16, "do")
    B, N, C3 = qkv.shape
    C = C3 // 3
    assert o.shape == (B, N, C) and do.shape == (B, N, C)
    dqkv = torch.empty_like(qkv)
    stats = torch.empty((B, N, 2), device=qkv.device, dtype=torch.float32)
    check(lib.gmk_attention_bwd(_p(qkv), _p(o), _p(do), _p(dqkv), _p(stats), B, N, C, float(C ** -0.5), _s()), "attention_bwd")
    return dqkv


def softmax_fwd(S, scale, dtype):
    """softmax(scale * S) over the last dimension; S fp32 contiguous -> P in `dtype`."""
    _f32(S, "S")
    N = S.shape[-1]
    P = torch.empty(S.shape, device=S.device, dtype=dtype)
    check(lib.gmk_softmax_fwd(_p(S), _p(P), S.numel() // N, N, float(scale), _DT[dtype], _s()), "softmax_fwd")
    return P


def softmax_bwd(P, dP, scale):
    """dS = scale * P * (dP - sum(dP * P)) per row; dP fp32, P / dS in P.dtype."""
    _chk(P, name="P"); _f32(dP, "dP")
    assert P.shape == dP.shape
    N = P.shape[-1]
    dS = torch.empty_like(P)
    check(lib.gmk_softmax_bwd(_p(P), _p(dP), _p(dS), P.numel() // N, N, float(scale), _DT[P.dtype], _s()), "softmax_bwd")
    return dS
