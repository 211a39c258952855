"""GPU tests of the profile labels: the name ops.PROFILE records for a launch is the name of the kernel id the C launcher reported
(include/gmk.h's kernel table), for the stem / head convolutions one by one and for a whole training step and a forward."""
import os
import sys
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_trace  # noqa: E402  (the landmark table of the host trace test; building nothing here)

# what a wrapper's `with _Timed(...)` block is called when the launcher reported nothing: never a kernel's name
FALLBACKS = {"gn_silu_fwd", "gn_stats", "gn_silu_bwd", "gn_silu_fwd_pair", "gn_silu_bwd_pair", "conv_igemm", "conv_subpixel", "conv_wgrad", "stem_fwd",
             "stem_wgrad", "head_fwd", "head_dgrad", "head_wgrad", "stem_dgrad"}
# the wrappers that time one kernel under its own name (fixed=True)
FIXED = {"chansum_kernel", "sumpool2x2_kernel", "batch_gather_kernel", "to_uint8_kernel", "image_grid_kernel", "rng_rademacher_kernel",
         "dequantize_kernel", "pf_ode_step_kernel", "slerp_kernel"}
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from generative_models_amd import ops as o
    return o


@pytest.fixture
def profile(ops):
    ops.PROFILE = []
    try:
        yield ops.PROFILE
    finally:
        ops.PROFILE = None


def rnd(*shape, seed, dtype=F32):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dtype).cuda()


@pytest.mark.parametrize("cs", [1, 3])
@pytest.mark.parametrize("C,dtype", [(128, BF16), (128, F16), (128, F32), (256, BF16)], ids=["c128-bf16", "c128-fp16", "c128-fp32", "c256-bf16"])
def test_stem_and_head_labels_name_the_launched_kernel(ops, profile, C, dtype, cs):
    """One call of each of the six stem / head wrappers (B = 2, 8 x 8; fp16 where the entry accepts it): the recorded name is the landmark
    table's - the kernel the host trace saw launched for this case - and the name of the id the launcher left in gmk_last_kernel."""
    from generative_models_amd._lib import kernel_name, lib
    B, S = 2, 8
    x, dout = rnd(B, cs, S, S, seed=1), rnd(B, cs, S, S, seed=2)
    w_stem, w_head, bias, bias_h = rnd(C, cs, 3, 3, seed=3) / 3, rnd(cs, C, 3, 3, seed=4) / 30, rnd(C, seed=5), rnd(cs, seed=6)
    act, grad = rnd(B, S, S, C, seed=7, dtype=dtype), rnd(B, S, S, C, seed=8, dtype=dtype)
    dw_stem, dwb_head = torch.empty(C * cs * 9, device="cuda"), torch.empty(cs * C * 9 + cs, device="cuda")
    grads = dtype != F16                    # gradient tensors are bf16 or fp32
    calls = [("stem_fwd", lambda: ops.stem_fwd(x, w_stem, bias, C, dtype)),
             ("head_fwd", lambda: ops.head_fwd(act, w_head, bias_h)),
             ("head_wgrad", lambda: ops.head_wgrad(dout, act, dwb_head)),
             ("stem_dgrad", lambda: ops.stem_dgrad(grad, w_stem))]
    if grads:
        calls += [("stem_wgrad", lambda: ops.stem_wgrad(x, grad, dw_stem)), ("head_dgrad", lambda: ops.head_dgrad(dout, w_head, dtype))]
    code = launch_trace.F16 if dtype == F16 else launch_trace.BF16 if dtype == BF16 else launch_trace.F32
    for entry, call in calls:
        del profile[:]
        out = call()
        reported = kernel_name(lib.gmk_last_kernel())
        assert len(profile) == 1 and bool(torch.isfinite(out.float()).all()), (entry, len(profile))
        name = profile[0][0]
        print(entry, C, dtype, cs, "->", name)
        assert name == launch_trace.SMALLCONV_LANDMARKS[(entry, code, C, cs, S, S, 0)] == reported and name not in FALLBACKS, (entry, name, reported)


def test_whole_step_labels_are_table_names(ops, profile):
    """One profiled training pass and one plain forward of SimpleUnet(128) at B = 2, 1 x 8 x 8: every recorded name is a name of the
    kernel table or one of the single-kernel names, none a wrapper's fallback."""
    from generative_models_amd._lib import parse_kernel_table
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    allowed = {name for _, _, name in parse_kernel_table()} | FIXED
    assert not allowed & FALLBACKS
    B, S = 2, 8
    net = SimpleUnet(128, 0.0).cuda()
    g = torch.Generator().manual_seed(0)
    x0 = (torch.rand((B, 1, S, S), generator=g) * 2 - 1).cuda()
    y = torch.tensor([3, -1]).cuda()
    u, eps = torch.rand((B,), generator=g).cuda(), torch.randn((B, 1, S, S), generator=g).cuda()
    side = ops.WGRAD_STREAM
    ops.WGRAD_STREAM = False                # as bench.py profiles: every launch on the stream its events are recorded on
    try:
        out = GaussianDiffusion(mean_type="v", num_steps=3).train_forward_backward(net=partial(net, guide=y), x=x0, grad_scale=1.0 / B, u=u, eps=eps)
        n_train = len(profile)
        v = net.forward_hip(x0, torch.tensor([1.5, -2.0]).cuda(), y, None)
    finally:
        ops.WGRAD_STREAM = side
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out["loss"]).all()) and bool(torch.isfinite(v).all())
    names = [rec[0] for rec in profile]
    print(n_train, "launches in the training pass,", len(names) - n_train, "in the forward:", sorted(set(names)))
    assert n_train > 50 and len(names) - n_train > 20
    assert set(names) <= allowed, sorted(set(names) - allowed)
    for must in ("expand3x3_tile16_kernel", "head_fwd_mfma_kernel", "wgrad3x3_tile16_kernel", "conv3x3_halo_ws_kernel", "gn_silu_fwd_kernel"):
        assert must in names, must
