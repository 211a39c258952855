"""GPU tests at the shapes of BASELINE.json configs[2] / [3] / [4] (3x32x32; 3x64x64; 3x64x64 + self-attention at 256 tokens):
whole-net parity against the oracle at small batch (fp32 1e-3 / bf16 1e-2), and full-batch property tests (determinism,
batch-split equivalence) at the sizes the bench runs.  3-channel inputs and the attention block are extensions of the reference
(parity unpinned - the oracle generalises by the same architectural rule).  Plus the small closures of round 2:
distillation's integer times bit for bit, gradient-bucket finality, in-place torch updates of the parameters, the fixed
`--sample_cond_w` policy, checkpoint / hps.yaml / teacher round trips through the CLI."""
import os
import subprocess
import sys
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
TOL = {torch.float32: 1e-3, torch.bfloat16: 1e-2}


def rel_err(a, b):
    a = a.detach().double().cpu(); b = b.detach().double().cpu()
    return float((a - b).abs().max() / max(1e-6, float(b.abs().max())))


def live_net(dtype, in_channels=1, attention=False, seed=0):
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    params = U.reference_init_params(128, in_channels, seed=seed, zero_out_layers=False, attention=attention)
    net = SimpleUnet(128, 0.0, in_channels=in_channels, compute_dtype=dtype, attention=attention)
    net.load_state_dict(params, strict=True)
    return net.cuda(), params


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("S,B,attention", [(32, 3, False), (64, 2, False), (64, 2, True)],
                         ids=["cfg2-3x32x32", "cfg3-3x64x64", "cfg4-3x64x64-attn256"])
def test_whole_net_at_config_shapes(dtype, S, B, attention):
    """Forward + gradients of the 3-channel net at the config's spatial size against the oracle.  64x64 puts the attention block
    at the 16x16 = 256-token level (configs[4]) and runs the 64-pixel-row instantiations of the halo / slot kernels."""
    from oracle import unet_ref as U
    net, params = live_net(dtype, in_channels=3, attention=attention)
    g = torch.Generator().manual_seed(100 + S + B)
    z = torch.randn((B, 3, S, S), generator=g)
    l = torch.tensor([-6.0, 0.7, 5.0][:B])
    y = torch.tensor([2, -1, 9][:B])
    dout = torch.randn((B, 3, S, S), generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref = U.unet_forward(p, z, l, guide=y)
    ref.backward(dout)
    if attention:
        plain = U.unet_forward({k: v for k, v in params.items() if not k.startswith("attn.")}, z, l, guide=y)
        assert rel_err(plain, ref) > 1e-3                              # the block is live
    ctx = {}
    out = net.forward_hip(z.cuda(), l.cuda(), y.cuda(), None, ctx=ctx)
    tol = TOL[dtype]
    assert rel_err(out, ref) < tol, rel_err(out, ref)
    net.backward_hip(ctx, dout.cuda())
    names = ["down.seq.0.conv.weight", "down.seq.1.in_layers.2.weight", "down.seq.3.conv.weight", "down.seq.6.conv.weight",
             "turn.out_layers.3.weight", "up.seq.0.1.conv.weight", "up.seq.3.1.conv.weight", "up.seq.5.skip_connection.weight",
             "up.seq.6.in_layers.2.weight", "up.seq.6.out_layers.0.weight", "out.2.weight", "time_embed.0.weight",
             "guide_embed.2.bias", "down.seq.2.in_layers.2.bias"]
    if attention:
        names += ["attn.qkv.weight", "attn.proj.weight", "attn.norm.bias"]
    bad = [(n, rel_err(net.grad(n), p[n].grad)) for n in names if rel_err(net.grad(n), p[n].grad) >= (1 if dtype == torch.float32 else 3 if attention else 2) * tol]      # (rounds 1-2: 6x)
    assert not bad, bad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cin,H,W,B", [(1, 12, 12, 5), (1, 20, 20, 3), (3, 36, 36, 2), (1, 44, 44, 2), (3, 24, 40, 3), (1, 52, 28, 2)],
                         ids=["1x12x12", "1x20x20", "3x36x36", "1x44x44", "3x24x40", "1x52x28"])
def test_whole_net_at_sizes_no_config_names(dtype, cin, H, W, B):
    """The reference net is size-agnostic (any H, W divisible by 4: two stride-2 levels, `simple_unet.py:44-72`): sizes that are no power of two,
    rows that fill neither a 64-slot chunk nor a 256-pixel tile, and non-square images - forward and a spread of gradients against the oracle,
    with whatever kernels the dispatch picks at these shapes."""
    from oracle import unet_ref as U
    net, params = live_net(dtype, in_channels=cin)
    g = torch.Generator().manual_seed(7 * H + W + B)
    z = torch.randn((B, cin, H, W), generator=g)
    l = torch.tensor([-6.0, 0.7, 5.0, -1.5, 9.0][:B])
    y = torch.tensor([2, -1, 9, 0, 5][:B])
    dout = torch.randn((B, cin, H, W), generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref = U.unet_forward(p, z, l, guide=y)
    ref.backward(dout)
    ctx = {}
    out = net.forward_hip(z.cuda(), l.cuda(), y.cuda(), None, ctx=ctx)
    tol = TOL[dtype]
    assert rel_err(out, ref) < tol, rel_err(out, ref)
    net.backward_hip(ctx, dout.cuda())
    names = ["down.seq.0.conv.weight", "down.seq.1.in_layers.2.weight", "down.seq.3.conv.weight", "down.seq.6.conv.weight",
             "turn.out_layers.3.weight", "up.seq.0.1.conv.weight", "up.seq.3.1.conv.weight", "up.seq.5.skip_connection.weight",
             "up.seq.6.in_layers.2.weight", "up.seq.6.out_layers.0.weight", "out.2.weight", "time_embed.0.weight",
             "guide_embed.2.bias", "down.seq.2.in_layers.2.bias"]
    bad = [(n, rel_err(net.grad(n), p[n].grad)) for n in names if rel_err(net.grad(n), p[n].grad) >= (1 if dtype == torch.float32 else 2) * tol]
    assert not bad, bad


@pytest.mark.parametrize("B,S,attention", [(2048, 32, False), (1024, 64, False), (512, 64, 1), (512, 64, 2)],
                         ids=["cfg2-B2048-3x32x32", "cfg3-shard-B1024-3x64x64", "cfg4-shard-B512-3x64x64-attn-bf16",
                              "cfg4-shard-B512-3x64x64-attn-fp8"])
def test_full_size_train_step_properties(B, S, attention):
    """The bench's own sizes (bf16): a train step is bit-for-bit reproducible, per-sample losses do not depend on the batch
    they ride in, and the gradient of the batch equals the sum of its halves' gradients (what data parallelism relies on)."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = live_net(torch.bfloat16, in_channels=3, attention=attention, seed=3)
    assert net.attention_fp8 == (attention == 2)            # configs[4] as written: QK^T / PV on the fp8 matrix cores
    d = GaussianDiffusion(mean_type="v", num_steps=1000)
    g = torch.Generator().manual_seed(B + S)
    x = (torch.rand((B, 3, S, S), generator=g) * 2 - 1).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    u = torch.rand((B,), generator=g).cuda()
    eps = torch.randn((B, 3, S, S), generator=g).cuda()
    o1 = d.train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, u=u, eps=eps)
    g1, l1 = net.flat_grads.clone(), o1["loss"].clone()
    o2 = d.train_forward_backward(net=partial(net, guide=y), x=x, grad_scale=1.0 / B, u=u, eps=eps)
    assert torch.equal(o2["loss"], l1) and torch.equal(net.flat_grads, g1)
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    acc, losses = torch.zeros_like(g1), []
    for sl in (slice(0, B // 2), slice(B // 2, B)):
        o = d.train_forward_backward(net=partial(net, guide=y[sl]), x=x[sl], grad_scale=1.0 / B, u=u[sl], eps=eps[sl])
        acc += net.flat_grads; losses.append(o["loss"])
    # a sample's loss does not depend on the batch it rides in - up to the rounding of the few launches whose KERNEL changes with
    # the batch size (the 8x8 level crosses the LDS-DMA kernel's size threshold between B and B/2): one bf16 ulp on a few values
    lh = torch.cat(losses)
    assert float(((lh - l1).abs() / l1.abs().clamp_min(1e-3)).max()) < 2e-3
    assert float((acc - g1).abs().max() / g1.abs().max()) < 5e-3
    # sampler at the same size: final-step select, finite, record=False returns the same bits
    ds = GaussianDiffusion(mean_type="v", num_steps=2, sampler="ddim")
    zs, xs, _ = ds.sample(net=partial(net, guide=y), init_x=eps)
    assert torch.equal(zs[-1], xs[-1]) and bool(torch.isfinite(zs).all()) and float(xs.abs().max()) <= 1.0
    assert torch.equal(ds.sample(net=partial(net, guide=y), init_x=eps, record=False)[0][-1], zs[-1])


@pytest.mark.parametrize("name", ["distill_c64_s8.npz", "distill_c128_s8.npz"])
def test_distillation_integer_times_bit_exact(golden, name):
    """Row I3 (gaussian_diffusion.py:87-91): i ~ randint(T) -> u = (i + 1) / T.  The kernel's u bytes equal the reference's."""
    from generative_models_amd import ops
    g = golden(name)
    i = T(g["step2_i"]).cuda()
    assert i.dtype == torch.int64
    logsnr, u = ops.logsnr_schedule(i.numel(), i.device, i_times=i, num_steps=8, want_u=True)
    assert u.cpu().numpy().tobytes() == g["step2_u"].astype(np.float32).tobytes()
    for steps in (250, 1000):                                          # every i of the two schedules the configs use
        ii = torch.arange(steps, dtype=torch.int64, device="cuda")
        _, uu = ops.logsnr_schedule(steps, ii.device, i_times=ii, num_steps=steps, want_u=True)
        ref = (torch.arange(steps, dtype=torch.int64) + 1).to(torch.float32) / steps       # the reference's expression (:90-91)
        assert uu.cpu().numpy().tobytes() == ref.numpy().tobytes()


def test_fp8_attention_net_vs_oracle():
    """configs[4] as written (`--attention 2`: fp8 e4m3 QK^T / PV) against the ORACLE (fp32 attention_block; parity unpinned: the block has
    no reference counterpart) at the config's shape, 3x64x64 -> 256 tokens.  The block moves this net's output by 1.8e-2 (max-norm;
    1.5e-2 in L2), its fp8 error is 5 - 8 % of the block's own output, so the whole net is held to the 16-bit bar of the north_star,
    1e-2 max-norm - a bar the net without the block misses."""
    from oracle import unet_ref as U
    net, params = live_net(torch.bfloat16, in_channels=3, attention=2)
    g = torch.Generator().manual_seed(8)
    B = 2
    z = torch.randn((B, 3, 64, 64), generator=g); l = torch.tensor([0.5, -3.0]); y = torch.tensor([1, 6])
    with torch.no_grad():
        ref = U.unet_forward(params, z, l, guide=y)
        plain = U.unet_forward({k: v for k, v in params.items() if not k.startswith("attn.")}, z, l, guide=y)
    out = net.forward_hip(z.cuda(), l.cuda(), y.cuda(), None)
    e_max = rel_err(out, ref)
    e_l2 = float((out.cpu().double() - ref.double()).norm() / ref.double().norm())
    assert rel_err(plain, ref) > 1.5e-2                                 # the block is live: dropping it fails the bar below
    assert e_max < 1e-2 and e_l2 < 5e-3, (e_max, e_l2)


def test_fp8_attention_net_vs_bf16_attention_net():
    """`--attention 2` (configs[4]: QK^T / PV on the fp8 matrix cores) against `--attention 1` on the same weights at the config's
    shape (3x64x64 -> 256 tokens): same parameters (166 tensors), outputs within 2e-2 of the output scale (the block is one of
    thirteen residual branches; its own fp8 error is 4e-2 ... 8e-2 of the block output, tests/test_gpu_ops.py)."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    net1, params = live_net(torch.bfloat16, in_channels=3, attention=True)
    net2 = SimpleUnet(128, 0.0, in_channels=3, compute_dtype=torch.bfloat16, attention=2)
    net2.load_state_dict(params, strict=True)
    net2 = net2.cuda()
    assert net2.attention and net2.attention_fp8 and not net1.attention_fp8 and len(net2.state_dict()) == 166
    g = torch.Generator().manual_seed(8)
    z = torch.randn((2, 3, 64, 64), generator=g).cuda(); l = torch.tensor([0.5, -3.0]).cuda(); y = torch.tensor([1, 6]).cuda()
    a, b = net1.forward_hip(z, l, y, None), net2.forward_hip(z, l, y, None)
    e = rel_err(b, a)
    assert 0 < e < 2e-2, e
    # training through the fp8 forward: the fused backward recomputes P in bf16 from the same q, k (straight-through for the e4m3 rounding)
    ctx = {}
    out = net2.forward_hip(z, l, y, None, ctx=ctx)
    net2.backward_hip(ctx, torch.randn_like(out))
    assert bool(torch.isfinite(net2.flat_grads).all()) and float(net2.grad("attn.qkv.weight").abs().max()) > 0


def test_gradient_buckets_are_final_when_handed_over():
    """Data parallelism hands bucket k to the all-reduce at `on_grads_ready(k)`.  The gradient arena is filled with a sentinel, a
    snapshot is taken inside each callback (in stream order, behind the side-stream join): the snapshot must already equal the
    final bucket (nothing writes into it afterwards), and at that moment the next bucket's first weight gradient must not have
    been enqueued yet (the exchange of bucket k overlaps the rest of the backward pass)."""
    net, _ = live_net(torch.bfloat16)
    B, S = 64, 28
    g = torch.Generator().manual_seed(1)
    z = torch.randn((B, 1, S, S), generator=g).cuda(); l = (torch.rand(B, generator=g) * 20 - 10).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda(); dout = torch.randn((B, 1, S, S), generator=g).cuda()
    ctx = {}
    net.forward_hip(z, l, y, None, ctx=ctx)
    SENT = 12345.0
    net.flat_grads.fill_(SENT)
    buckets = net.grad_buckets()
    first_of_next = {0: "up.seq.3.1.conv.weight", 1: "turn.out_layers.3.weight", 2: "time_embed.2.weight"}
    snaps, order, untouched = {}, [], {}
    def ready(k):
        order.append(k)
        s, e = buckets[k]
        snaps[k] = net.flat_grads[s:e].clone()
        if k in first_of_next:
            untouched[k] = bool((net.grad(first_of_next[k]) == SENT).all())
    net.backward_hip(ctx, dout, on_grads_ready=ready)
    torch.cuda.synchronize()
    assert order == [0, 1, 2, 3]
    for k, (s, e) in enumerate(buckets):
        assert torch.equal(snaps[k], net.flat_grads[s:e]), k
    assert untouched == {0: True, 1: True, 2: True}
    live = net.flat_grads != SENT            # everything but alignment padding and the unused cond_w_embed got a gradient
    for n in ("down.seq.0.conv.weight", "up.seq.6.in_layers.2.bias", "out.2.bias", "guide_embed.0.weight", "turn.emb_layers.1.bias"):
        o = net._offsets[n]
        assert bool(live[o:o + net.param(n).numel()].all()), n


def test_inplace_torch_updates_refresh_the_packed_weights():
    """A torch optimiser (or any in-place update through the nn.Parameter views) must not leave the convolutions on stale packs."""
    net, _ = live_net(torch.float32)
    g = torch.Generator().manual_seed(2)
    z = torch.randn((2, 1, 12, 12), generator=g).cuda(); l = torch.tensor([0.3, -2.0]).cuda()
    before = net.forward_hip(z, l)
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    for p in net.parameters():
        p.grad = torch.full_like(p, 0.01)
    opt.step()
    after = net.forward_hip(z, l)
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    fresh = SimpleUnet(128, 0.0, compute_dtype=torch.float32)
    fresh.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    fresh = fresh.cuda()
    assert torch.equal(after, fresh.forward_hip(z, l)) and not torch.equal(after, before)
    with torch.no_grad():
        net.get_parameter("down.seq.1.in_layers.2.weight").mul_(0.5)      # EMA-style in-place edit
    fresh2 = SimpleUnet(128, 0.0, compute_dtype=torch.float32)
    fresh2.load_state_dict({k: v.detach().cpu() for k, v in net.state_dict().items()})
    assert torch.equal(net.forward_hip(z, l), fresh2.cuda().forward_hip(z, l))


def test_small_fused_kernels_replace_stock_torch_ops():
    from generative_models_amd import ops
    B = 1000
    y = torch.randint(0, 10, (B,), device="cuda")
    ref = y.clone()
    ref.masked_fill_(ops.rng_uniform((B,), 77, 5, "cuda") < 0.1, -1)       # diffusion_model.py:67 with the device stream
    ops.label_drop(y, 0.1, 77, 5)
    assert torch.equal(y, ref) and 50 < int((y == -1).sum()) < 150
    x = torch.randn(2048, device="cuda")
    assert abs(float(ops.mean(x)) - float(x.double().mean())) < 1e-6
    a, w = torch.randn(5, 40, device="cuda"), torch.randn(40, 70, device="cuda")
    b1, b2 = torch.randn(70, device="cuda"), torch.randn(70, device="cuda")
    assert rel_err(ops.gemm(a, w, bias=b1, bias2=b2), a @ w + b1 + b2) < 1e-5


def test_sample_cond_w_policy_on_device():
    """`--sample_cond_w 2.0` guides every sampling call, also those that pass no cond_w (`evaluate`): gaussian_diffusion.py:257."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = live_net(torch.float32)
    g = torch.Generator().manual_seed(4)
    init = torch.randn((3, 1, 8, 8), generator=g).cuda(); y = torch.tensor([1, 5, 9]).cuda()
    fixed = GaussianDiffusion(mean_type="v", num_steps=3, sample_cond_w=2.0)
    free = GaussianDiffusion(mean_type="v", num_steps=3, sample_cond_w=-1.0)
    a = fixed.sample(net=partial(net, guide=y), init_x=init)[0]                                   # no cond_w passed
    b = free.sample(net=partial(net, guide=y), init_x=init, cond_w=0.5, net_cond_w=torch.full((3,), 2.0).cuda())[0]
    c = free.sample(net=partial(net, guide=y), init_x=init)[0]                                    # unguided
    assert torch.equal(a, b) and not torch.equal(a, c)


def _cli(args, timeout=900):
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main"] + args, cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [256, 64, 32, 96, 192, 224])
def test_hidden_size_256_vs_oracle_and_through_the_plugin(dtype, C):
    """`--hidden_size 256` (the default of gms/main.py:23; simple_unet.py:17 takes any width): two 128-channel output blocks per
    convolution, 8 / 16 channels per GroupNorm group; `--hidden_size 64 / 32`: zero-padded to one 128-channel tile, 2 / 1 (4 / 2 in the up
    blocks' first GroupNorm) channels per group.  Forward + every gradient against the oracle (itself pinned at these widths by
    tests/golden/*_c256_* / *_c64_* / *_c32_*), then a train step and a guided sample through the plugin surface.  Round 4: every other
    multiple of 32 up to 256 (96: 3 channels per GroupNorm group, padded to 128; 192 / 224: 6 / 7 channels, padded to 256) through the
    explicit-group-size form of the streaming GroupNorm kernels.  Widths above 256 and non-multiples of 32 raise."""
    from generative_models_amd import common
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    B, S = 3, 16
    params = U.reference_init_params(C, 1, seed=5, zero_out_layers=False)
    net = SimpleUnet(C, 0.0, compute_dtype=dtype); net.load_state_dict(params, strict=True); net = net.cuda()
    g = torch.Generator().manual_seed(6)
    z = torch.randn((B, 1, S, S), generator=g); l = torch.tensor([-4.0, 0.3, 6.0]); y = torch.tensor([3, -1, 8])
    dout = torch.randn((B, 1, S, S), generator=g)
    p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
    ref = U.unet_forward(p, z, l, guide=y)
    ref.backward(dout)
    ctx = {}
    out = net.forward_hip(z.cuda(), l.cuda(), y.cuda(), None, ctx=ctx)
    tol = TOL[dtype]
    assert rel_err(out, ref) < tol, rel_err(out, ref)
    net.backward_hip(ctx, dout.cuda())
    gmax = max(float(v.grad.abs().max()) for v in p.values() if v.grad is not None)
    bad = []
    for name, v in p.items():
        if v.grad is None:
            continue
        err = float((net.grad(name).cpu() - v.grad).abs().max())
        # fp32 at the bar of the outputs; 16-bit mode 2x at the native width, 4x for the zero-padded narrow nets (their gradients are small
        # against the floor 1e-3 x the largest gradient entry of the net)
        if err > (1 if dtype == torch.float32 else 2 if C in (128, 256) else 4) * tol * max(float(v.grad.abs().max()), 1e-3 * gmax):
            bad.append((name, err))
    assert not bad, bad[:8]
    for width in (48, 320, 384, 512):
        with pytest.raises(ValueError):
            SimpleUnet(width, 0.0)
    if dtype == torch.bfloat16:
        Model = common.discover_models()["diffusion"]
        G = common.AttrDict(dict(Model.DG)); G.update(hidden_size=C, timesteps=4, bs=8, lr=1e-3, seed=0)
        m = Model(G).cuda(); m.train()
        x = (torch.rand((8, 1, 28, 28), generator=g) * 2 - 1).cuda(); yy = torch.randint(0, 10, (8,), generator=g).cuda()
        l0 = float(m.train_step(x, yy.clone())["loss"])
        for _ in range(5):
            l1 = float(m.train_step(x, yy.clone())["loss"])
        assert np.isfinite(l0) and np.isfinite(l1)
        m.eval()
        s = m.sample(4, yy[:4])
        assert s.shape == (4, 1, 28, 28) and bool(torch.isfinite(s).all())
        sd = m.state_dict()                                   # checkpoints carry the reference's shapes at every width
        assert tuple(sd["net.turn.in_layers.2.weight"].shape) == (C, C, 3, 3) and tuple(sd["net.up.seq.1.in_layers.0.weight"].shape) == (2 * C,)
        m2 = Model(G).cuda(); m2.load_state_dict(sd)
        assert torch.equal(m2.net.flat_params, m.net.flat_params)


def test_cli_at_config_1_flags(tmp_path):
    """BASELINE.json configs[0] as the reference runs it: `python -m gms.main --model=diffusion` at MNIST 28x28x1, bs=32, T=200 (the
    reference's CPU plumbing case; here the same command line on the HIP path): one epoch = eval-first test pass, evaluate() with its
    25-image T=200 sampling, checkpoint, a few train steps - every flag at config 1's literal value."""
    import yaml
    out = _cli(["--model=diffusion", "--bs", "32", "--timesteps", "200", "--epochs=1", "--train_batches", "4", "--test_batches", "2",
                "--logdir", str(tmp_path / "cfg1")])
    assert "diffusion/test/loss" in out and "diffusion/train/loss" in out and "SAVED MODEL" in out
    # DiffusionModel.DG.eval_heavy = 1 (diffusion_model.py:22): with the reference's TorchScript arbiters absent the built-in
    # stand-ins run the heavy eval on the HIP samples (N3): FID / precision / recall / classifier loss are logged
    assert "RUNNING HEAVY EVAL" in out and "DONE HEAVY EVAL" in out
    for key in ("eval/randfeat_fid", "eval/randfeat_precision", "eval/randfeat_recall", "eval/randfeat_f1", "eval/randfeat_cond_fid",
                "eval/centroid_classifier_loss"):
        assert key in out, key
    with open(tmp_path / "cfg1" / "hps.yaml") as f:
        hps = yaml.load(f, Loader=yaml.Loader)
    assert hps["arbiters"] == "stand-in"
    assert hps["bs"] == 32 and hps["timesteps"] == 200 and hps["hidden_size"] == 128 and hps["act_dtype"] in ("fp16", "bf16")
    assert len(torch.load(tmp_path / "cfg1" / "model.pt", map_location="cpu")) == 160


def test_checkpoint_hps_and_teacher_round_trip(tmp_path):
    """gms/main.py:55-64,79-82 and diffusion_model.py:34-45 through the CLI: train one epoch -> model.pt + hps.yaml;
    `--weights_from` re-reads the flags from hps.yaml and continues from the saved weights (test loss of epoch 0 equals the
    saved model's); `--teacher_path` starts a distillation run whose student AND teacher are the saved weights."""
    import yaml
    run = tmp_path / "run"
    base = ["--bs", "8", "--train_batches", "3", "--test_batches", "1"]
    _cli(["--model=diffusion", "--epochs=1", "--timesteps", "4", "--logdir", str(run), "--lr", "1e-3"] + base)
    sd = torch.load(run / "model.pt", map_location="cpu")
    with open(run / "hps.yaml") as f:
        hps = yaml.load(f, Loader=yaml.Loader)
    assert hps["timesteps"] == 4 and hps["model"] == "diffusion" and hps["device"] == "cuda" and len(sd) == 160
    # resume: flags come from hps.yaml (timesteps 4 is not passed again), skip_training keeps the weights as loaded
    out = _cli(["--weights_from", str(run / "model.pt"), "--epochs=1", "--skip_training", "1", "--logdir", str(tmp_path / "resume")] + base)
    assert "SAVED MODEL" in out
    sd2 = torch.load(tmp_path / "resume" / "model.pt", map_location="cpu")
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    with open(tmp_path / "resume" / "hps.yaml") as f:
        hps2 = yaml.load(f, Loader=yaml.Loader)
    assert hps2["timesteps"] == 4 and str(hps2["weights_from"]).endswith("run/model.pt")
    # the loaded weights are what the model computes with: same seeded test batch -> same test loss as a model built from sd
    from generative_models_amd import common
    from generative_models_amd.main import SyntheticMNIST
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG)); G.update(hps)
    m = Model(G).cuda(); m.load_state_dict(sd, strict=False); m.eval()
    x, y = next(iter(SyntheticMNIST(8, 1, 0, hps["binarize"], "cuda", seed=2000)))
    with torch.no_grad():
        want = float(m.loss(x, y)[0])
    got = [float(line.split()[-1]) for line in out.splitlines() if line.startswith("diffusion/test/loss")]
    assert got and abs(got[0] - want) < 1e-3 * max(1.0, abs(want)), (got, want)
    # distillation from the checkpoint: teacher = student = saved weights at start (:34-43)
    out = _cli(["--model=diffusion", "--epochs=1", "--timesteps", "4", "--teacher_path", str(run / "model.pt"), "--teacher_mode", "step2",
                "--logdir", str(tmp_path / "distill")] + base)
    assert "Loading teacher model" in out and "diffusion/train/loss" in out
    G.update(teacher_path=run / "model.pt", teacher_mode="step2")
    dm = Model(G).cuda()
    assert dm.teacher_net is not None and torch.equal(dm.teacher_net.flat_params.cpu(), dm.net.flat_params.cpu())
    assert all(torch.equal(dm.net.state_dict()[k[4:]].cpu(), v) for k, v in sd.items())
    assert all(not p.requires_grad for p in dm.teacher_net.parameters())


SIZED = [("sized_c128_1x64.npz", 1, 64), ("sized_c128_3x32.npz", 3, 32), ("sized_c128_3x64.npz", 3, 64)]
SIZED_REPORT = {}


@pytest.mark.parametrize("forced", [False, True], ids=["auto", "halo+slot"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("name,cin,S", SIZED)
def test_sized_goldens_vs_reference(golden, name, cin, S, dtype, forced):
    """Round 4 (row X1): the HIP path above 32x32 and at 3 image channels against vectors generated by the REFERENCE itself
    (oracle/make_golden.py:gen_sized; the unmodified reference net at 1x64x64, its stem / head re-assigned to 3 channels at 3x32x32 and
    3x64x64).  `forced` runs the kernels the bench-size launches use - the LDS-halo convolution and the slot weight gradient, which the
    dispatcher only picks from 32 tiles up - on the same vectors, so the 64-pixel-row and 32-pixel-row instantiations of both and the
    64x64 resident GroupNorm kernels trace to the reference.  Bars: fp32 1e-3 / 16-bit 1e-2 max-norm on outputs, loss, every gradient norm
    and the stored gradients; DDIM chains 1e-3 / 1e-2 on every intermediate z and x prediction (guided: 5e-3 / 2e-2).
    The GUIDED chain is held to 5e-3 in fp32: its first step (logsnr = -20) recovers the x prediction from the mixed eps prediction as
    sqrt(1 + e^20) * (z - eps * rsqrt(1 + e^-20)) (gaussian_diffusion.py:181-186, diffusion_utils.py:76-82) where z and eps agree to 4.5e-5 of
    their size: fp32 rounding of eps ALONE is 6e-8 / 4.5e-5 = 1.3e-3 of the prediction - the reference's own chain carries that noise (the fp32
    HIP path measures 1.0e-3 there against 6e-7 on the unguided chain of the same net)."""
    from generative_models_amd._lib import lib
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    g = golden(name)
    params = U.reference_init_params(128, cin, seed=int(g["init_seed"]), zero_out_layers=False)
    net = SimpleUnet(128, 0.0, in_channels=cin, compute_dtype=dtype); net.load_state_dict(params, strict=True); net = net.cuda()
    tol = TOL[dtype]
    rep = {}
    if forced:
        if dtype == torch.float32:
            pytest.skip("the halo / slot kernels are 16-bit kernels")
        lib.gmk_set_kernel_choice(3, 2, -1)
    try:
        z, l, y = T(g["z"]).cuda(), T(g["logsnr"]).cuda(), T(g["guide"]).cuda()
        with torch.no_grad():
            rep["v"], rep["v_noguide"] = rel_err(net(z, l, guide=y), T(g["v"])), rel_err(net(z, l), T(g["v_noguide"]))
        assert rep["v"] < tol and rep["v_noguide"] < tol, rep
        diff = GaussianDiffusion(mean_type="v", num_steps=250)
        x0, u, eps = (T(g[k]).cuda() for k in ("x0", "u", "eps"))
        B = x0.shape[0]
        out = diff.train_forward_backward(net=partial(net, guide=y), x=x0, grad_scale=1.0 / B, u=u, eps=eps)
        rep["loss"] = rel_err(out["loss"], T(g["loss_b"]))
        assert rep["loss"] < tol, rep
        names = [str(n) for n in g["grad_names"]]
        norms = torch.stack([net.grad(n).norm() for n in names]).cpu()
        ref = T(g["grad_norms"])
        rep["grad_norms"] = float(((norms - ref).abs() / (ref.abs() + 1e-3 * ref.abs().max())).max())
        ok = (norms - ref).abs() <= tol * ref.abs() + 1e-3 * tol * ref.abs().max()
        assert bool(ok.all()), [(names[i], float(norms[i]), float(ref[i])) for i in (~ok).nonzero().flatten()[:8]]
        for k in g.files:
            if k.startswith("grad__"):
                rep[k] = rel_err(net.grad(k[6:]), T(g[k]))
                assert rep[k] < tol, (k, rep[k])
            elif k.startswith("gradslice__"):
                full = net.grad(k[11:])
                # a slice is judged on the scale of its tensor (the slice may sit where the gradient is small)
                rep[k] = float((full[:4, :6].cpu().double() - T(g[k]).double()).abs().max() / float(full.abs().max()))
                assert rep[k] < tol, (k, rep[k])
        if "chain_T" in g.files:
            steps, init, yc = int(g["chain_T"]), T(g["chain_init"]).cuda(), T(g["chain_y"]).cuda()
            ctol, gtol = (1e-3, 5e-3) if dtype == torch.float32 else (1e-2, 2e-2)      # measured 16-bit: 1.5e-3 / 7.8e-3 (profiles/r04_sized_report.txt)
            ddim = GaussianDiffusion(mean_type="v", num_steps=steps, sampler="ddim", sample_cond_w=-1.0)
            zs, xs, _ = ddim.sample(net=partial(net, guide=yc), init_x=init)
            rep["ddim_zs"], rep["ddim_xs"] = rel_err(zs, T(g["ddim_zs"])), rel_err(xs, T(g["ddim_xs"]))
            zs, _, _ = ddim.sample(net=partial(net, guide=yc), init_x=init, cond_w=0.5, net_cond_w=T(g["cfg_w"]).cuda())
            rep["cfg_zs"] = rel_err(zs, T(g["cfg_zs"]))
            assert max(rep["ddim_zs"], rep["ddim_xs"]) < ctol and rep["cfg_zs"] < gtol, rep
    finally:
        lib.gmk_set_kernel_choice(-1, -1, -1)
        SIZED_REPORT[(name, str(dtype), forced)] = rep
        print("sized", name, dtype, "forced" if forced else "auto", {k: f"{v:.2e}" for k, v in rep.items()})


def test_bench_dump_outputs_are_the_last_timed_step_and_reproducible(tmp_path):
    """`bench.py --dump-outputs DIR`: the headline's last timed train step as a caller holds it (loss, loss_scale, updated parameters and their
    gradients in the reference's shapes), fp32, and bit-identical between two runs with the same arguments (seeded weights, batches and RNG
    streams; every kernel of the step is deterministic).  3x32x32 at a batch above the graphed-step limit: the kernel-by-kernel path of the headline."""
    import json
    from oracle import unet_ref as U
    flags = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "custom", "--batch", "128", "--size", "32", "--in_channels", "3",
             "--sampler_steps", "0", "--others", "0", "--no_cpu"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    runs = []
    for name in ("a", "b"):
        d = tmp_path / name
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + flags + ["--dump-outputs", str(d)], capture_output=True,
                           text=True, timeout=900, cwd=ROOT, env=dict(env, OMP_NUM_THREADS="2", GMK_BENCH_STEADY_STEPS="4",
                                                                      GMK_BENCH_DETAIL=str(tmp_path / f"detail_{name}.json")))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 3 and line["ms_per_step"] > 0
        runs.append({k: np.load(d / f"{k}.npy") for k in ("loss", "loss_scale", "params", "grads")})
    a, b = runs
    n = sum(v.numel() for v in U.reference_init_params(128, 3).values())
    assert all(v.dtype == np.float32 for v in a.values())
    assert a["loss"].shape == () and np.isfinite(a["loss"]) and float(a["loss_scale"]) == 1.0
    assert a["params"].shape == a["grads"].shape == (n,) and np.isfinite(a["grads"]).all() and np.abs(a["grads"]).max() > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_bench_plain_run_is_the_headline_alone(tmp_path):
    """A plain `bench.py` run (no `--full`) times the headline's steps and prints its line: the sampler, steady-state, other-config and CPU
    flags keep their defaults here, and none of those runs happens."""
    import json
    flags = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "custom", "--batch", "64"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GMK_FORCE_EXCHANGE", "GMK_BENCH_STEADY_STEPS")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + flags, capture_output=True, text=True, timeout=600, cwd=ROOT,
                       env=dict(env, OMP_NUM_THREADS="2", GMK_BENCH_DETAIL=str(tmp_path / "detail.json")))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["metric"] == "ddpm_train_images_per_sec" and line["value"] > 0 and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["roofline"]["kernel"].startswith("conv")      # (from the timed steps' own events)
    full = json.load(open(tmp_path / "detail.json"))
    for d in (line, full):
        assert not {"steady_state", "sampler", "other_configs", "cpu_baseline", "exchange"} & {k for k, v in d.items() if v is not None}, sorted(d)
