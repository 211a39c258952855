"""GPU tests of the continuous-time variational bound (an extension; `GaussianDiffusion.nll`, `DiffusionModel.nlogp`, DG.nlogp_samples): the three
kernels against the float64 restatement (tests/vlb_ref.py), the known answer of a network whose output is zero, whole bounds against the oracle
U-Net pushed through the restatement with the same draws, and the plugin surface."""
import math
import os
import re
import subprocess
import sys
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import vlb_ref  # noqa: E402


def _rel(got, ref, atol=0.0):
    """max over images of |got - ref| / (|ref| + atol)"""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return float(((got - ref).abs() / (ref.abs() + atol)).max())


def _inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    B = shape[0]
    x = torch.rand(shape, generator=g) * 2 - 1
    eps, out = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    logsnr = torch.rand((B,), generator=g) * 40 - 20
    logsnr[0], logsnr[1] = 20.0, -20.0                                   # the end points themselves
    return x, eps, out, logsnr


SHAPES = [(7, 3, 5, 7), (7, 3, 8, 8), (5, 3, 32, 33), (3, 4, 32, 32)]     # B odd, rows of odd length and of 4k floats, several blocks a row


@pytest.mark.parametrize("shape", SHAPES)
def test_q_sample_logsnr_kernel(shape):
    from generative_models_amd import ops
    x, eps, _, logsnr = _inputs(shape, 1)
    z = ops.q_sample_logsnr(x.cuda(), eps.cuda(), logsnr.cuda())
    ref = vlb_ref.q_sample(x, eps, logsnr)
    assert float((z.cpu().double() - ref).abs().max()) <= 4e-7 * float(ref.abs().max())


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("mean_type", ["v", "eps", "x"])
def test_vlb_term_kernel(shape, mean_type):
    """acc += weight * sum (eps - eps_hat)^2 per image, to 1e-5 relative; accumulates onto what acc holds."""
    from generative_models_amd import ops
    x, eps, out, logsnr = _inputs(shape, 2)
    B = shape[0]
    z = vlb_ref.q_sample(x, eps, logsnr).float()
    weight = torch.rand((B,), generator=torch.Generator().manual_seed(3)) + 0.5
    acc0 = torch.rand((B,)) * 100
    acc = ops.vlb_term(out.cuda(), z.cuda(), eps.cuda(), logsnr.cuda(), weight.cuda(), acc0.cuda(), mean_type=mean_type)
    ref = acc0.double() + weight.double() * vlb_ref.sq_err(out, z, eps, logsnr, mean_type)
    assert _rel(acc, ref) <= 1e-5


def test_vlb_term_kernel_x_prediction_near_lambda_max():
    """mean_type 'x' with a nearly perfect prediction (out = x + 1e-2 N) at lambda near 20: eps_hat = (z - alpha out) / sigma divides the
    cancellation z - alpha out by sigma ~ 4.5e-5, so the fp32 rounding of z itself (ulp(x) / sigma ~ 1e-3 per element) enters against
    |eps - eps_hat| ~ 1e-2 / sigma ~ 220: a looser bar, 1e-4."""
    from generative_models_amd import ops
    x, eps, _, _ = _inputs((6, 3, 8, 8), 4)
    out = x + 1e-2 * torch.randn(x.shape, generator=torch.Generator().manual_seed(5))
    logsnr = torch.tensor([20.0, 19.9, 19.0, 18.0, 15.0, 10.0])
    z = vlb_ref.q_sample(x, eps, logsnr).float()
    acc = ops.vlb_term(out.cuda(), z.cuda(), eps.cuda(), logsnr.cuda(), torch.ones(6).cuda(), torch.zeros(6).cuda(), mean_type="x")
    ref = vlb_ref.sq_err(out, z, eps, logsnr, "x")
    assert _rel(acc, ref) <= 1e-4


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("binarised", [False, True])
def test_vlb_endpoints_kernel(shape, binarised):
    """Prior and decoder against the restatement, on-grid, edge and off-grid values (the pad32 zeros of [-1, 1] data), and a few eps_0 far
    outside any normal draw so that the decoder term is not ~0: 1e-5 relative per image (an absolute 1e-30 for terms that are 0)."""
    from generative_models_amd import ops
    g = torch.Generator().manual_seed(6)
    B = shape[0]
    if binarised:
        x, delta = (torch.rand(shape, generator=g) > 0.5).float(), 0.5
        x.view(B, -1)[:, :4] = torch.tensor([0.0, 0.0, 1.0, 0.0])         # so that each far draw below lands on a finite edge
    else:
        x, delta = torch.randint(0, 256, shape, generator=g).float() / 127.5 - 1, 1.0 / 255
        x.view(B, -1)[:, :5] = torch.tensor([1.0, -1.0, 0.0, 0.0, 1.0])    # the edges and the off-grid zero
    eps0 = torch.randn(shape, generator=g)
    far = eps0.view(B, -1)
    far[1:, 0] = 90.0 if not binarised else 1.2e4                         # [-1, 1]: the top value, whose open edge faces the draw (0 loss)
    far[1:, 1] = 1e3 if not binarised else 2e4                            # a finite edge far away
    far[2:, 2] = -95.0 if not binarised else -1.5e4
    far[3:, 3] = 87.0
    prior, dec = ops.vlb_endpoints(x.cuda(), eps0.cuda(), delta)
    rp, rd = vlb_ref.endpoints(x, eps0, delta)
    assert bool(torch.isfinite(prior).all()) and bool(torch.isfinite(dec).all())
    assert _rel(prior, rp) <= 1e-5
    assert _rel(dec, rd, atol=1e-30) <= 1e-5
    assert float(rd[1:].min()) > 1.0                                      # the far draws did reach the decoder term


def _net(dtype, C=128, in_channels=1, attention=False, seed=0, zero_out=False):
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    params = U.reference_init_params(C, in_channels, seed=seed, zero_out_layers=False, attention=attention)
    if zero_out:
        params["out.2.weight"].zero_()
        params["out.2.bias"].zero_()
    net = SimpleUnet(C, 0.0, in_channels=in_channels, compute_dtype=dtype, attention=attention)
    net.load_state_dict(params, strict=True)
    return net.cuda().eval(), params


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_known_answer_of_a_zero_output_net(dtype):
    """out.2 zeroed: the net outputs v = 0 exactly, so eps - eps_hat = alpha (alpha eps - sigma x) and E[diffusion] = 9.5 + mean(x^2) / 2 nats/dim
    (vlb_ref.zero_output_diffusion; the prior and decoder terms are < 1e-8).  B K = 1024 draws; the batch mean within 4 standard errors of its
    expectation.  The same call twice gives the same bits."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    net, _ = _net(dtype, zero_out=True)
    B, K = 256, 4
    x = torch.rand((B, 1, 8, 8), generator=torch.Generator().manual_seed(7)) * 2 - 1
    y = torch.full((B,), -1, dtype=torch.long).cuda()
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    r = d.nll(net=partial(net, guide=y), x=x.cuda(), num_samples=K)
    assert all(v.shape == (B,) and v.dtype == torch.float32 for v in r.values())
    expect = vlb_ref.zero_output_diffusion(x) / x[0].numel()
    se = float(r["se"].double().pow(2).sum().sqrt()) / B
    dev = float(r["nlogp"].double().mean()) - float(expect.mean())
    assert abs(dev) <= 4 * se, (dev, se)
    assert 0 < se < 0.6, se                                               # ~ 0.3: the naive formula is conservative under stratification
    assert float(r["prior"].max()) < 1e-8 and float(r["decoder"].abs().max()) < 1e-8
    assert torch.allclose(r["nlogp"], r["prior"] + r["decoder"] + r["diffusion"], rtol=1e-6, atol=0)
    again = d.nll(net=partial(net, guide=y), x=x.cuda(), num_samples=K)
    assert all(torch.equal(r[k], again[k]) for k in r)
    other = d.nll(net=partial(net, guide=y), x=x.cuda(), num_samples=K, seed=1)
    assert not torch.equal(r["nlogp"], other["nlogp"])


ORACLE_CASES = [  # (compute dtype, in_channels, attention, mean_type, image size, bar)
    (torch.float32, 1, False, "v", 8, 1e-4),
    (torch.float32, 3, True, "eps", 16, 1e-4),
    (torch.float32, 4, False, "x", 8, 1e-4),
    (torch.bfloat16, 1, False, "v", 8, 1e-2),
]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: f"{str(c[0])[6:]}-c{c[1]}-attn{int(c[2])}-{c[3]}")
def test_bound_against_the_oracle(case):
    """B = 4, K = 2: the per-image bound of `nll` against the oracle U-Net (oracle.unet_ref.unet_forward, fp32 on the CPU) pushed through the
    float64 restatement with the same Philox draws (regenerated in the documented order: u0, eps_0 ... eps_{K-1}, eps_0 of the decoder)."""
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, PhiloxStream
    from oracle import unet_ref as U
    dtype, cin, attn, mean_type, S, bar = case
    net, params = _net(dtype, in_channels=cin, attention=attn, seed=2)
    B, K = 4, 2
    x = torch.rand((B, cin, S, S), generator=torch.Generator().manual_seed(8)) * 2 - 1
    y = torch.tensor([1, 7, -1, 5])
    d = GaussianDiffusion(mean_type=mean_type, num_steps=4)
    r = d.nll(net=partial(net, guide=y.cuda()), x=x.cuda(), num_samples=K, seed=3)
    rng = PhiloxStream(3)
    u0 = rng.uniform((B,), "cuda").cpu()
    eps = torch.stack([rng.normal(x.shape, "cuda").cpu() for _ in range(K)])
    eps0 = rng.normal(x.shape, "cuda").cpu()
    with torch.no_grad():
        ref = vlb_ref.estimate(x, u0, eps, eps0, lambda z, l: U.unet_forward(params, z.float(), l.float(), guide=y), 1.0 / 255, mean_type)
    errs = {k: _rel(r[k], ref[k]) for k in ("nlogp", "diffusion", "se")}
    print(f"nll vs oracle {case[:5]}: relative error per image {errs}")
    assert errs["nlogp"] <= bar and errs["diffusion"] <= bar, errs
    assert _rel(r["prior"], ref["prior"]) <= 1e-5 and float((r["decoder"].cpu().double() - ref["decoder"]).abs().max()) < 1e-12


def test_no_dropout_whatever_the_training_flag():
    from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    net = SimpleUnet(128, 0.3)
    net.load_state_dict(U.reference_init_params(128, zero_out_layers=False))
    net = net.cuda()
    x = (torch.rand((6, 1, 8, 8), generator=torch.Generator().manual_seed(9)) * 2 - 1).cuda()
    y = torch.full((6,), -1, dtype=torch.long).cuda()
    d = GaussianDiffusion(mean_type="v", num_steps=4)
    net.train()
    a = d.nll(net=partial(net, guide=y), x=x, num_samples=2)["nlogp"]
    assert net.training                                                   # the flag is restored
    net.eval()
    b = d.nll(net=partial(net, guide=y), x=x, num_samples=2)["nlogp"]
    assert torch.equal(a, b)


# ---- the plugin -----------------------------------------------------------------------------------------------------------------------
def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=1e-3, pad32=0, device="cuda", bs=8, seed=3, timesteps=8)
    G.update(flags)
    torch.manual_seed(0)
    return Model(G).to("cuda")


def _batch(B=8, seed=5, binarize=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand((B, 1, 28, 28), generator=g)
    x = (x > 0.5).float() if binarize else x * 2 - 1
    return x.cuda(), torch.randint(0, 10, (B,), generator=g).cuda()


def test_loss_keys_and_values():
    """nlogp_samples = 0: loss() returns what it returned before the bound existed (the training objective's test loss, one key); > 0: the same
    loss bits plus `nlogp` (the unconditional batch mean of nlogp(), nats/dim) and `bpd`."""
    x, y = _batch()
    off = _model()
    with torch.no_grad():
        loss, metrics = off.loss(x, y)
    assert set(metrics) == {"loss"} and metrics["loss"] is loss
    twin = _model()                                                        # the pre-existing test loss, spelled out
    with torch.no_grad():
        expect = twin.diffusion.training_losses(net=partial(twin.net, guide=y), x=x)["loss"].mean()
    assert torch.equal(loss, expect)
    on = _model(nlogp_samples=4)
    with torch.no_grad():
        loss4, m4 = on.loss(x, y)
    assert set(m4) == {"loss", "nlogp", "bpd"} and torch.equal(loss4, loss)
    ref = on.nlogp(x)
    assert torch.equal(m4["nlogp"], ref["nlogp"].mean())
    assert float(m4["bpd"]) == pytest.approx(float(m4["nlogp"]) / math.log(2.0), rel=1e-6)
    assert 0.0 < float(m4["nlogp"]) < 30.0


def test_binarised_data_use_the_half_bins():
    x, _ = _batch(binarize=True)
    m = _model(binarize=1, nlogp_samples=2)
    r = m.nlogp(x)
    d = m.diffusion.nll(net=partial(m.net, guide=torch.full((8,), -1, device="cuda")), x=x, num_samples=2, delta=0.5)
    assert all(torch.equal(r[k], d[k]) for k in r)
    assert float(r["decoder"].abs().max()) == 0.0 and bool(torch.isfinite(r["nlogp"]).all())


def test_nlogp_uses_the_ema_net():
    m = _model(ema_decay=0.9, nlogp_samples=2)
    m.train()
    for s in range(3):
        m.train_step(*_batch(seed=10 + s))
    x, y = _batch()
    got = m.nlogp(x)
    guide = torch.full((8,), -1, dtype=torch.long, device="cuda")
    on_ema = m.diffusion.nll(net=partial(m.ema_net, guide=guide), x=x, num_samples=2, delta=1 / 255)
    on_raw = m.diffusion.nll(net=partial(m.net, guide=guide), x=x, num_samples=2, delta=1 / 255)
    assert all(torch.equal(got[k], on_ema[k]) for k in got)
    assert not torch.equal(got["nlogp"], on_raw["nlogp"])
    # labels give -log p(x | y) (the initial net's zeroed output layer ignores them; three steps later it does not)
    assert not torch.equal(m.nlogp(x, y)["nlogp"], got["nlogp"])


def test_cli_logs_eval_nlogp(tmp_path):
    import yaml
    run = tmp_path / "run"
    r = subprocess.run([sys.executable, "-m", "generative_models_amd.main", "--model=diffusion", "--epochs=1", "--bs", "8", "--timesteps", "4",
                        "--nlogp_samples", "2", "--train_batches", "2", "--test_batches", "1", "--eval_heavy", "0", "--save_n", "1",
                        "--logdir", str(run)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    vals = [float(v) for v in re.findall(r"^eval/nlogp (\S+)$", r.stdout, flags=re.M)]
    bpd = [float(v) for v in re.findall(r"^diffusion/test/bpd (\S+)$", r.stdout, flags=re.M)]
    assert len(vals) == 2 and len(bpd) == 2, r.stdout[-3000:]                           # the evaluation before and after the epoch
    assert all(math.isfinite(v) and v > 0.0 for v in vals), vals
    # before training the output layer is zero: every draw is 20 alpha^2 (alpha^2 |eps|^2 + ...) / D, about 20 nats/dim at most.  After two
    # Adam steps the bound has no such ceiling (the first steps move every output weight by ~ lr whatever its gradient): finite is all it owes
    assert vals[0] < 30.0, vals
    assert all(b == pytest.approx(v / math.log(2.0), rel=1e-5) for v, b in zip(vals, bpd)), (vals, bpd)
    with open(run / "hps.yaml") as f:
        assert yaml.load(f, Loader=yaml.Loader)["nlogp_samples"] == 2
