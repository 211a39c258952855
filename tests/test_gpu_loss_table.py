"""GPU test of the training objective's table: for every `LOSS_TABLE` row, `training_losses` through torch.autograd (the network's Function and
`_LossBridge`) leaves the gradient arena of the fused pass, bit for bit."""
import math
from functools import partial

import pytest
import torch

pytestmark = pytest.mark.gpu

C, S, B = 32, 8, 4          # SimpleUnet(32) on 1 x 8 x 8, the smallest the network takes; four images: 1 / B is a power of two
ROWS = {"snr_trunc": dict(), "snr": dict(loss_weight="snr"), "snr_plus1": dict(loss_weight="snr_plus1"), "min_snr": dict(loss_weight="min_snr"),
        "huber": dict(teacher_mode="consistency", consistency_loss="huber", consistency_grid=8), "hybrid": dict(learn_var=1, vlb_steps=100)}


def _net(seed, learn_var=False):
    """Default-init-scale weights of the reference's inventory (every convolution live); a variance head of the same scale."""
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    from oracle import unet_ref as U
    p = dict(U.reference_init_params(C, seed=seed, zero_out_layers=False))
    if learn_var:
        g = torch.Generator().manual_seed(seed)
        bound = 1.0 / math.sqrt(C * 9)
        p["out_var.weight"] = (torch.rand((1, C, 3, 3), generator=g) * 2 - 1) * bound
        p["out_var.bias"] = (torch.rand((1,), generator=g) * 2 - 1) * bound
    net = SimpleUnet(C, learn_var=learn_var)
    net.load_state_dict(p, strict=True)
    return net.cuda()


@pytest.mark.parametrize("row", sorted(ROWS))
def test_autograd_bridge_leaves_the_fused_pass_gradients(row):
    """(training_losses(...)["loss"].sum() * 0.25).backward() against train_forward_backward(grad_scale=0.25) on the same draws: the bridge
    forms the gradients at grad_scale 1 and scales their rows by 0.25 afterwards, and scaling by a power of two commutes with every rounding
    in them, so the two arenas are equal bit for bit - as are the losses."""
    from generative_models_amd.diffusion.gaussian_diffusion import LOSS_TABLE, GaussianDiffusion, loss_row
    g = torch.Generator().manual_seed(17)
    x = (torch.rand((B, 1, S, S), generator=g) * 2 - 1).cuda()
    eps = torch.randn((B, 1, S, S), generator=g).cuda()
    draws = dict(x=x, eps=eps, u=torch.tensor([0.15, 0.4, 0.65, 0.9]).cuda())
    opts = dict(ROWS[row])
    if "teacher_mode" in opts:              # the discrete-time mode takes its times and the guidance weights instead of u
        opts["teacher_net"] = _net(1).eval()
        draws.update(i_times=torch.tensor([5, 0, 7, 2]).cuda(), cond_w=(4.0 * torch.rand((B,), generator=g)).cuda())
    d = GaussianDiffusion(mean_type="v", num_steps=4, **opts)
    assert loss_row(d) is LOSS_TABLE[row]
    net = _net(2, learn_var=row == "hybrid")
    call = partial(net, guide=torch.tensor([3, -1, 0, 9]).cuda())
    net.zero_grad_arena()
    fused_out = d.train_forward_backward(net=call, grad_scale=0.25, **draws)
    torch.cuda.synchronize()
    fused = net.flat_grads.clone()
    net.zero_grad_arena()
    m = d.training_losses(net=call, **draws)
    (m["loss"].sum() * 0.25).backward()
    torch.cuda.synchronize()
    diff = float((net.flat_grads - fused).abs().max())
    print(f"{row}: largest |gradient| {float(fused.abs().max()):.3e}, largest difference {diff:.3e}")
    assert bool(torch.isfinite(fused).all()) and float(fused.abs().max()) > 0.0
    assert torch.equal(m["loss"].detach(), fused_out["loss"])
    assert torch.equal(net.flat_grads, fused)
