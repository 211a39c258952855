"""Cost of the steered optimiser step (DG.grad_clip / DG.skip_nonfinite): the gradient-norm launches and the steered Adam launch against
Adam alone, in the whole train step.

    python tools/clip_cost.py ab    [cfg2|bs32] [rounds=6] [steps=10]   same-process, interleaved step times, flags off vs
                                                                           --grad_clip 1.0 --skip_nonfinite 1
    python tools/clip_cost.py trace [cfg2|bs32] [steps=50]              `steps` train steps with the flags off, then `steps` with them on (to
                                                                           run under rocprofv3 --kernel-trace --stats: adam_kernel<false, false>
                                                                           next to grad_norm_partial_kernel, grad_norm_final_kernel and
                                                                           adam_kernel<false, true> (<EMA, CTL>))
cfg2: BASELINE configs[2] (3x32x32, bs = 2048, kernel-by-kernel step); bs32: 1x28x28, bs = 32 (the replayed-graph step).  Both print the
arena size and the bytes each launch moves (4 B per parameter for the norm, 28 for either Adam), to turn kernel times into bandwidth.  The
flags-off arm is the step as it was before the flags existed: no new kernel is launched in it."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import common  # noqa: E402

CONFIGS = {"cfg2": (3, 32, 2048), "bs32": (1, 28, 32)}
ARMS = {"off": {}, "on": dict(grad_clip=1.0, skip_nonfinite=1)}


def model(cfg, flags):
    cin, size, bs = CONFIGS[cfg]
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=int(size == 32), device="cuda", timesteps=1000, bs=bs, in_channels=cin)
    G.update(flags)
    torch.manual_seed(0)
    return Model(G).cuda().train()


def batch(cfg):
    cin, size, bs = CONFIGS[cfg]
    g = torch.Generator().manual_seed(1)
    return (torch.rand((bs, cin, size, size), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (bs,), generator=g).cuda()


def steps(m, x, y, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        m.train_step(x, y.clone())
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def main():
    mode = sys.argv[1]
    cfg = sys.argv[2] if len(sys.argv) > 2 else "cfg2"
    x, y = batch(cfg)
    models = {arm: model(cfg, flags) for arm, flags in ARMS.items()}
    n = models["off"].net.flat_params.numel()
    print(f"{cfg}: arena {n} floats; grad_norm_partial_kernel {4 * n / 1e6:.1f} MB, adam_kernel<false, false> / adam_kernel<false, true> {28 * n / 1e6:.1f} MB per launch",
          flush=True)
    if mode == "trace":
        k = int(sys.argv[3]) if len(sys.argv) > 3 else 50
        for arm, m in models.items():
            steps(m, x, y, 3)
            print(f"flags {arm}: {steps(m, x, y, k):.3f} ms per step over {k} steps", flush=True)
        return
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    k = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    for m in models.values():
        steps(m, x, y, 3)
    times = {arm: [] for arm in models}
    for r in range(rounds):
        for arm in (models if r % 2 == 0 else reversed(list(models))):
            times[arm].append(steps(models[arm], x, y, k))
    med = {arm: statistics.median(t) for arm, t in times.items()}
    for arm, t in times.items():
        print(f"flags {arm}: median {med[arm]:.3f} ms per step  (rounds: {', '.join(f'{v:.3f}' for v in t)})")
    print(f"clip + guard on / off: {med['on'] / med['off'] - 1:+.2%}")
    st = models["on"].optimizer.ctl_state.tolist()
    print(f"last step: grad_norm {st[0]:.4g}, coefficient {st[1]:.4g}, skipped steps {st[3]:.0f}")


if __name__ == "__main__":
    main()
