"""Cost of the weight EMA (DG.ema_decay > 0): the fused Adam + EMA launch against Adam alone, in the whole train step.

    python tools/ema_cost.py ab    [cfg2|bs32] [rounds=6] [steps=10]   same-process, interleaved step times, ema_decay 0 vs 0.9999
    python tools/ema_cost.py trace [cfg2|bs32] [steps=50]              `steps` train steps with EMA off, then `steps` with it on (to run
                                                                          under rocprofv3 --kernel-trace --stats: adam_kernel<false, false>
                                                                          and adam_kernel<true, false> (<EMA, CTL>) side by side)
cfg2: BASELINE configs[2] (3x32x32, bs = 2048, kernel-by-kernel step); bs32: 1x28x28, bs = 32 (the replayed-graph step).  Both print the
arena size and the bytes each optimiser launch moves (28 / 36 B per parameter), to turn kernel times into bandwidth."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import common  # noqa: E402

CONFIGS = {"cfg2": (3, 32, 2048), "bs32": (1, 28, 32)}


def model(cfg, ema_decay):
    cin, size, bs = CONFIGS[cfg]
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=int(size == 32), device="cuda", timesteps=1000, bs=bs, in_channels=cin, ema_decay=ema_decay)
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
    models = {d: model(cfg, d) for d in (0.0, 0.9999)}
    n = models[0.0].net.flat_params.numel()
    print(f"{cfg}: arena {n} floats; adam_kernel<false, false> {28 * n / 1e6:.1f} MB, adam_kernel<true, false> {36 * n / 1e6:.1f} MB per launch", flush=True)
    if mode == "trace":
        k = int(sys.argv[3]) if len(sys.argv) > 3 else 50
        for d, m in models.items():
            steps(m, x, y, 3)
            print(f"ema_decay {d}: {steps(m, x, y, k):.3f} ms per step over {k} steps", flush=True)
        return
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 6
    k = int(sys.argv[4]) if len(sys.argv) > 4 else 10
    for m in models.values():
        steps(m, x, y, 3)
    times = {d: [] for d in models}
    for r in range(rounds):
        for d in (models if r % 2 == 0 else reversed(list(models))):
            times[d].append(steps(models[d], x, y, k))
    med = {d: statistics.median(t) for d, t in times.items()}
    for d, t in times.items():
        print(f"ema_decay {d}: median {med[d]:.3f} ms per step  (rounds: {', '.join(f'{v:.3f}' for v in t)})")
    print(f"EMA on / off: {med[0.9999] / med[0.0] - 1:+.2%}")
    assert torch.equal(models[0.0].net.flat_params, models[0.9999].net.flat_params), "EMA moved the training weights"


if __name__ == "__main__":
    main()
