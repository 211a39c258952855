"""Cost of the weighted x-space loss (DG.loss_weight 'snr_plus1' / 'min_snr', gmk_x_loss_w) against the default objective's gmk_v_loss.

    python tools/loss_weight_cost.py [out=profiles/loss_weight_cost.txt] [rounds=7] [iters=100] [steps=8]

kernel   per shape: time per launch of gmk_x_loss_w ('min_snr', dv on: v, z, x read, dv written, 16 B per value) and of gmk_v_loss (dv on: v, z,
         x, eps read twice, dv written), HIP events around `iters` launches that rotate over enough buffer sets to exceed the 256 MiB
         Infinity Cache; `rounds` rounds, the two kernels interleaved and the order alternating; medians and their ratio.
step     per shape: ms per DiffusionModel.train_step with loss_weight 'min_snr' and with the default 'snr_trunc', same process, `steps` steps
         per round, interleaved the same way.
Shapes: 3x32x32 at B = 2048 and 1x28x28 at B = 1024.  Everything printed is also written to `out`."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402

SHAPES = [(3, 32, 2048), (1, 28, 1024)]
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def event_ms(fn, iters):
    """ms per call of fn(k), k = 0 ... iters - 1, between two device events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel(rounds, iters):
    for cin, size, B in SHAPES:
        n = cin * size * size
        per_tensor = B * n * 4
        sets = max(2, min(64, -(-(640 << 20) // (5 * per_tensor))))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn((B, cin, size, size), device="cuda", generator=g) for _ in range(4)] for _ in range(sets)]      # v, z, x, eps
        logsnr = torch.rand((B,), device="cuda", generator=g) * 40 - 20
        arms = {
            "gmk_x_loss_w": lambda k: ops.x_loss_w(*bufs[k % sets][:3], logsnr, "min_snr", 5.0, grad_scale=1.0 / B),
            "gmk_v_loss": lambda k: ops.v_loss(*bufs[k % sets], logsnr, grad_scale=1.0 / B),
        }
        for fn in arms.values():                    # warm-up over every buffer set
            for k in range(sets):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for r in range(rounds):
            for name in (arms if r % 2 == 0 else reversed(list(arms))):
                times[name].append(event_ms(arms[name], iters))
        med = {name: statistics.median(v) for name, v in times.items()}
        moved = {"gmk_x_loss_w": 4 * per_tensor if n <= ops.X_LOSS_KEEP else 7 * per_tensor, "gmk_v_loss": 9 * per_tensor}
        for name, v in times.items():
            say(f"{cin}x{size}x{size} B={B} {name} (dv on): median {med[name] * 1e3:.1f} us per launch, {moved[name] / 1e6:.1f} MB requested = "
                f"{moved[name] / med[name] / 1e9:.2f} TB/s  (rounds: {', '.join(f'{x * 1e3:.1f}' for x in v)}; {sets} buffer sets)")
        say(f"{cin}x{size}x{size} B={B}: gmk_x_loss_w / gmk_v_loss = {med['gmk_x_loss_w'] / med['gmk_v_loss']:.3f}")
        del bufs, arms


def step(rounds, steps):
    Model = common.discover_models()["diffusion"]
    for cin, size, B in SHAPES:
        models = {}
        for weight in ("snr_trunc", "min_snr"):
            G = common.AttrDict(dict(Model.DG))
            G.update(lr=3e-4, pad32=0, device="cuda", bs=B, in_channels=cin, image_size=size, loss_weight=weight)
            torch.manual_seed(0)
            models[weight] = Model(G).cuda().train()
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand((B, cin, size, size), device="cuda", generator=g) * 2 - 1
        y = torch.randint(0, 10, (B,), device="cuda", generator=g)

        def run(m):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.train_step(x, y.clone())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3
        for m in models.values():
            run(m)
        times = {w: [] for w in models}
        for r in range(rounds):
            for w in (models if r % 2 == 0 else reversed(list(models))):
                times[w].append(run(models[w]))
        med = {w: statistics.median(v) for w, v in times.items()}
        for w, v in times.items():
            say(f"{cin}x{size}x{size} B={B} train_step, loss_weight {w}: median {med[w]:.3f} ms  (rounds: {', '.join(f'{t:.3f}' for t in v)})")
        say(f"{cin}x{size}x{size} B={B}: min_snr / snr_trunc = {med['min_snr'] / med['snr_trunc']:.4f}  ({med['min_snr'] - med['snr_trunc']:+.3f} ms per step)")
        del models


def main():
    args = sys.argv[1:]
    out = args[0] if args else "profiles/loss_weight_cost.txt"
    rounds, iters, steps = (int(args[i]) if len(args) > i else d for i, d in ((1, 7), (2, 100), (3, 8)))
    assert torch.cuda.is_available(), "loss_weight_cost.py measures on the GPU"
    say(f"tools/loss_weight_cost.py on {torch.cuda.get_device_name(0)}: rounds {rounds}, iters {iters}, steps {steps}")
    kernel(rounds, iters)
    step(rounds, steps)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
