"""Cost of the parametrised noise schedules (DG.logsnr_schedule ..., gmk_q_sample_sched) against the default entry gmk_q_sample.

    python tools/schedule_cost.py [out=profiles/schedule_cost.txt] [rounds=7] [iters=100] [steps=8]

kernel   per shape: time per launch of gmk_q_sample_sched for each of the four kinds (range -15 ... 15, shift -0.5, so that no argument is a
         default) and of gmk_q_sample (x and eps read, z written: 12 B per value), HIP events around `iters` launches that rotate over enough
         buffer sets to exceed the 256 MiB Infinity Cache; `rounds` rounds, the arms interleaved and their order alternating; medians and
         each kind's ratio to gmk_q_sample.
step     per shape: ms per DiffusionModel.train_step under logsnr_schedule 'beta_linear' and under two default arms (two models built the
         same way: their spread is what a difference has to exceed), same process, `steps` steps per round, interleaved the same way.
Shapes: 3x32x32 at B = 2048 and 1x28x28 at B = 1024.  Everything printed is also written to `out`."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import SCHEDULE_KINDS, Schedule  # noqa: E402

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


def alternate(arms, r):
    return list(arms) if r % 2 == 0 else list(arms)[::-1]


def kernel(rounds, iters):
    for cin, size, B in SHAPES:
        n = cin * size * size
        per_tensor = B * n * 4
        sets = max(2, min(64, -(-(640 << 20) // (3 * per_tensor))))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn((B, cin, size, size), device="cuda", generator=g) for _ in range(2)] for _ in range(sets)]      # x, eps
        u = torch.rand((B,), device="cuda", generator=g)
        arms = {"gmk_q_sample": lambda k: ops.q_sample(*bufs[k % sets], u)}
        for kind in SCHEDULE_KINDS:
            arms[f"gmk_q_sample_sched {kind}"] = lambda k, S=Schedule(kind, -15.0, 15.0, -0.5): ops.q_sample(*bufs[k % sets], u, schedule=S)
        for fn in arms.values():                    # warm-up over every buffer set
            for k in range(sets):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for r in range(rounds):
            for name in alternate(arms, r):
                times[name].append(event_ms(arms[name], iters))
        med = {name: statistics.median(v) for name, v in times.items()}
        moved = 3 * per_tensor
        for name, v in times.items():
            say(f"{cin}x{size}x{size} B={B} {name}: median {med[name] * 1e3:.1f} us per launch, {moved / 1e6:.1f} MB requested = "
                f"{moved / med[name] / 1e9:.2f} TB/s  (rounds: {', '.join(f'{x * 1e3:.1f}' for x in v)}; {sets} buffer sets)")
        say(f"{cin}x{size}x{size} B={B}: against gmk_q_sample " +
            ", ".join(f"{kind} {med[f'gmk_q_sample_sched {kind}'] / med['gmk_q_sample']:.3f}" for kind in SCHEDULE_KINDS))
        del bufs, arms


def step(rounds, steps):
    Model = common.discover_models()["diffusion"]
    for cin, size, B in SHAPES:
        models = {}
        for arm, flags in (("default (a)", {}), ("beta_linear", {"logsnr_schedule": "beta_linear"}), ("default (b)", {})):
            G = common.AttrDict(dict(Model.DG))
            G.update(lr=3e-4, pad32=0, device="cuda", bs=B, in_channels=cin, image_size=size, **flags)
            torch.manual_seed(0)
            models[arm] = Model(G).cuda().train()
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
        times = {arm: [] for arm in models}
        for r in range(rounds):
            for arm in alternate(models, r):
                times[arm].append(run(models[arm]))
        med = {arm: statistics.median(v) for arm, v in times.items()}
        for arm, v in times.items():
            say(f"{cin}x{size}x{size} B={B} train_step, {arm}: median {med[arm]:.3f} ms  (rounds: {', '.join(f'{t:.3f}' for t in v)})")
        base = 0.5 * (med["default (a)"] + med["default (b)"])
        say(f"{cin}x{size}x{size} B={B}: beta_linear / default = {med['beta_linear'] / base:.4f}  ({med['beta_linear'] - base:+.3f} ms per step; "
            f"the two default arms differ by {abs(med['default (a)'] - med['default (b)']):.3f} ms)")
        del models


def main():
    args = sys.argv[1:]
    out = args[0] if args else "profiles/schedule_cost.txt"
    rounds, iters, steps = (int(args[i]) if len(args) > i else d for i, d in ((1, 7), (2, 100), (3, 8)))
    assert torch.cuda.is_available(), "schedule_cost.py measures on the GPU"
    say(f"tools/schedule_cost.py on {torch.cuda.get_device_name(0)}: rounds {rounds}, iters {iters}, steps {steps}")
    kernel(rounds, iters)
    step(rounds, steps)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
