"""Cost of the loss profile and the loss-aware time sampler (DG.time_importance, gmk_loss_profile / gmk_u_importance).

    python tools/time_importance_cost.py [out=profiles/time_importance_cost.txt] [rounds=7] [iters=200] [steps=8]

kernel   per shape: time per launch of gmk_loss_profile (u, v0, v1 of B values into the [5, 64] state; one workgroup) and of gmk_u_importance
         (B draws from a ready, steep state), HIP events around `iters` launches, against gmk_v_loss (dv on) at the same shape in the same
         run, its buffers rotating over enough sets to exceed the 256 MiB Infinity Cache; `rounds` rounds, the order alternating; medians.
step     per shape: ms per DiffusionModel.train_step with time_importance 1 (the sampler live: B >= 1024 fills every bin past the warm-up count
         in the first step) and of TWO models with the default flags, same process, `steps` steps per round, interleaved the same way.  The
         two default arms show the same-box noise the ratio has to be read against.
Shapes: 3x32x32 at B = 2048 and 1x28x28 at B = 1024.  Everything printed is also written to `out`.  Nothing here measures convergence or
the variance of the gradient: only what the feature costs per step."""
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


def steep_state():
    """A ready state with r_k = sqrt(S2 / W) rising over e^14 across the bins."""
    k = torch.arange(ops.PROFILE_BINS, dtype=torch.float64)
    r = torch.exp(14.0 * (k / (ops.PROFILE_BINS - 1) - 0.5))
    state = torch.zeros((5, ops.PROFILE_BINS), dtype=torch.float64)
    state[0] = 8.0
    state[1], state[2] = 8.0 * r, 8.0 * r * r
    state[3:] = 8.0
    return state.float().cuda()


def kernel(rounds, iters):
    for cin, size, B in SHAPES:
        n = cin * size * size
        per_tensor = B * n * 4
        sets = max(2, min(64, -(-(640 << 20) // (5 * per_tensor))))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn((B, cin, size, size), device="cuda", generator=g) for _ in range(4)] for _ in range(sets)]      # v, z, x, eps
        logsnr = torch.rand((B,), device="cuda", generator=g) * 40 - 20
        u0 = torch.rand((B,), device="cuda", generator=g)
        v0, v1 = torch.rand((B,), device="cuda", generator=g), torch.rand((B,), device="cuda", generator=g)
        ready, filling = steep_state(), torch.zeros((5, ops.PROFILE_BINS), device="cuda")
        arms = {
            "gmk_loss_profile": lambda k: ops.loss_profile(u0, v0, v1, filling, 0.9),
            "gmk_u_importance": lambda k: ops.u_importance(ready, u0, 5.0, 0.01),
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
        for name, v in times.items():
            say(f"{cin}x{size}x{size} B={B} {name}: median {med[name] * 1e3:.1f} us per launch  (rounds: {', '.join(f'{x * 1e3:.1f}' for x in v)})")
        say(f"{cin}x{size}x{size} B={B}: (gmk_loss_profile + gmk_u_importance) / gmk_v_loss = "
            f"{(med['gmk_loss_profile'] + med['gmk_u_importance']) / med['gmk_v_loss']:.3f}")
        del bufs, arms


def step(rounds, steps):
    Model = common.discover_models()["diffusion"]
    for cin, size, B in SHAPES:
        models = {}
        for arm, flag in (("default A", 0), ("time_importance 1", 1), ("default B", 0)):
            G = common.AttrDict(dict(Model.DG))
            G.update(lr=3e-4, pad32=0, device="cuda", bs=B, in_channels=cin, image_size=size, time_importance=flag)
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
        p = models["time_importance 1"].diffusion.profile("train")["p"]
        say(f"{cin}x{size}x{size} B={B}: after the warm-up round the sampler's p spans {p.min():.5f} ... {p.max():.5f} (uniform: {1 / 64:.5f})")
        times = {arm: [] for arm in models}
        for r in range(rounds):
            for arm in (models if r % 2 == 0 else reversed(list(models))):
                times[arm].append(run(models[arm]))
        med = {arm: statistics.median(v) for arm, v in times.items()}
        for arm, v in times.items():
            say(f"{cin}x{size}x{size} B={B} train_step, {arm}: median {med[arm]:.3f} ms  (rounds: {', '.join(f'{t:.3f}' for t in v)})")
        base = 0.5 * (med["default A"] + med["default B"])
        say(f"{cin}x{size}x{size} B={B}: default B / default A = {med['default B'] / med['default A']:.4f} (same-box noise);  time_importance 1 / "
            f"default (mean of A, B) = {med['time_importance 1'] / base:.4f}  ({med['time_importance 1'] - base:+.3f} ms per step)")
        del models


def main():
    args = sys.argv[1:]
    out = args[0] if args else "profiles/time_importance_cost.txt"
    rounds, iters, steps = (int(args[i]) if len(args) > i else d for i, d in ((1, 7), (2, 200), (3, 8)))
    assert torch.cuda.is_available(), "time_importance_cost.py measures on the GPU"
    say(f"tools/time_importance_cost.py on {torch.cuda.get_device_name(0)}: rounds {rounds}, iters {iters}, steps {steps}")
    kernel(rounds, iters)
    step(rounds, steps)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
