"""Cost of consistency distillation and of the multistep consistency sampler's update (teacher_mode / sampler 'consistency').

    python tools/consistency_cost.py kernel [out] [rounds=7] [iters=200]     per shape: time per gmk_consistency_step launch (v and z read, z_next
                                                                             written, the noise drawn in the kernel: 12 B per value) against the
                                                                             pair it replaces, gmk_rng_normal + gmk_sampler_step(noise=...) (the
                                                                             noise written and read back: 20 B per value), HIP events around `iters`
                                                                             launches that rotate over enough buffer sets to exceed the 256 MiB
                                                                             Infinity Cache; `rounds` rounds, the order alternating; medians
    python tools/consistency_cost.py train [out] [rounds=5] [steps=4]        per shape: ms per DiffusionModel.train_step under teacher_mode 'step2'
                                                                             and 'consistency' (consistency_loss 'l2' and 'huber'; the student is
                                                                             its own target net), same process, `steps` steps per round, interleaved,
                                                                             the order alternating.  Three forwards and one backward in every arm.
    python tools/consistency_cost.py all [out]                               both
Shapes: the bench's three, 1x28x28 B = 1024, 3x32x32 B = 2048, 3x64x64 B = 1024.  Everything printed is also written to `out` (default
profiles/consistency_cost.txt).  Reports, not assertions; nothing here measures sample quality or convergence."""
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402

SHAPES = [(1, 28, 1024), (3, 32, 2048), (3, 64, 1024)]
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


def spread(v):
    return f"{min(v):.4g} ... {max(v):.4g}"


def kernel(rounds, iters):
    lt, ls, seed = -1.0, 0.5, 7
    for cin, size, B in SHAPES:
        n = cin * size * size
        shape = (B, cin, size, size)
        nbytes = 3 * B * n * 4
        sets = max(2, min(64, -(-(640 << 20) // nbytes)))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn(shape, device="cuda", generator=g) for _ in range(2)] for _ in range(sets)]      # v, z
        q = B * n // 4

        def fused(k):
            v, z = bufs[k % sets]
            ops.consistency_step(v, z, lt, ls, False, seed, k * q)

        def pair(k):
            v, z = bufs[k % sets]
            ops.sampler_step(v, z, lt, ls, False, noise=ops.rng_normal(shape, seed, k * q, "cuda"))
        arms = {"gmk_consistency_step": fused, "gmk_rng_normal + gmk_sampler_step": pair}
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
            say(f"{cin}x{size}x{size} B={B} {name}: median {med[name] * 1e3:.1f} us per step  (rounds: {', '.join(f'{x * 1e3:.1f}' for x in v)})")
        a, b = med["gmk_consistency_step"], med["gmk_rng_normal + gmk_sampler_step"]
        say(f"{cin}x{size}x{size} B={B}: {sets} buffer sets, {nbytes / 1e6:.1f} MB per fused launch = {nbytes / a / 1e9:.2f} TB/s;  fused / pair = {a / b:.3f}")
        del bufs, arms


def train(rounds, steps):
    Model = common.discover_models()["diffusion"]
    arms = (("step2", dict(teacher_mode="step2")), ("consistency l2", dict(teacher_mode="consistency")),
            ("consistency huber", dict(teacher_mode="consistency", consistency_loss="huber")))
    for cin, size, B in SHAPES:
        base = dict(lr=3e-4, pad32=0, device="cuda", bs=B, in_channels=cin, image_size=size, timesteps=8)
        with tempfile.TemporaryDirectory() as tmp:
            path = os.path.join(tmp, "model.pt")
            G = common.AttrDict(dict(Model.DG))
            G.update(base)
            torch.manual_seed(0)
            torch.save(Model(G).state_dict(), path)
            models = {}
            for arm, flags in arms:
                G = common.AttrDict(dict(Model.DG))
                G.update(base, teacher_path=path, **flags)
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
            for arm in (models if r % 2 == 0 else reversed(list(models))):
                times[arm].append(run(models[arm]))
        med = {arm: statistics.median(v) for arm, v in times.items()}
        for arm, v in times.items():
            say(f"{cin}x{size}x{size} B={B} train_step, {arm}: median {med[arm]:.3f} ms  (rounds: {', '.join(f'{t:.3f}' for t in v)})")
        say(f"{cin}x{size}x{size} B={B}: consistency l2 / step2 = {med['consistency l2'] / med['step2']:.4f}, consistency huber / step2 = "
            f"{med['consistency huber'] / med['step2']:.4f}  (step2 rounds span {spread(times['step2'])} ms)")
        del models


def main():
    args = sys.argv[1:]
    mode = args[0] if args else "all"
    out = args[1] if len(args) > 1 else "profiles/consistency_cost.txt"
    assert mode in ("kernel", "train", "all"), mode
    assert torch.cuda.is_available(), "consistency_cost.py measures on the GPU"
    num = lambda i, d: int(args[i]) if mode != "all" and len(args) > i else d
    say(f"tools/consistency_cost.py {mode} on {torch.cuda.get_device_name(0)}")
    if mode in ("kernel", "all"):
        kernel(num(2, 7), num(3, 200))
    if mode in ("train", "all"):
        train(num(2, 5), num(3, 4))
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
