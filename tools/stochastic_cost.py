"""Cost of the stochastic samplers' update kernel (gmk_stochastic_step) and of the samplers on it.

    python tools/stochastic_cost.py kernel [out] [rounds=7] [iters=200]    per shape: time per launch of gmk_stochastic_step with coef_prev = 0 (v and
                                                                           z read, z_next written, the noise drawn in the kernel: 12 B per value)
                                                                           and with coef_prev != 0 (x_hist read and rewritten as well: 20 B), against
                                                                           the pair 'noisy' launches, gmk_rng_normal + gmk_sampler_step(noise=...)
                                                                           (the noise written and read back: 20 B), and gmk_dpm_solver_step
                                                                           (second order, no noise: 20 B).  HIP events around `iters` launches that
                                                                           rotate over enough buffer sets to exceed the 256 MiB Infinity Cache;
                                                                           `rounds` rounds, the arms interleaved, the order alternating; medians
    python tools/stochastic_cost.py sampler [out] [rounds=6] [steps=20]    per shape: steps/s of sample() (`steps` steps per call, unguided), same
                                                                           process, interleaved, the order alternating: 'noisy' against 'ancestral',
                                                                           'ddim' against 'ddim' at ddim_eta = 0.5, 'dpmpp_2m' against 'sde_dpmpp_2m'
    python tools/stochastic_cost.py all [out]                              both
Shapes: the bench's three, 1x28x28 B = 1024, 3x32x32 B = 2048, 3x64x64 B = 1024.  Everything printed is also written to `out` (default
profiles/stochastic_cost.txt).  The baselines are existing, unchanged paths.  Reports, not assertions; nothing here measures sample quality."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import stochastic_row  # noqa: E402

SHAPES = [(1, 28, 1024), (3, 32, 2048), (3, 64, 1024)]
PAIRS = (("noisy", dict(sampler="noisy"), "ancestral", dict(sampler="ancestral")),
         ("ddim", dict(sampler="ddim"), "ddim eta 0.5", dict(sampler="ddim", ddim_eta=0.5)),
         ("dpmpp_2m", dict(sampler="dpmpp_2m"), "sde_dpmpp_2m", dict(sampler="sde_dpmpp_2m")))
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
    lt, ls, seed = -1.0, 0.5, 7
    sde = stochastic_row("sde_dpmpp_2m", lt, ls)
    anc = stochastic_row("ancestral", lt, ls, 1.0)
    for cin, size, B in SHAPES:
        n = cin * size * size
        shape = (B, cin, size, size)
        nbytes = 3 * B * n * 4
        sets = max(2, min(64, -(-(640 << 20) // nbytes)))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn(shape, device="cuda", generator=g) for _ in range(3)] for _ in range(sets)]      # v, z, x_hist
        q = B * n // 4

        def first(k):
            v, z, _ = bufs[k % sets]
            ops.stochastic_step(v, z, lt, ls, *anc, 0.0, False, seed, k * q)

        def second(k):
            v, z, h = bufs[k % sets]
            ops.stochastic_step(v, z, lt, ls, *sde, 0.4, False, seed, k * q, x_hist=h)

        def pair(k):
            v, z, _ = bufs[k % sets]
            ops.sampler_step(v, z, lt, ls, False, noise=ops.rng_normal(shape, seed, k * q, "cuda"))

        def dpm(k):
            v, z, h = bufs[k % sets]
            ops.dpm_solver_step(v, z, h, lt, ls, sde[0], sde[1], 0.4, False)
        arms = {"gmk_stochastic_step k = 0": first, "gmk_stochastic_step k != 0": second, "gmk_rng_normal + gmk_sampler_step": pair,
                "gmk_dpm_solver_step": dpm}
        for fn in arms.values():                    # warm-up over every buffer set
            for k in range(sets):
                fn(k)
        torch.cuda.synchronize()
        times = {name: [] for name in arms}
        for r in range(rounds):
            for name in (list(arms) if r % 2 == 0 else reversed(list(arms))):
                times[name].append(event_ms(arms[name], iters))
        med = {name: statistics.median(v) for name, v in times.items()}
        for name, v in times.items():
            say(f"{cin}x{size}x{size} B={B} {name}: median {med[name] * 1e3:.1f} us per step  (rounds: {', '.join(f'{x * 1e3:.1f}' for x in v)}; "
                f"spread {(max(v) - min(v)) / med[name]:.1%})")
        a, b, c, d = (med[name] for name in arms)
        say(f"{cin}x{size}x{size} B={B}: {sets} buffer sets, {nbytes / 1e6:.1f} MB per k = 0 launch = {nbytes / a / 1e9:.2f} TB/s, "
            f"{5 * nbytes / 3e6:.1f} MB per k != 0 launch = {5 * nbytes / 3 / b / 1e9:.2f} TB/s;  k = 0 / pair = {a / c:.3f}, "
            f"k != 0 / dpm_solver_step = {b / d:.3f}")
        del bufs, arms


def sampler(rounds, steps):
    Model = common.discover_models()["diffusion"]
    for cin, size, B in SHAPES:
        models = {}
        for base, flags0, new, flags1 in PAIRS:
            for arm, flags in ((base, flags0), (new, flags1)):
                G = common.AttrDict(dict(Model.DG))
                G.update(lr=3e-4, pad32=0, device="cuda", timesteps=steps, bs=B, in_channels=cin, image_size=size, **flags)
                torch.manual_seed(0)
                models[arm] = Model(G).cuda().eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        init = torch.randn((B, cin, size, size), device="cuda", generator=g)
        y = torch.randint(0, 10, (B,), device="cuda", generator=g)

        def run(arm):
            m = models[arm]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                m.diffusion.sample(net=partial(m.net, guide=y), init_x=init, record=False)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)
        for arm in models:
            run(arm)
        rates = {arm: [] for arm in models}
        for r in range(rounds):
            for arm in (list(models) if r % 2 == 0 else reversed(list(models))):
                rates[arm].append(run(arm))
        med = {arm: statistics.median(v) for arm, v in rates.items()}
        head = f"{cin}x{size}x{size} B={B}, {steps} steps"
        for arm, v in rates.items():
            say(f"{head}, {arm}: median {med[arm]:.2f} steps/s  (rounds: {', '.join(f'{x:.2f}' for x in v)}; spread {(max(v) - min(v)) / med[arm]:.2%})")
        say(f"{head}: " + ", ".join(f"{new} / {base} = {med[new] / med[base]:.4f} ({1e3 / med[new] - 1e3 / med[base]:+.3f} ms per step)"
                                    for base, _, new, _ in PAIRS))
        del models


def main():
    args = sys.argv[1:]
    mode = args[0] if args else "all"
    out = args[1] if len(args) > 1 else "profiles/stochastic_cost.txt"
    assert mode in ("kernel", "sampler", "all"), mode
    assert torch.cuda.is_available(), "stochastic_cost.py measures on the GPU"
    num = lambda i, d: int(args[i]) if mode != "all" and len(args) > i else d
    say(f"tools/stochastic_cost.py {mode} on {torch.cuda.get_device_name(0)}")
    if mode in ("kernel", "all"):
        kernel(num(2, 7), num(3, 200))
    if mode in ("sampler", "all"):
        sampler(num(2, 6), num(3, 20))
    say("No sample-quality number was measured.")
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
