"""Cost of diffusion posterior sampling (`GaussianDiffusion.posterior_sample`: gmk_dps_backproject, the input VJP, gmk_dps_correct) at the three
bench shapes (1x28x28 B = 1024, 3x32x32 B = 2048, 3x64x64 B = 1024).

    python tools/dps_cost.py kernel [rounds=7] [launches=50]   per shape: the time of one gmk_dps_backproject launch (box:2 and blur:1.5) and of
                                                               one gmk_dps_correct launch, each against a device copy of the bytes it moves
                                                               (backproject: v, z, obs in, u out; correct: z, u, g in, z out); interleaved
                                                               rounds in one process, median and [min, max] of the rounds
    python tools/dps_cost.py chain [T=8] [rounds=3]            per shape, on the default 16-bit net: posterior_sample (DDIM, box:2) in steps/s
                                                               against two arms of the same build - sample() with the same sampler, and an
                                                               ode_nll evaluation (forward + input VJP + one launch per step, the closest
                                                               existing workload; T - 1 ODE steps = T evaluations) - interleaved rounds,
                                                               medians and the rounds themselves (their spread is the yardstick: a difference
                                                               inside it is not one)

A probe, not a gate."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion, measurement_op  # noqa: E402
from generative_models_amd.diffusion.simple_unet import SimpleUnet  # noqa: E402

SHAPES = (((1, 28, 28), 1024), ((3, 32, 32), 2048), ((3, 64, 64), 1024))
KINDS = ("box:2", "blur:1.5")


def round_ms(launch, k):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(k):
        launch()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / k


def kernels(rounds, k):
    print(f"{k} launches per round, {rounds} interleaved rounds, HIP events: median [min, max] us")
    for shape, B in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(0)
        rnd = lambda: torch.randn((B,) + shape, device="cuda", generator=g)
        v, z, gv = rnd(), rnd(), rnd()
        arms = {}
        for kind in KINDS:
            op, low = measurement_op(kind, (B,) + shape)
            obs = ops.measure(torch.rand((B,) + shape, device="cuda", generator=g) * 2 - 1, op)
            nbytes = 4 * (3 * v.numel() + obs.numel())
            src = torch.empty((nbytes // 8,), device="cuda")
            arms[f"backproject {kind}"] = (partial(ops.dps_backproject, v, z, obs, -1.0, op), partial(torch.empty_like(src).copy_, src), nbytes)
        u, en2 = ops.dps_backproject(v, z, obs, -1.0, op)
        zc = z.clone()
        nbytes = 4 * 4 * z.numel()
        src = torch.empty((nbytes // 8,), device="cuda")
        arms["correct"] = (partial(ops.dps_correct, zc, u, gv, en2, 0.6, -0.8, 1e-3), partial(torch.empty_like(src).copy_, src), nbytes)
        times = {name: ([], []) for name in arms}
        for r in range(rounds + 1):                     # round 0 warms up
            for name, (fn, copy, _) in arms.items():
                a, b = round_ms(fn, k), round_ms(copy, k)
                if r:
                    times[name][0].append(a); times[name][1].append(b)
        print(f"  {shape[0]}x{shape[1]}x{shape[2]}, B = {B}")
        for name, (ta, tb) in times.items():
            ma, mb = statistics.median(ta), statistics.median(tb)
            print(f"    {name:22s} {ma * 1e3:7.1f} [{min(ta) * 1e3:.1f}, {max(ta) * 1e3:.1f}] us for {arms[name][2] / 1e6:6.1f} MB = "
                  f"{arms[name][2] / ma / 1e9:5.2f} TB/s   copy of the same bytes {mb * 1e3:7.1f} [{min(tb) * 1e3:.1f}, {max(tb) * 1e3:.1f}] us   "
                  f"kernel / copy {ma / mb:.2f}x", flush=True)


def chain(T, rounds):
    for shape, B in SHAPES:
        torch.manual_seed(0)
        net = SimpleUnet(128, 0.0, in_channels=shape[0]).cuda().eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        init = torch.randn((B,) + shape, device="cuda", generator=g)
        y = torch.randint(0, 10, (B,), device="cuda", generator=g)
        x0 = torch.rand((B,) + shape, device="cuda", generator=g) * 2 - 1
        op, _ = measurement_op("box:2", (B,) + shape)
        obs = ops.measure(x0, op) + 0.05 * torch.randn(ops.measure(x0, op).shape, device="cuda", generator=g)
        d = GaussianDiffusion(mean_type="v", num_steps=T)
        gnet = partial(net, guide=y)
        runs = {"sample": lambda: d.sample(net=gnet, init_x=init, record=False),
                "ode_nll": lambda: d.ode_nll(net=gnet, x=x0, num_steps=T - 1),
                "posterior_sample": lambda: d.posterior_sample(net=gnet, obs=obs, op=op, init_x=init, zeta=1.0)}
        times = {k: [] for k in runs}
        for rnd in range(rounds + 1):                   # round 0 warms up
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) * 1e3)
        print(f"  {shape[0]}x{shape[1]}x{shape[2]}, B = {B}, 16-bit mode, DDIM, T = {T} network evaluations, {rounds} interleaved rounds, medians")
        base = statistics.median(times["ode_nll"])
        for name, ts in times.items():
            m = statistics.median(ts)
            print(f"    {name:17s} {m:9.2f} ms   {T / m * 1e3:7.2f} steps/s   {m / base:.4f} x ode_nll   spread {(max(ts) - min(ts)) / m * 100:.2f} %   "
                  f"rounds: {', '.join(f'{t:.2f}' for t in ts)}", flush=True)
        del net
        torch.cuda.empty_cache()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    a = [int(s) for s in sys.argv[2:]]
    if what == "kernel":
        kernels(*(a + [7, 50][len(a):]))
    else:
        chain(*(a + [8, 3][len(a):]))
