"""Cost of DDNM restoration (`GaussianDiffusion.restore`: gmk_box_residual, then gmk_sampler_step_ns) at 3x32x32, B = 2048.

    python tools/restore_cost.py kernel [rounds=7] [launches=50]   per operator, guided and not: time of the two launches of one network
                                                                   evaluation (residual + projected DDIM update) against the plain update
                                                                   (gmk_sampler_step) and against a device copy of the bytes the two move
    python tools/restore_cost.py chain [T=20] [rounds=3]           restore() against sample() on the default 16-bit net, DDIM, interleaved
                                                                   rounds in one process, medians and the rounds themselves (their spread
                                                                   is the yardstick: a difference inside it is not one)

Bytes of the two launches: the residual reads v, z (and v_uncond) and writes n / k floats per image; the update reads v, z (and v_uncond) and the
n / k residuals and writes z_next (and its copy for the guided 2B batch).  A probe, not a gate."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import GaussianDiffusion  # noqa: E402
from generative_models_amd.diffusion.simple_unet import SimpleUnet  # noqa: E402

B, SHAPE = 2048, (3, 32, 32)
OPERATORS = (("sr2", 1, 2), ("sr4", 1, 4), ("gray", 3, 1), ("gray+sr2", 3, 2))      # (name, cf, N)


def kernel_ms(launch, rounds, k):
    times = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(k):
            launch()
        e.record()
        torch.cuda.synchronize()
        times.append(s.elapsed_time(e) / k)
    return statistics.median(times)


def kernels(rounds, k):
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda: torch.randn((B,) + SHAPE, device="cuda", generator=g)
    v, vu, z = rnd(), rnd(), rnd()
    w = torch.full((B,), 0.5, device="cuda")
    lt, ls = -1.0, 0.5
    print(f"B = {B}, n = {n}, {k} launches per round, median of {rounds} rounds, HIP events")
    for name, cf, N in OPERATORS:
        obs = ops.box_mean(torch.rand((B,) + SHAPE, device="cuda", generator=g) * 2 - 1, cf, N)
        for guided in (False, True):
            kw = dict(v_uncond=vu, cond_w=w) if guided else {}
            r = ops.box_residual(v, z, obs, lt, cf, N, **kw)
            res = lambda: ops.box_residual(v, z, obs, lt, cf, N, **kw)
            ns = lambda: ops.sampler_step(v, z, lt, ls, False, dup=guided, ns=(r, cf, N), **kw)
            plain = lambda: ops.sampler_step(v, z, lt, ls, False, dup=guided, **kw)
            reads = (3 if guided else 2) * B * n
            nbytes = 4 * (reads + 2 * obs.numel() + reads + obs.numel() + (2 if guided else 1) * B * n)
            src = torch.empty((nbytes // 8,), device="cuda")
            dst = torch.empty_like(src)
            copy = lambda: dst.copy_(src)
            both = lambda: (res(), ns())
            for fn in (res, ns, plain, copy):
                kernel_ms(fn, 2, k)
            t_res, t_ns, t_plain, t_both, t_copy = (kernel_ms(fn, rounds, k) for fn in (res, ns, plain, both, copy))
            print(f"  {name:9s} {'guided  ' if guided else 'unguided'}  residual {t_res * 1e3:6.1f} us  update_ns {t_ns * 1e3:6.1f} us  (plain update "
                  f"{t_plain * 1e3:6.1f} us)  both {t_both * 1e3:6.1f} us for {nbytes / 1e6:6.1f} MB = {nbytes / t_both / 1e9:5.2f} TB/s   copy of the same "
                  f"bytes {t_copy * 1e3:6.1f} us   both / copy {t_both / t_copy:.2f}x", flush=True)


def chain(T, rounds):
    torch.manual_seed(0)
    net = SimpleUnet(128, 0.0, in_channels=SHAPE[0]).cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(1)
    init = torch.randn((B,) + SHAPE, device="cuda", generator=g)
    y = torch.randint(0, 10, (B,), device="cuda", generator=g)
    x0 = torch.rand((B,) + SHAPE, device="cuda", generator=g) * 2 - 1
    d = GaussianDiffusion(mean_type="v", num_steps=T)
    runs = {"sample": lambda: d.sample(net=partial(net, guide=y), init_x=init, record=False)}
    for name, cf, N in OPERATORS:
        obs = ops.box_mean(x0, cf, N)
        runs[f"restore {name}"] = partial(d.restore, net=partial(net, guide=y), obs=obs, factor=N, gray=cf > 1, init_x=init)
    times = {k: [] for k in runs}
    for rnd in range(rounds + 1):                       # round 0 warms up
        for name, fn in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
    print(f"3x32x32, B = {B}, 16-bit mode, DDIM, T = {T}, {rounds} interleaved rounds, medians")
    base = statistics.median(times["sample"])
    for name, ts in times.items():
        m = statistics.median(ts)
        print(f"  {name:17s} {m:9.3f} ms   {m / T:7.3f} ms per step   {m / base:.4f} x sample   rounds: {', '.join(f'{t:.3f}' for t in ts)}", flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "kernel"
    a = [int(s) for s in sys.argv[2:]]
    if what == "kernel":
        kernels(*(a + [7, 50][len(a):]))
    else:
        chain(*(a + [20, 3][len(a):]))
