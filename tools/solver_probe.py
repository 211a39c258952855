"""sampler='dpmpp_2m' (DPM-Solver++(2M)) against 'ddim': what a step costs and what a sample's accuracy costs in steps.

    python tools/solver_probe.py [rounds=3] [T=100]

1. Per-step time at BASELINE configs[2] (3x32x32, B = 2048, C = 128, bf16, bench.py's seeded weights, record=False), the two samplers
   interleaved `rounds` times in one process; and the update kernel alone (gmk_sampler_step vs gmk_dpm_solver_step) at that size, HIP events.
2. Final-sample error (relative L2) against a 1000-step DDIM chain of the same weights, for both samplers at N in {10, 20, 40, 80, 250}
   evaluations (fp32 mode and bf16 mode; B = 16 images of configs[2]'s shape, the graph-replayed small-batch path), and the fewest
   DPM++(2M) steps that reach DDIM-250's error, with the images/s that gives at configs[2]."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from generative_models_amd import common, ops  # noqa: E402

CIN, S, B, _, _ = bench.CONFIGS["cfg2"]


def model(dtype):
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=1000, bs=B, compute_dtype=dtype, in_channels=CIN, seed=0, attention=0)
    torch.manual_seed(G.seed)                  # bench.py's seeded weights
    m = Model(G).cuda().eval()
    m.size = S
    return m


def chain(m, kind, T, init, y, record=False):
    d = m.diffusion
    d.sampler, d.num_steps = kind, T
    return d.sample(net=partial(m.net, guide=y), init_x=init, record=record)[0][-1]


def step_times(rounds, T):
    m = model("bf16")
    g = torch.Generator().manual_seed(1)
    init = torch.randn((B, CIN, S, S), generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    for kind in ("ddim", "dpmpp_2m"):
        chain(m, kind, 2, init, y)
    times = {"ddim": [], "dpmpp_2m": []}
    for r in range(rounds):
        for kind in (("ddim", "dpmpp_2m") if r % 2 == 0 else ("dpmpp_2m", "ddim")):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            chain(m, kind, T, init, y)
            torch.cuda.synchronize()
            times[kind].append((time.perf_counter() - t0) / T * 1e3)
    print(f"1. per-step time, configs[2] (3x32x32, B = {B}, bf16, unguided, record=False), T = {T}, {rounds} interleaved rounds")
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        print(f"   {k:9s} median {med[k]:.3f} ms/step   rounds: {', '.join(f'{t:.3f}' for t in v)}")
    print(f"   dpmpp_2m / ddim: {med['dpmpp_2m'] / med['ddim'] - 1:+.2%}")
    # the update kernels alone at this size
    n = CIN * S * S
    v, z, hist = (torch.randn((B, CIN, S, S), device="cuda") for _ in range(3))
    runs = {"sampler_step (ddim)": lambda: ops.sampler_step(v, z, -1.0, -0.5, False),
            "dpm_solver_step": lambda: ops.dpm_solver_step(v, z, hist, -1.0, -0.5, 0.9, 0.1, 0.4, False)}
    for name, fn in runs.items():
        for _ in range(10):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            fn()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) / 200 * 1e3
        nbytes = (12 if name.startswith("sampler") else 20) * B * n
        print(f"   {name:20s} {us:7.1f} us per launch ({nbytes / 1e6:.0f} MB algorithmic: {nbytes / us / 1e6:.2f} TB/s)")
    return med


def errors(dtype, Ns, scan):
    m = model(dtype)
    g = torch.Generator().manual_seed(2)
    init = torch.randn((16, CIN, S, S), generator=g).cuda()
    y = torch.randint(0, 10, (16,), generator=g).cuda()
    ref = chain(m, "ddim", 1000, init, y).double()
    err = lambda kind, T: float((chain(m, kind, T, init, y).double() - ref).norm() / ref.norm())
    table = {(k, N): err(k, N) for k in ("ddim", "dpmpp_2m") for N in Ns}
    print(f"2. relative L2 error of the final sample against DDIM-1000, {dtype} mode (16 images, 3x32x32, unguided)")
    print("   N     " + "  ".join(f"{N:>9d}" for N in Ns))
    for k in ("ddim", "dpmpp_2m"):
        print(f"   {k:9s}" + "  ".join(f"{table[(k, N)]:9.2e}" for N in Ns))
    target = table[("ddim", 250)]
    match = next((N for N in scan if err("dpmpp_2m", N) <= target), None)
    print(f"   DDIM-250 error {target:.2e}: DPM++(2M) matches it from N = {match} (scanned {scan[0]} ... {scan[-1]})")
    return match


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    T = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    med = step_times(rounds, T)
    Ns = [10, 20, 40, 80, 250]
    scan = [8, 10, 12, 14, 16, 18, 20, 24, 28, 32, 40, 50, 60, 80, 100, 125, 160, 200, 250]
    for dtype in ("fp32", "bf16"):
        N = errors(dtype, Ns, scan)
        if N is not None:
            ips_ddim = B / (250 * med["ddim"] * 1e-3)
            ips_dpm = B / (N * med["dpmpp_2m"] * 1e-3)
            print(f"   at configs[2]: DDIM-250 {ips_ddim:.1f} images/s, DPM++(2M)-{N} {ips_dpm:.1f} images/s ({ips_dpm / ips_ddim:.1f}x)")


if __name__ == "__main__":
    main()
