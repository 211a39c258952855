"""The probability-flow ODE (`GaussianDiffusion.encode / decode / ode_nll`, DG.ode_nlogp_steps): what one likelihood evaluation costs, what
its kernels cost, how the likelihood converges with the number of ODE steps N, and how closely decode inverts encode.

    python tools/ode_probe.py [rounds=3]        (a) - (d) below
    python tools/ode_probe.py kernels           the kernels alone (the workload of a `rocprofv3 --kernel-trace --stats` run)
    python tools/ode_probe.py stats <csv>       our kernels' rows of that run's kernel_stats.csv

(a) GPU time at BASELINE configs[2] (3x32x32, B = 2048, C = 128, 16-bit mode, bench.py's seeded weights) and at the reference's 1x28x28
    (B = 256): `ode_nll` with N = 1 and N = 5 (2 and 6 evaluations), one unguided DDIM sampler chain (T = 20, record=False) and 10 train steps,
    interleaved in one process.  One likelihood evaluation (forward + input VJP + gmk_pf_ode_step + probe) = (t[N=5] - t[N=1]) / 4, set
    against the sampler's time per step and a train step.
(b) gmk_pf_ode_step (the likelihood form: out, z, r, g read, z written) and gmk_stem_dgrad (16-bit dy) alone at both shapes (HIP events,
    200 launches each), algorithmic bytes per launch and the fraction of the 8 TB/s HBM peak.
(c) batch-mean ode_nlogp of 256 synthetic test images (1x28x28, [-1, 1] data, unconditional) for N in {32, 64, 128, 256, 512} and three
    seeds, on the default net trained 300 steps at bs = 64, next to the ELBO (nlogp, K = 16) of the same images.
(d) decode(encode(x)) against x on the same net and images, against N: the mean over images of |decode(encode(x)) - x|_2 / sqrt(D)."""
import csv
import math
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
import bench  # noqa: E402
from generative_models_amd import common, ops  # noqa: E402
from generative_models_amd.data import SyntheticMNIST  # noqa: E402

HBM_PEAK = 8.0e12
KERNELS = ("pf_ode_step_kernel", "stem_dgrad_mfma_kernel", "stem_dgrad_kernel")
CIN2, S2, B2, _, _ = bench.CONFIGS["cfg2"]
SHAPES = {"configs[2]": (CIN2, S2, B2), "1x28x28": (1, 28, 256)}


def model(cin, **flags):
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=1000, bs=64, compute_dtype="bf16", in_channels=cin, seed=0, attention=0)
    G.update(flags)
    torch.manual_seed(G.seed)                  # bench.py's seeded weights
    return Model(G).cuda().eval()


def eval_times(rounds):
    for label, (cin, S, B) in SHAPES.items():
        m = model(cin)
        m.size = S
        g = torch.Generator().manual_seed(1)
        x = (torch.rand((B, cin, S, S), generator=g) * 2 - 1).cuda()
        init = torch.randn((B, cin, S, S), generator=g).cuda()
        y = torch.randint(0, 10, (B,), generator=g).cuda()
        T, STEPS = 20, 10
        d = m.diffusion
        d.sampler, d.num_steps = "ddim", T

        def train():
            m.train()
            for _ in range(STEPS):
                m.train_step(x, y.clone())
            m.eval()
        runs = {"ode_nll N=1": lambda: m.ode_nlogp(x, steps=1), "ode_nll N=5": lambda: m.ode_nlogp(x, steps=5),
                "ddim chain": lambda: d.sample(net=partial(m.net, guide=y), init_x=init, record=False), "10 train steps": train}
        for fn in runs.values():
            fn()
        times = {k: [] for k in runs}
        for r in range(rounds):
            for k in (list(runs) if r % 2 == 0 else list(runs)[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                runs[k]()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
        med = {k: statistics.median(v) for k, v in times.items()}
        step = med["ddim chain"] / T
        tstep = med["10 train steps"] / STEPS
        ev = (med["ode_nll N=5"] - med["ode_nll N=1"]) / 4
        print(f"(a) {label} ({cin}x{S}x{S}, B = {B}, 16-bit mode), {rounds} interleaved rounds, medians")
        for k, v in times.items():
            print(f"    {k:15s} {med[k]:9.3f} ms   rounds: {', '.join(f'{t:.3f}' for t in v)}")
        print(f"    DDIM sampler step (unguided, T = {T}): {step:.3f} ms;  train step: {tstep:.3f} ms")
        print(f"    likelihood evaluation, marginal (t[N=5] - t[N=1]) / 4: {ev:.3f} ms = {ev / step:.3f} x the sampler step = "
              f"{ev / tstep:.3f} x the train step")


def kernel_runs(label):
    cin, S, B = SHAPES[label]
    n = cin * S * S
    g = torch.Generator(device="cuda").manual_seed(2)
    out, z, gv = (torch.randn((B, cin, S, S), device="cuda", generator=g) for _ in range(3))
    r = ops.rng_rademacher((B, cin, S, S), 3, 0, "cuda")
    acc = torch.zeros((B,), device="cuda")
    dy = torch.randn((B, S, S, 128), device="cuda", generator=g).bfloat16()
    w = torch.randn((128, cin, 3, 3), device="cuda", generator=g) * 0.1
    return {"pf_ode_step_kernel": (lambda: ops.pf_ode_step(out, z, 1.0, 0.9, r=r, g=gv, acc=acc, div_a=0.1, div_b=-0.01), 20 * B * n + 8 * B),
            "gmk_stem_dgrad": (lambda: ops.stem_dgrad(dy, w), 2 * 128 * B * S * S + 4 * B * n)}


def kernel_times(reps=200):
    for label in SHAPES:
        cin, S, B = SHAPES[label]
        print(f"(b) the kernels alone at {label} (B = {B}, {cin}x{S}x{S}), {reps} launches each, HIP events")
        for name, (fn, nbytes) in kernel_runs(label).items():
            for _ in range(10):
                fn()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / reps * 1e3
            bw = nbytes / (us * 1e-6)
            print(f"    {name:20s} {us:7.1f} us per launch  {nbytes / 1e6:6.1f} MB algorithmic  {bw / 1e12:5.2f} TB/s = "
                  f"{bw / HBM_PEAK:.2f} of peak")


def convergence(steps=300, bs=64, seeds=3, n_test=256):
    m = model(1, bs=bs, timesteps=250)
    m.train()
    data = SyntheticMNIST(bs, steps, False, False, "cuda", seed=1000)
    t0 = time.perf_counter()
    for x, y in data:
        m.train_step(x, y)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    m.eval()
    x, _ = next(iter(SyntheticMNIST(n_test, 1, False, False, "cuda", seed=2000)))
    elbo = float(m.nlogp(x, num_samples=16)["nlogp"].double().mean())
    print(f"(c) batch-mean ode_nlogp of {n_test} synthetic test images (1x28x28, [-1, 1] data, unconditional) after {steps} steps at bs = {bs} "
          f"({train_s:.1f} s); {seeds} seeds per N.  ELBO (nlogp, K = 16) of the same images: {elbo:.4f} nats/dim")
    print("    N      mean over seeds   per seed                           prior     divergence   s")
    res = {}
    for N in (32, 64, 128, 256, 512):
        vals = []
        t0 = time.perf_counter()
        for seed in range(seeds):
            r = m.ode_nlogp(x, steps=N, seed=seed)
            vals.append(float(r["nlogp"].double().mean()))
            if seed == 0:
                pr, dv = float(r["prior"].double().mean()), float(r["divergence"].double().mean())
        torch.cuda.synchronize()
        res[N] = statistics.mean(vals)
        print(f"    {N:3d}    {res[N]:9.4f}      {', '.join(f'{v:.4f}' for v in vals):32s}  {pr:8.4f}  {dv:9.4f}  "
              f"{(time.perf_counter() - t0) / seeds:6.2f}")
    ok = [N for N in res if abs(res[N] - res[512]) <= 0.02]
    print(f"    smallest N within 0.02 nats/dim of N = 512: {min(ok)}")
    print("(d) decode(encode(x)) on the same net and images: mean over images of |decode(encode(x)) - x|_2 / sqrt(D)")
    D = x[0].numel()
    for N in (8, 32, 64, 128, 256, 512):
        back = m.decode(m.encode(x, steps=N), steps=N)
        err = float(((back - x).double().flatten(1).norm(dim=1) / math.sqrt(D)).mean())
        print(f"    N = {N:3d}   {err:.5f}")


def stats(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    print(f"rocprofv3 --kernel-trace --stats ({path.rsplit('/', 1)[-1]}), `python tools/ode_probe.py kernels`:")
    for row in rows:
        if any(k in row["Name"] for k in KERNELS):         # demangled or not
            print(f"    {row['Name'][:60]:60s} calls {row['Calls']:>5s}  average {float(row['AverageNs']) / 1e3:7.1f} us  "
                  f"min {float(row['MinNs']) / 1e3:7.1f} us  max {float(row['MaxNs']) / 1e3:7.1f} us")
    trace = path.replace("kernel_stats", "kernel_trace")
    with open(trace) as f:                   # the same dispatches split by shape: `kernels` launches each kernel 50 times per shape, in SHAPES order
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    print(f"  per shape ({trace.rsplit('/', 1)[-1]}, dispatch order), average over 50 dispatches:")
    for k in KERNELS:
        durs = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if k in r["Kernel_Name"]]
        if len(durs) == 50 * len(SHAPES):
            print("    " + f"{k:24s}" + "   ".join(f"{label} {statistics.mean(durs[50 * i:50 * (i + 1)]):7.1f} us"
                                                   for i, label in enumerate(SHAPES)))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "kernels":
        for label in SHAPES:                  # configs[2] first, then 1x28x28: 50 launches of each kernel per shape
            for fn, _ in kernel_runs(label).values():
                for _ in range(50):
                    fn()
        torch.cuda.synchronize()
        return
    if len(sys.argv) > 2 and sys.argv[1] == "stats":
        stats(sys.argv[2])
        return
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    eval_times(rounds)
    kernel_times()
    convergence()


if __name__ == "__main__":
    main()
