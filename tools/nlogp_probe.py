"""The variational bound (`GaussianDiffusion.nll`, DG.nlogp_samples): what one draw costs, what its kernels cost, and how its Monte-Carlo
error falls with the number of draws K.

    python tools/nlogp_probe.py [rounds=3]        (a) - (c) below
    python tools/nlogp_probe.py kernels           the three kernels alone (the workload of a `rocprofv3 --kernel-trace --stats` run)
    python tools/nlogp_probe.py stats <csv>       our kernels' rows of that run's kernel_stats.csv

(a) GPU time per ELBO draw at BASELINE configs[2] (3x32x32, B = 2048, C = 128, 16-bit mode, bench.py's seeded weights): `nll` with K = 1
    and K = 8 interleaved with one unguided DDIM sampler chain (record=False) in one process; the marginal cost of a draw (t8 - t1) / 7
    against the sampler's time per step.
(b) gmk_q_sample_logsnr, gmk_vlb_term and gmk_vlb_endpoints alone at that size (HIP events, 200 launches each), algorithmic bytes per launch
    and the fraction of the 8 TB/s HBM peak.
(c) The standard error of the batch-mean nlogp (256 test images) for K in {1, 4, 16}, on the default net (1x28x28, C = 128, 16-bit mode)
    trained 300 steps at bs = 64 on the synthetic data: the one `nll` reports (sqrt(sum se_b^2) / B; none for K = 1) and the spread of
    the batch mean over 8 seeds (its standard deviation: the Monte-Carlo error the stratified draws actually have)."""
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

CIN, S, B, _, _ = bench.CONFIGS["cfg2"]
HBM_PEAK = 8.0e12
KERNELS = ("q_sample_logsnr_kernel", "vlb_term_kernel", "vlb_endpoints_kernel")


def model(**flags):
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=1000, bs=B, compute_dtype="bf16", in_channels=CIN, seed=0, attention=0)
    G.update(flags)
    torch.manual_seed(G.seed)                  # bench.py's seeded weights
    return Model(G).cuda().eval()


def draw_times(rounds):
    m = model()
    m.size = S
    g = torch.Generator().manual_seed(1)
    x = (torch.rand((B, CIN, S, S), generator=g) * 2 - 1).cuda()
    init = torch.randn((B, CIN, S, S), generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    T = 20
    d = m.diffusion
    d.sampler, d.num_steps = "ddim", T
    runs = {"nll K=1": lambda: m.nlogp(x, num_samples=1), "nll K=8": lambda: m.nlogp(x, num_samples=8),
            "ddim chain": lambda: d.sample(net=partial(m.net, guide=y), init_x=init, record=False)}
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
    draw = (med["nll K=8"] - med["nll K=1"]) / 7
    print(f"(a) configs[2] (3x32x32, B = {B}, 16-bit mode), {rounds} interleaved rounds, medians")
    for k, v in times.items():
        print(f"    {k:10s} {med[k]:9.3f} ms   rounds: {', '.join(f'{t:.3f}' for t in v)}")
    print(f"    DDIM sampler step (unguided, T = {T}): {step:.3f} ms")
    print(f"    ELBO draw, marginal (t[K=8] - t[K=1]) / 7: {draw:.3f} ms = {draw / step:.3f} x the sampler step")
    print(f"    nll K=8 per draw, everything included: {med['nll K=8'] / 8:.3f} ms = {med['nll K=8'] / 8 / step:.3f} x the sampler step")


def kernel_runs():
    n = CIN * S * S
    g = torch.Generator(device="cuda").manual_seed(2)
    x = torch.rand((B, CIN, S, S), device="cuda", generator=g) * 2 - 1
    eps, out = (torch.randn((B, CIN, S, S), device="cuda", generator=g) for _ in range(2))
    logsnr = torch.rand((B,), device="cuda", generator=g) * 40 - 20
    z = ops.q_sample_logsnr(x, eps, logsnr)
    weight, acc = torch.full((B,), 20.0, device="cuda"), torch.zeros((B,), device="cuda")
    return {"q_sample_logsnr_kernel": (lambda: ops.q_sample_logsnr(x, eps, logsnr), 12 * B * n + 4 * B),
            "vlb_term_kernel": (lambda: ops.vlb_term(out, z, eps, logsnr, weight, acc), 12 * B * n + 16 * B),
            "vlb_endpoints_kernel": (lambda: ops.vlb_endpoints(x, eps, 1.0 / 255), 8 * B * n + 8 * B)}


def kernel_times(reps=200):
    print(f"(b) the kernels alone at configs[2] (B = {B}, n = {CIN * S * S}), {reps} launches each, HIP events")
    for name, (fn, nbytes) in kernel_runs().items():
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
        print(f"    {name:22s} {us:7.1f} us per launch  {nbytes / 1e6:5.1f} MB algorithmic  {bw / 1e12:5.2f} TB/s = {bw / HBM_PEAK:.2f} of peak")


def se_vs_k(steps=300, bs=64, seeds=8, n_test=256):
    m = model(in_channels=1, bs=bs, timesteps=250)
    m.train()
    data = SyntheticMNIST(bs, steps, False, False, "cuda", seed=1000)
    t0 = time.perf_counter()
    for x, y in data:
        m.train_step(x, y)
    torch.cuda.synchronize()
    train_s = time.perf_counter() - t0
    m.eval()
    x, _ = next(iter(SyntheticMNIST(n_test, 1, False, False, "cuda", seed=2000)))
    print(f"(c) batch-mean nlogp of {n_test} synthetic test images (1x28x28, [-1, 1] data, unconditional) after {steps} steps at bs = {bs} "
          f"({train_s:.1f} s); {seeds} seeds per K")
    print("    K    mean nlogp   bpd      reported SE   SE over seeds   mean per-image se")
    for K in (1, 4, 16):
        batch = []
        reported = None
        for seed in range(seeds):
            r = m.nlogp(x, num_samples=K, seed=seed)
            batch.append(float(r["nlogp"].double().mean()))
            if seed == 0:
                se = r["se"].double()
                reported = float(se.pow(2).sum().sqrt()) / n_test
                per_image = float(se.mean())
        mean = statistics.mean(batch)
        spread = statistics.stdev(batch)
        rep = "    -    " if math.isnan(reported) else f"{reported:9.4f}"
        pim = "    -    " if math.isnan(per_image) else f"{per_image:9.4f}"
        print(f"    {K:2d}   {mean:9.4f}   {mean / math.log(2):7.4f}   {rep}     {spread:9.4f}       {pim}")


def stats(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    print(f"rocprofv3 --kernel-trace --stats ({path.rsplit('/', 1)[-1]}), `python tools/nlogp_probe.py kernels`:")
    for row in rows:
        if any(row["Name"].startswith(k) or f" {k}" in row["Name"] or f"::{k}" in row["Name"] for k in KERNELS):
            print(f"    {row['Name'][:60]:60s} calls {row['Calls']:>5s}  average {float(row['AverageNs']) / 1e3:7.1f} us  "
                  f"min {float(row['MinNs']) / 1e3:7.1f} us  max {float(row['MaxNs']) / 1e3:7.1f} us")


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "kernels":
        for fn, _ in kernel_runs().values():
            for _ in range(50):
                fn()
        torch.cuda.synchronize()
        return
    if len(sys.argv) > 2 and sys.argv[1] == "stats":
        stats(sys.argv[2])
        return
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    draw_times(rounds)
    kernel_times()
    se_vs_k()


if __name__ == "__main__":
    main()
