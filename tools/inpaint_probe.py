"""RePaint inpainting (`GaussianDiffusion.inpaint`, gmk_inpaint_merge, DG.inpaint_eval): what the merge kernel costs, what it adds to a sampler
step, and how often the learning check's completions are right at each resample count.

    python tools/inpaint_probe.py [rounds=3]      (a) - (c) below
    python tools/inpaint_probe.py kernels         the merge kernel alone (the workload of a `rocprofv3 --kernel-trace --stats` run)
    python tools/inpaint_probe.py stats <csv>     the merge kernel's rows of that run's kernel_stats.csv

(a) gmk_inpaint_merge alone at BASELINE configs[2] (3x32x32, B = 2048, n = 3072) with the top half known, unguided and with z_dup, without and
    with the jump back (renoise), 200 launches each, HIP events.  Algorithmic bytes: z read 4 + x0 read 4 + mask 1 + z written 4 (+ 4 z_dup)
    per element, plus the logsnr_next fill (4 B per row, 8 with z_dup); the fraction of the 8 TB/s HBM peak.
(b) One inpainting step (r = 1, DDIM, T = 20, top half known) against one plain DDIM sampler step at configs[2] (C = 128, 16-bit mode,
    bench.py's seeded weights): whole chains (record=False), 3 interleaved rounds, medians, per step.
(c) The learning check of tests/test_gpu_inpaint.py (G7, tests/inpaint_ref.py): the default net trained on two fixed 1x28x28 images, then the
    fraction of 64 completions (32 per mode) whose bottom half is nearer the right mode, at r in {1, 2, 5, 10}, and the fraction of 64
    unconditional samples nearer mode 0."""
import csv
import os
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import bench  # noqa: E402
import inpaint_ref  # noqa: E402
from generative_models_amd import common, ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import inpaint_coefs  # noqa: E402

CIN, S, B, _, _ = bench.CONFIGS["cfg2"]
HBM_PEAK = 8.0e12
KERNEL = "inpaint_merge_kernel"


def model(**flags):
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=1000, bs=B, compute_dtype="bf16", in_channels=CIN, seed=0, attention=0)
    G.update(flags)
    torch.manual_seed(G.seed)                  # bench.py's seeded weights
    return Model(G).cuda().eval()


def top_half(c, s):
    m = torch.zeros((1, c, s, s), dtype=torch.uint8)
    m[:, :, : s // 2] = 1
    return m


def kernel_runs():
    n = CIN * S * S
    g = torch.Generator(device="cuda").manual_seed(2)
    z = torch.randn((B, CIN, S, S), device="cuda", generator=g)
    x0 = torch.rand((B, CIN, S, S), device="cuda", generator=g) * 2 - 1
    mask = top_half(CIN, S).expand(B, CIN, S, S).reshape(B, n).contiguous().cuda()
    z2 = torch.empty((2 * B, CIN, S, S), device="cuda")
    z2[:B] = z
    ln, ln2 = torch.empty((B,), device="cuda"), torch.empty((2 * B,), device="cuda")
    c = inpaint_coefs(20)[5]
    runs = {}
    for renoise in (False, True):
        args = (c.alpha_s, c.sigma_s, c.a, c.b, False, renoise, c.lt, c.ls, 7, 0)
        tag = "renoise" if renoise else "merge"
        runs[f"{tag:7s} unguided"] = (lambda a=args: ops.inpaint_merge(z, x0, mask, *a, logsnr_next=ln), 13 * B * n + 4 * B)
        runs[f"{tag:7s} z_dup"] = (lambda a=args: ops.inpaint_merge(z2[:B], x0, mask, *a, z_dup=z2[B:], logsnr_next=ln2), 17 * B * n + 8 * B)
    return runs


def kernel_times(reps=200):
    print(f"(a) {KERNEL} alone at configs[2] (B = {B}, n = {CIN * S * S}, top half known), {reps} launches each, HIP events")
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
        print(f"    {name:18s} {us:7.1f} us per launch  {nbytes / 1e6:5.1f} MB algorithmic  {bw / 1e12:5.2f} TB/s = {bw / HBM_PEAK:.2f} of peak")


def step_times(rounds):
    m = model()
    m.size = S
    g = torch.Generator().manual_seed(1)
    x0 = (torch.rand((B, CIN, S, S), generator=g) * 2 - 1).cuda()
    init = torch.randn((B, CIN, S, S), generator=g).cuda()
    y = torch.randint(0, 10, (B,), generator=g).cuda()
    mask = top_half(CIN, S).cuda()
    T = 20
    d = m.diffusion
    d.sampler, d.num_steps = "ddim", T
    net = partial(m.net, guide=y)
    runs = {"ddim chain": lambda: d.sample(net=net, init_x=init, record=False),
            "inpaint chain": lambda: d.inpaint(net=net, x0=x0, mask=mask, init_x=init, resample=1)}
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
    print(f"(b) configs[2] (3x32x32, B = {B}, 16-bit mode), DDIM, T = {T}, r = 1, {rounds} interleaved rounds, medians")
    for k, v in times.items():
        print(f"    {k:13s} {med[k]:9.3f} ms   rounds: {', '.join(f'{t:.3f}' for t in v)}")
    a, b = med["ddim chain"] / T, med["inpaint chain"] / T
    print(f"    per step: DDIM {a:.3f} ms, inpainting {b:.3f} ms = {b / a:.4f} x")


def accuracy():
    t0 = time.perf_counter()
    m = inpaint_ref.train_two_mode(lambda **f: model(**f))
    train_s = time.perf_counter() - t0
    print(f"(c) learning check: two modes, {inpaint_ref.LEARNING_CHECK_STEPS} steps at bs = {inpaint_ref.LEARNING_CHECK_BS} ({train_s:.1f} s "
          f"with start-up), DDIM T = {inpaint_ref.LEARNING_CHECK_T}, 64 completions per r, seeds fixed")
    for r in (1, 2, 5, 10):
        t0 = time.perf_counter()
        right, uncond = inpaint_ref.completion_accuracy(m, r)
        torch.cuda.synchronize()
        print(f"    r = {r:2d}   right mode {right:.3f}   unconditional nearer mode 0 {uncond:.3f}   ({time.perf_counter() - t0:.2f} s)")


def stats(path):
    with open(path) as f:
        rows = list(csv.DictReader(f))
    print(f"rocprofv3 --kernel-trace --stats ({path.rsplit('/', 1)[-1]}), `python tools/inpaint_probe.py kernels`:")
    for row in rows:
        if KERNEL in row["Name"]:
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
    kernel_times()
    step_times(rounds)
    accuracy()


if __name__ == "__main__":
    main()
