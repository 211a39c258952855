"""Cost of dynamic thresholding (DG.dyn_threshold, gmk_dyn_threshold): the select launch alone against a copy of the same bytes, and the guided
DDIM sampler with the option on against off.

    python tools/dyn_threshold_cost.py kernel [iters=200]                 per shape: time per gmk_dyn_threshold launch (guided: v, v_uncond and z read
                                                                          once, 12 B per value) and per copy that moves the same bytes (half of
                                                                          them read, half written), HIP events around `iters` launches that rotate
                                                                          over enough buffer sets to exceed the 256 MiB Infinity Cache
    python tools/dyn_threshold_cost.py sampler [rounds=6] [steps=10]      per shape: guided DDIM steps/s (`steps` steps per sample() call) with
                                                                          dyn_threshold 0 and 0.995, same process, interleaved, the order alternating
    python tools/dyn_threshold_cost.py all                                both
Shapes: the bench's three, 1x28x28 B = 1024, 3x32x32 B = 2048, 3x64x64 B = 1024.  The option-off arm is the sampler as it was before the option
existed: no new kernel is launched in it."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402

SHAPES = [(1, 28, 1024), (3, 32, 2048), (3, 64, 1024)]
P = 0.995


def event_ms(fn, iters):
    """ms per call of fn(k), k = 0 ... iters - 1, between two device events (after a warm-up over every buffer set)."""
    for k in range(min(iters, 16)):
        fn(k)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for k in range(iters):
        fn(k)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def kernel(iters):
    for cin, size, B in SHAPES:
        n = cin * size * size
        nbytes = 3 * B * n * 4
        sets = max(2, min(64, -(-(640 << 20) // nbytes)))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn((B, cin, size, size), device="cuda", generator=g) * 1.5 for _ in range(3)] for _ in range(sets)]
        w = torch.rand((B,), device="cuda", generator=g) * 4
        t_sel = event_ms(lambda k: ops.dyn_threshold(bufs[k % sets][0], bufs[k % sets][2], -1.0, P, v_uncond=bufs[k % sets][1], cond_w=w), iters)
        src = [torch.cat([t.flatten() for t in bs])[: 3 * B * n // 2] for bs in bufs]
        dst = torch.empty_like(src[0])
        t_cp = event_ms(lambda k: dst.copy_(src[k % sets]), iters)
        del bufs, src, dst
        print(f"{cin}x{size}x{size} B={B}: n = {n} ({'LDS' if n <= ops.DYN_THRESHOLD_KEYS else 'recompute'} path), {nbytes / 1e6:.1f} MB per launch, "
              f"{sets} buffer sets;  select {t_sel * 1e3:.1f} us = {nbytes / t_sel / 1e9:.2f} TB/s;  copy of the same bytes {t_cp * 1e3:.1f} us = "
              f"{nbytes / t_cp / 1e9:.2f} TB/s;  select / copy {t_sel / t_cp:.2f}", flush=True)


def sampler(rounds, steps):
    Model = common.discover_models()["diffusion"]
    for cin, size, B in SHAPES:
        models = {}
        for p in (0.0, P):
            G = common.AttrDict(dict(Model.DG))
            G.update(lr=3e-4, pad32=int(size == 32), device="cuda", timesteps=steps, bs=B, in_channels=cin, dyn_threshold=p)
            torch.manual_seed(0)
            models[p] = Model(G).cuda().eval()
        g = torch.Generator(device="cuda").manual_seed(1)
        init = torch.randn((B, cin, size, size), device="cuda", generator=g)
        y = torch.randint(0, 10, (B,), device="cuda", generator=g)

        def run(m):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                m.diffusion.sample(net=partial(m.net, guide=y), init_x=init, cond_w=0.5, record=False)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)
        for m in models.values():
            run(m)
        rates = {p: [] for p in models}
        for r in range(rounds):
            for p in (models if r % 2 == 0 else reversed(list(models))):
                rates[p].append(run(models[p]))
        med = {p: statistics.median(v) for p, v in rates.items()}
        for p, v in rates.items():
            print(f"{cin}x{size}x{size} B={B} guided ddim, dyn_threshold {p}: median {med[p]:.2f} steps/s  (rounds: {', '.join(f'{x:.2f}' for x in v)})")
        print(f"{cin}x{size}x{size} B={B}: on / off {med[P] / med[0.0] - 1:+.2%}  ({1e3 / med[P] - 1e3 / med[0.0]:+.3f} ms per step)", flush=True)
        del models


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "all"
    assert torch.cuda.is_available(), "dyn_threshold_cost.py measures on the GPU"
    if mode in ("kernel", "all"):
        kernel(int(sys.argv[2]) if mode == "kernel" and len(sys.argv) > 2 else 200)
    if mode in ("sampler", "all"):
        sampler(int(sys.argv[2]) if mode == "sampler" and len(sys.argv) > 2 else 6, int(sys.argv[3]) if mode == "sampler" and len(sys.argv) > 3 else 10)


if __name__ == "__main__":
    main()
