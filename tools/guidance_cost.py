"""Cost of the guided samplers' two options (DG.guidance_lo / DG.guidance_hi, DG.cfg_rescale; gmk_cfg_rescale): the rescale launch alone against
a copy of the same bytes, and the guided DDIM sampler with guidance everywhere, inside an interval, nowhere, and inside the interval with the
rescale.

    python tools/guidance_cost.py kernel [out] [iters=200]               per shape: time per gmk_cfg_rescale launch (v, v_uncond and z read once, 12 B
                                                                         per value, for images of up to ops.CFG_RESCALE_KEEP values) and per copy that
                                                                         moves the same bytes (half of them read, half written), HIP events around
                                                                         `iters` launches that rotate over enough buffer sets to exceed the 256 MiB
                                                                         Infinity Cache
    python tools/guidance_cost.py sampler [out] [rounds=6] [steps=20]    per shape: DDIM steps/s (`steps` steps per sample() call), same process,
                                                                         interleaved, the order alternating, for four arms:
                                                                           (a) guidance at every step          (b) guidance inside [-3, 3]
                                                                           (c) no guidance                     (d) arm (b) with cfg_rescale 0.7
                                                                         with rho, the share of steps (b) guides, and the rate that (a) and (c) of
                                                                         the same run predict for (b): 1 / (rho / r_a + (1 - rho) / r_c)
    python tools/guidance_cost.py all [out]                              both
Shapes: the bench's three, 1x28x28 B = 1024, 3x32x32 B = 2048, 3x64x64 B = 1024.  The lines go to stdout and to `out` (default
profiles/guidance_cost.txt).  Reports, not assertions; nothing here measures sample quality."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import guidance_evals, guidance_mask, sampler_plan  # noqa: E402

SHAPES = [(1, 28, 1024), (3, 32, 2048), (3, 64, 1024)]
LO, HI, PHI = -3.0, 3.0, 0.7
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


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
        t_res = event_ms(lambda k: ops.cfg_rescale(bufs[k % sets][0], bufs[k % sets][2], -1.0, PHI, bufs[k % sets][1], w), iters)
        src = [torch.cat([t.flatten() for t in bs])[: 3 * B * n // 2] for bs in bufs]
        dst = torch.empty_like(src[0])
        t_cp = event_ms(lambda k: dst.copy_(src[k % sets]), iters)
        del bufs, src, dst
        say(f"{cin}x{size}x{size} B={B}: n = {n} ({'resident' if n <= ops.CFG_RESCALE_KEEP else 're-read'} path), {nbytes / 1e6:.1f} MB per launch, "
            f"{sets} buffer sets;  rescale {t_res * 1e3:.1f} us = {nbytes / t_res / 1e9:.2f} TB/s;  copy of the same bytes {t_cp * 1e3:.1f} us = "
            f"{nbytes / t_cp / 1e9:.2f} TB/s;  rescale / copy {t_res / t_cp:.2f}")


ARMS = {"a: guidance everywhere": (dict(), True),
        "b: guidance in [-3, 3]": (dict(guidance_lo=LO, guidance_hi=HI), True),
        "c: unguided": (dict(), False),
        "d: b + cfg_rescale 0.7": (dict(guidance_lo=LO, guidance_hi=HI, cfg_rescale=PHI), True)}


def sampler(rounds, steps):
    Model = common.discover_models()["diffusion"]
    plan = sampler_plan(steps)
    mask = guidance_mask(plan, (LO, HI))
    rho = sum(mask) / len(mask)
    for cin, size, B in SHAPES:
        models = {}
        for arm, (flags, _) in ARMS.items():
            G = common.AttrDict(dict(Model.DG))
            G.update(lr=3e-4, pad32=int(size == 32), device="cuda", timesteps=steps, bs=B, in_channels=cin, **flags)
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
                m.diffusion.sample(net=partial(m.net, guide=y), init_x=init, cond_w=0.5 if ARMS[arm][1] else None, record=False)
            torch.cuda.synchronize()
            return steps / (time.perf_counter() - t0)
        for arm in models:
            run(arm)
        rates = {arm: [] for arm in models}
        for r in range(rounds):
            for arm in (list(models) if r % 2 == 0 else reversed(list(models))):
                rates[arm].append(run(arm))
        med = {arm: statistics.median(v) for arm, v in rates.items()}
        head = f"{cin}x{size}x{size} B={B} ddim, {steps} steps"
        for arm, v in rates.items():
            say(f"{head}, {arm}: median {med[arm]:.2f} steps/s  (rounds: {', '.join(f'{x:.2f}' for x in v)}; spread "
                f"{(max(v) - min(v)) / med[arm]:.2%})")
        a, b, c, d = (med[arm] for arm in ARMS)
        pred = 1.0 / (rho / a + (1.0 - rho) / c)
        spread = max((max(v) - min(v)) / med[arm] for arm, v in rates.items())
        say(f"{head}: rho = {sum(mask)}/{len(mask)} = {rho:.3f} of the steps guided under (b), {guidance_evals(plan, mask, B)} images forwarded per call "
            f"against {2 * B * steps} (a) and {B * steps} (c);  predicted (b) {pred:.2f} steps/s, measured {b:.2f}: {b / pred - 1:+.2%} "
            f"({'within' if abs(b / pred - 1) <= spread else 'outside'} the arms' largest spread {spread:.2%});  b / a {b / a:.3f}, c / a {c / a:.3f}, "
            f"d / b {d / b - 1:+.2%} ({1e3 / d - 1e3 / b:+.3f} ms per step, {(1e3 / d - 1e3 / b) / rho:+.3f} ms per guided step)")
        del models


def main():
    args = sys.argv[1:]
    mode = args[0] if args else "all"
    out = args[1] if len(args) > 1 else "profiles/guidance_cost.txt"
    assert mode in ("kernel", "sampler", "all"), mode
    assert torch.cuda.is_available(), "guidance_cost.py measures on the GPU"
    num = lambda i, d: int(args[i]) if mode != "all" and len(args) > i else d
    say(f"tools/guidance_cost.py {mode} on {torch.cuda.get_device_name(0)}")
    if mode in ("kernel", "all"):
        kernel(num(2, 200))
    if mode in ("sampler", "all"):
        sampler(num(2, 6), num(3, 20))
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
