"""Cost of the learned reverse-process variance: its two kernels, the train step and the sampler with it.

    python tools/learned_var_cost.py kernel [out] [rounds=7] [iters=200]   per shape: time per launch of gmk_hybrid_loss (gradients on: v, nu, z, x, eps
                                                                           read, dv and dnu written, 28 B per value at the sizes kept in LDS)
                                                                           against gmk_v_loss (dv on) and against a device copy that moves the
                                                                           same bytes; and of gmk_stochastic_step_lv (v, z, nu read, z_next written:
                                                                           16 B per value) against gmk_stochastic_step (12 B) and a copy of its own
                                                                           bytes.  HIP events around `iters` launches that rotate over enough buffer
                                                                           sets to exceed the 256 MiB Infinity Cache; `rounds` rounds, the arms
                                                                           interleaved, the order alternating; medians
    python tools/learned_var_cost.py train [out] [rounds=5] [steps=6]      per shape: ms per train_step of a learn_var 1 model against TWO default
                                                                           models of the same build (the spread between those two is the noise of
                                                                           the comparison; the default step launches what it launched before the
                                                                           variance head existed, so it stands in for that build's step)
    python tools/learned_var_cost.py sampler [out] [rounds=5] [steps=20]   per shape: steps/s of the 20-step 'ancestral' sampler with posterior_var
                                                                           'learned' against 'large' on the same learn_var network
    python tools/learned_var_cost.py all [out]                             all three
Shapes: the bench's three, 1x28x28 B = 1024, 3x32x32 B = 2048, 3x64x64 B = 1024.  Everything printed is also written to `out` (default
profiles/learned_var_cost.txt).  The profile also carries a block the tool does not produce, from the line that starts with ACCURACY_MARK to the
end: the error figures tests/test_gpu_learned_var.py prints; a run keeps that block of the default profile as it is.  Reports, not assertions;
nothing here measures sample quality or likelihood."""
import statistics
import sys
import time
from functools import partial

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402
from generative_models_amd.diffusion.gaussian_diffusion import learned_half_delta, stochastic_row  # noqa: E402

SHAPES = [(1, 28, 1024), (3, 32, 2048), (3, 64, 1024)]
PROFILE = "profiles/learned_var_cost.txt"
ACCURACY_MARK = "Accuracy of the two kernels"
LINES = []


def kept_block():
    """The hand-kept accuracy block of the default profile ('' if there is none): the lines from ACCURACY_MARK on."""
    try:
        lines = open(PROFILE).read().split("\n")
    except OSError:
        return ""
    at = next((i for i, line in enumerate(lines) if line.startswith(ACCURACY_MARK)), None)
    return "" if at is None else "\n" + "\n".join(lines[at:]).rstrip("\n") + "\n"


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


def interleaved(arms, rounds, run):
    """run(arm) `rounds` times per arm, the arms interleaved and the order alternating.  -> {arm: [values]}"""
    out = {name: [] for name in arms}
    for r in range(rounds):
        for name in (list(arms) if r % 2 == 0 else reversed(list(arms))):
            out[name].append(run(name))
    return out


def kernel(rounds, iters):
    lt_s, ls_s, seed = -1.0, 0.5, 7
    c_z, c_x, cn_small = stochastic_row("ancestral", lt_s, ls_s, 0.0)
    large = stochastic_row("ancestral", lt_s, ls_s, 1.0)
    hd = learned_half_delta(lt_s, ls_s)
    for cin, size, B in SHAPES:
        n = cin * size * size
        shape = (B, cin, size, size)
        per_tensor = B * n * 4
        sets = max(2, min(48, -(-(640 << 20) // (5 * per_tensor))))
        g = torch.Generator(device="cuda").manual_seed(0)
        bufs = [[torch.randn(shape, device="cuda", generator=g) for _ in range(5)] for _ in range(sets)]      # v, nu, z, x, eps
        u = torch.rand((B,), device="cuda", generator=g)
        logsnr = ops.logsnr_schedule(B, "cuda", u=u)
        logsnr_s = ops.logsnr_schedule(B, "cuda", u=ops.aligned((u - 1e-3).clamp_(min=0.0)))
        # one read pass + one write pass of a copy moves 2 bytes per byte copied: 3.5 tensors for the loss's 7, 2 for the step's 4, 1.5 for 3
        flat = [torch.cat([t.reshape(-1) for t in s]) for s in bufs]
        dst = torch.empty(4 * B * n, device="cuda")
        copy_of = lambda tensors_moved: (lambda k: dst[:tensors_moved * B * n // 2].copy_(flat[k % sets][:tensors_moved * B * n // 2]))
        q = B * n // 4
        assert n <= ops.X_LOSS_KEEP                 # every shape here stays in LDS: each tensor is read once
        moved = {"gmk_hybrid_loss": 7, "gmk_v_loss": 9, "copy of the loss's bytes": 7,
                 "gmk_stochastic_step_lv": 4, "gmk_stochastic_step": 3, "copy of the step's bytes": 4}      # tensors read + written

        def hybrid(k):
            v, nu, z, x, eps = bufs[k % sets]
            ops.hybrid_loss(v, nu, z, x, eps, logsnr, logsnr_s, 0.001, grad_scale=1.0 / B)

        def vloss(k):
            v, _, z, x, eps = bufs[k % sets]
            ops.v_loss(v, z, x, eps, logsnr, grad_scale=1.0 / B)

        def step_lv(k):
            v, nu, z, _, _ = bufs[k % sets]
            ops.stochastic_step_lv(v, z, nu, lt_s, ls_s, c_z, c_x, cn_small, hd, False, seed, k * q)

        def step(k):
            v, _, z, _, _ = bufs[k % sets]
            ops.stochastic_step(v, z, lt_s, ls_s, *large, 0.0, False, seed, k * q)
        arms = {"gmk_hybrid_loss": hybrid, "gmk_v_loss": vloss, "copy of the loss's bytes": copy_of(moved["copy of the loss's bytes"]),
                "gmk_stochastic_step_lv": step_lv, "gmk_stochastic_step": step, "copy of the step's bytes": copy_of(4)}
        for fn in arms.values():                    # warm-up over every buffer set
            for k in range(sets):
                fn(k)
        torch.cuda.synchronize()
        times = interleaved(arms, rounds, lambda name: event_ms(arms[name], iters))
        med = {name: statistics.median(v) for name, v in times.items()}
        for name, v in times.items():
            gb = moved[name] * per_tensor / 1e9
            say(f"{cin}x{size}x{size} B={B} {name}: median {med[name] * 1e3:.1f} us per launch, {gb * 1e3:.1f} MB = {gb / med[name]:.2f} TB/s  "
                f"(rounds: {', '.join(f'{x * 1e3:.1f}' for x in v)}; spread {(max(v) - min(v)) / med[name]:.1%})")
        loss_copy, step_copy = med["copy of the loss's bytes"], med["copy of the step's bytes"]
        say(f"{cin}x{size}x{size} B={B}: {sets} buffer sets;  gmk_hybrid_loss / gmk_v_loss = {med['gmk_hybrid_loss'] / med['gmk_v_loss']:.3f}, "
            f"gmk_hybrid_loss reaches {loss_copy / med['gmk_hybrid_loss']:.1%} of the copy rate;  "
            f"gmk_stochastic_step_lv / gmk_stochastic_step = {med['gmk_stochastic_step_lv'] / med['gmk_stochastic_step']:.3f}, "
            f"gmk_stochastic_step_lv reaches {step_copy / med['gmk_stochastic_step_lv']:.1%} of the copy rate")
        del bufs, flat, dst, arms


def _model(cin, size, B, steps=20, **flags):
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=steps, bs=B, in_channels=cin, image_size=size, **flags)
    torch.manual_seed(0)
    return Model(G).cuda()


def train(rounds, steps):
    for cin, size, B in SHAPES:
        models = {"default (a)": _model(cin, size, B).train(), "default (b)": _model(cin, size, B).train(),
                  "learn_var 1": _model(cin, size, B, learn_var=1).train()}
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.rand((B, cin, size, size), device="cuda", generator=g) * 2 - 1
        y = torch.randint(0, 10, (B,), device="cuda", generator=g)

        def run(arm):
            m = models[arm]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                m.train_step(x, y.clone())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3
        for arm in models:
            run(arm)
        ms = interleaved(models, rounds, run)
        med = {arm: statistics.median(v) for arm, v in ms.items()}
        head = f"{cin}x{size}x{size} B={B} train_step"
        for arm, v in ms.items():
            say(f"{head}, {arm}: median {med[arm]:.2f} ms  (rounds: {', '.join(f'{t:.2f}' for t in v)}; spread {(max(v) - min(v)) / med[arm]:.2%})")
        base = 0.5 * (med["default (a)"] + med["default (b)"])
        say(f"{head}: learn_var 1 / default = {med['learn_var 1'] / base:.4f} ({med['learn_var 1'] - base:+.3f} ms); the two default arms differ by "
            f"{abs(med['default (a)'] - med['default (b)']) / base:.2%}")
        del models


def sampler(rounds, steps):
    for cin, size, B in SHAPES:
        models = {"large": _model(cin, size, B, steps, learn_var=1, sampler="ancestral", posterior_var="large").eval(),
                  "learned": _model(cin, size, B, steps, learn_var=1, sampler="ancestral", posterior_var="learned").eval()}
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
        rates = interleaved(models, rounds, run)
        med = {arm: statistics.median(v) for arm, v in rates.items()}
        head = f"{cin}x{size}x{size} B={B}, {steps} steps, sampler 'ancestral'"
        for arm, v in rates.items():
            say(f"{head}, posterior_var {arm}: median {med[arm]:.2f} steps/s  (rounds: {', '.join(f'{x:.2f}' for x in v)}; "
                f"spread {(max(v) - min(v)) / med[arm]:.2%})")
        say(f"{head}: learned / large = {med['learned'] / med['large']:.4f} ({1e3 / med['learned'] - 1e3 / med['large']:+.3f} ms per step)")
        del models


def main():
    args = sys.argv[1:]
    mode = args[0] if args else "all"
    out = args[1] if len(args) > 1 else PROFILE
    assert mode in ("kernel", "train", "sampler", "all"), mode
    assert torch.cuda.is_available(), "learned_var_cost.py measures on the GPU"
    num = lambda i, d: int(args[i]) if mode != "all" and len(args) > i else d
    say(f"tools/learned_var_cost.py {mode} on {torch.cuda.get_device_name(0)}")
    if mode in ("kernel", "all"):
        kernel(num(2, 7), num(3, 200))
    if mode in ("train", "all"):
        train(num(2, 5), num(3, 6))
    if mode in ("sampler", "all"):
        sampler(num(2, 5), num(3, 20))
    say("No sample-quality or likelihood number was measured.")
    kept = kept_block()
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n" + kept)


if __name__ == "__main__":
    main()
