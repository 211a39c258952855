"""Cost of the power-function averages of post-hoc EMA (DG.ema_sigma_rel): writes profiles/posthoc_ema_cost.txt.

    python tools/posthoc_ema_cost.py [--out profiles/posthoc_ema_cost.txt] [--rounds 6] [--parts launch,combine,step]

launch   the optimiser launch with 0, 1, 2 and 3 power-function averages (28 + 8 k B per parameter) on the parameter arenas of the three
         bench shapes (bench.py CONFIGS cfg1, cfg2, cfg3), each set against a device copy that moves the same bytes, in the same run
combine  gmk_arena_combine at K = 32 on the cfg2 arena (4 K + 4 B per parameter) against a copy of its bytes
step     the train step under ema_sigma_rel = '0.05,0.1' against TWO default arms (their difference is the noise floor) at the three shapes

Every arm is warmed up first; the arms of a part alternate inside each round and the order flips from round to round; a figure is the median
over the rounds with the lowest and highest round beside it.  Launch and copy times are device-event times over `--launches` back-to-back
calls on the same buffers, so both arms see the same cache state; step times are a host clock around `--steps` steps ending in a device
synchronise."""
import argparse
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from generative_models_amd import common, ops  # noqa: E402

CONFIGS = {"cfg1": (1, 28, 1024), "cfg2": (3, 32, 2048), "cfg3": (3, 64, 1024)}      # bench.py: in_channels, size, per-GPU batch
ADAM = (3e-4, 0.9, 0.999, 1e-8)
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def model(cfg, **flags):
    cin, size, bs = CONFIGS[cfg]
    Model = common.discover_models()["diffusion"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=1000, bs=bs, in_channels=cin, seed=0, hidden_size=128)      # as bench.py builds it
    G.update(flags)
    torch.manual_seed(0)
    m = Model(G).cuda().train()
    m.size = size
    return m


def batch(cfg):
    cin, size, bs = CONFIGS[cfg]
    g = torch.Generator().manual_seed(1)
    return (torch.rand((bs, cin, size, size), generator=g) * 2 - 1).cuda(), torch.randint(0, 10, (bs,), generator=g).cuda()


def event_us(fn, launches):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(launches):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / launches


def alternate(arms, rounds, measure):
    """arms: {name: callable}.  -> {name: [one figure per round]}; the order of the arms flips every round."""
    for fn in arms.values():
        measure(fn)                                  # warm-up: code objects, allocator pools, captured graphs
    out = {name: [] for name in arms}
    for r in range(rounds):
        for name in (list(arms) if r % 2 == 0 else reversed(list(arms))):
            out[name].append(measure(arms[name]))
    return out


def fmt(vals, unit):
    return f"median {statistics.median(vals):9.3f} {unit}  [{min(vals):.3f} .. {max(vals):.3f}]"


def part_launch(args):
    say("# optimiser launch: adam_step (k = 0) / adam_pema_step (k power-function averages, no classic average, unsteered) against a device copy of the same bytes")
    for cfg in CONFIGS:
        n = model(cfg).net.flat_params.numel()
        torch.cuda.empty_cache()
        gen = torch.Generator(device="cuda").manual_seed(0)
        p, g, m, v = (torch.randn(n, device="cuda", generator=gen) * s for s in (1.0, 1e-2, 1e-3, 1.0))
        v = v.abs() * 1e-6
        store = torch.zeros((3, (n + 3) // 4 * 4), device="cuda")
        arms, nbytes = {}, {}
        for k in range(4):
            nbytes[k] = (28 + 8 * k) * n
            if k == 0:
                arms["k=0"] = lambda: ops.adam_step(p, g, m, v, *ADAM, 7)
            else:
                arms[f"k={k}"] = (lambda k: lambda: ops.adam_pema_step(p, g, m, v, store[:k, :n], (0.3, 0.2, 0.1)[:k], *ADAM, 7))(k)
            src = torch.zeros(nbytes[k] // 8, dtype=torch.float32, device="cuda")          # a copy reads and writes: half the bytes each way
            dst = torch.empty_like(src)
            arms[f"copy{k}"] = (lambda s, d: lambda: d.copy_(s))(src, dst)
        res = alternate(arms, args.rounds, lambda fn: event_us(fn, args.launches))
        say(f"{cfg}: arena {n} floats")
        for k in range(4):
            a, c = statistics.median(res[f"k={k}"]), statistics.median(res[f"copy{k}"])
            say(f"  k={k}  {nbytes[k] / 1e6:7.1f} MB  launch {fmt(res[f'k={k}'], 'us')}  {nbytes[k] / a / 1e6:6.2f} TB/s   "
                f"copy {fmt(res[f'copy{k}'], 'us')}  {nbytes[k] / c / 1e6:6.2f} TB/s   launch / copy {a / c:.3f}")
        base = statistics.median(res["k=0"])
        say("  launch time against k=0: " + ", ".join(f"k={k} x{statistics.median(res[f'k={k}']) / base:.3f} (bytes x{(28 + 8 * k) / 28:.3f})"
                                                       for k in range(1, 4)))
        del arms, p, g, m, v, store
        torch.cuda.empty_cache()


def part_combine(args):
    K = 32
    n = model("cfg2").net.flat_params.numel()
    torch.cuda.empty_cache()
    src = torch.randn((K, (n + 3) // 4 * 4), device="cuda")
    coef = torch.randn(K, dtype=torch.float64, device="cuda")
    out = torch.empty(n, device="cuda")
    nbytes = (4 * K + 4) * n
    a, b = torch.zeros(nbytes // 8, device="cuda"), torch.empty(nbytes // 8, device="cuda")
    arms = {"combine": lambda: ops.arena_combine(src[:, :n], coef, out=out), "copy": lambda: b.copy_(a)}
    res = alternate(arms, args.rounds, lambda fn: event_us(fn, max(1, args.launches // 4)))
    say(f"# gmk_arena_combine, K = {K}, cfg2 arena ({n} floats), {nbytes / 1e6:.1f} MB per launch, against a device copy of the same bytes")
    for name in arms:
        med = statistics.median(res[name])
        say(f"  {name:8s} {fmt(res[name], 'us')}  {nbytes / med / 1e6:6.2f} TB/s")
    say(f"  combine / copy {statistics.median(res['combine']) / statistics.median(res['copy']):.3f}")


def part_step(args):
    say("# train step: ema_sigma_rel = '0.05,0.1' (two averages, 44 B / parameter in the optimiser launch) against two default arms")
    for cfg in CONFIGS:
        x, y = batch(cfg)
        models = {"default A": model(cfg), "default B": model(cfg), "pema": model(cfg, ema_sigma_rel="0.05,0.1")}

        def steps(m):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                m.train_step(x, y.clone())
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps * 1e3

        res = alternate({k: (lambda m: lambda: m)(m) for k, m in models.items()}, args.rounds, lambda fn: steps(fn()))
        med = {k: statistics.median(v) for k, v in res.items()}
        say(f"{cfg}: arena {models['pema'].net.flat_params.numel()} floats, {args.steps} steps per round")
        for k, v in res.items():
            say(f"  {k:10s} {fmt(v, 'ms per step')}")
        base = 0.5 * (med["default A"] + med["default B"])
        say(f"  default B / default A {med['default B'] / med['default A'] - 1:+.3%} (noise floor);  pema / default {med['pema'] / base - 1:+.3%} "
            f"= {1e3 * (med['pema'] - base):+.1f} us per step")
        assert torch.equal(models["pema"].net.flat_params, models["default A"].net.flat_params), "the averages moved the training weights"
        del models
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/posthoc_ema_cost.txt")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--parts", default="launch,combine,step")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/posthoc_ema_cost.py measures on the GPU: no device found")
    say(f"# post-hoc EMA cost on one {torch.cuda.get_device_name(0)}: python tools/posthoc_ema_cost.py --rounds {args.rounds} --launches {args.launches} "
        f"--steps {args.steps}")
    say("# one GPU; multi-GPU runs are untested.  Figures: median over the rounds [lowest .. highest round]")
    for part in args.parts.split(","):
        {"launch": part_launch, "combine": part_combine, "step": part_step}[part](args)
        with open(args.out, "w") as f:               # after every part: a run cut short keeps what it measured
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
