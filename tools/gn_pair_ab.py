"""Paired GroupNorm + SiLU kernels against the launches they replace, same box, interleaved.
Per launch, at the train step's shapes (B = 2048, C = 128, fp16 x, bf16 gradients): gmk_gn_silu_bwd_pair against the two gmk_gn_silu_bwd launches at
32 x 32 and 16 x 16 (HBM: 9 tensor passes for the two launches, 4 + 5; the pair moves 7 at 32 x 32 - dy_dn twice - and 6 at 16 x 16), and
gmk_gn_silu_fwd_pair against two gmk_gn_silu_fwd launches at 16 x 16 (4 passes against 3).
Whole step: `python tools/gn_pair_ab.py N` then runs N interleaved pairs of `bench.py --gpus 1 --steps 50 --warmup 10` with GMK_GN_PAIR=0 / 1
(each in a process of its own) and prints the means, the spread of the two-launch runs and the gain."""
import json
import os
import subprocess
import sys
import torch
sys.path.insert(0, ".")
from generative_models_amd import ops


def timed(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n * 1e3


B, C = 2048, 128
for S in (32, 16):
    g = torch.Generator().manual_seed(0)
    x = torch.randn((B, S, S, C), generator=g).cuda().half()
    t = lambda: torch.randn((B, S, S, C), generator=g).cuda().bfloat16()
    dy_u, dadd_u, dy_d, dadd_d = t(), t(), t(), t()
    gam, bet = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
    _, mu, ru = ops.gn_silu_fwd(x, gam, bet, 16)
    _, md, rd = ops.gn_silu_fwd(x, gam, bet, 32)
    dxs = torch.empty((B, C), device="cuda")
    N = x.numel() * 2

    def two():
        ds, _, _ = ops.gn_silu_bwd(dy_u, x, gam, bet, mu, ru, dadd1=dadd_u)
        return ops.gn_silu_bwd(dy_d, x, gam, bet, md, rd, dadd1=dadd_d, dadd2=ds, dxsum=dxs)

    pair = lambda: ops.gn_silu_bwd_pair(x, (dy_u, dadd_u, gam, bet, mu, ru), (dy_d, dadd_d, gam, bet, md, rd), dxsum=dxs)
    assert ops.gn_pair_ok(x, 16, 32)
    np_ = 7 if S == 32 else 6
    for rnd in range(3):
        t2, t1 = timed(two), timed(pair)
        print(f"backward B={B} {S}x{S}: two launches {t2:7.1f} us ({9 * N / t2 / 1e6:5.2f} TB/s)  pair {t1:7.1f} us ({np_ * N / t1 / 1e6:5.2f} TB/s)  "
              f"ratio {t1 / t2:.3f}", flush=True)
    if ops.gn_pair_fwd_ok(x, 32, 16):
        two_f = lambda: (ops.gn_silu_fwd(x, gam, bet, 32), ops.gn_silu_fwd(x, gam, bet, 16))
        pair_f = lambda: ops.gn_silu_fwd_pair(x, (gam, bet, 32), (gam, bet, 16))
        for rnd in range(3):
            t2, t1 = timed(two_f), timed(pair_f)
            print(f"forward  B={B} {S}x{S}: two launches {t2:7.1f} us ({4 * N / t2 / 1e6:5.2f} TB/s)  pair {t1:7.1f} us ({3 * N / t1 / 1e6:5.2f} TB/s)  "
                  f"ratio {t1 / t2:.3f}", flush=True)
    del x, dy_u, dadd_u, dy_d, dadd_d

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 0
if reps:
    torch.cuda.empty_cache()
    ms = {"0": [], "1": []}
    for rep in range(reps):
        for v in ("0", "1"):
            r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "50", "--warmup", "10"], env=dict(os.environ, GMK_GN_PAIR=v),
                               capture_output=True, text=True, timeout=300, check=True)
            d = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")][-1]
            ms[v].append(d["ms_per_step"])
            print(f"step rep {rep + 1} GMK_GN_PAIR={v}: {d['ms_per_step']} ms/step {d['value']} img/s", flush=True)
    m0, m1 = sum(ms["0"]) / reps, sum(ms["1"]) / reps
    spread = max(ms["0"]) - min(ms["0"])
    print(f"two launches: mean {m0:.3f} ms, spread {spread:.3f} ms ({min(ms['0'])} .. {max(ms['0'])});  pair: mean {m1:.3f} ms, spread {max(ms['1']) - min(ms['1']):.3f} ms")
    print(f"gain {m0 - m1:.3f} ms = {100 * (m0 - m1) / m0:.2f} % of the two-launch mean;  3 x spread = {3 * spread:.3f} ms: "
          f"{'a gain' if m0 - m1 > 3 * spread else 'inside the noise'}")
