"""What the k-NN radius and ball-count kernels cost, against the torch chains they replace and against the fp32 vector roof; and where the
time of a heavy evaluation at 10 000 samples goes.  Same process, interleaved rounds.

    python tools/knn_cost.py [rounds=7] [out=profiles/knn_cost.txt] [eval=1]

Gaussian rows of D = 64, k = 3.
  N = 10 000   (a) radius   ops.knn_radius2 (tile launch + merge)          (c) torch radius   torch.cdist(a, a) + topk(k + 1, largest=False)
               (b) counts   ops.ball_counts (two memsets + tile launch)     (d) torch counts   torch.cdist(q, balls) < r, .any(1), .sum(1), .sum(0)
               every round times each arm once between two HIP events, the order alternating; medians and the spread over the rounds.
  N = 50 000   (a) and (b) alone, with the workspace bytes: (c) and (d) would each hold a 10 GB matrix.
Roof: MI355X_MICROARCH's fp32 vector peak, 157.3 TFLOP/s = 78.6 T lane-instructions/s at 2 FLOP each; a pair element costs two (one v_sub,
one v_fma), so the roof is 39.3 T pair elements/s and a launch over N x M pairs of D elements cannot take less than N M D / 39.3e12 s.
eval=1: metrics.eval_heavy at --eval_heavy_samples 10000 on the bench's 3 x 32 x 32 shape (hidden_size 128, bs 2048, 250 sampler steps,
class_cond 0; random weights and random bytes as data - none of the three times depends on the values), with an untrained
arbiter_models.Autoencoder as the encoder, split into sampling, embedding and metrics as the evaluation itself logs them.  The evaluation draws through sample(n, y = -1), the
reference's call, which is the guided sampler: 2 B images per step, the guided rate of profiles/guidance_cost.txt."""
import statistics
import sys
import tempfile
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, ".")
from generative_models_amd import ops  # noqa: E402

D, K = 64, 3
ROOF = 157.3e12 / 4          # pair elements per second


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def torch_radius(a):
    return torch.topk(torch.cdist(a, a), K + 1, dim=1, largest=False).values[:, -1]


def torch_counts(balls, r, queries):
    inside = torch.cdist(queries, balls) < r[None, :]
    return inside.any(1), inside.sum(1), inside.sum(0)


def rounds_of(arms, rounds):
    for fn in arms.values():             # warm-up: kernels loaded, allocator pools at their steady size
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {arm: [] for arm in arms}
    for r in range(rounds):
        for arm in (list(arms) if r % 2 == 0 else reversed(list(arms))):
            times[arm].append(timed(arms[arm])[0])
    return times


def report(emit, times, pairs):
    med = {arm: statistics.median(v) for arm, v in times.items()}
    for arm, v in times.items():
        line = f"  {arm}: median {med[arm]:9.3f} ms, spread {(max(v) - min(v)) / med[arm]:.1%}  (rounds: {', '.join(f'{x:.3f}' for x in v)})"
        if arm[:3] in ("(a)", "(b)"):
            line += f"; {pairs * D / med[arm] / 1e9:.2f} T pair elements/s = {pairs * D / ROOF / (med[arm] * 1e-3):.1%} of the fp32 vector roof"
        emit(line)
    return med


def heavy_eval_split(emit):
    from generative_models_amd import arbiter_models, common, main
    from generative_models_amd import metrics as heavy
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        rng = np.random.default_rng(0)
        for split, n in (("train", 2048), ("test", 10240)):
            np.save(tmp / f"{split}_images.npy", rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8))
            np.save(tmp / f"{split}_labels.npy", rng.integers(0, 10, n).astype(np.uint8))
        G = common.AttrDict(dict(arbiter_models.Autoencoder.DG))
        G.update(hidden_size=256, lr=3e-4, in_channels=3, image_size=32, model="autoencoder", pad32=0)
        arbiter = arbiter_models.Autoencoder(G).cuda()
        arbiter.save(tmp)
        model, train_ds, test_ds, autoencoder, classifier, G = main.load_model_and_data(
            ["--model=diffusion", "--hidden_size", "128", "--in_channels", "3", "--image_size", "32", "--bs", "2048", "--class_cond", "0",
             "--data", "npy", "--data_device", "1", "--data_root", str(tmp), "--eval_heavy", "1", "--eval_heavy_samples", "10000",
             "--autoencoder", str(tmp / "model.jit.pt"), "--logdir", str(tmp / "run")])
        model.eval()
        for n in range(2):
            log = defaultdict(list)
            heavy.eval_heavy(log, model, test_ds, autoencoder, classifier, G)
            torch.cuda.synchronize()
            took = {key: log[f"dt/eval_heavy_{key}"][0] for key in ("sampling", "embedding", "metrics")}
            emit(f"  run {n} ({'warm-up' if n == 0 else 'timed'}): {int(log['eval/heavy_samples'][0])} samples, 10 000 test images; sampling "
                 f"{took['sampling']:.2f} s ({int(G.timesteps)} steps x 5 batches of 2048), embedding {took['embedding']:.3f} s, metrics "
                 f"{took['metrics']:.3f} s (two radius launches, two count launches, the moments and a 64 x 64 eigenvalue problem on the host)")


def main_():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/knn_cost.txt"
    with_eval = (int(sys.argv[3]) if len(sys.argv) > 3 else 1) != 0
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"$ python tools/knn_cost.py {rounds}")
    emit(f"# {torch.cuda.get_device_name(0)}; D = {D}, k = {K}; ms per call between two HIP events, one call per arm and round, order alternating")
    emit(f"# roof: 157.3 TFLOP/s fp32 vector = {ROOF / 1e12:.1f} T pair elements/s at two instructions (v_sub, v_fma) per pair element")
    g = torch.Generator().manual_seed(0)
    for N in (10000, 50000):
        a = torch.randn((N, D), generator=g).cuda()
        q = (0.9 * torch.randn((N, D), generator=g) + 0.1).cuda()
        r2 = ops.knn_radius2(a, K)
        r = r2.sqrt()
        arms = {"(a) radius": lambda: ops.knn_radius2(a, K), "(b) counts": lambda: ops.ball_counts(a, r2, q)}
        if N <= 10000:
            arms["(c) torch radius"] = lambda: torch_radius(a)
            arms["(d) torch counts"] = lambda: torch_counts(a, r, q)
        emit(f"N = M = Q = {N}: {N * N * D / 1e9:.1f} G pair elements per launch; workspace of the radius launch "
             f"{ops.lib.gmk_knn_radius_workspace(N, K)} bytes")
        med = report(emit, rounds_of(arms, rounds), float(N) * N)
        if N <= 10000:
            emit(f"  (c) / (a) = {med['(c) torch radius'] / med['(a) radius']:.2f}; (d) / (b) = {med['(d) torch counts'] / med['(b) counts']:.2f}")
            got, want = ops.knn_radius2(a, K), torch_radius(a) ** 2
            emit(f"  radius: largest relative difference between (a) and (c)^2 {float(((got - want).abs() / want).max()):.2e}")
            gq, gm = ops.ball_counts(a, r2, q)
            _, tq, tm = torch_counts(a, r, q)
            emit(f"  counts: queries whose count differs between (b) and (d) {int((gq != tq).sum())} of {N}, balls {int((gm != tm).sum())} of {N} "
                 f"(cdist expands |a|^2 + |b|^2 - 2 a.b and compares distances, not squares)")
        del a, q, r2, r, arms
        torch.cuda.empty_cache()
    if with_eval:
        emit("heavy evaluation, --eval_heavy_samples 10000 at 3 x 32 x 32 (hidden_size 128, bs 2048, class_cond 0):")
        heavy_eval_split(emit)
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main_()
