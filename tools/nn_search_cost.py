"""What the nearest-neighbour search costs, against a copy of the database and against the stock torch chain it replaces; same process, interleaved.

    python tools/nn_search_cost.py [rounds=5] [out=profiles/nn_search_cost.txt] [seconds the new GPU tests took, to be recorded]

Q = 1024 queries, k = 3, against N = 50 000 rows of D = 3072 bytes (CIFAR-10's training set) and N = 60 000 of D = 784 (MNIST's); random bytes
(the time of none of the arms depends on the values).
  (a) search   ops.nn_search_u8 with the database norms passed in, as neighbours.NeighbourIndex calls it: the queries' norms, the slab search
               (int8 MFMA) and the merge - three launches, timed together
  (b) copy     a device-to-device copy of the database's N D bytes: what reading it once and writing it once costs
  (c) torch    the obvious chain: database.float() (included: the database lives on the device as bytes), torch.cdist in fp32 over chunks of
               16 384 rows, topk of each chunk and a running topk over the chunks' winners
Every round times each arm once between two HIP events, the order alternating; medians and the spread over the rounds are printed.  Also
printed: how many of (c)'s first neighbours are (a)'s (fp32 orders near-ties by rounding; (a) is exact), and sqnorm's own time."""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from generative_models_amd import ops  # noqa: E402

Q, K, CHUNK = 1024, 3, 16384
SHAPES = {"CIFAR-10 rows": (50000, 3072), "MNIST rows": (60000, 784)}


def torch_chain(q, db):
    qf, dbf = q.float(), db.float()
    best_d = best_i = None
    for lo in range(0, db.shape[0], CHUNK):
        d, i = torch.topk(torch.cdist(qf, dbf[lo:lo + CHUNK]), K, dim=1, largest=False)
        i = i + lo
        if best_d is None:
            best_d, best_i = d, i
        else:
            d, pick = torch.topk(torch.cat((best_d, d), 1), K, dim=1, largest=False)
            best_d, best_i = d, torch.gather(torch.cat((best_i, i), 1), 1, pick)
    return best_d, best_i


def timed(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    out = fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e), out


def main_():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    out = sys.argv[2] if len(sys.argv) > 2 else "profiles/nn_search_cost.txt"
    tests_s = sys.argv[3] if len(sys.argv) > 3 else None
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"$ python tools/nn_search_cost.py {rounds}")
    emit(f"# {torch.cuda.get_device_name(0)}; Q = {Q}, k = {K}; ms per call between two HIP events, one call per arm and round, order alternating")
    for name, (N, D) in SHAPES.items():
        rng = np.random.default_rng(0)
        db = torch.from_numpy(rng.integers(0, 256, (N, D), dtype=np.uint8)).cuda()
        q = torch.from_numpy(rng.integers(0, 256, (Q, D), dtype=np.uint8)).cuda()
        norms = ops.u8_sqnorm(db)
        dst = torch.empty_like(db)
        arms = {"(a) search": lambda: ops.nn_search_u8(q, db, K, norms), "(b) copy": lambda: dst.copy_(db), "(c) torch": lambda: torch_chain(q, db)}
        results = {}
        for arm, fn in arms.items():             # warm-up: kernels loaded, allocator pools at their steady size
            for _ in range(2):
                results[arm] = fn()
        torch.cuda.synchronize()
        times = {arm: [] for arm in arms}
        for r in range(rounds):
            for arm in (list(arms) if r % 2 == 0 else reversed(list(arms))):
                times[arm].append(timed(arms[arm])[0])
        med = {arm: statistics.median(v) for arm, v in times.items()}
        emit(f"{name}: N = {N}, D = {D}: database {N * D / 1e6:.1f} MB, 2 Q N D = {2 * Q * N * D / 1e12:.3f} T integer operations")
        for arm, v in times.items():
            emit(f"  {arm}: median {med[arm]:8.3f} ms, spread {(max(v) - min(v)) / med[arm]:.1%}  (rounds: {', '.join(f'{x:.3f}' for x in v)})")
        a = med["(a) search"]
        emit(f"  (a) reads the database at {N * D / a / 1e9:.3f} TB/s and multiplies at {2 * Q * N * D / a / 1e9:.1f} T integer operations/s; "
             f"(a) / (b) = {a / med['(b) copy']:.2f}; (c) / (a) = {med['(c) torch'] / a:.2f}")
        same = int((results["(a) search"][1][:, 0] == results["(c) torch"][1][:, 0]).sum())
        emit(f"  first neighbours of (c) that are (a)'s: {same} of {Q}")
        t = [timed(lambda: ops.u8_sqnorm(db))[0] for _ in range(rounds + 2)][2:]
        emit(f"  u8_sqnorm of the database (once per run of the driver): median {statistics.median(t):.3f} ms")
        del db, q, dst, arms, results
        torch.cuda.empty_cache()
    if tests_s is not None:
        emit(f"# tests/test_gpu_nn.py on the same machine: {tests_s} s for the whole file (pytest's own figure)")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main_()
