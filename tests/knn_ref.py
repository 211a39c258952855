"""Host restatement of the k-NN radius and ball-count kernels (include/gmk.h: gmk_knn_radius_f32, gmk_ball_counts_f32) in numpy float64:
the yardstick of tests/test_gpu_knn.py, tests/test_gpu_arbiters.py and the CPU test of metrics.manifold_metrics."""
import numpy as np


def d2(a, b):
    """[A, B] float64: sum_i (a[i] - b[i])^2 for every pair of rows, the direct difference (row blocks keep the temporaries small)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.empty((a.shape[0], b.shape[0]), dtype=np.float64)
    step = max(1, (1 << 22) // max(1, b.shape[0] * b.shape[1]))
    for lo in range(0, a.shape[0], step):
        diff = a[lo:lo + step, None, :] - b[None, :, :]
        out[lo:lo + step] = np.einsum("abi,abi->ab", diff, diff)
    return out


def radius2(pts, k):
    """[N] float64: the (k + 1)-th smallest value of every row of d2(pts, pts), the point itself (0) included."""
    return np.sort(d2(pts, pts), axis=1)[:, k]


def inside(balls, r2, queries):
    """[Q, M] bool: d2(queries[q], balls[j]) < r2[j], strict."""
    return d2(queries, balls) < np.asarray(r2, dtype=np.float64)[None, :]


def counts(balls, r2, queries):
    """(q_count [Q], m_count [M]) int64: balls that hold each query, queries that each ball holds."""
    hit = inside(balls, r2, queries)
    return hit.sum(1), hit.sum(0)


def window(D):
    """Relative half-width inside which an fp32 decision may differ from the float64 one: the fma chain's worst-case relative error D 2^-24
    plus the subtraction's 2 2^-24, once for d2 and once for r2.  Derived, not tuned: 7.9e-6 at D = 64."""
    return 2.0 * (D + 2) * 2.0 ** -24


def ambiguous(balls, r2, queries, D):
    """[Q, M] bool: the pairs whose float64 margin |d2 - r2| is at most window(D) r2."""
    r2 = np.asarray(r2, dtype=np.float64)[None, :]
    return np.abs(d2(queries, balls) - r2) <= window(D) * r2


def manifold(real, gen, k):
    """precision, recall, f1, density, coverage of metrics.manifold_metrics as floats."""
    q_gen, m_real = counts(real, radius2(real, k), gen)
    q_real, _ = counts(gen, radius2(gen, k), real)
    p, r = float(np.mean(q_gen > 0)), float(np.mean(q_real > 0))
    return {"precision": p, "recall": r, "f1": 2 * p * r / (p + r) if p + r else float("nan"),
            "density": float(q_gen.sum() / (k * len(gen))), "coverage": float(np.mean(m_real > 0))}
