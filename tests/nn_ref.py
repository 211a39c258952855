"""Host restatement of the nearest-neighbour search and report (generative_models_amd/neighbours.py, include/gmk.h: gmk_nn_search_u8) in numpy
int64: brute force, the (d2, j) ordering, the mirror rule and nn_report's three statistics.  Nothing here is shared with the code under test."""
import numpy as np


def sqnorm(rows):
    """sum_i (rows[j][i] - 128)^2, int64 [N]"""
    r = np.asarray(rows).reshape(len(rows), -1).astype(np.int64) - 128
    return (r * r).sum(1)


def dist2_matrix(queries, database):
    """int64 [Q, N] of sum_i (q_i - x_i)^2, by differences (not by the norm expansion the kernel uses)"""
    q = np.asarray(queries).reshape(len(queries), -1).astype(np.int64)
    x = np.asarray(database).reshape(len(database), -1).astype(np.int64)
    assert q.shape[1] == x.shape[1]
    out = np.empty((q.shape[0], x.shape[0]), dtype=np.int64)
    for i in range(q.shape[0]):          # a row at a time: [N, D] int64 temporaries, not [Q, N, D]
        d = x - q[i]
        out[i] = (d * d).sum(1)
    return out


def search(queries, database, k):
    """-> (dist2 int64 [Q, k], index int64 [Q, k]): per query the k smallest pairs (d2, j) in lexicographic order"""
    d = dist2_matrix(queries, database)
    assert 1 <= k <= d.shape[1]
    index = np.argsort(d, axis=1, kind="stable")[:, :k]          # stable: equal distances stay in index order
    return np.take_along_axis(d, index, 1), index.astype(np.int64)


def search_mirror(queries, database, k):
    """queries [Q, ..., W]: also searched flipped along W; per query the orientation with the smaller first pair (d2, j) wins, the unmirrored
    one on a tie -> (dist2, index, mirrored bool [Q])"""
    q = np.asarray(queries)
    d0, i0 = search(q, database, k)
    d1, i1 = search(q[..., ::-1], database, k)
    mirrored = np.array([(d1[n, 0], i1[n, 0]) < (d0[n, 0], i0[n, 0]) for n in range(len(q))], dtype=bool)
    return np.where(mirrored[:, None], d1, d0), np.where(mirrored[:, None], i1, i0), mirrored


def lower_median(values):
    v = sorted(int(x) for x in np.asarray(values).reshape(-1))
    return v[(len(v) - 1) // 2]


def rms(dist2_first, D):
    return float(np.mean(np.sqrt(np.asarray(dist2_first, dtype=np.float64) / D) / 255.0))


def report(train, samples, holdout, k, mirror):
    """nn_report's dict from the three image arrays (uint8 [n, ..., W])"""
    D = int(np.prod(np.asarray(train).shape[1:]))
    find = search_mirror if mirror else (lambda q, x, kk: search(q, x, kk) + (np.zeros(len(q), dtype=bool),))
    d, idx, mirrored = find(samples, train, k)
    dt, _, _ = find(holdout, train, 1)
    med = lower_median(dt[:, 0])
    return {"nn_dist": rms(d[:, 0], D), "nn_dist_test": rms(dt[:, 0], D), "nn_closer": sum(int(v) < med for v in d[:, 0]) / len(d),
            "index": idx, "dist2": d, "mirrored": mirrored, "test_dist2": dt[:, 0]}


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------------
def random_rows(n, D, seed):
    """random bytes; when there is room, rows of all 0, all 255 and 127 / 128 alternating (the last two straddle the sign flip b ^ 0x80)"""
    rows = np.random.default_rng(seed).integers(0, 256, (n, D), dtype=np.uint8)
    specials = [np.zeros(D), np.full(D, 255), np.where(np.arange(D) % 2 == 0, 127, 128)]
    for s, r in zip(specials, range(n - 1, 0, -2)):          # from the last row backwards, every other one; row 0 stays random
        rows[r] = s
    return rows


def structured_rows(n, D, a, b, c=0):
    """row j, byte i = (a i + b j + c) mod 251: no symmetry in i or j, and no period that a tile size could hide"""
    i, j = np.arange(D, dtype=np.int64)[None, :], np.arange(n, dtype=np.int64)[:, None]
    return ((a * i + b * j + c) % 251).astype(np.uint8)
