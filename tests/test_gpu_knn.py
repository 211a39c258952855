"""GPU tests of the k-NN radius and ball-count kernels (csrc/knn_f32.hip through ops.knn_radius2 / ops.ball_counts) against the numpy float64
restatement tests/knn_ref.py.  Integer-valued rows in [-4, 4] make every squared distance an exact fp32 integer (at most 64 D = 65,536 at
D = 1024): those comparisons are np.array_equal.  Gaussian rows are held to the fma chain's own error bound, knn_ref.window."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from generative_models_amd import ops as o
    return o


def _consts():
    from generative_models_amd import ops as o
    return o.KNN_TILE, o.NN_MAX_K


def _int_rows(n, D, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=(n, D)).astype(np.float32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _radius(ops, pts, k):
    r2 = ops.knn_radius2(_dev(pts), k)
    assert r2.dtype == torch.float32 and tuple(r2.shape) == (len(pts),)
    return r2.cpu().numpy()


def _counts(ops, balls, r2, queries, **kw):
    q, m = ops.ball_counts(_dev(balls), _dev(np.asarray(r2, dtype=np.float32)), _dev(queries), **kw)
    return (None if q is None else q.cpu().numpy()), (None if m is None else m.cpu().numpy())


# (N, D, k): the smallest; k + 1 == N at the largest k; a tile less and more than one row; four tiles both ways with D % 4 != 0 (the scalar staging
# path); five tiles at D = 256 (four chunks of D); D = 1024 (sixteen chunks); two slabs of columns (the merge launch merges)
def _cases():
    T, K = _consts()
    return [(2, 1, 1), (K + 1, 3, K), (T - 1, 32, 3), (T + 1, 32, 3), (3 * T + 7, 65, 3), (300, 256, 5), (257, 1024, 2), (1024 + 70, 8, 3)]


@pytest.mark.parametrize("case", range(8))
def test_integer_rows_are_exact(ops, case):
    N, D, k = _cases()[case]
    pts, queries = _int_rows(N, D, 300 + case), _int_rows(N, D, 400 + case)
    want_r2 = knn_ref.radius2(pts, k)
    r2 = _radius(ops, pts, k)
    assert np.array_equal(r2.astype(np.float64), want_r2)
    for q_set in (queries, pts):
        q_count, m_count = _counts(ops, pts, r2, q_set)
        want_q, want_m = knn_ref.counts(pts, want_r2, q_set)
        assert q_count.dtype == np.int32 and np.array_equal(q_count, want_q) and np.array_equal(m_count, want_m)


@pytest.mark.parametrize("M,Q", [(130, 1), (1, 130), (67, 133), (1030, 63)])
def test_rectangular_counts(ops, M, Q):
    balls, queries = _int_rows(M, 16, 11), _int_rows(Q, 16, 12)
    r2 = np.random.default_rng(13).integers(0, 200, size=M).astype(np.float32)          # any radii: d2 is around 16 * 13
    q_count, m_count = _counts(ops, balls, r2, queries)
    want_q, want_m = knn_ref.counts(balls, r2, queries)
    assert np.array_equal(q_count, want_q) and np.array_equal(m_count, want_m)
    only_m = _counts(ops, balls, r2, queries, want_q=False)
    only_q = _counts(ops, balls, r2, queries, want_m=False)
    assert only_m[0] is None and np.array_equal(only_m[1], want_m) and only_q[1] is None and np.array_equal(only_q[0], want_q)


def test_identical_rows(ops):
    pts = _int_rows(100, 24, 21)
    pts[17] = pts[63] = pts[3]
    for k in (1, 2, 3):
        r2 = _radius(ops, pts, k)
        assert np.array_equal(r2.astype(np.float64), knn_ref.radius2(pts, k))
        assert (r2[[3, 17, 63]] == 0).all() == (k <= 2)
        _, m_count = _counts(ops, pts, r2, pts)
        assert np.array_equal(m_count, knn_ref.counts(pts, r2, pts)[1])
        if k <= 2:
            assert (m_count[[3, 17, 63]] == 0).all()                          # a ball of radius 0 holds nothing, its own centre included


def test_rows_off_a_16_byte_boundary(ops):
    N, D, k = 150, 32, 3
    pts, queries = _int_rows(N, D, 31), _int_rows(N + 9, D, 32)

    def shifted(a):
        flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
        assert flat.data_ptr() % 16 == 0
        view = flat[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view

    r2 = ops.knn_radius2(shifted(pts), k)
    assert np.array_equal(r2.cpu().numpy().astype(np.float64), knn_ref.radius2(pts, k))
    want_q, want_m = knn_ref.counts(pts, r2.cpu().numpy(), queries)
    for b, q in ((shifted(pts), _dev(queries)), (_dev(pts), shifted(queries)), (shifted(pts), shifted(queries))):
        q_count, m_count = ops.ball_counts(b, r2, q)
        assert np.array_equal(q_count.cpu().numpy(), want_q) and np.array_equal(m_count.cpu().numpy(), want_m)


@pytest.fixture(scope="module")
def gaussian_pairs():
    rng = np.random.default_rng(0)
    pairs = []
    for (a, b) in (((1024, 64), (1000, 64)), ((517, 64), (333, 64))):
        A = rng.standard_normal(a).astype(np.float32)
        B = (0.9 * rng.standard_normal(b) + 0.1).astype(np.float32)
        pairs.append((A, B))
    return pairs


@pytest.mark.parametrize("pair", [0, 1])
def test_gaussian_rows_within_the_fma_bound(ops, gaussian_pairs, pair):
    """A = the balls (k = 3), B = the queries.  The float64 reference sees the same fp32 inputs."""
    A, B = gaussian_pairs[pair]
    D, k = A.shape[1], 3
    want_r2 = knn_ref.radius2(A, k)
    amb = knn_ref.ambiguous(A, want_r2, B, D)                                 # [Q, M]
    amb_q, amb_m = amb.any(1), amb.any(0)
    print("ambiguous queries", amb_q.mean(), "ambiguous balls", amb_m.mean())
    assert amb_q.mean() <= 0.02 and amb_m.mean() <= 0.02                      # from float64 alone
    r2 = _radius(ops, A, k)
    print("r2 max rel err", np.max(np.abs(r2 - want_r2) / want_r2))
    assert np.allclose(r2, want_r2, rtol=(D + 2) * 2.0 ** -24, atol=0.0)
    # every decision: one launch per ball gives the column of that ball
    want_in = knn_ref.inside(A, want_r2, B)
    r2_dev, A_dev, B_dev = _dev(r2), _dev(A), _dev(B)
    got_in = torch.stack([ops.ball_counts(A_dev[j:j + 1], r2_dev[j:j + 1], B_dev, want_m=False)[0] for j in range(len(A))], 1).cpu().numpy()
    assert set(np.unique(got_in)) <= {0, 1}
    assert np.array_equal(got_in.astype(bool)[~amb], want_in[~amb])
    # the counts of one launch over everything are those decisions summed
    q_count, m_count = _counts(ops, A, r2, B)
    assert np.array_equal(q_count, got_in.sum(1)) and np.array_equal(m_count, got_in.sum(0))
    want_q, want_m = want_in.sum(1), want_in.sum(0)
    assert np.array_equal(q_count[~amb_q], want_q[~amb_q]) and np.array_equal(m_count[~amb_m], want_m[~amb_m])
    assert np.mean(q_count[~amb_q] > 0) == np.mean(want_q[~amb_q] > 0)                                   # precision
    assert np.mean(m_count[~amb_m] > 0) == np.mean(want_m[~amb_m] > 0)                                   # coverage
    assert q_count[~amb_q].sum() / (k * (~amb_q).sum()) == want_q[~amb_q].sum() / (k * (~amb_q).sum())   # density


@pytest.mark.parametrize("pair", [0, 1])
def test_both_kernels_round_a_pair_alike(ops, gaussian_pairs, pair):
    """The ball of a point's own (k + 1)-th smallest distance holds, strictly inside, at most k points of its set, and exactly k where the
    k-th and (k + 1)-th values are apart: a count above k means the two kernels rounded one pair differently."""
    for pts in gaussian_pairs[pair]:
        D = pts.shape[1]
        dev = _dev(pts)
        ordered = np.sort(knn_ref.d2(pts, pts), axis=1)
        for k in (1, 3, 8):
            r2 = ops.knn_radius2(dev, k)
            _, m_count = ops.ball_counts(dev, r2, dev)
            m_count = m_count.cpu().numpy()
            assert m_count.max() <= k
            apart = ordered[:, k] - ordered[:, k - 1] > knn_ref.window(D) * ordered[:, k]
            assert apart.mean() > 0.9 and (m_count[apart] == k).all()


def test_launch_shape_and_determinism(ops, gaussian_pairs):
    A, B = (_dev(t) for t in gaussian_pairs[0])
    wide = _dev(np.random.default_rng(5).standard_normal((1100, 130)).astype(np.float32))

    def run():
        r2 = ops.knn_radius2(A, 3)
        return (r2, ops.knn_radius2(wide, 5)) + ops.ball_counts(A, r2, B)

    first, again = run(), run()
    assert all(torch.equal(x, y) for x, y in zip(first, again))
    before = ops.get_cu_limit()
    try:
        for limit in (8, 64, 200):
            ops.set_cu_limit(limit)
            assert all(torch.equal(x, y) for x, y in zip(first, run())), limit
    finally:
        ops.set_cu_limit(before)


def test_argument_errors(ops):
    from generative_models_amd._lib import C, GmkError, lib
    pts = _dev(_int_rows(10, 16, 1))
    out = torch.empty(10, dtype=torch.float32, device="cuda")
    ws = torch.empty(1 << 12, dtype=torch.float32, device="cuda")
    cnt = torch.empty(10, dtype=torch.int32, device="cuda")
    K = ops.NN_MAX_K
    assert lib.gmk_knn_radius_workspace(10, 3) == 4 * 10 * 4 and lib.gmk_knn_radius_workspace(2000, 8) == 2 * 9 * 2000 * 4
    for N_, k_ in ((10, 0), (10, K + 1), (3, 3), (0, 1), (1 << 31, 3)):
        assert lib.gmk_knn_radius_workspace(N_, k_) == -1
    for N_, D_, k_, bytes_ in ((10, 16, 0, ws.numel() * 4), (3, 16, 3, ws.numel() * 4), (10, 0, 3, ws.numel() * 4), (10, 16, 3, 4 * 10 * 4 - 4),
                               (10, 16, K + 1, ws.numel() * 4), (10, ops.KNN_MAX_D + 1, 3, ws.numel() * 4)):
        rc = lib.gmk_knn_radius_f32(pts.data_ptr(), N_, D_, k_, ws.data_ptr(), bytes_, out.data_ptr(), 0)
        assert rc == C["GMK_ERR_ARG"], (N_, D_, k_, bytes_)
    assert lib.gmk_ball_counts_f32(pts.data_ptr(), out.data_ptr(), 10, pts.data_ptr(), 10, 0, cnt.data_ptr(), cnt.data_ptr(), 0) == C["GMK_ERR_ARG"]
    assert lib.gmk_ball_counts_f32(pts.data_ptr(), out.data_ptr(), 0, pts.data_ptr(), 10, 16, cnt.data_ptr(), cnt.data_ptr(), 0) == C["GMK_ERR_ARG"]
    assert lib.gmk_ball_counts_f32(pts.data_ptr(), None, 10, pts.data_ptr(), 10, 16, cnt.data_ptr(), cnt.data_ptr(), 0) == C["GMK_ERR_ARG"]
    for bad in (lambda: ops.knn_radius2(pts, 0), lambda: ops.knn_radius2(pts[:3], 3), lambda: ops.knn_radius2(pts, K + 1),
                lambda: ops.knn_radius2(pts[:, :0], 3), lambda: ops.knn_radius2(pts.double(), 3), lambda: ops.knn_radius2(pts.cpu(), 3),
                lambda: ops.ball_counts(pts, out[:9], pts), lambda: ops.ball_counts(pts, out, pts[:, :8]),
                lambda: ops.ball_counts(pts, out.double(), pts)):
        with pytest.raises((ValueError, GmkError)):
            bad()
