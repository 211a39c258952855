"""GPU tests of the nearest-neighbour search (csrc/nn_search.hip through ops.nn_search_u8 / ops.u8_sqnorm), of neighbours.NeighbourIndex and
nn_report through it, and of the driver's --nn_eval report, against the numpy restatement tests/nn_ref.py.  Every comparison is bit-exact:
distances and indices with torch.equal / np.array_equal."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_ref  # noqa: E402
import nn_ref  # noqa: E402
import png_ref  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from generative_models_amd import ops as o
    return o


def _slab():
    from generative_models_amd import ops as o
    return o.NN_SLAB


def _check(ops, q, db, k):
    d2, idx = ops.nn_search_u8(torch.from_numpy(q).cuda(), torch.from_numpy(db).cuda(), k)
    want_d2, want_idx = nn_ref.search(q, db, k)
    assert d2.dtype == torch.int32 and idx.dtype == torch.int64 and tuple(d2.shape) == tuple(idx.shape) == (len(q), k)
    assert torch.equal(idx.cpu(), torch.from_numpy(want_idx)), (idx.cpu()[:4], want_idx[:4])
    assert torch.equal(d2.cpu().long(), torch.from_numpy(want_d2))
    return d2, idx


# (Q, N, D, k).  (1, 1, 1, 1) the smallest; (3, 5, 16, 5) k = N; (17, 70, 48, 3) a partial query tile, D below one 64-byte K-step; (33, 257, 64, 8)
# three slabs, one row in the last; (5, 300, 105, 4) D % 16 != 0: the per-byte staging path; (16, 1100, 784, 3) MNIST rows, 12 K-steps and a
# 16-byte tail; (8, 600, 3072, 8) CIFAR rows; slab - 1 and slab + 1 rows; (130, 3 slabs + 7, 80, 5) four slabs and two query tiles, so that the merge
# launch merges and the query loop loops.
def _cases():
    s = _slab()
    return [(1, 1, 1, 1), (3, 5, 16, 5), (17, 70, 48, 3), (33, 257, 64, 8), (5, 300, 105, 4), (16, 1100, 784, 3), (8, 600, 3072, 8),
            (4, s - 1, 32, 2), (4, s + 1, 32, 2), (130, 3 * s + 7, 80, 5)]


@pytest.mark.parametrize("case", range(10))
def test_search_matches_the_brute_force(ops, case):
    Q, N, D, k = _cases()[case]
    db = nn_ref.random_rows(N, D, seed=100 + case)
    q = nn_ref.random_rows(Q, D, seed=200 + case)
    if Q > 2 and N > 2:
        q[1] = db[N // 2]                                    # a query that is a database row
    d2, idx = _check(ops, q, db, k)
    if Q > 2 and N > 2:
        assert int(d2[1, 0]) == 0 and int(idx[1, 0]) <= N // 2 and np.array_equal(db[int(idx[1, 0])], db[N // 2])


def test_ties_resolve_to_the_lower_index(ops):
    """Rows 3, 40 and 41 are identical, row 7 lies at the same distance from the query through other bytes: the order is (d2, j) lexicographic."""
    rng = np.random.default_rng(5)
    db = rng.integers(100, 156, (50, 16), dtype=np.uint8)
    base = rng.integers(10, 20, 16).astype(np.uint8)
    db[3] = db[40] = db[41] = base
    q = base[None].copy()
    q[0, 0] += 2                                             # d2 = 4 to the three copies
    db[7] = q[0]
    db[7, 1:5] += 1                                          # d2 = 4 through four other bytes
    db[20] = q[0]                                            # and the query itself is a database row: d2 = 0 at that row
    d2, idx = _check(ops, q, db, 6)
    assert idx[0, :5].tolist() == [20, 3, 7, 40, 41] and d2[0, :5].tolist() == [0, 4, 4, 4, 4]


def test_the_largest_distance_and_the_range_checks(ops):
    D = ops.NN_MAX_D
    assert D == 32768 and ops.NN_MAX_K == 8
    q = torch.zeros((1, D), dtype=torch.uint8, device="cuda")
    db = torch.full((3, D), 255, dtype=torch.uint8, device="cuda")
    d2, idx = ops.nn_search_u8(q, db, 2)
    assert d2.tolist() == [[2130739200, 2130739200]] and idx.tolist() == [[0, 1]]
    d2, idx = ops.nn_search_u8(db[:1], q, 1)
    assert d2.tolist() == [[2130739200]] and idx.tolist() == [[0]]
    wide = torch.zeros((2, D + 1), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="D = 32769"):
        ops.nn_search_u8(wide, wide, 1)
    with pytest.raises(ValueError, match="D = 32769"):
        ops.u8_sqnorm(wide)
    small = torch.zeros((10, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="k = 9"):
        ops.nn_search_u8(small, small, 9)
    with pytest.raises(ValueError, match="k = 4 with N = 3"):
        ops.nn_search_u8(small, small[:3], 4)
    with pytest.raises(ValueError, match="k = 0"):
        ops.nn_search_u8(small, small, 0)
    with pytest.raises(ValueError, match="D = 16 bytes, database rows of D = 8"):
        ops.nn_search_u8(small, small[:, :8], 1)
    with pytest.raises(ValueError, match="dtype"):
        ops.nn_search_u8(small.float(), small, 1)
    # the C entry holds the same ranges, with the values in its message
    from generative_models_amd._lib import GmkError, lib
    out = torch.empty((10, 8), dtype=torch.int32, device="cuda")
    norms = ops.u8_sqnorm(small)
    ws = torch.empty((1 << 16,), dtype=torch.uint8, device="cuda")
    for D_, k_, text in ((32769, 1, "D = 32769"), (16, 9, "k = 9"), (16, 0, "k = 0")):
        rc = lib.gmk_nn_search_u8(small.data_ptr(), 10, small.data_ptr(), 10, D_, norms.data_ptr(), k_, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                  out.data_ptr(), 0)
        assert rc == -1 and text in lib.gmk_last_error().decode()
    rc = lib.gmk_nn_search_u8(small.data_ptr(), 10, small.data_ptr(), 3, 16, norms.data_ptr(), 4, ws.data_ptr(), ws.numel(), out.data_ptr(),
                              out.data_ptr(), 0)
    assert rc == -1 and "k = 4 with N = 3" in lib.gmk_last_error().decode()
    assert lib.gmk_nn_search_workspace(10, 10, 9) == -1 and lib.gmk_nn_search_workspace(10, 10, 8) == 16 * 3 + 10 * 2 * 8 * 8
    rc = lib.gmk_nn_search_u8(small.data_ptr(), 10, small.data_ptr(), 10, 16, norms.data_ptr(), 8, ws.data_ptr(), 100, out.data_ptr(), out.data_ptr(), 0)
    assert rc == -1 and "workspace of 100 bytes" in lib.gmk_last_error().decode() and GmkError is not None


def test_structured_rows_pin_the_operand_maps(ops):
    """Byte i of database row j is (7 i + 13 j) mod 251, of query q (5 i + 29 q + 3) mod 251: asymmetric in the row, the query and the byte
    index, over one and a half K-steps and both halves of every MFMA's K - rows, queries or K groups swapped or permuted between the two
    operands give other distances."""
    db = nn_ref.structured_rows(200, 96, 7, 13)
    q = nn_ref.structured_rows(40, 96, 5, 29, 3)
    _check(ops, q, db, 4)


def test_two_calls_give_the_same_bytes_and_views_give_their_clones_results(ops):
    N, D, Q, k = 300, 48, 21, 5
    db = torch.from_numpy(nn_ref.random_rows(N, D, seed=11)).cuda()
    q = torch.from_numpy(nn_ref.random_rows(Q, D, seed=12)).cuda()
    first, again = ops.nn_search_u8(q, db, k), ops.nn_search_u8(q, db, k)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    want = nn_ref.search(q.cpu().numpy(), db.cpu().numpy(), k)
    assert torch.equal(first[1].cpu(), torch.from_numpy(want[1]))
    # a database that starts one byte off alignment (contiguous rows, the per-byte path)
    buf = torch.empty((N * D + 1,), dtype=torch.uint8, device="cuda")
    off = buf[1:].view(N, D)
    off.copy_(db)
    assert off.data_ptr() % 16 == 1 and off.is_contiguous()
    got = ops.nn_search_u8(q, off, k)
    assert torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])
    # a non-contiguous query view, a higher-rank database, norms passed in
    wide = torch.zeros((Q, 2 * D), dtype=torch.uint8, device="cuda")
    wide[:, ::2] = q
    got = ops.nn_search_u8(wide[:, ::2], db.view(N, 3, 4, 4), k, db_sqnorm=ops.u8_sqnorm(db))
    assert not wide[:, ::2].is_contiguous() and torch.equal(got[0], first[0]) and torch.equal(got[1], first[1])


def test_query_blocks_under_the_workspace_cap(ops, monkeypatch):
    """A cap that makes nn_search_u8 take its queries in several blocks (16 at a time, then the rest): the rows of one call."""
    N, D, Q, k = 2 * _slab() + 3, 32, 45, 3
    db = nn_ref.random_rows(N, D, seed=21)
    q = nn_ref.random_rows(Q, D, seed=22)
    per_query = 2 * 3 * k * 8
    monkeypatch.setattr(ops, "NN_WORKSPACE_CAP", 20 * per_query)
    _check(ops, q, db, k)


@pytest.mark.parametrize("D", [1, 105, 784, 32768])
def test_sqnorm_matches_numpy(ops, D):
    rows = nn_ref.random_rows(9, D, seed=D)
    got = ops.u8_sqnorm(torch.from_numpy(rows).cuda())
    assert got.dtype == torch.int32 and torch.equal(got.cpu().long(), torch.from_numpy(nn_ref.sqnorm(rows)))
    off = torch.empty((9 * D + 3,), dtype=torch.uint8, device="cuda")[3:].view(9, D)
    off.copy_(torch.from_numpy(rows))
    assert torch.equal(ops.u8_sqnorm(off), got)


def test_index_mirror_search_and_report(ops):
    from generative_models_amd import neighbours
    rng = np.random.default_rng(31)
    train = rng.integers(0, 256, (64, 3, 8, 8), dtype=np.uint8)
    q = rng.integers(0, 256, (16, 3, 8, 8), dtype=np.uint8)
    planted = [5, 63, 0, 17, 17, 40, 33, 8]
    for n, j in enumerate(planted):
        q[2 * n] = train[j][..., ::-1]                       # every other query: a mirrored copy of a training image
    holdout = rng.integers(0, 256, (16, 3, 8, 8), dtype=np.uint8)
    holdout[3] = train[9]
    index = neighbours.NeighbourIndex(torch.from_numpy(train).cuda())
    assert len(index) == 64 and index.D == 192 and torch.equal(index.sqnorm.cpu().long(), torch.from_numpy(nn_ref.sqnorm(train)))
    d2, idx, mirrored = index.search(torch.from_numpy(q).cuda(), 3, mirror=True)
    want = nn_ref.search_mirror(q, train, 3)
    assert np.array_equal(d2.cpu().numpy(), want[0]) and np.array_equal(idx.cpu().numpy(), want[1]) and np.array_equal(mirrored.cpu().numpy(), want[2])
    assert mirrored[::2].all() and d2[::2, 0].tolist() == [0] * 8 and idx[::2, 0].tolist() == planted and not mirrored[1::2].all()
    plain = index.search(torch.from_numpy(q).cuda(), 3)
    assert not plain[2].any() and np.array_equal(plain[1].cpu().numpy(), nn_ref.search(q, train, 3)[1])
    for mirror in (False, True):
        got = neighbours.nn_report(index, torch.from_numpy(q).cuda(), torch.from_numpy(holdout).cuda(), 3, mirror)
        ref = nn_ref.report(train, q, holdout, 3, mirror)
        assert set(got) == set(ref)
        for key in ("nn_dist", "nn_dist_test", "nn_closer"):
            assert got[key] == ref[key], (key, got[key], ref[key])
        for key in ("index", "dist2", "mirrored", "test_dist2"):
            assert np.array_equal(got[key], ref[key]), key
    with pytest.raises(ValueError, match="images of"):
        index.search(torch.from_numpy(q[:, :1]).cuda(), 1)


def test_driver_writes_the_neighbour_report(tmp_path):
    from generative_models_amd import main
    rng = np.random.default_rng(41)
    root = tmp_path / "set"
    root.mkdir()
    sets = {}
    for split, n in (("train", 64), ("test", 16)):
        sets[split] = rng.integers(0, 256, (n, 1, 8, 8), dtype=np.uint8)
        np.save(root / f"{split}_images.npy", sets[split])
        np.save(root / f"{split}_labels.npy", rng.integers(0, 10, n, dtype=np.int64))
    logdir = tmp_path / "run"
    flags = ["--model=diffusion", "--data_root", str(root), "--in_channels", "1", "--image_size", "8", "--eval_heavy", "0", "--logdir", str(logdir),
             "--hidden_size", "32", "--bs", "8", "--timesteps", "2", "--epochs", "0", "--data", "npy", "--data_device", "1", "--binarize", "0",
             "--nn_eval", "16", "--nn_k", "3", "--save_images", "1"]
    # more neighbours than training images: named once the data is loaded
    tiny = tmp_path / "tiny"
    tiny.mkdir()
    for split in ("train", "test"):
        np.save(tiny / f"{split}_images.npy", sets["test"][:4])
        np.save(tiny / f"{split}_labels.npy", np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError, match="the training set has 4 images"):
        main.load_model_and_data(["--model=diffusion", "--data_root", str(tiny), "--in_channels", "1", "--image_size", "8", "--logdir", str(logdir),
                                  "--hidden_size", "32", "--bs", "2", "--timesteps", "2", "--data", "npy", "--data_device", "1", "--binarize", "0",
                                  "--nn_eval", "4", "--nn_k", "5"])
    loaded = main.load_model_and_data(flags)
    session = main.Session(*loaded)
    final = session.run()
    got = np.load(logdir / "nearest_neighbours.npz")
    assert sorted(got.files) == ["dist2", "epoch", "index", "mirrored", "samples", "test_dist2"]
    samples = got["samples"]
    assert samples.shape == (16, 1, 8, 8) and samples.dtype == np.uint8 and int(got["epoch"]) == 0
    assert got["index"].shape == (16, 3) and got["dist2"].shape == (16, 3) and got["mirrored"].shape == (16,) and got["test_dist2"].shape == (16,)
    ref = nn_ref.report(sets["train"], samples, sets["test"], 3, mirror=False)
    assert np.array_equal(got["index"], ref["index"]) and np.array_equal(got["dist2"], ref["dist2"]) and not got["mirrored"].any()
    assert np.array_equal(got["test_dist2"], ref["test_dist2"])
    for key in ("nn_dist", "nn_dist_test", "nn_closer"):
        assert final[f"eval/{key}"] == ref[key], (key, final[f"eval/{key}"], ref[key])
    assert final["dt/nn_eval"] > 0 and session.nn_index is not None and len(session.nn_index) == 64
    # the picture: the first 10 samples, each followed by its 3 neighbours as the dataset stores them
    picture = png_ref.decode((logdir / "images" / "nearest_0000.png").read_bytes())["frames"]
    assert picture.shape == (1, 2 + 10 * (8 + 2), 2 + 4 * (8 + 2), 1)
    tiles = np.concatenate((samples[:10, None], sets["train"][ref["index"][:10]]), 1).reshape(1, 40, 1, 8, 8)
    lines = image_ref.grid(tiles, ncol=4, gap=2, fill=0, out_channels=1, row_prefix=0)
    assert np.array_equal(picture, lines.reshape(1, lines.shape[1], -1, 1))
