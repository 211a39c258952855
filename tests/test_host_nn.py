"""CPU tests of the nearest-neighbour report: what tests/nn_ref.py (the restatement the GPU tests compare against) claims about itself, the
host arithmetic of neighbours.py against it, and the driver's flag validation.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nn_ref  # noqa: E402


def test_restatement_orders_by_distance_then_index():
    db = np.full((6, 4), 10, dtype=np.uint8)
    db[1] = db[4] = [10, 10, 10, 13]          # identical rows: d2 = 9 to the query below, lowest index first
    db[2] = [12, 11, 12, 10]                  # d2 = 9 through other bytes: sits between them by its index
    db[5] = [10, 10, 10, 11]                  # d2 = 1
    q = np.full((1, 4), 10, dtype=np.uint8)
    d, i = nn_ref.search(q, db, 6)
    assert i.tolist() == [[0, 3, 5, 1, 2, 4]] and d.tolist() == [[0, 0, 1, 9, 9, 9]]
    d, i = nn_ref.search(q, db, 2)
    assert i.tolist() == [[0, 3]] and d.dtype == np.int64 and i.dtype == np.int64
    # the distance is the one of the definition at the ends of the byte range (no wrap-around in uint8)
    ends = np.array([[0, 255], [255, 0]], dtype=np.uint8)
    assert nn_ref.dist2_matrix(ends[:1], ends).tolist() == [[0, 2 * 255 * 255]]
    assert nn_ref.sqnorm(ends).tolist() == [128 * 128 + 127 * 127] * 2


def test_restatement_mirror_rule():
    rng = np.random.default_rng(1)
    train = rng.integers(0, 256, (12, 2, 3, 4), dtype=np.uint8)
    train[5] = train[5][..., ::-1] * 0 + np.array([1, 2, 2, 1], dtype=np.uint8)          # a palindrome along W: both orientations tie on (0, 5)
    q = np.stack([train[3], train[7][..., ::-1], train[5]])
    d, i, m = nn_ref.search_mirror(q, train, 2)
    assert d[:, 0].tolist() == [0, 0, 0] and i[:, 0].tolist() == [3, 7, 5]
    assert m.tolist() == [False, True, False]                                            # the tie goes to the unmirrored orientation
    # the mirrored query's whole list is the mirrored search's
    d1, i1 = nn_ref.search(q[1:2, ..., ::-1], train, 2)
    assert np.array_equal(d[1:2], d1) and np.array_equal(i[1:2], i1)


def test_lower_median_and_host_statistics_agree_with_neighbours():
    from generative_models_amd import neighbours
    assert nn_ref.lower_median([5]) == 5 and nn_ref.lower_median([9, 1]) == 1 and nn_ref.lower_median([3, 1, 2]) == 2
    assert nn_ref.lower_median([4, 1, 3, 2]) == 2
    rng = np.random.default_rng(2)
    for n in (1, 2, 7, 16):
        v = rng.integers(0, 2 ** 31 - 1, n).astype(np.int32)
        assert int(neighbours.lower_median(v)) == nn_ref.lower_median(v)
        assert neighbours.rms_distance(v, 3072) == nn_ref.rms(v, 3072)
    assert nn_ref.rms([3072 * 255 * 255], 3072) == 1.0 and nn_ref.rms([0, 0], 5) == 0.0


def test_nn_closer_is_one_for_planted_copies_and_counts_directly_otherwise():
    rng = np.random.default_rng(3)
    train = rng.integers(0, 256, (40, 1, 6, 6), dtype=np.uint8)
    holdout = rng.integers(0, 256, (9, 1, 6, 6), dtype=np.uint8)
    copies = train[[4, 17, 17, 30, 39]].copy()
    for n, c in enumerate(copies):                       # one byte changed by 1: d2 = 1, far below any held-out image's distance
        v = int(c.reshape(-1)[n])
        c.reshape(-1)[n] = v + 1 if v < 255 else v - 1
    rep = nn_ref.report(train, copies, holdout, 3, mirror=False)
    assert rep["nn_closer"] == 1.0 and rep["dist2"][:, 0].tolist() == [1] * 5 and rep["index"][:, 0].tolist() == [4, 17, 17, 30, 39]
    assert abs(rep["nn_dist"] - np.sqrt(1 / 36) / 255) < 1e-15 and rep["nn_dist"] < rep["nn_dist_test"]
    # the samples are the held-out images themselves: the fraction strictly below their own lower median, counted directly
    rep = nn_ref.report(train, holdout, holdout, 1, mirror=True)
    first = sorted(rep["test_dist2"].tolist())
    assert rep["nn_closer"] == sum(v < first[4] for v in first) / 9 and rep["nn_dist"] == rep["nn_dist_test"]
    assert np.array_equal(rep["dist2"][:, 0], rep["test_dist2"])


def test_driver_flags_are_checked_before_a_model_is_built(tmp_path, monkeypatch):
    from generative_models_amd import common, main
    assert (main.DG.nn_eval, main.DG.nn_k) == (0, 3)
    built = []
    Model = common.discover_models()["diffusion"]
    real = Model.__init__
    monkeypatch.setattr(Model, "__init__", lambda self, G: built.append(1) or real(self, G))
    base = ["--model=diffusion", "--device", "cpu", "--logdir", str(tmp_path), "--hidden_size", "32"]
    device = ["--data_device", "1", "--data", "npy", "--data_root", str(tmp_path)]
    for flags, message in ((["--nn_eval", "4", "--binarize", "0"], "needs --data_device 1"),
                           (["--nn_eval", "4", "--binarize", "1"] + device, "needs --binarize 0"),
                           (["--nn_eval", "4", "--binarize", "0", "--nn_k", "9"] + device, "--nn_k 9: 1 .. 8"),
                           (["--nn_eval", "4", "--binarize", "0", "--nn_k", "0"] + device, "--nn_k 0: 1 .. 8"),
                           (["--nn_eval", "-1"], "--nn_eval -1")):
        with pytest.raises(ValueError, match=message):
            main.load_model_and_data(base + flags)
    assert built == []
    # against the training set's size, once it is known
    G, _ = main.FlagSpace(main.DG).resolve(base + ["--nn_eval", "4", "--binarize", "0", "--nn_k", "5"] + device)
    main._check_nn_flags(G)
    main._check_nn_flags(G, 5)
    with pytest.raises(ValueError, match="the training set has 4 images"):
        main._check_nn_flags(G, 4)
    # off by default: nothing is asked of the other flags
    G, _ = main.FlagSpace(main.DG).resolve(base + ["--nn_k", "99"])
    main._check_nn_flags(G)
    assert main.Session(None, None, None, None, None, G).nn_index is None
