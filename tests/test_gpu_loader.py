"""GPU tests of the device-resident data path: gmk_batch_gather / ops.batch_gather against the CPU transform chain, data.DeviceDataset against
the host restatement tests/loader_ref.py, and the driver end to end with --data_device 1.  Every comparison is bit-exact."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loader_ref  # noqa: E402

pytestmark = pytest.mark.gpu

N = 37
SEED, OFFSET = (1 << 40) + 12345, 77          # a seed above 2^32 and a nonzero counter; at B = 8 and p = 0.5 this stream flips images 0, 1, 3, 6, 7
INDICES = {1: [N - 1], 5: [N - 1, 0, 17, 0, 3], 8: [N - 1, 0, 5, 5, 20, 1, N - 1, 9]}      # repeated, unsorted, both ends


def _dataset(C, H, W):
    """uint8 [N, C, H, W]: a tiled arange (every byte value, 127 and 128 among them, in every shape), shifted per image so that no two images
    and no image and its mirror are equal."""
    chw = C * H * W
    flat = np.arange(N * chw, dtype=np.int64)
    images = ((flat + 3 * (flat // chw)) % 256).astype(np.uint8).reshape(N, C, H, W)
    assert len(np.unique(images)) == 256 and len({im.tobytes() for im in images}) == N
    return images, ((np.arange(N) * 7 + 3) % 256).astype(np.uint8)


@pytest.mark.parametrize("binarize", [0, 1])
@pytest.mark.parametrize("C,H,W,pad", [(1, 28, 28, 0), (1, 28, 28, 2), (3, 32, 32, 0), (1, 5, 7, 0), (3, 5, 7, 1), (3, 64, 64, 0)])
def test_batch_gather_matches_the_cpu_chain(C, H, W, pad, binarize):
    """(1, 28, 28, 2): source rows 2 bytes off the 16-byte output groups; (1, 5, 7, 0) / (3, 5, 7, 1): C H W % 4 != 0, unaligned image starts, rows
    that are no whole groups (the per-element path and its scalar tail); the others: aligned rows of whole groups, more than one workgroup."""
    from generative_models_amd import ops
    images, labels = _dataset(C, H, W)
    d_images, d_labels = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda()
    for B, idx in INDICES.items():
        d_idx = torch.tensor(idx, dtype=torch.int64, device="cuda")
        for flip_p in (0.0, 1.0, 0.5):
            flips = np.zeros(B, dtype=bool) if flip_p == 0 else loader_ref.philox_ref.label_drop_mask(SEED, OFFSET, B, flip_p)
            if flip_p == 1.0:
                assert flips.all()
            if flip_p == 0.5 and B == 8:
                assert flips.any() and not flips.all()
            want_x, want_y = loader_ref.expected_batch(images, labels, idx, binarize, pad, flips)
            x, y = ops.batch_gather(d_images, d_labels, d_idx, pad=pad, binarize=binarize, flip_p=flip_p, seed=SEED, offset=OFFSET)
            assert x.shape == (B, C, H + 2 * pad, W + 2 * pad) and x.dtype == torch.float32 and y.dtype == torch.int64
            assert torch.equal(y.cpu(), want_y), (B, flip_p)
            assert torch.equal(x.cpu(), want_x), (B, flip_p, int((x.cpu() != want_x).sum()))
            if pad:
                assert float(x[:, :, :pad].abs().max()) == 0.0 and float(x[:, :, :, -pad:].abs().max()) == 0.0      # 0, not -1, for signed data too


def test_wrapper_checks_and_fresh_outputs(monkeypatch):
    from generative_models_amd import ops
    images, labels = _dataset(1, 5, 7)
    d_images, d_labels = torch.from_numpy(images).cuda(), torch.from_numpy(labels).cuda()
    idx = torch.tensor([0, 3, N - 1], dtype=torch.int64, device="cuda")
    kw = dict(pad=0, binarize=0)
    launches = []
    real = ops.lib.gmk_batch_gather
    monkeypatch.setattr(ops.lib, "gmk_batch_gather", lambda *a: launches.append(a) or real(*a))
    for bad in ([0, N], [-1, 2], [N + 5]):
        with pytest.raises(ValueError, match="index"):
            ops.batch_gather(d_images, d_labels, torch.tensor(bad, dtype=torch.int64, device="cuda"), **kw)
    with pytest.raises(ValueError, match="dtype"):
        ops.batch_gather(d_images.float(), d_labels, idx, **kw)
    with pytest.raises(ValueError, match="dtype"):
        ops.batch_gather(d_images, d_labels.long(), idx, **kw)
    with pytest.raises(ValueError, match="dtype"):
        ops.batch_gather(d_images, d_labels, idx.int(), **kw)
    with pytest.raises(ValueError, match="device"):
        ops.batch_gather(d_images.cpu(), d_labels, idx, **kw)
    with pytest.raises(ValueError, match="device"):
        ops.batch_gather(d_images, d_labels, idx.cpu(), **kw)
    with pytest.raises(ValueError, match="N, C, H, W"):
        ops.batch_gather(d_images[:, 0], d_labels, idx, **kw)
    with pytest.raises(ValueError, match="flip_p"):
        ops.batch_gather(d_images, d_labels, idx, flip_p=1.5, **kw)
    with pytest.raises(ValueError, match="unsigned 64-bit"):
        ops.batch_gather(d_images, d_labels, idx, seed=-1, **kw)
    assert launches == []                                       # none of the above reached the library
    x1, y1 = ops.batch_gather(d_images, d_labels, idx, **kw)
    x2, y2 = ops.batch_gather(d_images, d_labels, idx, trusted=True, **kw)
    assert len(launches) == 2
    assert x1.data_ptr() != x2.data_ptr() and y1.data_ptr() != y2.data_ptr()      # fresh tensors: train_step overwrites y in place
    y1.fill_(-1)
    assert torch.equal(x1, x2) and y2.tolist() == labels[[0, 3, N - 1]].tolist()


def _loader(images, labels, **kw):
    from generative_models_amd import data
    return data.DeviceDataset(images, labels, 8, binarize=0, pad=1, device="cuda", **kw)


def _epoch(loader):
    return [(x.cpu(), y.cpu()) for x, y in loader]


def test_device_dataset_follows_the_restatement():
    rng = np.random.default_rng(4)
    n, seed = 50, 1000
    images, labels = rng.integers(0, 256, (n, 5, 7), dtype=np.uint8), np.arange(n)      # an image's label names its index
    ranks = [_loader(images, labels, seed=seed, rank=r, world=2) for r in (0, 1)]
    assert [len(r) for r in ranks] == [3, 3] and ranks[0].images.dtype == torch.uint8 and ranks[0].images.shape == (n, 1, 5, 7)
    seen = {}
    for epoch in (0, 1):
        perm = loader_ref.permutation(n, seed, epoch)
        for r, loader in enumerate(ranks):
            assert loader.epoch == epoch
            got, want = _epoch(loader), loader_ref.shard_batches(perm, r, 2, 8)
            assert len(got) == 3
            for (x, y), idx in zip(got, want):
                assert y.tolist() == idx.tolist()
                assert torch.equal(x, loader_ref.expected_batch(images[:, None], labels, idx, 0, 1, np.zeros(8, dtype=bool))[0])
            seen[epoch, r] = np.concatenate([y.numpy() for _, y in got])
        assert not set(seen[epoch, 0]) & set(seen[epoch, 1]) and len(set(seen[epoch, 0]) | set(seen[epoch, 1])) == 48      # disjoint shards
    assert not np.array_equal(seen[0, 0], seen[1, 0])           # epochs reshuffle
    a = ranks[0]
    a.epoch = 0                                                 # settable: epoch 0 again
    assert np.array_equal(np.concatenate([y.numpy() for _, y in _epoch(a)]), seen[0, 0]) and a.epoch == 1
    for x, y in a:                                              # what train_step does to the labels it is handed
        y.fill_(-1)
    assert a.epoch == 2
    a.epoch = 1
    assert np.array_equal(np.concatenate([y.numpy() for _, y in _epoch(a)]), seen[1, 0])      # the dataset's own labels are intact
    # a deep copy (main._feature_extractors copies the test set) iterates on its own
    a.epoch = 0
    k_before = a._k
    twin = copy.deepcopy(a)
    assert twin.images.data_ptr() != a.images.data_ptr()
    assert np.array_equal(np.concatenate([y.numpy() for _, y in _epoch(twin)]), seen[0, 0])
    assert (a.epoch, a._k) == (0, k_before) and (twin.epoch, twin._k) == (1, k_before + 3)
    assert np.array_equal(np.concatenate([y.numpy() for _, y in _epoch(a)]), seen[0, 0])


def test_device_dataset_flips_by_batch_count():
    rng = np.random.default_rng(5)
    n, seed = 50, 1000
    images, labels = rng.integers(0, 256, (n, 3, 5, 7), dtype=np.uint8), np.arange(n)
    loader = _loader(images, labels, seed=seed, flip_p=0.5)
    assert len(loader) == 6
    k, flipped = 0, 0
    for epoch in (0, 1):                                        # k runs on across epochs
        for (x, y), idx in zip(_epoch(loader), loader_ref.shard_batches(loader_ref.permutation(n, seed, epoch), 0, 1, 8)):
            flips = loader_ref.flip_mask(seed + 1, k, 8, 0.5)
            assert y.tolist() == idx.tolist()
            assert torch.equal(x, loader_ref.expected_batch(images, labels, idx, 0, 1, flips)[0]), k
            k, flipped = k + 1, flipped + int(flips.sum())
    assert k == 12 and 0 < flipped < 96


def _run_driver(argv):
    import yaml
    from generative_models_amd import main
    loaded = main.load_model_and_data(argv)
    model, train_ds, G = loaded[0], loaded[1], loaded[-1]
    final = main.train(*loaded)
    for key in ("diffusion/train/loss", "diffusion/test/loss"):
        assert final[key] and all(np.isfinite(v) for v in final[key]), (key, final[key])
    with open(os.path.join(str(G.logdir), "hps.yaml")) as f:
        hps = yaml.load(f, Loader=yaml.Loader)
    return model, train_ds, hps, final


def test_driver_end_to_end_on_the_device_path(tmp_path):
    from generative_models_amd import data
    rng = np.random.default_rng(6)
    raw = tmp_path / "MNIST" / "raw"
    raw.mkdir(parents=True)
    for train, n in ((True, 64), (False, 16)):
        data.write_idx(raw / data.FILES[train][0], rng.integers(0, 256, (n, 28, 28), dtype=np.uint8))
        data.write_idx(raw / data.FILES[train][1], rng.integers(0, 10, n, dtype=np.uint8))
        split = "train" if train else "test"
        np.save(tmp_path / f"{split}_images.npy", rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8))
        np.save(tmp_path / f"{split}_labels.npy", rng.integers(0, 10, n, dtype=np.int64))
    base = ["--model=diffusion", "--data_device", "1", "--data_root", str(tmp_path), "--bs", "8", "--epochs", "1", "--hidden_size", "32",
            "--timesteps", "4", "--eval_heavy", "0"]
    model, train_ds, hps, final = _run_driver(base + ["--data", "mnist", "--logdir", str(tmp_path / "mnist")])
    assert isinstance(train_ds, data.DeviceDataset) and len(train_ds) == 8 and len(final["diffusion/train/loss"]) == 8
    assert hps["data_device"] == 1 and hps["data"] == "mnist" and hps["flip_p"] == 0.0 and hps["image_size"] == 0 and model.size == 28
    model, train_ds, hps, final = _run_driver(base + ["--data", "npy", "--in_channels", "3", "--image_size", "32", "--binarize", "0",
                                                      "--flip_p", "0.5", "--logdir", str(tmp_path / "npy")])
    assert train_ds.flip_p == 0.5 and train_ds.images.shape == (64, 3, 32, 32) and len(final["diffusion/train/loss"]) == 8
    assert hps["data_device"] == 1 and hps["data"] == "npy" and hps["flip_p"] == 0.5 and hps["image_size"] == 32 and model.size == 32
    assert model.last_eval["samples"].shape == (25, 3, 32, 32)
    with pytest.raises(ValueError, match="image size 32"):
        model.train_step(torch.zeros((8, 3, 28, 28), device="cuda"), torch.zeros((8,), dtype=torch.long, device="cuda"))
