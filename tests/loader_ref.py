"""Host restatement (NumPy + tests/philox_ref.py + the CPU transform chain, no GPU import) of data.DeviceDataset: the per-epoch permutation,
the per-rank batches, the flip draws and one assembled batch.  tests/test_host_loader.py checks the restatement's own properties;
tests/test_gpu_loader.py checks the device path against it, bit for bit."""
import numpy as np
import torch

import philox_ref


def keys(N, seed, epoch):
    """float32 [N]: the sort keys of epoch `epoch`, rng_uniform((N,), seed, epoch * ((N + 3) // 4))."""
    return philox_ref.uniform(seed, epoch * ((N + 3) // 4), N)


def permutation(N, seed, epoch, keys_fn=keys):
    """int64 [N]: the STABLE argsort of the keys (equal keys keep their index order)."""
    return np.argsort(keys_fn(N, seed, epoch), kind="stable").astype(np.int64)


def shard_batches(perm, rank, world, bs):
    """-> the list of index arrays this rank yields: perm[rank::world] in slices of bs, the last partial one dropped, (N // world) // bs of them."""
    mine = perm[rank::world]
    return [mine[i * bs:(i + 1) * bs] for i in range((len(perm) // world) // bs)]


def flip_mask(seed, k, bs, p):
    """bool [bs]: the images of the k-th yielded batch that are mirrored; `seed` is the FLIP stream's seed (the loader's seed + 1)."""
    if p <= 0:
        return np.zeros(bs, dtype=bool)
    return philox_ref.label_drop_mask(seed, k * ((bs + 3) // 4), bs, p)


def expected_batch(images, labels, idx, binarize, pad, flips):
    """-> (x float32 [B, C, H + 2 pad, W + 2 pad], y int64 [B]) on the CPU.  images: uint8 [N, C, H, W]; flips: bool [B].  data.transform (the
    reference's chain) on the gathered images, torch.flip along W on the flagged ones, then the zero border."""
    from generative_models_amd import data
    images, idx = np.asarray(images), np.asarray(idx)
    sel = images[idx]
    B, C, H, W = sel.shape
    x = data.transform(sel.reshape(B * C, H, W), bool(binarize), False).reshape(B, C, H, W)
    flips = torch.from_numpy(np.asarray(flips, dtype=bool))
    x = torch.where(flips[:, None, None, None], torch.flip(x, dims=(3,)), x)
    if pad:
        x = torch.nn.functional.pad(x, (pad, pad, pad, pad))
    return x.contiguous(), torch.from_numpy(np.asarray(labels)[idx].astype(np.int64))
