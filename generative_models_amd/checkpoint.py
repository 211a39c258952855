"""Resumable training (an extension: the reference saves `model.pt`, the weights alone, and a stopped run can only be restarted).

`save(dir, model, train_ds, test_ds, epoch)` writes `<dir>/train_state.pt` beside `model.pt`; `load(dir, model, train_ds, test_ds)` puts it
back and returns the epoch.  Together with the weights that is everything the train step and the loaders read: a run stopped at a checkpoint
and resumed reaches the same bits as the run that never stopped (tests/test_gpu_resume.py).  The file, a `torch.save` of plain values:

    version      FORMAT_VERSION
    epoch        the state is "after evaluate(epoch) and checkpoint(epoch)": a resumed run continues with train_epoch
    world        the world size that wrote it (the data shards of another one differ: refused)
    model        model.train_state(): Adam's moments (fp32 arenas, None before the first step), step count, skipped-step count and ema_seeded; the
                 (seed, counter) pairs of the Philox streams; the dropout counter; the arena digests
    train_data   the loaders' state_dict(): a generator state (MnistLoader), counter + host generator (SyntheticMNIST), epoch + k (DeviceDataset)
    test_data
    digests      the model's arena digests again, at the top level, for tools that only compare

One file serves every rank: the streams are seeded per rank (the seed is rebuilt from the flags and checked) and the moments are replicas.

The ARENA DIGEST is a 64-bit sum of splitmix64-mixed (word, position) pairs over a buffer's 4-byte words (include/gmk.h, gmk_arena_digest; on
the device ops.arena_digest, here `digest_host` in numpy for files looked at without a GPU).  It ties model.pt to train_state.pt - a pair from
two different checkpoints is refused - and lets data-parallel replicas be compared without moving an arena (`parallel.check_replicas`)."""
import os
from pathlib import Path

import numpy as np
import torch

from . import parallel

FORMAT_VERSION = 1
FILE = "train_state.pt"

_MASK = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_CHUNK = 1 << 20


def digest_host(array):
    """gmk_arena_digest on the host: sum_i mix(w_i + (i + 1) * 0x9E3779B97F4A7C15) mod 2^64 over the 4-byte little-endian words w_i of the
    array's bytes (a numpy array or a CPU tensor, contiguous or not: its elements in C order), mix = splitmix64's finaliser.  -> unsigned int"""
    if isinstance(array, torch.Tensor):
        array = array.detach().cpu().contiguous().reshape(-1).view(torch.uint8).numpy()
    raw = np.ascontiguousarray(array).reshape(-1).view(np.uint8)
    if raw.size == 0 or raw.size % 4:
        raise ValueError(f"digest of {raw.size} bytes: a positive multiple of 4")
    words = raw.view("<u4")
    total = 0
    with np.errstate(over="ignore"):
        for lo in range(0, words.size, _CHUNK):
            w = words[lo:lo + _CHUNK].astype(np.uint64)
            x = w + np.arange(lo + 1, lo + 1 + w.size, dtype=np.uint64) * np.uint64(_GOLDEN)
            x ^= x >> np.uint64(30)
            x *= np.uint64(0xBF58476D1CE4E5B9)
            x ^= x >> np.uint64(27)
            x *= np.uint64(0x94D049BB133111EB)
            x ^= x >> np.uint64(31)
            total = (total + int(x.sum(dtype=np.uint64))) & _MASK
    return total


def arena_digest(t):
    """The digest of a tensor where it lives: the HIP kernel on a GPU, `digest_host` on the host."""
    if t.is_cuda:
        from . import ops
        return ops.arena_digest(t.contiguous())
    return digest_host(t)


def read(directory):
    """-> the dict of `<directory>/train_state.pt` after the checks that need no model: the file exists, its format is known, the world size is
    this run's."""
    path = Path(directory) / FILE
    if not path.exists():
        raise ValueError(f"{path} not found: --resume needs the state a run writes with --save_state 1 (with the weights alone, start a new "
                         f"run from them: --weights_from {Path(directory) / 'model.pt'})")
    state = torch.load(path, map_location="cpu")
    version = state.get("version") if isinstance(state, dict) else None
    if version != FORMAT_VERSION:
        raise ValueError(f"{path} has format version {version!r}, this code reads version {FORMAT_VERSION}: resume with the code that wrote it")
    if int(state["world"]) != parallel.world():
        raise ValueError(f"{path} was written by a run of {state['world']} rank(s), this one has {parallel.world()}: the data shards would "
                         f"differ - resume under the same world size")
    return state


def save(directory, model, train_ds, test_ds, epoch):
    """Write `<directory>/train_state.pt` (rank 0; every rank must call: with more than one rank the replicas are compared first, a collective).
    The file appears under its name complete or not at all: it is written under a temporary name in the same directory and renamed."""
    state = model.train_state()
    if parallel.exchanging():
        parallel.check_replicas(state["digests"]["params"], "flat_params", model.net.flat_params.device)
    if parallel.rank() != 0:
        return None
    directory = Path(directory)
    directory.mkdir(parents=True, exist_ok=True)
    record = {"version": FORMAT_VERSION, "epoch": int(epoch), "world": parallel.world(), "model": state,
              "train_data": train_ds.state_dict(), "test_data": test_ds.state_dict(), "digests": dict(state["digests"])}
    tmp = directory / f".{FILE}.tmp{os.getpid()}"
    try:
        torch.save(record, tmp)
        os.replace(tmp, directory / FILE)
    finally:
        if tmp.exists():
            tmp.unlink()
    return directory / FILE


def load(directory, model, train_ds, test_ds):
    """Restore what `save` wrote into a model that has loaded the `model.pt` written with it, and into both loaders.  -> the epoch"""
    state = read(directory)
    model.load_train_state(state["model"])
    train_ds.load_state_dict(state["train_data"])
    test_ds.load_state_dict(state["test_data"])
    return int(state["epoch"])
