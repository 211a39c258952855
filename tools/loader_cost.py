"""What feeding the train loop costs: the driver's own loop (main.Session.train_epoch) over three sources of batches, same process, interleaved.

    python tools/loader_cost.py [rounds=5] [data_root=data] [out=profiles/loader_cost.txt]

  (a) host     data.MnistLoader's per-step path as it stands: fp32 set on the host (pinned), `x[idx]` gather into a new pageable tensor, then a
               non_blocking copy to the device.  The class's own __iter__ / __len__; only the constructor is restated here, to take arrays
               and more than one channel.
  (b) device   data.DeviceDataset: uint8 set on the GPU, one gmk_batch_gather launch per batch (flip_p = 0.5 on the 3-channel shape).
  (c) replay   one device batch handed out again and again (y cloned, as bench.py does): no loader at all - the bench's feeding.
Shapes: 1x28x28 at B = 1024 over 60 000 images (MNIST) and 3x32x32 at B = 2048 over 50 000 (CIFAR-10): the real files under data_root when
they are there, random bytes of the same sizes otherwise (the time of the loop does not depend on the pixel values).  One model per shape is
shared by the three arms; every round times one epoch of each, the order alternating.  Also: the kernel's own time (HIP events) against a
device-to-device copy that moves the same number of bytes."""
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, ".")
from generative_models_amd import data, main, ops  # noqa: E402

SHAPES = {"1x28x28, B = 1024": (1, 28, 1024, 60000), "3x32x32, B = 2048": (3, 32, 2048, 50000)}


class HostLoader(data.MnistLoader):
    """MnistLoader over arrays [N, C, H, W]: the same attributes as its constructor leaves, hence the same per-step work."""

    def __init__(self, images, labels, bs, device, seed=1000):
        n, c, h, w = images.shape
        self.x = data.transform(images.reshape(n * c, h, w), False, False).reshape(n, c, h, w)
        self.y = torch.from_numpy(labels.astype(np.int64))
        self.bs, self.device, self.rank, self.world = int(bs), device, 0, 1
        self.gen = torch.Generator().manual_seed(seed)
        self.x, self.y = self.x.pin_memory(), self.y.pin_memory()


class Replay:
    def __init__(self, x, y, n):
        self.x, self.y, self.n = x, y, n

    def __len__(self):
        return self.n

    def __iter__(self):
        for _ in range(self.n):
            yield self.x, self.y.clone()


def arrays(c, size, n, root):
    try:
        if c == 1:
            images = data.read_idx(data._find(root, data.FILES[True][0]))[:, None]
            return images, data.read_idx(data._find(root, data.FILES[True][1])), "MNIST train files"
        (images, labels), _ = data.load_cifar10(root)
        return images, labels, "CIFAR-10 train files"
    except FileNotFoundError:
        rng = np.random.default_rng(0)
        return rng.integers(0, 256, (n, c, size, size), dtype=np.uint8), rng.integers(0, 10, n, dtype=np.uint8), "random bytes (files absent)"


def epoch(session, ds):
    session.train_ds = ds
    log = main.EpochLog("diffusion")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    session.train_epoch(log)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return len(ds) * ds.bs / dt if hasattr(ds, "bs") else len(ds) * ds.x.shape[0] / dt


def kernel_time(dev, bs, emit):
    idx = torch.randperm(dev.images.shape[0], device="cuda")[:bs].contiguous()
    n, c, h, w = dev.images.shape
    moved = bs * c * h * w + 4 * bs * c * (h + 2 * dev.pad) * (w + 2 * dev.pad)          # bytes read + bytes written
    src = torch.empty(moved // 2, dtype=torch.uint8, device="cuda")
    dst = torch.empty_like(src)
    run = {"batch_gather_kernel": lambda: ops.batch_gather(dev.images, dev.labels, idx, pad=dev.pad, binarize=dev.binarize, flip_p=dev.flip_p,
                                                           seed=1, offset=0, trusted=True),
           "copy of the same bytes": lambda: dst.copy_(src)}
    for name, fn in run.items():
        for _ in range(5):
            fn()
        times = []
        for _ in range(20):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); e.synchronize()
            times.append(s.elapsed_time(e) * 1e3)
        med = statistics.median(times)
        emit(f"  {name}: median {med:.1f} us of 20 (min {min(times):.1f}), {moved / 1e6:.1f} MB moved = {moved / med / 1e6:.2f} TB/s")


def main_():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    root = sys.argv[2] if len(sys.argv) > 2 else "data"
    out = sys.argv[3] if len(sys.argv) > 3 else "profiles/loader_cost.txt"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit(f"$ python tools/loader_cost.py {rounds}")
    emit(f"# {torch.cuda.get_device_name(0)}; images/s of main.Session.train_epoch, one epoch per arm and round, order alternating; torch host threads: "
         f"{torch.get_num_threads()}")
    for name, (c, size, bs, n) in SHAPES.items():
        images, labels, source = arrays(c, size, n, root)
        argv = ["--model=diffusion", "--bs", str(bs), "--in_channels", str(c), "--image_size", str(size), "--binarize", "0", "--timesteps", "1000",
                "--logdir", tempfile.mkdtemp()]
        G, Model = main.FlagSpace(main.DG).resolve(argv)
        torch.manual_seed(0)
        model = Model(G=G).to("cuda")
        model.run_device = "cuda"
        dev = data.DeviceDataset(images, labels, bs, binarize=0, pad=0, flip_p=0.5 if c == 3 else 0.0, device="cuda", seed=1000)
        arms = {"(a) host": HostLoader(images, labels, bs, "cuda"), "(b) device": dev}
        arms["(c) replay"] = Replay(*next(iter(dev)), len(dev))
        session = main.Session(model, None, None, None, None, G)
        emit(f"{name}: {images.shape[0]} images, {source}, {len(dev)} steps per epoch")
        for ds in arms.values():                 # warm-up: one epoch each (kernels loaded, allocator pools and pinned staging at their steady size)
            epoch(session, ds)
        rates = {arm: [] for arm in arms}
        for r in range(rounds):
            for arm in (list(arms) if r % 2 == 0 else reversed(list(arms))):
                rates[arm].append(epoch(session, arms[arm]))
        med = {arm: statistics.median(v) for arm, v in rates.items()}
        for arm, v in rates.items():
            emit(f"  {arm}: median {med[arm]:9.1f} images/s, {bs / med[arm] * 1e3:7.3f} ms per step, spread {(max(v) - min(v)) / med[arm]:.2%}  "
                 f"(rounds: {', '.join(f'{x:.0f}' for x in v)})")
        emit(f"  (b) / (a): {med['(b) device'] / med['(a) host'] - 1:+.2%};  (b) / (c): {med['(b) device'] / med['(c) replay'] - 1:+.2%};  "
             f"(a) / (c): {med['(a) host'] / med['(c) replay'] - 1:+.2%}")
        kernel_time(dev, bs, emit)
        del model, session, arms, dev
        torch.cuda.empty_cache()
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main_()
