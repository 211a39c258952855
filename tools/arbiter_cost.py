"""How long the two arbiters take to train (arbiter_models.py through the driver, stock torch modules on the GPU): one epoch each, timed once.

    python tools/arbiter_cost.py [out=profiles/arbiter_cost.txt]

  MNIST-sized    938 batches of 64 synthetic 1 x 28 x 28 images (60 032 images: one epoch of MNIST at the driver's default --bs 64)
  CIFAR-sized    781 batches of 64 random 3 x 32 x 32 images held on the device (--data npy --data_device 1, 50 000 images)
both at the driver's default --hidden_size 256.  The time does not depend on the pixel values.  Printed per run: dt/train of the epoch as the
driver logs it (a host clock around the epoch's steps, which may stop before the GPU has drained its queue) and the wall time of the whole run up to
a device synchronise: model and data set-up, both evaluation passes, the epoch, two checkpoints with their TorchScript traces.  The defaults train 50 epochs (autoencoder) and 6 (classifier)."""
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, ".")
from generative_models_amd import main  # noqa: E402


def one_epoch(model, extra, logdir):
    started = time.time()
    final = main.train(*main.load_model_and_data([f"--model={model}", "--epochs", "1", "--save_n", "1", "--bs", "64", "--logdir", str(logdir)] + extra))
    torch.cuda.synchronize()
    return float(np.mean(final["dt/train"])), time.time() - started


def main_():
    out = sys.argv[1] if len(sys.argv) > 1 else "profiles/arbiter_cost.txt"
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    emit("$ python tools/arbiter_cost.py")
    emit(f"# {torch.cuda.get_device_name(0)}; one epoch per run, --bs 64, --hidden_size 256, timed once (the first run of a shape also loads its kernels)")
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        rng = np.random.default_rng(0)
        for split, n in (("train", 50000), ("test", 1024)):
            np.save(tmp / f"{split}_images.npy", rng.integers(0, 256, (n, 3, 32, 32), dtype=np.uint8))
            np.save(tmp / f"{split}_labels.npy", rng.integers(0, 10, n).astype(np.uint8))
        shapes = {"MNIST-sized, 938 batches of 1 x 28 x 28": ["--train_batches", "938", "--test_batches", "16"],
                  "CIFAR-sized, 781 batches of 3 x 32 x 32": ["--data", "npy", "--data_device", "1", "--data_root", str(tmp), "--in_channels", "3",
                                                              "--image_size", "32"]}
        for name, extra in shapes.items():
            for model in ("autoencoder", "classifier"):
                train_s, wall_s = one_epoch(model, extra, tmp / f"{model}_{len(lines)}")
                emit(f"{name}: --model={model}: epoch {train_s:.2f} s (dt/train), whole run {wall_s:.2f} s")
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main_()
