"""The heavy evaluation's numbers for a dumped sample file (`--dump_samples N` of the driver) against a dataset's test split:

    python -m generative_models_amd.heavy_eval --samples <run>/samples_images.npy --data mnist|cifar10|npy --data_root data \\
        --autoencoder <arbiter run>/model.jit.pt [--k 3] [--max_real 0] [--binarize 0] [--pad32 0] [--bs 1024] [--device cuda]

A thin wrapper over metrics.score_latents (the Fréchet distance from float64 moments and metrics.manifold_metrics): both byte sets go through the
reference's transform chain (data.transform's: / 255, then 2 x - 1 or the binarize threshold, then the pad32 border) in batches, are embedded
by the TorchScript encoder, and the latents are scored on the device.  Prints one JSON line: fid, precision, recall, f1, density, coverage,
samples, real, k, encoder ("trained" when the file's directory holds this driver's hps.yaml, else "reference")."""
import argparse
import json
from pathlib import Path

import numpy as np
import torch

from . import data as datasets
from . import metrics


def load_test_images(kind, root):
    """uint8 [N, C, H, W]: the test split of `--data kind` under `root`."""
    if kind == "mnist":
        images = datasets.read_idx(datasets._find(root, datasets.FILES[False][0]))
    elif kind == "cifar10":
        images = datasets.load_cifar10(root)[1][0]
    elif kind == "npy":
        images = datasets.load_npy(root)[1][0]
    else:
        raise ValueError(f"--data {kind!r}: 'mnist', 'cifar10' or 'npy'")
    return images[:, None] if images.ndim == 3 else images


@torch.inference_mode()
def embed_bytes(encoder, images, device, bs=1024, binarize=False, pad32=False):
    """uint8 [N, C, H, W] -> fp32 latents [N, Z] on `device`."""
    out = []
    for lo in range(0, images.shape[0], bs):
        x = torch.from_numpy(np.ascontiguousarray(images[lo:lo + bs])).to(device).float().div(255)
        x = (x > 0.5).float() if binarize else 2 * x - 1
        if pad32:
            x = torch.nn.functional.pad(x, (2, 2, 2, 2))
        out.append(encoder(x).float())
    return torch.cat(out)


def score_files(samples, real, encoder, device, k=3, **transform):
    """-> score_latents' dict for two uint8 image arrays."""
    if samples.ndim == 3:
        samples = samples[:, None]
    if samples.dtype != np.uint8 or samples.ndim != 4 or samples.shape[1:] != real.shape[1:]:
        raise ValueError(f"samples {samples.dtype} {samples.shape} against test images {real.shape}: want uint8 [N, C, H, W] of the same image shape")
    return metrics.score_latents(embed_bytes(encoder, real, device, **transform), embed_bytes(encoder, samples, device, **transform), k)


def main(argv=None):
    from .main import _trained_here
    parser = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    parser.add_argument("--samples", type=Path, required=True)
    parser.add_argument("--data", default="mnist")
    parser.add_argument("--data_root", type=Path, default=Path("data"))
    parser.add_argument("--autoencoder", type=Path, required=True)
    parser.add_argument("--k", type=int, default=3)
    parser.add_argument("--max_real", type=int, default=0, help="0: the whole test split")
    parser.add_argument("--binarize", type=int, default=0)
    parser.add_argument("--pad32", type=int, default=0)
    parser.add_argument("--bs", type=int, default=1024)
    parser.add_argument("--device", default="cuda")
    args = parser.parse_args(argv)
    samples = np.load(args.samples, allow_pickle=False)
    real = load_test_images(args.data, str(args.data_root))
    if args.max_real > 0:
        real = real[:args.max_real]
    encoder = torch.jit.load(str(args.autoencoder)).to(args.device)
    scores = score_files(samples, real, encoder, args.device, args.k, bs=args.bs, binarize=bool(args.binarize), pad32=bool(args.pad32))
    scores.update(samples=int(samples.shape[0]), real=int(real.shape[0]), k=args.k, encoder="trained" if _trained_here(args.autoencoder) else "reference")
    print(json.dumps(scores))
    return scores


if __name__ == "__main__":
    main()
