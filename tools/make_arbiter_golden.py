"""Golden vectors of the two arbiters (test infrastructure; needs a checkout of the reference).

Runs the reference's own `Encoder`, `Decoder`, `Autoencoder.loss` and `Classifier.loss` (gms/arbiters/autoencoder.py, classifier.py) at
generation time only - nothing of the reference is copied here.  `gms.common` cannot be imported where torchvision and ignite are absent,
so the four class definitions are taken out of the two files with `ast` and executed against a stand-in `common` that holds what they
use of it (`AttrDict`, an `Arbiter` base that stores G), as the attn_core_*.npz fixtures were made.

    GMS_REFERENCE=<reference checkout> python tools/make_arbiter_golden.py

Writes tests/golden/arbiters_s28.npz - arrays and names only: hidden_size 16, batch 8, 1 x 28 x 28, seed 0, binarize 0 and 1.
  x_b0 [8, 1, 28, 28] in [-1, 1], x_b1 the same images as 0 / 1, y [8] int64
  ae_b{0,1}/<state-dict key>, clf/<state-dict key>          the weights (torch's default init under the seed)
  z_b{0,1} [8, 64] the encoder output, logits [8, 10],
  ae_b{0,1}/metric/<name> (full_loss, recon_loss, kl_loss, z_mean, z_std), clf/metric/cross_entropy_loss
"""
import ast
import os
import sys
import types

import numpy as np
import torch
from torch import nn

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "arbiters_s28.npz")


class AttrDict(dict):
    __setattr__ = dict.__setitem__
    __getattr__ = dict.__getitem__


class Arbiter(nn.Module):
    def __init__(self, G):
        super().__init__()
        self.G = G


def reference_classes(ref):
    """{name: class} of the class definitions of the two files, executed with their own imports except `gms.*`."""
    space = {"common": types.SimpleNamespace(AttrDict=AttrDict, Arbiter=Arbiter)}
    for name in ("autoencoder.py", "classifier.py"):
        tree = ast.parse(open(os.path.join(ref, "gms", "arbiters", name)).read())
        keep = [node for node in tree.body if isinstance(node, ast.ClassDef)
                or (isinstance(node, (ast.Import, ast.ImportFrom)) and not (getattr(node, "module", "") or "").startswith("gms"))]
        exec(compile(ast.Module(body=keep, type_ignores=[]), name, "exec"), space)
    return space


def main():
    ref = os.environ.get("GMS_REFERENCE")
    if not ref or not os.path.isdir(os.path.join(ref, "gms", "arbiters")):
        sys.exit("set GMS_REFERENCE to a checkout of the reference (the directory that holds gms/)")
    R = reference_classes(ref)
    g = torch.Generator().manual_seed(0)
    x = torch.rand((8, 1, 28, 28), generator=g) * 2 - 1
    y = torch.randint(0, 10, (8,), generator=g)
    out = {"x_b0": x.numpy(), "x_b1": (x > 0).float().numpy(), "y": y.numpy()}
    for b in (0, 1):
        torch.manual_seed(10 + b)
        G = AttrDict(hidden_size=16, z_size=64, beta=1e-6, binarize=b, lr=3e-4)
        model = R["Autoencoder"](G)
        xb = torch.from_numpy(out[f"x_b{b}"])
        with torch.no_grad():
            out[f"z_b{b}"] = model(xb).numpy()
            _, metrics = model.loss(xb)
        out.update({f"ae_b{b}/{key}": val.numpy() for key, val in model.state_dict().items()})
        out.update({f"ae_b{b}/metric/{key}": np.float64(val.item()) for key, val in metrics.items()})
    torch.manual_seed(20)
    clf = R["Classifier"](AttrDict(hidden_size=16, binarize=0, lr=3e-4))
    with torch.no_grad():
        out["logits"] = clf(x).numpy()
        _, metrics = clf.loss(x, y)
    out.update({f"clf/{key}": val.numpy() for key, val in clf.state_dict().items()})
    out.update({f"clf/metric/{key}": np.float64(val.item()) for key, val in metrics.items()})
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
