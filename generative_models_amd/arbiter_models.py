"""The two arbiters of the heavy evaluation as trainable plugins (reference gms/arbiters/autoencoder.py, classifier.py):

    python -m generative_models_amd.main --model=autoencoder [--data mnist|cifar10|npy --data_device 1] [--device cpu]
    python -m generative_models_amd.main --model=classifier

`Autoencoder` gives the 64-d latent space in which eval/fid and eval/precision|recall|f1 are taken, `Classifier` the logits behind
`classifier_loss`.  `save()` writes `model.pt` and `model.jit.pt`; the second is `torch.jit.trace` of `forward` (the encoder / the
logits), the file `--autoencoder` / `--classifier` load with `torch.jit.load` (gms/common.py:204-208).  Same layers, state-dict keys,
loss and metric names as the reference, so a reference checkpoint loads at 1 x 28 x 28.  Stock torch modules and torch.optim.Adam: an
arbiter trains once per dataset and runs only at evaluation, far off the hot path.

Past the reference, which is tied to 1 x 28 x 28 by its decoder: `--in_channels C` images of S x S, S % 4 == 0 and S >= 24
(`--image_size`, or 28 / 32 with `--pad32` as the diffusion model reads them).  The decoder's first kernel is S / 4 - 2 (5 at 28, 6 at
32, 14 at 64), which makes its output S x S; the encoder averages the spatial extent left in front of its flatten (1 x 1 at 28 - the
identity, bit for bit -, 2 x 2 at 32, 6 x 6 at 64), so the latent is z_size wide at every size.  One rank only."""
import math
from pathlib import Path

import torch
import torch.nn.functional as F
from torch import nn

from . import common, parallel

ARBITER_PLUGINS = True          # common.discover_models registers this file's models only when asked for arbiters (the driver does)
_EPS = torch.finfo(torch.float32).eps


def image_size(G):
    """S of the S x S images a run trains on: --image_size, else 32 with --pad32, else 28 (as the diffusion model reads the same flags)."""
    S = int(G.get("image_size", 0)) or (32 if G.get("pad32", 0) else 28)
    if S % 4 or S < 24:
        raise ValueError(f"images of {S} x {S}: the arbiters take S % 4 == 0 and S >= 24 (the decoder's first kernel is S / 4 - 2)")
    return S


class Encoder(nn.Module):
    """Four unpadded 3 x 3 convolutions (strides 2, 2, 1, 2), ReLU between them, the mean over what is left of the image, flatten."""

    def __init__(self, out_size, G):
        super().__init__()
        H, C = G.hidden_size, int(G.get("in_channels", 1))
        image_size(G)
        self.net = nn.Sequential(nn.Conv2d(C, H, 3, 2), nn.ReLU(), nn.Conv2d(H, H, 3, 2), nn.ReLU(), nn.Conv2d(H, H, 3, 1), nn.ReLU(),
                                 nn.Conv2d(H, out_size, 3, 2), nn.AdaptiveAvgPool2d(1), nn.Flatten(1, 3))

    def forward(self, x):
        return self.net(x)


class Decoder(nn.Module):
    """Four transposed convolutions (kernel / stride S / 4 - 2 / 1, 4 / 2, 4 / 2, 3 / 1) from a 1 x 1 latent to S x S, then tanh, or with
    binarize sigmoid."""

    def __init__(self, in_size, G):
        super().__init__()
        H, C = G.hidden_size, int(G.get("in_channels", 1))
        self.net = nn.Sequential(nn.ConvTranspose2d(in_size, H, image_size(G) // 4 - 2, 1), nn.ReLU(), nn.ConvTranspose2d(H, H, 4, 2), nn.ReLU(),
                                 nn.ConvTranspose2d(H, H, 4, 2), nn.ReLU(), nn.ConvTranspose2d(H, C, 3, 1))
        self.net.add_module("sigmoid" if G.binarize else "tanh", nn.Sigmoid() if G.binarize else nn.Tanh())

    def forward(self, z):
        return self.net(z[..., None, None])


def _to_unit(x, binarize):
    """Model-range pixels ([0, 1] with binarize, else [-1, 1]) -> [0, 1]."""
    return x if binarize else (x + 1.0) / 2.0


def _to_bytes(x):
    return (x.clamp(0.0, 1.0) * 255.0).round().to(torch.uint8).cpu()


class _ArbiterBase:
    """What both arbiters share, in front of common.GM in their bases (not a plugin itself): one rank, the image size, and a save() that
    also leaves the TorchScript file."""

    def __init__(self, G):
        super().__init__(G)
        if parallel.world() > 1:
            raise ValueError(f"--model={G.model}: the arbiters train on one rank (this run has {parallel.world()}); start it without torchrun")
        self.size = image_size(G)

    def _check(self, x):
        C = int(self.G.get("in_channels", 1))
        if x.dim() != 4 or tuple(x.shape[1:]) != (C, self.size, self.size):
            raise ValueError(f"batch of shape {tuple(x.shape)}: this model takes [B, {C}, {self.size}, {self.size}] (set --in_channels / "
                             f"--image_size / --pad32 to match the data)")

    def save(self, path, test_x=None, test_y=None):
        super().save(path, test_x, test_y)
        if test_x is None:
            test_x = torch.zeros((2, int(self.G.get("in_channels", 1)), self.size, self.size), device=next(self.parameters()).device)
        was_training = self.training
        self.eval()
        with torch.no_grad():
            torch.jit.save(torch.jit.trace(self, test_x), str(Path(path) / "model.jit.pt"))
        self.train(was_training)


class Autoencoder(_ArbiterBase, common.GM):
    DG = common.AttrDict()
    DG.eval_heavy = 0
    DG.z_size = 64
    DG.beta = 1e-6
    DG.binarize = 0
    DG.in_channels = 1
    DG.image_size = 0

    def __init__(self, G):
        super().__init__(G)
        self.encoder = Encoder(G.z_size, G)
        self.decoder = Decoder(G.z_size, G)
        self.optimizer = torch.optim.Adam(self.parameters(), lr=G.lr)

    def forward(self, x):
        return self.encoder(x)

    def loss(self, x, y=None):
        """recon + beta kl: -log p(x | z) per pixel under Bernoulli(decoded) (binarize) or Normal(decoded, 1), and KL(N(z, 1) || N(0, 1)) = z^2 / 2
        per latent, each averaged per image."""
        self._check(x)
        z = self.encoder(x)
        decoded = self.decoder(z)
        if self.G.binarize:
            p = decoded.clamp(_EPS, 1.0 - _EPS)              # torch.distributions.Bernoulli(probs=...): probabilities clamped, then logits
            recon = F.binary_cross_entropy_with_logits(p.log() - (-p).log1p(), x, reduction="none").mean((1, 2, 3))
        else:
            recon = (0.5 * (x - decoded) ** 2 + 0.5 * math.log(2.0 * math.pi)).mean((1, 2, 3))
        kl = (0.5 * z ** 2).mean(-1)
        loss = (recon + self.G.beta * kl).mean()
        return loss, {"full_loss": loss, "recon_loss": recon.mean(), "kl_loss": kl.mean(), "z_mean": z.mean(), "z_std": z.std()}

    def evaluate(self, writer, x, y, epoch):
        """The picture `reconstruction`: 8 test images, their reconstructions, and the error (grey = none), one line each."""
        if writer is None:
            return
        truth = x[:8]
        recon = self.decoder(self.encoder(truth))
        if self.G.binarize:
            recon = (recon > 0.5).float()
        span = 1.0 if self.G.binarize else 2.0
        rows = torch.cat([_to_unit(truth, self.G.binarize), _to_unit(recon, self.G.binarize), (recon - truth) / (2.0 * span) + 0.5], 0)
        n, (C, S) = truth.shape[0], truth.shape[1:3]
        grid = rows.reshape(3, n, C, S, S).permute(2, 0, 3, 1, 4).reshape(C, 3 * S, n * S)
        writer.add_image("reconstruction", _to_bytes(grid), epoch)


class Classifier(_ArbiterBase, common.GM):
    DG = common.AttrDict()
    DG.eval_heavy = 0
    DG.epochs = 6          # the reference's pick: it starts to overfit MNIST after about this many
    DG.binarize = 0
    DG.save_n = 1
    DG.in_channels = 1
    DG.image_size = 0

    def __init__(self, G):
        super().__init__(G)
        self.net = Encoder(10, G)
        self.optimizer = torch.optim.Adam(self.parameters(), lr=G.lr)

    def forward(self, x):
        return self.net(x)

    def loss(self, x, y):
        self._check(x)
        loss = F.cross_entropy(self.net(x), y)
        return loss, {"cross_entropy_loss": loss}

    def evaluate(self, writer, x, y, epoch):
        """The strip `classifier/pred`: the first 10 test images, green where the prediction is the label, red where it is not."""
        if writer is None:
            return
        shown, labels = x[:10], y[:10]
        right = self.net(shown).argmax(1) == labels
        grey = _to_unit(shown, self.G.binarize).mean(1)                            # [n, S, S]
        tint = torch.zeros((shown.shape[0], 3, self.size, self.size), device=x.device)
        tint[right, 1] = grey[right]
        tint[~right, 0] = grey[~right]
        writer.add_image("classifier/pred", _to_bytes(tint.permute(1, 2, 0, 3).reshape(3, self.size, -1)), epoch)
