"""Training driver for the `GM` plugin surface — the caller above the hot path (reference gms/main.py).

What is kept from the reference is its INTERFACE: the flag table `DG` (gms/main.py:20-40) merged with the selected model's own
`DG`, `--weights_from <dir>/model.pt` re-reading `<dir>/hps.yaml` (:55-64,79-82), the order in which a model is driven (evaluate
first, then train: :159-217), the calls made on it (`to / eval / loss / evaluate / save / train / train_step`), the metric key
naming (`<model>/test/<key>`, `<model>/train/<key>`, `eval/*`, `dt/*`, `num_vars`) and the `load_model_and_data()` / `train()`
entry points.  How it is built is this repository's own: one `Session` object per run, flags resolved in layers by `FlagSpace`,
an `EpochLog` that keeps device tensors on the device until the epoch ends (the reference's `.cpu()` per step, :215, would
serialise host and GPU every step), rank-aware logging and checkpointing for one-process-per-GPU runs.

Environment differences (no network, no tensorboard / ignite in the image): `--data synthetic` (default) is an MNIST-shaped
generator, `--data mnist` reads the IDX files if they are present; the writer is `common.NullWriter`, or with `--save_images 1`
`common.ImageWriter` (PNG / APNG files under <logdir>/images; `--dump_samples N` writes samples as an `npy` dataset).  `--data_device 1` keeps
`mnist`, `cifar10` or an `npy` array on the GPU and assembles every batch there (data.DeviceDataset); with it,
`--nn_eval Q` reports after every checkpoint how close Q samples lie to their nearest training images (neighbours.py).

    python -m generative_models_amd.main --model=diffusion --epochs=1 --bs 32
    torchrun --nproc-per-node 8 -m generative_models_amd.main --model=diffusion      (one process per GPU, RCCL)
"""
import argparse
import os
import re
import time
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch
import torch.distributed as dist
import yaml

from . import checkpoint as train_state
from . import common, parallel
from . import data as datasets
from . import metrics as heavy

DG = common.AttrDict()     # gms/main.py:20-40
DG.model = "vae"
DG.bs = 64
DG.hidden_size = 256
DG.device = "cuda"
DG.epochs = 50
DG.save_n = 5
DG.logdir = Path("./logs/")
DG.lr = 3e-4
DG.class_cond = 0
DG.binarize = 1
DG.pad32 = 0
DG.mode = "train"
DG.weights_from = Path(".")
DG.autoencoder = Path("./weights/autoencoder.pt")
DG.classifier = Path("./weights/classifier.pt")
DG.eval_heavy = 0
DG.skip_training = 0
# additions
DG.data = "synthetic"      # 'synthetic' | 'mnist' (IDX files under <data_root>/MNIST/raw) | with data_device 1 also 'cifar10'
                           # (<data_root>/cifar-10-batches-bin) and 'npy' (<data_root>/{train,test}_{images,labels}.npy)
DG.data_root = Path("data")
DG.train_batches = 8       # synthetic batches per epoch (per rank)
DG.test_batches = 2
DG.data_device = 0         # 1: the dataset stays on the GPU as uint8 and one HIP kernel assembles each batch (data.DeviceDataset)
DG.flip_p = 0.0            # probability of a horizontal flip per train image (data_device 1 only)
DG.save_images = 0         # 1: evaluation samples go to <logdir>/images as PNG grids and APNG strips (common.ImageWriter)
DG.image_frames = 60       # most frames an APNG keeps of a sampling trajectory (evenly spread, first and last always)
DG.save_state = 0          # 1: every checkpoint also writes <logdir>/train_state.pt, what --resume needs beside model.pt (checkpoint.py)
DG.resume = Path(".")      # <dir>: continue the run that wrote <dir>/model.pt + train_state.pt, with its hps.yaml under the command line
DG.dump_samples = 0        # N > 0: after every checkpoint, N samples as <logdir>/samples_{images,labels}.npy (data.load_npy's format)
DG.nn_eval = 0             # Q > 0: after every checkpoint, Q samples beside their nearest training images in pixel space (neighbours.py;
                           # data_device 1 and binarize 0 only): eval/nn_dist, eval/nn_dist_test, eval/nn_closer, <logdir>/nearest_neighbours.npz
DG.nn_k = 3                # neighbours kept per sample (1 .. 8)
DG.eval_heavy_samples = 0  # N > 0: the heavy evaluation draws at least N samples instead of the reference's 500 and scores them without a distance
                           # matrix (metrics.eval_heavy_at_scale: also eval/density, eval/coverage, eval/heavy_samples); this rank's shard only
DG.eval_heavy_k = 3        # neighbours of the k-NN balls of that evaluation (1 .. 8)

SyntheticMNIST = datasets.SyntheticMNIST       # kept importable from here


class FlagSpace:
    """Flags in layers: the driver's table, then either the model's own `DG` or — with `--weights_from` or `--resume` — the `hps.yaml`
    saved next to the checkpoint, then the command line (`--resume run --epochs 100` extends a run).  Only the command line starts a resume:
    a `resume` key in an `hps.yaml` is the record of how that run was started.  Driver keys parse through `common.args_type` (bools as
    'True'/'False', '1e3' for ints, expanded Paths); keys a later layer introduces parse with the type of their default."""

    def __init__(self, base):
        self.base = base

    @staticmethod
    def _parser(typed):
        parser = argparse.ArgumentParser()
        for key, (convert, default) in typed.items():
            parser.add_argument(f"--{key}", type=convert, default=default)
        return parser

    def resolve(self, argv=None):
        """-> (G, Model)"""
        typed = {key: (common.args_type(value), value) for key, value in self.base.items()}
        peek, _ = self._parser(typed).parse_known_args(argv)          # first look: which model, which checkpoint, which logdir
        registry = common.discover_models(arbiters=True)
        resuming = peek.resume != Path(".")
        if resuming and peek.weights_from != Path("."):
            raise ValueError(f"--resume {peek.resume} together with --weights_from {peek.weights_from}: a resumed run takes its weights from "
                             f"<resume>/model.pt; give one of the two")
        if resuming or peek.weights_from != Path("."):
            with open((peek.resume if resuming else peek.weights_from.parent) / "hps.yaml") as f:
                layer = dict(yaml.load(f, Loader=yaml.Loader))
            layer.pop("full_cmd", None)                                   # the saved command line is a record, not a flag
            layer.pop("arbiters", None)                                   # ... and so is the feature space of that run's eval/* numbers
            layer.pop("resume", None)                                     # ... and so is the directory that run itself was resumed from
            if resuming:
                layer["logdir"] = peek.resume
            Model = registry[layer["model"]]
        else:
            Model = registry[peek.model]
            layer = dict(Model.DG)
            layer["logdir"] = peek.logdir / peek.model
        for key, value in layer.items():
            convert = typed[key][0] if key in typed else type(value)
            typed[key] = (convert, value)
        G = common.AttrDict(vars(self._parser(typed).parse_args(argv)))
        if resuming:
            G.save_state = 1                                              # a resumed run stays resumable
        return G, Model


class EpochLog:
    """Metric lists of one epoch.  Values may be device tensors: they are moved to the host in ONE pass when the epoch is
    flushed, so nothing in the training loop waits for the GPU."""

    def __init__(self, model_key):
        self.model_key = model_key
        self.values = defaultdict(list)

    def key_for(self, split, name):
        if name == "nlogp":                                            # gms/main.py:170-174,212-214
            return "eval/nlogp" if split == "test" else "train/nlogp"
        return f"{self.model_key}/{split}/{name}"

    def add(self, split, metrics):
        for name, value in metrics.items():
            self.values[self.key_for(split, name)].append(value.detach() if isinstance(value, torch.Tensor) else value)

    def set(self, key, value):
        self.values[key] = value

    def to_host(self):
        out = {}
        for key, vals in self.values.items():
            if isinstance(vals, list):
                out[key] = [v.cpu().item() if isinstance(v, torch.Tensor) else v for v in vals]
            else:
                out[key] = vals
        return out


LOSS_PROFILE_FILE = "loss_profile.csv"
NN_FILE = "nearest_neighbours.npz"
NN_PICTURE_ROWS = 10
LOSS_PROFILE_COLUMNS = ("epoch", "split", "bin", "u_lo", "u_hi", "logsnr_hi", "logsnr_lo", "weight", "loss_mean", "loss_rms", "x_mse_mean", "p")


def append_loss_profile(logdir, epoch, split, rows):
    """Append one split's loss profile (`GaussianDiffusion.profile`'s dict of [64] arrays) to <logdir>/loss_profile.csv, one row per bin under
    LOSS_PROFILE_COLUMNS (the header when the file is new).  A mean of an empty bin (weight 0) and `p` without time_importance are left empty."""
    path = Path(logdir) / LOSS_PROFILE_FILE
    path.parent.mkdir(parents=True, exist_ok=True)
    new = not path.exists()
    num = lambda v: "" if v is None or not np.isfinite(v) else f"{float(v):.9g}"
    with open(path, "a") as f:
        if new:
            f.write(",".join(LOSS_PROFILE_COLUMNS) + "\n")
        for k in range(len(rows["weight"])):
            cells = [str(int(epoch)), split, str(k)] + [num(rows[c][k]) for c in LOSS_PROFILE_COLUMNS[3:-1]]
            cells.append("" if rows.get("p") is None else num(rows["p"][k]))
            f.write(",".join(cells) + "\n")
    return path


class Session:
    """One run of the driver: model, data, feature extractors, flags."""

    def __init__(self, model, train_ds, test_ds, autoencoder, classifier, G):
        self.model, self.train_ds, self.test_ds = model, train_ds, test_ds
        self.autoencoder, self.classifier, self.G = autoencoder, classifier, G
        self.device = getattr(model, "run_device", G.device)
        self.lead = parallel.rank() == 0                               # rank 0 prints, writes hps.yaml and checkpoints
        self.writer = common.ImageWriter(G.logdir, G.get("image_frames", 60)) if G.get("save_images", 0) else common.NullWriter(G.logdir)
        self.nn_index = None                                           # neighbours.NeighbourIndex of the training set, built at the first report

    def _batches(self, ds):
        for batch in ds:
            yield batch[0].to(self.device), batch[1].to(self.device)

    def flush(self, log, epoch):
        record = log.to_host()
        if self.lead:
            common.dump_logger(record, self.writer, epoch, self.G)
        return EpochLog(self.G.model)

    def evaluate(self, log, epoch):
        """Test-set pass + the model's own `evaluate` (gms/main.py:159-183)."""
        self.model.eval()
        last = None
        with torch.no_grad():
            if hasattr(self.model, "loss"):
                for last in self._batches(self.test_ds):
                    log.add("test", self.model.loss(*last)[1])
            else:
                last = next(self._batches(self.test_ds))
            if getattr(self.model, "loss_profile", 0):                  # an extension: where along the noise axis the loss sits
                self.write_loss_profile(epoch)
            started = time.time()
            self.model.evaluate(self.writer if self.lead else None, last[0], last[1], epoch)
            log.set("dt/eval", time.time() - started)
        log.set("num_vars", common.count_vars(self.model))
        return last

    def write_loss_profile(self, epoch):
        """After the test pass: the test split's profile of this evaluation (64 rows; the state is reset on read) and, once it holds any
        weight, the train split's running one, appended to <logdir>/loss_profile.csv by rank 0 (its own ranks' samples)."""
        diffusion = self.model.diffusion
        for split in ("test", "train"):
            rows = diffusion.profile(split, reset=split == "test")
            if self.lead and rows is not None and (split == "test" or rows["weight"].sum() > 0):
                append_loss_profile(self.G.logdir, epoch, split, rows)

    def checkpoint(self, log, last_batch, epoch=0):
        if self.lead:
            self._write_checkpoint(log, last_batch, epoch)
        # last: the heavy evaluation and dump_samples draw from the model's streams and advance the test loader, and the neighbour report
        # draws from the streams too.  Every rank enters (the replica check of a data-parallel run is a collective), rank 0 writes
        if self.G.get("save_state", 0):
            train_state.save(Path(self.G.logdir), self.model, self.train_ds, self.test_ds, epoch)
            if self.lead:
                print("SAVED TRAIN STATE", self.G.logdir)

    def _write_checkpoint(self, log, last_batch, epoch=0):
        Path(self.G.logdir).mkdir(parents=True, exist_ok=True)
        self.model.save(Path(self.G.logdir), *last_batch)
        print("SAVED MODEL", self.G.logdir)
        if self.G.eval_heavy:                                          # gms/main.py:191-196
            print("RUNNING HEAVY EVAL...")
            started = time.time()
            host_log = defaultdict(list)
            heavy.eval_heavy(host_log, self.model, self.test_ds, self.autoencoder, self.classifier, self.G)
            for key, vals in host_log.items():
                log.set(key, vals)
            log.set("dt/eval_heavy", time.time() - started)
            print("DONE HEAVY EVAL")
        if self.G.get("dump_samples", 0) > 0:
            self.dump_samples(int(self.G.dump_samples))
        if self.G.get("nn_eval", 0) > 0:
            self.nn_eval(log, int(self.G.nn_eval), int(self.G.nn_k), epoch)

    def draw_uint8(self, n):
        """-> (samples uint8 [n, C, H, W] on the device, labels int64 [n]): drawn in batches of `bs`; with class_cond the labels are
        arange(n) % 10 and the draw is guided as `sample(n, y)` is, else unconditional with labels 0."""
        cond = bool(self.G.get("class_cond", 0))
        labels = torch.arange(n, dtype=torch.long, device=self.device) % 10 if cond else torch.zeros(n, dtype=torch.long, device=self.device)
        was_training = self.model.training
        self.model.eval()
        parts = []
        for lo in range(0, n, int(self.G.bs)):
            y = labels[lo:lo + int(self.G.bs)]
            parts.append(self.model.sample_uint8(y.numel(), y.clone() if cond else None))
        self.model.train(was_training)
        return torch.cat(parts), labels

    def dump_samples(self, n):
        """n samples of the model as a dataset: <logdir>/samples_images.npy (uint8 [n, C, H, W]) and samples_labels.npy (uint8 [n]), the
        format of data.load_npy - renamed to train_* / test_*, a set `--data npy --data_device 1` trains on.  The draw: draw_uint8."""
        samples, labels = self.draw_uint8(n)
        logdir = Path(self.G.logdir)
        np.save(logdir / "samples_images.npy", samples.cpu().numpy())
        np.save(logdir / "samples_labels.npy", labels.cpu().numpy().astype(np.uint8))
        print("DUMPED", n, "SAMPLES", logdir)

    def nn_eval(self, log, n, k, epoch):
        """n samples (draw_uint8) and the first min(n, N_test) images of the test split, each beside its k nearest training images in pixel
        space (neighbours.nn_report; mirrored matches count when the train split flips): logs eval/nn_dist, eval/nn_dist_test, eval/nn_closer
        and dt/nn_eval, writes <logdir>/nearest_neighbours.npz (samples, index, dist2, mirrored, test_dist2, epoch) and, with save_images, the
        picture `nearest`: one line per sample for the first 10, the sample and then its neighbours as the dataset stores them.  The test
        loader is not advanced; the training set's norms are computed at the first report of the run."""
        from . import neighbours
        started = time.time()
        if self.nn_index is None:
            self.nn_index = neighbours.NeighbourIndex(self.train_ds.images)
        samples, _ = self.draw_uint8(n)
        holdout = self.test_ds.images[:min(n, self.test_ds.images.shape[0])]
        report = neighbours.nn_report(self.nn_index, samples, holdout, k, mirror=self.G.get("flip_p", 0.0) > 0)
        for key in ("nn_dist", "nn_dist_test", "nn_closer"):
            log.set(f"eval/{key}", report[key])
        np.savez(Path(self.G.logdir) / NN_FILE, samples=samples.cpu().numpy(), index=report["index"], dist2=report["dist2"],
                 mirrored=report["mirrored"], test_dist2=report["test_dist2"], epoch=np.int64(epoch))
        if self.G.get("save_images", 0) and samples.shape[1] in (1, 3):
            rows = min(NN_PICTURE_ROWS, n)
            found = self.train_ds.images[torch.from_numpy(report["index"][:rows]).to(self.device)]          # [rows, k, C, H, W]
            tiles = torch.cat((samples[:rows, None], found), 1).flatten(0, 1)
            # byte b as the float whose quantisation (ops.to_uint8's rule, trunc((x + 1) 127.5)) is b again: the middle of b's interval
            self.writer.write_frames("nearest", (tiles.float() + 0.5) / 127.5 - 1.0, epoch, ncol=k + 1)
        log.set("dt/nn_eval", time.time() - started)
        print("NEAREST NEIGHBOURS OF", n, "SAMPLES", {key: round(report[key], 6) for key in ("nn_dist", "nn_dist_test", "nn_closer")})

    def train_epoch(self, log):
        self.model.train()
        started = time.time()
        if not self.G.skip_training:
            for x, y in self._batches(self.train_ds):
                log.add("train", self.model.train_step(x, y))
        log.set("dt/train", time.time() - started)

    def run(self):
        # a resumed run's state is "after evaluate(e) and checkpoint(e)": it enters the loop at train_epoch(e)
        resumed = getattr(self.model, "resumed_epoch", None)
        epoch = 0 if resumed is None else int(resumed)
        log = self.flush(EpochLog(self.G.model), epoch)                 # writes hps.yaml before anything else, like the reference
        while True:
            if resumed is None:
                last = self.evaluate(log, epoch)
                if epoch % self.G.save_n == 0:
                    self.checkpoint(log, last, epoch)
                final = log.to_host() if epoch >= self.G.epochs else None
                log = self.flush(log, epoch)
                if final is not None:
                    return final
            resumed = None
            self.train_epoch(log)
            epoch += 1


def init_distributed():
    """One process per GPU under torchrun: RCCL (backend "nccl") when GPUs are present, gloo otherwise."""
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and "RANK" in os.environ and not dist.is_initialized():
        if torch.cuda.is_available():
            from .parallel import configure_rccl_env
            configure_rccl_env()
            torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))
            dist.init_process_group(backend="nccl")
        else:
            dist.init_process_group(backend="gloo")


def _run_device(flag):
    """The torch device of this rank.  `G.device` itself stays what the user passed ('cuda'), so an hps.yaml written by a
    multi-GPU run does not pin a later `--weights_from` run to one rank's card."""
    if str(flag) == "cuda" and torch.cuda.is_available() and dist.is_initialized():
        return f"cuda:{torch.cuda.current_device()}"
    return str(flag)


_HPS_MODEL = re.compile(r"^model:[ \t]*['\"]?([A-Za-z0-9_]+)['\"]?[ \t]*$", flags=re.M)


def _trained_here(path):
    """Whether a TorchScript arbiter was saved by this driver: its directory holds the hps.yaml of an --model=autoencoder / classifier run.
    Only the top-level `model:` line is read, as text: the file sits beside a path the user names, and nothing in it is constructed."""
    try:
        found = _HPS_MODEL.search((Path(path).parent / "hps.yaml").read_text())
    except (OSError, UnicodeDecodeError):
        return False
    return found is not None and found.group(1) in ("autoencoder", "classifier")


def _feature_extractors(G, device, test_ds=None):
    """TorchScript autoencoder / classifier of the heavy eval (gms/main.py:86-91) when the files exist: trained here with
    --model=autoencoder / --model=classifier (arbiter_models.py) or brought from elsewhere.  The reference's own weight files
    are not in its checkout (.MISSING_LARGE_BLOBS): without a file the stand-ins of `arbiters.py` take over (a fixed random-feature
    encoder; a nearest-class-centroid classifier fitted on the labelled test batches), so `--eval_heavy 1` runs end to end."""
    if not G.eval_heavy:
        return None, None
    from . import arbiters
    cond = bool(G.get("class_cond", 0))
    if Path(G.autoencoder).exists():
        autoencoder = torch.jit.load(str(G.autoencoder)).to(device)
    else:
        print(f"eval_heavy: {G.autoencoder} not found - using the built-in random-feature encoder (values not comparable with the "
              f"reference's autoencoder space)")
        autoencoder = arbiters.RandomFeatureEncoder().to(device)
    classifier = None
    if cond and Path(G.classifier).exists():
        classifier = torch.jit.load(str(G.classifier)).to(device)
    elif cond:
        print(f"eval_heavy: {G.classifier} not found - fitting the built-in nearest-centroid classifier on the test batches")
        import copy
        batches = ((b[0].to(device), b[1].to(device)) for b in copy.deepcopy(test_ds))      # a copy: the run's own test stream stays untouched
        classifier = arbiters.CentroidClassifier(arbiters.RandomFeatureEncoder().to(device)).to(device).fit(batches)
    # recorded in hps.yaml next to the flags: which feature space the eval/* numbers of this run live in
    G.arbiters = "stand-in" if (getattr(autoencoder, "stand_in", False) or getattr(classifier, "stand_in", False)) else "reference"
    if G.arbiters == "reference" and _trained_here(G.autoencoder) and (classifier is None or _trained_here(G.classifier)):
        G.arbiters = "trained"          # TorchScript files of arbiter_models.py: the reference's architecture and keys, this driver's training run
    return autoencoder, classifier


DEVICE_DATA = ("mnist", "cifar10", "npy")


def _check_data_flags(G):
    """Flag combinations the data path does not serve, named before any model or file is touched."""
    if G.data not in DEVICE_DATA + ("synthetic",):
        raise ValueError(f"--data {G.data!r}: 'synthetic', 'mnist', or with --data_device 1 'cifar10' / 'npy'")
    if G.data_device not in (0, 1):
        raise ValueError(f"--data_device {G.data_device}: 0 (host loader) or 1 (dataset on the GPU)")
    if not 0.0 <= G.flip_p <= 1.0:
        raise ValueError(f"--flip_p {G.flip_p}: a probability")
    if G.data_device and G.data not in DEVICE_DATA:
        raise ValueError(f"--data_device 1 serves --data {' / '.join(DEVICE_DATA)}; --data {G.data} already draws on the device")
    if not G.data_device and G.data in ("cifar10", "npy"):
        raise ValueError(f"--data {G.data} needs --data_device 1 (there is no host loader for it)")
    if G.flip_p > 0 and not G.data_device:
        raise ValueError(f"--flip_p {G.flip_p} needs --data_device 1 (the flip is part of the device batch kernel)")


def _check_resume_flags(G, Model):
    """The flags of the train state, named before any model is built."""
    if G.save_state not in (0, 1):
        raise ValueError(f"--save_state {G.save_state}: 0 (weights only) or 1 (also <logdir>/train_state.pt, for --resume)")
    if G.save_state and not hasattr(Model, "train_state"):
        raise ValueError(f"--save_state 1: the model {G.model!r} has no train_state() / load_train_state() to save and resume from")
    if G.resume != Path("."):
        state = train_state.read(G.resume)                             # missing file, unknown format, another world size: before the model exists
        if int(state["epoch"]) >= G.epochs:
            raise ValueError(f"{G.resume / train_state.FILE} holds the state after epoch {state['epoch']} and --epochs is {G.epochs}: "
                             f"nothing is left to train - extend the run with --epochs N, N > {state['epoch']}")


def _check_image_flags(G):
    """The flags of the picture and sample output, named before any model is built."""
    if G.save_images not in (0, 1):
        raise ValueError(f"--save_images {G.save_images}: 0 (no pictures) or 1 (PNG / APNG files under <logdir>/images)")
    if G.image_frames < 2:
        raise ValueError(f"--image_frames {G.image_frames}: at least 2 (an animation keeps the first and the last frame)")
    if G.dump_samples < 0:
        raise ValueError(f"--dump_samples {G.dump_samples}: 0 (off) or the number of samples to write after a checkpoint")


def _check_nn_flags(G, n_train=None):
    """The flags of the nearest-neighbour report, named before any model is built; with n_train (once the data is loaded) also against the
    training set's size."""
    if G.nn_eval < 0:
        raise ValueError(f"--nn_eval {G.nn_eval}: 0 (off) or the number Q >= 1 of samples to search neighbours for after a checkpoint")
    if not G.nn_eval:
        return
    if not 1 <= G.nn_k <= 8:
        raise ValueError(f"--nn_k {G.nn_k}: 1 .. 8 neighbours per sample")
    if not G.data_device:
        raise ValueError(f"--nn_eval {G.nn_eval} needs --data_device 1 (the search runs against the training set held on the GPU as bytes)")
    if G.binarize:
        raise ValueError(f"--nn_eval {G.nn_eval} needs --binarize 0 (samples and dataset bytes are compared as grey levels; a binarized model "
                         f"draws 0 / 1 images)")
    if n_train is not None and G.nn_k > n_train:
        raise ValueError(f"--nn_k {G.nn_k}: the training set has {n_train} images")


def _check_heavy_flags(G):
    """The flags of the heavy evaluation at scale, named before any model is built."""
    if G.eval_heavy_samples < 0:
        raise ValueError(f"--eval_heavy_samples {G.eval_heavy_samples}: 0 (the reference's 500 samples) or the number N >= 1 of samples to draw")
    if G.eval_heavy_samples and not 1 <= G.eval_heavy_k <= 8:
        raise ValueError(f"--eval_heavy_k {G.eval_heavy_k}: 1 .. 8 neighbours per ball")


def _check_posthoc_flags(G):
    """The flags of the power-function averages (models that have them), named before any model is built."""
    if "ema_sigma_rel" in G or "ema_snapshot_every" in G:
        from . import posthoc_ema
        posthoc_ema.check_flags(G.get("ema_sigma_rel", ""), G.get("ema_snapshot_every", 0))


def _device_datasets(G, device, rank, world):
    root = str(G.data_root)
    if G.data == "mnist":
        train, test = ((datasets.read_idx(datasets._find(root, img)), datasets.read_idx(datasets._find(root, lab)))
                       for img, lab in (datasets.FILES[True], datasets.FILES[False]))
    else:
        train, test = (datasets.load_cifar10 if G.data == "cifar10" else datasets.load_npy)(root)
    common_kw = dict(binarize=G.binarize, pad=2 if G.pad32 else 0, device=device, rank=rank, world=world)
    return (datasets.DeviceDataset(*train, G.bs, flip_p=G.flip_p, seed=1000, **common_kw),      # seeds as load_mnist's; flips on the train split only
            datasets.DeviceDataset(*test, G.bs, flip_p=0.0, seed=1001, **common_kw))


def _datasets(G, device):
    rank, world = parallel.rank(), parallel.world()
    _check_data_flags(G)
    if G.data_device:
        return _device_datasets(G, device, rank, world)
    if G.data == "mnist":          # gms/main.py:84 `load_mnist`
        return datasets.load_mnist(G.bs, G.binarize, G.pad32, root=str(G.data_root), device=device, seed=1000, rank=rank, world=world)
    if G.data == "synthetic":
        return (datasets.SyntheticMNIST(G.bs, G.train_batches, G.pad32, G.binarize, device, seed=1000 + rank),
                datasets.SyntheticMNIST(G.bs, G.test_batches, G.pad32, G.binarize, device, seed=2000 + rank))
    raise ValueError(f"--data {G.data!r}: 'synthetic' or 'mnist'")


def load_model_and_data(argv=None):
    """-> (model, train_ds, test_ds, autoencoder, classifier, G), the reference's call shape (gms/main.py:43-92)."""
    G, Model = FlagSpace(DG).resolve(argv)
    _check_data_flags(G)
    _check_image_flags(G)
    _check_nn_flags(G)
    _check_heavy_flags(G)
    _check_posthoc_flags(G)
    init_distributed()
    _check_resume_flags(G, Model)                                      # after init_distributed: the state file names its world size
    device = _run_device(G.device)
    model = Model(G=G).to(device)
    model.run_device = device
    resuming = G.resume != Path(".")
    if G.weights_from != Path(".") and not resuming:                   # a resumed run is built as its first start was; its weights come below
        model.load_state_dict(torch.load(G.weights_from, map_location=device), strict=False)
    if parallel.world() > 1 and hasattr(model, "net"):
        parallel.GradSync(model.net).broadcast_params(0)
    train_ds, test_ds = _datasets(G, device)
    if G.nn_eval:
        _check_nn_flags(G, int(train_ds.images.shape[0]))
    if parallel.rank() == 0:
        print("num_vars", common.count_vars(model))
    autoencoder, classifier = _feature_extractors(G, device, test_ds)
    if resuming:                                                       # last: everything above ran as at the first start, on fresh loaders
        model.load_state_dict(torch.load(G.resume / "model.pt", map_location=device))
        model.resumed_epoch = train_state.load(G.resume, model, train_ds, test_ds)
        if parallel.rank() == 0:
            print("RESUMED", G.resume, "AT EPOCH", model.resumed_epoch)
    return model, train_ds, test_ds, autoencoder, classifier, G


def train(model, train_ds, test_ds, autoencoder, classifier, G):
    """Evaluate-then-train epochs until `G.epochs`; returns the host-side metrics of the final evaluation pass."""
    return Session(model, train_ds, test_ds, autoencoder, classifier, G).run()


if __name__ == "__main__":
    train(*load_model_and_data())
