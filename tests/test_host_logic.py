"""CPU tests (no GPU): host logic of the plugin surface, the C-ABI library's exports, arena / bucket layout,
the multi-rank gradient exchange over gloo, and the rule that the product never touches the oracle."""
import ctypes
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import launch_trace  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def free_port():
    """A TCP port nobody listens on right now (bind to 0, read it back): fixed rendezvous ports collide between test runs."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return str(s.getsockname()[1])


def test_args_type_truth_table():
    """Restates gms/common.py:85-92."""
    from generative_models_amd.common import args_type
    assert args_type(True)("True") is True and args_type(False)("False") is False
    with pytest.raises(ValueError):
        args_type(True)("1")
    assert args_type(5)("7") == 7 and isinstance(args_type(5)("7"), int)
    assert args_type(5)("1e3") == 1000.0 and isinstance(args_type(5)("1e3"), float)
    assert args_type(5)("2.5") == 2.5
    assert args_type(Path("."))("~/x") == Path("~/x").expanduser()
    assert args_type(3e-4) is float and args_type("abc") is str


def test_registry_keys():
    """gms/common.py:33-35,38-55: snake-cased class name; `diffusion` alias (run_all.sh:16)."""
    from generative_models_amd import common
    assert common.convert_camel_to_snake("DiffusionModel") == "diffusion_model"
    assert common.convert_camel_to_snake("VQVAE") == "vqvae"
    assert common.convert_camel_to_snake("PixelCNN") == "pixel_cnn"
    models = common.discover_models()
    assert set(models) == {"diffusion_model", "diffusion"}
    M = models["diffusion_model"]
    assert issubclass(M, common.GM)
    ref_defaults = dict(binarize=0, timesteps=250, hidden_size=128, dropout=0.0, sampler="ddim", mean_type="v",
                        eval_heavy=1, class_cond=1, sample_cond_w=-1.0, cf_drop_prob=0.1, teacher_path=Path("."),
                        teacher_mode="step1", lr_scheduler="none")          # diffusion_model.py:15-29
    for k, v in ref_defaults.items():
        assert M.DG[k] == v, k


def test_make_plugin_on_foreign_base():
    """the same class can be built on the reference's own GM base."""
    from torch import nn
    from generative_models_amd.diffusion.diffusion_model import make_plugin

    class ForeignGM(nn.Module):
        def __init__(self, G):
            super().__init__()
            self.G = G

    class AD(dict):
        __setattr__ = dict.__setitem__
        __getattr__ = dict.__getitem__

    cls = make_plugin(ForeignGM, AD)
    assert issubclass(cls, ForeignGM) and cls.__name__ == "DiffusionModel" and cls.DG.timesteps == 250


def test_cabi_library_exports_every_declared_symbol():
    from generative_models_amd import _lib
    protos = _lib.parse_header()
    assert len(protos) >= 29
    dll = ctypes.CDLL(_lib.LIBPATH)
    for name in protos:
        assert hasattr(dll, name), name
    assert dll.gmk_version() == 1
    # argument errors are reported without touching a GPU
    rc = dll.gmk_colsum(None, ctypes.c_int64(4), None, 1, 1, 0, None)
    assert rc == -1
    _lib.lib.gmk_last_error.restype = ctypes.c_char_p
    assert b"gmk_colsum" in _lib.lib.gmk_last_error()
    assert _lib.lib.gmk_conv_wgrad_workspace_bytes(1024 * 784, 9, 128, 128) > 0
    assert _lib.lib.gmk_conv_wgrad_workspace_bytes(64, 9, 128, 100) == -1


def test_header_cites_reference_for_every_entry_point():
    text = open(os.path.join(ROOT, "include", "gmk.h")).read()
    assert text.count(".py:") >= 15


def test_param_inventory_and_arena():
    from generative_models_amd.diffusion.simple_unet import SimpleUnet, param_inventory
    inv = param_inventory(128)
    assert len(inv) == 160 and sum(int(np.prod(s)) for _, s in inv) == 6033665
    net = SimpleUnet(128)
    assert [k for k, _ in net.state_dict().items()] == [n for n, _ in inv]
    # zero-initialised out_layers.3 (simple_unet.py:172), GroupNorm affine 1/0
    assert float(net.param("turn.out_layers.3.weight").abs().max()) == 0.0
    assert float(net.param("out.0.weight").min()) == 1.0 and float(net.param("out.0.bias").abs().max()) == 0.0
    b = net.grad_buckets()
    assert sorted(b)[0][0] == 0 and sorted(b)[-1][1] == net.flat_params.numel()
    assert sum(e - s for s, e in b) == net.flat_params.numel()
    for name, _ in inv:                       # 16-byte alignment of every tensor in the arena
        assert net._offsets[name] % 4 == 0
    # parameters and grads are views of the arenas, and survive load_state_dict
    sd = {k: torch.full_like(v, 0.5) for k, v in net.state_dict().items()}
    net.load_state_dict(sd)
    assert float(net.flat_params[net._offsets["turn.in_layers.2.weight"]]) == 0.5 and net._packs_stale
    for bad in (48, 320, 512):                    # not a multiple of 32 / above 256
        with pytest.raises(ValueError):
            SimpleUnet(bad)
    # every other multiple of 32 up to 256 lives zero-padded in a 128- or 256-channel arena and speaks the reference's shapes at the
    # state-dict boundary (the reference takes any width, simple_unet.py:17)
    from oracle import unet_ref as U
    wide = SimpleUnet(256)
    for width in (32, 64, 96, 192):
        narrow = SimpleUnet(width)
        like = net if width <= 128 else wide
        assert narrow.hidden_size == width and narrow.channels == like.channels and narrow.flat_params.numel() == like.flat_params.numel()
        assert (narrow._g1, narrow._g2) == {32: (128, 64), 64: (64, 32), 96: (-3, -6), 192: (-6, -12)}[width]      # groups, or -(channels per group)
        spec = U.param_spec(width)
        sdn = narrow.state_dict()
        assert [(k, tuple(v.shape)) for k, v in sdn.items()] == [(k, tuple(s)) for k, s in spec]
        filled = {k: torch.full_like(v, 0.25) for k, v in sdn.items()}
        narrow.load_state_dict(filled)
        assert int((narrow.flat_params == 0.25).sum()) == sum(int(np.prod(s)) for _, s in spec)       # everything else is padding: zeros
        assert int((narrow.flat_params != 0).sum()) == int((narrow.flat_params == 0.25).sum())
        assert all(torch.equal(v, filled[k]) for k, v in narrow.state_dict().items())
        from generative_models_amd import common
        assert common.count_vars(narrow) == sum(int(np.prod(s)) for _, s in spec)
        if width in (32, 64):
            assert common.count_vars(narrow) == {32: 387137, 64: 1521793}[width]
    net3 = SimpleUnet(128, in_channels=3)
    assert sum(p.numel() for p in net3.parameters()) == 6038275


def test_cpu_use_fails_loudly():
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    net = SimpleUnet(128)
    with pytest.raises((RuntimeError, ValueError)):
        net.forward_hip(torch.zeros(1, 1, 8, 8), torch.zeros(1))


def test_sampler_index_arithmetic_bit_exact(golden):
    from generative_models_amd.diffusion.gaussian_diffusion import logsnr_schedule_cosine_host, sampler_times
    g = golden("schedule.npz")
    for steps in (4, 8, 200, 250, 1000):
        ut = np.array([sampler_times(i, steps)[0] for i in range(steps)], np.float32)
        us = np.array([sampler_times(i, steps)[1] for i in range(steps)], np.float32)
        assert ut.tobytes() == g[f"T{steps}_u_t"].tobytes() and us.tobytes() == g[f"T{steps}_u_s"].tobytes()
        lt = np.array([logsnr_schedule_cosine_host(u) for u in ut], np.float32)
        ref = g[f"T{steps}_logsnr_t"]
        assert np.all(np.abs(lt - ref) <= 2e-6 * np.maximum(1.0, np.abs(ref)))


def test_product_never_imports_the_oracle():
    pkg = Path(ROOT) / "generative_models_amd"
    for f in pkg.rglob("*.py"):
        text = f.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", text, flags=re.M), f
        assert "/root/reference" not in text, f
    for f in (pkg / "csrc").glob("*"):
        if f.suffix in (".hip", ".h", ".cpp"):
            assert "oracle" not in f.read_text()


def test_synthetic_data_source():
    from generative_models_amd.main import SyntheticMNIST
    ds = SyntheticMNIST(4, 2, pad32=1, binarize=0, device="cpu", seed=0)
    batches = list(ds)
    assert len(batches) == 2
    x, y = batches[0]
    assert x.shape == (4, 1, 32, 32) and x.dtype == torch.float32 and y.dtype == torch.int64
    assert float(x.min()) >= -1 and float(x.max()) <= 1 and float(x[:, :, :2].abs().max()) == 0.0   # pad32 pads with 0
    assert int(y.min()) >= 0 and int(y.max()) <= 9


_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from generative_models_amd import parallel
from generative_models_amd.diffusion.simple_unet import SimpleUnet
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
torch.manual_seed(r)
net = SimpleUnet(128)                        # CPU arena; only the exchange is exercised here
sync = parallel.GradSync(net)
sync.broadcast_params(0)
ref = [torch.zeros(1) for _ in range(w)]
dist.all_gather(ref, net.flat_params[123456:123457])
assert all(float(t) == float(ref[0]) for t in ref)
g_local = torch.arange(net.flat_grads.numel(), dtype=torch.float32) * (r + 1) * 1e-6
net.flat_grads.copy_(g_local)
for k in range(4):
    sync.hook(k)
sync.finish()
expect = torch.arange(net.flat_grads.numel(), dtype=torch.float32) * 1e-6 * sum(range(1, w + 1))
assert torch.allclose(net.flat_grads, expect, rtol=1e-6, atol=0), float((net.flat_grads - expect).abs().max())
# merged buckets (GMK_GRAD_BUCKETS=2): two all-reduces, issued when the LAST natural bucket of each pair is ready
sync2 = parallel.GradSync(net, buckets=2)
net.flat_grads.copy_(g_local)
order = []
for k in range(4):
    sync2.hook(k)
    order.append(len(sync2.works))
assert order == [0, 1, 1, 2], order
assert [k for k, _, _ in sync2.issued] == [1, 3]
sync2.finish()
assert torch.allclose(net.flat_grads, expect, rtol=1e-6, atol=0)
d = sync2.describe()
assert d["world"] == w and d["backend"] == "gloo" and sum(d["bucket_bytes"]) == 4 * net.flat_grads.numel() and len(d["bucket_bytes"]) == 2
# a step that raises between hook() and finish(): abort() drains what was issued and leaves the exchange reusable (round 4)
net.flat_grads.copy_(g_local)
sync.hook(0); sync.hook(1)
assert len(sync.works) == 2
sync.abort()
assert not sync.works and not sync.issued and not sync._carved
net.flat_grads.copy_(g_local)
for k in range(4):
    sync.hook(k)
sync.finish()
assert torch.allclose(net.flat_grads, expect, rtol=1e-6, atol=0)
sync.set_carve(0); sync.set_carve(8)          # no-ops on a CPU arena; must not raise between steps
assert parallel.configure_rccl_env() is None or os.environ.get("GMK_RCCL_CAP") == "1"      # the RCCL channel cap is opt-in
x = torch.arange(8.0)
assert parallel.shard_batch(x).tolist() == x[r * 8 // w:(r + 1) * 8 // w].tolist()
dist.destroy_process_group()
print("rank", r, "ok")
"""


def test_gradient_exchange_two_ranks_gloo(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(_WORKER)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", free_port(), str(script), ROOT]
    env = dict(os.environ, OMP_NUM_THREADS="2")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert r.stdout.count("ok") == 2


_FORCED_WORKER = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
import torch, torch.distributed as dist
from generative_models_amd import parallel
from generative_models_amd.diffusion.simple_unet import SimpleUnet
dist.init_process_group("gloo")
assert dist.get_world_size() == 1
net = SimpleUnet(128)                        # CPU arena; only the exchange is exercised here
g = torch.arange(net.flat_grads.numel(), dtype=torch.float32) * 1e-6
# unforced: one rank exchanges nothing
os.environ["GMK_FORCE_EXCHANGE"] = "0"
assert not parallel.exchanging()
sync = parallel.GradSync(net)
net.flat_grads.copy_(g)
for k in range(4):
    sync.hook(k)
assert not sync.works and not sync.issued
sync.finish()
# forced: the four buckets are all-reduced (a one-rank sum is the identity), in readiness order, tiling the arena
os.environ["GMK_FORCE_EXCHANGE"] = "1"
assert parallel.exchanging()
sync = parallel.GradSync(net)
for k in range(4):
    sync.hook(k)
assert [k for k, _, _ in sync.issued] == [0, 1, 2, 3] and len(sync.works) == 4
assert sum(e - s for _, s, e in sync.issued) == net.flat_grads.numel()
sync.finish()
assert [k for k, _, _, _ in sync.last_issued] == [0, 1, 2, 3] and not sync.works
assert torch.equal(net.flat_grads, g)
d = sync.describe()
assert d["world"] == 1 and d["forced"] and d["backend"] == "gloo"
dist.destroy_process_group()
print("forced one-rank exchange ok")
"""


def test_forced_exchange_with_one_rank_gloo(tmp_path):
    """`GMK_FORCE_EXCHANGE=1` (round 6): with ONE rank the bucketed exchange still runs - what lets RCCL execute on a one-GPU box
    (tests/test_gpu_ddp.py); here the host logic over gloo: nothing is issued unforced, four buckets in readiness order when forced, values unchanged."""
    script = tmp_path / "forced_worker.py"
    script.write_text(_FORCED_WORKER)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr",
           "127.0.0.1", "--master-port", free_port(), str(script), ROOT]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "GMK_FORCE_EXCHANGE")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(env, OMP_NUM_THREADS="2"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "forced one-rank exchange ok" in r.stdout


def test_mnist_idx_loader_and_transform(tmp_path):
    """Row N4: IDX reader + the reference's transform chain (gms/common.py:104-111) + shuffle / drop_last batching."""
    import numpy as np
    from generative_models_amd import data
    rng = np.random.default_rng(0)
    raw = tmp_path / "MNIST" / "raw"
    raw.mkdir(parents=True)
    imgs = {True: rng.integers(0, 256, (70, 28, 28), dtype=np.uint8), False: rng.integers(0, 256, (23, 28, 28), dtype=np.uint8)}
    labs = {True: rng.integers(0, 10, 70, dtype=np.uint8), False: rng.integers(0, 10, 23, dtype=np.uint8)}
    for train in (True, False):
        data.write_idx(raw / data.FILES[train][0], imgs[train])
        data.write_idx(raw / (data.FILES[train][1] + ".gz"), labs[train])          # gz and plain are both accepted
    assert np.array_equal(data.read_idx(raw / data.FILES[True][0]), imgs[True])
    with pytest.raises(ValueError):
        (tmp_path / "bad").write_bytes(b"\x01\x02\x03\x04rest")
        data.read_idx(tmp_path / "bad")
    # transform chain restated from the reference
    x8 = imgs[True]
    to_tensor = torch.from_numpy(x8).float().div(255).unsqueeze(1)
    assert torch.equal(data.transform(x8, binarize=True, pad32=False), (to_tensor > 0.5).float())
    ref = torch.nn.functional.pad(2 * to_tensor - 1, (2, 2, 2, 2))
    got = data.transform(x8, binarize=False, pad32=True)
    assert got.shape == (70, 1, 32, 32) and torch.equal(got, ref) and float(got[:, :, 0].abs().max()) == 0.0   # zero border
    # loaders: drop_last, every sample at most once per epoch, labels follow their images, epochs reshuffle
    tr, te = data.load_mnist(16, binarize=False, pad32=False, root=str(tmp_path), seed=3)
    assert len(tr) == 4 and len(te) == 1
    full = data.transform(imgs[True], False, False)
    seen = []
    for x, y in tr:
        assert x.shape == (16, 1, 28, 28) and y.dtype == torch.int64 and float(x.min()) >= -1 and float(x.max()) <= 1
        for xi, yi in zip(x, y):
            idx = int((full == xi).flatten(1).all(1).nonzero()[0])
            assert int(labs[True][idx]) == int(yi)
            seen.append(idx)
    assert len(set(seen)) == 64
    assert [int(i) for i in seen] != [int((full == xi).flatten(1).all(1).nonzero()[0]) for x, _ in tr for xi in x]
    # two ranks see disjoint shards of one permutation
    a = data.MnistLoader(str(tmp_path), True, 8, False, False, seed=5, rank=0, world=2)
    b = data.MnistLoader(str(tmp_path), True, 8, False, False, seed=5, rank=1, world=2)
    ia = {int((full == xi).flatten(1).all(1).nonzero()[0]) for x, _ in a for xi in x}
    ib = {int((full == xi).flatten(1).all(1).nonzero()[0]) for x, _ in b for xi in x}
    assert len(a) == 4 and not (ia & ib)
    with pytest.raises(FileNotFoundError):
        data.load_mnist(4, root=str(tmp_path / "nowhere"))


def test_write_grid_and_gridvid_match_the_einops_patterns():
    """gms/common.py:177-193: '(n1 n2) c h w -> c (n1 h) (n2 w)' and the 3-channel video with fps = min(T // 3, 60)."""
    from einops import rearrange, repeat
    from generative_models_amd import common

    class W:
        def add_image(self, tag, img, epoch): self.img = (tag, img, epoch)
        def add_video(self, tag, vid, epoch, fps): self.vid = (tag, vid, epoch, fps)

    w = W()
    x = torch.arange(25 * 28 * 28, dtype=torch.float32).reshape(25, 1, 28, 28)
    common.write_grid(w, "samples", x, 7)
    assert w.img[0] == "samples" and w.img[2] == 7
    assert torch.equal(w.img[1], rearrange(x, "(n1 n2) c h w -> c (n1 h) (n2 w)", n1=5, n2=5))
    t = torch.arange(9 * 25 * 28 * 28, dtype=torch.float32).reshape(9, 25, 1, 28, 28)
    common.write_gridvid(w, "sampling_process", t, 2)
    ref = repeat(rearrange(t, "t (n1 n2) c h w -> t c (n1 h) (n2 w)", n1=5, n2=5)[None], "b t c h w -> b t (repeat c) h w", repeat=3)
    assert torch.equal(w.vid[1], ref) and w.vid[3] == 3 and w.vid[0] == "sampling_process"
    with pytest.raises(AssertionError):
        common.write_grid(w, "samples", x[:24], 0)


def test_fid_and_precision_recall_vs_reference_goldens(golden):
    """Row N3: compute_fid / precision_recall_f1 against values produced by the reference's own function bodies
    (oracle/make_golden.py:gen_metrics executes gms/common.py:267-319 as they stand)."""
    from generative_models_amd import metrics
    g = golden("metrics.npz")
    real = torch.from_numpy(g["real"])
    for tag in ("near", "far", "mid"):
        gen = torch.from_numpy(g[f"gen_{tag}"])
        assert abs(metrics.compute_fid(gen.numpy(), real.numpy()) - float(g[f"fid_{tag}"])) < 1e-6 * max(1.0, float(g[f"fid_{tag}"]))
        for k in (1, 3):
            prf = metrics.precision_recall_f1(real=real, gen=gen, k=k)
            got = torch.stack([prf["precision"], prf["recall"], prf["f1"]])
            ref = torch.from_numpy(g[f"prf_{tag}_k{k}"])
            assert torch.equal(torch.isnan(got), torch.isnan(ref)) and torch.allclose(torch.nan_to_num(got), torch.nan_to_num(ref), atol=1e-6)
    assert np.isnan(metrics.compute_fid(real.numpy()[0], real.numpy()))            # the reference swallows failures into NaN


def test_eval_heavy_flow_and_metric_keys():
    """gms/main.py:95-149 with stand-in model / autoencoder / classifier: sample counts, label conventions, metric keys."""
    from collections import defaultdict
    from generative_models_amd import common, metrics
    calls = []

    class M:
        def sample(self, n, y=None):
            calls.append((n, None if y is None else y.clone()))
            g = torch.Generator().manual_seed(len(calls))
            return torch.randn((n, 1, 28, 28), generator=g).clamp(-1, 1)

    enc = lambda x: x.flatten(1)[:, :24] * 3
    clf = lambda x: x.flatten(1)[:, :10]
    ds = [(torch.rand(40, 1, 28, 28) * 2 - 1, torch.randint(0, 10, (40,))) for _ in range(30)]
    G = common.AttrDict(device="cpu", class_cond=1)
    logger = defaultdict(list)
    out = metrics.eval_heavy(logger, M(), ds, enc, clf, G, total_samples=100)
    assert len(calls) == 6                                          # 3 batches x (conditional + unconditional), stops at >= 100 samples
    assert all((y == -1).all() for _, y in calls[1::2]) and all((y >= 0).all() for _, y in calls[0::2])
    for key in ("fid", "precision", "recall", "f1", "cond_fid", "cond_precision", "cond_recall", "cond_f1", "classifier_loss"):
        assert f"eval/{key}" in logger and len(logger[f"eval/{key}"]) == 1, key
    assert set(out) >= {"fid", "cond_f1", "classifier_loss"}
    logger2 = defaultdict(list)
    metrics.eval_heavy(logger2, M(), ds, enc, None, common.AttrDict(device="cpu", class_cond=0), total_samples=50)
    assert "eval/cond_fid" not in logger2 and "eval/classifier_loss" not in logger2 and "eval/fid" in logger2


def test_builtin_feature_extractors_for_heavy_eval():
    """arbiters.py: the stand-ins that keep `--eval_heavy 1` running when the reference's TorchScript blobs are absent.  The random-feature
    encoder is deterministic and separates image populations (FID of a shifted population >> FID of a resample of the same one); the
    centroid classifier, fitted in closed form on labelled batches, recognises its classes and prefers the right label."""
    from collections import defaultdict
    from generative_models_amd import arbiters, common, metrics
    enc, enc2 = arbiters.RandomFeatureEncoder(), arbiters.RandomFeatureEncoder()
    g = torch.Generator().manual_seed(0)
    templates = F.interpolate(torch.randn(10, 1, 7, 7, generator=g), size=28, mode="bicubic", align_corners=False).clamp(-1, 1)
    def draw(n, shift=0.0):
        y = torch.randint(0, 10, (n,), generator=g)
        return (templates[y] + 0.15 * torch.randn(n, 1, 28, 28, generator=g) + shift).clamp(-1, 1), y
    x, y = draw(200)
    z = enc(x)
    assert z.shape == (200, 64) and torch.equal(z, enc2(x)) and len(list(enc.parameters())) > 0
    assert all(not p.requires_grad for p in enc.parameters())
    same = metrics.compute_fid(enc(draw(200)[0]).numpy(), z.numpy())
    far = metrics.compute_fid(enc(draw(200, shift=0.6)[0]).numpy(), z.numpy())
    assert np.isfinite(same) and far > 5 * same, (same, far)
    clf = arbiters.CentroidClassifier(arbiters.RandomFeatureEncoder()).fit([draw(100) for _ in range(4)])
    xt, yt = draw(200)
    logits = clf(xt)
    assert logits.shape == (200, 10) and float((logits.argmax(1) == yt).float().mean()) > 0.9
    assert float(F.cross_entropy(logits, yt)) < float(F.cross_entropy(logits, (yt + 1) % 10))
    # and through the heavy-eval flow
    class M:
        def sample(self, n, y=None):
            lab = torch.where(y < 0, torch.randint(0, 10, y.shape, generator=g), y)
            return (templates[lab] + 0.15 * torch.randn(n, 1, 28, 28, generator=g)).clamp(-1, 1)
    logger = defaultdict(list)
    out = metrics.eval_heavy(logger, M(), [draw(50) for _ in range(4)], enc, clf, common.AttrDict(device="cpu", class_cond=1), total_samples=150)
    # the stand-ins log under their OWN keys: nothing of this run may read as a reference-space number (advisor, round 3)
    assert np.isfinite(out["randfeat_fid"]) and 0.0 <= float(np.mean(out["centroid_classifier_loss"])) < 2.0 and "eval/randfeat_cond_f1" in logger
    assert not any(k in logger for k in ("eval/fid", "eval/precision", "eval/classifier_loss", "eval/cond_fid"))


def test_guidance_weight_policy_table():
    """gaussian_diffusion.py:246-257,271-278 as a truth table: {caller asked for guidance or not} x {--sample_cond_w -1 / 2.0}
    x {no teacher / teacher / teacher_test}."""
    from generative_models_amd.diffusion.gaussian_diffusion import resolve_guidance
    draw = torch.tensor([0.5, 3.0])
    R = lambda **kw: resolve_guidance(kw_cond_w=None, **kw)
    # no teacher: sample_cond_w wins whenever it is not -1, whether or not the caller passed cond_w (`evaluate` passes none)
    assert R(sample_cond_w=-1.0, net_cond_w=None, has_teacher=False, sampler="ddim") == (None, None, False)
    s, g, t = R(sample_cond_w=-1.0, net_cond_w=draw, has_teacher=False, sampler="ddim")
    assert s is None and g is draw and not t
    assert R(sample_cond_w=2.0, net_cond_w=None, has_teacher=False, sampler="ddim") == (None, 2.0, False)
    assert R(sample_cond_w=2.0, net_cond_w=draw, has_teacher=False, sampler="noisy") == (None, 2.0, False)
    assert R(sample_cond_w=None, net_cond_w=None, has_teacher=False, sampler="ddim") == (None, None, False)
    # distillation: the student is conditioned on the draw, never guided, sample_cond_w is ignored
    s, g, t = R(sample_cond_w=2.0, net_cond_w=draw, has_teacher=True, sampler="ddim")
    assert s is draw and g is None and not t
    assert R(sample_cond_w=-1.0, net_cond_w=None, has_teacher=True, sampler="ddim") == (None, None, False)
    # teacher_test: the teacher, guided by the student's weight; unguided when there is none
    s, g, t = R(sample_cond_w=-1.0, net_cond_w=draw, has_teacher=True, sampler="teacher_test")
    assert s is None and g is draw and t
    assert R(sample_cond_w=-1.0, net_cond_w=None, has_teacher=True, sampler="teacher_test") == (None, None, True)
    with pytest.raises(ValueError):
        R(sample_cond_w=-1.0, net_cond_w=None, has_teacher=False, sampler="teacher_test")
    # a cond_w the caller's partial already carried conditions the (undistilled) network and does not guide
    kw = torch.tensor([1.0, 1.0])
    s, g, t = resolve_guidance(sample_cond_w=-1.0, net_cond_w=None, kw_cond_w=kw, has_teacher=False, sampler="ddim")
    assert s is kw and g is None and not t


def test_bucket_merging():
    from generative_models_amd import parallel
    from generative_models_amd.diffusion.simple_unet import SimpleUnet
    net = SimpleUnet(128)
    nat = net.grad_buckets()
    n = net.flat_params.numel()
    for count in (1, 2, 4):
        groups = parallel.merge_buckets(nat, count)
        assert len(groups) == count and sum(e - s for s, e, _ in groups) == n
        assert [last for _, _, last in groups] == {1: [3], 2: [1, 3], 4: [0, 1, 2, 3]}[count]
    with pytest.raises(ValueError):
        parallel.merge_buckets(nat, 3)
    # the 12 conv1 biases ride with the embedding block at the front of the arena (second bias table of the emb_layers GEMM)
    o = [net._offsets[f"{b}.in_layers.2.bias"] for b in ("down.seq.1", "down.seq.2", "up.seq.6")]
    assert o[1] - o[0] == 128 and nat[3][0] == 0 and nat[3][0] <= o[0] < o[2] < nat[3][1]


def test_flag_space_layers_and_hps_roundtrip(tmp_path):
    """gms/main.py:43-76: driver table -> model DG -> command line; with --weights_from the saved hps.yaml replaces the model DG
    layer (and its model key selects the class), `full_cmd` is dropped, the command line still wins."""
    import yaml
    from generative_models_amd import common, main
    G, Model = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--bs", "8", "--epochs=1e1", "--timesteps", "4"])
    assert Model.__name__ == "DiffusionModel" and G.bs == 8 and G.epochs == 10.0 and G.timesteps == 4
    assert G.logdir == Path("logs") / "diffusion" and G.hidden_size == 128 and G.sample_cond_w == -1.0
    G2, _ = main.FlagSpace(main.DG).resolve(["--model=diffusion", "--logdir", str(tmp_path / "run")])
    assert G2.logdir == tmp_path / "run"                               # an explicit --logdir is used as is
    saved = dict(G)
    saved.update(full_cmd="python old", timesteps=7, model="diffusion_model", logdir=tmp_path / "ck")
    (tmp_path / "ck").mkdir()
    with open(tmp_path / "ck" / "hps.yaml", "w") as f:
        yaml.dump(saved, f, width=float("inf"))
    G3, M3 = main.FlagSpace(main.DG).resolve(["--weights_from", str(tmp_path / "ck" / "model.pt"), "--bs", "16"])
    assert M3 is Model and G3.timesteps == 7 and G3.bs == 16 and "full_cmd" not in G3 and G3.logdir == tmp_path / "ck"
    assert G3.weights_from == tmp_path / "ck" / "model.pt"


def test_epoch_log_keys_and_deferred_host_transfer():
    from generative_models_amd.main import EpochLog
    log = EpochLog("diffusion")
    log.add("train", {"loss": torch.tensor(2.0), "nlogp": torch.tensor(1.0)})
    log.add("train", {"loss": torch.tensor(4.0)})
    log.add("test", {"loss": torch.tensor(3.0), "nlogp": 0.5})
    log.set("dt/train", 1.5)
    host = log.to_host()
    assert host == {"diffusion/train/loss": [2.0, 4.0], "train/nlogp": [1.0], "diffusion/test/loss": [3.0], "eval/nlogp": [0.5],
                    "dt/train": 1.5}


def _rates_above_peak(rec, peak=None, depth=0, path=""):
    """Every {"achieved": A, "peak": P} block of a bench record and every `other_kernels` entry under a roofline block (which inherits the
    block's peak): A <= P."""
    bad = []
    if isinstance(rec, dict):
        pk = rec["peak"] if isinstance(rec.get("peak"), (int, float)) else (peak if depth > 0 else None)
        if isinstance(rec.get("achieved"), (int, float)) and isinstance(pk, (int, float)) and rec["achieved"] > pk:
            bad.append((path, rec["achieved"], pk))
        for k, v in rec.items():
            if k == "other_kernels":
                bad += _rates_above_peak(v, pk, 2, f"{path}/{k}")
            else:
                bad += _rates_above_peak(v, pk, depth - 1, f"{path}/{k}")
    return bad


def test_no_rate_above_its_peak_in_the_committed_bench_detail():
    """Round 5's detail record quoted 2,572 TFLOP/s for a sub-pixel kernel: the REFERENCE op's 36 tap-products divided by the time of a kernel that
    multiplies 16.  Since round 6 `achieved` counts the products the MFMAs form (`multiplied_tflops`), the reference count is `reference_tflops`
    (an effective rate), and no `achieved` of the newest committed record may exceed the `peak` it stands beside."""
    import glob
    import json
    assert _rates_above_peak({"roofline": {"achieved": 1.0, "peak": 2.0, "other_kernels": {"k": {"achieved": 3.0}}}}) == [("/roofline/other_kernels/k", 3.0, 2.0)]
    files = sorted(f for f in glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_detail.json")) if os.path.basename(f) >= "r06")
    for f in files:
        assert _rates_above_peak(json.load(open(f))) == [], f


def test_bench_line_stays_inside_the_drivers_window():
    """The driver parses the LAST stdout line of bench.py and keeps a bounded tail of stdout: round 3's 20 KB line was cut and the
    headline went unmeasured.  The compact line built from that very record (and from an N = 8 variant of it with the exchange block and
    its carve-out A/B) must stay under 4 KB and keep every field the measurement contract names."""
    import copy
    import json
    import bench
    full = json.load(open(os.path.join(ROOT, "profiles", "r03_bench.json")))
    assert len(json.dumps(full)) > 3 * bench.LINE_LIMIT                      # the canned record is the one that broke the parse
    full["cpu_baseline"]["cfg0_shape"] = {"value": 40.0, "sampler_steps_per_sec": 7.0, "sample": "oracle train step, B=32, 1x28x28, 9 steps in 9.0 s",
                                          "sampler_sample": "x" * 200}
    text = bench.compact_line(full, "gpurun_out/bench_detail.json")
    assert len(text) <= bench.LINE_LIMIT and "\n" not in text
    d = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
              "data", "config", "roofline", "cpu_baseline", "sampler", "other_configs"):
        assert k in d, k
    assert d["value"] == full["value"] and d["config"]["key"] == "cfg2" and d["vs_baseline"] is None
    r = d["roofline"]
    assert set(("bound", "achieved", "peak", "unit", "frac", "traffic")) <= set(r) and r["frac"] == full["roofline"]["frac"]
    assert r["hbm"]["kernel"].startswith("gn_silu") and r["hbm"]["peak"] == 8000.0
    assert set(("value", "unit", "cores", "kind", "sample")) <= set(d["cpu_baseline"]) and d["cpu_baseline"]["cfg0_shape"]["value"] == 40.0
    assert set(d["other_configs"]) == {"cfg1", "cfg3", "cfg4"} and d["other_configs"]["cfg3"]["frac"] > 0
    # N = 8: every per-config record carries an exchange block, the headline's has the A/B
    many = copy.deepcopy(full)
    many["n_gpus"] = 8
    many.pop("cpu_baseline")
    ex = {"world": 8, "backend": "nccl", "bucket_bytes": [6029312, 6029312, 6029312, 6046724], "persistent_kernel_cus": 248,
          "rccl_max_channels": None, "exposed_ms": 0.1234, "issue": "prose " * 40, "rccl_version": "2.22.3",
          "ab": {"carved": {"ms_per_step": 50.123, "exposed_ms": 0.1234, "persistent_kernel_cus": 248},
                 "uncarved": {"ms_per_step": 50.456, "exposed_ms": 1.2345, "persistent_kernel_cus": None}}}
    many["exchange"] = ex
    for o in many["other_configs"].values():
        o["exchange"] = dict(ex)
    text8 = bench.compact_line(many, "gpurun_out/bench_detail.json")
    d8 = json.loads(text8)
    assert len(text8) <= bench.LINE_LIMIT and d8["exchange"]["ab"]["uncarved"]["ms_per_step"] == 50.456 and "issue" not in d8["exchange"]
    assert d8["other_configs"]["cfg3"]["exposed_ms"] == 0.1234
    # a record that cannot fit sheds optional blocks instead of printing an unparseable line
    fat = copy.deepcopy(full)
    fat["other_configs"] = {f"cfg{i}": fat["other_configs"]["cfg1"] for i in range(60)}
    assert len(bench.compact_line(fat)) <= bench.LINE_LIMIT


def test_bench_arguments_and_output_dump(tmp_path):
    """`--steps` is the number of timed steps (at least one), `--dump-outputs DIR` writes fp32 .npy files: small arrays whole, and past the
    64 MB limit the large ones cut to one seeded set of positions, the same on every call and for every array of one length."""
    import bench
    a = bench.parse(["--steps", "7", "--warmup", "0", "--dump-outputs", str(tmp_path / "d")])
    assert a.steps == 7 and a.warmup == 0 and a.dump_outputs == str(tmp_path / "d")
    assert bench.parse([]).dump_outputs is None
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        with pytest.raises(SystemExit):
            bench.parse(bad)
    g = torch.Generator().manual_seed(1)
    arrays = {"loss": torch.tensor(0.25, dtype=torch.float64), "params": torch.randn(3000, 50, generator=g),
              "grads": torch.randn(150000, generator=g).to(torch.bfloat16)}
    w = bench.write_outputs(str(tmp_path / "whole"), arrays)
    assert w == {"loss": [[], False], "params": [[3000, 50], False], "grads": [[150000], False]}
    for k, t in arrays.items():
        f = np.load(tmp_path / "whole" / f"{k}.npy")
        assert f.dtype == np.float32 and np.array_equal(f, t.float().numpy())
    limit = 4 * 100000
    for d in ("cut1", "cut2"):
        w = bench.write_outputs(str(tmp_path / d), arrays, limit=limit)
        assert w == {"loss": [[], False], "params": [[49903], True], "grads": [[49903], True]}
        assert sum(os.path.getsize(tmp_path / d / f"{k}.npy") for k in arrays) <= limit
    p1, g1 = (np.load(tmp_path / "cut1" / f"{k}.npy") for k in ("params", "grads"))
    assert np.array_equal(p1, np.load(tmp_path / "cut2" / "params.npy")) and np.array_equal(g1, np.load(tmp_path / "cut2" / "grads.npy"))
    flat = arrays["params"].reshape(-1).numpy()
    idx = np.array([int(np.flatnonzero(flat == v)[0]) for v in p1[:200]])      # sampled values are entries of the array, in position order
    assert np.all(np.diff(idx) > 0)
    assert np.array_equal(g1[:200], arrays["grads"].float().numpy()[idx])  # the same positions in both arrays of one length


def test_bench_plain_run_measures_the_headline_alone(tmp_path, monkeypatch, capsys):
    """`bench.py --steps K --warmup W` runs the headline config and prints its line; the other configs, the fp32 modes and the CPU baseline
    run with `--full` only, after the headline, and the headline's own run is the same call in both modes."""
    import json
    import bench
    from generative_models_amd._lib import lib
    calls = []

    def run_config(self, key, spec, steps, warmup, headline, dtype=None, sampler=True):
        calls.append((key, steps, warmup, headline, dtype))
        return {"value": 100.0, "ms_per_step": 20.0, "workload": key, "baseline_entry": spec[4], "global_batch": spec[2]}

    def cpu(seconds, S, cin):
        calls.append(("cpu", S, cin))
        return {"value": 1.0, "sampler_steps_per_sec": 1.0, "sample": "s", "sampler_sample": "s"}

    monkeypatch.setattr(bench.Bench, "run_config", run_config)
    monkeypatch.setattr(bench, "cpu_baseline", cpu)
    monkeypatch.setattr(bench, "fp32_mode", lambda: ("fp32 storage, exact-fp32 MFMA", bench.MFMA_F32_PEAK_TFLOPS))
    monkeypatch.setattr(lib, "gmk_set_fp32_exact", lambda exact: 0)
    monkeypatch.setenv("GMK_BENCH_DETAIL", str(tmp_path / "detail.json"))
    lines = {}
    for mode, extra in (("plain", []), ("full", ["--full"])):
        b = object.__new__(bench.Bench)          # (no device: run_config is the stand-in above)
        b.a, b.world, b.rank = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"] + extra), 1, 0
        calls.clear()
        b.main()
        lines[mode] = (json.loads(capsys.readouterr().out.strip().splitlines()[-1]), list(calls))
    line, ran = lines["plain"]
    assert ran == [("cfg2", 7, 2, True, None)]
    assert (line["metric"], line["value"], line["unit"], line["higher_is_better"], line["ms_per_step"]) == ("ddpm_train_images_per_sec", 100.0, "images/s", True, 20.0)
    assert line["steps"] == 7 and line["warmup"] == 2 and line["dtype"] == "fp16_fwd+bf16_bwd"
    assert not {"other_configs", "cpu_baseline", "steady_state", "sampler"} & set(line)
    line, ran = lines["full"]
    assert ran[0] == ("cfg2", 7, 2, True, None) and ran[1:4] == [(k, 50, 10, False, None) for k in ("cfg1", "cfg3", "cfg4")]
    assert ran[4:6] == [("cfg2", 10, 3, False, "fp32")] * 2 and ran[6:] == [("cpu", 32, 3), ("cpu", 28, 1)]
    assert line["value"] == 100.0 and set(line["other_configs"]) == {"cfg1", "cfg3", "cfg4", "cfg2_fp32", "cfg2_fp32_split"}
    assert line["cpu_baseline"]["cfg0_shape"]["value"] == 1.0


def test_bench_launcher_branch_starts_ranks_without_touching_the_gpu():
    """Plain `python bench.py --gpus N` (no WORLD_SIZE: how the driver has called bench.py so far) must start its own N ranks as a child
    `torch.distributed.run`, from a process that has not initialised the GPU; with WORLD_SIZE set (the documented launcher form) or N = 1
    it must not."""
    import json
    import subprocess
    import bench
    ns = lambda n: type("A", (), {"gpus": n})()
    assert bench.needs_launcher(ns(8), {}) and bench.needs_launcher(ns(2), {"RANK": "0"})
    assert not bench.needs_launcher(ns(1), {}) and not bench.needs_launcher(ns(8), {"WORLD_SIZE": "8"})
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "7", "--warmup", "2"], capture_output=True,
                       text=True, timeout=300, env=dict(env, GMK_BENCH_LAUNCH_DRYRUN="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    assert d["cuda_initialized"] is False
    cmd = d["launch"]
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"] and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and int(cmd[cmd.index("--master-port") + 1]) > 0
    k = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[k + 1:] == ["--gpus", "4", "--steps", "7", "--warmup", "2"]
    # the child's exit code is the parent's: a launcher that cannot start its ranks must not look like a finished bench (the ranks see no
    # device, on a machine with a GPU too)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--no_cpu"],
                       capture_output=True, text=True, timeout=600, env=dict(env, GMK_DIST_BACKEND="gloo", OMP_NUM_THREADS="1",
                                                                             HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1"))
    assert r.returncode != 0 and "bench.py needs an MI355X" in r.stderr       # (no visible GPU: both ranks refuse, loudly)


def _device_asm(src_name):
    """gfx950 assembly of one kernel source (hipcc -S, device only), compiled from the tree into a temporary directory: a few seconds per file."""
    import shutil
    import tempfile
    csrc = os.path.join(ROOT, "generative_models_amd", "csrc")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    flags = re.search(r"^HIPFLAGS\s*[:+]?=\s*(.*)$", open(os.path.join(csrc, "Makefile")).read(), flags=re.M)
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, src_name + ".s")
        cmd = [hipcc] + (flags.group(1).split() if flags else ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off"])
        cmd = [c for c in cmd if c != "-fPIC"] + ["--cuda-device-only", "-S", os.path.join(csrc, src_name), "-o", out]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        return open(out).read().splitlines()


def _regs(operand_text):
    """VGPR numbers named in an instruction's operand text."""
    out = set()
    for a, b in re.findall(r"\bv\[(\d+):(\d+)\]", operand_text):
        out.update(range(int(a), int(b) + 1))
    out.update(int(a) for a in re.findall(r"\bv(\d+)\b", operand_text))
    return out


def _check_register_loads_in_flight(src, name_regex, n_instances, vm_per_step, min_consumed):
    """Mechanical check of COMPILED kernels whose producer waves keep inline-asm `buffer_load_dwordx4` results in C++ variables across barriers,
    retired only by a hand-counted `s_waitcnt vmcnt(N)` steps later (the compiler believes the registers are defined when the asm statement
    ends, so a copy, phi move or spill of a set before the wait would read stale VGPRs).  Over the control-flow graph of every instance:
      * no scratch memory, no VGPR / SGPR spills;
      * on EVERY path from a register load, no instruction reads or writes its destination registers while the load may still be in flight
        (in-order vmcnt: it has retired once a `vmcnt(N)` is crossed with at least N younger VMEM operations issued), and the first
        instruction that does read them is their consumer - the fp16 -> fp32 conversion of an activation chunk, or a `ds_write_b128`;
      * between two barriers of the steady-state loop exactly `vm_per_step` VMEM operations are issued on every path (the wait literal is
        vm_per_step x 3 steps)."""
    L = _device_asm(src)
    text = "\n".join(L)
    names = sorted(set(re.findall(r"^(_ZN\S*%s\S*):" % name_regex, text, flags=re.M)))
    assert len(names) == n_instances, names
    is_reg_load = lambda t: t.startswith("buffer_load_dwordx4 v[") and " lds" not in t
    is_vmem = lambda t: re.match(r"(buffer|global|flat)_(load|store|atomic)", t) is not None
    for name in names:
        m = re.search(r"\.name:\s+%s\n" % re.escape(name), text)
        lo, hi = text.rfind("  - .agpr_count", 0, m.start()), text.find("  - .agpr_count", m.end())
        blk = text[lo: hi if hi > 0 else len(text)]
        for key in ("private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count"):
            assert re.search(r"\.%s:\s+0\b" % key, blk), (name, key)
        s0 = next(i for i, l in enumerate(L) if l.startswith(name + ":"))
        e0 = next(i for i in range(s0, len(L)) if L[i].startswith(".Lfunc_end"))
        ins = [L[i].split(";")[0].strip() for i in range(s0 + 1, e0)]
        ins = [t for t in ins if t and (not t.startswith(".") or t.endswith(":"))]
        assert not any(t.startswith("scratch_") for t in ins), name
        labels = {t[:-1]: k for k, t in enumerate(ins) if t.endswith(":")}

        def sregs(op):
            m = re.match(r"s\[(\d+):(\d+)\]$", op)
            return {f"s{i}" for i in range(int(m.group(1)), int(m.group(2)) + 1)} if m else {op}

        def succ(k, known):
            """Successors of instruction k as (index, known) pairs.  The compiler emits the same scalar compare several times in a row in front
            of the loop exits of the unrolled steps (also through `s_mov` copies of the loop counter); following both edges of the later
            branches would walk paths no execution can take.  So the walk carries one fact: known = (compare opcode, registers equal to
            its left operand, registers equal to its right operand, outcome or None, SCC-still-holds-it).  VALU / memory instructions keep
            it, `s_mov_b32` extends the alias sets, any other scalar write drops its destination from them and (if it writes SCC) the link
            between the fact and the SCC bit."""
            t = ins[k]
            if t.startswith("s_endpgm"):
                return []
            if t.startswith("s_branch"):
                return [(labels[t.split()[-1]], known)]
            m = re.match(r"s_cbranch_scc([01]) (\S+)", t)
            if m:
                want, tgt = int(m.group(1)), labels[m.group(2)]
                if known and known[4] and known[3] is not None:
                    return [(tgt, known)] if known[3] == want else [(k + 1, known)]
                if known and known[4]:
                    return [(tgt, known[:3] + (want, True)), (k + 1, known[:3] + (1 - want, True))]
                return [(tgt, known), (k + 1, known)]
            if t.startswith("s_cbranch"):
                return [(k + 1, known), (labels[t.split()[-1]], known)]
            if t.startswith("s_cmp"):
                op, rest = t.split(None, 1)
                x, y = [o.strip() for o in rest.split(",")]
                if known and known[0] == op and x in known[1] and y in known[2]:
                    known = known[:4] + (True,)
                else:
                    known = (op, frozenset([x]), frozenset([y]), None, True)
            elif t.startswith("s_") and not re.match(r"s_(waitcnt|barrier|nop|sleep|setprio)", t) and known:
                op, rest = (t.split(None, 1) + [""])[:2]
                ops = [o.strip() for o in rest.split(",")] if rest else []
                dst = sregs(ops[0]) if ops else set()
                lhs, rhs = set(known[1]) - dst, set(known[2]) - dst
                if op == "s_mov_b32" and len(ops) == 2:
                    if ops[1] in known[1]:
                        lhs |= dst
                    if ops[1] in known[2]:
                        rhs |= dst
                holds = known[4] and bool(re.match(r"s_(mov_b32|mov_b64|load|buffer_load|mul_i32|cselect)", op))
                known = (known[0], frozenset(lhs), frozenset(rhs), known[3], holds) if lhs and rhs else None
            return [(k + 1, known)] if k + 1 < len(ins) else []

        loads = [k for k, t in enumerate(ins) if is_reg_load(t)]
        assert len(loads) >= 2 * vm_per_step, (name, len(loads))
        consumed = 0
        for k0 in loads:
            dest = _regs(ins[k0].split(",")[0])
            assert len(dest) == 4, ins[k0]
            seen, stack, hit, parent = set(), [(n, 0, False, kn) for n, kn in succ(k0, None)], False, {}

            def trace(st):           # the control-flow path that led here: branches, labels, waits, VMEM operations
                out = []
                while st is not None:
                    t = ins[st[0]]
                    if re.match(r"(buffer_|global_|s_waitcnt|s_barrier|s_c?branch|s_cmp)", t) or t.endswith(":"):
                        out.append(f"{st[0]}:{t} [younger {st[1]}]")
                    st = parent.get(st)
                return " <- ".join(out[:60])
            while stack:
                st = stack.pop()
                if st in seen:
                    continue
                seen.add(st)
                k, younger, retired, known = st
                t = ins[k]
                w = re.match(r"s_waitcnt .*vmcnt\((\d+)\)", t)
                if w and younger >= int(w.group(1)):
                    retired = True
                ops = t.split(None, 1)[1] if " " in t and not t.endswith(":") else ""
                if not t.endswith(":") and _regs(ops) & dest:
                    assert retired, (name, ins[k0], "touched while possibly in flight by", t, "path: " + trace(st))
                    # the consumers: the fp16 -> fp32 conversion of an activation chunk, the LDS write of a dY chunk (no conversion)
                    hit = hit or t.startswith("v_cvt_f32_f16") or t.startswith("ds_write_b128")
                    continue                                   # the value is consumed or dead behind this instruction
                if is_vmem(t):
                    younger = min(younger + 1, 63)
                for n, kn in succ(k, known):
                    nxt_st = (n, younger, retired, kn)
                    parent.setdefault(nxt_st, st)
                    stack.append(nxt_st)
            consumed += hit
        assert consumed >= min_consumed, (name, consumed)       # the steady-state loads of the 4 unrolled steps all reach their consumer
        # vm_per_step VMEM operations between two barriers of the steady-state loop, on every path
        bars = [k for k, t in enumerate(ins) if t == "s_barrier"]

        def to_next_barrier(b):
            found, seen, stack = set(), set(), [(n, 0, kn) for n, kn in succ(b, None)]
            while stack:
                st = stack.pop()
                k, n, known = st
                if st in seen or n > 16:
                    continue
                seen.add(st)
                if ins[k] == "s_barrier":
                    found.add((k, n)); continue
                stack.extend((x, n + is_vmem(ins[k]), kn) for x, kn in succ(k, known))
            return found
        nxt = {b: to_next_barrier(b) for b in bars}
        cyc = [b for b in bars if any(b in {k for k, _ in nxt[c]} for c in bars if c != b) and nxt[b]]      # barriers inside the loop
        steady = [b for b in cyc if all(k in cyc for k, _ in nxt[b])]
        assert len(steady) >= 4, (name, steady)
        loop_loads = set(loads[-2 * vm_per_step:])
        for b in steady:
            counts = {n for _, n in nxt[b]}
            # (the prologue's barrier-free issue blocks are not in `steady`: every one of these barriers is followed by another loop barrier)
            if any(ins[k] for k in range(b, min(b + 400, len(ins))) if k in loop_loads):
                assert counts == {vm_per_step}, (name, b, counts)


def test_wgrad_register_loads_stay_untouched_while_in_flight():
    """The advisor's medium finding of round 3 (csrc/conv_wgrad_slots.hip, kXF16 producers: activation AND dY chunks through registers since
    round 4; four VMEM operations per step, `vmcnt(12)`): LOOK in {1, 2} x kShare in {0, 1}, all with kXF16 = true - and the stride-2 four-plane
    form of round 6 (kS2: eight blocks in flight, `vmcnt(28)`, eight unrolled steps)."""
    _check_register_loads_in_flight("conv_wgrad_slots.hip", r"conv_wgrad_slots_ws_kernelILi\dELb1ELb[01]ELb[01]E", 5, 4, 16)


def test_subpixel_wgrad_register_loads_stay_untouched_while_in_flight():
    """The same guard for the sub-pixel `Upsample` weight gradient (csrc/conv_wgrad_subpixel.hip, round 5): one activation chunk and two dY
    parity streams through registers - six VMEM operations per step, `vmcnt(18)` - with fp16 and with bf16 activations."""
    _check_register_loads_in_flight("conv_wgrad_subpixel.hip", r"conv_wgrad_subpixel_ws_kernelILb[01]E", 2, 6, 24)


def test_counter_records_are_keyed_per_template_instantiation():
    """tools/kernel_names.py (the round-4 verdict's item 4a): the 3x3 halo kernel's instantiations do different work per launch (fp16 forward, bf16
    data gradient, folded skip convolution, in-convolution GroupNorm) and so do the sub-pixel kernel's modes - each gets its own counter record;
    rocprofv3 prints some names demangled (bf16 garbled as "bool _Accum, bool, E") and some mangled."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from kernel_names import instantiation, short
    finally:
        sys.path.pop(0)
    cases = {
        "void (anonymous namespace)::conv3x3_halo_ws_kernel<bool _Accum, bool, E, 16, false, false>((anonymous namespace)::HaloParams)": "conv3x3_halo_ws_kernel<bf16>",
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16_Lb1ELi16ELb0ELb0EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<f16>",
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16_Lb1ELi16ELb0ELb1EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<f16,+skip>",
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16_Lb1ELi16ELb1ELb0EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<f16,+gn>",
        "_ZN12_GLOBAL__N_123conv_subpixel_ws_kernelIDF16_Li0EEEvNS_9SubParamsE": "conv_subpixel_ws_kernel<f16,upsample>",
        "_ZN12_GLOBAL__N_123conv_subpixel_ws_kernelIDF16bLi2EEEvNS_9SubParamsE": "conv_subpixel_ws_kernel<bf16,upsample dgrad>",
        # a demangled bf16 name whose mode literal rocprofv3 garbled is NOT guessed any more (round 6; it was taken for "transposed", wrong for bf16
        # activations): the counter passes run with --mangled-kernels
        "void (anonymous namespace)::conv_subpixel_ws_kernel<bool _Accum, int, E>((anonymous namespace)::SubParams)": "conv_subpixel_ws_kernel<bf16,?>",
        "_ZN12_GLOBAL__N_123conv_subpixel_ws_kernelIDF16bLi1EEEvNS_9SubParamsE": "conv_subpixel_ws_kernel<bf16,transposed>",
        # round 6's template parameters (kStamp, kMerge, kRes, kRing4; a negative literal is mangled Lin1E): same keys
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16_Lb1ELi16ELb0ELb0ELb0ELb0ELi0ELb1EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<f16>",
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16bLb1ELi16ELb0ELb0ELb0ELb0ELi1ELb0EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<bf16>",
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16_Lb1ELi16ELb0ELb1ELb0ELb1ELi0ELb0EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<f16,+skip>",
        "_ZN12_GLOBAL__N_122conv3x3_halo_ws_kernelIDF16_Lb1ELi16ELb1ELb0ELb0ELb0ELin1ELb0EEEvNS_10HaloParamsE": "conv3x3_halo_ws_kernel<f16,+gn>",
    }
    for name, want in cases.items():
        assert instantiation(name) == want, (name, instantiation(name))
        assert short(name) == want.split("<")[0]
    assert instantiation("_ZN12_GLOBAL__N_125gn_silu_bwd_hybrid_kernelIDF16_Li8ELi512ELi4ELi8ELi0ELb1EEEvPKDF16bPKT_") is None
    assert short("void (anonymous namespace)::wgrad_reduce_kernel<4>(float const*, float*, int, int, int, int)") == "wgrad_reduce_kernel"


@pytest.fixture(scope="module")
def gn_launch_trace():
    """tools/gn_launch_trace.cpp against the tree's gn_silu.hip (about half a minute)"""
    return launch_trace.build("gn_launch_trace", ("gn_silu", "gmk_common"))


@pytest.fixture(scope="module")
def conv_launch_trace():
    """tools/conv_launch_trace.cpp against the tree's six convolution sources (a minute or two)"""
    return launch_trace.build("conv_launch_trace", launch_trace.CONV_SOURCES)


@pytest.fixture(scope="module")
def smallconv_launch_trace():
    """tools/smallconv_launch_trace.cpp against the tree's smallconv.hip (under a minute)"""
    return launch_trace.build("smallconv_launch_trace", launch_trace.SMALLCONV_SOURCES)


def test_groupnorm_dispatch_landmarks(gn_launch_trace):
    """The plan rows that the comments of csrc/gn_silu.hip and DESIGN.md quote, read off the host dispatch itself (C = 128, 32 groups, B = 2;
    16-bit = fp16 activations beside bf16 gradients): which instantiation, how many threads, how much LDS - and that gmk_gn_stats and the two
    pair predicates follow the same plans."""
    rows = {}
    for line in gn_launch_trace("landmarks"):
        head, _, tail = line.partition(" -> ")
        f = dict(kv.split("=", 1) for kv in (head.split()[1:] + re.sub(r'err="[^"]*"', "", tail).split()) if "=" in kv)
        f["kernel"] = int(f["kernel"])
        rows[(head.split()[0], int(f.get("dtype", f.get("grad_dtype", -1))), int(f.get("x_dtype", -1)), int(f["HW"]))] = f
        assert "no-metadata" not in tail
    from generative_models_amd._lib import K
    F32, BF16, F16 = 0, 1, 2
    ints = lambda name: [int(v) for v in re.findall(r"L[ib](\d+)E", name)]
    reg = {256: ([4, 8], 512), 784: ([14, 8], 448), 1024: ([16, 8], 512), 4096: ([16, 4], 1024)}
    hyb = {256: ([4, 256, 4, 4, 0, 0], 16 << 10), 784: ([13, 256, 4, 13, 0, 0], 49 << 10), 1024: ([8, 512, 4, 8, 0, 1], 64 << 10),
           4096: ([32, 512, 4, 28, 13, 1], 152 << 10)}
    for HW in (64, 256, 784, 1024, 4096):
        fwd, st, bwd = rows[("gn_silu_fwd", F16, -1, HW)], rows[("gn_stats", F16, -1, HW)], rows[("gn_silu_bwd", BF16, F16, HW)]
        assert fwd["rc"] == st["rc"] == bwd["rc"] == "0"
        if HW == 64:        # 8 x 8: the whole-sample streaming kernels
            assert fwd["kernel"] == K.GN_FWD and "gn_silu_fwd_kernelIDF16_Lb0E" in fwd["launch"] and fwd["block"] == "256,1,1" and fwd["grid"] == "2,1,1"
            assert bwd["kernel"] == K.GN_BWD and "gn_silu_bwd_kernelIDF16bDF16_E" in bwd["launch"] and bwd["lds"] == "0"
        else:
            assert fwd["kernel"] == K.GN_FWD_REG and "gn_silu_fwd_reg_kernelIDF16_" in fwd["launch"]
            assert (ints(fwd["launch"]), int(fwd["block"].split(",")[0])) == reg[HW]
            assert fwd["grid"] == "%d,1,1" % (2 * 128 // (8 * reg[HW][0][1]))
            assert bwd["kernel"] == K.GN_BWD_HYBRID and "gn_silu_bwd_hybrid_kernelIDF16_" in bwd["launch"]
            assert (ints(bwd["launch"]), int(bwd["lds"])) == hyb[HW] and bwd["block"] == "%d,1,1" % hyb[HW][0][1] and bwd["grid"] == "8,1,1"
            assert ("attr" in bwd) == (HW == 4096)      # only the 152 KiB form raises the kernel's LDS limit
        # the statistics pass picks the forward's row: same instantiation, same geometry (and the bf16 one its bf16 twin)
        assert (st["kernel"], st["launch"], st["grid"], st["block"]) == (fwd["kernel"], fwd["launch"], fwd["grid"], fwd["block"])
        st_bf = rows[("gn_stats", BF16, -1, HW)]
        assert (st_bf["launch"], st_bf["grid"], st_bf["block"]) == (fwd["launch"].replace("DF16_", "DF16b"), fwd["grid"], fwd["block"])
        # fp32 always streams
        f32, b32 = rows[("gn_silu_fwd", F32, -1, HW)], rows[("gn_silu_bwd", F32, F32, HW)]
        assert f32["kernel"] == K.GN_FWD and "gn_silu_fwd_kernelIfLb0E" in f32["launch"] and b32["kernel"] == K.GN_BWD and "gn_silu_bwd_kernelIffE" in b32["launch"]
        assert rows[("gn_pair_fwd_ok", F16, -1, HW)]["rc"] == ("1" if HW == 256 else "0")
        assert rows[("gn_pair_ok", BF16, F16, HW)]["rc"] == ("1" if HW in (256, 1024) else "0")
        assert rows[("gn_pair_ok", F16, F16, HW)]["rc"] == "0"      # fp16 gradients: never


def test_conv_dispatch_landmarks(conv_launch_trace):
    """The routes that the comments of the convolution sources and DESIGN.md quote, read off the host dispatch itself (C = 128, B = 2048, fp16
    activations beside bf16 gradients, and the fp32 twin, at the U-Net's 8 x 8 ... 64 x 64): which kernel and instantiation, the id
    gmk_last_kernel reports, and that the three predicates answer 1 exactly where the matching launch takes that route."""
    rows = {}
    for line in conv_launch_trace("landmarks"):
        assert "no-metadata" not in line
        head, _, tail = line.partition(" -> ")
        words = head.split()
        call = dict(kv.split("=", 1) for kv in words[1:] if "=" in kv)
        f = dict(kv.split("=", 1) for kv in re.sub(r'err="[^"]*"', "", tail).split() if "=" in kv)      # rc, kernel, and the last launch's grid / block
        f["launches"] = re.findall(r"launch=(\S+)", tail)
        f["kernel"] = int(f["kernel"])
        tag = words[1] if "=" not in words[1] else ""
        rows[(words[0], tag, int(call.get("dtype", -1)), call["grid"])] = f
    from generative_models_amd._lib import K
    F32, BF16, F16 = 0, 1, 2
    # template arguments after the type: conv3x3_halo_ws_kernel<T, prefetch, shape, fuse, skip, stamp, merge, res, ring4>
    targs = lambda name: [int(v.replace("n", "-")) for v in re.findall(r"L[ib](n?\d+)E", name)]
    for S in (8, 16, 32, 64):
        g, half = "%dx%d" % (S, S), "%dx%d" % (S // 2, S // 2)
        ring4 = S < 64                                   # a tile's halo within 384 slots
        for dt, ty in ((F16, "DF16_"), (BF16, "DF16b")):
            for tag, want in (("plain", [1, 16, 0, 0, 0, 0, 0, int(ring4)]), ("two-sources", [1, 16, 0, 0, 0, 0, 0, int(ring4)]), ("residual", [1, 16, 0, 0, 0, 0, 1, 0]),
                              ("upsample", [1, 16, 0, 0, 0, 0, 0, int(ring4)])):
                r = rows[("conv_igemm", tag, dt, g)]
                assert (r["rc"], r["kernel"], r["block"]) == ("0", K.CONV_HALO_WS, "512,1,1") and len(r["launches"]) == 1, (tag, dt, S, r)
                assert "conv3x3_halo_ws_kernelI" + ty in r["launches"][0] and targs(r["launches"][0]) == want, (tag, dt, S, r["launches"])
            # the stride-2 convolution: im2col (LDS-DMA from 256 x 512 rows)
            r = rows[("conv_igemm", "stride2", dt, half)]
            assert (r["kernel"], "conv_igemm_dma_kernelI" + ty in r["launches"][0]) == ((K.CONV_IGEMM_DMA, True) if S > 8 else (K.CONV_IGEMM, False)), (dt, S, r)
            # its data gradient: the sub-pixel kernel where the low-resolution grid fits a halo tile, else the halo kernel on the zero-stuffed source;
            # under GMK_CONV_KERNEL=2 four parity phases of the LDS-DMA kernel
            r = rows[("conv_igemm", "transposed", dt, g)]
            if S > 8:
                assert r["kernel"] == K.CONV_SUBPIXEL_TRANSPOSED and r["launches"] == [next(n for n in r["launches"] if "conv_subpixel_ws_kernelI" + ty + "Li1E" in n)], (dt, S, r)
            else:
                assert r["kernel"] == K.CONV_HALO_STUFFED and "conv3x3_halo_ws_kernelI" + ty in r["launches"][0] and targs(r["launches"][0])[6] == 1, (dt, S, r)
            r = rows[("conv_igemm", "transposed-choice2", dt, g)]
            assert r["kernel"] == K.CONV_DMA_PHASES and len(r["launches"]) == 4 and all("conv_igemm_dma_kernelI" + ty in n for n in r["launches"]), (dt, S, r)
            # Upsample in its sub-pixel form, and the predicate that offers it
            r, ok = rows[("conv_subpixel", "", dt, g)], rows[("conv_subpixel_ok", "", dt, g)]["rc"]
            assert ok == ("1" if S > 8 else "0") and (r["rc"] == "0") == (ok == "1"), (dt, S, r, ok)
            if ok == "1":
                assert r["kernel"] == K.CONV_SUBPIXEL_UPSAMPLE and "conv_subpixel_ws_kernelI" + ty + "Li0E" in r["launches"][0], (dt, S, r)
            # conv2 with the folded 1x1 skip: +skip, merged sub-phases up to 32 x 32
            r, ok = rows[("conv3x3_skipfold", "", dt, g)], rows[("conv3x3_skipfold_ok", "", -1, g)]["rc"]
            assert ok == "1" and r["rc"] == "0" and r["kernel"] == K.CONV_HALO_SKIPFOLD, (dt, S, r)
            assert "conv3x3_halo_ws_kernelI" + ty in r["launches"][0] and targs(r["launches"][0]) == [1, 16, 0, 1, 0, int(S < 64), 0, 0], (dt, S, r["launches"])
            r = rows[("conv1x1_pair", "", dt, g)]
            assert r["kernel"] == K.CONV1X1_PAIR_STREAM and "conv1x1_pair_stream_kernelI" + ty in r["launches"][0] and r["grid"] == "256,1,1", (dt, S, r)
        # the fused GroupNorm-apply and its predicate
        r, ok = rows[("conv_igemm", "gn", F16, g)], rows[("conv_gn_fusable", "", -1, g)]["rc"]
        assert ok == ("1" if S > 8 else "0") and (r["rc"] == "0") == (ok == "1"), (S, r, ok)
        if ok == "1":
            assert r["kernel"] == K.CONV_HALO_WS and targs(r["launches"][0]) == [1, 16, 1, 0, 0, 0, -1, 0], (S, r)
        # weight gradients, bf16 beside fp16 activations: slots for the 3x3 forms (the 128-slot window at 64 x 64, four planes for stride 2), a stream for the skip
        slot = lambda look, share, s2: "conv_wgrad_slots_ws_kernelILi%dELb1ELb%dELb%dEE" % (look, share, s2)
        look = 2 if S == 64 else 1
        for tag, grid, kernel, name in (("3x3", g, K.CONV_WGRAD_SLOTS_WS, slot(look, 1, 0)), ("3x3-two-sources", g, K.CONV_WGRAD_SLOTS_WS, slot(look, 1, 0)),
                                        ("upsample", g, K.CONV_WGRAD_SLOTS_WS, slot(look, 0, 0)),
                                        ("stride2", half, K.CONV_WGRAD_SLOTS_S2 if S > 8 else K.CONV_WGRAD, slot(1, 1, 1) if S > 8 else "conv_wgrad_kernelIDF16bDF16_Lb0EE"),
                                        ("skip-1x1", g, K.CONV1X1_WGRAD_STREAM, "conv1x1_wgrad_stream_kernelIDF16_E")):
            r = rows[("conv_wgrad", tag, BF16, grid)]
            assert r["rc"] == "0" and r["kernel"] == kernel and name in r["launches"][0] and "wgrad_reduce_kernel" in r["launches"][1], (tag, S, r)
        assert rows[("conv_wgrad_subpixel_ok", "", -1, g)]["rc"] == "1"
        r = rows[("conv_wgrad_subpixel", "", -1, g)]
        assert r["kernel"] == K.CONV_WGRAD_SUBPIXEL and "conv_wgrad_subpixel_ws_kernelILb1EE" in r["launches"][0] and len(r["launches"]) == 3, (S, r)
        # the fp32 twin: im2col everywhere (the register-staged kernel where a buffer passes 2^32 bytes), phases for the transposed form, no halo family
        big = S == 64
        for tag in ("plain", "residual", "two-sources", "upsample"):
            r = rows[("conv_igemm", tag, F32, g)]
            assert r["kernel"] == (K.CONV_IGEMM if big else K.CONV_IGEMM_DMA) and ("conv_igemm_kernelIfLb0E" if big else "conv_igemm_dma_kernelIfLb0E") in r["launches"][0], (tag, S, r)
        r = rows[("conv_igemm", "transposed", F32, g)]
        assert (r["kernel"], len(r["launches"])) == ((K.CONV_IGEMM, 1) if big else (K.CONV_DMA_PHASES, 4)), (S, r)
        assert rows[("conv_subpixel", "", F32, g)]["rc"] == "-1" and rows[("conv_subpixel_ok", "", F32, g)]["rc"] == "0"
        assert rows[("conv3x3_skipfold", "", F32, g)]["rc"] == "-1"
        assert rows[("conv1x1_pair", "", F32, g)]["kernel"] == (K.CONV_IGEMM if big else K.CONV_IGEMM_DMA)
        for tag, grid in (("3x3", g), ("stride2", half), ("upsample", g), ("skip-1x1", g)):
            r = rows[("conv_wgrad", tag, F32, grid)]
            assert r["kernel"] == K.CONV_WGRAD and "conv_wgrad_kernelIffLb0E" in r["launches"][0], (tag, S, r)


# ops.KERNEL_NAMES as it stood when the table moved into include/gmk.h: bench.py's KERNEL_DESC and tools/kernel_names.py key on these strings
_FROZEN_KERNEL_NAMES = {
    1: "conv_igemm_kernel", 2: "conv_igemm_dma_kernel", 3: "conv3x3_halo_kernel", 4: "conv3x3_halo_ws_kernel",
    5: "conv3x3_halo_ws_kernel[zero-stuffed transposed conv]", 6: "conv_igemm_dma_kernel[stride-2 dgrad phases]", 7: "conv3x3_halo_ws_kernel[+1x1 skip]",
    8: "conv_subpixel_ws_kernel[upsample]", 9: "conv_subpixel_ws_kernel[transposed]", 10: "conv_subpixel_ws_kernel[upsample dgrad]", 11: "conv_wgrad_kernel",
    12: "conv_wgrad_slots_kernel", 13: "conv_wgrad_slots_ws_kernel", 14: "conv1x1_pair_stream_kernel", 15: "conv1x1_wgrad_stream_kernel",
    16: "conv_wgrad_subpixel_ws_kernel", 17: "conv_wgrad_slots_ws_kernel[stride-2 planes]", 21: "gn_silu_fwd_reg_kernel", 22: "gn_silu_fwd_kernel",
    23: "gn_silu_bwd_hybrid_kernel", 24: "gn_silu_bwd_kernel", 25: "gn_silu_bwd_pair_kernel", 26: "gn_silu_fwd_pair_kernel"}
_SMALLCONV_KERNELS = ["expand3x3_kernel", "expand3x3_mfma_kernel", "expand3x3_tile16_kernel", "wgrad3x3_kernel", "wgrad3x3_mfma_kernel",
                      "wgrad3x3_tile16_kernel", "head_fwd_kernel", "head_fwd_mfma_kernel", "stem_dgrad_kernel", "stem_dgrad_mfma_kernel"]


def test_kernel_table_is_the_library_s_and_keeps_the_profile_names():
    """include/gmk.h's GMK_KERNEL_TABLE as _lib parses it: distinct ids, names and symbols; gmk_kernel_name (generated from the same list) agrees
    on every id and answers NULL for 0 and for unused numbers; ids 1 - 17 and 21 - 26 keep their numbers and names; 31 on are the ten device
    functions of smallconv.hip.  The integer constants ops takes from the header are there."""
    from generative_models_amd import _lib
    rows = _lib.parse_kernel_table()
    ids, names = [kid for _, kid, _ in rows], [name for _, _, name in rows]
    assert len(set(ids)) == len(set(names)) == len({sym for sym, _, _ in rows}) == len(rows) and all(names) and min(ids) > 0
    assert vars(_lib.K) == {sym: kid for sym, kid, _ in rows}
    for _, kid, name in rows:
        assert _lib.lib.gmk_kernel_name(kid) == name.encode() and _lib.kernel_name(kid) == name
    for kid in (0, -1, 18, 20, 27, 30, max(ids) + 1):
        assert kid not in ids and _lib.lib.gmk_kernel_name(kid) is None and _lib.kernel_name(kid) is None
    table = dict(zip(ids, names))
    assert {kid: table[kid] for kid in table if kid < 31} == _FROZEN_KERNEL_NAMES
    assert [table[kid] for kid in sorted(table) if kid >= 31] == sorted(_SMALLCONV_KERNELS, key=_SMALLCONV_KERNELS.index) and min(k for k in table if k >= 31) == 31
    src = open(os.path.join(ROOT, "generative_models_amd", "csrc", "smallconv.hip")).read()
    for name in _SMALLCONV_KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % name, src), name
    assert _lib.C["GMK_PROFILE_BINS"] == 64 and _lib.C["GMK_ERR_ARG"] == -1 and _lib.C["GMK_CONV_TRANSPOSED2"] == 3


def test_reported_kernel_is_the_launched_kernel(gn_launch_trace, conv_launch_trace):
    """Every successful launching line of the GroupNorm and convolution landmark traces: the name gmk_kernel_name gives for the reported id
    is a kernel that the line launched - no exception on these lines.  (Over the tool's whole sweep one pair breaks it, as it did before the
    table: GMK_CONV_KERNEL=3 with GMK_DEV_VARIANT 3 runs the zero-stuffed transposed convolution on conv3x3_halo_kernel and reports
    CONV_HALO_STUFFED, the id tests/test_gpu_ops.py expects there; the weight-pack entries report nothing and are behind no profile label.)"""
    from generative_models_amd._lib import kernel_name
    n_gn = launch_trace.check_reported_kernels(gn_launch_trace("landmarks"), kernel_name)
    n_conv = launch_trace.check_reported_kernels(conv_launch_trace("landmarks"), kernel_name)
    assert (n_gn, n_conv) == (30, 157)


def test_smallconv_reports_what_it_launches(smallconv_launch_trace):
    """The six stem / head entry points over every storage type each accepts, C = 128 / 256, 1 - 4 image channels, five grids and
    GMK_DEV_VARIANT 0 / 41 / 42 (B = 2): every call launches, reports an id, and the id's name is the kernel launched - no exception; and
    the landmark table, written from the launchers' conditions, names the same kernels."""
    from generative_models_amd._lib import kernel_name
    lines = smallconv_launch_trace("all")
    assert len(lines) == 3 * 2 * 4 * 5 * (3 + 2 + 3 + 2 + 3 + 3) == 1920
    assert all(" -> rc=0 " in line and " launch=" in line and "no-metadata" not in line for line in lines)
    assert launch_trace.check_reported_kernels(lines, kernel_name) == 1920
    got = {}
    for line in lines:
        head, _, tail = line.partition(" -> ")
        f = dict(kv.split("=", 1) for kv in head.split()[1:])
        H, W = (int(v) for v in f["grid"].split("x"))
        got[(head.split()[0], int(f["dtype"]), int(f["C"]), int(f["cs"]), H, W, int(f["variant"]))] = kernel_name(int(re.findall(r'" kernel=(\d+)', tail)[-1]))
    assert len(got) == 1920 and set(got.values()) == set(_SMALLCONV_KERNELS)
    for case, name in launch_trace.SMALLCONV_LANDMARKS.items():
        assert got[case] == name, (case, got[case], name)


def _smallconv_rows(lines):
    """trace lines -> [(entry, call fields, rc, error text, kernel id, [launch fields: name, grid, block, lds, args (explicit arguments as little-endian ints)])]"""
    rows = []
    for line in lines:
        head, _, tail = line.partition(" -> ")
        f = dict(kv.split("=", 1) for kv in head.split()[1:])
        launches = []
        for text in tail.split(" launch=")[1:]:
            w = dict(kv.split("=", 1) for kv in ("name=" + text).split())
            w["args"] = [int.from_bytes(bytes.fromhex(a.split(":")[1]), "little") for a in w["args"].split(",")]
            launches.append(w)
        rc, err, kid = re.match(r'rc=(-?\d+) err="(.*)" kernel=(-?\d+)', tail).groups()
        rows.append((head.split()[0], f, int(rc), err, int(kid), launches))
    return rows


def test_smallconv_sweeps_launch_every_instantiation(smallconv_launch_trace):
    """Every expand3x3_*, wgrad3x3_*, head_fwd* and stem_dgrad* kernel in the code object of smallconv.hip is launched by at least one line of
    the tool's two sweeps (`all` + `limits`): no instantiation that no call reaches, none that only an untraced call reaches."""
    notes = open(smallconv_launch_trace.notes).read()
    symbols = {s for s in re.findall(r"\.name:\s+(\S+)", notes) if re.search(r"\d+(expand3x3_|wgrad3x3_|head_fwd|stem_dgrad)\w*kernelI", s) and not s.endswith(".kd")}
    assert len(symbols) == 88
    launched = set()
    for mode in ("all", "limits"):
        for line in smallconv_launch_trace(mode):
            launched.update(re.findall(r" launch=(\S+)", line))
    assert not symbols - launched, sorted(symbols - launched)
    assert launched <= symbols


def test_smallconv_plans_at_their_clamps(smallconv_launch_trace):
    """The `limits` sweep of the stem / head entry points: the persistent grids under the CU limits 256 / 248 / 8, the byte limit that demotes a
    C = 128 call to the VALU kernel, the contraction's bands, the refusal at 2^24 pixels - values worked out by hand from the launchers as they
    stood before the planners and confirmed on their trace - and, on every line, gmk_*_wgrad_blocks(B H W) = the grid of the weight-gradient
    launch = the rows ops sizes the partials with.  The byte limit is one number in the source: every kBadOff is the file-scope one."""
    from generative_models_amd._lib import K
    F32, BF16, F16 = 0, 1, 2
    lines = smallconv_launch_trace("limits")
    assert len(lines) == 3 * 2 * 4 * 13 * (3 * 16 + 6) + 36 and all("no-metadata" not in line for line in lines)
    rows = _smallconv_rows(lines)
    at = {(e, int(f["cu"]), int(f["variant"]), int(f["C"]), int(f["cs"]), int(f["B"]), f["grid"], int(f["dtype"])): (rc, kid, ls)
          for e, f, rc, _, kid, ls in rows if "cu" in f}
    # (c) the partial rows
    n = 0
    for e, f, rc, _, kid, ls in rows:
        if e in ("stem_wgrad", "head_wgrad") and rc == 0 and "blocks" in f:
            blocks = int(f["blocks"].split(",")[e == "head_wgrad"])
            assert ls and all(w["grid"] == "%d,1,1" % blocks for w in ls) and len(ls) == (int(f["cs"]) if kid == K.WGRAD3 else 1), (f, ls)
            n += 1
    assert n == 3 * 3 * 2 * 4 * (13 - 2) * (2 + 3)          # every accepted size (two of the 13 are 2^24 pixels), the five weight-gradient lines
    # (b) B = 2048 at 32 x 32, 3 image channels, C = 128
    for L in (256, 248, 8):
        rc, kid, (w,) = at[("stem_fwd", L, 0, 128, 3, 2048, "32x32", BF16)]
        assert (rc, kid, w["grid"], w["block"]) == (0, K.EXPAND_TILE16, "%d,1,1" % min(2048 * 8, 2 * L), "256,1,1") and "expand3x3_tile16_kernel" in w["name"]
        assert {256: 512, 248: 496, 8: 16}[L] == min(2048 * 8, 2 * L) and w["args"][-4:-2] == [8, 2048 * 8]          # tps, ntiles
        rc, kid, (w,) = at[("stem_wgrad", L, 0, 128, 3, 2048, "32x32", F32)]
        assert (rc, kid, w["grid"]) == (0, K.WGRAD3_MFMA, "%d,1,1" % min(2048, 2 * L)) and "wgrad3x3_mfma_kernel" in w["name"]      # 1024 pixels per block: 2048 blocks
        assert w["args"][-1] == (-(-2 ** 20 // (4 * min(2048, 2 * L))) + 7) // 8 * 8 and (L != 256 or w["args"][-1] == 512)      # ppw: pairs per wave, groups of 8
    rc, kid, (w,) = at[("head_fwd", 256, 0, 128, 3, 2048, "32x32", F16)]
    assert (rc, kid, w["grid"], w["block"], w["lds"]) == (0, K.HEAD_FWD_MFMA, "2048,1,1", "512,1,1", str(27 * 34 * 32 * 4)) and 27 * 34 * 32 * 4 == 117504
    assert w["args"][-3:-1] == [32, 1] and "head_fwd_mfma_kernel" in w["name"]          # band, nbands
    rc, kid, (w,) = at[("head_fwd", 256, 0, 128, 3, 1024, "64x64", F16)]
    assert (rc, kid, w["grid"], w["lds"], w["args"][-3:-1]) == (0, K.HEAD_FWD_MFMA, "4096,1,1", "124416", [16, 4])
    # B = 8192 at 32 x 32: the fp32 output is exactly 4 GiB - the VALU kernel, 1024 pixels per block; the bf16 one stays tiled
    rc, kid, (w,) = at[("stem_fwd", 256, 0, 128, 3, 8192, "32x32", F32)]
    assert (rc, kid, w["grid"], w["args"][-1]) == (0, K.EXPAND, "8192,1,1", 1024) and "expand3x3_kernel" in w["name"]
    rc, kid, (w,) = at[("stem_fwd", 256, 0, 128, 3, 8192, "32x32", BF16)]
    assert (rc, kid, w["grid"]) == (0, K.EXPAND_TILE16, "512,1,1")
    # exactly 2^20 pixels: still 512 per block; a 16-bit tensor of exactly the byte limit: the VALU kernels
    assert at[("stem_fwd", 256, 0, 256, 3, 1024, "32x32", BF16)][2][0]["grid"] == "2048,1,1"
    for e, kid in (("stem_fwd", K.EXPAND), ("head_fwd", K.HEAD_FWD), ("stem_dgrad", K.STEM_DGRAD)):
        assert at[(e, 256, 0, 128, 3, 479349, "5x7", BF16)][:2] == (0, kid)
    # rows of exactly 128 pixels are the last the tiled kernels take; 2 image channels there: 11 band rows fit the contraction's LDS, so 12 rows are 2 bands of 6
    assert at[("stem_fwd", 256, 0, 128, 2, 2, "12x128", BF16)][:2] == (0, K.EXPAND_TILE16) and at[("stem_wgrad", 256, 0, 128, 2, 2, "12x128", BF16)][:2] == (0, K.WGRAD3_TILE16)
    rc, kid, (w,) = at[("head_fwd", 256, 0, 128, 2, 2, "12x128", BF16)]
    assert (rc, kid, w["grid"], w["lds"], w["args"][-3:-1]) == (0, K.HEAD_FWD_MFMA, "4,1,1", str(18 * 8 * 128 * 4), [6, 2])
    # 2^24 pixels: every entry refuses, with the texts it has always had
    texts = {"stem_fwd": "gmk_stem_fwd: unsupported shape B=16384 cin=3 32x32 C=128", "stem_dgrad": "gmk_stem_dgrad: unsupported shape B=16384 cin=3 32x32 C=128"}
    for e, f, rc, err, kid, ls in rows:
        if f.get("B") == "16384" and f["cs"] == "3" and f["C"] == "128":
            assert rc == -1 and not ls and err == texts.get(e, "gmk_%s: unsupported shape" % e), (e, f, err)
    assert all(rc == 0 for (e, L, v, C, cs, B, g, dt), (rc, _, _) in at.items() if B == 16383 and dt != 7)
    # an illegal storage type, a null pointer, an image too wide for any kernel
    assert all(rc == -1 and not ls for (e, L, v, C, cs, B, g, dt), (rc, _, ls) in at.items() if dt == 7)
    nulls = [(e, f, rc, err) for e, f, rc, err, _, ls in rows if "null" in f]
    order = ["stem_fwd", "stem_wgrad", "head_fwd", "head_dgrad", "head_wgrad", "stem_dgrad"]
    assert len(nulls) == 36 and all((rc, err) == (-1, "gmk_%s: null pointer" % e) if order[int(f["null"])] == e else rc == 0 for e, f, rc, err in nulls)
    assert at[("head_fwd", 256, 0, 128, 3, 2, "1x2048", BF16)][0] == -1 and at[("head_fwd", 256, 0, 128, 3, 2, "2x400", BF16)][:2] == (0, K.HEAD_FWD)
    src = open(os.path.join(ROOT, "generative_models_amd", "csrc", "smallconv.hip")).read()
    assert set(re.findall(r"kBadOff = (\w+);", src)) == {"0xFFFFFF00u"} and "0xFFFFFF00ull" not in src
