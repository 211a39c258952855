"""GPU tests of the image output: gmk_to_uint8 / gmk_image_grid through ops.to_uint8 / ops.image_grid against the host restatement
tests/image_ref.py, DiffusionModel.evaluate writing PNG / APNG files through common.ImageWriter (read back with tests/png_ref.py), and the
driver with --save_images 1 --dump_samples N, whose dump trains as an npy dataset.  Every comparison is bit-exact."""
import os
import shutil
import sys
from functools import partial

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_ref  # noqa: E402
import loader_ref  # noqa: E402
import png_ref  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- ops.to_uint8 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,H,W,crop", [(25, 1, 28, 28, 0), (25, 1, 32, 32, 2), (3, 3, 5, 7, 0), (3, 3, 5, 7, 1), (2, 3, 64, 64, 0), (1, 1, 1, 1, 0)])
def test_to_uint8_matches_the_cpu_chain(n, C, H, W, crop):
    """(25, 1, 32, 32, 2): the pad32 crop, source rows 8 bytes off the 16-byte groups; (3, 3, 5, 7, *): rows that are no whole 4-byte groups, odd
    image starts, the scalar tail; (2, 3, 64, 64, 0): more than one workgroup; (1, 1, 1, 1, 0): the tail alone."""
    from generative_models_amd import ops
    x = image_ref.images((n, C, H, W))
    want = image_ref.crop(image_ref.quantize(x), crop)
    if n * C * H * W >= 1811:
        assert len(set(want.flatten().tolist())) > 200          # the boundary set is in there
    got = ops.to_uint8(x.cuda(), crop=crop)
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (n, C, H - 2 * crop, W - 2 * crop) and got.is_contiguous()
    assert torch.equal(got.cpu(), want), int((got.cpu() != want).sum())
    # a trajectory [T, n, C, H, W] is the same bytes
    got5 = ops.to_uint8(x.cuda()[None].expand(2, n, C, H, W), crop=crop)
    assert got5.shape == (2,) + tuple(want.shape) and torch.equal(got5[1].cpu(), want)


def test_to_uint8_boundaries_nan_and_slices():
    from generative_models_amd import ops
    b = torch.from_numpy(image_ref.boundary_values())
    want = image_ref.quantize(b)
    assert len(set(want.tolist())) == 256
    got = ops.to_uint8(b.reshape(1, 1, 1, -1).cuda()).cpu().flatten()
    assert torch.equal(got, want), int((got != want).sum())      # a fused or reordered evaluation differs at 216 / 136 of these
    x = image_ref.images((3, 3, 5, 7))
    holes = torch.zeros(x.shape, dtype=torch.bool)
    holes[0, 0, 0, 0] = holes[1, 2, 3, 6] = holes[2, 1, 4, 3] = holes[2, 2, 4, 6] = True
    got = ops.to_uint8(torch.where(holes, torch.tensor(float("nan")), x).cuda()).cpu()
    assert torch.equal(got[~holes], image_ref.quantize(x)[~holes]) and int(got[holes].max()) == 0      # NaN -> 0
    big = image_ref.images((4, 3, 9, 12)).cuda()
    for view in (big[1:, :, 1:8, 3:10], big[::2], big.permute(0, 1, 3, 2), big.flatten()[1:1 + 3 * 5 * 7].reshape(1, 3, 5, 7)):
        assert (not view.is_contiguous()) or view.data_ptr() % 16
        assert torch.equal(ops.to_uint8(view, crop=1), ops.to_uint8(view.contiguous().clone(), crop=1))
        assert torch.equal(ops.to_uint8(view, crop=1).cpu(), image_ref.crop(image_ref.quantize(view), 1))


# ---- ops.image_grid -----------------------------------------------------------------------------------------------------------------------
# (T, N, ncol, C, out_channels, H, W, crop, gap, fill, row_prefix): a representative product of the axes, not the full one
GRID_CASES = [
    (3, 7, 3, 3, 3, 5, 7, 1, 2, 128, 1),       # nothing aligned: odd w, filter byte, partial last row, three frames, three planes
    (1, 25, 5, 1, 1, 28, 28, 0, 2, 0, 0),      # the reference's 5 x 5 grid of MNIST samples
    (1, 25, 5, 1, 3, 28, 28, 0, 2, 0, 1),      # ... as RGB scanlines (what write_frames would make of out_channels = 3)
    (3, 25, 5, 1, 1, 32, 32, 2, 2, 255, 1),    # pad32: cropped to 28 x 28 inside the kernel
    (1, 25, 5, 3, 3, 32, 32, 0, 2, 0, 1),      # CIFAR-10 shape
    (3, 25, 5, 3, 3, 32, 32, 2, 0, 128, 0),    # no gaps: every group of four pixels is a run, rows of whole dwords
    (1, 25, 5, 1, 1, 28, 28, 0, 0, 255, 0),    # no gaps, grey: the 16-byte loads
    (1, 7, 3, 1, 1, 28, 28, 0, 2, 255, 0),     # empty tiles filled with 255
    (3, 7, 3, 1, 3, 32, 32, 2, 0, 128, 1),
    (1, 7, 3, 3, 3, 5, 7, 0, 2, 0, 0),
    (1, 7, 3, 1, 1, 5, 7, 1, 0, 255, 1),
    (3, 7, 3, 1, 3, 5, 7, 0, 2, 128, 0),
    (1, 1, 1, 1, 1, 28, 28, 0, 2, 0, 0),       # N = 1
    (3, 1, 1, 3, 3, 5, 7, 1, 0, 255, 1),
    (1, 1, 5, 1, 3, 32, 32, 2, 2, 128, 1),     # N = 1 in a line of five: four empty tiles
    (1, 25, 5, 3, 3, 5, 7, 0, 0, 0, 1),
]


@pytest.mark.parametrize("T,N,ncol,C,oc,H,W,crop,gap,fill,prefix", GRID_CASES)
def test_image_grid_matches_the_restatement(T, N, ncol, C, oc, H, W, crop, gap, fill, prefix):
    from generative_models_amd import ops
    x = image_ref.images((T, N, C, H, W), seed=N + H)
    want = image_ref.grid(image_ref.crop(image_ref.quantize(x), crop), ncol, gap, fill, oc, prefix)
    h, w, nrow = H - 2 * crop, W - 2 * crop, -(-N // ncol)
    assert want.shape == (T, gap + nrow * (h + gap), prefix + (gap + ncol * (w + gap)) * oc)
    got = ops.image_grid(x.cuda(), ncol=ncol, crop=crop, gap=gap, fill=fill, out_channels=oc, row_prefix=prefix)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == want.shape
    assert np.array_equal(got.cpu().numpy(), want), int((got.cpu().numpy() != want).sum())
    if prefix:
        assert int(got[:, :, 0].max()) == 0
    # [N, C, H, W] is one frame, returned without the frame axis
    one = ops.image_grid(x[0].cuda(), ncol=ncol, crop=crop, gap=gap, fill=fill, out_channels=oc, row_prefix=prefix)
    assert tuple(one.shape) == want.shape[1:] and np.array_equal(one.cpu().numpy(), want[0])


def test_image_grid_defaults_and_views():
    from generative_models_amd import ops
    x = image_ref.images((2, 7, 3, 5, 7)).cuda()
    want = image_ref.grid(image_ref.quantize(x), 3, 2, 0, 3, 0)
    assert np.array_equal(ops.image_grid(x, ncol=3).cpu().numpy(), want)          # crop 0, gap 2, fill 0, out_channels C, no filter byte
    big = image_ref.images((2, 7, 3, 6, 9)).cuda()
    view = big[..., 1:, 2:]
    assert not view.is_contiguous()
    assert np.array_equal(ops.image_grid(view, ncol=3).cpu().numpy(), image_ref.grid(image_ref.quantize(view), 3, 2, 0, 3, 0))
    nan = x.clone()
    nan[1, 6, 2, 4, 6] = float("nan")
    got = ops.image_grid(nan, ncol=3).cpu().numpy()
    want[1, 2 + 2 * 7 + 4, (2 + 0 * 9 + 6) * 3 + 2] = 0                            # image 6: tile (2, 0)
    assert np.array_equal(got, want)


def test_wrapper_checks_and_fresh_outputs(monkeypatch):
    from generative_models_amd import ops
    x = image_ref.images((7, 3, 5, 7)).cuda()
    launches = []
    real_u8, real_grid = ops.lib.gmk_to_uint8, ops.lib.gmk_image_grid
    monkeypatch.setattr(ops.lib, "gmk_to_uint8", lambda *a: launches.append(a) or real_u8(*a))
    monkeypatch.setattr(ops.lib, "gmk_image_grid", lambda *a: launches.append(a) or real_grid(*a))
    grid = partial(ops.image_grid, ncol=3)
    for call in (ops.to_uint8, grid):
        with pytest.raises(ValueError, match="dtype"):
            call(x.half())
        with pytest.raises(ValueError, match="dtype"):
            call(x.to(torch.uint8))
        with pytest.raises(ValueError, match="device"):
            call(x.cpu())
        with pytest.raises(ValueError, match="rank"):
            call(x.flatten())
        with pytest.raises(ValueError, match="empty"):
            call(x[:0])
        for crop in (-1, 3, 1.5):                                   # 2 crop < min(5, 7)
            with pytest.raises(ValueError, match="crop"):
                call(x, crop=crop)
    with pytest.raises(ValueError, match="rank"):
        grid(x[0])
    with pytest.raises(ValueError, match="rank"):
        grid(x[None, None])
    with pytest.raises(ValueError, match="1 or 3"):
        grid(x[:, :2])
    for bad in (dict(ncol=0), dict(ncol=-3), dict(ncol=2.5), dict(gap=-1), dict(fill=256), dict(fill=-1), dict(row_prefix=2)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            ops.image_grid(x, **{"ncol": 3, **bad})
    for oc in (0, 2, 4, 1):                                         # 3 planes cannot become 1
        with pytest.raises(ValueError, match="out_channels"):
            grid(x, out_channels=oc)
    assert launches == []                                           # none of the above reached the library
    a, b = ops.to_uint8(x), ops.to_uint8(x)
    c, d = grid(x), grid(x)
    assert len(launches) == 4
    assert a.data_ptr() != b.data_ptr() and c.data_ptr() != d.data_ptr()      # fresh tensors
    a.fill_(7), c.fill_(7)
    assert torch.equal(b.cpu(), image_ref.quantize(x)) and np.array_equal(d.cpu().numpy(), image_ref.grid(image_ref.quantize(x)[None], 3)[0])


# ---- DiffusionModel.evaluate --------------------------------------------------------------------------------------------------------------
def _model(**flags):
    from generative_models_amd import common
    Model = common.discover_models()["diffusion_model"]
    G = common.AttrDict(dict(Model.DG))
    G.update(lr=3e-4, pad32=0, device="cuda", timesteps=3, bs=8, hidden_size=32)
    G.update(flags)
    torch.manual_seed(0)                                            # the same initial weights for every model of a test
    model = Model(G).to("cuda")
    model.eval()
    return model


def _picture(path):
    return png_ref.decode(path.read_bytes())


def _as_frames(u8):
    """what a decoded file holds for the scanline grids of uint8 [T, N, C, h, w]: [T, GH, GW, C]"""
    T, C = u8.shape[0], u8.shape[2]
    lines = image_ref.grid(u8, ncol=5, gap=2, fill=0, out_channels=C, row_prefix=0)
    return lines.reshape(T, lines.shape[1], -1, C)


@pytest.mark.parametrize("flags,S,crop", [(dict(in_channels=3, image_size=8), 8, 0), (dict(in_channels=1, pad32=1), 32, 2)])
def test_evaluate_writes_what_it_records(tmp_path, flags, S, crop):
    from generative_models_amd import common
    from generative_models_amd.diffusion.gaussian_diffusion import PhiloxStream
    C = flags["in_channels"]
    x = torch.rand(25, C, S, S, device="cuda") * 2 - 1
    y = torch.arange(25, device="cuda") % 10
    model = _model(inpaint_eval=1, **flags)
    model.evaluate(common.ImageWriter(tmp_path), x, y.clone(), epoch=4)
    ev = model.last_eval
    # last_eval: the torch chain and the crop of the float trajectories, recomputed here
    labels = torch.arange(25, dtype=torch.long, device="cuda") % 10
    with torch.no_grad():
        zs, xs, eps = model.diffusion.sample(net=partial(model.net, guide=labels), init_x=PhiloxStream(0).normal((25, C, S, S), "cuda"))
    for key, traj in (("sampling_process", zs), ("x", xs), ("eps", eps)):
        want = image_ref.crop(image_ref.quantize(traj), crop)
        assert ev[key].dtype == torch.uint8 and not ev[key].is_cuda and ev[key].shape == (3, 25, C, S - 2 * crop, S - 2 * crop)
        assert torch.equal(ev[key], want), key
    assert torch.equal(ev["samples"], ev["sampling_process"][-1]) and ev["inpaint"].shape == ev["samples"].shape
    # the files: exactly these five, each the grid of what last_eval holds
    images = tmp_path / "images"
    names = ["diffusion_model_eps_0004.png", "diffusion_model_x_0004.png", "inpaint_0004.png", "samples_0004.png", "sampling_process_0004.png"]
    assert sorted(p.name for p in images.iterdir()) == names
    for name, key in (("samples", "samples"), ("inpaint", "inpaint")):
        got = _picture(images / f"{name}_0004.png")
        assert not got["animated"] and got["channels"] == C
        assert np.array_equal(got["frames"], _as_frames(ev[key][None].numpy())), name
    for name, key in (("sampling_process", "sampling_process"), ("diffusion_model_eps", "eps"), ("diffusion_model_x", "x")):
        got = _picture(images / f"{name}_0004.png")
        assert got["animated"] and got["plays"] == 0 and got["frames"].shape[0] == 3 and got["delays"] == [(1, 1)] * 3      # min(3 // 3, 60) fps
        want = _as_frames(ev[key].numpy())
        for t in range(3):
            assert np.array_equal(got["frames"][t], want[t]), (name, t)
    # a NullWriter writes nothing and records the same bytes
    quiet = tmp_path / "quiet"
    quiet.mkdir()
    twin = _model(inpaint_eval=1, **flags)
    twin.evaluate(common.NullWriter(quiet), x, y.clone(), epoch=4)
    assert list(quiet.iterdir()) == []
    for key in ev:
        assert torch.equal(twin.last_eval[key], ev[key]), key


def test_write_frames_thins_long_trajectories(tmp_path):
    from generative_models_amd import common
    writer = common.ImageWriter(tmp_path, max_frames=4)
    x = image_ref.images((9, 3, 1, 5, 7)).cuda()
    writer.write_frames("strip", x, 2, ncol=2, fps=None)
    got = _picture(tmp_path / "images" / "strip_0002.png")
    keep = common.frame_indices(9, 4)
    assert keep == [0, 2, 5, 8] and got["frames"].shape[0] == 4 and got["delays"] == [(1, 1)] * 4
    want = image_ref.grid(image_ref.quantize(x)[keep], ncol=2)
    assert np.array_equal(got["frames"], want.reshape(4, want.shape[1], -1, 1))
    writer.write_frames("strip", x[:3], 3, ncol=2, crop=1, fps=20)
    got = _picture(tmp_path / "images" / "strip_0003.png")
    want = image_ref.grid(image_ref.crop(image_ref.quantize(x[:3]), 1), ncol=2)
    assert got["delays"] == [(1, 20)] * 3 and np.array_equal(got["frames"], want.reshape(3, want.shape[1], -1, 1))


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------
def test_driver_saves_images_and_dumps_a_dataset(tmp_path):
    import yaml
    from generative_models_amd import common, data, main
    rng = np.random.default_rng(7)
    root = tmp_path / "set"
    root.mkdir()
    for split, n in (("train", 16), ("test", 8)):
        np.save(root / f"{split}_images.npy", rng.integers(0, 256, (n, 3, 8, 8), dtype=np.uint8))
        np.save(root / f"{split}_labels.npy", rng.integers(0, 10, n, dtype=np.int64))
    logdir = tmp_path / "run"
    loaded = main.load_model_and_data(["--model=diffusion", "--data_device", "1", "--data", "npy", "--data_root", str(root), "--in_channels", "3",
                                       "--image_size", "8", "--binarize", "0", "--hidden_size", "32", "--bs", "8", "--epochs", "1", "--timesteps", "2",
                                       "--eval_heavy", "0", "--save_images", "1", "--dump_samples", "12", "--logdir", str(logdir)])
    model, G = loaded[0], loaded[-1]
    final = main.train(*loaded)
    assert final["diffusion/train/loss"] and all(np.isfinite(v) for v in final["diffusion/train/loss"])
    with open(logdir / "hps.yaml") as f:
        hps = yaml.load(f, Loader=yaml.Loader)
    assert (hps["save_images"], hps["image_frames"], hps["dump_samples"]) == (1, 60, 12)
    names = sorted(p.name for p in (logdir / "images").iterdir())
    assert names == sorted(f"{tag}_{epoch:04d}.png" for tag in ("samples", "sampling_process", "diffusion_model_eps", "diffusion_model_x")
                           for epoch in (0, 1))
    last = _picture(logdir / "images" / "samples_0001.png")
    assert np.array_equal(last["frames"], _as_frames(model.last_eval["samples"][None].numpy()))
    assert _picture(logdir / "images" / "sampling_process_0001.png")["frames"].shape == (2, 2 + 5 * 10, 2 + 5 * 10, 3)
    # the dump, written after the checkpoint of epoch 0
    images, labels = np.load(logdir / "samples_images.npy"), np.load(logdir / "samples_labels.npy")
    assert images.shape == (12, 3, 8, 8) and images.dtype == np.uint8
    assert labels.dtype == np.uint8 and labels.tolist() == (np.arange(12) % 10).tolist()
    assert (logdir / "model.pt").exists()
    # ... is a dataset: under the names data.load_npy reads, DeviceDataset yields the transform of exactly these bytes
    again = tmp_path / "again"
    again.mkdir()
    for split in ("train", "test"):
        for kind in ("images", "labels"):
            shutil.copy(logdir / f"samples_{kind}.npy", again / f"{split}_{kind}.npy")
    (train_images, train_labels), _ = data.load_npy(str(again))
    assert np.array_equal(train_images, images)
    ds = data.DeviceDataset(train_images, train_labels, 4, binarize=0, pad=0, device="cuda", seed=1000)
    batches = [(bx.cpu(), by.cpu()) for bx, by in ds]
    want_idx = loader_ref.shard_batches(loader_ref.permutation(12, 1000, 0), 0, 1, 4)
    assert len(batches) == 3 and sorted(np.concatenate(want_idx).tolist()) == list(range(12))
    for (bx, by), idx in zip(batches, want_idx):
        want_x, want_y = loader_ref.expected_batch(images, labels, idx, 0, 0, np.zeros(4, dtype=bool))
        assert torch.equal(bx, want_x) and torch.equal(by, want_y)
        assert torch.equal(bx, 2 * (torch.from_numpy(images[idx]).float() / 255) - 1)
    # sample_uint8 is sample() through the same kernel
    model.eval()
    counter = model._aux_rng.counter
    u8 = model.sample_uint8(3, torch.tensor([1, 2, 3], device="cuda"))
    model._aux_rng.counter = counter
    assert u8.is_cuda and u8.dtype == torch.uint8 and u8.shape == (3, 3, 8, 8)
    assert isinstance(main.Session(*loaded).writer, common.ImageWriter)
