"""CPU tests (no GPU) of the image output's host side: the PNG / APNG encoders of generative_models_amd/pngio.py against the decoder
tests/png_ref.py (and, where it is installed, against PIL), common.ImageWriter's files and frame selection, the driver's flags, and the host
restatement tests/image_ref.py itself.  Every comparison is exact."""
import os
import struct
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_ref  # noqa: E402
import png_ref  # noqa: E402

# (width, height, channels, frames): grey and RGB, width 1, odd widths, one frame and three
PICTURES = [(1, 1, 1, 1), (1, 4, 3, 3), (7, 5, 1, 3), (7, 5, 3, 1), (37, 19, 3, 3), (16, 8, 1, 1)]


def _frames(width, height, channels, T, seed=0):
    rng = np.random.default_rng(seed)
    pix = rng.integers(0, 256, (T, height, width, channels), dtype=np.uint8)
    pix[:, 0, 0, :] = 255                                       # both extremes in every frame
    pix[:, -1, -1, :] = 0
    lines = np.zeros((T, height, 1 + width * channels), dtype=np.uint8)
    lines[:, :, 1:] = pix.reshape(T, height, width * channels)
    return pix, lines


def _files(tmp_path):
    """{name: (path, pixels [T, H, W, C], animated)} of one PNG and one APNG per entry of PICTURES."""
    from generative_models_amd import pngio
    out = {}
    for k, (w, h, c, T) in enumerate(PICTURES):
        pix, lines = _frames(w, h, c, T, seed=k)
        still, strip = tmp_path / f"still_{k}.png", tmp_path / f"strip_{k}.png"
        still.write_bytes(pngio.encode_png(lines[0], w, h, c))
        strip.write_bytes(pngio.encode_apng(lines, w, h, c, fps=4))
        out[f"still_{k}"] = (still, pix[:1], False)
        out[f"strip_{k}"] = (strip, pix, True)
    return out


def test_png_and_apng_round_trip(tmp_path):
    from generative_models_amd import pngio
    for name, (path, pix, animated) in _files(tmp_path).items():
        got = png_ref.decode(path.read_bytes())
        T, h, w, c = pix.shape
        assert (got["width"], got["height"], got["channels"], got["animated"]) == (w, h, c, animated), name
        assert np.array_equal(got["frames"], pix), name
        if animated:
            assert got["plays"] == 0 and len(got["delays"]) == T and got["sequence"] == list(range(2 * T - 1)), name
    # bytes, an ndarray of another shape and every compression level give the same picture
    pix, lines = _frames(7, 5, 3, 1)
    for buf, level in ((lines[0].tobytes(), 6), (lines[0].reshape(-1), 0), (lines[0], 9)):
        assert np.array_equal(png_ref.decode(pngio.encode_png(buf, 7, 5, 3, level=level))["frames"], pix)
    # what is no scanline buffer is named
    with pytest.raises(ValueError, match="scanline bytes"):
        pngio.encode_png(lines[0][:, :-1], 7, 5, 3)
    bad = lines[0].copy()
    bad[2, 0] = 1
    with pytest.raises(ValueError, match="filter byte"):
        pngio.encode_png(bad, 7, 5, 3)
    with pytest.raises(ValueError, match="channels"):
        pngio.encode_png(lines[0], 7, 5, 2)
    with pytest.raises(ValueError, match="no frames"):
        pngio.encode_apng([], 7, 5, 3, fps=4)
    with pytest.raises(ValueError, match="fps"):
        pngio.encode_apng(lines, 7, 5, 3, fps=0)


def test_decoder_rejects_what_is_outside_the_subset():
    """The decoder is the yardstick of the GPU tests: a wrong CRC, a filtered line and a broken sequence must not pass it."""
    from generative_models_amd import pngio
    _, lines = _frames(7, 5, 3, 3)
    blob = pngio.encode_apng(lines, 7, 5, 3, fps=4)
    png_ref.decode(blob)
    flipped = bytearray(blob)
    flipped[44] ^= 1                                            # inside acTL's payload
    with pytest.raises(AssertionError, match="CRC"):
        png_ref.decode(bytes(flipped))
    with pytest.raises(AssertionError, match="signature"):
        png_ref.decode(b"\x88" + blob[1:])
    with pytest.raises(AssertionError):
        png_ref.decode(blob + b"\0")
    import zlib
    filtered = lines[0].copy()
    filtered[1, 0] = 2
    body = pngio.SIGNATURE + pngio._ihdr(7, 5, 3) + pngio._chunk(b"IDAT", zlib.compress(filtered.tobytes())) + pngio._chunk(b"IEND", b"")
    with pytest.raises(AssertionError, match="filter"):
        png_ref.decode(body)


@pytest.mark.parametrize("fps", [1, 4, 20, 60, 24.5])
def test_fctl_delay_and_sequence(fps):
    from generative_models_amd import pngio
    _, lines = _frames(5, 3, 1, 3)
    blob = pngio.encode_apng(lines, 5, 3, 1, fps=fps)
    got = png_ref.decode(blob)
    assert len(got["delays"]) == 3
    for num, den in got["delays"]:
        assert Fraction(num, den) == 1 / Fraction(fps)          # every rate here has an exact 16-bit fraction
    assert got["sequence"] == [0, 1, 2, 3, 4]                    # fcTL 0, IDAT, fcTL 1, fdAT 2, fcTL 3, fdAT 4
    kinds = [k for k, _ in png_ref.chunks(blob)]
    assert kinds == [b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fcTL", b"fdAT", b"fcTL", b"fdAT", b"IEND"]
    assert struct.unpack(">II", png_ref.chunks(blob)[1][1]) == (3, 0)
    one = png_ref.decode(pngio.encode_apng(lines[:1], 5, 3, 1, fps=fps))      # T = 1 is a valid APNG
    assert one["animated"] and one["frames"].shape == (1, 3, 5, 1) and one["sequence"] == [0]


def test_files_open_in_pil(tmp_path):
    """The same files through an independent reader.  Apart from the others, so that a missing PIL shows as one skip and hides nothing."""
    Image = pytest.importorskip("PIL.Image")
    for name, (path, pix, animated) in _files(tmp_path).items():
        T, h, w, c = pix.shape
        with Image.open(path) as im:
            assert im.size == (w, h) and im.mode == ("L" if c == 1 else "RGB"), name
            assert getattr(im, "n_frames", 1) == T, name
            for t in range(T):
                im.seek(t)
                assert np.array_equal(np.asarray(im.convert("L" if c == 1 else "RGB")).reshape(h, w, c), pix[t]), (name, t)


def test_image_writer_files(tmp_path):
    from generative_models_amd import common
    writer = common.ImageWriter(tmp_path / "run")
    assert isinstance(writer, common.NullWriter) and writer.max_frames == 60
    writer.add_scalar("loss", 1.5, 3)
    assert writer.scalars["loss"] == [(3, 1.5)]                 # scalars as in NullWriter
    rng = np.random.default_rng(1)
    rgb = torch.from_numpy(rng.integers(0, 256, (3, 6, 9), dtype=np.uint8))
    grey = rng.integers(0, 256, (1, 6, 9), dtype=np.uint8)      # arrays are taken as well as tensors
    writer.add_image("samples", rgb, 4)
    writer.add_image("diffusion_model/grey", grey, 12345)
    vid = torch.from_numpy(rng.integers(0, 256, (1, 3, 3, 6, 9), dtype=np.uint8))
    writer.add_video("diffusion_model/x", vid, 0, fps=20)
    images = tmp_path / "run" / "images"
    assert sorted(p.name for p in images.iterdir()) == ["diffusion_model_grey_12345.png", "diffusion_model_x_0000.png", "samples_0004.png"]
    got = png_ref.decode((images / "samples_0004.png").read_bytes())
    assert not got["animated"] and np.array_equal(got["frames"][0], rgb.permute(1, 2, 0).numpy())
    got = png_ref.decode((images / "diffusion_model_grey_12345.png").read_bytes())
    assert got["channels"] == 1 and np.array_equal(got["frames"][0], grey.transpose(1, 2, 0))
    got = png_ref.decode((images / "diffusion_model_x_0000.png").read_bytes())
    assert got["animated"] and got["delays"] == [(1, 20)] * 3 and np.array_equal(got["frames"], vid[0].permute(0, 2, 3, 1).numpy())
    with pytest.raises(ValueError, match="max_frames"):
        common.ImageWriter(tmp_path, max_frames=1)
    with pytest.raises(ValueError, match=r"\[1, T, C, H, W\]"):
        writer.add_video("v", vid[0], 0, fps=4)
    # the tensorboard surface of the reference's grid helpers lands in files too
    common.write_grid(writer, "grid", torch.zeros((25, 1, 28, 28), dtype=torch.uint8), 1)
    common.write_gridvid(writer, "gridvid", torch.zeros((6, 25, 1, 28, 28), dtype=torch.uint8), 1)
    assert png_ref.decode((images / "grid_0001.png").read_bytes())["frames"].shape == (1, 140, 140, 1)
    got = png_ref.decode((images / "gridvid_0001.png").read_bytes())
    assert got["frames"].shape == (6, 140, 140, 3) and got["delays"] == [(1, 2)] * 6


def test_frame_selection():
    from generative_models_amd import common
    assert common.frame_indices(1, 60) == [0] and common.frame_indices(60, 60) == list(range(60)) and common.frame_indices(3, 2) == [0, 2]
    idx = common.frame_indices(1000, 60)
    assert len(idx) == 60 and idx[0] == 0 and idx[-1] == 999 and all(b > a for a, b in zip(idx, idx[1:]))
    assert idx == [k * 999 // 59 for k in range(60)]
    assert common.frame_indices(61, 60)[-1] == 60 and len(set(common.frame_indices(61, 60))) == 60
    with pytest.raises(ValueError, match="max_frames"):
        common.frame_indices(10, 1)


def test_flags_are_checked_before_a_model_is_built(tmp_path, monkeypatch):
    from generative_models_amd import common, main
    assert (main.DG.save_images, main.DG.image_frames, main.DG.dump_samples) == (0, 60, 0)
    built = []
    Model = common.discover_models()["diffusion"]
    real = Model.__init__
    monkeypatch.setattr(Model, "__init__", lambda self, G: built.append(1) or real(self, G))
    base = ["--model=diffusion", "--device", "cpu", "--logdir", str(tmp_path), "--hidden_size", "32"]
    for flags, name in ((["--save_images", "2"], "save_images"), (["--image_frames", "1"], "image_frames"), (["--dump_samples", "-1"], "dump_samples")):
        with pytest.raises(ValueError, match=name):
            main.load_model_and_data(base + flags)
    assert built == []
    # the defaults leave the writer a plain NullWriter; save_images 1 makes it an ImageWriter with image_frames
    G, _ = main.FlagSpace(main.DG).resolve(base)
    main._check_image_flags(G)
    assert type(main.Session(None, None, None, None, None, G).writer) is common.NullWriter
    G, _ = main.FlagSpace(main.DG).resolve(base + ["--save_images", "1", "--image_frames", "7", "--dump_samples", "12"])
    main._check_image_flags(G)
    writer = main.Session(None, None, None, None, None, G).writer
    assert type(writer) is common.ImageWriter and writer.max_frames == 7 and str(writer.logdir) == str(G.logdir) and G.dump_samples == 12


def test_the_restatement():
    """What tests/image_ref.py claims about its own inputs (they are what makes the GPU comparison sharp), and its tiling on a case small
    enough to write down."""
    b = image_ref.boundary_values()
    x = torch.from_numpy(b)
    q = image_ref.quantize(x)
    assert b.shape == (1811,) and len(set(q.tolist())) == 256
    as_f64 = ((x.double() + 1) * 127.5).clamp(0, 255).to(torch.uint8)
    with np.errstate(over="ignore"):
        fused = torch.from_numpy(np.float32(b.astype(np.float64) * 127.5 + 127.5)).clamp(0, 255).to(torch.uint8)      # one rounding
    assert int((as_f64 != q).sum()) == 136 and int((fused != q).sum()) == 216
    imgs = image_ref.images((3, 7, 3, 5, 7))
    assert len({im.numpy().tobytes() for im in imgs.reshape(21, -1)}) == 21 and len(set(image_ref.quantize(imgs).flatten().tolist())) == 256
    u8 = np.arange(3 * 2 * 2, dtype=np.uint8).reshape(1, 3, 1, 2, 2) + 1
    g = image_ref.grid(u8, ncol=2, gap=1, fill=9, out_channels=1, row_prefix=1)[0]
    assert g.tolist() == [[0, 9, 9, 9, 9, 9, 9, 9],
                          [0, 9, 1, 2, 9, 5, 6, 9],
                          [0, 9, 3, 4, 9, 7, 8, 9],
                          [0, 9, 9, 9, 9, 9, 9, 9],
                          [0, 9, 9, 10, 9, 9, 9, 9],
                          [0, 9, 11, 12, 9, 9, 9, 9],
                          [0, 9, 9, 9, 9, 9, 9, 9]]
    rgb = image_ref.grid(u8[:, :1], ncol=1, gap=0, fill=0, out_channels=3, row_prefix=0)[0]
    assert rgb.tolist() == [[1, 1, 1, 2, 2, 2], [3, 3, 3, 4, 4, 4]]
