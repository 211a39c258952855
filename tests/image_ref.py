"""Host restatement of the image-output kernels (gmk_to_uint8, gmk_image_grid; include/gmk.h), for the tests.  Not a test file.

`quantize` is torch's own CPU chain, the definition the kernels are held to bit for bit; `grid` is the tiling written out from the layout in
the header; `boundary_values` is the set of inputs at which a different evaluation order of the quantisation shows."""
import numpy as np
import torch


def quantize(x):
    """fp32 tensor -> uint8 tensor: the chain of DiffusionModel.evaluate's `proc` (gms/diffusion/diffusion_model.py:92) on the CPU."""
    x = x.detach().cpu()
    assert x.dtype == torch.float32
    return ((x + 1) * 127.5).clamp(0, 255).to(torch.uint8)


def crop(u8, c):
    return u8[..., c:u8.shape[-2] - c, c:u8.shape[-1] - c] if c else u8


def grid(u8, ncol, gap=2, fill=0, out_channels=None, row_prefix=0):
    """uint8 [T, N, C, h, w] (tensor or array) -> uint8 array [T, GH, row_prefix + GW out_channels]: image j of a frame at tile
    (j // ncol, j % ncol) of a GH x GW picture, GH = gap + nrow (h + gap), GW = gap + ncol (w + gap), everything else the byte `fill`;
    channels interleaved, a grey value repeated when out_channels = 3 with C = 1; row_prefix 1: a byte 0 in front of every line."""
    u8 = np.asarray(u8)
    assert u8.dtype == np.uint8 and u8.ndim == 5
    T, N, C, h, w = u8.shape
    oc = C if out_channels is None else out_channels
    assert oc == C or (oc == 3 and C == 1)
    nrow = -(-N // ncol)
    GH, GW = gap + nrow * (h + gap), gap + ncol * (w + gap)
    canvas = np.full((T, GH, GW, oc), fill, dtype=np.uint8)
    for j in range(N):
        y0, x0 = gap + (j // ncol) * (h + gap), gap + (j % ncol) * (w + gap)
        tile = u8[:, j].transpose(0, 2, 3, 1)                              # [T, h, w, C]
        canvas[:, y0:y0 + h, x0:x0 + w, :] = tile if oc == C else np.repeat(tile, 3, axis=3)
    out = np.zeros((T, GH, row_prefix + GW * oc), dtype=np.uint8)
    out[:, :, row_prefix:] = canvas.reshape(T, GH, GW * oc)
    return out


def boundary_values():
    """fp32 [1811]: for k = 0 .. 256 the float nearest to k / 127.5 - 1 (where the chain's result steps from k - 1 to k) with its three
    neighbours on either side, plus the ends of the range, both zeros, values far outside, infinities, the smallest subnormals and values near
    the largest finite float."""
    centre = (np.arange(257, dtype=np.float64) / 127.5 - 1.0).astype(np.float32)
    vals = [centre]
    lo = hi = centre
    for _ in range(3):
        lo = np.nextafter(lo, np.float32(-np.inf))
        hi = np.nextafter(hi, np.float32(np.inf))
        vals += [lo, hi]
    extra = np.array([-1, 1, -0.0, 0.0, -3.5, 7.25, np.inf, -np.inf, 1e-45, -1e-45, 3e38, -3e38], dtype=np.float32)
    out = np.concatenate(vals + [extra]).astype(np.float32)
    assert out.shape == (1811,) and not np.isnan(out).any()
    return out


def images(shape, seed=0):
    """fp32 tensor of `shape` = (..., C, H, W): the boundary values tiled (or truncated) over it, with a per-image step of a few ulps - an
    arange-based perturbation, so that no two images are equal while the values stay on the rounding boundaries' doorstep - and a seeded
    shuffle of the positions inside an image, so that every row and column of a small image sees interior and exterior values."""
    shape = tuple(shape)
    n = int(np.prod(shape))
    per = int(np.prod(shape[-3:]))
    base = boundary_values()
    order = np.random.default_rng(seed).permutation(len(base))
    flat = base[order][np.arange(n) % len(base)]
    image = np.arange(n) // per
    bits = flat.view(np.int32).copy()
    finite = np.isfinite(flat) & (np.abs(flat) > 1e-30) & (np.abs(flat) < 1e30)
    bits[finite] += (image[finite] % 7).astype(np.int32) - 3                # -3 .. +3 ulps, by image
    return torch.from_numpy(bits.view(np.float32).reshape(shape).copy())
