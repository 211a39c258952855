"""PNG and APNG files from scanline buffers, with the standard library only (zlib, struct).

The encoders take what `ops.image_grid(..., row_prefix=1)` returns once it is on the host: `height` lines of one filter byte 0 (filter type
"None") followed by `width * channels` bytes, channels interleaved - the byte stream a PNG's IDAT payload is the deflation of.  Nothing is
reordered here; the work is one `zlib.compress` per frame plus the chunk framing.  Output: 8 bits per sample, colour type 0 (grey) or 2
(RGB), non-interlaced.  APNG per the Mozilla specification (https://wiki.mozilla.org/APNG_Specification): acTL before the first IDAT, one fcTL
per frame, frame 0 in IDAT (so a plain PNG reader shows the first frame) and later frames in fdAT, one sequence counter over fcTL and fdAT.
"""
import struct
import zlib
from fractions import Fraction

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"
_COLOUR_TYPE = {1: 0, 3: 2}


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def _scanlines(buf, width, height, channels):
    """-> the buffer as bytes, after checking its size and its filter bytes."""
    if channels not in _COLOUR_TYPE:
        raise ValueError(f"channels = {channels}: 1 (grey) or 3 (RGB)")
    if width < 1 or height < 1:
        raise ValueError(f"a picture of {width} x {height} pixels")
    if isinstance(buf, np.ndarray):
        if buf.dtype != np.uint8:
            raise ValueError(f"scanlines of dtype {buf.dtype}, expected uint8")
        buf = np.ascontiguousarray(buf).tobytes()
    buf = bytes(buf)
    stride = 1 + width * channels
    if len(buf) != height * stride:
        raise ValueError(f"{len(buf)} scanline bytes, expected {height} x (1 + {width} x {channels}) = {height * stride}")
    if any(buf[::stride]):
        raise ValueError("a scanline does not start with filter byte 0")
    return buf


def _ihdr(width, height, channels):
    return _chunk(b"IHDR", struct.pack(">IIBBBBB", width, height, 8, _COLOUR_TYPE[channels], 0, 0, 0))


def encode_png(scanlines, width, height, channels, level=6):
    """-> the bytes of a PNG file.  scanlines: uint8 ndarray (any shape) or bytes of size height * (1 + width * channels)."""
    data = _scanlines(scanlines, width, height, channels)
    return SIGNATURE + _ihdr(width, height, channels) + _chunk(b"IDAT", zlib.compress(data, level)) + _chunk(b"IEND", b"")


def frame_delay(fps):
    """-> (numerator, denominator) of 1 / fps seconds as the two 16-bit fields of an fcTL chunk."""
    if not fps > 0:
        raise ValueError(f"fps = {fps}: a positive rate")
    delay = (1 / Fraction(fps)).limit_denominator(65535)
    if delay.numerator > 65535:
        raise ValueError(f"fps = {fps}: a frame delay above 65535 s")
    return delay.numerator, delay.denominator


def encode_apng(frames, width, height, channels, fps, level=6):
    """-> the bytes of an APNG file that loops forever.  frames: [T] buffers as encode_png takes (a [T, height, 1 + width * channels] array
    among them); every frame is full size, shown for 1 / fps seconds, dispose 0 (none), blend 0 (source)."""
    frames = [_scanlines(f, width, height, channels) for f in frames]
    if not frames:
        raise ValueError("an animation of no frames")
    num, den = frame_delay(fps)
    parts = [SIGNATURE, _ihdr(width, height, channels), _chunk(b"acTL", struct.pack(">II", len(frames), 0))]
    seq = 0
    for k, data in enumerate(frames):
        parts.append(_chunk(b"fcTL", struct.pack(">IIIIIHHBB", seq, width, height, 0, 0, num, den, 0, 0)))
        seq += 1
        packed = zlib.compress(data, level)
        if k == 0:
            parts.append(_chunk(b"IDAT", packed))
        else:
            parts.append(_chunk(b"fdAT", struct.pack(">I", seq) + packed))
            seq += 1
    parts.append(_chunk(b"IEND", b""))
    return b"".join(parts)


def from_chw(img_u8):
    """uint8 [C, H, W] (C 1 or 3; tensor or array) -> (scanlines uint8 [H, 1 + W C], W, H, C): the filter bytes added on the host, for callers
    that hold an ordinary picture instead of ops.image_grid's buffer."""
    img = np.asarray(img_u8.detach().cpu() if hasattr(img_u8, "detach") else img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[0] not in _COLOUR_TYPE:
        raise ValueError(f"a picture of dtype {img.dtype}, shape {img.shape}: want uint8 [C, H, W] with C 1 or 3")
    C, H, W = img.shape
    lines = np.zeros((H, 1 + W * C), dtype=np.uint8)
    lines[:, 1:] = img.transpose(1, 2, 0).reshape(H, W * C)
    return lines, W, H, C
