"""A PNG / APNG decoder for the tests, written from the specifications (PNG: W3C Recommendation, second edition, sections 5 and 11; APNG:
https://wiki.mozilla.org/APNG_Specification) for exactly the subset generative_models_amd/pngio.py emits: 8 bits per sample, colour type 0 or
2, non-interlaced, filter type 0 on every line, every APNG frame full size at offset 0.  Anything else is an error, so a file that decodes here
is a file of that subset with a correct signature, chunk order and CRCs.  Not a test file."""
import struct
import zlib

import numpy as np

SIGNATURE = bytes([137, 80, 78, 71, 13, 10, 26, 10])


def chunks(blob):
    """-> [(type, payload)], every length and CRC checked, nothing after IEND."""
    assert blob[:8] == SIGNATURE, "not a PNG signature"
    pos, out = 8, []
    while pos < len(blob):
        assert pos + 12 <= len(blob), "truncated chunk"
        (length,) = struct.unpack(">I", blob[pos:pos + 4])
        kind = blob[pos + 4:pos + 8]
        payload = blob[pos + 8:pos + 8 + length]
        assert len(payload) == length, "truncated chunk payload"
        (crc,) = struct.unpack(">I", blob[pos + 8 + length:pos + 12 + length])
        assert crc == (zlib.crc32(kind + payload) & 0xFFFFFFFF), f"bad CRC in {kind!r}"
        out.append((kind, payload))
        pos += 12 + length
        if kind == b"IEND":
            break
    assert pos == len(blob), "bytes after IEND"
    assert out and out[0][0] == b"IHDR" and out[-1][0] == b"IEND" and out[-1][1] == b"", "IHDR first, an empty IEND last"
    return out


def _pixels(packed, width, height, channels):
    raw = zlib.decompress(packed)
    stride = 1 + width * channels
    assert len(raw) == height * stride, f"{len(raw)} bytes inflate, {height * stride} expected"
    lines = np.frombuffer(raw, dtype=np.uint8).reshape(height, stride)
    assert not lines[:, 0].any(), "a filter type other than 0"
    return lines[:, 1:].reshape(height, width, channels)


def decode(blob):
    """-> dict(frames uint8 [T, H, W, C], width, height, channels, animated, plays, delays [(num, den)] per frame, sequence [int])."""
    cs = chunks(blob)
    width, height, depth, colour, compression, filt, interlace = struct.unpack(">IIBBBBB", cs[0][1])
    assert depth == 8 and colour in (0, 2) and (compression, filt, interlace) == (0, 0, 0), "outside the subset"
    channels = {0: 1, 2: 3}[colour]
    kinds = [k for k, _ in cs]
    assert set(kinds) <= {b"IHDR", b"acTL", b"fcTL", b"IDAT", b"fdAT", b"IEND"}, kinds
    assert kinds.count(b"IHDR") == 1 and kinds.count(b"IDAT") == 1
    if b"acTL" not in kinds:
        assert kinds == [b"IHDR", b"IDAT", b"IEND"], kinds
        return dict(frames=_pixels(cs[1][1], width, height, channels)[None], width=width, height=height, channels=channels, animated=False,
                    plays=None, delays=[], sequence=[])
    assert kinds[1] == b"acTL" and kinds.count(b"acTL") == 1, "acTL before the first frame, once"
    num_frames, plays = struct.unpack(">II", cs[1][1])
    assert num_frames >= 1
    body = cs[2:-1]
    assert len(body) == 2 * num_frames, "one fcTL and one data chunk per frame"
    frames, delays, sequence = [], [], []
    for k in range(num_frames):
        (ckind, control), (dkind, data) = body[2 * k], body[2 * k + 1]
        assert ckind == b"fcTL" and dkind == (b"IDAT" if k == 0 else b"fdAT"), (k, ckind, dkind)
        seq, w, h, x0, y0, num, den, dispose, blend = struct.unpack(">IIIIIHHBB", control)
        assert (w, h, x0, y0, dispose, blend) == (width, height, 0, 0, 0, 0), "a full frame at offset 0, dispose 0, blend 0"
        sequence.append(seq)
        delays.append((num, den))
        if k:
            sequence.append(struct.unpack(">I", data[:4])[0])
            data = data[4:]
        frames.append(_pixels(data, width, height, channels))
    assert sequence == list(range(len(sequence))), f"sequence numbers {sequence}"
    return dict(frames=np.stack(frames), width=width, height=height, channels=channels, animated=True, plays=plays, delays=delays,
                sequence=sequence)
