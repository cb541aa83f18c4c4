"""tests/png16_reference.py -- numpy restatement of the rows ptl_average_f32_to_rgb48 writes (include/portal_amd.h), and a
reader for the files ptl_png_write_rgb48 makes of them.

TEST INFRASTRUCTURE ONLY: written from the formulas of the contract and from the PNG specification; shares no code with the kernel or
with png_io.cpp.  The averaged frame A = (E_R, E_G, E_B) is yuv_deep_reference.encode16, imported, not copied.

    raw row y, bytes 6x .. 6x+5:   E_R >> 8, E_R & 255, E_G >> 8, E_G & 255, E_B >> 8, E_B & 255
    FILTER_NONE (0):               out = raw
    FILTER_SUB  (1):               out[y][i] = (raw[y][i] - (i >= 6 ? raw[y][i - 6] : 0)) mod 256
H rows of 6 W bytes, packed, no filter-type bytes.
"""
import struct
import zlib

import numpy as np

from tests import yuv_deep_reference as dr

FILTER_NONE, FILTER_SUB = 0, 1


def raw_rows(a):
    """A (H, W, 3), values 0 .. 65535 -> (H, 6 W) uint8: big-endian samples."""
    a = np.asarray(a).astype(np.int64)
    assert a.ndim == 3 and a.shape[2] == 3 and int(a.min(initial=0)) >= 0 and int(a.max(initial=0)) <= 65535
    h, w = a.shape[:2]
    return np.stack([a >> 8, a & 255], axis=-1).astype(np.uint8).reshape(h, 6 * w)


def filtered(raw, filter):
    """(H, 6 W) uint8 raw rows -> the rows as they are written."""
    assert filter in (FILTER_NONE, FILTER_SUB)
    raw = np.asarray(raw, np.uint8)
    if filter == FILTER_NONE:
        return raw.copy()
    wide = raw.astype(np.int64)
    wide[:, 6:] -= raw[:, :-6].astype(np.int64)  # Python-sized integers, then mod 256: nothing borrows
    return (wide % 256).astype(np.uint8)


def rows_from_a(a, filter) -> bytes:
    return filtered(raw_rows(a), filter).tobytes()


def rows(frames, filter) -> bytes:
    """n RGBA32F sub-frames (H, W, >= 3) -> the H * 6 W bytes ptl_average_f32_to_rgb48 writes with `filter`."""
    return rows_from_a(dr.encode16(frames), filter)


def undo(payload: bytes, w, h, filter):
    """Rows as written -> A (H, W, 3) int64.  Sub is undone by a prefix sum along the row in each of the six byte lanes, mod 256."""
    got = np.frombuffer(payload, np.uint8).reshape(h, w, 6)
    if filter == FILTER_SUB:
        got = (np.cumsum(got.astype(np.int64), axis=1) % 256).astype(np.uint8)
    else:
        assert filter == FILTER_NONE
    pairs = got.reshape(h, w, 3, 2).astype(np.int64)
    return pairs[..., 0] * 256 + pairs[..., 1]


def read_png16(path, header=False):
    """A PNG of colour type 2, bit depth 16, not interlaced, rows of filter type 0 or 1 -> (H, W, 3) uint16 (header=True: that and what the
    file said about itself).  Asserts on anything else, on a bad CRC and on bytes behind IEND."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, chunks = 8, []
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos: pos + 4]), data[pos + 4: pos + 8]
        body = data[pos + 8: pos + 8 + length]
        assert len(body) == length and struct.unpack(">I", data[pos + 8 + length: pos + 12 + length])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        pos += 12 + length
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and all(k in (b"IHDR", b"IDAT", b"IEND") for k, _ in chunks)
    w, h, depth, colour, compression, filter_method, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filter_method, interlace) == (16, 2, 0, 0, 0), (depth, colour, compression, filter_method, interlace)
    lines = np.frombuffer(zlib.decompress(b"".join(body for kind, body in chunks if kind == b"IDAT")), np.uint8)
    assert lines.size == h * (6 * w + 1), "not H rows of 1 + 6 W bytes"
    lines = lines.reshape(h, 6 * w + 1)
    types = lines[:, 0]
    assert np.isin(types, (0, 1)).all(), sorted(set(types.tolist()))
    recon = lines[:, 1:].reshape(h, w, 6).astype(np.int64)
    summed = np.cumsum(recon, axis=1) % 256  # Recon(x) = Filt(x) + Recon(a), a = the byte six to the left, zero at the start of a row
    recon = np.where((types == 1)[:, None, None], summed, recon).astype(np.uint8)
    image = np.ascontiguousarray(recon).view(">u2").reshape(h, w, 3).astype(np.uint16)
    return image if not header else (image, {"width": w, "height": h, "depth": depth, "colour": colour, "ihdr": chunks[0][1], "filter_types": types.copy(), "idat_chunks": sum(k == b"IDAT" for k, _ in chunks)})
