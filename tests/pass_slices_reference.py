"""ptl_pass_slices_to_gray16, restated in numpy (include/portal_amd.h has the contract): the records of the N blur sub-frames of one output
frame merged per pixel into three 16-bit grey images.  Shares nothing with the kernel or the C library; the depth's division and quantisation
are tests/pass_reference.py's, the integer parts are Python integers.
"""
import numpy as np

from tests import pass_reference as ref

NAMES = ("depth", "trips", "cut")


def merged_depth(slices):
    """(D, has_final) per pixel of slices (N, n): D starts as depth_near of the lowest-numbered slice with a final path and is replaced by a
    later such slice where its depth_near < D (so a NaN that came first stays); slices without a final path are never read."""
    slices = np.asarray(slices)
    d = np.zeros(slices.shape[1], np.float32)
    has = np.zeros(slices.shape[1], bool)
    for rec in slices:
        final = (rec["final_escaped"] & 0xFFFF) != 0
        with np.errstate(invalid="ignore"):
            takes = final & (~has | (rec["depth_near"] < d))
        d = np.where(takes, rec["depth_near"], d).astype(np.float32)
        has |= final
    return d, has


def depth(slices, lo=0.0, hi=1.0):
    d, has = merged_depth(slices)
    one = ref.records(d, 0, final=has.astype(np.uint32))  # the merged pixel as ONE record: the sample is ptl_passes_to_gray16's
    return ref.gray16(one, ref.DEPTH, lo, hi)


def trips(slices):
    total = np.asarray(slices)["trips"].astype(np.uint64).sum(axis=0, dtype=np.uint64)  # at most 256 (2^32 - 1) < 2^40: exact
    return np.minimum(total, 65535).astype(np.uint16)


def cut_sample(exhausted, paths):
    """ceil(65535 E / P) in Python integers; 0 where no path was traced."""
    exhausted, paths = int(exhausted), int(paths)
    return 0 if paths == 0 else -((-65535 * exhausted) // paths)


def cut(slices):
    """The same over records, in uint64: E <= 256 * 65535 < 2^24 and P < 2^26, so 65535 E + P - 1 < 2^41 and nothing rounds."""
    final, escaped, exhausted, _ = ref.counts(np.asarray(slices))
    e, p = exhausted.sum(axis=0, dtype=np.uint64), (final + escaped + exhausted).sum(axis=0, dtype=np.uint64)
    safe = np.maximum(p, np.uint64(1))
    return np.where(p == 0, np.uint64(0), (np.uint64(65535) * e + safe - np.uint64(1)) // safe).astype(np.uint16)


def gray16(slices, lo=0.0, hi=1.0):
    """slices: records of shape (N, n) -> {"depth", "trips", "cut"}: uint16 arrays of n samples (host order)."""
    slices = np.asarray(slices)
    assert slices.ndim == 2 and 1 <= slices.shape[0] <= 256
    return {"depth": depth(slices, lo, hi), "trips": trips(slices), "cut": cut(slices)}


def read_png_gray16_up(path):
    """A PNG of colour type 0, bit depth 16, not interlaced, ONE IDAT, rows of filter type 0 or 2 (Up) -> (H, W) uint16: the files
    ptl_png_write_stream_gray16 frames.  Asserts on anything else, on a bad CRC and on bytes behind IEND."""
    import struct
    import zlib

    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, chunks = 8, []
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos: pos + 4]), data[pos + 4: pos + 8]
        body = data[pos + 8: pos + 8 + length]
        assert len(body) == length and struct.unpack(">I", data[pos + 8 + length: pos + 12 + length])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        pos += 12 + length
    assert pos == len(data) and [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"], [k for k, _ in chunks]
    w, h, depth, colour, compression, filter_method, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filter_method, interlace) == (16, 0, 0, 0, 0), (depth, colour, compression, filter_method, interlace)
    lines = np.frombuffer(zlib.decompress(chunks[1][1]), np.uint8)
    assert lines.size == h * (2 * w + 1), "not H rows of 1 + 2 W bytes"
    lines = lines.reshape(h, 2 * w + 1)
    assert np.isin(lines[:, 0], (0, 2)).all() and lines[0, 0] == 0
    recon = np.zeros((h, 2 * w), np.uint8)
    above = np.zeros(2 * w, np.uint8)
    for y in range(h):  # Recon(x) = Filt(x) + Recon(b), b = the byte above
        recon[y] = lines[y, 1:] + above if lines[y, 0] == 2 else lines[y, 1:]
        above = recon[y]
    return recon.view(">u2").astype(np.uint16)
