"""Trace passes, restated in numpy: the statistics block of ptl_pass_stats and both conversions of ptl_passes_to_gray16
(include/portal_amd.h has the contract).  Shares nothing with the kernels or the C library: records are plain structured
arrays, the depth keys are recomputed from the float's bits here, the division is numpy's binary32 division.
"""
import struct
import zlib

import numpy as np

RECORD = np.dtype([("depth_near", "<f4"), ("trips", "<u4"), ("final_escaped", "<u4"), ("exhausted_outside", "<u4")])
HIST_BINS = 256
DEPTH, TRIPS = 0, 1


def records(depth_near, trips, final=0, escaped=0, exhausted=0, outside=0):
    """Records from per-field arrays (scalars broadcast)."""
    depth_near = np.asarray(depth_near, np.float32)
    r = np.zeros(depth_near.shape, RECORD)
    r["depth_near"] = depth_near
    r["trips"] = np.asarray(trips, np.uint32)
    r["final_escaped"] = np.asarray(final, np.uint32) | (np.asarray(escaped, np.uint32) << np.uint32(16))
    r["exhausted_outside"] = np.asarray(exhausted, np.uint32) | (np.asarray(outside, np.uint32) << np.uint32(16))
    return r


def counts(rec):
    fe, xo = rec["final_escaped"].astype(np.uint64), rec["exhausted_outside"].astype(np.uint64)
    return fe & 0xFFFF, fe >> 16, xo & 0xFFFF, xo >> 16


def depth_key(values):
    """Order-preserving unsigned key of binary32 values: negative floats complemented, the others with the top bit set."""
    bits = np.asarray(values, np.float32).view(np.uint32).astype(np.uint64)
    return np.where(bits >> 31 == 1, bits ^ 0xFFFFFFFF, bits | 0x80000000)


def empty_stats():
    return dict(pixels=0, paths=0, trips=0, final_paths=0, escaped=0, exhausted=0, outside=0, exhausted_pixels=0, max_trips=0, depth_max_key=0, depth_min_key_inv=0,
                trips_histogram=np.zeros(HIST_BINS, np.uint64))


def add_stats(stats, rec, per_launch=None, slot=0):
    """One sweep of ptl_pass_stats over `rec` added into `stats` (a dict from empty_stats); per_launch[slot] += its exhausted paths."""
    rec = np.asarray(rec).reshape(-1)
    final, escaped, exhausted, outside = counts(rec)
    trips = rec["trips"].astype(np.uint64)
    stats["pixels"] += rec.size
    stats["paths"] += int((final + escaped + exhausted + outside).sum())
    stats["trips"] += int(trips.sum())
    stats["final_paths"] += int(final.sum())
    stats["escaped"] += int(escaped.sum())
    stats["exhausted"] += int(exhausted.sum())
    stats["outside"] += int(outside.sum())
    stats["exhausted_pixels"] += int((exhausted > 0).sum())
    stats["max_trips"] = max(stats["max_trips"], int(trips.max()))
    finite = rec["depth_near"][np.isfinite(rec["depth_near"])]
    if finite.size:
        keys = depth_key(finite)
        stats["depth_max_key"] = max(stats["depth_max_key"], int(keys.max()))
        stats["depth_min_key_inv"] = max(stats["depth_min_key_inv"], int((keys ^ 0xFFFFFFFF).max()))
    stats["trips_histogram"] += np.bincount(np.minimum(trips, HIST_BINS - 1).astype(np.int64), minlength=HIST_BINS).astype(np.uint64)
    if per_launch is not None:
        per_launch[slot] += int(exhausted.sum())
    return stats


def depth_range(stats):
    """(lo, hi) as float32 from the two keys, or None."""
    if stats["depth_max_key"] == 0 or stats["depth_min_key_inv"] == 0:
        return None

    def value(key):
        bits = key & 0x7FFFFFFF if key >> 31 else key ^ 0xFFFFFFFF
        return np.array([bits], np.uint32).view(np.float32)[0]

    return value(stats["depth_min_key_inv"] ^ 0xFFFFFFFF), value(stats["depth_max_key"])


def q16(v):
    """0 if !(v > 0), 65535 if v >= 1, else floor(v * 65535 + 0.5), product and sum each rounded to binary32."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        c = np.where(v > 0, v, np.float32(0)).astype(np.float32)
        c = np.where(c >= 1, np.float32(1), c).astype(np.float32)
    scaled = (c * np.float32(65535.0)).astype(np.float32)
    return (scaled + np.float32(0.5)).astype(np.float32).astype(np.uint32)


def gray16(rec, which, lo=0.0, hi=1.0):
    """The 16-bit samples of ptl_passes_to_gray16 as a uint16 array (host order); gray16_bytes gives the big-endian scanline bytes."""
    rec = np.asarray(rec)
    if which == TRIPS:
        return np.minimum(rec["trips"], 65535).astype(np.uint16)
    lo, hi = np.float32(lo), np.float32(hi)
    with np.errstate(all="ignore"):
        span = np.float32(hi - lo)
        span = span if span > np.float32(1e-6) else np.float32(1e-6)
        t = ((rec["depth_near"] - lo).astype(np.float32) / span).astype(np.float32)
    has_final = (rec["final_escaped"] & 0xFFFF) != 0
    return np.where(has_final, q16(t), 0).astype(np.uint16)


def gray16_bytes(samples):
    return np.asarray(samples, np.uint16).astype(">u2").tobytes()


def read_png_gray16(path):
    """An independent reader on zlib for what ptl_png_write_gray16 writes: -> (height, width) uint16.  Checks the signature, every chunk's
    CRC, the header (colour type 0, bit depth 16, no interlace) and that every scanline has filter type 0."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, header, seen_end = 8, b"", None, False
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos:pos + 4]), data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + length]
        (crc,) = struct.unpack(">I", data[pos + 8 + length:pos + 12 + length])
        assert zlib.crc32(kind + body) & 0xFFFFFFFF == crc, kind
        if kind == b"IHDR":
            header = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat += body
        elif kind == b"IEND":
            seen_end = True
        pos += 12 + length
    assert seen_end and header is not None
    width, height, depth, colour, compression, filter_method, interlace = header
    assert (depth, colour, compression, filter_method, interlace) == (16, 0, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(height, 1 + 2 * width)
    assert not raw[:, 0].any(), "filter type None on every scanline"
    return raw[:, 1:].copy().view(">u2").astype(np.uint16)
