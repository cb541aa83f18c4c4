"""The stream contract of the GPU deflate of 16-bit PNG frames (include/portal_amd.h: ptl_png_deflate_rgb48), restated in
numpy and plain Python, independent of the product.  The segments, the length tables, the code builder, the code-length code and the greedy
16 / 17 / 18 rule are those of tests/png_deflate_reference.py and tests/png_huffman_reference.py, imported, not copied.  New here: the raw
scanlines of rows of 6 W bytes, the band cut for them, the token rule at distance 6, the distance code (symbol 4, one extra bit of value
1; HDIST = 4 in a dynamic block), the header's magic word "PTL6", and a reader for 16-bit RGB files whose rows are of filter type 0 or 2."""
import struct
import zlib

import numpy as np

from tests import png_deflate_reference as pr
from tests import png_huffman_reference as hr

DISTANCE = 6           # a pixel: three big-endian 16-bit samples
DISTANCE_SYMBOL = 4    # RFC 1951 3.2.5: distances 5 .. 6, one extra bit; 6 is the extra bit 1
MAGIC = 0x364C5450     # "PTL6"
HEADER_BYTES = pr.HEADER_BYTES
SEGMENT = pr.SEGMENT
DISTANCE_LENGTHS = [0, 0, 0, 0, 1]  # HDIST = 4: one code, one bit, sent as 0
# what a match adds to its length code and extra bits, as (value, count) in packing order
FIXED_DISTANCE = (0b100 | (1 << 5), 6)  # 00100 most-significant bit first, then the extra bit 1
DYNAMIC_DISTANCE = (0b10, 2)            # the one-bit code 0, then the extra bit 1


# ---- the raw scanlines, bands -------------------------------------------------------------------
def rows_bytes(a):
    """A (H, W, 3), values 0 .. 65535 -> (H, 6 W) uint8, big-endian samples: the unfiltered rows of ptl_average_f32_to_rgb48."""
    a = np.asarray(a).astype(np.int64)
    assert a.ndim == 3 and a.shape[2] == 3 and int(a.min(initial=0)) >= 0 and int(a.max(initial=0)) <= 65535
    h, w = a.shape[:2]
    return np.stack([a >> 8, a & 255], axis=-1).astype(np.uint8).reshape(h, 6 * w)


def raw16_of_rows(rows):
    """(H, 6 W) uint8 unfiltered rows -> raw16: per row the filter-type byte (0 for row 0, 2 = Up below), then the row minus the row above
    per byte, mod 256."""
    rows = np.ascontiguousarray(rows, np.uint8)
    h, n = rows.shape
    out = np.empty((h, n + 1), np.uint8)
    out[0, 0], out[1:, 0] = 0, 2
    out[0, 1:] = rows[0]
    out[1:, 1:] = rows[1:] - rows[:-1]
    return out.tobytes()


def raw16(a):
    return raw16_of_rows(rows_bytes(a))


def rows_of_raw16(raw, w, h):
    """raw16 -> the (H, 6 W) unfiltered rows (Up undone)."""
    lines = np.frombuffer(raw, np.uint8).reshape(h, 6 * w + 1)
    assert lines[0, 0] == 0 and (lines[1:, 0] == 2).all()
    return np.cumsum(lines[:, 1:].astype(np.uint64), axis=0).astype(np.uint8)


def a_of_rows(rows):
    h, n = rows.shape
    return np.ascontiguousarray(rows).view(">u2").reshape(h, n // 6, 3).astype(np.int64)


def band_rows(w):
    return max(1, pr.BAND_TARGET // (6 * w + 1))


def band_count(w, h):
    return -(-h // band_rows(w))


def cut_bands(raw, w, h):
    step = band_rows(w) * (6 * w + 1)
    assert len(raw) == h * (6 * w + 1)
    return [raw[at: at + step] for at in range(0, len(raw), step)]


cut_segments = pr.cut_segments
band_capacity = pr.band_capacity


def stream_capacity(w, h):
    full, bands = band_rows(w) * (6 * w + 1), band_count(w, h)
    return (bands - 1) * band_capacity(full) + band_capacity(h * (6 * w + 1) - (bands - 1) * full)


def result_bytes(w, h):
    """ptl_png_stream16_bytes: header | room for the longest stream, rounded up to 16 | a 16-byte table entry per band | a slot per band."""
    slot = (band_capacity(band_rows(w) * (6 * w + 1)) + 15) // 16 * 16
    return HEADER_BYTES + (stream_capacity(w, h) + 15) // 16 * 16 + band_count(w, h) * (16 + slot)


def download_bytes(w, h):
    return HEADER_BYTES + (stream_capacity(w, h) + 15) // 16 * 16


# ---- the token rule ---------------------------------------------------------------------------
def segment_tokens_plain(segment, distance=DISTANCE):
    """The token rule word for word, in plain Python: [("lit", v)] and [("match", length)].  Byte i is covered when i >= distance and
    s[i] == s[i - distance].  Every byte that is not covered is a literal; it is followed by the maximal stretch of m covered bytes behind
    it: while m >= 3, a match of min(m, 258) at that distance; the remaining 0 .. 2 bytes are literals."""
    tokens, i, n = [], 0, len(segment)

    def covered(k):
        return k >= distance and segment[k] == segment[k - distance]

    while i < n:
        assert not covered(i)
        tokens.append(("lit", segment[i]))
        m = 0
        while i + 1 + m < n and covered(i + 1 + m):
            m += 1
        at = i + 1
        while m >= 3:
            length = min(m, 258)
            tokens.append(("match", length))
            at += length
            m -= length
        tokens += [("lit", segment[k]) for k in range(at, at + m)]
        i = at + m
    return tokens


def segment_symbols_plain(segment, distance=DISTANCE):
    """-> [(symbol, extra value, extra bits)]"""
    return [(x, 0, 0) if kind == "lit" else (int(hr.LENGTH_SYMBOL[x]), int(hr.LENGTH_EXTRA[x]), int(hr.LENGTH_EXTRA_BITS[x])) for kind, x in segment_tokens_plain(segment, distance)]


def segment_symbols(segment, distance=DISTANCE):
    """The same in numpy -> (symbols, extra values, extra bits)."""
    s = np.frombuffer(segment, np.uint8)
    covered = np.zeros(s.size, bool)
    covered[distance:] = s[distance:] == s[:-distance]
    starts = np.flatnonzero(~covered)
    assert starts[0] == 0
    stretch = np.diff(np.concatenate((starts, [s.size])))  # the non-covered byte and the covered ones behind it
    m = stretch - 1
    whole, rest = m // 258, m % 258
    last = (rest >= 3).astype(np.int64)
    tail = np.where(last == 1, 0, rest)
    per = 1 + whole + last + tail
    of = np.repeat(np.arange(starts.size), per)
    k = np.arange(of.size) - np.repeat(np.cumsum(per) - per, per)  # the token's place in its stretch
    length = np.where((k >= 1) & (k <= whole[of]), 258, np.where((k == whole[of] + 1) & (last[of] == 1), rest[of], 0))
    # a literal's byte: the stretch's first, or one of its last `tail` bytes
    back = per[of] - k  # 1 for the last token of the stretch
    at = np.where(k == 0, starts[of], starts[of] + stretch[of] - back)
    return np.where(length > 0, hr.LENGTH_SYMBOL[length], s[np.minimum(at, s.size - 1)].astype(np.int64)), hr.LENGTH_EXTRA[length], hr.LENGTH_EXTRA_BITS[length]


def band_histogram(band, symbols=segment_symbols, distance=DISTANCE):
    hist = np.zeros(hr.N_SYMBOLS, np.int64)
    for segment in cut_segments(band):
        found = symbols(segment, distance)
        hist += np.bincount(np.asarray([t[0] for t in found] if symbols is segment_symbols_plain else found[0], np.int64), minlength=hr.N_SYMBOLS)
    hist[hr.END_OF_BLOCK] += 1
    return hist


# ---- a band -----------------------------------------------------------------------------------
def block_header(lengths, distance_lengths=None):
    """BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN = 15, the 19 lengths of the code-length code, then the HLIT + 257 lengths followed by the
    distance lengths, coded as ONE sequence -> (values, counts)."""
    distance_lengths = DISTANCE_LENGTHS if distance_lengths is None else distance_lengths
    lengths = [int(n) for n in lengths]
    n_lit = max(s for s, n in enumerate(lengths) if n) + 1
    assert n_lit >= 257
    pairs = [(0, 1), (2, 2), (n_lit - 257, 5), (len(distance_lengths) - 1, 5), (15, 4)] + [(hr.CL_LENGTHS[s], 3) for s in hr.CL_ORDER]
    for symbol, extra, extra_bits in hr.length_sequence_tokens(lengths[:n_lit] + list(distance_lengths)):
        code, bits = hr.CL_CODES[symbol]
        pairs.append((code | (extra << bits), bits + extra_bits))
    return np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


def _segment_bits(segment, table, lengths, distance_bits, distance):
    symbols, extras, extra_bits = segment_symbols(segment, distance)
    match = symbols >= 257
    counts = lengths[symbols] + extra_bits
    values = table[symbols] | (extras << lengths[symbols]) | np.where(match, distance_bits[0] << counts, 0)
    counts = counts + match * distance_bits[1]
    return values, counts


FIXED_TABLE = np.array([hr._reversed(*pr.fixed_code(s)) for s in range(hr.N_SYMBOLS)], np.int64)


def encode_band(band, builder=hr.code_lengths, distance=DISTANCE):
    """One band -> dict(data, dynamic, lengths, header_bits, dynamic_bits, fixed_bits, segment_bits, hist, dynamic_data, fixed_data).  Dynamic
    only where it has FEWER bits than fixed.  `distance` = 1 parses with today's 8-bit rule (a yardstick for the size caps only: its
    distance bits are counted as this contract's)."""
    fixed_distance = FIXED_DISTANCE if distance == DISTANCE else (0, 5)
    dynamic_distance = DYNAMIC_DISTANCE if distance == DISTANCE else (0, 1)
    distance_lengths = DISTANCE_LENGTHS if distance == DISTANCE else [1]
    hist = band_histogram(band, distance=distance)
    lengths = np.asarray(builder(hist)[0] if builder is hr.code_lengths_plain else builder(hist), np.int64)
    assert ((lengths > 0) == (hist > 0)).all() and lengths.max() <= hr.LIMIT and sum(2.0 ** -n for n in lengths[lengths > 0]) == 1.0
    head_values, head_counts = block_header(lengths, distance_lengths)
    matches = int(hist[257:].sum())
    extra = int((hist * hr.SYMBOL_EXTRA_BITS).sum())
    dynamic_bits = int(head_counts.sum()) + int((hist * lengths).sum()) + extra + dynamic_distance[1] * matches
    fixed_bits = 3 + int((hist * hr.FIXED_LENGTHS).sum()) + extra + fixed_distance[1] * matches
    info = dict(dynamic=dynamic_bits < fixed_bits, lengths=lengths, header_bits=int(head_counts.sum()), dynamic_bits=dynamic_bits, fixed_bits=fixed_bits, hist=hist)
    table = np.array([hr._reversed(c, int(n)) for c, n in zip(hr.canonical_codes(lengths), lengths)], np.int64)
    parts, fixed_parts, info["segment_bits"] = [hr._bits(head_values, head_counts)], [np.array([0, 1, 0], np.uint8)], []
    for segment in cut_segments(band):
        values, counts = _segment_bits(segment, table, lengths, dynamic_distance, distance)
        parts.append(hr._bits(values, counts))
        info["segment_bits"].append(int(counts.sum()))
        fixed_parts.append(hr._bits(*_segment_bits(segment, FIXED_TABLE, hr.FIXED_LENGTHS, fixed_distance, distance)))
    parts.append(hr._bits(np.array([table[hr.END_OF_BLOCK]]), np.array([lengths[hr.END_OF_BLOCK]])))
    parts.append(np.zeros(3, np.uint8))  # the empty stored block: BFINAL = 0, BTYPE = 00
    fixed_parts.append(np.zeros(7 + 3, np.uint8))
    bits, fixed = np.concatenate(parts), np.concatenate(fixed_parts)
    assert bits.size == dynamic_bits + 3 and fixed.size == fixed_bits + 3
    info["dynamic_data"] = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
    info["fixed_data"] = np.packbits(fixed, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
    info["data"] = info["dynamic_data"] if info["dynamic"] else info["fixed_data"]
    assert len(info["data"]) <= len(info["fixed_data"]) <= band_capacity(len(band))
    return info


def encode_bands(raw, w, h, builder=hr.code_lengths, distance=DISTANCE):
    return [encode_band(b, builder, distance) for b in cut_bands(raw, w, h)]


def header(w, h, n_stream, adler):
    return struct.pack("<16I", MAGIC, w, h, n_stream, adler, band_rows(w), band_count(w, h), *([0] * 9))


def result(raw, w, h, bands=None, fixed=False):
    """The result buffer up to the end of the stream: the 64-byte header, then the stream.  fixed: PTL_PNG_CODES_FIXED, the fixed block in
    every band."""
    bands = bands if bands is not None else encode_bands(raw, w, h)
    body = b"".join(b["fixed_data" if fixed else "data"] for b in bands)
    return header(w, h, len(body), zlib.adler32(raw)) + body


def parse(buffer):
    data = bytes(memoryview(np.ascontiguousarray(buffer)).cast("B")) if not isinstance(buffer, bytes) else buffer
    magic, w, h, n, adler, rows, bands = struct.unpack("<7I", data[:28])
    assert magic == MAGIC and data[28:64] == bytes(36) and len(data) >= HEADER_BYTES + n
    return dict(w=w, h=h, adler=adler, rows=rows, bands=bands, stream=data[HEADER_BYTES: HEADER_BYTES + n])


def inflate(buffer):
    """A result buffer -> raw16, through zlib (which also checks the Adler-32)."""
    p = parse(buffer)
    return zlib.decompress(pr.zlib_stream(p["stream"], p["adler"]))


# ---- a reader for the files ---------------------------------------------------------------------
def read_png16_up(path, header=False):
    """A PNG of colour type 2, bit depth 16, not interlaced, rows of filter type 0 or 2 -> (H, W, 3) uint16 (header=True: that and what the
    file said about itself, the IDAT bodies included).  Asserts on anything else, on a bad CRC and on bytes behind IEND."""
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, chunks = 8, []
    while pos < len(data):
        (length,), kind = struct.unpack(">I", data[pos: pos + 4]), data[pos + 4: pos + 8]
        body = data[pos + 8: pos + 8 + length]
        assert len(body) == length and struct.unpack(">I", data[pos + 8 + length: pos + 12 + length])[0] == zlib.crc32(kind + body), kind
        chunks.append((kind, body))
        pos += 12 + length
    assert pos == len(data) and chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"") and all(k in (b"IHDR", b"IDAT", b"IEND") for k, _ in chunks)
    w, h, depth, colour, compression, filter_method, interlace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, colour, compression, filter_method, interlace) == (16, 2, 0, 0, 0), (depth, colour, compression, filter_method, interlace)
    idat = [body for kind, body in chunks if kind == b"IDAT"]
    lines = np.frombuffer(zlib.decompress(b"".join(idat)), np.uint8)
    assert lines.size == h * (6 * w + 1), "not H rows of 1 + 6 W bytes"
    lines = lines.reshape(h, 6 * w + 1)
    types = lines[:, 0]
    assert np.isin(types, (0, 2)).all() and types[0] == 0, sorted(set(types.tolist()))
    recon = np.zeros((h, 6 * w), np.uint8)
    above = np.zeros(6 * w, np.uint8)
    for y in range(h):  # Recon(x) = Filt(x) + Recon(b), b = the byte above
        recon[y] = lines[y, 1:] + above if types[y] == 2 else lines[y, 1:]
        above = recon[y]
    image = np.ascontiguousarray(recon).view(">u2").reshape(h, w, 3).astype(np.uint16)
    return image if not header else (image, {"width": w, "height": h, "ihdr": chunks[0][1], "filter_types": types.copy(), "idat": idat})
