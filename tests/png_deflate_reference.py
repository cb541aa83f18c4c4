"""The stream contract of the GPU deflate of 8-bit PNG frames (include/portal_amd.h: ptl_png_deflate_rgba8), restated in numpy,
independent of the product: the raw scanlines of a frame, the cut into bands and segments, the token rule, the bit packing, and the whole
result buffer (header and stream).  The code tables are written out from RFC 1951 3.2.5 / 3.2.6; the Adler-32 is zlib's."""
import struct
import zlib

import numpy as np

SEGMENT = 4096       # runs never cross a multiple of this inside a band
BAND_TARGET = 16384  # a band: as many whole rows as fit into this many raw bytes, at least one
HEADER_BYTES = 64
MAGIC = 0x5A4C5450   # "PTLZ"
MAX_RAW = 1 << 31

# RFC 1951 3.2.5: length codes 257 .. 285 -> (extra bits, first length)
LENGTH_CODES = [(257, 0, 3), (258, 0, 4), (259, 0, 5), (260, 0, 6), (261, 0, 7), (262, 0, 8), (263, 0, 9), (264, 0, 10), (265, 1, 11), (266, 1, 13), (267, 1, 15),
                (268, 1, 17), (269, 2, 19), (270, 2, 23), (271, 2, 27), (272, 2, 31), (273, 3, 35), (274, 3, 43), (275, 3, 51), (276, 3, 59), (277, 4, 67),
                (278, 4, 83), (279, 4, 99), (280, 4, 115), (281, 5, 131), (282, 5, 163), (283, 5, 195), (284, 5, 227), (285, 0, 258)]


def fixed_code(symbol):
    """RFC 1951 3.2.6 -> (code, bits) of a literal/length symbol."""
    if symbol <= 143:
        return 0b00110000 + symbol, 8
    if symbol <= 255:
        return 0b110010000 + (symbol - 144), 9
    if symbol <= 279:
        return symbol - 256, 7
    return 0b11000000 + (symbol - 280), 8


def _reversed(code, bits):
    return int(format(code, f"0{bits}b")[::-1], 2)


def literal_bits(v):
    """(value, count): the bits of literal v in the order they are packed, bit 0 first."""
    code, bits = fixed_code(v)
    return _reversed(code, bits), bits  # Huffman codes go most-significant bit first


def match_bits(length):
    """A match of `length` (3 .. 258) at distance 1: the length code, its extra bits least-significant bit first, distance code 0 (five 0 bits)."""
    symbol, extra, first = [c for c in LENGTH_CODES if c[2] <= length][-1]
    assert 0 <= length - first < (1 << extra) or (extra == 0 and length == first)
    code, bits = fixed_code(symbol)
    return _reversed(code, bits) | ((length - first) << bits), bits + extra + 5


LITERAL = np.array([literal_bits(v) for v in range(256)], np.int64)
MATCH = np.array([(0, 0)] * 3 + [match_bits(n) for n in range(3, 259)], np.int64)


def raw_scanlines(frame):
    """(H, W, 4) uint8 -> what ptl_png_write_level deflates: per row the filter-type byte (0 for row 0, 2 = Up below), then the row minus the
    row above, mod 256."""
    frame = np.ascontiguousarray(frame, np.uint8)
    h, w = frame.shape[:2]
    rows = frame.reshape(h, 4 * w)
    out = np.empty((h, 4 * w + 1), np.uint8)
    out[0, 0], out[1:, 0] = 0, 2
    out[0, 1:] = rows[0]
    out[1:, 1:] = rows[1:] - rows[:-1]
    return out.tobytes()


def band_rows(w):
    return max(1, BAND_TARGET // (4 * w + 1))


def band_count(w, h):
    return -(-h // band_rows(w))


def band_capacity(n):
    """The bound of a band of n raw bytes: 9 bits per byte, 3 + 7 + 3 bits of block headers and end-of-block, 7 of padding, 00 00 FF FF."""
    return -(-(9 * n + 20) // 8) + 4


def cut_bands(raw, w, h):
    """raw -> the bands, whole rows each."""
    step = band_rows(w) * (4 * w + 1)
    assert len(raw) == h * (4 * w + 1)
    return [raw[at: at + step] for at in range(0, len(raw), step)]


def cut_segments(band):
    return [band[at: at + SEGMENT] for at in range(0, len(band), SEGMENT)]


def segment_tokens_plain(segment):
    """The token rule word for word, in plain Python: [("lit", v)] and [("match", length)]."""
    tokens, i, n = [], 0, len(segment)
    while i < n:
        v, run = segment[i], 1
        while i + run < n and segment[i + run] == v:
            run += 1
        tokens.append(("lit", v))
        m = run - 1
        while m >= 3:
            tokens.append(("match", min(m, 258)))
            m -= min(m, 258)
        tokens += [("lit", v)] * m
        i += run
    return tokens


def segment_tokens(segment):
    """The same in numpy -> (values, counts): the bits of every token and how many they are."""
    s = np.frombuffer(segment, np.uint8)
    n = s.size
    starts = np.concatenate(([0], np.flatnonzero(s[1:] != s[:-1]) + 1))
    runs = np.diff(np.concatenate((starts, [n])))
    v = s[starts].astype(np.int64)
    m = runs - 1
    whole, rest = m // 258, m % 258
    last = (rest >= 3).astype(np.int64)
    per_run = 1 + whole + last + np.where(last == 1, 0, rest)
    run_of = np.repeat(np.arange(runs.size), per_run)
    k = np.arange(run_of.size) - np.repeat(np.cumsum(per_run) - per_run, per_run)  # the token's place in its run
    is_258 = (k >= 1) & (k <= whole[run_of])
    is_last = (k == whole[run_of] + 1) & (last[run_of] == 1)
    length = np.where(is_258, 258, np.where(is_last, rest[run_of], 0))
    table = np.where((length > 0)[:, None], MATCH[length], LITERAL[v[run_of]])
    return table[:, 0], table[:, 1]


def tokens_to_bits(tokens):
    """segment_tokens_plain's output -> (values, counts)"""
    pairs = [literal_bits(x) if kind == "lit" else match_bits(x) for kind, x in tokens]
    return np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


def _bits(values, counts):
    """-> one uint8 per bit, in packing order"""
    total = int(counts.sum())
    which = np.repeat(np.arange(counts.size), counts)
    place = np.arange(total) - np.repeat(np.cumsum(counts) - counts, counts)
    return ((values[which] >> place) & 1).astype(np.uint8)


def deflate_band(band, tokens=segment_tokens):
    """One band -> its bytes: a non-final fixed block with the tokens of its segments, end-of-block, an empty stored block."""
    parts = [np.array([0, 1, 0], np.uint8)]  # BFINAL = 0, BTYPE = 01 (least-significant bit first)
    for segment in cut_segments(band):
        parts.append(_bits(*tokens(segment)))
    parts.append(np.zeros(7 + 3, np.uint8))  # end-of-block; BFINAL = 0, BTYPE = 00
    bits = np.concatenate(parts)
    out = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"  # (packbits pads the last byte with zeros)
    assert len(out) <= band_capacity(len(band))
    return out


def band_streams(frame):
    h, w = frame.shape[:2]
    return [deflate_band(b) for b in cut_bands(raw_scanlines(frame), w, h)]


def stream(frame):
    """The bands, one behind the other: what the result buffer holds behind its header."""
    return b"".join(band_streams(frame))


def zlib_stream(body, adler):
    """78 01, the bands, 03 00 (an empty final fixed block), the Adler-32 of raw, big-endian: the contents of the file's one IDAT."""
    return b"\x78\x01" + body + b"\x03\x00" + struct.pack(">I", adler)


def header(w, h, n_stream, adler):
    return struct.pack("<16I", MAGIC, w, h, n_stream, adler, band_rows(w), band_count(w, h), *([0] * 9))


def result(frame):
    """The result buffer up to the end of the stream: the 64-byte header, then the stream."""
    h, w = frame.shape[:2]
    body = stream(frame)
    return header(w, h, len(body), zlib.adler32(raw_scanlines(frame))) + body


def parse(buffer):
    """A result buffer (bytes or uint8 array, at least header + stream) -> dict(w, h, adler, rows, bands, stream)."""
    data = bytes(memoryview(np.ascontiguousarray(buffer)).cast("B")) if not isinstance(buffer, bytes) else buffer
    magic, w, h, n, adler, rows, bands = struct.unpack("<7I", data[:28])
    assert magic == MAGIC and data[28:64] == bytes(36) and len(data) >= HEADER_BYTES + n
    return dict(w=w, h=h, adler=adler, rows=rows, bands=bands, stream=data[HEADER_BYTES: HEADER_BYTES + n])


def inflate(buffer):
    """A result buffer -> raw, through zlib (which also checks the Adler-32)."""
    p = parse(buffer)
    return zlib.decompress(zlib_stream(p["stream"], p["adler"]))


def stream_capacity(w, h):
    full, bands = band_rows(w) * (4 * w + 1), band_count(w, h)
    return (bands - 1) * band_capacity(full) + band_capacity(h * (4 * w + 1) - (bands - 1) * full)


def result_bytes(w, h):
    """ptl_png_stream_bytes: header | room for the longest stream, rounded up to 16 | a 16-byte table entry per band | a slot per band."""
    slot = (band_capacity(band_rows(w) * (4 * w + 1)) + 15) // 16 * 16
    return HEADER_BYTES + (stream_capacity(w, h) + 15) // 16 * 16 + band_count(w, h) * (16 + slot)


def undo_up(raw, w, h):
    """raw -> the (H, W, 4) frame"""
    rows = np.frombuffer(raw, np.uint8).reshape(h, 4 * w + 1)
    assert rows[0, 0] == 0 and (rows[1:, 0] == 2).all()
    return np.cumsum(rows[:, 1:].astype(np.uint64), axis=0).astype(np.uint8).reshape(h, w, 4)
