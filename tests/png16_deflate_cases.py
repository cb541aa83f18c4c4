"""Frames for the tests of the GPU deflate of 16-bit PNG frames (tests/test_png16_deflate.py, tests/test_gpu_png16_deflate.py), as (H, W, 3)
arrays of 16-bit values A.  Row 0 of a frame is not filtered, so the raw bytes of an H = 1 frame can be chosen freely: `frame_of_row`."""
import numpy as np

from tests import png16_deflate_reference as r6


def frame_of_row(body):
    """Bytes (padded with 5s to whole pixels) -> the 1-row frame whose raw16 is 0 | body."""
    body = list(body)
    body += [5] * (-len(body) % 6)
    row = np.array(body, np.uint8).reshape(1, -1)
    assert r6.raw16_of_rows(row) == bytes([0]) + row.tobytes()
    return r6.a_of_rows(row)


def noise(w, h, seed=0):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 65536, (h, w, 3)).astype(np.int64)


def one_colour(w, h, value=(0x1234, 0xfedc, 0x8000)):
    return np.tile(np.array(value, np.int64), (h, w, 1))


def mixed(w, h, seed=0):
    """Noise with stretches of repeated pixels, and rows that repeat the row above."""
    rng = np.random.default_rng(seed + 7000 * w + h)
    a = np.repeat(rng.integers(0, 65536, (h, -(-w // 5), 3)), 5, axis=1)[:, :w].astype(np.int64)
    speck = rng.random((h, w)) < 0.15
    a[speck] = rng.integers(0, 65536, (int(speck.sum()), 3))
    a[2::3] = a[1::3][: len(a[2::3])]
    return a


def every_literal():
    v = np.arange(256)
    return frame_of_row(np.concatenate([v, v[::-1], (v * 7 + 3) % 256, (v * 151 + 144) % 256]))


def covered_stretches():
    """Covered stretches of 1 .. 20, 257 .. 263 and 515 .. 521 bytes: a pixel of six distinct bytes, repeated for as long as the stretch asks,
    then a pixel that differs in every byte -- wherever they fall relative to the segment boundaries (a stretch that crosses one is cut: the
    six bytes behind the boundary are literals)."""
    body, k = [], 0
    for n in list(range(1, 21)) + list(range(257, 264)) + list(range(515, 522)):
        pixel = [(17 * k + 31 * j + 1) % 256 for j in range(6)]
        body += (pixel * (n // 6 + 2))[: 6 + n]
        body += [(b + 128) % 256 for b in (pixel * 2)[(6 + n) % 6: (6 + n) % 6 + 6]]  # differs from the byte six back in every place
        k += 1
    return frame_of_row(body)


def across_a_segment_boundary():
    """One pixel repeated over 3 segments and a half: every segment starts with six literals, then matches of 258."""
    return frame_of_row([1, 2, 3, 4, 5, 6] * 2400)


def distance_one_not_six():
    """Equal at distance 1 but not at 6: runs of five equal bytes (nothing to match), then equal at 6 but not at 1: a pixel of six distinct
    bytes repeated."""
    runs = [v for k in range(300) for v in [(k * 37 + 1) % 256] * 5]
    pixels = [10, 20, 30, 40, 50, 60] * 300
    return frame_of_row(runs + pixels + runs[:700])


def fibonacci():
    """1127x1, one band of 6763 raw bytes whose symbol counts are the Fibonacci numbers: end-of-block and the literal 0 of the filter-type byte
    once each, the byte values 1 .. 16 F(3) .. F(18) = 2, 3, 5 ... 2584 times (6762 bytes); no byte equals the byte six back, so every byte is
    a literal.  The unlimited Huffman tree of such counts is a chain: 18 symbols, depth 17.  (The six byte lanes i, i + 6, i + 12 ... are laid
    end to end, and along that chain the commonest values go on the even places, never beside themselves.)"""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    counts = fib[2:]
    grouped = np.concatenate([np.full(n, v, np.uint8) for v, n in sorted(zip(range(1, 17), counts), key=lambda p: -p[1])])
    assert grouped.size == 6762 == 6 * 1127 and counts[-1] <= grouped.size // 2
    chain = np.empty(grouped.size, np.uint8)
    half = (grouped.size + 1) // 2
    chain[0::2], chain[1::2] = grouped[:half], grouped[half:]
    body = chain.reshape(6, 1127).T.reshape(-1)  # chain place 1127 lane + k -> byte 6 k + lane
    assert (body[6:] != body[:-6]).all() and sorted(np.bincount(body)[1:].tolist()) == counts
    return frame_of_row(body)


def costly_last_segment():
    """2730x1, one band of 16381 raw bytes in four segments.  The first three hold the values 1 .. 4 only, the last (4093 bytes) goes round the
    250 values 5 .. 254; no byte equals the byte six back.  With the band's own code the four common literals cost about 2 bits, the 250 rare
    ones more than 9: the last segment is dearer per byte than any segment of fixed codes can be."""
    rng = np.random.default_rng(2730)
    body = np.empty(6 * 2730, np.uint8)
    common = 3 * r6.SEGMENT - 1
    lanes = np.cumsum(rng.integers(1, 4, (common // 6 + 1, 6)), axis=0) % 4 + 1  # every lane a walk with steps of 1 .. 3 mod 4
    body[:common] = lanes.reshape(-1)[:common]
    body[common:] = (np.arange(body.size - common) * 7) % 250 + 5
    assert (body[6:] != body[:-6]).all() and body.size - common == 4093
    return frame_of_row(body)


def both_choices():
    """64x43 noise: a band is 42 rows (16170 bytes, its own code pays for the block header); the last band is one row of 385 bytes, which a
    header does not pay for."""
    return noise(64, 43, 64)


def period_six_rows(w, h, seed=3, carry=False):
    """Each row is the row above plus a constant per byte lane of the pixel, mod 256: the Up differences have exactly period 6, so every row
    below the first is six literals and matches.  carry=True: plus a constant per 16-bit sample instead, mod 65536 -- the high byte's
    difference then depends on the carry out of the low byte, and the period breaks wherever a sample carries."""
    rng = np.random.default_rng(seed)
    if carry:
        first, steps = rng.integers(0, 65536, (1, w, 3)), rng.integers(0, 65536, (h, 1, 3))
        steps[0] = 0
        return ((first + np.cumsum(steps, axis=0)) % 65536).astype(np.int64)
    first, steps = rng.integers(0, 256, (1, w, 6)), rng.integers(0, 256, (h, 1, 6))
    steps[0] = 0
    return r6.a_of_rows(((first + np.cumsum(steps, axis=0)) % 256).astype(np.uint8).reshape(h, 6 * w))


def all_255_differences(w, h):
    """Every byte of every row below the first is 255 more than the byte above it (mod 256), and row 0 is all 255: raw16 is 255 wherever
    it is not a filter-type byte -- the largest Adler sums."""
    rows = np.zeros((h, 6 * w), np.uint8)
    for y in range(h):
        rows[y] = (255 * (y + 1)) % 256
    a = r6.a_of_rows(rows)
    raw = np.frombuffer(r6.raw16(a), np.uint8).reshape(h, 6 * w + 1)
    assert (raw[:, 1:] == 255).all()
    return a
