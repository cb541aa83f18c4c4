"""Frames the tests of the dynamic-code GPU deflate share (tests/test_png_huffman.py on the CPU, tests/test_gpu_png_huffman.py on the GPU)."""
import numpy as np

from tests import png_deflate_reference as pr


def frame_of_raw(body):
    """(H, 4 W) bytes the raw scanlines are to hold behind their filter-type bytes -> the (H, W, 4) frame whose Up filter gives them."""
    body = np.asarray(body, np.uint8)
    return np.cumsum(body.astype(np.uint64), axis=0).astype(np.uint8).reshape(body.shape[0], body.shape[1] // 4, 4)


def fibonacci_frame():
    """1691x1, one band of 6765 raw bytes whose symbol counts are the Fibonacci numbers: end-of-block and the literal 0 of the filter-type byte
    once each, the byte values 1 .. 16 F(3) .. F(18) = 2, 3, 5 ... 2584 times (the last two times more, to fill the row: 6764 bytes); no two
    equal bytes next to each other, so every byte is a literal.  The unlimited Huffman tree of such counts is a chain: 18 symbols, depth 17."""
    fib = [1, 1]
    while len(fib) < 18:
        fib.append(fib[-1] + fib[-2])
    counts = fib[2:]
    counts[-1] += 2
    grouped = np.concatenate([np.full(n, v, np.uint8) for v, n in sorted(zip(range(1, 17), counts), key=lambda p: -p[1])])
    assert grouped.size == 6764 and counts[-1] <= grouped.size // 2
    body = np.empty(grouped.size, np.uint8)
    half = (grouped.size + 1) // 2
    body[0::2], body[1::2] = grouped[:half], grouped[half:]  # the commonest value on the even places, never beside itself
    assert (np.diff(body.astype(int)) != 0).all() and sorted(np.bincount(body)[1:].tolist()) == counts
    return frame_of_raw(body[None, :])


def costly_last_segment_frame():
    """4095x1, one band of 16381 raw bytes in four segments.  The first three hold the values 1 .. 4 only, the last (4093 bytes) goes round the
    250 values 5 .. 254; no two equal bytes are neighbours.  With the band's own code the four common literals cost about 2 bits, the 250 rare
    ones more than 9: the last segment is dearer per byte than any segment of fixed codes can be."""
    rng = np.random.default_rng(4095)
    body = np.empty(4 * 4095, np.uint8)
    common = 3 * pr.SEGMENT - 1
    body[:common] = np.cumsum(rng.integers(1, 4, common)) % 4 + 1
    body[common:] = (np.arange(body.size - common) * 7) % 250 + 5
    assert (np.diff(body.astype(int)) != 0).all() and body.size - common == 4093
    return frame_of_raw(body[None, :])
