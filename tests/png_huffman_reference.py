"""The stream contract of the GPU deflate with per-band dynamic Huffman codes (include/portal_amd.h: ptl_png_deflate_rgba8_codes, PTL_PNG_CODES_DYNAMIC;
DESIGN.md 2.3.6), restated in numpy and plain Python, independent of the product.  The raw scanlines, the cut into bands and segments and the
token rule are those of tests/png_deflate_reference.py; new here are the band's histogram, its length-limited prefix code, the block header
of RFC 1951 3.2.7 and the choice between the dynamic and the fixed block.  The tables are written out from RFC 1951."""
import heapq
import zlib

import numpy as np

from tests import png_deflate_reference as pr

END_OF_BLOCK = 256
N_SYMBOLS = 286
LIMIT = 15
# RFC 1951 3.2.7: the order in which the lengths of the code-length code are stored
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# The contract's one code-length code (a complete code, index = symbol 0 .. 18): zero lengths and their long repeats cost 3 bits, the common
# lengths 2 .. 9 and the repeats 16 / 17 four, the rare ones up to 7.  The last symbol of CL_ORDER has a length, so HCLEN is always 15.
CL_LENGTHS = (3, 7, 4, 4, 4, 4, 4, 4, 4, 4, 5, 5, 6, 6, 6, 7, 4, 4, 3)
assert sum(2 ** (7 - n) for n in CL_LENGTHS) == 2 ** 7 and len(CL_LENGTHS) == 19

# per match length 3 .. 258: symbol, extra bits, their value (RFC 1951 3.2.5)
LENGTH_SYMBOL = np.zeros(259, np.int64)
LENGTH_EXTRA_BITS = np.zeros(259, np.int64)
LENGTH_EXTRA = np.zeros(259, np.int64)
for _symbol, _extra, _first in pr.LENGTH_CODES:
    for _n in range(_first, min(259, _first + (1 << _extra))):
        if _symbol == 284 and _n == 258:
            continue  # 258 is symbol 285's
        LENGTH_SYMBOL[_n], LENGTH_EXTRA_BITS[_n], LENGTH_EXTRA[_n] = _symbol, _extra, _n - _first
SYMBOL_EXTRA_BITS = np.zeros(N_SYMBOLS, np.int64)
SYMBOL_EXTRA_BITS[LENGTH_SYMBOL[3:]] = LENGTH_EXTRA_BITS[3:]
FIXED_LENGTHS = np.array([pr.fixed_code(s)[1] for s in range(N_SYMBOLS)], np.int64)


# ---- tokens as symbols ------------------------------------------------------------------------
def segment_symbols_plain(segment):
    """The token rule in plain Python -> [(symbol, extra value, extra bits)]."""
    out = []
    for kind, x in pr.segment_tokens_plain(segment):
        out.append((x, 0, 0) if kind == "lit" else (int(LENGTH_SYMBOL[x]), int(LENGTH_EXTRA[x]), int(LENGTH_EXTRA_BITS[x])))
    return out


def segment_symbols(segment):
    """The same in numpy -> (symbols, extra values, extra bits)."""
    s = np.frombuffer(segment, np.uint8)
    starts = np.concatenate(([0], np.flatnonzero(s[1:] != s[:-1]) + 1))
    runs = np.diff(np.concatenate((starts, [s.size])))
    m = runs - 1
    whole, rest = m // 258, m % 258
    last = (rest >= 3).astype(np.int64)
    per_run = 1 + whole + last + np.where(last == 1, 0, rest)
    run_of = np.repeat(np.arange(runs.size), per_run)
    k = np.arange(run_of.size) - np.repeat(np.cumsum(per_run) - per_run, per_run)
    length = np.where((k >= 1) & (k <= whole[run_of]), 258, np.where((k == whole[run_of] + 1) & (last[run_of] == 1), rest[run_of], 0))
    return np.where(length > 0, LENGTH_SYMBOL[length], s[starts].astype(np.int64)[run_of]), LENGTH_EXTRA[length], LENGTH_EXTRA_BITS[length]


def band_histogram(band, symbols=segment_symbols):
    """The 286 counts of a band's tokens, end-of-block counted once."""
    hist = np.zeros(N_SYMBOLS, np.int64)
    for segment in pr.cut_segments(band):
        hist += np.bincount(np.asarray([t[0] for t in symbols(segment)] if symbols is segment_symbols_plain else symbols(segment)[0], np.int64), minlength=N_SYMBOLS)
    hist[END_OF_BLOCK] += 1
    return hist


# ---- the code builder -------------------------------------------------------------------------
def _repair(count, limit):
    """Per-length leaf counts with everything deeper than `limit` already counted at `limit` -> counts of a complete code.  While the Kraft sum
    (in units of 2^-limit) exceeds 2^limit: one leaf less at `limit`; the deepest length below `limit` that has a leaf gives one up, and the
    length below it gains two.  Each round takes exactly one unit off the sum and keeps the number of leaves."""
    count = [int(c) for c in count]
    total = sum(c << (limit - n) for n, c in enumerate(count) if n > 0)
    while total > 1 << limit:
        count[limit] -= 1
        n = max(k for k in range(1, limit) if count[k] > 0)
        count[n] -= 1
        count[n + 1] += 2
        total -= 1
    assert total == 1 << limit
    return count


def code_lengths_plain(hist, limit=LIMIT):
    """Plain Python, the two-queue form.  The used symbols sorted by (count, symbol) are the leaves; merged nodes queue up behind each other in
    the order they are made.  Each merge takes twice the lighter of the two queue heads, the leaf on a tie.  A leaf's depth is its number of
    edges to the root; depths beyond `limit` count as `limit`, the counts are repaired (_repair), and the lengths go to the symbols in sorted
    order, the longest to the rarest.  -> (lengths per symbol, the unlimited depth of the tree)"""
    used = sorted((int(c), s) for s, c in enumerate(hist) if c > 0)
    n = len(used)
    assert n >= 2
    weight, parent = [c for c, _ in used], [0] * (2 * n - 1)
    leaf, head = 0, n
    for made in range(n, 2 * n - 1):
        picks = []
        for _ in range(2):
            if leaf < n and (head >= len(weight) or weight[leaf] <= weight[head]):
                picks.append(leaf)
                leaf += 1
            else:
                picks.append(head)
                head += 1
        weight.append(weight[picks[0]] + weight[picks[1]])
        for p in picks:
            parent[p] = made
    depth = [0] * (2 * n - 1)
    for node in range(2 * n - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    count = [0] * (limit + 1)
    for d in depth[:n]:
        count[min(d, limit)] += 1
    count = _repair(count, limit)
    lengths, at = [0] * len(hist), 0
    for bits in range(limit, 0, -1):
        for _, s in used[at: at + count[bits]]:
            lengths[s] = bits
        at += count[bits]
    assert at == n
    return lengths, max(depth[:n])


def code_lengths(hist, limit=LIMIT):
    """The same rule in another form: a heap keyed by (weight, leaf before merged node, place in the sorted order or order of making), depths by
    pointer jumping, counts and lengths with numpy.  -> lengths per symbol (an int64 array)"""
    hist = np.asarray(hist, np.int64)
    order = np.lexsort((np.arange(hist.size), hist))
    order = order[hist[order] > 0]
    n = order.size
    assert n >= 2
    heap = [(int(hist[s]), 0, k) for k, s in enumerate(order)]
    heapq.heapify(heap)
    parent = np.zeros(2 * n - 1, np.int64)
    for made in range(n, 2 * n - 1):
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[2]] = parent[b[2]] = made
        heapq.heappush(heap, (a[0] + b[0], 1, made))
    root = 2 * n - 2
    parent[root] = root
    depth, up = (np.arange(2 * n - 1) != root).astype(np.int64), parent.copy()
    for _ in range(int(2 * n).bit_length()):
        depth, up = depth + depth[up], up[up]
    count = _repair(np.bincount(np.minimum(depth[:n], limit), minlength=limit + 1), limit)
    lengths = np.zeros(hist.size, np.int64)
    lengths[order] = np.repeat(np.arange(limit, 0, -1), np.array(count[limit:0:-1]))
    return lengths


def canonical_codes(lengths):
    """RFC 1951 3.2.2 -> the code of every symbol with a length (0 elsewhere)."""
    lengths = [int(n) for n in lengths]
    count = [0] * (max(lengths) + 2)
    for n in lengths:
        if n:
            count[n] += 1
    code, first = 0, [0] * len(count)
    for bits in range(1, len(count)):
        code = (code + count[bits - 1]) << 1
        first[bits] = code
    out = []
    for n in lengths:
        out.append(first[n] if n else 0)
        first[n] += 1 if n else 0
    return out


def _reversed(code, bits):
    return int(format(code, f"0{bits}b")[::-1], 2) if bits else 0


CL_CODES = [(_reversed(c, n), n) for c, n in zip(canonical_codes(CL_LENGTHS), CL_LENGTHS)]


# ---- the block header -------------------------------------------------------------------------
def length_sequence_tokens(sequence):
    """The greedy rule for the HLIT + 257 literal/length lengths followed by the one distance length, as one sequence.  For every maximal run of
    r equal lengths v.  v = 0: while r >= 138, symbol 18 with 138; then 18 with r if r >= 11, 17 with r if r >= 3, else r times symbol 0.
    v > 0: symbol v; m = r - 1; while m >= 6, symbol 16 with 6; then 16 with m if m >= 3, else m times symbol v.
    -> [(symbol, extra value, extra bits)]"""
    out, at = [], 0
    while at < len(sequence):
        v, r = sequence[at], 1
        while at + r < len(sequence) and sequence[at + r] == v:
            r += 1
        at += r
        if v == 0:
            while r >= 138:
                out.append((18, 127, 7))
                r -= 138
            out += [(18, r - 11, 7)] if r >= 11 else [(17, r - 3, 3)] if r >= 3 else [(0, 0, 0)] * r
        else:
            out.append((v, 0, 0))
            m = r - 1
            while m >= 6:
                out.append((16, 3, 2))
                m -= 6
            out += [(16, m - 3, 2)] if m >= 3 else [(v, 0, 0)] * m
    return out


def block_header(lengths):
    """BFINAL = 0, BTYPE = 10, HLIT, HDIST = 0, HCLEN = 15, the 19 lengths of the code-length code, the coded lengths -> (values, counts) to
    pack least-significant bit first."""
    lengths = [int(n) for n in lengths]
    n_lit = max(s for s, n in enumerate(lengths) if n) + 1
    assert n_lit >= 257
    pairs = [(0, 1), (2, 2), (n_lit - 257, 5), (0, 5), (15, 4)] + [(CL_LENGTHS[s], 3) for s in CL_ORDER]
    for symbol, extra, extra_bits in length_sequence_tokens(lengths[:n_lit] + [1]):  # the one distance code: code 0, one bit
        code, bits = CL_CODES[symbol]
        pairs.append((code | (extra << bits), bits + extra_bits))
    return np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)


def _bits(values, counts):
    total = int(counts.sum())
    which = np.repeat(np.arange(counts.size), counts)
    place = np.arange(total) - np.repeat(np.cumsum(counts) - counts, counts)
    return ((values[which] >> place) & 1).astype(np.uint8)


# ---- a band -----------------------------------------------------------------------------------
def encode_band(band, builder=code_lengths):
    """One band -> dict(data: its bytes, dynamic: which block it chose, lengths, header_bits, dynamic_bits, fixed_bits, segment_bits: the
    dynamic block's token bits per segment).  The block sizes count the block header, the tokens and end-of-block; the empty stored block
    behind them is the same for both.  Dynamic only where it has FEWER bits."""
    hist = band_histogram(band)
    lengths = np.asarray(builder(hist)[0] if builder is code_lengths_plain else builder(hist), np.int64)
    assert ((lengths > 0) == (hist > 0)).all() and lengths.max() <= LIMIT and sum(2.0 ** -n for n in lengths[lengths > 0]) == 1.0
    head_values, head_counts = block_header(lengths)
    matches = int(hist[257:].sum())
    extra = int((hist * SYMBOL_EXTRA_BITS).sum())
    dynamic_bits = int(head_counts.sum()) + int((hist * lengths).sum()) + extra + matches
    fixed_bits = 3 + int((hist * FIXED_LENGTHS).sum()) + extra + 5 * matches
    info = dict(dynamic=dynamic_bits < fixed_bits, lengths=lengths, header_bits=int(head_counts.sum()), dynamic_bits=dynamic_bits, fixed_bits=fixed_bits, hist=hist)
    fixed = pr.deflate_band(band)
    assert len(fixed) == -(-(fixed_bits + 3) // 8) + 4
    codes = canonical_codes(lengths)
    table = np.array([_reversed(c, int(n)) for c, n in zip(codes, lengths)], np.int64)
    parts, info["segment_bits"] = [_bits(head_values, head_counts)], []
    for segment in pr.cut_segments(band):
        symbols, extras, extra_bits = segment_symbols(segment)
        counts = lengths[symbols] + extra_bits + (symbols >= 257)  # the distance code: one 0 bit
        parts.append(_bits(table[symbols] | (extras << lengths[symbols]), counts))
        info["segment_bits"].append(int(counts.sum()))
    parts.append(_bits(np.array([table[END_OF_BLOCK]]), np.array([lengths[END_OF_BLOCK]])))
    parts.append(np.zeros(3, np.uint8))  # the empty stored block: BFINAL = 0, BTYPE = 00
    bits = np.concatenate(parts)
    assert bits.size == dynamic_bits + 3
    dynamic = np.packbits(bits, bitorder="little").tobytes() + b"\x00\x00\xff\xff"
    info["data"] = dynamic if info["dynamic"] else fixed
    info["dynamic_data"] = dynamic
    assert len(info["data"]) <= len(fixed) <= pr.band_capacity(len(band))
    return info


def encode_bands(frame, builder=code_lengths):
    h, w = frame.shape[:2]
    return [encode_band(b, builder) for b in pr.cut_bands(pr.raw_scanlines(frame), w, h)]


def stream(frame):
    return b"".join(b["data"] for b in encode_bands(frame))


def result(frame, bands=None):
    """The result buffer up to the end of the stream: the same 64-byte header as the fixed mode's, then the stream."""
    h, w = frame.shape[:2]
    body = b"".join(b["data"] for b in (bands if bands is not None else encode_bands(frame)))
    return pr.header(w, h, len(body), zlib.adler32(pr.raw_scanlines(frame))) + body


def read_block_header(data):
    """The start of a band's bytes -> None for a fixed block, else the literal/length lengths an inflater would read from its dynamic header
    (a check of the header that does not go through the writer above)."""
    bits = np.unpackbits(np.frombuffer(data[:400], np.uint8), bitorder="little")
    at = 0

    def take(n):
        nonlocal at
        v = int(sum(int(b) << k for k, b in enumerate(bits[at: at + n])))
        at += n
        return v

    assert take(1) == 0
    kind = take(2)
    if kind == 1:
        return None
    assert kind == 2
    n_lit, n_dist, n_cl = take(5) + 257, take(5) + 1, take(4) + 4
    cl = [0] * 19
    for s in CL_ORDER[:n_cl]:
        cl[s] = take(3)
    decode = {(n, c): s for s, (c, n) in enumerate(zip(canonical_codes(cl), cl)) if n}
    out = []
    while len(out) < n_lit + n_dist:
        code = n = 0
        while (n, code) not in decode:
            code, n = (code << 1) | take(1), n + 1
            assert n <= 7
        s = decode[(n, code)]
        out += [s] if s < 16 else [out[-1]] * (3 + take(2)) if s == 16 else [0] * (3 + take(3)) if s == 17 else [0] * (11 + take(7))
    assert len(out) == n_lit + n_dist and out[n_lit:] == [1]
    return out[:n_lit]
