"""tests/yuv_chroma_reference.py -- numpy restatement of the frames ptl_average_to_yuv10 and ptl_average_f32_to_yuv10 write at the three
chroma samplings (include/portal_amd.h).

TEST INFRASTRUCTURE ONLY: written from the formulas of the contract; shares no code with the kernels and no chroma code with
tests/yuv_reference.py / tests/yuv_deep_reference.py.  The averaged frame A is taken from those: for RGBA8 sub-frames the frame
oracle.postprocess.average_images gives (8-bit values), for float sub-frames yuv_deep_reference.encode16 (16-bit values).

    bits  luma                                                     chroma rows (Cb; Cr)                             k at 420 / 422 / 444
    8     (55896 R + 188037 G + 18982 B + 32768) >> 16             -30123 -101335 131458; 131458 -119404 -12054      19 / 18 / 16
    16    (13920 R + 46826 G + 4727 B + (1 << 21)) >> 22           -15003 -50470 65473;   65473 -59470 -6003         26 / 25 / 23
    C = min(1023, (row . S + (512 << k) + (1 << (k - 1))) >> k)
    S at 444: A(x, y), cw = W, ch = H.   422: A(2i-1, y) + 2 A(2i, y) + A(2i+1, y), columns clamped, cw = (W+1)/2, ch = H.
    420: the 422 sums of rows 2j and 2j+1 (row clamped) added, ch = (H+1)/2.
Payload: Y (W*H little-endian uint16), then Cb, then Cr (cw*ch each).
"""
import numpy as np

SAMPLINGS = (420, 422, 444)
LUMA = {8: ((55896, 188037, 18982), 16), 16: ((13920, 46826, 4727), 22)}
ROWS = {8: ((-30123, -101335, 131458), (131458, -119404, -12054)), 16: ((-15003, -50470, 65473), (65473, -59470, -6003))}
SHIFT = {8: {420: 19, 422: 18, 444: 16}, 16: {420: 26, 422: 25, 444: 23}}
TAPS = {420: 8, 422: 4, 444: 1}  # the weights of S add up to this
# the smallest accumulators there are (yellow's Cb, cyan's Cr), as the contract states them
MINIMA = {8: {422: 261640, 444: 65410}, 16: {422: 33554180, 444: 8388545}}


def plane_size(w, h, chroma):
    return {420: ((w + 1) // 2, (h + 1) // 2), 422: ((w + 1) // 2, h), 444: (w, h)}[chroma]


def frame_bytes(w, h, chroma):
    cw, ch = plane_size(w, h, chroma)
    return 2 * (w * h + 2 * cw * ch)


def y4m_header(w, h, fps, chroma):
    return f"YUV4MPEG2 W{w} H{h} F{fps}:1 Ip A1:1 C{chroma}p10 XYSCSS={chroma}P10 XCOLORRANGE=FULL\n".encode()


def weighted_sums(a, chroma):
    """(H, W, 3) int64 -> S, (ch, cw, 3)."""
    h, w = a.shape[:2]
    if chroma == 444:
        return a
    i = np.arange((w + 1) // 2)
    across = a[:, np.maximum(2 * i - 1, 0)] + 2 * a[:, 2 * i] + a[:, np.minimum(2 * i + 1, w - 1)]
    if chroma == 422:
        return across
    j = np.arange((h + 1) // 2)
    return across[2 * j] + across[np.minimum(2 * j + 1, h - 1)]


def planes(a, chroma, bits, clamp=True):
    """A (H, W, >= 3), `bits`-bit values -> (Y (H, W), Cb (ch, cw), Cr (ch, cw)) int64.  clamp=False: the chroma before min(1023, .).
    Asserts what the contract promises of its arithmetic: every accumulator positive, the 8-bit ones inside 32 bits, nothing above 1024."""
    assert chroma in SAMPLINGS and bits in (8, 16)
    a = np.asarray(a)[..., :3].astype(np.int64)
    assert a.ndim == 3 and int(a.min(initial=0)) >= 0 and int(a.max(initial=0)) < 1 << bits
    (kr, kg, kb), luma_shift = LUMA[bits]
    y = (kr * a[..., 0] + kg * a[..., 1] + kb * a[..., 2] + (1 << (luma_shift - 1))) >> luma_shift
    s = weighted_sums(a, chroma)
    assert s.shape[:2] == plane_size(a.shape[1], a.shape[0], chroma)[::-1] and int(s.max(initial=0)) <= TAPS[chroma] * ((1 << bits) - 1)
    k = SHIFT[bits][chroma]
    out = []
    for row in ROWS[bits]:
        acc = row[0] * s[..., 0] + row[1] * s[..., 1] + row[2] * s[..., 2] + (512 << k) + (1 << (k - 1))
        assert int(acc.min(initial=1)) > 0, "an accumulator is not positive: >> would not be a plain shift"
        if chroma in MINIMA[bits]:
            assert int(acc.min(initial=1 << 62)) >= MINIMA[bits][chroma]
        assert bits == 16 or int(acc.max(initial=0)) < 1 << 31, "an 8-bit accumulator leaves 32 bits"
        c = acc >> k
        assert int(c.max(initial=0)) <= 1024
        out.append(np.minimum(1023, c) if clamp else c)
    return y, out[0], out[1]


def payload(a, chroma, bits, clamp=True) -> bytes:
    """The payload of one Y4M frame.  (clamp=False: what a kernel without the min would write; 1024 fits a uint16.)"""
    return b"".join(np.ascontiguousarray(p).astype("<u2").tobytes() for p in planes(a, chroma, bits, clamp))


def split_planes(data: bytes, w, h, chroma):
    """payload -> (Y, Cb, Cr) uint16 arrays."""
    cw, ch = plane_size(w, h, chroma)
    flat = np.frombuffer(data, "<u2")
    assert flat.size == w * h + 2 * cw * ch
    return flat[: w * h].reshape(h, w), flat[w * h: w * h + cw * ch].reshape(ch, cw), flat[w * h + cw * ch:].reshape(ch, cw)


def real_valued(colours, bits):
    """H.273 (BT.709, full range, 10 bit) on flat colours in real numbers, unclamped: (K, 3) -> (Y, Cb, Cr) float64."""
    kr, kg, kb = 0.2126, 0.7152, 0.0722
    e = np.asarray(colours, np.float64) / float((1 << bits) - 1)
    ey = kr * e[:, 0] + kg * e[:, 1] + kb * e[:, 2]
    return 1023.0 * ey, 1023.0 * (e[:, 2] - ey) / (2.0 * (1.0 - kb)) + 512.0, 1023.0 * (e[:, 0] - ey) / (2.0 * (1.0 - kr)) + 512.0
