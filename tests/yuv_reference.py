"""tests/yuv_reference.py -- numpy restatement of the frame ptl_average_to_yuv420p10 writes (include/portal_amd.h).

TEST INFRASTRUCTURE ONLY: written from the formulas of the contract, shares no code with the kernel.

The frame is a pure function of the RGBA8 frame A the PNG path would have written (alpha ignored).  BT.709 matrix on the
gamma-encoded values, full range, 10 bit, all arithmetic 32-bit integer (every accumulator is positive and below 2^30):
    Y  = (55896 R + 188037 G + 18982 B + 32768) >> 16
    S_c = sum over rows 2j, 2j+1 of A_c(2i-1) + 2 A_c(2i) + A_c(2i+1), coordinates clamped to the frame  (MPEG-2 siting)
    Cb = min(1023, (-30123 S_R - 101335 S_G + 131458 S_B + (512 << 19) + (1 << 18)) >> 19)
    Cr = min(1023, (131458 S_R - 119404 S_G - 12054 S_B + (512 << 19) + (1 << 18)) >> 19)
Payload: the Y plane (W*H little-endian uint16, row 0 on top), then Cb and Cr ((W+1)/2 * (H+1)/2 each).
"""
import numpy as np

KR, KG, KB = 0.2126, 0.7152, 0.0722


def yuv_planes(rgba8, clamp=True):
    """(H, W, >=3) uint8 -> (Y (H, W), Cb (ch, cw), Cr (ch, cw)) as int32.  clamp=False: the chroma values before min(1023, .) -- not
    what the kernel writes; tests use it to show that an input reaches the clamp (pure blue and pure red give 1024)."""
    a = np.asarray(rgba8)[..., :3].astype(np.int32)
    h, w = a.shape[:2]
    y = (55896 * a[..., 0] + 188037 * a[..., 1] + 18982 * a[..., 2] + 32768) >> 16
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rows = 2 * np.arange(ch)
    two_rows = a[rows] + a[np.minimum(rows + 1, h - 1)]  # (ch, W, 3)
    cols = 2 * np.arange(cw)
    s = two_rows[:, np.maximum(cols - 1, 0)] + 2 * two_rows[:, cols] + two_rows[:, np.minimum(cols + 1, w - 1)]  # (ch, cw, 3), 0..2040
    bias = (512 << 19) + (1 << 18)
    cb = (-30123 * s[..., 0] - 101335 * s[..., 1] + 131458 * s[..., 2] + bias) >> 19
    cr = (131458 * s[..., 0] - 119404 * s[..., 1] - 12054 * s[..., 2] + bias) >> 19
    if clamp:
        cb, cr = np.minimum(1023, cb), np.minimum(1023, cr)
    return y, cb, cr


def yuv_reference(rgba8) -> bytes:
    """The payload of one Y4M frame (C420p10, full range) for the RGBA8 frame `rgba8`."""
    return b"".join(np.ascontiguousarray(p).astype("<u2").tobytes() for p in yuv_planes(rgba8))


def frame_bytes(w: int, h: int) -> int:
    return 2 * (w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2))


def y4m_header(w: int, h: int, fps: int) -> bytes:
    return f"YUV4MPEG2 W{w} H{h} F{fps}:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n".encode()


def split_planes(payload: bytes, w: int, h: int):
    """payload -> (Y, Cb, Cr) uint16 arrays."""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    flat = np.frombuffer(payload, "<u2")
    assert flat.size == w * h + 2 * cw * ch
    return flat[: w * h].reshape(h, w), flat[w * h: w * h + cw * ch].reshape(ch, cw), flat[w * h + cw * ch:].reshape(ch, cw)


def real_valued(rgb):
    """H.273 on flat colours, real-valued and unclamped: (K, 3) values 0..255 -> (Y, Cb, Cr) float64, 10-bit full range."""
    e = np.asarray(rgb, np.float64) / 255.0
    ey = KR * e[:, 0] + KG * e[:, 1] + KB * e[:, 2]
    epb = (e[:, 2] - ey) / (2.0 * (1.0 - KB))
    epr = (e[:, 0] - ey) / (2.0 * (1.0 - KR))
    return 1023.0 * ey, 1023.0 * epb + 512.0, 1023.0 * epr + 512.0
