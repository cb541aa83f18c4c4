"""tests/yuv_deep_reference.py -- numpy restatement of the frame ptl_average_f32_to_yuv420p10 writes (include/portal_amd.h).

TEST INFRASTRUCTURE ONLY: written from the formulas of the contract, shares no code with the kernel.

Input: n (1 .. 256) RGBA32F sub-frames, gamma-2 encoded, alpha ignored.  ONE quantisation in float32, to 16 bits:
    q(v) = 0 if !(v > 0), 65535 if v >= 1, else floor(v * 65535.0f + 0.5f)        product and sum each rounded to binary32
then integers (int64 / uint64 / Python int), per pixel and channel:
    M = floor(sum_k q_k^2 / n),    E = the e with e (e - 1) < M <= e (e + 1)      (math.isqrt, no floating point)
    Y  = (13920 E_R + 46826 E_G + 4727 E_B + (1 << 21)) >> 22
    S_c = sum over rows 2j, 2j+1 of E_c(2i-1) + 2 E_c(2i) + E_c(2i+1), coordinates clamped to the frame  (MPEG-2 siting, 0 .. 524 280)
    Cb = min(1023, (-15003 S_R - 50470 S_G + 65473 S_B + (512 << 26) + (1 << 25)) >> 26)
    Cr = min(1023, ( 65473 S_R - 59470 S_G -  6003 S_B + (512 << 26) + (1 << 25)) >> 26)
Payload: the layout of tests/yuv_reference.py (Y plane, then Cb, then Cr, little-endian uint16).
"""
import math

import numpy as np

KR, KG, KB = 0.2126, 0.7152, 0.0722
Y_COEFF = (13920, 46826, 4727)
CB_COEFF = (-15003, -50470, 65473)
CR_COEFF = (65473, -59470, -6003)
CHROMA_BIAS = (512 << 26) + (1 << 25)


def quantise16(v):
    """float32 array -> int64 array of q(v).  The only floating-point step of the contract; two float32 operations, each rounded."""
    v = np.asarray(v, np.float32)
    inside = (v > np.float32(0)) & (v < np.float32(1))  # (False for NaN)
    with np.errstate(all="ignore"):
        scaled = np.where(inside, v, np.float32(0)) * np.float32(65535.0)  # float32 * float32 -> float32
        assert scaled.dtype == np.float32
        biased = scaled + np.float32(0.5)
        assert biased.dtype == np.float32
        q = np.floor(biased).astype(np.int64)
        q = np.where(v >= np.float32(1), 65535, np.where(inside, q, 0))  # (v >= 1 is False for NaN: it stays 0)
    return q.astype(np.int64)


def nearest_root(m: int) -> int:
    """The e with e (e - 1) < m <= e (e + 1); 0 for m = 0.  Python integers only."""
    e = math.isqrt(m)  # e^2 <= m < (e + 1)^2
    return e + 1 if m > e * (e + 1) else e


def nearest_roots(m):
    """nearest_root over an int64 array (m < 2^32).  A float64 guess, then the definition in integers decides and is asserted."""
    m = np.asarray(m, np.int64)
    e = np.sqrt(m.astype(np.float64)).astype(np.int64)
    for _ in range(2):
        e = np.where(m > e * (e + 1), e + 1, e)
        e = np.where((e > 0) & (m <= e * (e - 1)), e - 1, e)
    assert ((e * (e - 1) < m) | ((e == 0) & (m == 0))).all() and (m <= e * (e + 1)).all()
    return e


def encode16_from_q(q_frames):
    """(n, ...) integer q values -> E, int64, same trailing shape."""
    q = np.asarray(q_frames).astype(np.uint64)
    n = q.shape[0]
    assert 1 <= n <= 256
    total = (q * q).sum(axis=0, dtype=np.uint64)  # <= 256 * 65535^2 < 2^40
    mean = total // np.uint64(n)
    return nearest_roots(mean.astype(np.int64))


def encode16(frames):
    """n sub-frames (H, W, >= 3) float32 -> A = (H, W, 3) int64, 16-bit gamma-encoded."""
    return encode16_from_q(np.stack([quantise16(np.asarray(f, np.float32)[..., :3]) for f in frames]))


def planes_from_e(e, clamp=True):
    """(H, W, 3) 16-bit values -> (Y (H, W), Cb (ch, cw), Cr (ch, cw)) int64.  clamp=False: the chroma before min(1023, .)."""
    a = np.asarray(e).astype(np.int64)
    h, w = a.shape[:2]
    y = (Y_COEFF[0] * a[..., 0] + Y_COEFF[1] * a[..., 1] + Y_COEFF[2] * a[..., 2] + (1 << 21)) >> 22
    assert int(a.max(initial=0)) <= 65535 and int(a.min(initial=0)) >= 0
    cw, ch = (w + 1) // 2, (h + 1) // 2
    rows = 2 * np.arange(ch)
    two_rows = a[rows] + a[np.minimum(rows + 1, h - 1)]
    cols = 2 * np.arange(cw)
    s = two_rows[:, np.maximum(cols - 1, 0)] + 2 * two_rows[:, cols] + two_rows[:, np.minimum(cols + 1, w - 1)]
    cb_acc = CB_COEFF[0] * s[..., 0] + CB_COEFF[1] * s[..., 1] + CB_COEFF[2] * s[..., 2] + CHROMA_BIAS
    cr_acc = CR_COEFF[0] * s[..., 0] + CR_COEFF[1] * s[..., 1] + CR_COEFF[2] * s[..., 2] + CHROMA_BIAS
    assert int(cb_acc.min(initial=1)) > 0 and int(cr_acc.min(initial=1)) > 0
    cb, cr = cb_acc >> 26, cr_acc >> 26
    if clamp:
        cb, cr = np.minimum(1023, cb), np.minimum(1023, cr)
    return y, cb, cr


def payload_from_e(e) -> bytes:
    return b"".join(np.ascontiguousarray(p).astype("<u2").tobytes() for p in planes_from_e(e))


def deep_reference(frames) -> bytes:
    """The payload of one Y4M frame (C420p10, full range) for the float sub-frames `frames`."""
    return payload_from_e(encode16(frames))


def real_valued(e16):
    """H.273 on flat colours, real-valued and unclamped: (K, 3) values 0 .. 65535 -> (Y, Cb, Cr) float64, 10-bit full range."""
    e = np.asarray(e16, np.float64) / 65535.0
    ey = KR * e[:, 0] + KG * e[:, 1] + KB * e[:, 2]
    epb = (e[:, 2] - ey) / (2.0 * (1.0 - KB))
    epr = (e[:, 0] - ey) / (2.0 * (1.0 - KR))
    return 1023.0 * ey, 1023.0 * epb + 512.0, 1023.0 * epr + 512.0
