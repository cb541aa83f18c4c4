"""`render --frames y4m --chroma 420|422|444`: the 4:2:2 and 4:4:4 kernels (portal_amd/csrc/kernels/yuv10.hip, yuv10_f32.hip), their C
ABI (ptl_average_to_yuv10, ptl_average_f32_to_yuv10, ptl_yuv10_frame_bytes, ptl_y4m_header_chroma), the Python mirror and the CLI option,
against tests/yuv_chroma_reference.py (a numpy restatement of the contract in DESIGN.md 2.3.3).  Every comparison of a payload is byte
equality."""
import os
import subprocess

import numpy as np
import pytest

from tests import yuv_chroma_reference as cr
from tests import yuv_deep_reference as dr
from tests import yuv_reference as yr
from tests.yuv_harness import (KNOB, ROOT, _assert_same_payload, _averaged, _c_getenv, _case, _check_stream, _compile_with_usage, _convert, _copying_stub, _entries,
                               _expected_stream, _frame_from_values, _render, _special_values, gpu)  # noqa: F401 (gpu: a fixture)

NEW = (422, 444)
KERNELS = [(False, 422), (False, 444), (True, 422), (True, 444)]  # (float sub-frames, sampling): the four new kernels
KERNEL_IDS = ["rgba8-422", "rgba8-444", "f32-422", "f32-444"]


def _corners(bits):
    top = (1 << bits) - 1
    return [(r, g, b) for r in (0, top) for g in (0, top) for b in (0, top)]


# ---------------------------------------------------------------------------------------------
# CPU: the reference's own properties
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("chroma", NEW)
def test_accumulators_stay_positive_and_the_corners_reach_both_ends(bits, chroma):
    """The eight cube corners as flat frames: the smallest accumulator is the one the contract names (yellow's Cb, cyan's Cr: asserted
    inside the helper as a lower bound, here as reached), the 8-bit maxima fit 32 bits, pure blue and pure red reach exactly 1024 before
    the min and nothing exceeds it, yellow and cyan reach 0, and a reference without the min differs exactly where the unclamped value is 1024."""
    top = (1 << bits) - 1
    blue, red, yellow, cyan = (0, 0, top), (top, 0, 0), (top, top, 0), (0, top, top)
    k, taps = cr.SHIFT[bits][chroma], cr.TAPS[chroma]
    assert 1 << (k - cr.SHIFT[bits][444]) == taps and cr.SHIFT[bits][420] - k == {422: 1, 444: 3}[chroma]
    for row, zero_at in zip(cr.ROWS[bits], (yellow, cyan)):
        assert sum(row) == 0  # a grey's chroma is the bias alone
        lowest = sum(c * taps * v for c, v in zip(row, zero_at)) + (512 << k) + (1 << (k - 1))
        assert lowest == cr.MINIMA[bits][chroma] and 0 < lowest < 1 << k
        highest = max(row) * taps * top + (512 << k) + (1 << (k - 1))
        assert highest >> k == 1024 and (bits == 16 or highest < 1 << 31) and (bits == 8 or highest >= 1 << 32)  # the float forms need 64 bits
    for rgb in _corners(bits):
        frame = np.tile(np.array(rgb, np.int64), (3, 6, 1))
        _, cb, crr = cr.planes(frame, chroma, bits)
        _, ucb, ucr = cr.planes(frame, chroma, bits, clamp=False)
        assert (ucb == 1024).all() == (rgb == blue) == (ucb == 1024).any() and (ucr == 1024).all() == (rgb == red) == (ucr == 1024).any(), rgb
        assert np.array_equal(cb, np.minimum(1023, ucb)) and np.array_equal(crr, np.minimum(1023, ucr))
        assert (cb == 0).all() == (rgb == yellow) and (crr == 0).all() == (rgb == cyan), rgb
        differs = cr.payload(frame, chroma, bits, clamp=False) != cr.payload(frame, chroma, bits)
        assert differs == (rgb in (blue, red)), rgb  # the guard: dropping the min changes the payload exactly there
        if rgb == (top, top, top):
            y, _, _ = cr.planes(frame, chroma, bits)
            assert (y == 1023).all() and (cb == 512).all() and (crr == 512).all()


@pytest.mark.parametrize("bits", [8, 16])
@pytest.mark.parametrize("chroma", NEW)
def test_every_grey_gives_512(bits, chroma):
    g = np.arange(1 << bits, dtype=np.int64)
    frame = np.repeat(np.repeat(g[:, None, None], 4, axis=1), 3, axis=2)  # row k is grey k, four pixels wide
    y, cb, crr = cr.planes(frame, chroma, bits)
    top = (1 << bits) - 1
    assert (cb == 512).all() and (crr == 512).all() and np.array_equal(y[:, 0], (2 * 1023 * g + top) // (2 * top))


@pytest.mark.parametrize("chroma", NEW)
def test_distance_to_the_real_valued_definition_8_bit(chroma):
    """All 2^24 colours as flat rows (two pixels wide: a 4:2:2 sample then sees one colour): within 0.51 codes of H.273 in real numbers."""
    worst = 0.0
    for start in range(0, 1 << 24, 1 << 21):
        packed = np.arange(start, start + (1 << 21), dtype=np.int64)
        colours = np.stack([packed & 255, (packed >> 8) & 255, packed >> 16], axis=1)
        y, cb, crr = cr.planes(np.repeat(colours[:, None, :], 2, axis=1), chroma, 8, clamp=False)
        ry, rcb, rcr = cr.real_valued(colours, 8)
        worst = max(worst, float(np.abs(y[:, 1] - ry).max()), float(np.abs(cb[:, 0] - rcb).max()), float(np.abs(crr[:, 0] - rcr).max()))
    print(chroma, worst)
    assert worst <= 0.51


@pytest.mark.parametrize("chroma", NEW)
def test_distance_to_the_real_valued_definition_16_bit(chroma):
    """4 M seeded 16-bit colours plus the cube corners, as flat rows: within 0.51 codes."""
    rng = np.random.default_rng(444)
    worst = 0.0
    for part in range(4):
        colours = np.concatenate([np.array(_corners(16)), rng.integers(0, 65536, (1 << 20, 3))]).astype(np.int64)
        y, cb, crr = cr.planes(np.repeat(colours[:, None, :], 2, axis=1), chroma, 16, clamp=False)
        ry, rcb, rcr = cr.real_valued(colours, 16)
        worst = max(worst, float(np.abs(y[:, 1] - ry).max()), float(np.abs(cb[:, 0] - rcb).max()), float(np.abs(crr[:, 0] - rcr).max()))
    print(chroma, worst)
    assert worst <= 0.51


def test_siting_of_a_422_sample():
    """Sample i sits ON luma column 2i with weights 1-2-1, columns clamped; rows are independent."""
    a = np.zeros((2, 5, 3), np.int64)
    a[0, :, 2] = [10, 20, 30, 40, 50]
    a[1, :, 2] = 255
    s = cr.weighted_sums(a, 422)
    assert s.shape == (2, 3, 3) and s[0, :, 2].tolist() == [10 + 2 * 10 + 20, 20 + 2 * 30 + 40, 40 + 2 * 50 + 50] and (s[1, :, 2] == 1020).all()
    assert cr.weighted_sums(a, 444) is a and cr.weighted_sums(a, 420).shape == (1, 3, 3)
    assert cr.weighted_sums(a, 420)[0, :, 2].tolist() == [50 + 1020, 120 + 1020, 190 + 1020]


@pytest.mark.parametrize("w,h", [(13, 11), (16, 4)])
def test_420_through_the_new_helper_is_the_shipped_reference(w, h):
    """With chroma = 420 the helper's payload equals yuv_reference.yuv_reference and yuv_deep_reference.deep_reference."""
    rng = np.random.default_rng(w)
    frame = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    assert cr.payload(frame, 420, 8) == yr.yuv_reference(frame)
    floats = [rng.random((h, w, 4), dtype=np.float32) for _ in range(3)]
    assert cr.payload(dr.encode16(floats), 420, 16) == dr.deep_reference(floats)
    assert cr.frame_bytes(w, h, 420) == yr.frame_bytes(w, h) and cr.y4m_header(w, h, 24, 420) == yr.y4m_header(w, h, 24)


# ---------------------------------------------------------------------------------------------
# CPU: header text, frame sizes, refusals, the build, the CLI's refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(64, 36), (3840, 2160), (1, 1), (1023, 3)])
def test_header_text_and_frame_bytes(pa, w, h):
    import ctypes as C

    for chroma in cr.SAMPLINGS:
        want = f"YUV4MPEG2 W{w} H{h} F24:1 Ip A1:1 C{chroma}p10 XYSCSS={chroma}P10 XCOLORRANGE=FULL\n".encode()
        assert pa.y4m_header(w, h, 24, chroma=chroma) == want == cr.y4m_header(w, h, 24, chroma)
        buf = C.create_string_buffer(len(want) + 1)  # the text and its NUL fit exactly
        assert pa.lib().ptl_y4m_header_chroma(w, h, 24, chroma, buf, len(buf)) == len(want) and buf.value == want
        assert pa.lib().ptl_y4m_header_chroma(w, h, 24, chroma, buf, len(want)) == -1
        cw, ch = {420: ((w + 1) // 2, (h + 1) // 2), 422: ((w + 1) // 2, h), 444: (w, h)}[chroma]
        assert pa.yuv10_frame_bytes(w, h, chroma) == 2 * (w * h + 2 * cw * ch) == cr.frame_bytes(w, h, chroma)
        if w % 2 == 0:
            assert pa.yuv10_frame_bytes(w, h, chroma) == {420: 3, 422: 4, 444: 6}[chroma] * w * h
    assert pa.y4m_header(w, h, 24) == yr.y4m_header(w, h, 24) and pa.yuv10_frame_bytes(w, h, 420) == pa.yuv420p10_frame_bytes(w, h)
    buf = C.create_string_buffer(128)
    for unknown in (0, 411, 421, -444):
        assert pa.yuv10_frame_bytes(w, h, unknown) == 0 and pa.lib().ptl_y4m_header_chroma(w, h, 24, unknown, buf, len(buf)) < 0
    assert pa.yuv10_frame_bytes(0, h, 444) == 0 and pa.yuv10_frame_bytes(w, -1, 422) == 0


@pytest.mark.parametrize("deep", [False, True])
def test_entry_points_refuse_before_any_gpu_call(pa, deep):
    """An unknown sampling (with a message that names the three), no frames, bad counts, null and unaligned pointers, sizes beyond the
    32-bit byte offsets -> PTL_ERR_INVALID; no device needed."""
    import ctypes as C

    f = pa.lib().ptl_average_f32_to_yuv10 if deep else pa.lib().ptl_average_to_yuv10
    ptrs = (C.c_void_p * 2)(4096, 8192)
    out = C.c_void_p(1 << 20)
    for unknown in (0, 411):
        assert f(0, ptrs, 2, out, 4, 4, unknown, None, None) == -1
        message = pa.lib().ptl_last_error().decode()
        assert all(v in message for v in ("420", "422", "444", str(unknown))), message
    for chroma in cr.SAMPLINGS:
        assert f(0, None, 2, out, 4, 4, chroma, None, None) == -1
        assert f(0, ptrs, 2, None, 4, 4, chroma, None, None) == -1
        assert f(0, (C.c_void_p * 2)(4096, None), 2, out, 4, 4, chroma, None, None) == -1
        assert f(0, ptrs, 0, out, 4, 4, chroma, None, None) == -1
        many = (C.c_void_p * 257)(*([4096] * 257))
        assert f(0, many, 257, out, 4, 4, chroma, None, None) == -1
        assert f(0, (C.c_void_p * 2)(4096, 8200), 2, out, 4, 4, chroma, None, None) == -1  # 8-byte aligned only
        assert f(0, ptrs, 2, C.c_void_p((1 << 20) + 8), 4, 4, chroma, None, None) == -1
        assert f(0, ptrs, 2, out, 0, 4, chroma, None, None) == -1
        assert f(0, ptrs, 2, out, 4, -2, chroma, None, None) == -1
        if deep:
            assert f(0, ptrs, 2, out, 1 << 14, (1 << 14) + 1, chroma, None, None) == -1  # beyond 2^28 pixels
        else:
            assert f(0, ptrs, 2, out, 1 << 15, (1 << 14) + 1, chroma, None, None) == -1  # beyond 2^29 pixels
    with pytest.raises(Exception):
        (pa.average_f32_to_yuv10_device if deep else pa.average_to_yuv10_device)([4096], 1 << 20, 4, 4, 411)
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    assert "#define PTL_CHROMA_420 420" in header and "#define PTL_CHROMA_422 422" in header and "#define PTL_CHROMA_444 444" in header


@pytest.mark.parametrize("source,prefix", [("yuv10", "ptl_average_to_yuv"), ("yuv10_f32", "ptl_average_f32_to_yuv")])
def test_make_kernels_builds_the_code_objects_without_scratch(pa, tmp_path, source, prefix):
    """`make kernels` leaves the code object; the file has exactly its six entries, the four of 4:2:2 and 4:4:4 among them, each with 0 bytes
    of scratch, no LDS and at most 128 VGPRs (the compiler's own notes, printed); the shared device functions live in yuv_common.h."""
    import re

    subprocess.run(["make", "kernels"], cwd=ROOT, check=True, capture_output=True)
    assert os.path.getsize(os.path.join(ROOT, "portal_amd", "kernels", source + ".hsaco")) > 1000
    usage = _compile_with_usage(source, tmp_path)
    assert set(usage) == _entries(prefix) > {f"{prefix}{c}p10{t}_kernel" for c in NEW for t in ("", "_table")}
    for entry, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0, (entry, u)
        assert u["VGPRs"] <= 128, (entry, u)  # four waves per SIMD
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert f"portal_amd/kernels/{source}.hsaco" in re.search(r"^KERNELS\s*:=(.*)$", makefile, re.M).group(1)
    for kernel in ("yuv10.hip", "yuv10_f32.hip"):
        text = open(os.path.join(ROOT, "portal_amd", "csrc", "kernels", kernel)).read()
        assert '#include "average_common.h"' in text and '#include "yuv_common.h"' in text


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--chroma", "444"], "--chroma needs --frames y4m"),
                                              ("render", ["--chroma", "422", "--frames", "png"], "--chroma needs --frames y4m"),
                                              ("render", ["--frames", "y4m", "--chroma", "411"], "--chroma 420|422|444"),
                                              ("render", ["--frames", "y4m", "--chroma", "4:4:4"], "--chroma 420|422|444"),
                                              ("render", ["--frames", "y4m", "--chroma", "0444"], "--chroma 420|422|444"),
                                              ("render-frame", ["--frames", "y4m", "--chroma", "444"], "--chroma is an option of render"),
                                              ("precompile", ["--chroma", "420", "--frames", "y4m"], "--chroma is an option of render"),
                                              ("render", ["--frames", "bogus", "--chroma", "444"], "--frames png|y4m")])
def test_cli_refuses_chroma_where_it_means_nothing(pa, tmp_path, cmd, extra, reason):
    """Refused while the arguments are parsed: exit status 2, one line that says why, nothing rendered (this machine has no GPU to ask)."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    clip = pa.Scene.from_file(pa.scene_path("basics")).animations()[0][0]
    args = [exe, cmd, pa.scene_path("basics")] + ([clip, "--out-dir", str(tmp_path)] if cmd == "render" else []) + extra
    out = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _is_fast(deep, w):
    """The decision of the kernels and of the host: 8x1 pixels per lane (RGBA8) or 4x1 (float) where the width allows it."""
    return w % (4 if deep else 8) == 0


def _bits(deep):
    return 16 if deep else 8


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 64, 65, 256])
@pytest.mark.parametrize("deep,chroma", KERNELS, ids=KERNEL_IDS)
def test_kernel_matches_reference_for_every_subframe_count(gpu, deep, chroma, n):
    """13x11: the general path.  32x34: the fast path, 136 blocks (RGBA8) and 272 (float): waves span several rows and the last wave is
    partial.  n = 1 is a plain conversion; beyond 64 sub-frames the pointer-table entry."""
    assert not _is_fast(deep, 13) and _is_fast(deep, 32) and (32 // (4 if deep else 8)) * 34 == (272 if deep else 136)
    for w, h in ((13, 11), (32, 34)):
        frames, a = _case(deep, 100 * n + w, n, w, h)
        _assert_same_payload(_convert(gpu, deep, chroma, frames, w, h), cr.payload(a, chroma, _bits(deep)), w, h, f"{w}x{h} n={n}", chroma)


SIZES = [(1, 1), (2, 1), (1, 2), (5, 3), (13, 11), (8, 1), (24, 3), (128, 5), (1032, 3), (244, 135)]


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("deep,chroma", KERNELS, ids=KERNEL_IDS)
def test_kernel_matches_reference_at_any_frame_size(gpu, deep, chroma, w, h):
    """Three sub-frames.  24x3 takes the fast path though W % 16 != 0 and H is odd; 1032x3 has 129 (258) blocks per row, so wave starts fall
    mid-row and row starts mid-wave: the 4:2:2 left-column rule.  On the general path the frame lies 16 bytes into its buffer (the entry
    point wants 16-byte alignment), and where W*H is odd -- 1x1, 5x3, 13x11 -- the chroma planes start on odd multiples of 2 bytes."""
    assert _is_fast(False, w) == ((w, h) in ((8, 1), (24, 3), (128, 5), (1032, 3))) and _is_fast(True, w) == (w % 4 == 0)
    frames, a = _case(deep, 1000 * w + h, 3, w, h)
    offset = 0 if _is_fast(deep, w) else 16
    if (w, h) in ((1, 1), (5, 3), (13, 11)):
        assert offset == 16 and (offset + 2 * w * h) % 4 == 2
    _assert_same_payload(_convert(gpu, deep, chroma, frames, w, h, offset=offset), cr.payload(a, chroma, _bits(deep)), w, h, f"{w}x{h}", chroma)


def _saturation_frames(deep, w, h, bands):
    """[(label, frame)]: the eight corner bands (16 columns each) or the eight flat corner frames."""
    top = 1.0 if deep else 255
    corners = [(r, g, b) for r in (0, top) for g in (0, top) for b in (0, top)]
    dtype = np.float32 if deep else np.uint8
    if bands:
        frame = np.empty((h, w, 4), dtype)
        for k, rgb in enumerate(corners):
            frame[:, 16 * k: 16 * (k + 1)] = rgb + (top,)
        return [("bands", frame)]
    return [(str(rgb), np.tile(np.array(rgb + (top,), dtype), (h, w, 1))) for rgb in corners]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["bands-128x4", "flat-16x2", "flat-5x3"])
@pytest.mark.parametrize("deep,chroma", KERNELS, ids=KERNEL_IDS)
def test_saturated_colours(gpu, deep, chroma, shape):
    """The min(1023, .) and the zero end on both paths: the eight corner bands at 128x4 and flat corner frames at 16x2 (fast path) and 5x3
    (general), as one sub-frame and as two and three identical ones.  Cb / Cr hold 1023 where the reference before its min holds 1024,
    and 0 is reached."""
    w, h = (int(v) for v in shape.split("-")[1].split("x"))
    assert _is_fast(deep, w) == (shape != "flat-5x3")
    reached = {"cb_clamp": 0, "cr_clamp": 0, "cb_zero": 0, "cr_zero": 0}
    for label, frame in _saturation_frames(deep, w, h, shape.startswith("bands")):
        for n in (1, 2, 3):
            a = _averaged(deep, [frame] * n)
            assert np.array_equal(np.asarray(a)[..., :3], (np.asarray(frame)[..., :3] * (65535 if deep else 1)).astype(np.int64))  # identical sub-frames: exact
            got = _convert(gpu, deep, chroma, [frame] * n, w, h)
            _assert_same_payload(got, cr.payload(a, chroma, _bits(deep)), w, h, f"{shape} {label} n={n}", chroma)
            _, cb, crr = cr.split_planes(got, w, h, chroma)
            _, ucb, ucr = cr.planes(a, chroma, _bits(deep), clamp=False)
            assert ucb.max() <= 1024 and ucr.max() <= 1024 and cb.max() <= 1023 and crr.max() <= 1023
            assert (cb[ucb == 1024] == 1023).all() and (crr[ucr == 1024] == 1023).all()
            assert np.array_equal(cb == 1023, ucb >= 1023) and np.array_equal(crr == 1023, ucr >= 1023)
            reached["cb_clamp"] += int((ucb == 1024).sum())
            reached["cr_clamp"] += int((ucr == 1024).sum())
            reached["cb_zero"] += int((cb == 0).sum())
            reached["cr_zero"] += int((crr == 0).sum())
    assert all(reached.values()), (shape, reached)  # not vacuous


@pytest.mark.gpu
def test_every_8_bit_colour_once_at_444(gpu):
    """4096x4096 holding all 2^24 RGB triples (alpha 0: ignored), n = 1, at 4:4:4: all three planes equal the reference."""
    w = h = 4096
    frame = np.arange(1 << 24, dtype="<u4").view(np.uint8).reshape(h, w, 4)
    assert frame[0, 1].tolist() == [1, 0, 0, 0] and frame[-1, -1].tolist() == [255, 255, 255, 0]
    got = _convert(gpu, False, 444, [frame], w, h)
    _assert_same_payload(got, cr.payload(frame, 444, 8), w, h, "every colour", 444)
    y, cb, crr = cr.split_planes(got, w, h, 444)
    assert y.min() == 0 and y.max() == 1023 and cb.min() == 0 and cb.max() == 1023 and crr.min() == 0 and crr.max() == 1023


@pytest.mark.gpu
@pytest.mark.parametrize("chroma", NEW)
def test_every_16_bit_value_once(gpu, chroma):
    """256x256, n = 1: pixel p holds p / 65535, (65535 - p) / 65535 and (7 p mod 65536) / 65535 -- every q in every channel; and the same
    frame one column narrower, on the general path."""
    w = h = 256
    p = np.arange(65536, dtype=np.int64)
    q = np.stack([p, 65535 - p, (7 * p) % 65536], axis=1).reshape(h, w, 3)
    frame = np.zeros((h, w, 4), np.float32)
    frame[..., :3] = (q / 65535.0).astype(np.float32)
    assert np.array_equal(dr.encode16([frame]), q)
    for c in range(3):
        assert np.array_equal(np.sort(q[..., c].ravel()), p)
    _assert_same_payload(_convert(gpu, True, chroma, [frame], w, h), cr.payload(q, chroma, 16), w, h, "every q", chroma)
    narrow = np.ascontiguousarray(frame[:, : w - 1])
    _assert_same_payload(_convert(gpu, True, chroma, [narrow], w - 1, h), cr.payload(q[:, : w - 1], chroma, 16), w - 1, h, "every q, general path", chroma)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(32, 12), (33, 11)])
@pytest.mark.parametrize("chroma", NEW)
def test_special_float_inputs_as_bit_patterns(gpu, chroma, w, h):
    """As one sub-frame, as two (the values reversed in the second) and as three; 32x12 the fast path, 33x11 the general one."""
    values = _special_values()
    assert values.size <= 3 * w * h and _is_fast(True, w) == (w == 32)
    frame, reversed_frame = _frame_from_values(values, w, h), _frame_from_values(values[::-1], w, h)
    for frames in ([frame], [frame, reversed_frame], [frame, frame, reversed_frame]):
        _assert_same_payload(_convert(gpu, True, chroma, frames, w, h), cr.payload(dr.encode16(frames), chroma, 16), w, h, f"special n={len(frames)}", chroma)


def _lanes(deep, chroma, w, h):
    """The lanes the host asks for."""
    block = 4 if deep else 8
    return (w // block) * h if w % block == 0 else (w * h if chroma == 444 else ((w + 1) // 2) * h)


KNOB_SHAPES = {"256x134": (256, 134), "244x135": (244, 135), "243x135": (243, 135)}  # the last: the general path of the float kernels too


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("kind", list(KNOB_SHAPES))
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, kind, cap, n):
    """The grid-stride loops going round more than twice with 1 and 3 workgroups (PTL_AVERAGE_IMAGES_GRID_CAP, which launch_over_subframes
    reads at each call), for the four kernels, both entries (n = 65: the pointer table) and both paths.  256x134 RGBA8 is 4 288 blocks:
    with 3 workgroups the last trip ends after 448 lanes, and the float form's 8 576 blocks end after 128; 244x135 float is 8 235 blocks,
    whose last trip ends in the middle of a wave (43 lanes), and the cross-lane move of 4:2:2 still finds its lower neighbour.  Equal to
    the reference and to the same call with the shipped grid."""
    w, h = KNOB_SHAPES[kind]
    assert _lanes(True, 422, 244, 135) == 8235 and 8235 % 768 == 555 and 555 % 64 == 43 and _lanes(False, 422, 256, 134) == 4288
    for deep, chroma in KERNELS:
        lanes = _lanes(deep, chroma, w, h)
        assert 2 * cap * 256 < lanes <= 4096 * 256  # at least three trips, all of them the knob's
        frames, a = _case(deep, 7000 + n, n, w, h)
        want = cr.payload(a, chroma, _bits(deep))
        monkeypatch.delenv(KNOB, raising=False)
        assert _c_getenv(KNOB) is None
        shipped = _convert(gpu, deep, chroma, frames, w, h)
        monkeypatch.setenv(KNOB, str(cap))
        assert _c_getenv(KNOB) == str(cap).encode()
        got = _convert(gpu, deep, chroma, frames, w, h)
        _assert_same_payload(got, want, w, h, f"{kind} deep={deep} cap={cap} n={n}", chroma)
        assert got == shipped


@pytest.mark.gpu
@pytest.mark.parametrize("deep", [False, True], ids=["rgba8", "f32"])
@pytest.mark.parametrize("w,h", [(13, 11), (32, 34), (244, 135)])
def test_samplings_agree_with_the_shipped_entries(gpu, deep, w, h):
    """The Y plane at 4:2:2 and 4:4:4 is the Y plane of the shipped 4:2:0 entry for the same input, and chroma = 420 through the new entry
    is the old entry: same bytes."""
    import torch

    pa = gpu
    frames, a = _case(deep, 31 * w + h, 3, w, h)
    dev = [torch.from_numpy(f).cuda() for f in frames]
    out = torch.zeros(pa.yuv420p10_frame_bytes(w, h), dtype=torch.uint8, device="cuda")
    old = pa.average_f32_to_yuv420p10_device if deep else pa.average_to_yuv420p10_device
    old([d.data_ptr() for d in dev], out.data_ptr(), w, h, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    shipped = out.cpu().numpy().tobytes()
    assert shipped == (dr.deep_reference(frames) if deep else yr.yuv_reference(a))
    assert _convert(pa, deep, 420, dev, w, h) == shipped == cr.payload(a, 420, _bits(deep))
    for chroma in NEW:
        assert _convert(pa, deep, chroma, dev, w, h)[: 2 * w * h] == shipped[: 2 * w * h], chroma


@pytest.mark.gpu
@pytest.mark.parametrize("deep,chroma", KERNELS, ids=KERNEL_IDS)
def test_elapsed_ms_and_a_stream_of_the_callers(gpu, deep, chroma):
    """Launched on the stream it is given (a non-default torch stream, the inputs produced on it); with elapsed_ms the launch is bracketed by
    events and waited for."""
    import torch

    pa = gpu
    w, h = 320, 90
    call = pa.average_f32_to_yuv10_device if deep else pa.average_to_yuv10_device
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.Generator(device="cuda").manual_seed(11)
        if deep:
            frames = [torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=g) for _ in range(4)]
        else:
            frames = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
        out = torch.zeros(pa.yuv10_frame_bytes(w, h, chroma), dtype=torch.uint8, device="cuda")
        ms = call([f.data_ptr() for f in frames], out.data_ptr(), w, h, chroma, stream=side.cuda_stream, timed=True)
        assert ms is not None and 0.0 < ms < 1000.0
        got = out.cpu().numpy().tobytes()  # the timed call has waited; the copy is ordered behind it on the same stream anyway
        out.zero_()
        assert call([f.data_ptr() for f in frames], out.data_ptr(), w, h, chroma, stream=side.cuda_stream) is None
        side.synchronize()
        assert out.cpu().numpy().tobytes() == got
    a = _averaged(deep, [f.cpu().numpy() for f in frames])
    _assert_same_payload(got, cr.payload(a, chroma, _bits(deep)), w, h, "side stream", chroma)


# ---- the CLI ---------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("deep", [False, True], ids=["plain", "deep-colour"])
@pytest.mark.parametrize("chroma", [444, 422])
@pytest.mark.parametrize("blur", [3, 1])
def test_render_cli_streams_the_sampling_it_is_asked_for(gpu, tmp_path, blur, chroma, deep):
    """`portal-amd render --frames y4m --chroma C [--deep-colour]` end to end.  Without an ffmpeg on the PATH the stream is <clip>.y4m: the
    header that names the sampling plus, per frame, FRAME and the numpy reference of the sub-frames the library draws.  With one -- a stub
    that records its arguments and copies stdin to its last argument -- the encoder is told the stream's pixel format and is piped the
    same bytes."""
    pa = gpu
    want, frames, clip = _expected_stream(pa, blur, chroma, lambda subs8, subs32: cr.payload(_averaged(deep, subs32 if deep else subs8), chroma, _bits(deep)))
    options = ["--motion-blur-frames", str(blur), "--aa-count", "2", "--render-depth", "12", "--chroma", str(chroma)] + (["--deep-colour"] if deep else [])
    out = _render(pa, tmp_path / "file", clip, options)
    video = tmp_path / "file" / "video" / "basics"
    in_file = (video / f"{clip}.y4m").read_bytes()
    _check_stream(in_file, want, len(frames), chroma)
    assert f"-pix_fmt yuv{chroma}p10le" in out.stdout and "yuv420p10le" not in out.stdout  # the message names the command that would encode the file
    assert not (video / f"{clip}.mov").exists()

    args_file = tmp_path / "stub_args.txt"
    out = _render(pa, tmp_path / "pipe", clip, options, path=_copying_stub(tmp_path / "bin", args_file))
    video = tmp_path / "pipe" / "video" / "basics"
    assert (video / f"{clip}.mov").read_bytes() == in_file  # the piped bytes are the file's
    args = args_file.read_text().splitlines()
    assert args[:4] == ["-f", "yuv4mpegpipe", "-i", "-"] and args[-1] == str(video / f"{clip}.mov")
    assert args[args.index("-pix_fmt") + 1] == f"yuv{chroma}p10le" and args.count("-pix_fmt") == 1
    assert "ffmpeg status: 0" in out.stdout and not (video / f"{clip}.y4m").exists()
