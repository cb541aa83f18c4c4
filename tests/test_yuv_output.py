"""`render --frames y4m`: the fused average-and-convert kernel (portal_amd/csrc/kernels/yuv10.hip), its C ABI and the Y4M stream
of the CLI, against tests/yuv_reference.py (a numpy restatement of the contract in DESIGN.md 2.3).  Every comparison is byte equality."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import yuv_reference as yr
from tests.yuv_harness import (FPS, H, KNOB, ROOT, W, _assert_same_payload, _averaged, _c_getenv, _case_payload, _check_stream, _compile_with_usage, _convert, _copying_stub,
                               _entries, _expected_stream, _path_without_ffmpeg, _render, _shipped_grid_cap, _write_stub, gpu)  # noqa: F401 (gpu: a fixture)

SIZES = [(1, 1), (2, 2), (3, 1), (5, 7), (13, 11), (16, 2), (64, 36), (1023, 3), (1920, 1080), (3840, 2160)]


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,fps", [(64, 36, 2), (3840, 2160, 60), (7680, 2160, 600), (1, 1, 1), (1023, 3, 24)])
def test_y4m_header_text(pa, w, h, fps):
    import ctypes as C

    want = f"YUV4MPEG2 W{w} H{h} F{fps}:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n".encode()
    assert pa.y4m_header(w, h, fps) == want == yr.y4m_header(w, h, fps)
    buf = C.create_string_buffer(len(want) + 1)  # the text and its NUL fit exactly
    assert pa.lib().ptl_y4m_header(w, h, fps, buf, len(buf)) == len(want) and buf.value == want
    for cap in (0, 1, 16, len(want)):
        short = C.create_string_buffer(max(cap, 1))
        assert pa.lib().ptl_y4m_header(w, h, fps, short, cap) == -1  # PTL_ERR_INVALID
    assert pa.lib().ptl_y4m_header(w, h, 0, buf, len(buf)) == -1 and pa.lib().ptl_y4m_header(0, h, fps, buf, len(buf)) == -1


def test_frame_bytes_is_the_formula(pa):
    for w, h in SIZES + [(7680, 4320), (7, 7), (1, 2), (2, 1)]:
        cw, ch = (w + 1) // 2, (h + 1) // 2
        assert pa.yuv420p10_frame_bytes(w, h) == 2 * (w * h + 2 * cw * ch) == yr.frame_bytes(w, h), (w, h)
        if w * h < 1 << 16:
            assert len(yr.yuv_reference(np.zeros((h, w, 4), np.uint8))) == yr.frame_bytes(w, h)
    assert pa.yuv420p10_frame_bytes(3840, 2160) == 3 * 3840 * 2160  # 3 bytes per pixel where both sizes are even
    assert pa.yuv420p10_frame_bytes(0, 4) == 0 and pa.yuv420p10_frame_bytes(4, -1) == 0


def test_entry_points_refuse_what_average_images_refuses(pa):
    """Validation comes before any GPU call: no frames, bad counts, bad sizes, unaligned pointers -> PTL_ERR_INVALID."""
    import ctypes as C

    L = pa.lib()
    ptrs = (C.c_void_p * 2)(4096, 8192)
    out = C.c_void_p(1 << 20)
    assert L.ptl_average_to_yuv420p10(0, None, 2, out, 4, 4, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, ptrs, 2, None, 4, 4, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, ptrs, 0, out, 4, 4, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, ptrs, 2, out, 0, 4, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, ptrs, 2, out, 4, -2, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, ptrs, 2, C.c_void_p((1 << 20) + 8), 4, 4, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, (C.c_void_p * 2)(4096, 8196), 2, out, 4, 4, None, None) == -1
    many = (C.c_void_p * 257)(*([4096] * 257))
    assert L.ptl_average_to_yuv420p10(0, many, 257, out, 4, 4, None, None) == -1
    assert L.ptl_average_to_yuv420p10(0, ptrs, 2, out, 1 << 15, (1 << 14) + 1, None, None) == -1  # beyond 2^29 pixels


def test_make_kernels_builds_the_code_object_without_scratch(pa, tmp_path):
    """`make kernels` leaves portal_amd/kernels/yuv10.hsaco; its six entries compile for gfx950 with 0 bytes of scratch and no LDS,
    and average_images.hip still gets its device functions from the header the two kernels share."""
    subprocess.run(["make", "kernels"], cwd=ROOT, check=True, capture_output=True)
    assert os.path.getsize(os.path.join(ROOT, "portal_amd", "kernels", "yuv10.hsaco")) > 1000
    usage = _compile_with_usage("yuv10", tmp_path)
    assert set(usage) == _entries("ptl_average_to_yuv") >= {"ptl_average_to_yuv420p10_kernel", "ptl_average_to_yuv420p10_table_kernel"}
    for entry, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0, (entry, u)
        assert u["VGPRs"] <= 128, (entry, u)  # four waves per SIMD
    for kernel in ("average_images.hip", "yuv10.hip"):
        assert '#include "average_common.h"' in open(os.path.join(ROOT, "portal_amd", "csrc", "kernels", kernel)).read()


@pytest.mark.parametrize("extra,reason", [(["--frames", "y4m", "--shard", "0/2"], "a stream needs every frame, in order"),
                                          (["--shard", "1/3", "--frames", "y4m"], "a stream needs every frame, in order"),
                                          (["--frames", "bogus"], "--frames png|y4m"),
                                          (["--concurrent-draws", "2"], "unknown option")])  # (removed: a choice between two paths of which one was never better)
def test_render_refuses_what_a_stream_cannot_do(pa, tmp_path, extra, reason):
    """Refused while the arguments are parsed: exit status 2, one line of reason, nothing rendered (this machine has no GPU to ask)."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    clip = pa.Scene.from_file(pa.scene_path("basics")).animations()[0][0]
    out = subprocess.run([exe, "render", pa.scene_path("basics"), clip, "--out-dir", str(tmp_path)] + extra, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


def test_reference_helper_against_the_real_valued_definition():
    """Pins the fixture, not the product: on flat colours (all 256 greys, the eight cube corners, 10^5 seeded colours) the integer
    contract stays within 0.51 codes of H.273 in real numbers (measured: 0.502), greys are exact and have neutral chroma."""
    rng = np.random.default_rng(709)
    greys = np.repeat(np.arange(256)[:, None], 3, axis=1)
    corners = np.array([[r, g, b] for r in (0, 255) for g in (0, 255) for b in (0, 255)])
    colours = np.concatenate([greys, corners, rng.integers(0, 256, (100000, 3))]).astype(np.uint8)
    # colour k fills rows 2k, 2k+1 of a two-pixel-wide frame: each chroma sample then sees one flat colour (its columns clamp to the frame)
    frame = np.repeat(np.repeat(colours[:, None, :], 2, axis=0), 2, axis=1)
    y, cb, cr = yr.yuv_planes(frame)
    assert y.min() >= 0 and y.max() <= 1023 and cb.min() >= 0 and cb.max() <= 1023 and cr.min() >= 0 and cr.max() <= 1023
    ry, rcb, rcr = yr.real_valued(colours)
    worst = {}
    for name, got, real in (("Y", y[::2, 0], ry), ("Y'", y[1::2, 1], ry), ("Cb", cb[:, 0], rcb), ("Cr", cr[:, 0], rcr)):
        worst[name] = float(np.abs(got - real).max())
    print(worst)
    assert max(worst.values()) <= 0.51, worst
    assert np.array_equal(y[0:512:2, 0], np.round(1023 * np.arange(256) / 255).astype(np.int32))
    assert (cb[:256] == 512).all() and (cr[:256] == 512).all()
    # siting: a frame that is black left of column 2 and white from it: sample 1 sits ON column 2 (weights 1-2-1 over columns 1, 2, 3)
    step = np.zeros((2, 6, 3), np.uint8)
    step[:, 2:, 2] = 255  # blue only, so Cb moves
    _, cb, _ = yr.yuv_planes(step)
    s = np.array([0, 3 * 2 * 255, 4 * 2 * 255])  # S_B of the three samples: columns (0,0,1), (1,2,3), (3,4,5)
    assert np.array_equal(cb[0], np.minimum(1023, (131458 * s + (512 << 19) + (1 << 18)) >> 19))


CORNERS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]  # the eight corners of the RGB cube
BLUE, RED, YELLOW, CYAN = (0, 0, 255), (255, 0, 0), (255, 255, 0), (0, 255, 255)
SATURATION_SHAPES = {"bands-128x4": (128, 4), "flat-16x2": (16, 2), "flat-5x3": (5, 3), "flat-1x1": (1, 1)}  # the first two take the block path


def _flat_frame(w, h, rgb, alpha=255):
    return np.tile(np.array(tuple(rgb) + (alpha,), np.uint8), (h, w, 1))


def _corner_bands(w=128, h=4):
    """Eight flat bands of 16 columns, one cube corner each: chroma sample i of band k sees one colour for 8k < i < 8k + 8."""
    frame = np.empty((h, w, 4), np.uint8)
    for k, rgb in enumerate(CORNERS):
        frame[:, 16 * k: 16 * (k + 1)] = rgb + (255,)
    return frame


def _saturation_inputs(shape):
    """[(label, sub-frames)] of one shape: every saturated frame as n = 1 and as 2 and 3 identical sub-frames (the mean of n equal squares
    is that square: the averaged frame is the frame), and white + black, which averages to code 180."""
    w, h = SATURATION_SHAPES[shape]
    singles = [("bands", _corner_bands(w, h))] if shape.startswith("bands") else [(str(rgb), _flat_frame(w, h, rgb)) for rgb in CORNERS]
    inputs = [(f"{label} n={n}", [frame] * n) for label, frame in singles for n in (1, 2, 3)]
    return inputs + [("white+black", [_flat_frame(w, h, (255, 255, 255)), _flat_frame(w, h, (0, 0, 0))])]


def test_saturated_colours_reach_both_ends_of_the_chroma_range():
    """The clamp of the contract is needed and the inputs of test_saturated_colours_on_the_gpu reach it: six taps of pure blue give an
    unclamped Cb of 1024, pure red a Cr of 1024; the clamped planes hold 1023; yellow gives Cb 0 and cyan Cr 0 (accumulator 523 280, just
    above the shift).  A reference without the clamp differs from the reference on these inputs, so a kernel without it would too."""
    for rgb in CORNERS:
        frame = _flat_frame(2, 2, rgb)
        _, cb, cr = yr.yuv_planes(frame)
        _, ucb, ucr = yr.yuv_planes(frame, clamp=False)
        assert cb.shape == (1, 1) and 0 <= cb[0, 0] <= 1023 and 0 <= cr[0, 0] <= 1023
        assert (ucb[0, 0] == 1024) == (rgb == BLUE) and (ucr[0, 0] == 1024) == (rgb == RED), rgb
        assert ucb[0, 0] <= 1024 and ucr[0, 0] <= 1024 and ucb[0, 0] >= 0 and ucr[0, 0] >= 0
        assert cb[0, 0] == min(1023, ucb[0, 0]) and cr[0, 0] == min(1023, ucr[0, 0])
        assert (cb[0, 0] == 0) == (rgb == YELLOW) and (cr[0, 0] == 0) == (rgb == CYAN), rgb
        if rgb == YELLOW:  # S_R = S_G = 2040, S_B = 0: what is left of the bias
            assert (512 << 19) + (1 << 18) - (30123 + 101335) * 2040 == 523280 and 523280 >> 19 == 0
        if rgb in (BLUE, RED):
            assert (cb if rgb == BLUE else cr)[0, 0] == 1023
    for shape, (w, h) in SATURATION_SHAPES.items():
        reached = {"cb_clamp": 0, "cr_clamp": 0, "cb_zero": 0, "cr_zero": 0}
        for label, frames in _saturation_inputs(shape):
            a = _averaged(False, frames)
            if len(frames) > 1 and label != "white+black":
                assert np.array_equal(a[..., :3], frames[0][..., :3]), (shape, label)  # identical sub-frames: exact
            if label == "white+black":
                assert (a[..., :3] == 180).all()
            _, cb, cr = yr.yuv_planes(a)
            _, ucb, ucr = yr.yuv_planes(a, clamp=False)
            clamped = (ucb == 1024).any() or (ucr == 1024).any()
            assert clamped == (label != "white+black" and (shape.startswith("bands") or label.startswith((str(BLUE), str(RED))))), (shape, label)
            without = b"".join(p.astype("<u2").tobytes() for p in yr.yuv_planes(a, clamp=False))
            assert (without != yr.yuv_reference(a)) == clamped, (shape, label)  # the guard: dropping the clamp changes the payload
            reached["cb_clamp"] += int((ucb == 1024).sum())
            reached["cr_clamp"] += int((ucr == 1024).sum())
            reached["cb_zero"] += int((cb == 0).sum())
            reached["cr_zero"] += int((cr == 0).sum())
        assert all(reached.values()), (shape, reached)
    # the bands: the seven interior samples of a band (and sample 0 of the first, whose left tap clamps to the frame) see one colour
    _, ucb, ucr = yr.yuv_planes(_corner_bands(), clamp=False)
    k_blue, k_red = CORNERS.index(BLUE), CORNERS.index(RED)
    assert (ucb[:, 8 * k_blue + 1: 8 * k_blue + 8] == 1024).all() and (ucr[:, 8 * k_red + 1: 8 * k_red + 8] == 1024).all()
    assert int((ucb == 1024).sum()) == 2 * 7 and int((ucr == 1024).sum()) == 2 * 7


def _yuv_lanes(w, h):
    """The lanes ptl_average_to_yuv420p10 asks for: 8x2 blocks on the block path, chroma samples on the general path."""
    return (w // 8) * (h // 2) if w % 16 == 0 and h % 2 == 0 else ((w + 1) // 2) * ((h + 1) // 2)


CAP_CROSSING = {"general-2050x2049": (2050, 2049), "block-4096x4112": (4096, 4112)}
KNOB_SHAPES = {"block-256x134": (256, 134), "general-244x135": (244, 135)}


def test_stride_shapes_cross_the_grid_cap():
    """The shapes of the GPU stride tests against the cap in the host code: two that cross the shipped one by less than a grid, and trips
    of the knob's caps that end inside a wave on the block path."""
    cap = _shipped_grid_cap()
    assert cap == 4096
    for name, (w, h) in CAP_CROSSING.items():
        assert (name.startswith("block")) == (w % 16 == 0 and h % 2 == 0)
        assert cap * 256 < _yuv_lanes(w, h) < 2 * cap * 256, name  # a second trip that ends inside the grid
    assert _yuv_lanes(2050, 2049) == 1050625 and _yuv_lanes(4096, 4112) == 1052672
    assert _yuv_lanes(4096, 4096) == cap * 256  # (test_every_colour_once fills the grid exactly: one trip)
    assert _yuv_lanes(256, 134) == 2144 and _yuv_lanes(244, 135) == 8296
    for knob in (1, 3):
        for w, h in KNOB_SHAPES.values():
            assert _yuv_lanes(w, h) > 2 * knob * 256  # at least three trips
    assert 2144 % (3 * 256) == 608 and 608 % 64 == 32 and 2144 % 256 == 96 and 96 % 64 == 32  # the last trip ends in the middle of a wave


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 64, 65, 256])
def test_kernel_matches_reference_for_every_subframe_count(gpu, n):
    """244x135 (general path): the frame == yuv_reference(average_images(sub-frames)); n = 1 converts the input's own RGB; beyond 64
    sub-frames the pointer-table entry."""
    from oracle import postprocess as pp

    w, h = 244, 135
    rng = np.random.default_rng(1000 + n)
    frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
    frames[0][:4] = 255
    frames[-1][-4:] = 0
    want = yr.yuv_reference(pp.average_images(frames) if n > 1 else frames[0])
    _assert_same_payload(_convert(gpu, False, None, frames, w, h), want, w, h, f"n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 64, 65, 256])
def test_block_path_matches_reference_for_every_subframe_count(gpu, n):
    """The same at 256x134 (W % 16 == 0, H even: a lane owns an 8x2 block; 32 blocks per row, so waves span two row pairs)."""
    from oracle import postprocess as pp

    w, h = 256, 134
    rng = np.random.default_rng(2000 + n)
    frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
    want = yr.yuv_reference(pp.average_images(frames) if n > 1 else frames[0])
    _assert_same_payload(_convert(gpu, False, None, frames, w, h), want, w, h, f"n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES)
def test_kernel_matches_reference_at_any_frame_size(gpu, w, h):
    """Odd sizes, one-pixel frames, video sizes, three sub-frames: byte-exact, and nothing written behind frame_bytes."""
    from oracle import postprocess as pp

    rng = np.random.default_rng(w * 100 + h)
    frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(3)]
    _assert_same_payload(_convert(gpu, False, None, frames, w, h), yr.yuv_reference(pp.average_images(frames)), w, h, f"{w}x{h}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(13, 11), (5, 7), (1, 1)])
def test_chroma_planes_need_no_alignment(gpu, w, h):
    """The frame starts 16-byte aligned (as the entry point demands) but W*H is odd: Cb starts at byte 2*W*H, 2-byte aligned only."""
    from oracle import postprocess as pp

    assert (w * h) % 2 == 1
    rng = np.random.default_rng(77 + w)
    frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(3)]
    _assert_same_payload(_convert(gpu, False, None, frames, w, h, offset=16), yr.yuv_reference(pp.average_images(frames)), w, h, f"{w}x{h} at +16")


@pytest.mark.gpu
def test_every_colour_once(gpu):
    """4096x4096 holding all 2^24 RGB triples (alpha 0: ignored), n = 1: all three planes equal the reference."""
    w = h = 4096
    frame = np.arange(1 << 24, dtype="<u4").view(np.uint8).reshape(h, w, 4)
    assert frame[0, 1].tolist() == [1, 0, 0, 0] and frame[-1, -1].tolist() == [255, 255, 255, 0]
    got = _convert(gpu, False, None, [frame], w, h)
    _assert_same_payload(got, yr.yuv_reference(frame), w, h, "every colour")
    y, cb, cr = yr.split_planes(got, w, h)
    assert y.min() == 0 and y.max() == 1023 and cb.max() <= 1023 and cr.max() <= 1023


@pytest.mark.gpu
@pytest.mark.parametrize("shape", list(SATURATION_SHAPES))
def test_saturated_colours_on_the_gpu(gpu, shape):
    """The min(1023, .) of ptl_cb10 / ptl_cr10 and the zero end, on both paths: flat cube corners (the bands and the 16x2 frames take the
    block path, where every left tap of the 16x2 frames clamps and lane 0 loads its own left column; 5x3 and 1x1 the general one), as one
    sub-frame, as identical sub-frames and as white + black.  No random or every-colour frame gets there (unclamped Cb <= 1011, Cr <= 1007)."""
    w, h = SATURATION_SHAPES[shape]
    assert (w % 16 == 0 and h % 2 == 0) == (shape in ("bands-128x4", "flat-16x2"))
    reached = {"cb_clamp": 0, "cr_clamp": 0, "cb_zero": 0, "cr_zero": 0}
    for label, frames in _saturation_inputs(shape):
        a = _averaged(False, frames)
        got = _convert(gpu, False, None, frames, w, h)
        _assert_same_payload(got, yr.yuv_reference(a), w, h, f"{shape} {label}")
        _, cb, cr = yr.split_planes(got, w, h)
        _, ucb, ucr = yr.yuv_planes(a, clamp=False)
        assert ucb.max() <= 1024 and ucr.max() <= 1024
        assert np.array_equal(cb == 1023, ucb >= 1023) and np.array_equal(cr == 1023, ucr >= 1023), (shape, label)
        assert (cb[ucb == 1024] == 1023).all() and (cr[ucr == 1024] == 1023).all()
        assert cb.max() <= 1023 and cr.max() <= 1023
        reached["cb_clamp"] += int((ucb == 1024).sum())
        reached["cr_clamp"] += int((ucr == 1024).sum())
        reached["cb_zero"] += int((cb == 0).sum())
        reached["cr_zero"] += int((cr == 0).sum())
        if label == "white+black":
            y, _, _ = yr.split_planes(got, w, h)
            assert (a[..., :3] == 180).all() and (y == (262915 * 180 + 32768) >> 16).all() and (cb == 512).all() and (cr == 512).all()
    assert all(reached.values()), (shape, reached)  # not vacuous: the clamp was reached (unclamped 1024) in both planes, and so was 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("kind", list(KNOB_SHAPES))
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, kind, cap, n):
    """`for (b = first; b < n_blocks; b += stride)` of ptl_yuv_frame going round more than twice, on both paths and both entries (n = 65: the
    pointer table): PTL_AVERAGE_IMAGES_GRID_CAP, which launch_over_subframes reads at each call, shrinks the grid to 1 and 3 workgroups.
    256x134 is 2 144 blocks: with 3 workgroups the third trip ends after 608 lanes, in the middle of a wave, and the __shfl_up of the
    block path still finds its lower neighbour.  Equal to the reference and to the same call with the shipped grid."""
    w, h = KNOB_SHAPES[kind]
    frames, want = _case_payload("yuv420", False, 3000 + 10 * n + len(kind), n, w, h, lambda frames, a: yr.yuv_reference(a))  # once per (shape, n), shared by the caps
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None
    shipped = _convert(gpu, False, None, frames, w, h)
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    lanes = _yuv_lanes(w, h)
    assert lanes > 2 * cap * 256 and lanes <= _shipped_grid_cap() * 256  # the knob makes the trips, not the shape
    got = _convert(gpu, False, None, frames, w, h)  # (checks the guard bytes behind the frame)
    _assert_same_payload(got, want, w, h, f"{kind} cap={cap} n={n}")
    assert got == shipped


@pytest.mark.gpu
@pytest.mark.parametrize("kind", list(CAP_CROSSING))
def test_grid_stride_at_the_shipped_cap(gpu, monkeypatch, kind):
    """The second trip of the grid-stride loop as an 8K clip runs it, with no knob: launch_over_subframes caps the grid at
    `long cap = 256 * 16` workgroups = 2^20 lanes, 2050x2049 has 1 050 625 chroma samples (general path) and 4096x4112 has 1 052 672
    blocks (block path).  n = 2, against the reference."""
    import torch
    from oracle import postprocess as pp

    w, h = CAP_CROSSING[kind]
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None
    lanes = _yuv_lanes(w, h)
    assert _shipped_grid_cap() == 4096 and lanes > 4096 * 256
    g = torch.Generator(device="cuda").manual_seed(w)
    frames = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2)]
    got = _convert(gpu, False, None, frames, w, h)
    want = yr.yuv_reference(pp.average_images([f.cpu().numpy() for f in frames]))
    _assert_same_payload(got, want, w, h, kind)


@pytest.mark.gpu
def test_full_size_properties(gpu):
    """4K, 4 sub-frames: permuting the inputs changes no byte; four copies of one frame equal n = 1 of that frame, which equals the reference."""
    import torch

    w, h = 3840, 2160
    g = torch.Generator(device="cuda").manual_seed(5)
    frames = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
    forward = _convert(gpu, False, None, frames, w, h)
    assert forward == _convert(gpu, False, None, list(reversed(frames)), w, h)
    one = _convert(gpu, False, None, [frames[0]], w, h)
    assert one == _convert(gpu, False, None, [frames[0]] * 4, w, h)
    _assert_same_payload(one, yr.yuv_reference(frames[0].cpu().numpy()), w, h, "4K n=1")
    assert forward != one


@pytest.mark.gpu
def test_elapsed_ms_and_a_stream_of_the_callers(gpu):
    """Like ptl_average_images: launched on the stream it is given (here a non-default torch stream, with the inputs produced on it),
    and with elapsed_ms the launch is bracketed by events and waited for."""
    import torch
    from oracle import postprocess as pp

    pa = gpu
    w, h = 640, 360
    nbytes = pa.yuv420p10_frame_bytes(w, h)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.Generator(device="cuda").manual_seed(11)
        frames = [torch.randint(0, 256, (h, w, 4), dtype=torch.uint8, device="cuda", generator=g) for _ in range(4)]
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        ms = pa.average_to_yuv420p10_device([f.data_ptr() for f in frames], out.data_ptr(), w, h, stream=side.cuda_stream, timed=True)
        assert ms is not None and 0.0 < ms < 1000.0
        got = out.cpu().numpy().tobytes()  # the timed call has waited; the copy is ordered behind it on the same stream anyway
        out.zero_()
        assert pa.average_to_yuv420p10_device([f.data_ptr() for f in frames], out.data_ptr(), w, h, stream=side.cuda_stream) is None
        side.synchronize()
        assert out.cpu().numpy().tobytes() == got
    want = yr.yuv_reference(pp.average_images([f.cpu().numpy() for f in frames]))
    _assert_same_payload(got, want, w, h, "side stream")


# ---- the CLI ---------------------------------------------------------------------------------
def _options(blur):
    return ["--motion-blur-frames", str(blur), "--aa-count", "2", "--render-depth", "12"]


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [3, 1])
def test_render_cli_streams_the_frames_the_library_draws(gpu, tmp_path, blur):
    """`portal-amd render --frames y4m` end to end, with motion blur (a, b) and with --motion-blur-frames 1 (c): without an ffmpeg the
    stream is <clip>.y4m; with one it goes through the encoder's stdin -- here a stub that copies stdin to its last argument, so the
    .mov holds the stream byte for byte.  Header, frame count, every payload, the PNG stills; no anim/ directory."""
    from oracle import postprocess as pp

    pa = gpu
    want, frames, clip = _expected_stream(pa, blur, 420, lambda subs8, subs32: yr.yuv_reference(pp.average_images(subs8)))
    assert want.startswith(yr.y4m_header(W, H, FPS) + b"FRAME\n")
    first, last, count = frames[0][0][0], frames[-1][0][-1], len(frames)
    video = tmp_path / "file" / "video" / "basics"
    out = _render(pa, tmp_path / "file", clip, _options(blur))
    _check_stream((video / f"{clip}.y4m").read_bytes(), want, count)
    assert "ffmpeg -f yuv4mpegpipe -i" in out.stdout  # the message names the command that would encode the file
    assert np.array_equal(pa.png_read(str(video / f"{clip}.start.png")), first)
    assert np.array_equal(pa.png_read(str(video / f"{clip}.end.png")), last)
    assert not (tmp_path / "file" / "anim").exists() and not (video / f"{clip}.frames").exists() and not (video / f"{clip}.mov").exists()

    args_file = tmp_path / "stub_args.txt"
    out = _render(pa, tmp_path / "pipe", clip, _options(blur), path=_copying_stub(tmp_path / "bin", args_file))
    video = tmp_path / "pipe" / "video" / "basics"
    _check_stream((video / f"{clip}.mov").read_bytes(), want, count)
    args = args_file.read_text().splitlines()
    assert args[:4] == ["-f", "yuv4mpegpipe", "-i", "-"] and args[4:6] == ["-c:v", "libx265"] and args[-1] == str(video / f"{clip}.mov")
    assert not any("zscale" in a or a in ("-framerate", "-vf") or "frame_%d" in a for a in args)
    assert "ffmpeg status: 0" in out.stdout
    assert np.array_equal(pa.png_read(str(video / f"{clip}.start.png")), first)
    assert np.array_equal(pa.png_read(str(video / f"{clip}.end.png")), last)
    assert not (tmp_path / "pipe" / "anim").exists() and not (video / f"{clip}.y4m").exists()


@pytest.mark.gpu
def test_render_cli_fails_when_the_encoder_dies(gpu, tmp_path):
    """(d) An encoder that exits at once: the CLI reports it and returns non-zero, within the timeout, instead of blocking on the pipe."""
    pa = gpu
    clip = pa.Scene.from_file(pa.scene_path("basics")).animations()[0][0]
    out = _render(pa, tmp_path / "dead", clip, _options(3), path=_write_stub(tmp_path / "bin", 'if [ "$1" = "-version" ]; then exit 0; fi\nexit 1\n'), check=False)
    assert out.returncode not in (0, 2), out.stderr + out.stdout
    assert "encoder" in out.stderr
