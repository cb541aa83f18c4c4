"""16-bit PNG stills and frames from the float sub-frames (`render --png-depth 16`, `render-frame --png-depth 16`): the kernel
(portal_amd/csrc/kernels/rgb48_f32.hip), the C ABI (ptl_average_f32_to_rgb48, ptl_png_write_rgb48), the Python mirror and the CLI, against
tests/png16_reference.py (a numpy restatement of the contract on top of yuv_deep_reference.encode16, and a PNG reader on zlib).  Every
comparison is equality of bytes."""
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import png16_reference as pr
from tests import yuv_deep_reference as dr
from tests.yuv_harness import (FPS, GUARD, H, HIPCC, KNOB, ROOT, W, _c_getenv, _case, _compile_with_usage, _drawn_clip, _frame_from_values, _once, _path_without_ffmpeg,
                               _random_frames, _shipped_grid_cap, _special_values, gpu)  # noqa: F401 (gpu: a fixture)

FILTERS = (pr.FILTER_NONE, pr.FILTER_SUB)
ENTRIES = {f"ptl_average_f32_to_rgb48_{f}{t}_kernel" for f in ("none", "sub") for t in ("", "_table")}
# adjacent 16-bit values whose difference carries out of the low byte, wraps in both bytes, or moves the bytes in opposite directions: a
# subtraction that borrows from one byte into the next gets each of them wrong
PAIRS = ((0x00ff, 0x0100), (0xffff, 0x0000), (0x00ff, 0xff00))


def _exact(values):
    """16-bit values -> the floats k / 65535, which quantise to k."""
    v = (np.asarray(values, np.int64) / 65535.0).astype(np.float32)
    assert np.array_equal(dr.quantise16(v), np.asarray(values, np.int64))
    return v


def _frame_of_a(a):
    """A (H, W, 3) -> one float sub-frame that encodes to it (alpha: NaN, which is ignored)."""
    frame = np.full(a.shape[:2] + (4,), np.nan, np.float32)
    frame[..., :3] = _exact(a)
    return frame


def _directed(w, h, seed):
    """Random 16-bit values with the PAIRS in adjacent pixels: in every channel (so in each of the six byte positions of a pixel), with the
    left pixel at the columns `at` -- inside a lane's block, on the boundary between two lanes (3 | 4), between two waves (255 | 256) and on
    the last lane boundary of a row -- and once in all three channels together."""
    a = np.random.default_rng(seed).integers(0, 65536, (h, w, 3)).astype(np.int64)
    at = sorted({x for x in (1, 3, 255, w - 5) if 0 <= x < w - 1})
    row = 0
    for x in at:
        for before, after in PAIRS:
            for c in range(3):
                a[row % h, x, c], a[row % h, x + 1, c] = before, after
                row += 1
            a[row % h, x], a[row % h, x + 1] = before, after
            row += 1
    assert row <= h, "the pairs overwrite each other"
    return a


# ---------------------------------------------------------------------------------------------
# CPU: the reference, the writer, the entry point, the build, the CLI's refusals
# ---------------------------------------------------------------------------------------------
def test_sub_rows_are_undone_by_a_prefix_sum_per_byte_lane():
    """rows(..., SUB) summed along the row in each of the six byte lanes, mod 256, gives the raw rows -- for random A, and for rows made of
    the byte pairs where a borrow would show."""
    a = np.random.default_rng(1).integers(0, 65536, (7, 33, 3)).astype(np.int64)
    for before, after in PAIRS:
        alternating = np.where((np.arange(40) % 2 == 0)[None, :, None], before, after) * np.ones((2, 40, 3), np.int64)
        for case in (a, alternating, _directed(64, 40, 2)):
            h, w = case.shape[:2]
            raw, sub = pr.rows_from_a(case, pr.FILTER_NONE), pr.rows_from_a(case, pr.FILTER_SUB)
            assert len(raw) == len(sub) == 6 * w * h and raw != sub
            assert np.array_equal(pr.undo(sub, w, h, pr.FILTER_SUB), case) and np.array_equal(pr.undo(raw, w, h, pr.FILTER_NONE), case)
            assert np.frombuffer(sub, np.uint8).reshape(h, 6 * w)[:, :6].tobytes() == np.frombuffer(raw, np.uint8).reshape(h, 6 * w)[:, :6].tobytes()  # every row starts from zero
    assert pr.rows_from_a(np.array([[[0x00ff] * 3, [0x0100] * 3]]), pr.FILTER_SUB) == bytes([0x00, 0xff] * 3 + [0x01, 0x01] * 3)
    assert pr.rows_from_a(np.array([[[0xffff] * 3, [0x0000] * 3]]), pr.FILTER_SUB) == bytes([0xff, 0xff] * 3 + [0x01, 0x01] * 3)
    assert pr.rows_from_a(np.array([[[0x00ff] * 3, [0xff00] * 3]]), pr.FILTER_SUB) == bytes([0x00, 0xff] * 3 + [0xff, 0x01] * 3)
    assert pr.rows_from_a(np.array([[[0x1234, 0x5678, 0x9abc]]]), pr.FILTER_NONE) == bytes([0x12, 0x34, 0x56, 0x78, 0x9a, 0xbc])
    frames = _random_frames(3, 3, 9, 5)
    assert pr.rows(frames, pr.FILTER_NONE) == dr.encode16(frames).astype(">u2").tobytes()


def test_a_4096_step_ramp_keeps_its_4096_codes():
    """What the feature is for: 4 096 equal steps in [0, 1) stay 4 096 distinct codes in the 16-bit frame; the 8-bit frame keeps 256."""
    ramp = (np.arange(4096) / 4096.0).astype(np.float32)
    frame = np.repeat(ramp[None, :, None], 4, axis=2)
    a = pr.undo(pr.rows([frame], pr.FILTER_SUB), 4096, 1, pr.FILTER_SUB)
    assert len(np.unique(a[0, :, 0])) == 4096 and np.array_equal(a[..., 0], a[..., 1]) and (np.diff(a[0, :, 2]) > 0).all()
    eight = np.floor(ramp * np.float32(255.0) + np.float32(0.5)).astype(np.int64)  # unorm8 of the render entries
    assert len(np.unique(eight)) == 256


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 36)])
def test_png_write_rgb48_files_decode_to_the_averaged_frame(pa, tmp_path, w, h):
    """Reference rows through the writer, both filters, levels 0, 3 and 9: the independent reader returns A, ptl_png_read returns A >> 8
    with alpha 255, and IHDR says 16 bits, colour type 2."""
    frames = _random_frames(w + h, 2, w, h)
    a = dr.encode16(frames)
    for filter in FILTERS:
        payload = pr.rows(frames, filter)
        for level in (0, 3, 9):
            path = str(tmp_path / f"f{filter}_l{level}.png")
            pa.png_write_rgb48(path, payload, w, h, filter, level)
            image, header = pr.read_png16(path, header=True)
            assert np.array_equal(image, a), (filter, level)
            assert header["ihdr"] == w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([16, 2, 0, 0, 0]) and header["idat_chunks"] == 1
            assert (header["filter_types"] == filter).all()
            eight = pa.png_read(path)
            assert eight.shape == (h, w, 4) and np.array_equal(eight[..., :3], a >> 8) and (eight[..., 3] == 255).all()
    sizes = {level: os.path.getsize(tmp_path / f"f1_l{level}.png") for level in (0, 9)}
    assert sizes[0] >= 6 * w * h + h and sizes[9] > 0
    assert pa.rgb48_frame_bytes(w, h) == 6 * w * h == len(payload) and pa.rgb48_frame_bytes(0, 4) == 0 and pa.rgb48_frame_bytes(4, -1) == 0
    assert (pa.PNG_FILTER_NONE, pa.PNG_FILTER_SUB) == (pr.FILTER_NONE, pr.FILTER_SUB) == (0, 1)


def test_png_write_rgb48_refuses(pa, tmp_path):
    """Null pointers, sizes that are not positive, level 10, PNG's other filter types -> PTL_ERR_INVALID, no file."""
    f = pa.lib().ptl_png_write_rgb48
    rows = np.zeros(6 * 4 * 2, np.uint8)
    path = str(tmp_path / "no.png").encode()
    assert f(None, rows.ctypes.data, 4, 2, 1, 6) == -1 and f(path, None, 4, 2, 1, 6) == -1
    assert f(path, rows.ctypes.data, 0, 2, 1, 6) == -1 and f(path, rows.ctypes.data, 4, 0, 1, 6) == -1 and f(path, rows.ctypes.data, -4, 2, 1, 6) == -1
    assert f(path, rows.ctypes.data, 4, 2, 1, 10) == -1 and f(path, rows.ctypes.data, 4, 2, 1, -1) == -1
    for filter in (2, 3, 4, -1):
        assert f(path, rows.ctypes.data, 4, 2, filter, 6) == -1
    assert not os.listdir(tmp_path)
    assert f(path, rows.ctypes.data, 4, 2, 0, 6) == 0 and os.listdir(tmp_path) == ["no.png"]
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    assert "int ptl_png_write_rgb48(" in header and "#define PTL_PNG_FILTER_NONE 0" in header and "#define PTL_PNG_FILTER_SUB 1" in header


def test_entry_point_refuses_before_any_gpu_call(pa):
    """No frames, bad counts, bad sizes, unaligned pointers, more pixels than 32-bit byte offsets reach, an unknown filter -> PTL_ERR_INVALID;
    no device needed."""
    import ctypes as C

    f = pa.lib().ptl_average_f32_to_rgb48
    ptrs = (C.c_void_p * 2)(4096, 8192)
    out = C.c_void_p(1 << 20)
    for filter in FILTERS:
        assert f(0, None, 2, out, 4, 4, filter, None, None) == -1
        assert f(0, ptrs, 2, None, 4, 4, filter, None, None) == -1
        assert f(0, (C.c_void_p * 2)(4096, None), 2, out, 4, 4, filter, None, None) == -1
        assert f(0, ptrs, 0, out, 4, 4, filter, None, None) == -1
        many = (C.c_void_p * 257)(*([4096] * 257))
        assert f(0, many, 257, out, 4, 4, filter, None, None) == -1
        assert f(0, (C.c_void_p * 2)(4096, 8200), 2, out, 4, 4, filter, None, None) == -1  # 8-byte aligned only
        assert f(0, ptrs, 2, C.c_void_p((1 << 20) + 8), 4, 4, filter, None, None) == -1
        assert f(0, ptrs, 2, out, 0, 4, filter, None, None) == -1
        assert f(0, ptrs, 2, out, 4, -2, filter, None, None) == -1
        assert f(0, ptrs, 2, out, 1 << 14, (1 << 14) + 1, filter, None, None) == -1  # beyond 2^28 pixels
        assert f(0, ptrs, 2, out, (1 << 14) + 1, 1 << 14, filter, None, None) == -1
    for filter in (2, 3, 4, -1, 420):
        assert f(0, ptrs, 2, out, 4, 4, filter, None, None) == -1
        assert "filter" in pa.lib().ptl_last_error().decode()
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    assert "int ptl_average_f32_to_rgb48(" in header and "size_t ptl_rgb48_frame_bytes(" in header


def test_make_builds_the_code_object_without_scratch(tmp_path):
    """`make portal_amd/kernels/rgb48_f32.hsaco` in a copy of the tree's Makefile and kernel sources: its four entries compile for gfx950 with
    0 bytes of scratch, no spills, no LDS and at most 128 VGPRs; the numbers are printed from the compiler's own notes."""
    shutil.copy(os.path.join(ROOT, "Makefile"), tmp_path / "Makefile")
    shutil.copytree(os.path.join(ROOT, "portal_amd", "csrc", "kernels"), tmp_path / "portal_amd" / "csrc" / "kernels")
    target = "portal_amd/kernels/rgb48_f32.hsaco"
    out = subprocess.run(["make", target, f"HIPCC={HIPCC} -Rpass-analysis=kernel-resource-usage"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / target) > 1000
    from tests.yuv_harness import _resource_usage

    usage = _resource_usage(out.stderr)
    assert set(usage) == ENTRIES
    for entry, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0, (entry, u)
        assert u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (entry, u)
        assert u["VGPRs"] <= 128, (entry, u)  # four waves per SIMD
    print("VGPRs, unroll 2:", {e: u["VGPRs"] for e, u in sorted(usage.items())})
    assert _compile_with_usage("rgb48_f32", tmp_path) == usage  # the harness's own compile line is the Makefile's
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert target in re.search(r"^KERNELS\s*:=(.*)$", makefile, re.M).group(1) and makefile.count("rgb48_shape.h") == 2
    source = open(os.path.join(ROOT, "portal_amd", "csrc", "kernels", "rgb48_f32.hip")).read()
    assert '#include "yuv_common.h"' in source and '#include "rgb48_shape.h"' in source and "asm" not in source and "__shared__" not in source
    assert '#include "../kernels/rgb48_shape.h"' in open(os.path.join(ROOT, "portal_amd", "csrc", "host", "postprocess.cpp")).read()


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--png-depth", "12"], "--png-depth 8|16"), ("render-frame", ["--png-depth", "0"], "--png-depth 8|16"),
                                              ("render-frame", ["--png-depth", "sixteen"], "--png-depth 8|16"),
                                              ("render", ["--png-depth", "16", "--frames", "y4m"], "cannot be combined with --frames y4m"),
                                              ("render", ["--frames", "y4m", "--deep-colour", "--png-depth", "16"], "cannot be combined with --frames y4m"),
                                              ("precompile", ["--png-depth", "16"], "--png-depth is an option of render and render-frame"),
                                              ("check", ["--png-depth", "8"], "--png-depth is an option of render and render-frame"),
                                              ("emit-source", ["--png-depth", "16"], "--png-depth is an option of render and render-frame"),
                                              ("render-frame", ["--png-depth", "16", "--gpus", "2"], "one GPU"),
                                              ("render-frame", ["--devices", "0,1", "--png-depth", "16"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--gpus", "2", "--multi-process"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--multi-process"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--shard", "0/2"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--transport", "rccl"], "one GPU"),
                                              ("render-frame", ["--transport", "rccl", "--device", "0", "--png-depth", "16"], "--transport rccl")])
def test_cli_refuses_while_the_arguments_are_parsed(pa, tmp_path, cmd, extra, reason):
    """Exit status 2, one line that says why, nothing rendered or written."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    target = ["anim.4.portals", "--out-dir", str(tmp_path)] if cmd == "render" else ["--output", str(tmp_path / "f.png")] if cmd == "render-frame" else []
    out = subprocess.run([exe, cmd, pa.scene_path("basics")] + target + extra, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


def test_usage_names_the_option(pa):
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and out.stderr.count("--png-depth 8|16") == 2  # render-frame's and render's


SANITIZED_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "include/portal_amd.h"
namespace ptl { void set_last_error(const std::string& msg) { std::fprintf(stderr, "%s\n", msg.c_str()); } }
int main(int argc, char** argv) {
    const int sizes[3][2] = {{1, 1}, {5, 3}, {64, 36}};
    for (auto& s : sizes)
        for (int filter = 0; filter < 2; ++filter)
            for (int level : {0, 3, 9}) {
                const int w = s[0], h = s[1];
                std::vector<uint8_t> rows((size_t)6 * w * h);  // exactly the bytes the writer may read
                for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint8_t)(i * 37 + 11);
                const std::string path = std::string(argv[1]) + "/s" + std::to_string(w) + "_" + std::to_string(filter) + "_" + std::to_string(level) + ".png";
                if (ptl_png_write_rgb48(path.c_str(), rows.data(), w, h, filter, level) != PTL_OK) return 1;
                uint8_t* rgba = nullptr;
                int rw = 0, rh = 0;
                if (ptl_png_read(path.c_str(), &rgba, &rw, &rh) != PTL_OK || rw != w || rh != h) return 2;
                for (int y = 0; y < h; ++y)  // the high bytes, Sub undone: the running sum of the row's bytes at stride 6
                    for (int c = 0; c < 3; ++c) {
                        uint8_t run = 0;
                        for (int x = 0; x < w; ++x) {
                            const uint8_t byte = rows[((size_t)y * w + x) * 6 + 2 * c];
                            run = filter ? (uint8_t)(run + byte) : byte;
                            if (rgba[((size_t)y * w + x) * 4 + c] != run || rgba[((size_t)y * w + x) * 4 + 3] != 255) return 3;
                        }
                    }
                std::free(rgba);
            }
    if (ptl_png_write_rgb48(nullptr, nullptr, 1, 1, 0, 6) != PTL_ERR_INVALID) return 4;
    std::puts("sanitized writer ok");
    return 0;
}
"""


def test_writer_under_sanitizers(tmp_path):
    """ptl_png_write_rgb48 and ptl_png_read in a stand-alone program compiled with png_io.cpp under AddressSanitizer and
    UndefinedBehaviorSanitizer, run as a plain child process on rows of exactly 6 W H bytes: 1x1, 5x3 and 64x36, both filters, three
    levels; the files are read back.  The sanitizer runtimes are linked statically and the child inherits the environment untouched.  Nothing is
    loaded into Python under a sanitizer."""
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "sanitized_writer"
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT, str(tmp_path / "main.cpp"),
                            os.path.join(ROOT, "portal_amd", "csrc", "host", "png_io.cpp"), "-lz", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", build.stderr):
        print(build.stderr)
        pytest.skip("no sanitizer runtimes to link against on this machine: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    files = tmp_path / "files"
    files.mkdir()
    run = subprocess.run([str(exe), str(files)], capture_output=True, text=True, timeout=120)  # (the environment as it is: the runtimes are linked statically, so nothing about the order of loaded libraries matters)
    assert run.returncode == 0 and "sanitized writer ok" in run.stdout, (run.returncode, run.stderr)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    assert len(os.listdir(files)) == 18
    pr.read_png16(str(files / "s64_1_3.png"))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _is_fast(w):
    return w % 4 == 0


def _lanes(w, h):
    return (w // 4) * h if _is_fast(w) else w * h


def _convert16(pa, frames, w, h, filter, offset=0):
    """Float sub-frames (numpy (h, w, 4), or cuda tensors; the same object may appear more than once) -> the rows; the 64 guard bytes behind
    the frame (and `offset` before it) must survive."""
    import torch

    staged = {}
    for f in frames:
        if id(f) not in staged:
            staged[id(f)] = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda()
            assert staged[id(f)].numel() == w * h * 4 and staged[id(f)].dtype == torch.float32 and staged[id(f)].data_ptr() % 16 == 0
    nbytes = pa.rgb48_frame_bytes(w, h)
    assert nbytes == 6 * w * h and offset % 16 == 0
    buf = torch.full((offset + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    pa.average_f32_to_rgb48_device([staged[id(f)].data_ptr() for f in frames], buf.data_ptr() + offset, w, h, filter, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == GUARD).all() and (host[offset + nbytes:] == GUARD).all(), "written outside the frame"
    return host[offset: offset + nbytes].tobytes()


def _assert_same_rows(got: bytes, want: bytes, w, h, what):
    if got == want:
        return
    assert len(got) == len(want) == 6 * w * h, (what, len(got), len(want))
    g, r = np.frombuffer(got, np.uint8).reshape(h, w, 6), np.frombuffer(want, np.uint8).reshape(h, w, 6)
    bad = np.argwhere(g != r)
    y, x, k = bad[0]
    pytest.fail(f"{what}: {len(bad)} of {g.size} bytes differ, first at x={x} y={y} byte {k}: got {g[y, x].tolist()}, want {r[y, x].tolist()}")


def _check_both(pa, frames, w, h, what, a=None, offset=0):
    """Both filters of the same sub-frames against the reference (A computed once)."""
    a = dr.encode16([f if isinstance(f, np.ndarray) else f.cpu().numpy() for f in frames]) if a is None else a
    for filter in FILTERS:
        _assert_same_rows(_convert16(pa, frames, w, h, filter, offset), pr.rows_from_a(a, filter), w, h, f"{what} filter={filter}")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 64, 65, 256])
@pytest.mark.parametrize("w,h", [(37, 23), (256, 6)])
def test_kernel_matches_reference_for_every_subframe_count(gpu, w, h, n):
    """37x23: the general path.  256x6: the fast path, 64 blocks = a wave per row.  Beyond 64 sub-frames the pointer-table entry."""
    assert _is_fast(w) == ((w, h) == (256, 6))
    _check_both(gpu, _random_frames(100 * n + w, n, w, h), w, h, f"{w}x{h} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (4, 1), (4, 2), (5, 3), (8, 3), (244, 135), (260, 3)])
def test_kernel_matches_reference_at_any_frame_size(gpu, w, h):
    """The smallest frames of both paths; 244x135: 61 blocks per row, so wave starts fall mid-row; 260x3: 65 blocks per row, so lane 0 of
    the second wave takes the left pixel it loaded itself and row 1 starts inside a wave.  Three sub-frames and one, the frame 16 bytes
    into its buffer: nothing before or behind it is written."""
    assert _is_fast(w) == (w in (4, 8, 244, 260))
    frames = _random_frames(w * 1000 + h, 3, w, h)
    _check_both(gpu, frames, w, h, f"{w}x{h}", offset=16)
    _check_both(gpu, frames[:1], w, h, f"{w}x{h} n=1")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(32, 12), (33, 11)])
def test_special_inputs_as_bit_patterns(gpu, w, h):
    """NaN of both signs, both infinities, both zeros, negatives, denormals, 1.0 and its neighbours, values above 1, and the floats around
    the rounding boundaries (k + 1/2) / 65535 -- as one sub-frame, and as two and three.  Both paths."""
    values = _special_values()
    assert values.size <= 3 * w * h and _is_fast(w) == (w == 32)
    frame, reversed_frame = _frame_from_values(values, w, h), _frame_from_values(values[::-1], w, h)
    for frames in ([frame], [frame, reversed_frame], [frame, frame, reversed_frame]):
        _check_both(gpu, frames, w, h, f"{w}x{h} special n={len(frames)}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(4, 2), (5, 3)])
def test_saturated_colours(gpu, w, h):
    """The eight cube corners as flat frames, on both paths, as one sub-frame and as two: Sub leaves the first pixel of a row and zeros."""
    for rgb in [(r, g, b) for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)]:
        frame = np.tile(np.array([c / 65535.0 for c in rgb] + [0.25], np.float32), (h, w, 1))
        for n in (1, 2):
            _check_both(gpu, [frame] * n, w, h, f"{rgb} n={n}")
            sub = np.frombuffer(_convert16(gpu, [frame] * n, w, h, pr.FILTER_SUB), np.uint8).reshape(h, w, 6)
            assert not sub[:, 1:].any() and np.array_equal(sub[:, 0] == 255, np.repeat(np.array(rgb) == 65535, 2)[None].repeat(h, 0))


@pytest.mark.gpu
def test_every_16_bit_value_once(gpu):
    """256x256, n = 1: pixel p holds p / 65535, (65535 - p) / 65535 and (7 p mod 65536) / 65535 -- every value in every channel."""
    w = h = 256
    p = np.arange(65536, dtype=np.int64)
    a = np.stack([p, 65535 - p, (7 * p) % 65536], axis=1).reshape(h, w, 3)
    for c in range(3):
        assert np.array_equal(np.sort(a[..., c].ravel()), p)
    _check_both(gpu, [_frame_of_a(a)], w, h, "every value", a=a)


@pytest.mark.gpu
def test_no_byte_borrows_from_its_neighbour(gpu):
    """1024x64, n = 1, random 16-bit values and the directed pairs in adjacent pixels, in each of the six byte positions, inside a lane's
    block, across two lanes and across two waves; the same values through the general path (1023 columns)."""
    w, h = 1024, 64
    a = _directed(w, h, 48)
    frame = _frame_of_a(a)
    assert np.array_equal(dr.encode16([frame]), a)
    _check_both(gpu, [frame], w, h, "directed pairs", a=a)
    _check_both(gpu, [frame[:, : w - 1]], w - 1, h, "directed pairs, general path", a=a[:, : w - 1])
    _check_both(gpu, [frame, frame], w, h, "directed pairs n=2", a=a)  # identical sub-frames average to themselves


KNOB_SHAPES = {"fast-136x70": (136, 70), "general-61x29": (61, 29)}


def test_knob_shapes_make_the_trips_they_are_meant_to():
    assert _shipped_grid_cap() == 4096
    assert _lanes(136, 70) == 2380 and _lanes(61, 29) == 1769
    for w, h in KNOB_SHAPES.values():
        for cap in (1, 3):
            assert 2 * cap * 256 < _lanes(w, h) <= 4096 * 256  # at least three trips, all of them the knob's
    assert 2380 % 256 == 76 and 2380 % 768 == 76 and 76 % 64 == 12  # fast path: the last trip ends in the middle of a wave, under both caps
    assert 136 // 4 == 34 and 34 % 64  # ... and rows start in the middle of a wave: lanes 0 of most waves load their left pixel themselves
    assert 4096 * 256 < _lanes(2052, 2050) == 1051650 < 2 * 4096 * 256  # the shipped cap crossed once


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("kind", list(KNOB_SHAPES))
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, kind, cap, n):
    """The grid-stride loops going round more than twice, on both paths and both entries (n = 65: the pointer table), with 1 and 3
    workgroups: the cross-lane move of the Sub filter still finds its lower neighbour when a trip ends inside a wave.  Equal to the
    reference and to the same call with the shipped grid."""
    w, h = KNOB_SHAPES[kind]
    assert _is_fast(w) == kind.startswith("fast")
    frames, a = _case(True, 9000 + 10 * n + len(kind), n, w, h)  # once per (shape, n), shared by the caps
    for filter in FILTERS:
        monkeypatch.delenv(KNOB, raising=False)
        assert _c_getenv(KNOB) is None
        shipped = _convert16(gpu, frames, w, h, filter)
        monkeypatch.setenv(KNOB, str(cap))
        assert _c_getenv(KNOB) == str(cap).encode()
        got = _convert16(gpu, frames, w, h, filter)
        _assert_same_rows(got, pr.rows_from_a(a, filter), w, h, f"{kind} cap={cap} n={n} filter={filter}")
        assert got == shipped


@pytest.mark.gpu
def test_grid_stride_at_the_shipped_cap(gpu, monkeypatch):
    """The second trip with no knob: 2052x2050 is 1 051 650 blocks against 4096 x 256 lanes; n = 1, a 67 MB input made on the card."""
    import torch

    w, h = 2052, 2050
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None and _lanes(w, h) > _shipped_grid_cap() * 256
    g = torch.Generator(device="cuda").manual_seed(2052)
    frame = torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=g) * 1.25 - 0.125
    _check_both(gpu, [frame], w, h, "2052x2050")


@pytest.mark.gpu
def test_elapsed_ms_and_a_stream_of_the_callers(gpu):
    """Launched on the stream it is given (a non-default torch stream, the inputs produced on it); with elapsed_ms the launch is bracketed by
    events and waited for."""
    import torch

    pa = gpu
    w, h = 640, 360
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.Generator(device="cuda").manual_seed(11)
        frames = [torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=g) for _ in range(4)]
        out = torch.zeros(pa.rgb48_frame_bytes(w, h), dtype=torch.uint8, device="cuda")
        ms = pa.average_f32_to_rgb48_device([f.data_ptr() for f in frames], out.data_ptr(), w, h, pa.PNG_FILTER_SUB, stream=side.cuda_stream, timed=True)
        assert ms is not None and 0.0 < ms < 1000.0
        got = out.cpu().numpy().tobytes()  # the timed call has waited; the copy is ordered behind it on the same stream anyway
        out.zero_()
        assert pa.average_f32_to_rgb48_device([f.data_ptr() for f in frames], out.data_ptr(), w, h, pa.PNG_FILTER_SUB, stream=side.cuda_stream) is None
        side.synchronize()
        assert out.cpu().numpy().tobytes() == got
    _assert_same_rows(got, pr.rows([f.cpu().numpy() for f in frames], pr.FILTER_SUB), w, h, "side stream")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 9), (37, 5)])
def test_the_same_tensor_listed_several_times(gpu, w, h):
    """[a, b, a, a]: a sub-frame may be listed more than once; each listing counts."""
    a, b = _random_frames(w + 7, 2, w, h)
    _check_both(gpu, [a, b, a, a], w, h, f"{w}x{h} repeated")


# ---- the CLI ---------------------------------------------------------------------------------
def _run_cli(pa, arguments, limit=300):
    """One child under a time limit of its own, no ffmpeg on its PATH."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run(["timeout", "-k", "10", str(limit), exe] + arguments, capture_output=True, text=True, timeout=limit + 100, env=dict(os.environ, PATH=_path_without_ffmpeg()), cwd=ROOT)
    assert out.returncode == 0, out.stderr + out.stdout
    return out


def _render_clip(pa, out_dir, clip, options):
    scene = pa.scene_path("basics")
    return _run_cli(pa, ["render", scene, clip, "--width", str(W), "--height", str(H), "--fps", str(FPS), "--out-dir", str(out_dir), "--asset-root", os.path.dirname(os.path.dirname(scene)),
                         "--aa-count", "2", "--render-depth", "12"] + options)


def _drawn_clip_adaptive(pa, blur, threshold):
    """_drawn_clip with every sub-frame an adaptive draw (the refine entry): per frame the float sub-frames.  -> (frames, clip name)"""
    def draw():
        clip, duration = pa.Scene.from_file(pa.scene_path("basics")).animations()[0]
        count = max(1, int(np.float32(duration) * np.float32(FPS)))
        scene = pa.Scene.from_file(pa.scene_path("basics"))
        r = pa.SceneRenderer(scene, device=0, flags=pa.FLAG_REFINE)
        r.set_option("aa_count", 2)
        r.set_option("render_depth", 12)
        scene.init_animation(clip)
        r.update(0.0)
        frames = []
        for i in range(count):
            subs32 = []
            for j in range(blur):
                r.set_option("aa_start", j)
                r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
                subs32.append(np.array(r.draw_adaptive(W, H, threshold=threshold, rgba32f=True)["rgba32f"]))
            frames.append(subs32)
        return frames, clip

    return _once(("png16 adaptive clip", blur, threshold), draw)


def _clip_frames(pa, blur, adaptive):
    """Per frame of the clip the float sub-frames the CLI draws -> (list of sub-frame lists, clip name)"""
    if adaptive is not None:
        return _drawn_clip_adaptive(pa, blur, adaptive)
    frames, clip = _drawn_clip(pa, blur)
    return [subs32 for _, subs32 in frames], clip


@pytest.mark.gpu
@pytest.mark.parametrize("blur,adaptive,more", [(3, None, []), (1, None, []), (3, 4, []), (2, 4, ["--batch-subframes", "0"])])
def test_render_cli_writes_16_bit_frames(gpu, tmp_path, blur, adaptive, more):
    """`portal-amd render ... --png-depth 16` with no ffmpeg on the PATH: every frame_<i>.png, decoded by the independent reader, is encode16
    of the float sub-frames of the same draws -- batched (blur 3), one sub-frame (blur 1: converted with n = 1), with --clip-adaptive-aa 4
    batched and, with --batch-subframes 0, as one adaptive draw per sub-frame: the four draw calls of the clip loop.  The start still stays
    8-bit.  Once more with --shard 1/2: only the odd frames exist, and they are the same files."""
    pa = gpu
    frames, clip = _clip_frames(pa, blur, adaptive)
    options = ["--motion-blur-frames", str(blur)] + (["--clip-adaptive-aa", str(adaptive)] if adaptive is not None else []) + more + ["--png-depth", "16"]
    _render_clip(pa, tmp_path / "whole", clip, options)
    video = tmp_path / "whole" / "video" / "basics"
    kept = video / f"{clip}.frames"  # (no ffmpeg: the clip's anim/ is parked next to where the video would be)
    assert sorted(os.listdir(kept)) == sorted(f"frame_{i}.png" for i in range(len(frames))) and len(frames) >= 2
    for i, subs32 in enumerate(frames):
        image, header = pr.read_png16(str(kept / f"frame_{i}.png"), header=True)
        assert (header["width"], header["height"]) == (W, H) and (header["filter_types"] == 1).all()
        want = dr.encode16(subs32)
        assert np.array_equal(image, want), f"frame {i}: {int((image != want).any(axis=2).sum())} of {W * H} pixels differ"
    start = (video / f"{clip}.start.png").read_bytes()
    assert start[24] == 8 and start[25] == 6  # IHDR of the still: 8 bits, RGBA
    assert pa.png_read(str(video / f"{clip}.start.png")).shape == (H, W, 4)
    _render_clip(pa, tmp_path / "shard", clip, options + ["--shard", "1/2"])
    anim = tmp_path / "shard" / "anim"
    assert sorted(os.listdir(anim)) == sorted(f"frame_{i}.png" for i in range(1, len(frames), 2))
    for name in os.listdir(anim):
        assert (anim / name).read_bytes() == (kept / name).read_bytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("adaptive", [None, 4])
def test_render_frame_cli_writes_a_16_bit_file(gpu, tmp_path, adaptive):
    """`portal-amd render-frame scenes/basics.ron --png-depth 16` at 70x37 (the general path), with and without --adaptive-aa 4: the decoded
    file is encode16 of the one float frame the Python mirror draws for the same state, and ptl_png_read still opens it.  Without the
    option the call writes today's 8-bit file: the mirror's RGBA8 frame."""
    pa = gpu
    w, h = 70, 37
    spec = pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL
    common = ["render-frame", pa.scene_path("basics"), "--width", str(w), "--height", str(h), "--aa-count", "4", "--render-depth", "12"] + (["--adaptive-aa", "4"] if adaptive is not None else [])
    _run_cli(pa, common + ["--png-depth", "16", "--output", str(tmp_path / "deep.png")])
    _run_cli(pa, common + ["--output", str(tmp_path / "plain.png")])
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path("basics")), device=0, flags=spec | pa.FLAG_QUICK_JIT | (pa.FLAG_REFINE if adaptive is not None else 0))
    r.set_option("aa_count", 4)
    r.set_option("render_depth", 12)
    r.set_option("view_angle", 90.0 / 180.0 * math.pi)
    r.update(0.0)
    mirror = r.draw_adaptive(w, h, threshold=adaptive, rgba32f=True) if adaptive is not None else r.draw(w, h, rgba8=True, rgba32f=True)
    image, header = pr.read_png16(str(tmp_path / "deep.png"), header=True)
    want = dr.encode16([np.array(mirror["rgba32f"])])
    assert (header["width"], header["height"]) == (w, h) and (header["filter_types"] == 1).all()
    assert np.array_equal(image, want), f"{int((image != want).any(axis=2).sum())} of {w * h} pixels differ"
    opened = pa.png_read(str(tmp_path / "deep.png"))
    assert np.array_equal(opened[..., :3], want >> 8) and (opened[..., 3] == 255).all()
    plain = (tmp_path / "plain.png").read_bytes()
    assert plain[24] == 8 and plain[25] == 6
    assert np.array_equal(pa.png_read(str(tmp_path / "plain.png")), np.array(mirror["rgba8"]))
    assert len(np.unique(want)) > 256  # the frame holds more than 8 bits can
