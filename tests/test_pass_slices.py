"""Pass images of a clip's frames without a GPU: the numpy restatement of ptl_pass_slices_to_gray16 against tests/pass_reference.py and Python
integers, the entry point's and the command line's refusals, and the cross-compile of the kernel.  The GPU leg is tests/test_gpu_pass_slices.py.
"""
import ctypes as C
import functools
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from tests import pass_reference as ref
from tests import pass_slices_reference as sref
from tests.yuv_harness import _compile_with_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPECIAL_DEPTHS = np.array([np.nan, -np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-30, -1e-30, 0.5, 1.0, 2.75, -3.5, 9.25e5], np.float32)


def random_slices(n_slices, n, seed):
    """(n_slices, n) records that exercise every field: special depths, trips around and far beyond 65535, slices with and without final paths."""
    rng = np.random.default_rng(seed)
    shape = (n_slices, n)
    depth = np.where(rng.random(shape) < 0.3, rng.choice(SPECIAL_DEPTHS, shape), rng.normal(2.0, 3.0, shape)).astype(np.float32)
    trips = rng.choice(np.array([0, 1, 2, 7, 40, 300, 65534, 65535, 65536, 70000, 2**32 - 1], np.uint32), shape)
    final = rng.integers(0, 4, shape) * (rng.random(shape) < 0.6)
    escaped, outside = rng.integers(0, 4, shape), rng.integers(0, 3, shape)
    exhausted = rng.integers(0, 4, shape) * (rng.random(shape) < 0.4)
    if n > 3:
        final[0, 0], escaped[0, 1], exhausted[0, 2], outside[0, 3] = 65535, 65535, 65535, 65535
    return ref.records(depth, trips, final, escaped, exhausted, outside)


# ---- the reference itself ---------------------------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(0.0, 1.0), (-1.0, 7.5), (2.75, 2.75), (5.0, 1.0), (np.nan, 1.0)])
def test_one_slice_is_passes_to_gray16(lo, hi):
    rec = random_slices(1, 5000, 3)
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, 0x3F800000], np.uint32).view(np.float32)
    special = ref.records(np.concatenate([bits, bits]), 7, final=np.repeat([1, 0], bits.size))[None]
    for slices in (rec, special):
        got = sref.gray16(slices, lo, hi)
        assert np.array_equal(got["depth"], ref.gray16(slices[0], ref.DEPTH, lo, hi))
        assert np.array_equal(got["trips"], ref.gray16(slices[0], ref.TRIPS))


def test_the_depth_rule():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    # pixel 0: the first slice with a final path has a NaN depth: it stays (no later depth is < NaN) and quantises to 0
    # pixel 1: a slice WITHOUT a final path holds a finite garbage depth nearer than all: never read
    # pixel 2: later equal depths change nothing; pixel 3: a later nearer one replaces; pixel 4: no final path anywhere
    # pixel 5: the first slice has no final path and a NaN: skipped, the later finite one counts
    depth = np.array([[nan, 0.10, 0.50, 0.75, 0.20, nan], [0.25, 0.75, 0.50, 0.25, 0.30, 0.50], [0.10, 0.50, 0.50, 0.50, inf, 0.75]], np.float32)
    final = np.array([[1, 0, 1, 1, 0, 0], [1, 1, 1, 2, 0, 1], [1, 1, 3, 1, 0, 1]])
    slices = ref.records(depth, 1, final=final)
    d, has = sref.merged_depth(slices)
    assert np.isnan(d[0]) and d[1:4].tolist() == [0.5, 0.5, 0.25] and d[5] == 0.5 and has.tolist() == [True, True, True, True, False, True]
    assert sref.depth(slices, 0.0, 1.0).tolist() == [0, 32768, 32768, 16384, 0, 32768]


def test_trips_saturate_and_do_not_wrap():
    slices = ref.records(np.zeros((2, 3), np.float32), np.array([[65533, 65534, 65535], [1, 1, 1]], np.uint32))
    assert sref.trips(slices).tolist() == [65534, 65535, 65535]
    many = ref.records(np.zeros((256, 2), np.float32), np.array([[2**32 - 1, 0]] * 255 + [[2**32 - 1, 9]], np.uint32))
    assert sref.trips(many).tolist() == [65535, 9]  # 256 (2^32 - 1) is 0xFFFFFF00 modulo 2^32, and that would pass; 2^40 - 256 is what is clamped
    wrapping = ref.records(np.zeros((2, 1), np.float32), np.array([[2**32 - 1], [2]], np.uint32))  # 1 modulo 2^32
    assert sref.trips(wrapping).tolist() == [65535]
    per_term = np.minimum(many["trips"], 65535).astype(np.uint32).sum(axis=0, dtype=np.uint32)  # clamping each term first stays in 32 bits ...
    assert np.minimum(per_term, 65535).tolist() == [65535, 9]  # ... and gives the same value


def test_cut_against_fractions():
    rng = np.random.default_rng(11)
    for _ in range(2000):
        n_slices = int(rng.integers(1, 6))
        final, escaped, exhausted, outside = (rng.integers(0, 5, (n_slices, 1)) * (rng.random((n_slices, 1)) < 0.7) for _ in range(4))
        got = int(sref.cut(ref.records(np.zeros((n_slices, 1), np.float32), 0, final, escaped, exhausted, outside))[0])
        e, p = int(exhausted.sum()), int((final + escaped + exhausted).sum())
        if p == 0:
            assert got == 0
            continue
        share = Fraction(65535 * e, p)
        assert got - 1 < share <= got and (got == 0) == (e == 0) and (got == 65535) == (e == p)
    assert sref.cut_sample(0, 7) == 0 and sref.cut_sample(7, 7) == 65535 and sref.cut_sample(0, 0) == 0
    assert sref.cut_sample(1, 3 * 65535 * 256) == 1 and sref.cut_sample(3 * 65535 * 256 - 1, 3 * 65535 * 256) == 65535
    # ... and through records: 256 slices of saturated counts, one exhausted path among them; outside samples do not count
    final = np.full((256, 2), 65535)
    exhausted = np.full((256, 2), 65535)
    exhausted[1:, 0] = 0
    exhausted[0, 0] = 1
    big = ref.records(np.zeros((256, 2), np.float32), 0, final, 65535, exhausted, 65535)
    assert sref.cut(big).tolist() == [1, 21845]
    assert sref.cut(ref.records(np.zeros((1, 1), np.float32), 0, 0, 0, 0, 4)).tolist() == [0]


# ---- the library ------------------------------------------------------------------------------
def test_entry_point_refuses_before_any_gpu_call(pa):
    fn = pa.lib().ptl_pass_slices_to_gray16
    vp = C.c_void_p
    rec, out = 0x10000, 0x20000  # never read: every case is refused on its arguments alone

    def call(records=rec, n_slices=2, slice_records=100, n=100, depth=out, trips=None, cut=None, device=-1):
        return fn(device, vp(records), n_slices, slice_records, n, vp(depth), vp(trips), vp(cut), 0.0, 1.0, None, None)

    bad = {
        "null records": dict(records=None),
        "no output": dict(depth=None),
        "misaligned records": dict(records=rec + 8),
        "misaligned depth": dict(depth=out + 2),
        "misaligned trips": dict(trips=out + 4),
        "misaligned cut": dict(cut=out + 8),
        "no slice": dict(n_slices=0),
        "257 slices": dict(n_slices=257),
        "no pixel": dict(n=0),
        "negative n": dict(n=-4),
        "n beyond 2^31": dict(n=2**31 + 1, slice_records=2**32),
        "slices overlap": dict(slice_records=99),
    }
    for what, arguments in bad.items():
        assert call(**arguments) == -1, what  # PTL_ERR_INVALID
        assert "pass_slices_to_gray16" in pa.last_error(), what
    # what is allowed gets as far as the device, and there is none with this number
    for arguments in (dict(), dict(n_slices=1, slice_records=0), dict(n_slices=256), dict(n=2**31, slice_records=2**31), dict(depth=None, cut=out)):
        assert call(**arguments) == -6, arguments  # PTL_ERR_NO_DEVICE
    with pytest.raises(pa.PortalError):
        pa.pass_slices_to_gray16_device(rec, 2, 99, 100, out_depth_ptr=out, device=-1)


REFUSED = [
    ("render-frame", ["--clip-passes", "depth"], "--clip-passes is an option of render"),
    ("precompile", ["--clip-passes", "depth"], "--clip-passes is an option of render"),
    ("check", ["--clip-passes", "cut"], "--clip-passes is an option of render"),
    ("render", ["--clip-passes", ""], "name at least one pass"),
    ("render", ["--clip-passes", " , "], "name at least one pass"),
    ("render", ["--clip-passes", "depth,normals"], "unknown pass `normals`"),
    ("render", ["--clip-passes", "cut", "--clip-adaptive-aa"], "--clip-adaptive-aa"),
    ("render", ["--clip-passes", "cut", "--adaptive-aa"], "--adaptive-aa"),
    ("render", ["--clip-passes", "trips", "--gpus", "2"], "one GPU"),
    ("render", ["--clip-passes", "trips", "--devices", "0,1"], "one GPU"),
    ("render", ["--passes", "cut"], "--passes is an option of render-frame"),
    ("render-frame", ["--passes", "cut,normals"], "unknown pass `normals`"),
    ("render", ["--pass-encoder", "gpu"], "--pass-encoder needs --clip-passes"),
    ("render", ["--pass-encoder", "host"], "--pass-encoder needs --clip-passes"),
    ("render-frame", ["--passes", "cut", "--pass-encoder", "gpu"], "--pass-encoder needs --clip-passes"),
    ("render", ["--clip-passes", "cut", "--pass-encoder", "zlib"], "--pass-encoder host|gpu"),
    ("render", ["--clip-passes", "cut", "--pass-encoder", "gpu", "--width", "64", "--height", "36"], "multiple of 3"),
    ("render", ["--clip-passes", "cut", "--pass-encoder", "gpu", "--width", "34", "--height", "36", "--stereoimage"], "multiple of 3"),
    ("render", ["--clip-passes", "cut", "--pass-encoder", "gpu", "--width", "30000", "--height", "40000"], "2^31 bytes of scanlines"),
]


@pytest.mark.parametrize("command,arguments,reason", REFUSED)
def test_cli_refuses_while_parsing(pa, tmp_path, command, arguments, reason):
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run([exe, command, pa.scene_path("portal_in_portal"), "--out-dir", str(tmp_path), "--output", str(tmp_path / "f.png")] + arguments, capture_output=True, text=True,
                         timeout=120, cwd=str(tmp_path))
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1, out.stderr
    assert os.listdir(tmp_path) == []


def test_usage_names_the_option(pa):
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and out.stderr.count("--clip-passes depth,trips,cut") == 1 and "--passes depth,trips,cut" in out.stderr
    assert "anim/cut_<i>.png" in out.stderr and "<output stem>.cut.png" in out.stderr and out.stderr.count("--pass-encoder host|gpu") == 1


def test_kernel_cross_compiles_without_scratch_or_lds(tmp_path):
    """The new kernel with the Makefile's flags for gfx950: 0 bytes of scratch, 0 of LDS, no spills; no inline assembly; the Makefile builds it."""
    import re

    usage = _compile_with_usage("pass_slices_gray16", tmp_path)
    assert set(usage) == {"ptl_pass_slices_to_gray16_kernel"}
    u = usage["ptl_pass_slices_to_gray16_kernel"]
    assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, u
    assert 0 < u["VGPRs"] <= 128, u  # four waves per SIMD at least
    print("VGPRs:", u["VGPRs"])
    source = open(os.path.join(ROOT, "portal_amd", "csrc", "kernels", "pass_slices_gray16.hip")).read()
    assert "asm" not in source and "atomic" not in source.replace("no atomics", "") and "__shared__" not in source
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert "portal_amd/kernels/pass_slices_gray16.hsaco" in re.search(r"^KERNELS\s*:=(.*)$", makefile, re.M).group(1)


# ---- pass frames through the 16-bit GPU encoder: the writer --------------------------------------
def grey_case(w, h, seed):
    """(H, W) uint16 with what pass images hold: a smooth ramp, flat stretches, a few steps and some noise."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    a = (x * 257 + y * 1021) % 65536
    a = np.where(rng.random((h, w)) < 0.3, 40000, a)
    a = np.where(rng.random((h, w)) < 0.1, rng.integers(0, 65536, (h, w)), a)
    return a.astype(np.uint16)


@functools.lru_cache(maxsize=None)
def grey_result(w, h):
    """-> (image, the result buffer the reference makes of its rows taken as W / 3 RGB pixels)"""
    from tests import png16_deflate_reference as r6

    a = grey_case(w, h, 100 * w + h)
    raw = r6.raw16(a.reshape(h, w // 3, 3))
    assert len(raw) == h * (2 * w + 1)  # the grey image's own scanlines: the filter-type bytes sit where a grey reader expects them
    return a, r6.result(raw, w // 3, h)


@pytest.mark.parametrize("w,h", [(3, 1), (9, 5), (96, 40), (1536, 3)])
def test_stream_writer_frames_a_grey_file(pa, tmp_path, w, h):
    from PIL import Image

    a, result = grey_result(w, h)
    path = str(tmp_path / "grey.png")
    pa.png_write_stream_gray16(path, result, w, h)
    assert np.array_equal(sref.read_png_gray16_up(path), a)
    with Image.open(path) as image:
        assert image.size == (w, h) and image.mode in ("I;16", "I;16B", "I")
        assert np.array_equal(np.asarray(image).astype(np.uint16), a)


def test_stream_writer_refuses(pa, tmp_path):
    import struct

    a, good = grey_result(9, 5)
    fn = pa.lib().ptl_png_write_stream_gray16
    buffer = lambda data: np.frombuffer(data, np.uint8).copy()  # noqa: E731
    with_word = lambda k, v: good[: 4 * k] + struct.pack("<I", v) + good[4 * k + 4:]  # noqa: E731
    cases = {"width 10": (good, 10, 5), "width 8": (good, 8, 5), "another height": (good, 9, 6), "another width": (good, 12, 5), "PTLZ": (with_word(0, struct.unpack("<I", b"PTLZ")[0]), 9, 5),
             "a header for 4 x 5": (with_word(1, 4), 9, 5), "no stream": (with_word(3, 0), 9, 5), "a stream beyond the room": (with_word(3, 0xFFFFFFF0), 9, 5)}
    for what, (data, w, h) in cases.items():
        b = buffer(data)
        assert fn(str(tmp_path / "no.png").encode(), b.ctypes.data, w, h) == -1, what
    assert fn(None, buffer(good).ctypes.data, 9, 5) == -1 and fn(str(tmp_path / "no.png").encode(), None, 9, 5) == -1
    assert os.listdir(tmp_path) == []
    with pytest.raises(pa.PortalError):
        pa.png_write_stream_gray16(str(tmp_path / "no.png"), good[:80], 9, 5)
    pa.png_write_stream_rgb48(str(tmp_path / "rgb.png"), good, 3, 5)  # the same buffer IS a 3 x 5 RGB frame's
    assert os.listdir(tmp_path) == ["rgb.png"]


SANITIZED_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "include/portal_amd.h"
namespace ptl { void set_last_error(const std::string& msg) { std::fprintf(stderr, "%s\n", msg.c_str()); } }
static std::vector<uint8_t> read_file(const std::string& path) {
    std::vector<uint8_t> data;
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) return data;
    uint8_t buf[4096];
    size_t n;
    while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) data.insert(data.end(), buf, buf + n);
    std::fclose(f);
    return data;
}
int main(int argc, char** argv) {
    // argv[1]: a result buffer of exactly header + stream bytes (a heap block of that size: one byte read behind it is reported); argv[2], argv[3]: W, H
    const std::vector<uint8_t> file = read_file(argv[1]);
    const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
    if (file.size() < 64) return 1;
    std::vector<uint8_t> exact(file.begin(), file.end());
    exact.shrink_to_fit();
    const std::string out = std::string(argv[4]) + "/ok.png";
    if (ptl_png_write_stream_gray16(out.c_str(), exact.data(), w, h) != PTL_OK) return 2;
    // corrupted headers, each a block of 64 bytes only: the writer refuses on the header alone and never reads a stream
    const uint32_t beyond = 0xfffffff0u, magic = 0x5a4c5450u, width = (uint32_t)w / 3u + 1u, none = 0u;
    const struct { size_t at; const uint32_t* value; } bad[4] = {{0, &magic}, {4, &width}, {12, &beyond}, {12, &none}};
    for (int k = 0; k < 4; ++k) {
        std::vector<uint8_t> header(file.begin(), file.begin() + 64);
        header.shrink_to_fit();
        std::memcpy(header.data() + bad[k].at, bad[k].value, 4);
        const std::string no = std::string(argv[4]) + "/no" + std::to_string(k) + ".png";
        if (ptl_png_write_stream_gray16(no.c_str(), header.data(), w, h) != PTL_ERR_INVALID) return 4 + k;
        if (FILE* f = std::fopen(no.c_str(), "rb")) { std::fclose(f); return 8; }
    }
    if (ptl_png_write_stream_gray16(nullptr, nullptr, 3, 1) != PTL_ERR_INVALID) return 9;
    if (ptl_png_write_stream_gray16(out.c_str(), exact.data(), w + 1, h) != PTL_ERR_INVALID) return 10;  // not a multiple of 3: refused before the header is read
    std::puts("sanitized grey stream writer ok");
    return 0;
}
"""


def test_stream_writer_under_sanitizers(tmp_path):
    """ptl_png_write_stream_gray16 in a stand-alone program compiled with png_io.cpp under AddressSanitizer and UndefinedBehaviorSanitizer, run as a
    plain child process: valid buffers of exactly header + stream bytes, and corrupted headers of exactly 64 bytes.  The sanitizer runtimes are
    linked statically and the child inherits the environment untouched.  Nothing is loaded into Python under a sanitizer."""
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "sanitized_grey_stream_writer"
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                            str(tmp_path / "main.cpp"), os.path.join(ROOT, "portal_amd", "csrc", "host", "png_io.cpp"), "-lz", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    files = tmp_path / "files"
    files.mkdir()
    for k, (w, h) in enumerate([(9, 5), (96, 40)]):
        a, result = grey_result(w, h)
        (tmp_path / f"result{k}.bin").write_bytes(result)
        run = subprocess.run([str(exe), str(tmp_path / f"result{k}.bin"), str(w), str(h), str(files)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "sanitized grey stream writer ok" in run.stdout, (run.returncode, run.stderr)
        assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
        assert os.listdir(files) == ["ok.png"]
        assert np.array_equal(sref.read_png_gray16_up(str(files / "ok.png")), a)
