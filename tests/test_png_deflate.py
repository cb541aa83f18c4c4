"""GPU deflate of 8-bit PNG frames (`--png-encoder gpu`), the part that needs no GPU: the numpy restatement of the stream
contract (tests/png_deflate_reference.py) against zlib's inflater, the slot bound, what the format is expected to reach in size, the host's
writer (ptl_png_write_stream) on reference-made buffers, the refusals of the entry points and of the CLI, the writer under sanitizers, and the
cross-compile of the kernel file."""
import os
import re
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_deflate_reference as pr
from tests.yuv_harness import HIPCC, ROOT, _compile_with_usage

def _noise(w, h, seed=0):
    return np.random.default_rng(seed + 1000 * w + h).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _one_colour(w, h, v=77):
    """Every byte v: row 0 is not filtered, so only a colour of four equal bytes makes it a run as well."""
    return np.full((h, w, 4), v, np.uint8)


def _directed():
    """One row of raw bytes: runs of 1 .. 20, 257 .. 263 and 515 .. 521 of 0, 143, 144 and 255 with a 77 between them, wherever they fall
    relative to the segment boundaries."""
    body = [77]
    for v in (0, 143, 144, 255):
        for n in list(range(1, 21)) + list(range(257, 264)) + list(range(515, 522)):
            body += [v] * n + [77]
    body += [5] * (-len(body) % 4)
    return np.array(body, np.uint8).reshape(1, -1, 4)


CASES = {"1x1": lambda: _noise(1, 1), "h=1": lambda: _noise(33, 1), "w=1": lambda: _noise(1, 9), "w=3": lambda: _noise(3, 4), "w=5": lambda: _noise(5, 70),
         "w=17": lambda: _noise(17, 300), "one colour": lambda: _one_colour(256, 64), "noise": lambda: _noise(256, 64), "directed runs": _directed}


@pytest.mark.parametrize("case", list(CASES))
def test_reference_streams_inflate_to_the_raw_scanlines(case):
    """zlib.decompress of 78 01 | stream | 03 00 | Adler-32 returns raw (zlib checks the Adler-32 itself); the numpy tokeniser agrees with the
    token rule written out in plain Python; the header says what the frame is."""
    frame = CASES[case]()
    h, w = frame.shape[:2]
    raw = pr.raw_scanlines(frame)
    result = pr.result(frame)
    assert len(raw) == h * (4 * w + 1) and np.array_equal(pr.undo_up(raw, w, h), frame)
    assert pr.inflate(result) == raw
    p = pr.parse(result)
    assert (p["w"], p["h"], p["rows"], p["bands"], p["adler"]) == (w, h, pr.band_rows(w), pr.band_count(w, h), zlib.adler32(raw))
    assert zlib.decompress(pr.zlib_stream(p["stream"], p["adler"])) == raw
    plain = b"".join(pr.deflate_band(b, tokens=lambda s: pr.tokens_to_bits(pr.segment_tokens_plain(s))) for b in pr.cut_bands(raw, w, h))
    assert plain == p["stream"]
    for band in pr.cut_bands(raw, w, h):  # every band on its own is a whole number of bytes that an inflater reads as two blocks
        d = zlib.decompressobj(-15)
        assert d.decompress(pr.deflate_band(band) + b"\x03\x00") == band and d.eof


def test_the_token_rule_on_runs_around_the_258_cap():
    for n, want in ((1, []), (3, []), (4, [3]), (259, [258]), (260, [258]), (261, [258]), (262, [258, 3]), (517, [258, 258]), (520, [258, 258, 3])):
        tokens = pr.segment_tokens_plain(bytes([9]) * n)
        assert tokens[0] == ("lit", 9) and [x for kind, x in tokens if kind == "match"] == want, (n, tokens)
        assert 1 + sum(want) + sum(1 for kind, _ in tokens[1:] if kind == "lit") == n
    assert pr.literal_bits(0) == (0b00001100, 8) and pr.literal_bits(143)[1] == 8 and pr.literal_bits(144) == (0b000010011, 9) and pr.literal_bits(255) == (0b111111111, 9)
    assert pr.match_bits(3) == (0b1000000, 12) and pr.match_bits(258) == (0b10100011, 13) and pr.match_bits(257)[1] == 18 and pr.match_bits(11)[1] == 13


def test_no_band_exceeds_its_slot():
    """Noise is the worst case (a literal of 8 or 9 bits per byte): every band stays within ceil((9 n + 20) / 8) + 4, and so does a band of
    nothing but 9-bit literals."""
    for w, h in ((256, 64), (1023, 3), (5000, 2), (1, 4000)):
        frame = _noise(w, h, 3)
        bands = pr.cut_bands(pr.raw_scanlines(frame), w, h)
        sizes = [len(s) for s in pr.band_streams(frame)]
        assert len(sizes) == pr.band_count(w, h)
        assert all(n <= pr.band_capacity(len(b)) for n, b in zip(sizes, bands)) and sum(sizes) <= pr.stream_capacity(w, h)
    body = (np.arange(16384) % 2 * 100 + 150).astype(np.uint8)  # 150, 250, 150 ...: no run, nine bits each
    assert len(pr.deflate_band(body.tobytes())) in (pr.band_capacity(body.size) - 1, pr.band_capacity(body.size))


def test_sizes_the_format_reaches(pa):
    """What runs alone carry: a host-build frame of scenes/portal_in_portal.ron at 640x360, depth 40, comes out at most 3x zlib level 3 and at
    most 25 % of raw; 256x64 of one colour at most 1 % of raw.  (Caps that catch a match finder that stops finding, not a ranking.)"""
    from oracle import host_build

    scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
    r = pa.SceneRenderer(scene, device=-1, flags=0)
    r.set_option("render_depth", 40)
    frame = np.array(host_build.host_kernel_for(r, scene, 640, 360).render(640, 360)["rgba8"])
    raw, body = pr.raw_scanlines(frame), pr.stream(frame)
    level3 = len(zlib.compress(raw, 3))
    print(f"portal_in_portal 640x360 d40: raw {len(raw)}, stream {len(body)} = {100 * len(body) / len(raw):.1f} % of raw = {len(body) / level3:.2f} x level 3 ({level3})")
    assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 100  # a rendered frame, not a blank one
    assert len(body) <= 3 * level3 and len(body) <= 0.25 * len(raw)
    flat = _one_colour(256, 64)
    assert len(pr.stream(flat)) <= 0.01 * len(pr.raw_scanlines(flat))


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n = struct.unpack(">I", data[at: at + 4])[0]
        kind, body, crc = data[at + 4: at + 8], data[at + 8: at + 8 + n], struct.unpack(">I", data[at + 8 + n: at + 12 + n])[0]
        assert crc == zlib.crc32(kind + body), kind
        out.append((kind, body))
        at += 12 + n
    return out


@pytest.mark.parametrize("case", ["1x1", "w=5", "one colour", "noise", "directed runs"])
def test_png_write_stream_files_open_to_the_frame(pa, tmp_path, case):
    """Reference-made buffers through the writer: PIL (an independent reader) and ptl_png_read return the input pixels; IHDR says depth 8,
    colour type 6; there is ONE IDAT, 78 01 | stream | 03 00 | Adler-32; every CRC is right."""
    from PIL import Image

    frame = CASES[case]()
    h, w = frame.shape[:2]
    result = pr.result(frame)
    path = str(tmp_path / "f.png")
    pa.png_write_stream(path, result + bytes(11), w, h)  # (what lies behind the stream is not read)
    image = Image.open(path)
    assert image.mode == "RGBA" and image.size == (w, h) and np.array_equal(np.array(image), frame)
    assert np.array_equal(pa.png_read(path), frame)
    chunks = _chunks(open(path, "rb").read())
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">II", w, h) + bytes([8, 6, 0, 0, 0]) and chunks[2][1] == b""
    p = pr.parse(result)
    assert chunks[1][1] == pr.zlib_stream(p["stream"], p["adler"])
    assert pa.png_stream_bytes(w, h) == pr.result_bytes(w, h) >= len(result) and pa.png_stream_band_rows(w) == pr.band_rows(w)


def test_png_write_stream_refuses_a_header_that_does_not_match(pa, tmp_path):
    """A wrong magic word, another size, another band cut, a byte count beyond the room for the stream: PTL_ERR_INVALID, no file."""
    f = pa.lib().ptl_png_write_stream
    w, h = 17, 5
    good = bytearray(pr.result(_noise(w, h)))
    path = str(tmp_path / "no.png").encode()

    def with_word(k, value):
        bad = bytearray(good)
        bad[4 * k: 4 * k + 4] = struct.pack("<I", value)
        return np.frombuffer(bytes(bad), np.uint8)

    n = struct.unpack("<I", good[12:16])[0]
    beyond = pr.stream_capacity(w, h) + 1
    assert pr.HEADER_BYTES + beyond <= pa.png_stream_bytes(w, h)  # (still inside the buffer: the bound is the room for the stream, not the scratch behind it)
    for bad in (with_word(0, pr.MAGIC + 1), with_word(0, 0), with_word(1, w + 1), with_word(2, h - 1), with_word(3, beyond), with_word(3, 0xFFFFFFFF), with_word(3, 0), with_word(5, 2), with_word(6, 7)):
        assert f(path, bad.ctypes.data, w, h) == -1
        assert "header" in pa.lib().ptl_last_error().decode()
    ok = np.frombuffer(bytes(good), np.uint8)
    assert f(path, ok.ctypes.data, h, w) == -1  # the frame's sizes exchanged
    assert f(None, ok.ctypes.data, w, h) == -1 and f(path, None, w, h) == -1
    assert f(path, ok.ctypes.data, 0, h) == -1 and f(path, ok.ctypes.data, w, -1) == -1 and f(path, ok.ctypes.data, 1 << 15, 1 << 15) == -1
    assert not os.listdir(tmp_path)
    with pytest.raises(pa.PortalError):
        pa.png_write_stream(str(tmp_path / "short.png"), bytes(good[: 64 + n - 1]), w, h)  # the mirror knows the buffer's length
    assert not os.listdir(tmp_path)
    assert f(path, ok.ctypes.data, w, h) == 0 and os.listdir(tmp_path) == ["no.png"]


def test_entry_point_refuses_before_any_gpu_call(pa):
    """Null pointers, sizes that are not positive, pointers that are not 16-byte aligned, more scanline bytes than 32-bit offsets reach ->
    PTL_ERR_INVALID with no device needed; the size functions say 0 for the same frames."""
    import ctypes as C

    f = pa.lib().ptl_png_deflate_rgba8
    frame, out = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    assert f(0, None, 4, 4, out, None, None) == -1 and f(0, frame, 4, 4, None, None, None) == -1
    assert f(0, frame, 0, 4, out, None, None) == -1 and f(0, frame, 4, 0, out, None, None) == -1 and f(0, frame, -4, 4, out, None, None) == -1
    assert f(0, C.c_void_p((1 << 20) + 8), 4, 4, out, None, None) == -1 and f(0, frame, 4, 4, C.c_void_p((1 << 24) + 4), None, None) == -1
    for w, h in ((1 << 15, 1 << 15), (1 << 29, 1), (1, 1 << 29), ((1 << 29) - 1, 2)):
        assert h * (4 * w + 1) > pr.MAX_RAW
        assert f(0, frame, w, h, out, None, None) == -1 and "2^31" in pa.lib().ptl_last_error().decode()
        assert pa.png_stream_bytes(w, h) == 0
    assert pa.png_stream_bytes(0, 4) == 0 and pa.png_stream_bytes(4, -1) == 0 and pa.png_stream_band_rows(0) == 0
    w, h = (1 << 29) - 1, 1  # the largest row there is: one band, and the size function still says what the reference says
    assert h * (4 * w + 1) <= pr.MAX_RAW and pa.png_stream_bytes(w, h) == pr.result_bytes(w, h) > 2 * 4 * w
    assert f(-1, frame, 4, 4, out, None, None) == -6  # PTL_ERR_NO_DEVICE: checked last
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    for name in ("size_t ptl_png_stream_bytes(", "int ptl_png_deflate_rgba8(", "int ptl_png_write_stream(", "int ptl_png_stream_band_rows("):
        assert name in header
    for words in ("ceil((9 n + 20) / 8) + 4", "segments of 4096 bytes", "00 00 FF FF", "78 01"):
        assert words in header


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--png-encoder", "fast"], "--png-encoder host|gpu"), ("render-frame", ["--png-encoder", "GPU"], "--png-encoder host|gpu"),
                                              ("render-frame", ["--png-encoder", "1"], "--png-encoder host|gpu"),
                                              ("render", ["--png-encoder", "gpu", "--frames", "y4m"], "cannot be combined with --frames y4m"),
                                              ("render", ["--frames", "y4m", "--png-encoder", "gpu"], "cannot be combined with --frames y4m"),
                                              ("render", ["--png-encoder", "gpu", "--png-depth", "16"], "cannot be combined with --png-depth 16"),
                                              ("render-frame", ["--png-depth", "16", "--png-encoder", "gpu"], "cannot be combined with --png-depth 16"),
                                              ("precompile", ["--png-encoder", "gpu"], "--png-encoder is an option of render and render-frame"),
                                              ("check", ["--png-encoder", "host"], "--png-encoder is an option of render and render-frame"),
                                              ("emit-source", ["--png-encoder", "gpu"], "--png-encoder is an option of render and render-frame"),
                                              ("render-frame", ["--png-encoder", "gpu", "--gpus", "2"], "the one GPU"),
                                              ("render-frame", ["--devices", "0,1", "--png-encoder", "gpu"], "the one GPU"),
                                              ("render-frame", ["--png-encoder", "gpu", "--multi-process"], "the one GPU"),
                                              ("render-frame", ["--png-encoder", "gpu", "--transport", "rccl"], "the one GPU"),
                                              ("render-frame", ["--png-encoder", "gpu", "--shard", "0/2"], "the one GPU"),
                                              ("render-frame", ["--png-encoder", "gpu", "--width", "30000", "--height", "30000"], "at most 2^31"),
                                              ("render", ["--png-encoder", "gpu", "--width", "16000", "--height", "20000", "--stereoimage"], "at most 2^31")])
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
    assert out.returncode == 2 and out.stderr.count("--png-encoder host|gpu") == 2  # render-frame's and render's


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
    if (ptl_png_write_stream(out.c_str(), exact.data(), w, h) != PTL_OK) return 2;
    uint8_t* rgba = nullptr;
    int rw = 0, rh = 0;
    if (ptl_png_read(out.c_str(), &rgba, &rw, &rh) != PTL_OK || rw != w || rh != h) return 3;
    std::free(rgba);
    // three corrupted headers, each a block of 64 bytes only: the writer refuses on the header alone and never reads a stream
    const uint32_t beyond = 0xfffffff0u, magic = 0x12345678u, width = (uint32_t)w + 1u;
    const struct { size_t at; const uint32_t* value; } bad[3] = {{0, &magic}, {4, &width}, {12, &beyond}};
    for (int k = 0; k < 3; ++k) {
        std::vector<uint8_t> header(file.begin(), file.begin() + 64);
        header.shrink_to_fit();
        std::memcpy(header.data() + bad[k].at, bad[k].value, 4);
        const std::string no = std::string(argv[4]) + "/no" + std::to_string(k) + ".png";
        if (ptl_png_write_stream(no.c_str(), header.data(), w, h) != PTL_ERR_INVALID) return 4 + k;
        if (FILE* f = std::fopen(no.c_str(), "rb")) { std::fclose(f); return 8; }
    }
    if (ptl_png_write_stream(nullptr, nullptr, 1, 1) != PTL_ERR_INVALID) return 9;
    std::puts("sanitized stream writer ok");
    return 0;
}
"""


def test_stream_writer_under_sanitizers(tmp_path):
    """ptl_png_write_stream (and ptl_png_read on its file) in a stand-alone program compiled with png_io.cpp under AddressSanitizer and
    UndefinedBehaviorSanitizer, run as a plain child process: a valid buffer of exactly header + stream bytes, and three corrupted headers of
    exactly 64 bytes.  The sanitizer runtimes are linked statically and the child inherits the environment untouched.  Nothing is loaded into
    Python under a sanitizer."""
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "sanitized_stream_writer"
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                            str(tmp_path / "main.cpp"), os.path.join(ROOT, "portal_amd", "csrc", "host", "png_io.cpp"), "-lz", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    files = tmp_path / "files"
    files.mkdir()
    for k, frame in enumerate((_noise(17, 5), _one_colour(64, 36), _directed())):
        h, w = frame.shape[:2]
        (tmp_path / f"result{k}.bin").write_bytes(pr.result(frame))
        run = subprocess.run([str(exe), str(tmp_path / f"result{k}.bin"), str(w), str(h), str(files)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "sanitized stream writer ok" in run.stdout, (run.returncode, run.stderr)
        assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
        assert os.listdir(files) == ["ok.png"]
        from PIL import Image

        assert np.array_equal(np.array(Image.open(files / "ok.png")), frame)


# code object -> its entries; for a bands kernel the place of its LDS figure among the "= N bytes.  No scratch" of the source's header comment
CODE_OBJECTS = {"png_deflate": {"ptl_png_deflate_bands_kernel": 0, "ptl_png_deflate_pack_kernel": None},
                "png_huffman": {"ptl_png_huffman_bands_kernel": 0, "ptl_png_deflate16_bands_kernel": 1}}


@pytest.mark.parametrize("name", list(CODE_OBJECTS))
def test_make_builds_the_code_object_without_scratch(tmp_path, name):
    """`make portal_amd/kernels/<name>.hsaco` in a copy of the tree's Makefile and kernel sources: exactly the entries above compile for gfx950
    with 0 bytes of scratch and no VGPR spills; a bands kernel's LDS is what the source's header comment states, eight workgroups' worth fits a
    compute unit's LDS, and three waves fit a SIMD; the pack kernel keeps eight; no inline assembly; the shared steps come from the one
    common header and the shape from the one shape header, which the host files include as well."""
    import shutil

    from tests.yuv_harness import _resource_usage

    shutil.copy(os.path.join(ROOT, "Makefile"), tmp_path / "Makefile")
    shutil.copytree(os.path.join(ROOT, "portal_amd", "csrc", "kernels"), tmp_path / "portal_amd" / "csrc" / "kernels")
    target = f"portal_amd/kernels/{name}.hsaco"
    out = subprocess.run(["make", target, f"HIPCC={HIPCC} -Rpass-analysis=kernel-resource-usage"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / target) > 1000
    usage = _resource_usage(out.stderr)
    assert set(usage) == set(CODE_OBJECTS[name])
    kernels = os.path.join(ROOT, "portal_amd", "csrc", "kernels")
    source, common = open(os.path.join(kernels, name + ".hip")).read(), open(os.path.join(kernels, "png_deflate_common.h")).read()
    stated = [int(n) for n in re.findall(r"= (\d+) bytes\.  No scratch", source)]
    assert len(stated) == sum(1 for at in CODE_OBJECTS[name].values() if at is not None)
    for entry, at in CODE_OBJECTS[name].items():
        u = usage[entry]
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0, (entry, u)
        if at is None:
            assert u["LDS Size [bytes/block]"] <= min(stated) and u["Occupancy [waves/SIMD]"] == 8, (entry, u)
        else:
            assert u["LDS Size [bytes/block]"] == stated[at] and 8 * stated[at] <= 160 * 1024 and u["Occupancy [waves/SIMD]"] >= 3, (entry, u)
    if name == "png_deflate":
        assert stated[0] <= 10 * 1024 + 512  # "about 10 KB"
    print("VGPRs:", {e: u["VGPRs"] for e, u in sorted(usage.items())}, "LDS:", {e: u["LDS Size [bytes/block]"] for e, u in sorted(usage.items())})
    assert _compile_with_usage(name, tmp_path) == usage  # the harness's own compile line is the Makefile's
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert target in re.search(r"^KERNELS\s*:=(.*)$", makefile, re.M).group(1) and makefile.count("png_deflate_shape.h") == 2 and "png_deflate_common.h" in makefile
    assert "deflate16" not in makefile and sorted(f for f in os.listdir(kernels) if "deflate" in f or "huffman" in f) == ["png_deflate.hip", "png_deflate_common.h", "png_deflate_shape.h", "png_huffman.hip"]
    assert '#include "png_deflate_common.h"' in source and '#include "png_deflate_shape.h"' in common
    for text in (source, common):
        assert "asm" not in text and "atomicAdd(&table" not in text
    assert "atomicOr(&bits[" in common and "ptl_png_or_bits(lds.bits" in common
    if name == "png_huffman":
        assert "atomicAdd(&lds.hist[" in source and "static_assert(kLimit + 5u + F::dynamic_distance_bits <= 24u" in source
    for host in ("postprocess.cpp", "png_io.cpp"):
        assert '#include "../kernels/png_deflate_shape.h"' in open(os.path.join(ROOT, "portal_amd", "csrc", "host", host)).read()
