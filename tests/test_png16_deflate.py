"""GPU deflate of 16-bit PNG frames (`--png-depth 16 --png16-encoder gpu`), the part that needs no GPU: the restatement of
the contract (tests/png16_deflate_reference.py) against zlib's inflater, the token rule at distance 6, the bounds, the sizes the format
reaches, the host's writer on reference-made buffers (also in a stand-alone program under sanitizers), the refusals of the writer, of the
entry point and of the CLI, and the cross-compile of the kernel file."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import png16_deflate_cases as cs
from tests import png16_deflate_reference as r6
from tests import png16_reference as p16
from tests import png_deflate_reference as pr
from tests import png_huffman_reference as hr
from tests import yuv_deep_reference as dr
from tests.yuv_harness import ROOT, _once

CASES = {"1x1": lambda: cs.noise(1, 1), "2x1": lambda: cs.noise(2, 1), "h=1": lambda: cs.noise(33, 1), "w=1": lambda: cs.noise(1, 9), "w=3": lambda: cs.noise(3, 4),
         "w=5": lambda: cs.noise(5, 70), "w=17": lambda: cs.noise(17, 300), "64x64": lambda: cs.noise(64, 64), "one colour": lambda: cs.one_colour(256, 64),
         "noise": lambda: cs.noise(256, 64), "mixed": lambda: cs.mixed(683, 3), "every literal": cs.every_literal, "covered stretches": cs.covered_stretches,
         "across a segment boundary": cs.across_a_segment_boundary, "distance 1 but not 6": cs.distance_one_not_six, "fibonacci": cs.fibonacci,
         "costly last segment": cs.costly_last_segment, "both choices": cs.both_choices, "period 6 rows": lambda: cs.period_six_rows(37, 9),
         "sample steps": lambda: cs.period_six_rows(37, 9, carry=True)}


def _encoded(case):
    """(A, raw16, bands) of a case, computed once."""
    def make():
        a = CASES[case]()
        h, w = a.shape[:2]
        raw = r6.raw16(a)
        return a, raw, r6.encode_bands(raw, w, h)

    return _once(("png16 deflate cpu", case), make)


@pytest.mark.parametrize("case", list(CASES))
def test_reference_streams_inflate_to_the_raw_scanlines(case):
    """zlib.decompress of 78 01 | stream | 03 00 | Adler-32 returns raw16, whole and band by band, in both code modes (the losing dynamic
    block as well); the plain-Python and the numpy tokeniser agree; the two forms of the builder give the same bytes; no band exceeds its
    bound, and every dynamic band is at most its fixed band."""
    a, raw, bands = _encoded(case)
    h, w = a.shape[:2]
    assert len(raw) == h * (6 * w + 1) and np.array_equal(r6.a_of_rows(r6.rows_of_raw16(raw, w, h)), a)
    for fixed in (False, True):
        result = r6.result(raw, w, h, bands, fixed=fixed)
        assert r6.inflate(result) == raw
        p = r6.parse(result)
        assert (p["w"], p["h"], p["rows"], p["bands"], p["adler"]) == (w, h, r6.band_rows(w), r6.band_count(w, h), zlib.adler32(raw))
        assert len(p["stream"]) <= r6.stream_capacity(w, h)
    assert len(bands) == r6.band_count(w, h)
    for band, info in zip(r6.cut_bands(raw, w, h), bands):
        for key in ("data", "dynamic_data", "fixed_data"):
            d = zlib.decompressobj(-15)
            assert d.decompress(info[key] + b"\x03\x00") == band and d.eof, key
        assert (r6.band_histogram(band, r6.segment_symbols_plain) == info["hist"]).all()
        for segment in r6.cut_segments(band):
            numpy_form = r6.segment_symbols(segment)
            assert r6.segment_symbols_plain(segment) == list(zip(*(x.tolist() for x in numpy_form)))
            assert [k for k, _ in r6.segment_tokens_plain(segment)[:6]] == ["lit"] * min(6, len(segment))  # no match reaches before its segment
        assert len(info["data"]) <= len(info["fixed_data"]) <= r6.band_capacity(len(band))
        assert info["dynamic"] == (info["dynamic_bits"] < info["fixed_bits"])
        assert info["data"] == (info["dynamic_data"] if info["dynamic"] else info["fixed_data"])
        assert hr.code_lengths_plain(info["hist"])[0] == info["lengths"].tolist()
    plain = r6.encode_band(r6.cut_bands(raw, w, h)[0], builder=hr.code_lengths_plain)
    assert plain["data"] == bands[0]["data"]


def test_the_token_rule_at_distance_six():
    pixel = bytes([1, 2, 3, 4, 5, 6])
    for m, want in ((0, []), (2, []), (3, [3]), (258, [258]), (259, [258]), (260, [258]), (261, [258, 3]), (516, [258, 258]), (519, [258, 258, 3])):
        segment = (pixel * 100)[: 6 + m]
        tokens = r6.segment_tokens_plain(segment)
        assert tokens[:6] == [("lit", v) for v in pixel] and [x for kind, x in tokens if kind == "match"] == want, (m, tokens)
        assert sum(x if kind == "match" else 1 for kind, x in tokens) == len(segment)
        assert [t for t in tokens[6:] if t[0] == "lit"] == [("lit", segment[k]) for k in range(6 + sum(want), len(segment))]  # the remaining bytes, as they are
    # equal at distance 1 but not at 6: nothing to match; equal at 6 and not at 1: matches
    assert all(kind == "lit" for kind, _ in r6.segment_tokens_plain(bytes([7] * 5 + [8] * 5 + [9] * 5)))
    assert r6.segment_tokens_plain(bytes([7] * 12)) == [("lit", 7)] * 6 + [("match", 6)]
    assert r6.FIXED_DISTANCE == (0b100100, 6) and r6.DYNAMIC_DISTANCE == (0b10, 2) and r6.MAGIC == struct.unpack("<I", b"PTL6")[0]
    # the bits of one fixed match of 3 at distance 6: length code 257 (0000001), then 00100 and the extra bit 1
    info = r6.encode_band(bytes([0]) + pixel + pixel[:3])
    bits = np.unpackbits(np.frombuffer(info["fixed_data"], np.uint8), bitorder="little")
    assert bits[3 + 7 * 8: 3 + 7 * 8 + 13].tolist() == [0, 0, 0, 0, 0, 0, 1] + [0, 0, 1, 0, 0] + [1]


def test_both_choices_the_length_limit_and_a_costly_segment():
    assert [b["dynamic"] for b in _encoded("both choices")[2]] == [True, False]
    assert [b["dynamic"] for b in _encoded("1x1")[2]] == [False] and all(b["dynamic"] for b in _encoded("one colour")[2])
    a, raw, bands = _encoded("fibonacci")
    assert a.shape == (1, 1127, 3) and len(bands) == 1 and bands[0]["dynamic"]
    assert hr.code_lengths_plain(bands[0]["hist"])[1] == 17 and int(bands[0]["lengths"].max()) == 15
    a, raw, bands = _encoded("costly last segment")
    assert len(bands) == 1 and bands[0]["dynamic"] and [len(s) for s in r6.cut_segments(raw)] == [4096, 4096, 4096, 4093]
    assert bands[0]["segment_bits"][3] > 9 * 4093 and max(bands[0]["segment_bits"][:3]) < 3 * 4096
    a, raw, bands = _encoded("covered stretches")
    found = {x for s in r6.cut_segments(raw) for kind, x in r6.segment_tokens_plain(s) if kind == "match"}
    assert set(range(3, 21)) | {257, 258} <= found
    a, raw, bands = _encoded("period 6 rows")
    lines = np.frombuffer(raw, np.uint8).reshape(9, -1)
    assert (lines[1:, 7:] == lines[1:, 1:-6]).all() and len(r6.result(raw, 37, 9)) < len(raw) // 2


def test_the_dynamic_header_says_hdist_4():
    """An inflater's reading of a dynamic header: HDIST = 4, the distance lengths 0 0 0 0 1 behind the literal/length lengths."""
    for case in ("one colour", "noise", "fibonacci"):
        for info in _encoded(case)[2]:
            bits = np.unpackbits(np.frombuffer(info["dynamic_data"][:4], np.uint8), bitorder="little")
            value = lambda at, n: int(sum(int(b) << k for k, b in enumerate(bits[at: at + n])))  # noqa: E731
            assert (value(0, 1), value(1, 2), value(8, 5), value(13, 4)) == (0, 2, 4, 15)
            n_lit = value(3, 5) + 257
            assert n_lit == max(s for s, n in enumerate(info["lengths"]) if n) + 1


def test_sizes_the_format_reaches(pa):
    """The host-build float frame of scenes/portal_in_portal.ron at 640x360, depth 40, through encode16.  Caps that catch a parse or a builder
    that stopped working, chosen so that the reference alone holds them; the measured values are printed beside them (the reference's
    stream is 419 542 bytes, 90 of 90 bands dynamic, the longest code 13 bits)."""
    from oracle import host_build

    scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
    r = pa.SceneRenderer(scene, device=-1, flags=0)
    r.set_option("render_depth", 40)
    w, h = 640, 360
    a = dr.encode16([np.array(host_build.host_kernel_for(r, scene, w, h).render(w, h)["rgba32f"])])
    assert len(np.unique(a.reshape(-1, 3), axis=0)) > 1000  # a rendered frame, not a blank one
    raw = r6.raw16(a)
    bands = r6.encode_bands(raw, w, h)
    body = b"".join(b["data"] for b in bands)
    assert r6.inflate(r6.result(raw, w, h, bands)) == raw
    sub = np.concatenate([np.full((h, 1), 1, np.uint8), np.frombuffer(p16.rows_from_a(a, p16.FILTER_SUB), np.uint8).reshape(h, 6 * w)], axis=1).tobytes()  # what Png16Output deflates
    level3_sub, level3_up = len(zlib.compress(sub, 3)), len(zlib.compress(raw, 3))
    at_one = sum(len(b["data"]) for b in r6.encode_bands(raw, w, h, distance=1))
    print(f"portal_in_portal 640x360 d40, 16 bit: raw {len(raw)}, stream {len(body)} = {100 * len(body) / len(raw):.1f} % of raw; zlib level 3 of the Sub scanlines {level3_sub}, of the same Up scanlines {level3_up}; the same bands at distance 1 {at_one}")
    print(f"  = {len(body) / level3_sub:.3f} x level 3 Sub, {len(body) / level3_up:.3f} x level 3 Up, {len(body) / at_one:.3f} x distance 1; {sum(b['dynamic'] for b in bands)} of {len(bands)} bands dynamic, longest code {max(int(b['lengths'].max()) for b in bands)}")
    assert len(body) <= 1.25 * level3_sub
    assert len(body) <= 1.5 * level3_up
    assert len(body) <= 0.35 * len(raw)
    assert len(body) <= 0.75 * at_one


def _chunks(data):
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    at, out = 8, []
    while at < len(data):
        n = struct.unpack(">I", data[at: at + 4])[0]
        kind, body, crc = data[at + 4: at + 8], data[at + 8: at + 8 + n], struct.unpack(">I", data[at + 8 + n: at + 12 + n])[0]
        assert zlib.crc32(kind + body) == crc, kind
        out.append((kind, body))
        at += 12 + n
    assert at == len(data)
    return out


@pytest.mark.parametrize("case", ["1x1", "w=5", "one colour", "noise", "covered stretches", "fibonacci", "period 6 rows"])
def test_png_write_stream_rgb48_files_open_to_the_frame(pa, tmp_path, case):
    """Reference-made buffers through the writer, both code modes: the reader for rows of filter type 0 / 2 returns A; ptl_png_read returns
    the high bytes; ONE IDAT = 78 01 | stream | 03 00 | Adler-32; every CRC is right; IHDR says 16 bits, colour type 2."""
    a, raw, bands = _encoded(case)
    h, w = a.shape[:2]
    for fixed in (False, True):
        result = r6.result(raw, w, h, bands, fixed=fixed)
        path = str(tmp_path / f"f{int(fixed)}.png")
        pa.png_write_stream_rgb48(path, result + bytes(11), w, h)
        image, said = r6.read_png16_up(path, header=True)
        assert np.array_equal(image, a) and (said["filter_types"][1:] == 2).all() and said["filter_types"][0] == 0
        eight = pa.png_read(path)
        assert eight.shape == (h, w, 4) and np.array_equal(eight[..., :3], a >> 8) and (eight[..., 3] == 255).all()
        chunks = _chunks(open(path, "rb").read())
        assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
        assert chunks[0][1] == struct.pack(">II", w, h) + bytes([16, 2, 0, 0, 0])
        p = r6.parse(result)
        assert chunks[1][1] == pr.zlib_stream(p["stream"], p["adler"])
    assert 64 + r6.stream_capacity(w, h) <= pa.png_stream16_download_bytes(w, h) == r6.download_bytes(w, h) < pa.png_stream16_bytes(w, h) == r6.result_bytes(w, h)
    assert pa.png_stream16_band_rows(w) == r6.band_rows(w)


def test_the_writer_refuses(pa, tmp_path):
    """A header that does not match -- the magic word (an 8-bit "PTLZ" buffer included), W, H, the band cut, a byte count beyond the room or
    below six bytes a band -- null pointers, sizes that are not positive: PTL_ERR_INVALID, and nothing is written.  The 8-bit writer refuses
    this format's buffers as well."""
    a, raw, bands = _encoded("w=5")
    h, w = a.shape[:2]
    good = r6.result(raw, w, h, bands)
    f = pa.lib().ptl_png_write_stream_rgb48
    path = str(tmp_path / "no.png").encode()

    def with_word(k, value):
        return good[: 4 * k] + struct.pack("<I", value) + good[4 * k + 4:]

    eight = pr.result(np.zeros((h, w, 4), np.uint8))
    bad = [with_word(0, pr.MAGIC), with_word(0, 0), with_word(1, w + 1), with_word(2, h + 1), with_word(5, r6.band_rows(w) + 1), with_word(6, r6.band_count(w, h) + 1),
           with_word(3, r6.stream_capacity(w, h) + 1), with_word(3, 0xfffffff0), with_word(3, 6 * r6.band_count(w, h) - 1), eight + bytes(len(good))]
    for k, buffer in enumerate(bad):
        array = np.frombuffer(buffer, np.uint8)
        assert f(path, array.ctypes.data, w, h) == -1, k
        assert "header" in pa.lib().ptl_last_error().decode()
    array = np.frombuffer(good, np.uint8)
    assert f(None, array.ctypes.data, w, h) == -1 and f(path, None, w, h) == -1
    assert f(path, array.ctypes.data, 0, h) == -1 and f(path, array.ctypes.data, w, -1) == -1 and f(path, array.ctypes.data, h, w) == -1
    assert f(path, array.ctypes.data, 1 << 15, 1 << 15) == -1
    assert pa.lib().ptl_png_write_stream(path, array.ctypes.data, w, h) == -1  # neither writer takes the other's buffer
    with pytest.raises(pa.PortalError):
        pa.png_write_stream_rgb48(str(tmp_path / "no.png"), good[:70], w, h)
    assert not os.listdir(tmp_path)
    assert f(path, array.ctypes.data, w, h) == 0 and os.listdir(tmp_path) == ["no.png"]


def test_entry_point_refuses_before_any_gpu_call(pa):
    """Any `codes` but 0 and 1 -> PTL_ERR_INVALID whatever else is passed; null or misaligned pointers, sizes <= 0, W H > 2^28,
    H (6 W + 1) > 2^31; the device is looked at last.  The size functions are 0 for such sizes.  The mirror passes everything on."""
    f = pa.lib().ptl_png_deflate_rgb48
    rows, out = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    for codes in (2, -1, 7, 1 << 20):
        assert f(0, rows, 4, 4, codes, out, None, None) == -1 and "PTL_PNG_CODES" in pa.lib().ptl_last_error().decode()
        assert f(-1, None, 0, 0, codes, None, None, None) == -1
    for codes in (0, 1):
        assert f(0, None, 4, 4, codes, out, None, None) == -1 and f(0, rows, 4, 4, codes, None, None, None) == -1
        assert f(0, rows, 0, 4, codes, out, None, None) == -1 and f(0, rows, 4, -4, codes, out, None, None) == -1
        assert f(0, C.c_void_p((1 << 20) + 8), 4, 4, codes, out, None, None) == -1 and f(0, rows, 4, 4, codes, C.c_void_p((1 << 24) + 4), None, None) == -1
        assert f(0, rows, (1 << 14) + 1, 1 << 14, codes, out, None, None) == -1 and "2^28" in pa.lib().ptl_last_error().decode()
        assert f(0, rows, 1 << 15, 1 << 15, codes, out, None, None) == -1
        assert f(-1, rows, 4, 4, codes, out, None, None) == -6  # PTL_ERR_NO_DEVICE: checked last
    with pytest.raises(pa.PortalError):
        pa.png_deflate_rgb48_device(1 << 20, 1 << 24, 4, 4, codes=2)
    with pytest.raises(pa.PortalError):
        pa.png_deflate_rgb48_device(0, 1 << 24, 4, 4)
    for w, h in ((0, 4), (4, -1), ((1 << 14) + 1, 1 << 14), (1 << 15, 1 << 15)):
        assert pa.png_stream16_bytes(w, h) == 0 and pa.png_stream16_download_bytes(w, h) == 0
    assert pa.png_stream16_band_rows(0) == 0 and pa.png_stream16_band_rows(3840) == 1 and pa.png_stream16_band_rows(640) == 4
    for w, h in ((1 << 14, 1 << 14), (1, 1 << 28), (3840, 2160), (1, 1)):
        assert pa.png_stream16_bytes(w, h) == r6.result_bytes(w, h) and h * (6 * w + 1) <= pr.MAX_RAW
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    for words in ("int ptl_png_deflate_rgb48(", "size_t ptl_png_stream16_bytes(", "size_t ptl_png_stream16_download_bytes(", "int ptl_png_stream16_band_rows(",
                  "int ptl_png_write_stream_rgb48(", '"PTL6" (0x364c5450)', "HDIST = 4", "0 0 0 0 1", "floor(16384 / (6 W + 1))", "s[i] == s[i - 6]", "00100"):
        assert words in header, words


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--png-depth", "16", "--png16-encoder", "fast"], "--png16-encoder host|gpu"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "GPU"], "--png16-encoder host|gpu"),
                                              ("render-frame", ["--png16-encoder", "1", "--png-depth", "16"], "--png16-encoder host|gpu"),
                                              ("render", ["--png16-encoder", "gpu"], "--png16-encoder needs --png-depth 16"),
                                              ("render", ["--png16-encoder", "host"], "--png16-encoder needs --png-depth 16"),
                                              ("render-frame", ["--png16-encoder", "gpu", "--png-depth", "8"], "--png16-encoder needs --png-depth 16"),
                                              ("render-frame", ["--png16-encoder", "gpu", "--png-encoder", "gpu"], "--png16-encoder needs --png-depth 16"),
                                              ("render", ["--png16-encoder", "gpu", "--frames", "y4m"], "--png16-encoder needs --png-depth 16"),
                                              ("render", ["--png16-encoder", "gpu", "--png-depth", "16", "--frames", "y4m"], "cannot be combined with --frames y4m"),
                                              ("precompile", ["--png-depth", "16", "--png16-encoder", "gpu"], "is an option of render and render-frame"),
                                              ("check", ["--png16-encoder", "host"], "--png16-encoder is an option of render and render-frame"),
                                              ("emit-source", ["--png16-encoder", "gpu"], "--png16-encoder is an option of render and render-frame"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "gpu", "--gpus", "2"], "one GPU"),
                                              ("render-frame", ["--devices", "0,1", "--png-depth", "16", "--png16-encoder", "gpu"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "gpu", "--multi-process"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "gpu", "--shard", "0/2"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "gpu", "--transport", "rccl"], "one GPU"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "gpu", "--width", "30000", "--height", "30000"], "at most 2^28 pixels"),
                                              # the old spelling stays refused, with its message, with and without the new option
                                              ("render", ["--png-encoder", "gpu", "--png-depth", "16"], "--png-encoder gpu cannot be combined with --png-depth 16"),
                                              ("render-frame", ["--png-depth", "16", "--png16-encoder", "gpu", "--png-encoder", "gpu"], "--png-encoder gpu cannot be combined with --png-depth 16"),
                                              ("render", ["--png-depth", "16", "--png16-encoder", "gpu", "--png-codes", "dynamic"], "--png-codes needs --png-encoder gpu")])
def test_cli_refuses_while_the_arguments_are_parsed(pa, tmp_path, cmd, extra, reason):
    """Exit status 2, one line that says why, nothing rendered or written."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    target = ["anim.4.portals", "--out-dir", str(tmp_path)] if cmd == "render" else ["--output", str(tmp_path / "f.png")] if cmd == "render-frame" else []
    out = subprocess.run([exe, cmd, pa.scene_path("basics")] + target + extra, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


def test_usage_names_the_option_and_its_default(pa):
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and out.stderr.count("--png16-encoder host|gpu") == 2 and out.stderr.count("host (default)") == 2  # render-frame's and render's


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
    if (ptl_png_write_stream_rgb48(out.c_str(), exact.data(), w, h) != PTL_OK) return 2;
    uint8_t* rgba = nullptr;
    int rw = 0, rh = 0;
    if (ptl_png_read(out.c_str(), &rgba, &rw, &rh) != PTL_OK || rw != w || rh != h) return 3;
    std::free(rgba);
    // four corrupted headers, each a block of 64 bytes only: the writer refuses on the header alone and never reads a stream
    const uint32_t beyond = 0xfffffff0u, magic = 0x5a4c5450u, width = (uint32_t)w + 1u, none = 0u;
    const struct { size_t at; const uint32_t* value; } bad[4] = {{0, &magic}, {4, &width}, {12, &beyond}, {12, &none}};
    for (int k = 0; k < 4; ++k) {
        std::vector<uint8_t> header(file.begin(), file.begin() + 64);
        header.shrink_to_fit();
        std::memcpy(header.data() + bad[k].at, bad[k].value, 4);
        const std::string no = std::string(argv[4]) + "/no" + std::to_string(k) + ".png";
        if (ptl_png_write_stream_rgb48(no.c_str(), header.data(), w, h) != PTL_ERR_INVALID) return 4 + k;
        if (FILE* f = std::fopen(no.c_str(), "rb")) { std::fclose(f); return 8; }
    }
    if (ptl_png_write_stream_rgb48(nullptr, nullptr, 1, 1) != PTL_ERR_INVALID) return 9;
    if (ptl_png_write_stream(out.c_str(), exact.data(), w, h) != PTL_ERR_INVALID) return 10;  // the 8-bit writer does not take this buffer
    std::puts("sanitized stream16 writer ok");
    return 0;
}
"""


def test_stream_writer_under_sanitizers(tmp_path):
    """ptl_png_write_stream_rgb48 (and ptl_png_read on its file) in a stand-alone program compiled with png_io.cpp under AddressSanitizer and
    UndefinedBehaviorSanitizer, run as a plain child process: a valid buffer of exactly header + stream bytes, and four corrupted headers
    of exactly 64 bytes.  The sanitizer runtimes are linked statically and the child inherits the environment untouched.  Nothing is loaded
    into Python under a sanitizer."""
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "sanitized_stream16_writer"
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I", ROOT,
                            str(tmp_path / "main.cpp"), os.path.join(ROOT, "portal_amd", "csrc", "host", "png_io.cpp"), "-lz", "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr
    files = tmp_path / "files"
    files.mkdir()
    for k, case in enumerate(("w=17", "one colour", "covered stretches")):
        a, raw, bands = _encoded(case)
        h, w = a.shape[:2]
        (tmp_path / f"result{k}.bin").write_bytes(r6.result(raw, w, h, bands))
        run = subprocess.run([str(exe), str(tmp_path / f"result{k}.bin"), str(w), str(h), str(files)], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and "sanitized stream16 writer ok" in run.stdout, (run.returncode, run.stderr)
        assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
        assert os.listdir(files) == ["ok.png"]
        assert np.array_equal(r6.read_png16_up(str(files / "ok.png")), a)
