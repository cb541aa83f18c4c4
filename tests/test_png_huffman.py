"""GPU deflate of 8-bit PNG frames with a Huffman code per band (`--png-codes dynamic`), the part that needs no GPU: the
restatement of the contract (tests/png_huffman_reference.py) against zlib's inflater, the length limit, the invariants against the fixed-code
stream, the sizes the format reaches, the host's writer on reference-made buffers, the refusals of the entry point and of the CLI, and the
cross-compile of the kernel file."""
import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

from tests import png_deflate_reference as pr
from tests import png_huffman_reference as hr
from tests.png_huffman_cases import costly_last_segment_frame, fibonacci_frame
from tests.test_png_deflate import CASES, _chunks
from tests.yuv_harness import ROOT, _once

ALL_CASES = dict(CASES)
ALL_CASES.update({"w=1 column": lambda: np.random.default_rng(19).integers(0, 256, (40, 1, 4), dtype=np.uint8), "64x64": lambda: np.random.default_rng(64).integers(0, 256, (64, 64, 4), dtype=np.uint8),
                  "fibonacci": fibonacci_frame, "costly last segment": costly_last_segment_frame})


def _encoded(case):
    """(frame, bands) of a case, computed once."""
    def make():
        frame = ALL_CASES[case]()
        return frame, hr.encode_bands(frame)

    return _once(("png huffman cpu", case), make)


@pytest.mark.parametrize("case", list(ALL_CASES))
def test_reference_streams_inflate_to_the_raw_scanlines(case):
    """zlib.decompress of 78 01 | stream | 03 00 | Adler-32 returns raw, whole and band by band; the plain-Python and the heap/numpy form of the
    code builder give the same lengths and the same bytes; an inflater's reading of every dynamic header returns the lengths; every band is at
    most its fixed-code band and the stream at most the fixed stream."""
    frame, bands = _encoded(case)
    h, w = frame.shape[:2]
    raw = pr.raw_scanlines(frame)
    result = hr.result(frame, bands)
    assert pr.inflate(result) == raw
    p = pr.parse(result)
    assert (p["w"], p["h"], p["rows"], p["bands"], p["adler"]) == (w, h, pr.band_rows(w), pr.band_count(w, h), zlib.adler32(raw))
    fixed = pr.band_streams(frame)
    assert len(bands) == len(fixed) == pr.band_count(w, h)
    for band, info, old in zip(pr.cut_bands(raw, w, h), bands, fixed):
        d = zlib.decompressobj(-15)
        assert d.decompress(info["data"] + b"\x03\x00") == band and d.eof
        d = zlib.decompressobj(-15)
        assert d.decompress(info["dynamic_data"] + b"\x03\x00") == band and d.eof  # (the dynamic block is a valid one even where it lost)
        plain_lengths, _ = hr.code_lengths_plain(info["hist"])
        assert plain_lengths == info["lengths"].tolist()
        assert (hr.band_histogram(band, hr.segment_symbols_plain) == info["hist"]).all()
        assert len(info["data"]) <= len(old) <= pr.band_capacity(len(band))
        assert info["data"] == (info["dynamic_data"] if info["dynamic_bits"] < info["fixed_bits"] else old)
        read = hr.read_block_header(info["dynamic_data"])
        assert read == info["lengths"][: len(read)].tolist() and not info["lengths"][len(read):].any()
        assert hr.read_block_header(old) is None
    assert len(p["stream"]) <= len(b"".join(fixed))
    plain = hr.encode_band(pr.cut_bands(raw, w, h)[0], builder=hr.code_lengths_plain)
    assert plain["data"] == bands[0]["data"]


def test_both_choices_occur_and_tiny_bands_choose_fixed():
    choices = {case: [b["dynamic"] for b in _encoded(case)[1]] for case in ALL_CASES}
    assert choices["1x1"] == [False] and choices["w=1 column"] == [False] and choices["w=3"] == [False], choices
    assert choices["64x64"] == [True, False]  # 63 rows of noise, then one row of 257 bytes: a header does not pay
    assert all(choices["one colour"]) and all(choices["noise"]) and all(choices["fibonacci"]) and all(choices["costly last segment"])
    assert any(any(c) for c in choices.values()) and any(not all(c) for c in choices.values())
    for case in ALL_CASES:  # a tie goes to fixed: dynamic only where it is strictly smaller
        for b in _encoded(case)[1]:
            assert b["dynamic"] == (b["dynamic_bits"] < b["fixed_bits"])


def test_the_length_limit():
    """1691x1: end-of-block and the literal 0 once, the literals 1 .. 16 F(3) .. F(18) times, never beside themselves.  The unlimited tree -- built here, with heapq, apart
    from the reference -- is deeper than 15; the stream has no length above 15, a complete code, and inflates."""
    import heapq

    frame, bands = _encoded("fibonacci")
    assert frame.shape == (1, 1691, 4) and len(bands) == 1
    raw = pr.raw_scanlines(frame)
    assert len(raw) == 6765 and all(a != b for a, b in zip(raw, raw[1:]))
    counts = np.bincount(np.frombuffer(raw, np.uint8), minlength=256)
    assert sorted(counts[counts > 0].tolist()) == [1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2586]
    heap = [(int(c), 0) for c in counts[counts > 0]] + [(1, 0)]  # (weight, depth of the subtree); end-of-block counts once
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    assert heap[0][1] == 17, heap
    assert hr.code_lengths_plain(bands[0]["hist"])[1] == 17
    lengths = hr.read_block_header(bands[0]["data"])
    assert bands[0]["dynamic"] and max(lengths) == 15 and sum(2.0 ** -n for n in lengths if n) == 1.0
    assert sum(1 for n in lengths if n) == 18
    assert pr.inflate(hr.result(frame, bands)) == raw


def test_a_segment_can_cost_more_than_nine_bits_a_byte():
    frame, bands = _encoded("costly last segment")
    assert len(bands) == 1 and bands[0]["dynamic"] and [len(s) for s in pr.cut_segments(pr.raw_scanlines(frame))] == [4096, 4096, 4096, 4093]
    assert bands[0]["segment_bits"][3] > 9 * 4093 and max(bands[0]["segment_bits"][:3]) < 3 * 4096
    assert int(bands[0]["lengths"].max()) <= 15


def _optimal_header_bits(lengths):
    """The block header's bits were the code-length code built like the first code (limit 7) and HCLEN trimmed, instead of the contract's table."""
    lengths = [int(n) for n in lengths]
    n_lit = max(s for s, n in enumerate(lengths) if n) + 1
    tokens = hr.length_sequence_tokens(lengths[:n_lit] + [1])
    hist = np.bincount([t[0] for t in tokens], minlength=19)
    cl = hr.code_lengths(hist, limit=7) if (hist > 0).sum() > 1 else (hist > 0).astype(np.int64)
    n_cl = max(4, max(k for k, s in enumerate(hr.CL_ORDER) if cl[s]) + 1)
    return 17 + 3 * n_cl + sum(int(cl[s]) + bits for s, _, bits in tokens)


def test_sizes_the_format_reaches(pa):
    """The frame tests/test_png_deflate.py uses: the host build of scenes/portal_in_portal.ron at 640x360, depth 40.  The stream is at most 60 % of
    the fixed-code stream, at most 1.35 x zlib level 3, and at most 1.05 x the per-band sum of zlib's own run-length strategy (raw deflate,
    level 9, Z_RLE, one Z_SYNC_FLUSH per band).  Caps that catch a code builder that stopped building, not a ranking.  Printed beside them:
    what the contract's fixed code-length code costs against one built per band."""
    from oracle import host_build

    scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
    r = pa.SceneRenderer(scene, device=-1, flags=0)
    r.set_option("render_depth", 40)
    frame = np.array(host_build.host_kernel_for(r, scene, 640, 360).render(640, 360)["rgba8"])
    assert len(np.unique(frame.reshape(-1, 4), axis=0)) > 100  # a rendered frame, not a blank one
    raw = pr.raw_scanlines(frame)
    bands = hr.encode_bands(frame)
    body, fixed = b"".join(b["data"] for b in bands), pr.stream(frame)
    assert pr.inflate(hr.result(frame, bands)) == raw
    level3 = len(zlib.compress(raw, 3))
    rle = 0
    for band in pr.cut_bands(raw, 640, 360):
        c = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
        rle += len(c.compress(band) + c.flush(zlib.Z_SYNC_FLUSH))
    table = sum(b["header_bits"] for b in bands)
    optimal = sum(_optimal_header_bits(b["lengths"]) for b in bands)
    print(f"portal_in_portal 640x360 d40: raw {len(raw)}, dynamic stream {len(body)} = {100 * len(body) / len(raw):.2f} % of raw, fixed stream {len(fixed)}, zlib level 3 {level3}, zlib Z_RLE per band {rle}")
    print(f"  = {100 * len(body) / len(fixed):.1f} % of fixed, {len(body) / level3:.3f} x level 3, {len(body) / rle:.4f} x Z_RLE; {sum(b['dynamic'] for b in bands)} of {len(bands)} bands dynamic, longest code {max(int(b['lengths'].max()) for b in bands)}")
    print(f"  block headers: {table / 8 / len(bands):.1f} bytes a band with the contract's code-length code, {optimal / 8 / len(bands):.1f} with one built per band: the table costs {100 * (table - optimal) / 8 / len(body):.2f} % of the stream")
    assert len(body) <= 0.60 * len(fixed)
    assert len(body) <= 1.35 * level3
    assert len(body) <= 1.05 * rle


@pytest.mark.parametrize("case", ["1x1", "w=5", "one colour", "noise", "directed runs", "fibonacci"])
def test_png_write_stream_files_open_to_the_frame(pa, tmp_path, case):
    """Reference-made dynamic buffers through the unchanged writer: PIL and ptl_png_read return the input pixels; ONE IDAT, 78 01 | stream |
    03 00 | Adler-32; every CRC is right."""
    from PIL import Image

    frame, bands = _encoded(case)
    h, w = frame.shape[:2]
    result = hr.result(frame, bands)
    path = str(tmp_path / "f.png")
    pa.png_write_stream(path, result + bytes(11), w, h)
    image = Image.open(path)
    assert image.mode == "RGBA" and image.size == (w, h) and np.array_equal(np.array(image), frame)
    assert np.array_equal(pa.png_read(path), frame)
    chunks = _chunks(open(path, "rb").read())
    assert [k for k, _ in chunks] == [b"IHDR", b"IDAT", b"IEND"]
    assert chunks[0][1] == struct.pack(">II", w, h) + bytes([8, 6, 0, 0, 0])
    p = pr.parse(result)
    assert chunks[1][1] == pr.zlib_stream(p["stream"], p["adler"])
    assert 64 + pr.stream_capacity(w, h) <= pa.png_stream_download_bytes(w, h) == 64 + (pr.stream_capacity(w, h) + 15) // 16 * 16 < pa.png_stream_bytes(w, h)


def test_entry_point_refuses_before_any_gpu_call(pa):
    """Any `codes` but 0 and 1 -> PTL_ERR_INVALID whatever else is passed; every refusal of ptl_png_deflate_rgba8 carries over to both modes; the
    device is looked at last.  The mirror passes `codes` on."""
    f = pa.lib().ptl_png_deflate_rgba8_codes
    frame, out = C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    for codes in (2, -1, 7, 1 << 20):
        assert f(0, frame, 4, 4, codes, out, None, None) == -1 and "PTL_PNG_CODES" in pa.lib().ptl_last_error().decode()
        assert f(-1, None, 0, 0, codes, None, None, None) == -1
    for codes in (0, 1):
        assert f(0, None, 4, 4, codes, out, None, None) == -1 and f(0, frame, 4, 4, codes, None, None, None) == -1
        assert f(0, frame, 0, 4, codes, out, None, None) == -1 and f(0, frame, 4, -4, codes, out, None, None) == -1
        assert f(0, C.c_void_p((1 << 20) + 8), 4, 4, codes, out, None, None) == -1 and f(0, frame, 4, 4, codes, C.c_void_p((1 << 24) + 4), None, None) == -1
        assert f(0, frame, 1 << 15, 1 << 15, codes, out, None, None) == -1 and "2^31" in pa.lib().ptl_last_error().decode()
        assert f(-1, frame, 4, 4, codes, out, None, None) == -6  # PTL_ERR_NO_DEVICE: checked last
    with pytest.raises(pa.PortalError):
        pa.png_deflate_rgba8_device(1 << 20, 1 << 24, 4, 4, codes=2)
    assert (pa.PNG_CODES_FIXED, pa.PNG_CODES_DYNAMIC) == (0, 1)
    assert pa.png_stream_download_bytes(0, 4) == 0 and pa.png_stream_download_bytes(1 << 15, 1 << 15) == 0
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    for words in ("int ptl_png_deflate_rgba8_codes(", "#define PTL_PNG_CODES_FIXED 0", "#define PTL_PNG_CODES_DYNAMIC 1", "size_t ptl_png_stream_download_bytes(",
                  " ".join(str(n) for n in hr.CL_LENGTHS), " ".join(str(s) for s in hr.CL_ORDER), "HDIST = 0", "the leaf where the weights are equal"):
        assert words in header, words


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--png-encoder", "gpu", "--png-codes", "best"], "--png-codes fixed|dynamic"),
                                              ("render-frame", ["--png-encoder", "gpu", "--png-codes", "Dynamic"], "--png-codes fixed|dynamic"),
                                              ("render-frame", ["--png-encoder", "gpu", "--png-codes", "1"], "--png-codes fixed|dynamic"),
                                              ("render", ["--png-codes", "dynamic"], "--png-codes needs --png-encoder gpu"),
                                              ("render", ["--png-codes", "fixed"], "--png-codes needs --png-encoder gpu"),
                                              ("render-frame", ["--png-codes", "dynamic", "--png-encoder", "host"], "--png-codes needs --png-encoder gpu"),
                                              ("render", ["--png-codes", "dynamic", "--frames", "y4m"], "--png-codes needs --png-encoder gpu"),
                                              ("render-frame", ["--png-codes", "dynamic", "--png-depth", "16"], "--png-codes needs --png-encoder gpu"),
                                              ("render", ["--png-encoder", "gpu", "--png-codes", "dynamic", "--png-depth", "16"], "cannot be combined with --png-depth 16"),
                                              ("precompile", ["--png-encoder", "gpu", "--png-codes", "dynamic"], "is an option of render and render-frame"),
                                              ("check", ["--png-codes", "dynamic"], "--png-codes is an option of render and render-frame"),
                                              ("emit-source", ["--png-codes", "fixed"], "--png-codes is an option of render and render-frame"),
                                              ("render-frame", ["--png-encoder", "gpu", "--png-codes", "dynamic", "--gpus", "2"], "the one GPU")])
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
    assert out.returncode == 2 and out.stderr.count("--png-codes fixed|dynamic") == 2 and out.stderr.count("fixed (default)") == 2  # render-frame's and render's
