"""GPU deflate of 16-bit PNG frames (`--png-depth 16 --png16-encoder gpu`): the bands and the pack kernel
(portal_amd/csrc/kernels/png_huffman.hip, png_deflate.hip) through ptl_png_deflate_rgb48 and the Python mirror, and the CLI.  In every case the whole
result buffer -- header and stream, up to the header's byte count -- is compared byte for byte with tests/png16_deflate_reference.py, and
zlib.decompress of the stream has to return the raw scanlines."""
import functools
import math
import os
import zlib

import numpy as np
import pytest

from tests import png16_deflate_cases as cs
from tests import png16_deflate_reference as r6
from tests import png16_reference as p16
from tests import png_deflate_harness as hs
from tests import yuv_deep_reference as dr
from tests.test_png16 import _clip_frames, _render_clip, _run_cli
from tests.yuv_harness import GUARD, H, KNOB, W, _c_getenv, _once, _shipped_grid_cap, gpu  # noqa: F401 (gpu: a fixture)

DYNAMIC, FIXED = 1, 0
_band_cache = {}


def _bands(raw, w, h):
    """encode_bands with every distinct band encoded once (a frame of many equal rows stays cheap)."""
    out = []
    for band in r6.cut_bands(raw, w, h):
        if band not in _band_cache:
            _band_cache[band] = r6.encode_band(band)
        out.append(_band_cache[band])
    return out


def _encode(a):
    h, w = a.shape[:2]
    raw = r6.raw16(a)
    bands = _bands(raw, w, h)
    return {False: r6.result(raw, w, h, bands), True: r6.result(raw, w, h, bands, fixed=True)}, bands, raw


RGB48 = hs.Format("png16 deflate", r6, 6, "png_stream16_bytes", "png_stream16_band_rows", "png_deflate_rgb48_device", hs.DYNAMIC, r6.rows_bytes, _encode)
_deflate, _assert_matches, _check = (functools.partial(f, RGB48) for f in (hs._deflate, hs._assert_matches, hs._check))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (2, 1), (1, 5), (5, 3), (64, 64), (683, 3), (682, 2), (2731, 2), (64, 43), (17, 300)])
def test_kernel_matches_reference_at_any_frame_size(gpu, w, h):
    """683x3: rows of 4099 bytes, longer than a segment, odd W (rows 1 and 2 start 2-byte aligned only).  682x2: even W.  2731x2: a row longer
    than the band target, a band per row, five segments each.  64x43 and 17x300: a short last band (42 + 1 rows, 159 + 141).  Noise, and
    noise mixed with repeated pixels and repeated rows."""
    assert r6.band_rows(2731) == 1 and 6 * 2731 + 1 > 16384 and r6.band_rows(64) == 42 and r6.band_rows(17) == 159
    _check(gpu, cs.noise(w, h, 100 * w + h), f"{w}x{h} noise")
    _check(gpu, cs.mixed(w, h, 100 * w + h + 1), f"{w}x{h} mixed")


@pytest.mark.gpu
def test_directed_rows(gpu):
    """H = 1 frames whose raw bytes are chosen: all 256 literals; covered stretches of 1 .. 20, 257 .. 263, 515 .. 521; one pixel repeated
    across segment boundaries (six literals behind each); bytes equal at distance 1 but not 6, and at 6 but not 1."""
    bands = _check(gpu, cs.every_literal(), "every literal")
    assert (bands[0]["hist"][:256] > 0).all()
    bands = _check(gpu, cs.covered_stretches(), "covered stretches")
    assert (bands[0]["hist"][257:270] > 0).all() and bands[0]["hist"][284] > 0 and bands[0]["hist"][285] > 0  # lengths 3 .. 20, 257, 258
    bands = _check(gpu, cs.across_a_segment_boundary(), "across a segment boundary")
    assert len(bands) == 1 and 6 * 4 <= int(bands[0]["hist"][:256].sum()) <= 6 * 4 + 3 and bands[0]["hist"][285] >= 3 * 15
    bands = _check(gpu, cs.distance_one_not_six(), "distance 1 but not 6")
    assert int(bands[0]["hist"][257:].sum()) >= 6


@pytest.mark.gpu
def test_the_length_limit_a_costly_segment_and_both_choices(gpu):
    """The Fibonacci frame: the unlimited tree is deeper than 15, the repair applies.  A band whose last segment costs more than 9 bits per
    byte while the band chooses dynamic: the bit buffer has to hold 15 bits per byte.  64x43 noise: a dynamic and a fixed band in one
    frame; 1x1 chooses fixed."""
    from tests import png_huffman_reference as hr

    bands = _check(gpu, cs.fibonacci(), "fibonacci")
    assert len(bands) == 1 and bands[0]["dynamic"] and int(bands[0]["lengths"].max()) == 15 and hr.code_lengths_plain(bands[0]["hist"])[1] > 15
    bands = _check(gpu, cs.costly_last_segment(), "costly last segment")
    assert len(bands) == 1 and bands[0]["dynamic"] and bands[0]["segment_bits"][3] > 9 * 4093, bands[0]["segment_bits"]
    assert [b["dynamic"] for b in _check(gpu, cs.both_choices(), "both choices")] == [True, False]
    assert [b["dynamic"] for b in _check(gpu, cs.noise(1, 1, 11), "1x1")] == [False]


@pytest.mark.gpu
def test_rows_whose_differences_have_period_six(gpu):
    """Each row the row above plus a constant per byte lane (every row below the first: six literals and matches), and plus a constant per
    16-bit sample (the carries break the period); 300x60 is 9 rows per band, 640x7 four rows per band."""
    for w, h in ((300, 60), (640, 7)):
        bands = _check(gpu, cs.period_six_rows(w, h), f"period 6 {w}x{h}")
        assert sum(int(b["hist"][285]) for b in bands) >= (h - 1) * ((6 * w - 6) // 258 - 1)
        _check(gpu, cs.period_six_rows(w, h, carry=True), f"sample steps {w}x{h}")


@pytest.mark.gpu
def test_largest_adler_sums_one_colour_and_noise(gpu):
    """341x128: every raw byte behind a filter-type byte is 255.  256x64 of one colour: six literals and matches per segment.  Noise at
    256x64: the stream stays below the fixed-code one."""
    _check(gpu, cs.all_255_differences(341, 128), "all 255 at 341x128")
    bands = _check(gpu, cs.one_colour(256, 64), "one colour 256x64")
    assert all(b["dynamic"] for b in bands)
    noise = cs.noise(256, 64, 25664)
    got = _deflate(gpu, noise)
    bands = _assert_matches(got, noise, "noise 256x64")
    assert len(r6.parse(got)["stream"]) <= sum(len(b["fixed_data"]) for b in bands)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, cap):
    """64x2048 is 49 bands: with the knob at 1 and 3 the workgroups of both kernels go round their loops 49 and 17 times."""
    w, h = 64, 2048
    a = _once(("png16 deflate knob frame",), lambda: cs.mixed(w, h, 642048))
    assert r6.band_count(w, h) == 49
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    _assert_matches(_deflate(gpu, a), a, f"cap={cap}", key="knob frame")


@pytest.mark.gpu
def test_grid_stride_at_the_shipped_cap(gpu, monkeypatch):
    """2731x4100: a band per row, 4100 bands against the shipped cap of 4096 workgroups, so four workgroups take a second band.  Cheap
    content -- a row of noise repeated, with three other rows in between and at the end -- so the reference encodes a handful of distinct
    bands."""
    w, h = 2731, 4100
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None and r6.band_count(w, h) == h > _shipped_grid_cap()
    rng = np.random.default_rng(2731)
    a = np.repeat(rng.integers(0, 65536, (1, w, 3)), h, axis=0).astype(np.int64)
    for y in (1, 2000, 4097, 4099):
        a[y] = rng.integers(0, 65536, (w, 3))
    _check(gpu, a, "2731x4100")
    assert len(_band_cache) < 200


@pytest.mark.gpu
def test_a_reused_buffer_keeps_no_stale_bits(gpu):
    import torch

    w, h = 256, 64
    buf = torch.full((gpu.png_stream16_bytes(w, h) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    noise, flat = cs.noise(w, h, 7), cs.one_colour(w, h)
    for k, (a, key) in enumerate(((noise, "reuse noise"), (flat, "reuse flat"), (noise, "reuse noise"))):
        _assert_matches(_deflate(gpu, a, buf=buf), a, f"launch {k}", key=key)


@pytest.mark.gpu
def test_elapsed_ms_a_stream_of_the_callers_and_the_fixed_mode(gpu):
    """Launched on the stream it is given, timed when asked; codes = 0 is the reference's fixed form: the fixed block in every band."""
    import torch

    pa = gpu
    w, h = 640, 360
    a = cs.mixed(w, h, 11)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rows = torch.from_numpy(r6.rows_bytes(a)).cuda()
        got, ms = _deflate_rows(pa, rows, w, h, side.cuda_stream)
        assert ms is not None and 0.0 < ms < 1000.0
    _assert_matches(got, a, "side stream")
    fixed = _deflate(pa, a, codes=FIXED)
    _assert_matches(fixed, a, "fixed mode", key="side stream", fixed=True)
    assert fixed[64] & 7 == 2 and len(r6.parse(fixed)["stream"]) > len(r6.parse(got)["stream"])  # BFINAL = 0, BTYPE = 01


def _deflate_rows(pa, rows, w, h, stream):
    import torch

    nbytes = pa.png_stream16_bytes(w, h)
    buf = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    ms = pa.png_deflate_rgb48_device(rows.data_ptr(), buf.data_ptr(), w, h, stream=stream, timed=True)
    host = buf.cpu().numpy()  # (the timed call has waited)
    assert (host[nbytes:] == GUARD).all()
    return host[:nbytes].tobytes(), ms


@pytest.mark.gpu
def test_rows_from_the_float_kernel_deflate_to_the_same_stream(gpu):
    """The chain the CLI runs: ptl_average_f32_to_rgb48(PTL_PNG_FILTER_NONE) into a device frame, ptl_png_deflate_rgb48 of that frame."""
    import torch

    from tests.yuv_harness import _random_frames

    pa = gpu
    w, h = 70, 37
    frames = _random_frames(7037, 3, w, h)
    staged = [torch.from_numpy(np.ascontiguousarray(f, np.float32)).cuda() for f in frames]
    rows = torch.zeros(pa.rgb48_frame_bytes(w, h), dtype=torch.uint8, device="cuda")
    pa.average_f32_to_rgb48_device([f.data_ptr() for f in staged], rows.data_ptr(), w, h, pa.PNG_FILTER_NONE, stream=torch.cuda.current_stream().cuda_stream)
    nbytes = pa.png_stream16_bytes(w, h)
    buf = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    pa.png_deflate_rgb48_device(rows.data_ptr(), buf.data_ptr(), w, h, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    _assert_matches(buf.cpu().numpy()[:nbytes].tobytes(), dr.encode16(frames), "70x37 from floats")


# ---- the CLI ---------------------------------------------------------------------------------
def _gpu_made(path):
    """The file is the GPU encoder's: 16 bits, colour type 2, one IDAT that starts 78 01."""
    data = open(path, "rb").read()
    at = data.index(b"IDAT") + 4
    return data.count(b"IDAT") == 1 and data[24] == 16 and data[25] == 2 and data[at: at + 2] == b"\x78\x01"


def _file_is_the_reference_stream(path, a):
    h, w = a.shape[:2]
    raw = r6.raw16(a)
    want = r6.result(raw, w, h, _bands(raw, w, h))
    image, said = r6.read_png16_up(str(path), header=True)
    assert len(said["idat"]) == 1 and said["idat"][0][2: 2 + len(want) - 64] == want[64:] and said["idat"][0][-4:] == zlib.adler32(raw).to_bytes(4, "big")
    return image


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [1, 4])
def test_render_cli_writes_the_same_frames(gpu, tmp_path, blur):
    """`portal-amd render ... --png-depth 16 --png16-encoder gpu` for a 64x36 clip, one sub-frame and four: every frame decodes to encode16 of
    the float sub-frames the Python mirror draws and to the pixels of the host-encoded file of the same command, and its IDAT is the
    reference's stream; `--png16-encoder host` writes the files of no option at all; --shard 1/2 writes the odd frames, the same files."""
    pa = gpu
    frames, clip = _clip_frames(pa, blur, None)
    options = ["--motion-blur-frames", str(blur), "--png-depth", "16"]
    _render_clip(pa, tmp_path / "gpu", clip, options + ["--png16-encoder", "gpu"])
    _render_clip(pa, tmp_path / "host", clip, options + ["--png16-encoder", "host"])
    _render_clip(pa, tmp_path / "plain", clip, options)
    kept = {which: tmp_path / which / "video" / "basics" / f"{clip}.frames" for which in ("gpu", "host", "plain")}
    names = sorted(os.listdir(kept["host"]))
    assert names == sorted(os.listdir(kept["gpu"])) == sorted(f"frame_{i}.png" for i in range(len(frames))) and len(names) >= 2
    for i, subs32 in enumerate(frames):
        name = f"frame_{i}.png"
        want = dr.encode16(subs32)
        got = _file_is_the_reference_stream(kept["gpu"] / name, want)
        assert got.shape == (H, W, 3) and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} of {W * H} pixels differ"
        assert np.array_equal(got, p16.read_png16(str(kept["host"] / name))) and _gpu_made(kept["gpu"] / name)
        assert (kept["host"] / name).read_bytes() == (kept["plain"] / name).read_bytes()
    start = (tmp_path / "gpu" / "video" / "basics" / f"{clip}.start.png").read_bytes()
    assert start[24] == 8 and start[25] == 6  # the still stays 8-bit, host-encoded
    _render_clip(pa, tmp_path / "shard", clip, options + ["--png16-encoder", "gpu", "--shard", "1/2"])
    anim = tmp_path / "shard" / "anim"
    assert sorted(os.listdir(anim)) == sorted(f"frame_{i}.png" for i in range(1, len(names), 2))
    for name in os.listdir(anim):
        assert (anim / name).read_bytes() == (kept["gpu"] / name).read_bytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("adaptive", [None, 4])
def test_render_frame_cli_writes_the_same_file(gpu, tmp_path, adaptive):
    """`portal-amd render-frame scenes/basics.ron --png-depth 16 --png16-encoder gpu` at 70x37 (odd rows: 2-byte aligned), with and without
    --adaptive-aa 4: the file decodes to encode16 of the float frame the Python mirror draws and to the pixels of the host-encoded file, and
    its IDAT is the reference's stream of those pixels."""
    pa = gpu
    w, h = 70, 37
    spec = pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL
    common = ["render-frame", pa.scene_path("basics"), "--width", str(w), "--height", str(h), "--aa-count", "4", "--render-depth", "12", "--png-depth", "16"] + (["--adaptive-aa", "4"] if adaptive is not None else [])
    out = _run_cli(pa, common + ["--png16-encoder", "gpu", "--timing", "--output", str(tmp_path / "gpu.png")])
    assert "png16 encoder gpu: deflate" in out.stdout
    _run_cli(pa, common + ["--png16-encoder", "host", "--output", str(tmp_path / "host.png")])
    _run_cli(pa, common + ["--output", str(tmp_path / "plain.png")])
    assert (tmp_path / "host.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path("basics")), device=0, flags=spec | pa.FLAG_QUICK_JIT | (pa.FLAG_REFINE if adaptive is not None else 0))
    r.set_option("aa_count", 4)
    r.set_option("render_depth", 12)
    r.set_option("view_angle", 90.0 / 180.0 * math.pi)
    r.update(0.0)
    mirror = r.draw_adaptive(w, h, threshold=adaptive, rgba32f=True) if adaptive is not None else r.draw(w, h, rgba8=True, rgba32f=True)
    want = dr.encode16([np.array(mirror["rgba32f"])])
    got = _file_is_the_reference_stream(tmp_path / "gpu.png", want)
    assert np.array_equal(got, want), f"{int((got != want).any(axis=2).sum())} of {w * h} pixels differ"
    assert np.array_equal(got, p16.read_png16(str(tmp_path / "host.png"))) and _gpu_made(tmp_path / "gpu.png")
    opened = pa.png_read(str(tmp_path / "gpu.png"))
    assert np.array_equal(opened[..., :3], want >> 8) and (opened[..., 3] == 255).all()
    assert len(np.unique(want)) > 256  # the frame holds more than 8 bits can
