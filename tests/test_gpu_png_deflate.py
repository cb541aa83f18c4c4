"""GPU deflate of 8-bit PNG frames (`--png-encoder gpu`): the kernels (portal_amd/csrc/kernels/png_deflate.hip) through the C
ABI and the Python mirror, and the CLI.  In every case the whole result buffer -- header and stream, up to the header's byte count -- is
compared byte for byte with tests/png_deflate_reference.py, and zlib.decompress of the stream has to return the raw scanlines."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import png_deflate_harness as hs
from tests import png_deflate_reference as pr
from tests.yuv_harness import FPS, GUARD, H, KNOB, ROOT, W, _c_getenv, _once, _path_without_ffmpeg, _shipped_grid_cap, gpu  # noqa: F401 (gpu: a fixture)

RUN_VALUES = (0, 143, 144, 255)  # both sides of the 8- / 9-bit literal boundary, and the ends
RUN_LENGTHS = tuple(range(1, 21)) + tuple(range(257, 264)) + tuple(range(515, 522))


def _frame_of_raw(body):
    """(H, 4 W) bytes the raw scanlines are to hold behind their filter-type bytes -> the (H, W, 4) frame whose Up filter gives them."""
    body = np.asarray(body, np.uint8)
    frame = np.cumsum(body.astype(np.uint64), axis=0).astype(np.uint8).reshape(body.shape[0], body.shape[1] // 4, 4)
    assert pr.raw_scanlines(frame) == np.concatenate((np.where(np.arange(body.shape[0]) == 0, 0, 2).astype(np.uint8)[:, None], body), axis=1).tobytes()
    return frame


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)


def _mixed(w, h, seed):
    """Raw scanlines that are part noise, part runs of random lengths (1 .. 700) of random values, zero most often."""
    rng = np.random.default_rng(seed)
    flat = rng.integers(0, 256, 4 * w * h, dtype=np.uint8)
    at = 0
    while at < flat.size:
        n = int(rng.integers(1, 700 if rng.random() < 0.2 else 12))
        if rng.random() < 0.6:
            flat[at: at + n] = 0 if rng.random() < 0.5 else rng.integers(0, 256)
        at += n
    return _frame_of_raw(flat.reshape(h, 4 * w))


FIXED8 = hs.Format("png deflate", pr, 4, "png_stream_bytes", "png_stream_band_rows", "png_deflate_rgba8_device", hs.FIXED, lambda frame: np.ascontiguousarray(frame, np.uint8),
                  lambda frame: ({True: pr.result(frame)}, None, pr.raw_scanlines(frame)))
_deflate, _assert_matches = functools.partial(hs._deflate, FIXED8), functools.partial(hs._assert_matches, FIXED8)


def _check(pa, frame, what):
    got = _deflate(pa, frame)
    _assert_matches(got, frame, what)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (3, 1), (17, 5), (64, 64), (1023, 3), (64, 130), (1100, 5), (4100, 3)])
def test_kernel_matches_reference_at_any_frame_size(gpu, w, h):
    """1023x3: the filter-type byte puts every row at another alignment.  64x64 and 64x130: 63 rows per band, so a short last band (1 and 4
    rows).  1100x5: a row of 4401 bytes is longer than a segment.  4100x3: a row of 16401 bytes is longer than the 16384 a band aims at, so a
    band per row, five segments each.  Noise, and noise mixed with runs."""
    assert pr.band_rows(64) == 63 and pr.band_rows(1100) == 3 and pr.band_rows(4100) == 1 and 4 * 4100 + 1 > pr.BAND_TARGET
    _check(gpu, _noise(w, h, 100 * w + h), f"{w}x{h} noise")
    _check(gpu, _mixed(w, h, 100 * w + h + 1), f"{w}x{h} mixed")


@pytest.mark.gpu
def test_every_literal(gpu):
    """All 256 byte values as literals, no two equal neighbours: the 8- and 9-bit codes on both sides of 143 | 144, in four orders."""
    v = np.arange(256)
    body = np.stack([v, v[::-1], (v * 7 + 3) % 256, (v * 151 + 144) % 256]).astype(np.uint8)
    assert all((np.diff(row.astype(int)) != 0).all() and len(set(row.tolist())) == 256 for row in body)
    _check(gpu, _frame_of_raw(body), "every literal")


def _runs_frame():
    """One row: for each of RUN_VALUES, runs of every length of RUN_LENGTHS, a 77 between them; where a run would cross a segment boundary it is
    moved behind the boundary (the gap filled with 1, 2, 1, 2 ...), so every run is tokenised at its full length."""
    body, at = [77], 2  # `at`: the raw offset of the next byte (the filter-type byte is raw byte 0)
    for v in RUN_VALUES:
        for n in RUN_LENGTHS + (tuple(range(21, 257)) if v == 0 else ()):  # (and every length in between, of zeros)
            to_boundary = pr.SEGMENT - at % pr.SEGMENT
            if n + 1 > to_boundary:
                body += [1 + (k % 2) for k in range(to_boundary)]
                at += to_boundary
            body += [v] * n + [77]
            at += n + 1
    body += [3 + (k % 2) for k in range(-len(body) % 4)]
    return _frame_of_raw(np.array(body, np.uint8)[None, :])


@pytest.mark.gpu
def test_runs_of_every_length(gpu):
    """Runs of 1 .. 20, 257 .. 263 and 515 .. 521 bytes of 0, 143, 144 and 255: every length code with its extra-bit boundaries up to 19, the
    258 cap once and twice, and 0, 1 and 2 literals left over."""
    frame = _runs_frame()
    tokens = [t for band in pr.cut_bands(pr.raw_scanlines(frame), frame.shape[1], 1) for s in pr.cut_segments(band) for t in pr.segment_tokens_plain(s)]
    want = set()
    for n in RUN_LENGTHS:
        m = n - 1
        while m >= 3:
            want.add(min(m, 258))
            m -= min(m, 258)
    assert want == set(range(3, 20)) | {256, 257, 258}, sorted(want)
    assert {x for kind, x in tokens if kind == "match"} == set(range(3, 259))  # with the zeros of every length: every match there is
    for v in RUN_VALUES:  # each run as a whole: a literal, then its matches (never cut by a segment boundary)
        assert sum(1 for kind, x in tokens if kind == "lit" and x == v) >= len(RUN_LENGTHS)
    assert tokens.count(("match", 258)) >= 4 * 17  # per value: five runs with one, two with one, five with two
    _check(gpu, frame, "runs of every length")


@pytest.mark.gpu
@pytest.mark.parametrize("value", [2, 0, 255])
def test_runs_across_segments_rows_and_bands(gpu, value):
    """64x130, every raw byte behind the filter-type bytes the same: with 2, the filter-type bytes join the runs, which then cross row, segment
    and band boundaries (63 rows per band) and are cut by the latter two only; with 0 and 255 every row's run ends at the next filter byte."""
    body = np.full((130, 256), value, np.uint8)
    got = _check(gpu, _frame_of_raw(body), f"all {value}")
    assert pr.parse(got)["bands"] == 3
    if value == 2:
        raw = pr.raw_scanlines(_frame_of_raw(body))
        assert raw[1:] == bytes([2]) * (len(raw) - 1)


@pytest.mark.gpu
def test_noise_on_every_bit_offset(gpu):
    """Uniform noise at 256x64: 8- and 9-bit tokens on every bit offset, dwords straddled by tokens and by lanes; the worst case for a slot."""
    frame = _noise(256, 64, 25664)
    got = _check(gpu, frame, "noise 256x64")
    assert len(pr.parse(got)["stream"]) > len(pr.raw_scanlines(frame))


@pytest.mark.gpu
def test_largest_adler_sums(gpu):
    """512x256, every row the row above minus 1: raw is all 255 but for the filter-type bytes, the Adler sums are the largest there are,
    and s2 wraps 65521 some hundred thousand times."""
    w, h = 512, 256
    frame = _frame_of_raw(np.full((h, 4 * w), 255, np.uint8))
    assert np.array_equal(frame[1], frame[0] - 1) and 255 * (4 * w * h) ** 2 // 2 // 65521 > 100000
    _check(gpu, frame, "all 255")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, cap):
    """64x2048 is 33 bands: with PTL_AVERAGE_IMAGES_GRID_CAP at 1 and 3 the workgroups of both kernels go round their loops 33 and 11 times.
    Equal to the reference and to the same call with the shipped grid."""
    w, h = 64, 2048
    assert pr.band_count(w, h) == 33
    frame = _once(("png deflate knob frame",), lambda: _mixed(w, h, 642048))
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None
    shipped = _deflate(gpu, frame)
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    got = _deflate(gpu, frame)
    _assert_matches(got, frame, f"cap={cap}")
    n = pr.HEADER_BYTES + len(pr.parse(got)["stream"])
    assert got[:n] == shipped[:n]


@pytest.mark.gpu
def test_grid_stride_at_the_shipped_cap(gpu, monkeypatch):
    """2048x4100: a band per row (8193 bytes each: two do not fit into 16384), 4100 bands against the 4096 workgroups a post-process launch
    gets at most.  The frame is mostly flat, with 1 % of its bytes random, made on the host once."""
    w, h = 2048, 4100
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None and pr.band_rows(w) == 1 and pr.band_count(w, h) > _shipped_grid_cap()
    rng = np.random.default_rng(20484100)
    frame = np.full((h, w, 4), 90, np.uint8)
    where = rng.integers(0, frame.size, frame.size // 100)
    frame.reshape(-1)[where] = rng.integers(0, 256, where.size, dtype=np.uint8)
    _check(gpu, frame, "2048x4100")


@pytest.mark.gpu
def test_a_reused_buffer_keeps_no_stale_bits(gpu):
    """Noise, then a frame of one colour, then noise again into the SAME result buffer, never cleared: each result is the reference's."""
    import torch

    w, h = 256, 64
    buf = torch.full((gpu.png_stream_bytes(w, h) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    noise, flat = _noise(w, h, 7), np.full((h, w, 4), 77, np.uint8)
    for k, frame in enumerate((noise, flat, noise, flat)):
        _assert_matches(_deflate(gpu, frame, buf=buf), frame, f"launch {k}")


@pytest.mark.gpu
def test_elapsed_ms_and_a_stream_of_the_callers(gpu):
    """Launched on the stream it is given (a non-default torch stream, the input produced on it); with elapsed_ms the launches are bracketed
    by events and waited for."""
    import torch

    pa = gpu
    w, h = 640, 360
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.Generator(device="cuda").manual_seed(11)
        frame = (torch.rand((h, w, 4), device="cuda", generator=g) * 4.0).to(torch.uint8) * 60  # five byte values: literals and short runs
        got, ms = _deflate(pa, frame, timed=True, stream=side.cuda_stream)
        assert ms is not None and 0.0 < ms < 1000.0
        again = _deflate(pa, frame, stream=side.cuda_stream)
    _assert_matches(got, frame, "side stream")
    n = pr.HEADER_BYTES + len(pr.parse(got)["stream"])
    assert again[:n] == got[:n]


# ---- the CLI ---------------------------------------------------------------------------------
def _run_cli(pa, arguments, limit=300):
    """One child under a time limit of its own, waited for before the next starts; no ffmpeg on its PATH."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run(["timeout", "-k", "10", str(limit), exe] + arguments, capture_output=True, text=True, timeout=limit + 100, env=dict(os.environ, PATH=_path_without_ffmpeg()), cwd=ROOT)
    assert out.returncode == 0, out.stderr + out.stdout
    return out


def _render_clip(pa, out_dir, clip, options):
    scene = pa.scene_path("basics")
    return _run_cli(pa, ["render", scene, clip, "--width", str(W), "--height", str(H), "--fps", str(FPS), "--out-dir", str(out_dir), "--asset-root", os.path.dirname(os.path.dirname(scene)),
                         "--aa-count", "2", "--render-depth", "12"] + options)


def _pixels(path):
    from PIL import Image

    image = Image.open(path)
    assert image.mode == "RGBA"
    return np.array(image)


def _one_idat_of_fixed_blocks(path):
    """The file is the GPU encoder's: one IDAT that starts 78 01 and whose first block is a non-final one with the fixed codes."""
    data = open(path, "rb").read()
    assert data.count(b"IDAT") == 1 and data[24] == 8 and data[25] == 6
    at = data.index(b"IDAT") + 4
    return data[at: at + 2] == b"\x78\x01" and data[at + 2] & 7 == 2


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [1, 4])
def test_render_cli_writes_the_same_frames_with_the_gpu_encoder(gpu, tmp_path, blur):
    """`portal-amd render ... --png-encoder gpu` for a 64x36 clip, one sub-frame per frame and four averaged: every frame_<i>.png opens in
    PIL to the pixels of the file `--png-encoder host` writes for the same frame; the stills stay host-encoded.  Once more with --shard 1/2:
    only the odd frames exist, and they are the same files."""
    pa = gpu
    clip = pa.Scene.from_file(pa.scene_path("basics")).animations()[0][0]
    options = ["--motion-blur-frames", str(blur)]
    _render_clip(pa, tmp_path / "gpu", clip, options + ["--png-encoder", "gpu"])
    _render_clip(pa, tmp_path / "host", clip, options + ["--png-encoder", "host"])
    kept = {which: tmp_path / which / "video" / "basics" / f"{clip}.frames" for which in ("gpu", "host")}  # (no ffmpeg: anim/ is parked next to where the video would be)
    names = sorted(os.listdir(kept["host"]))
    assert names == sorted(os.listdir(kept["gpu"])) and len(names) >= 2 and names[0] == "frame_0.png"
    differing = set()
    for name in names:
        got, want = _pixels(kept["gpu"] / name), _pixels(kept["host"] / name)
        assert got.shape == (H, W, 4) and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} of {W * H} pixels differ"
        assert _one_idat_of_fixed_blocks(kept["gpu"] / name) and not _one_idat_of_fixed_blocks(kept["host"] / name)
        differing.add(want.tobytes())
    assert len(differing) > 1  # the clip moves
    for still in (f"{clip}.start.png", f"{clip}.end.png"):
        assert (tmp_path / "gpu" / "video" / "basics" / still).read_bytes() == (tmp_path / "host" / "video" / "basics" / still).read_bytes()
    _render_clip(pa, tmp_path / "shard", clip, options + ["--png-encoder", "gpu", "--shard", "1/2"])
    anim = tmp_path / "shard" / "anim"
    assert sorted(os.listdir(anim)) == sorted(f"frame_{i}.png" for i in range(1, len(names), 2))
    for name in os.listdir(anim):
        assert (anim / name).read_bytes() == (kept["gpu"] / name).read_bytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("adaptive", [None, 4])
def test_render_frame_cli_writes_the_same_file_with_the_gpu_encoder(gpu, tmp_path, adaptive):
    """`portal-amd render-frame scenes/basics.ron --png-encoder gpu` at 64x36, with and without --adaptive-aa 4: the file opens in PIL to the
    pixels of the file the host encoder writes, and without the option the file is byte for byte the one `--png-encoder host` writes."""
    pa = gpu
    common = ["render-frame", pa.scene_path("basics"), "--width", str(W), "--height", str(H), "--aa-count", "4", "--render-depth", "12"] + (["--adaptive-aa", "4"] if adaptive is not None else [])
    _run_cli(pa, common + ["--png-encoder", "gpu", "--output", str(tmp_path / "gpu.png")])
    _run_cli(pa, common + ["--png-encoder", "host", "--output", str(tmp_path / "host.png")])
    _run_cli(pa, common + ["--output", str(tmp_path / "plain.png")])
    got, want = _pixels(tmp_path / "gpu.png"), _pixels(tmp_path / "host.png")
    assert got.shape == (H, W, 4) and np.array_equal(got, want), f"{int((got != want).any(axis=2).sum())} of {W * H} pixels differ"
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 16  # a rendered frame
    assert _one_idat_of_fixed_blocks(tmp_path / "gpu.png") and not _one_idat_of_fixed_blocks(tmp_path / "host.png")
    assert (tmp_path / "plain.png").read_bytes() == (tmp_path / "host.png").read_bytes()
    assert np.array_equal(pa.png_read(str(tmp_path / "gpu.png")), want)
