"""GPU deflate of 8-bit PNG frames with a Huffman code per band (`--png-codes dynamic`): the bands kernel
(portal_amd/csrc/kernels/png_huffman.hip) and the shared pack kernel through ptl_png_deflate_rgba8_codes and the Python mirror, and the CLI.
In every case the whole result buffer -- header and stream, up to the header's byte count -- is compared byte for byte with
tests/png_huffman_reference.py, and zlib.decompress of the stream has to return the raw scanlines."""
import functools
import os

import numpy as np
import pytest

from tests import png_deflate_harness as hs
from tests import png_deflate_reference as pr
from tests import png_huffman_reference as hr
from tests.png_huffman_cases import costly_last_segment_frame, fibonacci_frame
from tests.test_gpu_png_deflate import _frame_of_raw, _mixed, _noise, _pixels, _render_clip, _run_cli, _runs_frame
from tests.yuv_harness import GUARD, H, KNOB, W, _c_getenv, _once, gpu  # noqa: F401 (gpu: a fixture)

def _encode(frame):
    bands = hr.encode_bands(frame)
    return {False: hr.result(frame, bands)}, bands, pr.raw_scanlines(frame)


DYNAMIC8 = hs.Format("png huffman", pr, 4, "png_stream_bytes", "png_stream_band_rows", "png_deflate_rgba8_device", hs.DYNAMIC, lambda frame: np.ascontiguousarray(frame, np.uint8), _encode)
_deflate, _assert_matches, _check = (functools.partial(f, DYNAMIC8) for f in (hs._deflate, hs._assert_matches, hs._check))


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 64), (1023, 3), (64, 130), (1100, 5), (4100, 3)])
def test_kernel_matches_reference_at_any_frame_size(gpu, w, h):
    """1023x3: every row at another alignment.  64x64 and 64x130: 63 rows per band, so a short last band.  1100x5: a row longer than a segment.
    4100x3: a row longer than the band target, a band per row, five segments each.  Noise, and noise mixed with runs."""
    _check(gpu, _noise(w, h, 100 * w + h), f"{w}x{h} noise")
    _check(gpu, _mixed(w, h, 100 * w + h + 1), f"{w}x{h} mixed")


@pytest.mark.gpu
def test_bands_of_both_choices_in_one_frame(gpu):
    """64x64 noise: the band of 63 rows is dearer with the fixed code than with its own, the band of one row (257 bytes) cannot pay for a block
    header.  A 1x1 frame chooses fixed as well."""
    bands = _check(gpu, _noise(64, 64, 6464), "64x64 noise, both choices")
    assert [b["dynamic"] for b in bands] == [True, False]
    assert [b["dynamic"] for b in _check(gpu, _noise(1, 1, 11), "1x1")] == [False]


@pytest.mark.gpu
def test_every_literal(gpu):
    v = np.arange(256)
    body = np.stack([v, v[::-1], (v * 7 + 3) % 256, (v * 151 + 144) % 256]).astype(np.uint8)
    bands = _check(gpu, _frame_of_raw(body), "every literal")
    assert (bands[0]["hist"][:256] > 0).all()


@pytest.mark.gpu
def test_runs_of_every_length(gpu):
    """The directed runs of the fixed-code suite: lengths 1 .. 20, 257 .. 263, 515 .. 521 of four values, and zeros of every length up to 256, so
    every length symbol and every extra-bit count occurs under a code of the band's own."""
    bands = _check(gpu, _runs_frame(), "runs of every length")
    assert any(b["dynamic"] for b in bands) and sum(int((b["hist"][257:] > 0).sum()) for b in bands) >= 29


@pytest.mark.gpu
@pytest.mark.parametrize("value", [2, 0, 255])
def test_runs_across_segments_rows_and_bands(gpu, value):
    body = np.full((130, 256), value, np.uint8)
    bands = _check(gpu, _frame_of_raw(body), f"all {value}")
    assert len(bands) == 3


@pytest.mark.gpu
def test_one_colour_and_noise(gpu):
    """256x64 of one colour: two or three literals per band (0, 2 and in the first row the colour), the match of 258 in one bit.  Noise: about 256 symbols of about 8 bits on every bit
    offset; the stream stays below the fixed-code one."""
    flat = np.full((64, 256, 4), 77, np.uint8)
    bands = _check(gpu, flat, "one colour 256x64")
    assert all(2 <= int((b["hist"][:256] > 0).sum()) <= 3 and b["dynamic"] and b["lengths"][285] == 1 for b in bands)
    noise = _noise(256, 64, 25664)
    got = _deflate(gpu, noise)
    _assert_matches(got, noise, "noise 256x64")
    assert len(pr.parse(got)["stream"]) <= len(pr.stream(noise))


@pytest.mark.gpu
def test_largest_adler_sums(gpu):
    w, h = 512, 256
    _check(gpu, _frame_of_raw(np.full((h, 4 * w), 255, np.uint8)), "all 255 at 512x256")


@pytest.mark.gpu
def test_the_length_limit(gpu):
    """The Fibonacci frame: the unlimited tree is deeper than 15, the repair applies."""
    frame = fibonacci_frame()
    bands = _check(gpu, frame, "fibonacci")
    assert len(bands) == 1 and bands[0]["dynamic"] and int(bands[0]["lengths"].max()) == 15
    assert hr.code_lengths_plain(bands[0]["hist"])[1] > 15


@pytest.mark.gpu
def test_a_segment_dearer_than_nine_bits_a_byte(gpu):
    """The last of four segments costs more than 9 bits per byte under the band's own code, while the band as a whole chooses dynamic: the
    kernel's bit buffer has to hold 15 bits per byte."""
    frame = costly_last_segment_frame()
    bands = _check(gpu, frame, "costly last segment")
    assert len(bands) == 1 and bands[0]["dynamic"] and len(bands[0]["segment_bits"]) == 4
    assert bands[0]["segment_bits"][3] > 9 * 4093, bands[0]["segment_bits"]


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, cap):
    """64x2048 is 33 bands: with the knob at 1 and 3 the workgroups of both kernels go round their loops 33 and 11 times."""
    w, h = 64, 2048
    frame = _once(("png huffman knob frame",), lambda: _mixed(w, h, 642048))
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    _assert_matches(_deflate(gpu, frame), frame, f"cap={cap}", key="knob frame")


@pytest.mark.gpu
def test_a_reused_buffer_keeps_no_stale_bits(gpu):
    import torch

    w, h = 256, 64
    buf = torch.full((gpu.png_stream_bytes(w, h) + 64,), GUARD, dtype=torch.uint8, device="cuda")
    noise, flat = _noise(w, h, 7), np.full((h, w, 4), 77, np.uint8)
    for k, (frame, key) in enumerate(((noise, "reuse noise"), (flat, "reuse flat"), (noise, "reuse noise"))):
        _assert_matches(_deflate(gpu, frame, buf=buf), frame, f"launch {k}", key=key)


@pytest.mark.gpu
def test_elapsed_ms_a_stream_of_the_callers_and_the_fixed_mode(gpu):
    """Launched on the stream it is given, timed when asked; codes = 0 is ptl_png_deflate_rgba8, byte for byte, whole buffer."""
    import ctypes as C

    import torch

    pa = gpu
    w, h = 640, 360
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.Generator(device="cuda").manual_seed(11)
        frame = (torch.rand((h, w, 4), device="cuda", generator=g) * 4.0).to(torch.uint8) * 60
        got, ms = _deflate(pa, frame, timed=True, stream=side.cuda_stream)
        assert ms is not None and 0.0 < ms < 1000.0
    _assert_matches(got, frame, "side stream")
    nbytes = pa.png_stream_bytes(w, h)
    old = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    pa.png_deflate_rgba8_device(frame.data_ptr(), old.data_ptr(), w, h)
    new = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert pa.lib().ptl_png_deflate_rgba8_codes(0, C.c_void_p(frame.data_ptr()), w, h, 0, C.c_void_p(new.data_ptr()), None, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(old, new)
    assert bytes(old[: 64 + len(pr.stream(frame.cpu().numpy()))].cpu().numpy()) == pr.result(frame.cpu().numpy())


# ---- the CLI ---------------------------------------------------------------------------------
def _dynamic_blocks(path):
    """The file is the GPU encoder's with codes of its own: one IDAT that starts 78 01 and whose first block is a non-final dynamic one."""
    data = open(path, "rb").read()
    assert data.count(b"IDAT") == 1 and data[24] == 8 and data[25] == 6
    at = data.index(b"IDAT") + 4
    return data[at: at + 2] == b"\x78\x01" and data[at + 2] & 7 == 4


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [1, 4])
def test_render_cli_writes_the_same_frames_with_dynamic_codes(gpu, tmp_path, blur):
    """`portal-amd render ... --png-encoder gpu --png-codes dynamic` for a 64x36 clip: every frame opens in PIL to the pixels of the host
    encoder's file and is smaller than the fixed-code file; `--png-codes fixed` writes the files of no option at all; --shard 1/2 writes the
    odd frames, the same files."""
    pa = gpu
    clip = pa.Scene.from_file(pa.scene_path("basics")).animations()[0][0]
    options = ["--motion-blur-frames", str(blur)]
    _render_clip(pa, tmp_path / "dynamic", clip, options + ["--png-encoder", "gpu", "--png-codes", "dynamic"])
    _render_clip(pa, tmp_path / "host", clip, options + ["--png-encoder", "host"])
    _render_clip(pa, tmp_path / "fixed", clip, options + ["--png-encoder", "gpu", "--png-codes", "fixed"])
    _render_clip(pa, tmp_path / "plain", clip, options + ["--png-encoder", "gpu"])
    kept = {which: tmp_path / which / "video" / "basics" / f"{clip}.frames" for which in ("dynamic", "host", "fixed", "plain")}
    names = sorted(os.listdir(kept["host"]))
    assert names == sorted(os.listdir(kept["dynamic"])) and len(names) >= 2 and names[0] == "frame_0.png"
    for name in names:
        got, want = _pixels(kept["dynamic"] / name), _pixels(kept["host"] / name)
        assert got.shape == (H, W, 4) and np.array_equal(got, want), f"{name}: {int((got != want).any(axis=2).sum())} of {W * H} pixels differ"
        assert _dynamic_blocks(kept["dynamic"] / name)
        assert (kept["fixed"] / name).read_bytes() == (kept["plain"] / name).read_bytes()
        assert os.path.getsize(kept["dynamic"] / name) < os.path.getsize(kept["fixed"] / name)
    _render_clip(pa, tmp_path / "shard", clip, options + ["--png-encoder", "gpu", "--png-codes", "dynamic", "--shard", "1/2"])
    anim = tmp_path / "shard" / "anim"
    assert sorted(os.listdir(anim)) == sorted(f"frame_{i}.png" for i in range(1, len(names), 2))
    for name in os.listdir(anim):
        assert (anim / name).read_bytes() == (kept["dynamic"] / name).read_bytes(), name


@pytest.mark.gpu
@pytest.mark.parametrize("adaptive", [None, 4])
def test_render_frame_cli_writes_the_same_file_with_dynamic_codes(gpu, tmp_path, adaptive):
    pa = gpu
    common = ["render-frame", pa.scene_path("basics"), "--width", str(W), "--height", str(H), "--aa-count", "4", "--render-depth", "12"] + (["--adaptive-aa", "4"] if adaptive is not None else [])
    _run_cli(pa, common + ["--png-encoder", "gpu", "--png-codes", "dynamic", "--output", str(tmp_path / "dynamic.png")])
    _run_cli(pa, common + ["--png-encoder", "host", "--output", str(tmp_path / "host.png")])
    got, want = _pixels(tmp_path / "dynamic.png"), _pixels(tmp_path / "host.png")
    assert got.shape == (H, W, 4) and np.array_equal(got, want), f"{int((got != want).any(axis=2).sum())} of {W * H} pixels differ"
    assert len(np.unique(want.reshape(-1, 4), axis=0)) > 16  # a rendered frame
    assert _dynamic_blocks(tmp_path / "dynamic.png")
    assert np.array_equal(pa.png_read(str(tmp_path / "dynamic.png")), want)
    # the file is the reference's stream of these pixels
    p = hr.result(want)
    chunk = open(tmp_path / "dynamic.png", "rb").read()
    at = chunk.index(b"IDAT") + 4
    assert chunk[at + 2: at + 2 + len(p) - 64] == p[64:]
