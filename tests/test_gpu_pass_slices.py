"""Pass images of a clip's frames on the MI355X: ptl_pass_slices_to_gray16 against tests/pass_slices_reference.py, byte for byte, with 64 guard
bytes behind every output, and `render --clip-passes` / `render-frame --passes cut` end to end.  One child process at a time.
"""
import functools
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pass_reference as ref
from tests import pass_slices_reference as sref
from tests.test_gpu_passes import LINE, run_cli
from tests.test_pass_slices import random_slices
from tests.yuv_harness import GUARD, KNOB, _c_getenv, _shipped_grid_cap, gpu  # noqa: F401 (gpu: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (True, True, True)
POISON = ref.records(np.float32(-1.0), 2**32 - 1, final=1, escaped=0, exhausted=65535, outside=0)  # a padding record: every image shows a read of it


def run_slices(pa, slices, lo=0.0, hi=1.0, outputs=ALL, padding=0, stream=None, timed=False):
    """slices (N, n) uploaded with slice_records = n + padding (the padding poisoned) -> {name: bytes} of the outputs asked for."""
    import torch

    slices = np.ascontiguousarray(slices)
    n_slices, n = slices.shape
    block = np.full((n_slices, n + padding), POISON, ref.RECORD)
    block[:, :n] = slices
    dev = torch.from_numpy(block.view(np.uint8).reshape(-1).copy()).cuda()
    outs = [torch.full((2 * n + 64,), GUARD, dtype=torch.uint8, device="cuda") if want else None for want in outputs]
    assert dev.data_ptr() % 16 == 0 and all(o is None or o.data_ptr() % 16 == 0 for o in outs)
    torch.cuda.synchronize()
    ms = pa.pass_slices_to_gray16_device(dev.data_ptr(), n_slices, n + padding, n, *[0 if o is None else o.data_ptr() for o in outs], lo=lo, hi=hi,
                                         stream=torch.cuda.current_stream().cuda_stream if stream is None else stream, timed=timed)
    torch.cuda.synchronize()
    got = {}
    for name, o in zip(sref.NAMES, outs):
        if o is not None:
            seen = o.cpu().numpy()
            assert (seen[2 * n:] == GUARD).all(), f"written behind the {name} image"
            got[name] = seen[: 2 * n].tobytes()
    return (got, ms) if timed else got


def check(pa, slices, lo=0.0, hi=1.0, what="", **how):
    got = run_slices(pa, slices, lo, hi, **how)
    want = sref.gray16(slices, lo, hi)
    for name, data in got.items():
        if data != ref.gray16_bytes(want[name]):
            g, r = np.frombuffer(data, ">u2"), want[name]
            bad = np.flatnonzero(g != r)
            pytest.fail(f"{what} {name}: {len(bad)} of {g.size} samples differ, first at {bad[0]}: got {g[bad[0]]}, want {r[bad[0]]} for {np.asarray(slices)[:, bad[0]]}")
    return got


# ---- the kernel -------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 1023, 1024, 1025, 3074])
def test_any_count_and_any_number_of_slices(gpu, n):
    """n around the four pixels of a lane and the 1024 of a workgroup, N around the four slices of a loop trip: packed slices, and slices five
    poisoned records apart."""
    for n_slices in (1, 2, 3, 5, 16, 17):
        slices = random_slices(n_slices, n, 1000 * n + n_slices)
        for padding in (0, 5):
            got = check(gpu, slices, -1.0, 7.5, f"n {n} N {n_slices} padding {padding}", padding=padding)
            assert sorted(got) == ["cut", "depth", "trips"]


@pytest.mark.gpu
def test_every_subset_of_outputs(gpu):
    slices = random_slices(3, 1025, 8)
    for outputs in itertools.product((False, True), repeat=3):
        if any(outputs):
            got = check(gpu, slices, 0.0, 4.0, f"outputs {outputs}", outputs=outputs, padding=5)
            assert sorted(got) == sorted(name for name, want in zip(sref.NAMES, outputs) if want)


@pytest.mark.gpu
def test_one_slice_is_passes_to_gray16_on_the_same_records(gpu):
    import torch

    pa = gpu
    rec = random_slices(1, 4099, 21)
    dev = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
    outs = [torch.full((2 * rec.size + 64,), GUARD, dtype=torch.uint8, device="cuda") for _ in range(4)]
    stream = torch.cuda.current_stream().cuda_stream
    for lo, hi in ((-1.0, 7.5), (np.nan, 1.0), (2.75, 2.75)):
        pa.pass_slices_to_gray16_device(dev.data_ptr(), 1, 0, rec.size, outs[0].data_ptr(), outs[1].data_ptr(), 0, lo=lo, hi=hi, stream=stream)  # (slice_records is not looked at)
        pa.passes_to_gray16_device(dev.data_ptr(), rec.size, outs[2].data_ptr(), ref.DEPTH, lo, hi, stream=stream)
        pa.passes_to_gray16_device(dev.data_ptr(), rec.size, outs[3].data_ptr(), ref.TRIPS, lo, hi, stream=stream)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
        assert outs[0][: 2 * rec.size].cpu().numpy().tobytes() == ref.gray16_bytes(ref.gray16(rec[0], ref.DEPTH, lo, hi))


@pytest.mark.gpu
def test_saturation_rounding_and_the_depth_rule(gpu):
    pa = gpu
    zeros = lambda *shape: np.zeros(shape, np.float32)  # noqa: E731
    sums = check(pa, ref.records(zeros(2, 3), np.array([[65533, 65534, 65535], [1, 1, 1]], np.uint32)), what="trips sums")
    assert np.frombuffer(sums["trips"], ">u2").tolist() == [65534, 65535, 65535]
    many = check(pa, ref.records(zeros(256, 2), np.array([[2**32 - 1, 0]] * 255 + [[2**32 - 1, 9]], np.uint32)), what="256 slices of 2^32 - 1 trips")
    assert np.frombuffer(many["trips"], ">u2").tolist() == [65535, 9]
    wrapping = check(pa, ref.records(zeros(2, 1), np.array([[2**32 - 1], [2]], np.uint32)), what="a sum that is 1 modulo 2^32")
    assert np.frombuffer(wrapping["trips"], ">u2").tolist() == [65535]
    final, exhausted = np.full((256, 4), 65535), np.full((256, 4), 65535)
    exhausted[:, 0], exhausted[0, 0] = 0, 1          # E = 1 of P = 2 * 65535 * 256 + 1: the smallest share there is -> 1
    final[1:, 2], final[0, 2] = 0, 1                 # escaped 0 below: E = P - 1 of the largest E -> 65535 (ceil)
    escaped = np.full((256, 4), 65535)
    escaped[:, 2] = 0
    final[:, 3], escaped[:, 3] = 0, 0                # E = P
    big = check(pa, ref.records(zeros(256, 4), 0, final, escaped, exhausted, 65535), what="saturated counts over 256 slices")
    assert np.frombuffer(big["cut"], ">u2").tolist() == [1, 21845, 65535, 65535]
    rng = np.random.default_rng(5)
    shape = (7, 4099)  # shares of every size: counts up to 65535 in a few slices, up to 3 in the others
    counts = [np.where(rng.random(shape) < 0.2, rng.integers(0, 65536, shape), rng.integers(0, 4, shape)) for _ in range(4)]
    check(pa, ref.records(zeros(*shape), 1, *counts), what="random shares")
    none = check(pa, ref.records(zeros(2, 2), 0, [[0, 3], [0, 2]], [[0, 1], [0, 1]], 0, [[4, 0], [4, 0]]), what="nothing traced, nothing cut")
    assert np.frombuffer(none["cut"], ">u2").tolist() == [0, 0]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    depth = np.array([[nan, 0.10, 0.50, 0.75, 0.20, nan], [0.25, 0.75, 0.50, 0.25, 0.30, 0.50], [0.10, 0.50, 0.50, 0.50, inf, 0.75]], np.float32)
    rule = check(pa, ref.records(depth, 1, final=np.array([[1, 0, 1, 1, 0, 0], [1, 1, 1, 2, 0, 1], [1, 1, 3, 1, 0, 1]])), what="the depth rule")
    assert np.frombuffer(rule["depth"], ">u2").tolist() == [0, 32768, 32768, 16384, 0, 32768]
    k = np.arange(0, 65536, dtype=np.int64)
    edges = np.concatenate([(k + 0.5) / 65535.0, np.nextafter(((k + 0.5) / 65535.0).astype(np.float32), np.float32(-1))]).astype(np.float32)
    far = np.full(edges.shape, 9.0, np.float32)
    check(pa, ref.records(np.stack([far, edges, far]), 1, final=1), what="every code's rounding boundary in the middle slice")


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(5.0, 1.0), (2.75, 2.75), (0.0, 1e-7), (np.nan, 1.0), (0.0, np.nan), (0.0, np.inf), (-3.5, 9.25e5)])
def test_depth_ranges(gpu, lo, hi):
    check(gpu, random_slices(3, 4099, 77), lo, hi, f"lo {lo} hi {hi}")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride(gpu, monkeypatch, cap):
    """The grid shrunk to 1 and 3 workgroups: 4 * 256 * 3 + 2 pixels take several trips round the stride loop and leave two for the tail lanes."""
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    check(gpu, random_slices(5, 4 * 256 * 3 + 2, 12 + cap), 0.0, 4.0, f"cap {cap}", padding=5)


@pytest.mark.gpu
def test_a_count_past_the_shipped_grid_cap(gpu):
    n = 4 * 256 * _shipped_grid_cap() + 4 * 256 + 3  # one workgroup's worth and three pixels more than the capped grid takes in one trip
    small = random_slices(2, 4099, 31)
    slices = np.ascontiguousarray(np.tile(small, (1, n // 4099 + 1))[:, :n])
    check(gpu, slices, -1.0, 7.5, f"n {n}")


@pytest.mark.gpu
def test_a_callers_stream_and_the_time(gpu):
    import torch

    stream = torch.cuda.Stream()
    slices = random_slices(4, 100003, 41)
    with torch.cuda.stream(stream):
        got, ms = run_slices(gpu, slices, 0.0, 4.0, stream=stream.cuda_stream, timed=True)
    want = sref.gray16(slices, 0.0, 4.0)
    assert all(got[name] == ref.gray16_bytes(want[name]) for name in sref.NAMES)
    assert 0.0 < ms < 100.0


@pytest.mark.gpu
def test_real_sub_frames_side_by_side(gpu):
    """Three pass draws of the headline scene that differ as blur sub-frames do (`_aa_start` 0, 1, 2), at render depth 1: every path through a portal is cut there."""
    pa = gpu
    w, h = 37, 19
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path("portal_in_portal")), device=0, flags=pa.FLAG_PASSES)
    r.set_option("render_depth", 1)
    r.set_option("aa_count", 3)
    slices = []
    for start in range(3):
        r.set_option("aa_start", start)
        slices.append(r.draw_passes(w, h, rgba8=False)["passes"].reshape(-1))
    slices = np.stack(slices)
    lo, hi = float(r.uniform_value("_depth_map_min", w, h)), float(r.uniform_value("_depth_map_max", w, h))
    got = check(pa, slices, lo, hi, "three real sub-frames")
    cut = np.frombuffer(got["cut"], ">u2")
    assert cut.max() > 0 and (cut == 0).any() and len(set(np.frombuffer(got["depth"], ">u2").tolist())) > 10


# ---- the command line -------------------------------------------------------------------------
W, H, FPS, DEPTH, AA, FRAMES = 64, 36, 2, 2, 2, 2


def clip_arguments(pa, blur, more=(), width=W):
    scene_file = pa.scene_path("portal_in_portal")
    clip, _ = pa.Scene.from_file(scene_file).animations()[0]
    return ["render", scene_file, clip, "--width", str(width), "--height", str(H), "--fps", str(FPS), "--asset-root", os.path.dirname(os.path.dirname(scene_file)), "--aa-count", str(AA),
            "--render-depth", str(DEPTH), "--max-frames", str(FRAMES), "--motion-blur-frames", str(blur)] + list(more)


@functools.lru_cache(maxsize=None)
def mirror_images(blur):
    """The pass images of the clip's first FRAMES frames from the same sub-frames drawn through the Python mirror: [{name: (H, W) uint16}]"""
    import portal_amd as pa

    scene_file = pa.scene_path("portal_in_portal")
    scene = pa.Scene.from_file(scene_file)
    clip, duration = scene.animations()[0]
    count = max(1, int(np.float32(duration) * np.float32(FPS)))
    assert count >= FRAMES
    r = pa.SceneRenderer(scene, device=0, flags=pa.FLAG_PASSES, options={"aa_count": AA, "render_depth": DEPTH})
    scene.init_animation(clip)
    r.update(0.0)
    frames = []
    for i in range(FRAMES):
        slices = []
        for j in range(blur):
            r.set_option("aa_start", j)
            r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
            slices.append(r.draw_passes(W, H, rgba8=False)["passes"].reshape(-1))
        lo, hi = float(r.uniform_value("_depth_map_min", W, H)), float(r.uniform_value("_depth_map_max", W, H))
        frames.append({name: image.reshape(H, W) for name, image in sref.gray16(np.stack(slices), lo, hi).items()})
    return frames


def files_of(folder, pattern):
    found = {}
    for at, _, files in os.walk(folder):
        for f in files:
            if re.fullmatch(pattern, f):
                found[f] = open(os.path.join(at, f), "rb").read()
    return found


def assert_pass_files(folder, blur, frames=range(FRAMES), names=sref.NAMES):
    anim = os.path.join(folder, "anim")
    assert sorted(f for f in os.listdir(anim) if not f.startswith("frame_")) == sorted(f"{name}_{i}.png" for name in names for i in frames)
    for i in frames:
        for name in names:
            got, want = ref.read_png_gray16(os.path.join(anim, f"{name}_{i}.png")), mirror_images(blur)[i][name]
            assert np.array_equal(got, want), (blur, name, i, int((got != want).sum()))


@pytest.mark.gpu
@pytest.mark.parametrize("blur,more", [(1, []), (3, []), (3, ["--batch-subframes", "0"]), (17, [])])
def test_render_cli_writes_the_pass_images_of_a_clip(gpu, tmp_path, blur, more):
    """One sub-frame per frame, three in one launch, three drawn one by one, seventeen (beyond the batched launch): the three files of every frame
    decode to the reference's merge of the same sub-frames' records, the frames are the files of the run without the option, and the report
    line is the line of the run without it."""
    pa = gpu
    common = clip_arguments(pa, blur, more)
    both = run_cli(pa, common + ["--out-dir", str(tmp_path / "both"), "--clip-passes", "depth,trips,cut", "--depth-report"])
    report = run_cli(pa, common + ["--out-dir", str(tmp_path / "report"), "--depth-report"])
    run_cli(pa, common + ["--out-dir", str(tmp_path / "plain")])
    assert_pass_files(tmp_path / "both", blur)
    frames = files_of(tmp_path / "both", r"frame_\d+\.png")
    assert len(frames) == FRAMES and frames == files_of(tmp_path / "plain", r"frame_\d+\.png") == files_of(tmp_path / "report", r"frame_\d+\.png")
    assert not files_of(tmp_path / "plain", r"(depth|trips|cut)_\d+\.png") and not files_of(tmp_path / "report", r"(depth|trips|cut)_\d+\.png")
    assert len(LINE.findall(both.stdout)) == 1 and LINE.findall(both.stdout) == LINE.findall(report.stdout), both.stdout + report.stdout
    images = mirror_images(blur)
    assert any(image["cut"].max() > 0 for image in images) and all(len(np.unique(image["depth"])) > 10 for image in images)  # (the case shows something)


@pytest.mark.gpu
def test_render_cli_resumes_shards_and_streams(gpu, tmp_path):
    pa = gpu
    blur = 3
    common = clip_arguments(pa, blur)
    # a subset of the passes; a deleted pass file comes back on the second run, with the frame it belongs to
    out_dir = tmp_path / "resume"
    run_cli(pa, common + ["--out-dir", str(out_dir), "--clip-passes", "cut,depth"])
    assert_pass_files(out_dir, blur, names=("depth", "cut"))
    before = files_of(out_dir, r".*\.png")
    os.remove(out_dir / "anim" / "cut_1.png")
    (out_dir / "anim" / "frame_1.png").write_bytes(b"stale")
    (out_dir / "anim" / "frame_0.png").write_bytes(b"kept")  # frame 0 has all its files: it is not drawn again
    run_cli(pa, common + ["--out-dir", str(out_dir), "--clip-passes", "cut,depth"])
    after = files_of(out_dir, r".*\.png")
    assert after.pop("frame_0.png") == b"kept" and before.pop("frame_0.png")
    assert after == before
    # shard 1 of 2 takes frame 1 only: its frame and its three pass files
    run_cli(pa, common + ["--out-dir", str(tmp_path / "shard"), "--clip-passes", "depth,trips,cut", "--shard", "1/2"])
    assert sorted(os.listdir(tmp_path / "shard" / "anim")) == ["cut_1.png", "depth_1.png", "frame_1.png", "trips_1.png"]
    assert_pass_files(tmp_path / "shard", blur, frames=[1])
    assert (tmp_path / "shard" / "anim" / "frame_1.png").read_bytes() == before["frame_1.png"]
    # a Y4M stream is what it is without the option, and every frame gets its pass files
    run_cli(pa, common + ["--out-dir", str(tmp_path / "y4m"), "--frames", "y4m", "--clip-passes", "depth,trips,cut"])
    run_cli(pa, common + ["--out-dir", str(tmp_path / "y4m_plain"), "--frames", "y4m"])
    streams = files_of(tmp_path / "y4m", r".*\.y4m")
    assert len(streams) == 1 and streams == files_of(tmp_path / "y4m_plain", r".*\.y4m")
    assert_pass_files(tmp_path / "y4m", blur)
    assert not os.path.exists(tmp_path / "y4m_plain" / "anim")


@pytest.mark.gpu
def test_render_frame_cli_writes_the_cut_pass(gpu, tmp_path):
    import math

    pa = gpu
    w, h, depth, aa = 64, 36, 1, 3
    scene_file = pa.scene_path("portal_in_portal")
    common = ["render-frame", scene_file, "--width", str(w), "--height", str(h), "--aa-count", str(aa), "--render-depth", str(depth), "--asset-root", os.path.dirname(os.path.dirname(scene_file))]
    run_cli(pa, common + ["--output", str(tmp_path / "f.png"), "--passes", "cut,trips"])
    run_cli(pa, common + ["--output", str(tmp_path / "plain.png")])
    assert sorted(os.listdir(tmp_path)) == ["f.cut.png", "f.png", "f.trips.png", "plain.png"]
    assert (tmp_path / "f.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    r = pa.SceneRenderer(pa.Scene.from_file(scene_file), device=0, flags=pa.FLAG_PASSES | pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL | pa.FLAG_QUICK_JIT)
    for k, v in (("aa_count", aa), ("render_depth", depth), ("view_angle", 90.0 / 180.0 * math.pi)):
        r.set_option(k, v)
    r.update(0.0)
    rec = r.draw_passes(w, h, rgba8=False)["passes"]
    want = sref.gray16(rec.reshape(1, -1))
    assert np.array_equal(ref.read_png_gray16(str(tmp_path / "f.cut.png")), want["cut"].reshape(h, w))
    assert np.array_equal(ref.read_png_gray16(str(tmp_path / "f.trips.png")), want["trips"].reshape(h, w))
    assert 0 < want["cut"].max() and (want["cut"] == 0).any()


@pytest.mark.gpu
def test_pass_encoder_gpu_writes_the_samples_of_the_host_encoder(gpu, tmp_path):
    """66x36 (a width the GPU deflate takes as 22 RGB pixels), blur 3: every pass file of `--pass-encoder gpu` -- one IDAT, Up-filtered rows --
    decodes to the samples of the host-encoded file, the frames are the same files, and at 64x36 the option is refused before anything is drawn."""
    pa = gpu
    common = clip_arguments(pa, 3, width=66)
    run_cli(pa, common + ["--out-dir", str(tmp_path / "host"), "--clip-passes", "depth,trips,cut", "--pass-encoder", "host"])
    run_cli(pa, common + ["--out-dir", str(tmp_path / "gpu"), "--clip-passes", "depth,trips,cut", "--pass-encoder", "gpu"])
    assert files_of(tmp_path / "host", r"frame_\d+\.png") == files_of(tmp_path / "gpu", r"frame_\d+\.png")
    names = sorted(f"{name}_{i}.png" for name in sref.NAMES for i in range(FRAMES))
    assert sorted(files_of(tmp_path / "gpu", r"(depth|trips|cut)_\d+\.png")) == names == sorted(files_of(tmp_path / "host", r"(depth|trips|cut)_\d+\.png"))
    shown = set()
    for f in names:
        host, made = ref.read_png_gray16(str(tmp_path / "host" / "anim" / f)), sref.read_png_gray16_up(str(tmp_path / "gpu" / "anim" / f))
        assert host.shape == (H, 66) and np.array_equal(host, made), f
        shown.add(len(np.unique(host)) > 2)
    assert True in shown
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    refused = subprocess.run(["timeout", "-k", "10", "60", exe] + clip_arguments(pa, 3) + ["--out-dir", str(tmp_path / "no"), "--clip-passes", "cut", "--pass-encoder", "gpu"], capture_output=True, text=True)
    assert refused.returncode == 2 and "multiple of 3" in refused.stderr and not os.path.exists(tmp_path / "no")
