"""`portal-amd render`: the paths of the clip loop that the end-to-end tests of test_gpu_parity.py and test_yuv_output.py do not reach --
scheduling options that must not change a byte, the unblurred PNG path, two clips in one run, stereo, a resumed run.  Everything is
`basics` at 64x36, aa 2, depth 12, without an ffmpeg on the PATH (frames are parked in <clip>.frames)."""
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H = 64, 36
CLIP = "anim.4.portals"  # 3 s: six frames at --fps 2


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


def _path_without_ffmpeg():
    return os.pathsep.join(d for d in os.environ.get("PATH", "").split(os.pathsep) if d and not os.path.exists(os.path.join(d, "ffmpeg")))


def _render(pa, out_dir, clips, extra, width=W):
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    scene = pa.scene_path("basics")
    cmd = [exe, "render", scene] + ([clips] if clips else []) + ["--width", str(width), "--height", str(H), "--aa-count", "2", "--render-depth", "12", "--out-dir", str(out_dir),
                                                                 "--asset-root", os.path.dirname(os.path.dirname(scene))] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PATH=_path_without_ffmpeg()))
    assert out.returncode == 0, out.stderr + out.stdout
    return out


def _clip_files(out_dir, clip, count):
    """Every file a PNG clip leaves behind, as bytes: the parked frames and both stills."""
    video = out_dir / "video" / "basics"
    assert sorted(os.listdir(video / f"{clip}.frames")) == sorted(f"frame_{i}.png" for i in range(count))
    files = {f"frame_{i}.png": (video / f"{clip}.frames" / f"frame_{i}.png").read_bytes() for i in range(count)}
    for still in ("start", "end"):
        files[still] = (video / f"{clip}.{still}.png").read_bytes()
    return files


def _mirror_clip(pa, scene, r, clip, fps, blur, width=W):
    """One clip through the Python mirror, as `render` walks it: (frames, first sub-frame, last sub-frame)."""
    from oracle import postprocess as pp

    duration = dict(scene.animations())[clip]
    count = max(1, int(np.float32(duration) * np.float32(fps)))
    scene.init_animation(clip)
    r.update(0.0)
    frames, first, last = [], None, None
    for i in range(count):
        subs = []
        for j in range(blur):
            r.set_option("aa_start", j)
            r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
            subs.append(r.draw(width, H)["rgba8"])
        first = subs[0] if first is None else first
        last = subs[-1]
        frames.append(pp.average_images(subs) if blur > 1 else subs[0])
    return frames, first, last


def _mirror(pa, options=None):
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    r = pa.SceneRenderer(scene, device=0, options=options)
    r.set_option("aa_count", 2)
    r.set_option("render_depth", 12)
    return scene, r


def _assert_clip_is(pa, out_dir, clip, frames, first, last):
    video = out_dir / "video" / "basics"
    assert sorted(os.listdir(video / f"{clip}.frames")) == sorted(f"frame_{i}.png" for i in range(len(frames)))
    for i, want in enumerate(frames):
        assert np.array_equal(pa.png_read(str(video / f"{clip}.frames" / f"frame_{i}.png")), want), (clip, i)
    assert np.array_equal(pa.png_read(str(video / f"{clip}.start.png")), first), clip
    assert np.array_equal(pa.png_read(str(video / f"{clip}.end.png")), last), clip


BLURRED = ["--fps", "2", "--motion-blur-frames", "3"]


@pytest.fixture(scope="module")
def default_png(gpu, tmp_path_factory):
    out_dir = tmp_path_factory.mktemp("default_png")
    _render(gpu, out_dir, CLIP, BLURRED)
    return _clip_files(out_dir, CLIP, 6)


@pytest.fixture(scope="module")
def default_y4m(gpu, tmp_path_factory):
    out_dir = tmp_path_factory.mktemp("default_y4m")
    _render(gpu, out_dir, CLIP, BLURRED + ["--frames", "y4m"])
    return (out_dir / "video" / "basics" / f"{CLIP}.y4m").read_bytes()


@pytest.mark.parametrize("extra", [["--batch-subframes", "0"], ["--timing"], ["--specialize", "1"], ["--specialize", "0"]], ids=" ".join)
def test_scheduling_options_change_no_png_byte(gpu, tmp_path, default_png, extra):
    """One launch per frame or one per sub-frame, waiting for every kernel, a clip-constant kernel or none: how a clip is scheduled and built
    changes no byte of its frames and stills."""
    _render(gpu, tmp_path, CLIP, BLURRED + extra)
    got = _clip_files(tmp_path, CLIP, 6)
    assert sorted(got) == sorted(default_png)
    for name in got:
        assert got[name] == default_png[name], name


@pytest.mark.parametrize("extra", [["--batch-subframes", "0"], ["--specialize", "1"]], ids=" ".join)
def test_scheduling_options_change_no_stream_byte(gpu, tmp_path, default_y4m, extra):
    _render(gpu, tmp_path, CLIP, BLURRED + ["--frames", "y4m"] + extra)
    assert (tmp_path / "video" / "basics" / f"{CLIP}.y4m").read_bytes() == default_y4m
    assert len(default_y4m) > 6 * gpu.yuv420p10_frame_bytes(W, H)


def test_blur_above_the_batching_range_draws_one_by_one(gpu, tmp_path):
    """--motion-blur-frames 17 is past the 2..16 the slices entry takes: a draw per sub-frame plus the averaging kernel, without any option."""
    _render(gpu, tmp_path, CLIP, ["--fps", "2", "--motion-blur-frames", "17"])
    scene, r = _mirror(gpu)
    _assert_clip_is(gpu, tmp_path, CLIP, *_mirror_clip(gpu, scene, r, CLIP, 2, 17))


def test_unblurred_frames_are_the_draws(gpu, tmp_path):
    """--motion-blur-frames 1: no averaging kernel, the draw lands in the frame that is downloaded."""
    _render(gpu, tmp_path, CLIP, ["--fps", "2", "--motion-blur-frames", "1"])
    scene, r = _mirror(gpu)
    _assert_clip_is(gpu, tmp_path, CLIP, *_mirror_clip(gpu, scene, r, CLIP, 2, 1))


def test_two_clips_in_one_run(gpu, tmp_path):
    """No clip name: every clip of the scene, one after the other on the same scene and renderer (the first renderer is created on the
    first clip's clip-constant kernel, the second clip's is compiled ahead by a worker); 15 and 3 frames."""
    out = _render(gpu, tmp_path, None, ["--fps", "1", "--motion-blur-frames", "1", "--specialize", "1"])
    scene, r = _mirror(gpu)
    clips = scene.animations()
    assert [c for c, _ in clips] == ["anim.2.portals", CLIP]
    for k, (clip, _) in enumerate(clips):
        assert f"Rendering animation {clip}, {k + 1}/2" in out.stdout
        frames, first, last = _mirror_clip(gpu, scene, r, clip, 1, 1)
        assert len(frames) == (15, 3)[k]
        _assert_clip_is(gpu, tmp_path, clip, frames, first, last)


def test_stereo_frames_are_side_by_side(gpu, tmp_path):
    _render(gpu, tmp_path, CLIP, ["--fps", "2", "--motion-blur-frames", "1", "--stereoimage"])
    scene, r = _mirror(gpu, options={"draw_side_by_side": 1})
    frames, first, last = _mirror_clip(gpu, scene, r, CLIP, 2, 1, width=2 * W)
    assert frames[0].shape == (H, 2 * W, 4)
    _assert_clip_is(gpu, tmp_path, CLIP, frames, first, last)


@pytest.mark.parametrize("extra", [[], ["--no-skip-existing"]], ids=["default", "--no-skip-existing"])
def test_resumed_run_equals_an_uninterrupted_one(gpu, tmp_path, default_png, extra):
    """--max-frames 2 leaves two frames in anim/; the second run finds them, steps the camera through them without drawing and goes on:
    the clip it parks is the uninterrupted run's, byte for byte, and the two frames were not written again."""
    _render(gpu, tmp_path, CLIP, BLURRED + extra + ["--max-frames", "2"])
    anim = tmp_path / "anim"
    assert sorted(os.listdir(anim)) == ["frame_0.png", "frame_1.png"]
    before = {name: ((anim / name).read_bytes(), os.stat(anim / name).st_mtime_ns) for name in os.listdir(anim)}
    _render(gpu, tmp_path, CLIP, BLURRED + extra)
    got = _clip_files(tmp_path, CLIP, 6)
    frames = tmp_path / "video" / "basics" / f"{CLIP}.frames"
    for name, (data, mtime) in before.items():
        assert got[name] == data and os.stat(frames / name).st_mtime_ns == mtime, name
    for name in got:
        assert got[name] == default_png[name], name


# ---- a frame form and the pass images in the same clip: two rings on the card freed by one event, two kinds of job in one pool ----
WP = 66  # (the GPU pass encoder takes a row as W / 3 RGB pixels)
FORMS = {"png": [], "png-gpu-dynamic": ["--png-encoder", "gpu", "--png-codes", "dynamic"], "png16-gpu": ["--png-depth", "16", "--png16-encoder", "gpu"], "y4m": ["--frames", "y4m"]}
PASSES = ["--clip-passes", "depth,trips,cut"]
PASS_NAMES = sorted(f"{name}_{i}.png" for name in ("depth", "trips", "cut") for i in range(6))


def _form_files(out_dir, extra):
    """What the frame form of a whole clip leaves behind, as bytes: the parked frames or the stream, and both stills."""
    if "y4m" not in extra:
        return _clip_files(out_dir, CLIP, 6)
    video = out_dir / "video" / "basics"
    return {name: (video / f"{CLIP}.{name}").read_bytes() for name in ("y4m", "start.png", "end.png")}


def _parked_passes(out_dir):
    parked = out_dir / "video" / "basics" / f"{CLIP}.passes"
    assert sorted(os.listdir(parked)) == PASS_NAMES
    return parked


@pytest.fixture(scope="module")
def png_with_passes(gpu, tmp_path_factory):
    """The form without an option beside the GPU-encoded pass images: (its files, the folder of its pass files)."""
    out_dir = tmp_path_factory.mktemp("png_with_passes")
    _render(gpu, out_dir, CLIP, BLURRED + PASSES + ["--pass-encoder", "gpu"], width=WP)
    return _form_files(out_dir, []), _parked_passes(out_dir)


@pytest.mark.parametrize("form", list(FORMS))
def test_frame_forms_and_pass_images_leave_each_other_alone(gpu, tmp_path, png_with_passes, form):
    """Every frame form with `--clip-passes depth,trips,cut --pass-encoder gpu` (for the GPU forms: two deflates per frame on one stream):
    the frames or the stream and both stills are byte for byte those of the form alone, and the pass files are byte for byte those written
    beside the form without an option."""
    extra = FORMS[form]
    _render(gpu, tmp_path / "alone", CLIP, BLURRED + extra, width=WP)
    alone = _form_files(tmp_path / "alone", extra)
    both, parked = png_with_passes
    if extra:
        _render(gpu, tmp_path / "both", CLIP, BLURRED + extra + PASSES + ["--pass-encoder", "gpu"], width=WP)
        both, parked = _form_files(tmp_path / "both", extra), _parked_passes(tmp_path / "both")
    assert sorted(both) == sorted(alone)
    for name in alone:
        assert both[name] == alone[name], (form, name)
    for name in PASS_NAMES:
        assert (parked / name).read_bytes() == (png_with_passes[1] / name).read_bytes(), (form, name)


def test_host_and_gpu_pass_encoders_write_the_same_samples_beside_the_frames(gpu, tmp_path, png_with_passes):
    from tests import pass_reference as ref
    from tests import pass_slices_reference as sref

    _render(gpu, tmp_path, CLIP, BLURRED + PASSES + ["--pass-encoder", "host"], width=WP)
    assert _form_files(tmp_path, []) == png_with_passes[0]
    host, shown = _parked_passes(tmp_path), set()
    for name in PASS_NAMES:
        want, made = ref.read_png_gray16(str(host / name)), sref.read_png_gray16_up(str(png_with_passes[1] / name))
        assert want.shape == (H, WP) and np.array_equal(want, made), name
        shown.add(len(np.unique(want)) > 2)
    assert True in shown
