"""Trace passes on the MI355X: the records a pass draw stores against the host build of the same source (byte for byte), the launch forms
(sharded, in place, slices), the two post-process kernels against tests/pass_reference.py, and the command line end to end.
Every comparison is exact: the record holds integers and one float minimum.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pass_reference as ref
from tests.test_passes import host_passes
from tests.yuv_harness import GUARD, KNOB, _c_getenv, _path_without_ffmpeg, gpu  # noqa: F401 (gpu: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 37, 19
SCENES = ("basics", "monoportal", "portal_in_portal")
CASES = [(aa, depth) for aa in (1, 3) for depth in (1, 2, 3, 40)]  # `_aa_start` 2 throughout, like the CPU leg


@functools.lru_cache(maxsize=None)
def host_records(scene_name, w, h, depth, aa, aa_start):
    """The host build's records of a case, computed once for every GPU build that is compared with them."""
    import portal_amd as pa

    return host_passes(pa, scene_name, w, h, depth, aa, aa_start=aa_start)


@functools.lru_cache(maxsize=None)
def renderer(scene_name, flags):
    import portal_amd as pa

    return pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene_name)), device=0, flags=flags)


def set_case(r, depth, aa, aa_start=2):
    for k, v in (("render_depth", depth), ("aa_count", aa), ("aa_start", aa_start)):
        r.set_option(k, v)


def same_records(got, want, what):
    if got.tobytes() == want.tobytes():
        return
    bad = np.argwhere(got != want)
    y, x = bad[0]
    pytest.fail(f"{what}: {len(bad)} of {got.size} records differ, first at x={x} y={y}: got {got[y, x]}, want {want[y, x]}")


# ---------------------------------------------------------------------------------------------
# 1. - 3. the records, the colours, the counter
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("build", ["shipped", "unspecialised"])
@pytest.mark.parametrize("scene_name", SCENES)
def test_records_equal_the_host_build(gpu, scene_name, build):
    """37x19 (a partial last tile in both directions), aa 1 and 3 from `_aa_start` 2, render depth 1, 2, 3 and 40: the records of the GPU pass
    draw are the host build's, byte for byte, in the build render-frame ships (the scene state baked in) and in the un-specialised one; and
    the colours of a pass draw are those of a plain draw of the same renderer and of a renderer that never heard of the flag."""
    pa = gpu
    spec = pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL if build == "shipped" else 0
    r, plain = renderer(scene_name, spec | pa.FLAG_PASSES), renderer(scene_name, spec)
    assert "#define PTL_PASSES 1\n" in r.kernel_source() and "PTL_PASSES" not in plain.kernel_source()
    for aa, depth in CASES:
        set_case(r, depth, aa)
        set_case(plain, depth, aa)
        got = r.draw_passes(W, H, rgba8=True, rgba32f=True)
        want = host_records(scene_name, W, H, depth, aa, 2)
        same_records(got["passes"], want["passes"], f"{scene_name} {build} aa {aa} depth {depth}")
        assert np.array_equal(got["rgba8"], want["rgba8"])
        for other in (r.draw(W, H, rgba8=True, rgba32f=True), plain.draw(W, H, rgba8=True, rgba32f=True)):  # (a plain draw of a pass kernel stores no records)
            assert np.array_equal(got["rgba8"], other["rgba8"]) and got["rgba32f"].tobytes() == other["rgba32f"].tobytes()
    res = r.resources()
    print(scene_name, build, "pass build", res, "plain build", plain.resources())
    assert res["scratch_bytes"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name", SCENES)
def test_trips_add_up_to_the_segment_counter(gpu, scene_name):
    pa = gpu
    r = renderer(scene_name, pa.FLAG_PASSES | pa.FLAG_COUNT_SEGMENTS)
    for aa, depth in ((1, 3), (3, 40)):
        set_case(r, depth, aa)
        got = r.draw_passes(W, H, rgba8=False, segments=True)
        assert got["segments"] == int(got["passes"]["trips"].sum()) > 0
        same_records(got["passes"], host_records(scene_name, W, H, depth, aa, 2)["passes"], f"{scene_name} counting build")


# ---------------------------------------------------------------------------------------------
# 4. - 5. the launch forms
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_sharded_frames_assemble_to_the_unsharded_records(gpu):
    """37x45 = six row blocks, the last of five rows; rb_stride 3, every phase.  Packed shards are put back block by block; in-place shards
    are drawn into one full-frame buffer, whose guard bytes and untouched rows must stay what they were."""
    import torch

    pa = gpu
    w, h, stride = 37, 45, 3
    r = renderer("portal_in_portal", pa.FLAG_PASSES)
    set_case(r, 40, 3)
    whole = r.draw_passes(w, h, rgba8=False)["passes"]
    same_records(whole, host_records("portal_in_portal", w, h, 40, 3, 2)["passes"], "unsharded 37x45")
    packed = np.zeros((h, w), pa.PASS_RECORD)
    for phase in range(stride):
        shard = r.draw_passes(w, h, rgba8=False, rb_phase=phase, rb_stride=stride)["passes"]
        blocks = list(range(phase, (h + 7) // 8, stride))
        assert shard.shape == (sum(min(8, h - 8 * b) for b in blocks), w)
        at = 0
        for b in blocks:
            rows = min(8, h - 8 * b)
            packed[8 * b: 8 * b + rows] = shard[at: at + rows]
            at += rows
    same_records(packed, whole, "packed shards")
    nbytes = pa.pass_record_bytes(w, h)
    buf = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    for phase in range(stride):
        frame = pa.Frame(w, h, phase, stride, 1)
        r.draw_passes_device(frame, buf.data_ptr(), nbytes, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        seen = buf.cpu().numpy()
        assert (seen[nbytes:] == GUARD).all(), "written behind the frame"
        drawn = seen[:nbytes].view(pa.PASS_RECORD).reshape(h, w)
        for b in range((h + 7) // 8):
            rows = slice(8 * b, min(h, 8 * b + 8))
            if b % stride <= phase:
                same_records(drawn[rows], whole[rows], f"in place, block {b} after phase {phase}")
            else:
                assert (seen[:nbytes].reshape(h, w * 16)[rows] == GUARD).all(), f"block {b} touched before its phase"
    small = torch.zeros(nbytes - 16, dtype=torch.uint8, device="cuda")
    with pytest.raises(pa.PortalError, match="16 bytes per pixel"):  # an in-place shard needs the whole frame's room
        r.draw_passes_device(pa.Frame(w, h, 0, stride, 1), small.data_ptr(), nbytes - 16)


@pytest.mark.gpu
def test_slices_entry_equals_three_single_draws(gpu):
    """One launch over three staged slices with differing uniform blocks (`_aa_start`, `_aa_count`, `_ray_tracing_depth`): slice z lands
    behind slice z - 1, padded to slice_pixels, and equals the single draw of the same state."""
    import torch

    pa = gpu
    w, h = W, H
    r = renderer("portal_in_portal", pa.FLAG_PASSES | pa.FLAG_SLICES)
    states = [(40, 1, 0), (2, 3, 2), (3, 2, 5)]  # render depth, aa, aa start
    singles = []
    for depth, aa, start in states:
        set_case(r, depth, aa, start)
        singles.append(r.draw_passes(w, h, rgba8=True))
        same_records(singles[-1]["passes"], host_records("portal_in_portal", w, h, depth, aa, start)["passes"], "single draw of a slices module")
    slice_pixels = w * h + 11  # room between the slices, which must stay untouched
    frame = pa.Frame(w, h, 0, 1, 0)
    nbytes = 16 * (2 * slice_pixels + w * h)
    records = torch.full((nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    colours = torch.zeros((3 * slice_pixels * 4,), dtype=torch.uint8, device="cuda")
    for z, (depth, aa, start) in enumerate(states):
        set_case(r, depth, aa, start)
        r.stage_slice(frame, z)
    r.draw_slices_passes(frame, 3, records.data_ptr(), nbytes, out_rgba8=colours.data_ptr(), slice_pixels=slice_pixels, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    seen, seen8 = records.cpu().numpy(), colours.cpu().numpy()
    assert (seen[nbytes:] == GUARD).all()
    for z in range(3):
        at = 16 * z * slice_pixels
        same_records(seen[at: at + 16 * w * h].view(pa.PASS_RECORD).reshape(h, w), singles[z]["passes"], f"slice {z}")
        assert np.array_equal(seen8[4 * z * slice_pixels: 4 * (z * slice_pixels + w * h)].reshape(h, w, 4), singles[z]["rgba8"])
        if z < 2:
            assert (seen[at + 16 * w * h: at + 16 * slice_pixels] == GUARD).all(), "written between two slices"
    assert not np.array_equal(singles[0]["passes"], singles[1]["passes"])


# ---------------------------------------------------------------------------------------------
# 6. ptl_pass_stats
# ---------------------------------------------------------------------------------------------
def synthetic(n, seed, exhausted="some"):
    """n records that exercise every field: trips around the last bin and far beyond it, saturated counts, depths of both signs, zeros,
    infinities and a NaN."""
    rng = np.random.default_rng(seed)
    trips = rng.choice(np.array([0, 1, 2, 7, 40, 254, 255, 256, 300, 70000], np.uint32), n)
    depth = rng.choice(np.array([-3.5, -1e-30, -0.0, 0.0, 1e-30, 1.0, 2.75, 9.25e5, np.inf, -np.inf, np.nan], np.float32), n)
    final, escaped = rng.integers(0, 5, n), rng.integers(0, 4, n)
    outside = rng.integers(0, 3, n)
    gone = {"some": rng.integers(0, 3, n) * (rng.random(n) < 0.3), "all": rng.integers(1, 4, n), "none": np.zeros(n, np.int64)}[exhausted]
    if n > 3:
        final[0], escaped[1], gone[2], outside[3] = 65535, 65535, 65535 if exhausted != "none" else 0, 65535
    return ref.records(depth, trips, final, escaped, gone, outside)


def run_stats(pa, launches):
    """launches: [(records, slot)] added into one zeroed block -> (block as a structured scalar, per_launch counters)"""
    import torch

    block = torch.zeros(pa.PASS_STATS_BLOCK.itemsize + 64, dtype=torch.uint8, device="cuda")
    block[pa.PASS_STATS_BLOCK.itemsize:] = GUARD
    per_launch = torch.zeros(4, dtype=torch.int64, device="cuda")
    for rec, slot in launches:
        dev = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1).copy()).cuda()
        assert dev.data_ptr() % 16 == 0
        pa.pass_stats_device(dev.data_ptr(), rec.size, block.data_ptr(), per_launch.data_ptr(), slot, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    seen = block.cpu().numpy()
    assert (seen[pa.PASS_STATS_BLOCK.itemsize:] == GUARD).all(), "written behind the block"
    return seen[: pa.PASS_STATS_BLOCK.itemsize].view(pa.PASS_STATS_BLOCK)[0], per_launch.cpu().numpy().astype(np.uint64)


def check_stats(pa, launches, what):
    got, got_per_launch = run_stats(pa, launches)
    want, want_per_launch = ref.empty_stats(), np.zeros(4, np.uint64)
    for rec, slot in launches:
        ref.add_stats(want, rec, want_per_launch, slot)
    for name in ("pixels", "paths", "trips", "final_paths", "escaped", "exhausted", "outside", "exhausted_pixels", "max_trips", "depth_max_key", "depth_min_key_inv"):
        assert int(got[name]) == int(want[name]), (what, name, int(got[name]), int(want[name]))
    assert np.array_equal(got["trips_histogram"], want["trips_histogram"]), what
    assert int(got["reserved"]) == 0 and np.array_equal(got_per_launch, want_per_launch), what
    assert pa.pass_stats_depth_range(np.array([got])) == ref.depth_range(want)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 513, 256 * 7 - 1, 256 * 7 + 1])
def test_pass_stats_at_any_count(gpu, n):
    check_stats(gpu, [(synthetic(n, n), 0)], f"n = {n}")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 3])
def test_pass_stats_grid_stride(gpu, monkeypatch, cap):
    """The grid shrunk to 1 and 3 workgroups: 256 * 9 + 1 records take ten and four trips round the stride loop, the last one a single lane."""
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    check_stats(gpu, [(synthetic(256 * 9 + 1, 90 + cap), 0)], f"cap {cap}")


@pytest.mark.gpu
def test_pass_stats_edges(gpu):
    pa = gpu
    tail = check_stats(pa, [(ref.records([1.0, 2.0, 3.0, 4.0], [254, 255, 256, 70000], final=1), 0)], "the last bin")
    assert tail["trips_histogram"][254] == 1 and tail["trips_histogram"][255] == 3 and tail["max_trips"] == 70000
    everything = check_stats(pa, [(synthetic(1000, 5, "all"), 0)], "all exhausted")
    assert everything["exhausted_pixels"] == everything["pixels"] == 1000
    nothing = check_stats(pa, [(synthetic(1000, 6, "none"), 0)], "none exhausted")
    assert nothing["exhausted_pixels"] == 0 and nothing["exhausted"] == 0
    signs = check_stats(pa, [(ref.records([-2.5, -0.0, 0.0, np.inf, -np.inf, np.nan], 1, final=1), 0)], "depth signs")
    assert pa.pass_stats_depth_range(np.array([signs])) == (-2.5, 0.0)
    none = check_stats(pa, [(ref.records([np.inf, np.inf], 1), 0)], "no depth at all")
    assert pa.pass_stats_depth_range(np.array([none])) is None and none["depth_max_key"] == 0 and none["depth_min_key_inv"] == 0


@pytest.mark.gpu
def test_pass_stats_accumulates_over_launches(gpu):
    """Two launches into one block, their exhausted paths in per_launch[0] and per_launch[1]; a third into slot 1 again."""
    a, b, c = synthetic(700, 1), synthetic(300, 2, "all"), synthetic(65, 3)
    got = check_stats(gpu, [(a, 0), (b, 1), (c, 1)], "three launches")
    assert got["pixels"] == 1065


# ---------------------------------------------------------------------------------------------
# 7. ptl_passes_to_gray16
# ---------------------------------------------------------------------------------------------
def run_gray16(pa, rec, which, lo, hi, offset=0):
    import torch

    rec = np.ascontiguousarray(rec).reshape(-1)
    dev = torch.from_numpy(rec.view(np.uint8).copy()).cuda()
    out = torch.full((offset + 2 * rec.size + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 16 == 0 and out.data_ptr() % 256 == 0 and offset % 16 == 0
    pa.passes_to_gray16_device(dev.data_ptr(), rec.size, out.data_ptr() + offset, which, lo, hi, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    seen = out.cpu().numpy()
    assert (seen[:offset] == GUARD).all() and (seen[offset + 2 * rec.size:] == GUARD).all(), "written outside the rows"
    return seen[offset: offset + 2 * rec.size].tobytes()


def check_gray16(pa, rec, lo, hi, what):
    for which in (ref.DEPTH, ref.TRIPS):
        got, want = run_gray16(pa, rec, which, lo, hi), ref.gray16_bytes(ref.gray16(rec, which, lo, hi))
        if got != want:
            g, r = np.frombuffer(got, ">u2"), np.frombuffer(want, ">u2")
            bad = np.flatnonzero(g != r)
            pytest.fail(f"{what} which={which}: {len(bad)} of {g.size} samples differ, first at {bad[0]}: got {g[bad[0]]}, want {r[bad[0]]} for {np.asarray(rec).reshape(-1)[bad[0]]}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (3, 1), (37, 19), (70, 37), (256, 6), (257, 5)])
def test_gray16_at_any_frame_size(gpu, w, h):
    """Rows are packed, so only w * h matters: 37x19 and 257x5 leave records for the tail lanes, and every wave but the first starts mid-row."""
    rec = synthetic(w * h, w * 1000 + h)
    check_gray16(gpu, rec, -1.0, 7.5, f"{w}x{h}")
    assert len(run_gray16(gpu, rec, ref.TRIPS, 0.0, 1.0, offset=32)) == 2 * w * h


@pytest.mark.gpu
def test_gray16_ranges_and_rounding(gpu):
    pa = gpu
    k = np.arange(0, 65536, dtype=np.int64)
    on_boundaries = np.concatenate([(k + 0.5) / 65535.0, k / 65535.0, np.nextafter(((k + 0.5) / 65535.0).astype(np.float32), np.float32(2)),
                                    np.nextafter(((k + 0.5) / 65535.0).astype(np.float32), np.float32(-1))]).astype(np.float32)
    rec = ref.records(on_boundaries, 1, final=1)
    check_gray16(pa, rec, 0.0, 1.0, "every code's rounding boundary, and its neighbours")
    assert len(set(ref.gray16(rec, ref.DEPTH, 0.0, 1.0).tolist())) == 65536
    check_gray16(pa, ref.records(on_boundaries * np.float32(65535.0), 1, final=1), 0.0, 65535.0, "the same through a real division")
    every = synthetic(4099, 77)
    for lo, hi in ((2.75, 2.75), (5.0, 1.0), (0.0, 1e-7), (-3.5, 9.25e5), (0.0, np.inf), (np.nan, 1.0)):
        check_gray16(pa, every, lo, hi, f"lo {lo} hi {hi}")
    flat = ref.gray16(ref.records([2.0, 2.75, 3.0], 1, final=1), ref.DEPTH, 2.75, 2.75)
    assert flat.tolist() == [0, 0, 65535]  # lo == hi: the divisor is 1e-6, a step at lo
    no_final = ref.records([1.0, 1.0], [3, 70000], final=[0, 1])
    assert np.frombuffer(run_gray16(pa, no_final, ref.DEPTH, 0.0, 2.0), ">u2").tolist() == [0, 32768]
    assert np.frombuffer(run_gray16(pa, no_final, ref.TRIPS, 0.0, 2.0), ">u2").tolist() == [3, 65535]


@pytest.mark.gpu
def test_gray16_grid_stride(gpu, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    check_gray16(gpu, synthetic(4 * 256 * 3 + 2, 12), 0.0, 4.0, "one workgroup, three trips and a tail")


# ---------------------------------------------------------------------------------------------
# 8. the command line
# ---------------------------------------------------------------------------------------------
LINE = re.compile(r"^Paths: (\d+) traced, (\d+) cut at depth (\d+) \(([\d.]+) %\) in (\d+) pixels; deepest pixel (\d+) trips; depth (\S+) … (\S+?)(;.*)?$", re.M)


def run_cli(pa, arguments, limit=300):
    """One child under a time limit of its own, no ffmpeg on its PATH (a clip's frames stay where they were written)."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run(["timeout", "-k", "10", str(limit), exe] + arguments, capture_output=True, text=True, timeout=limit + 100, env=dict(os.environ, PATH=_path_without_ffmpeg()), cwd=ROOT)
    assert out.returncode == 0, out.stderr + out.stdout
    return out


def line_of(stats, depth):
    traced = stats["paths"] - stats["outside"]
    lo, hi = ref.depth_range(stats)
    return (str(traced), str(stats["exhausted"]), str(depth), "%.2f" % (100.0 * stats["exhausted"] / traced), str(stats["exhausted_pixels"]), str(stats["max_trips"]), "%g" % lo, "%g" % hi)


@pytest.mark.gpu
def test_render_frame_cli_writes_the_passes_and_the_report(gpu, tmp_path):
    """`render-frame --passes depth,trips --depth-report` at 64x36, depth 1 (every path through a portal is lost there): the two files decode to the
    records of the same state drawn through the Python mirror, the line's numbers are the statistics of those records, and the frame itself
    is the file the call writes without the options."""
    import math

    pa = gpu
    w, h, depth, aa = 64, 36, 1, 3
    scene_file = pa.scene_path("portal_in_portal")
    common = ["render-frame", scene_file, "--width", str(w), "--height", str(h), "--aa-count", str(aa), "--render-depth", str(depth), "--asset-root", os.path.dirname(os.path.dirname(scene_file))]
    out = run_cli(pa, common + ["--output", str(tmp_path / "f.png"), "--passes", "depth,trips", "--depth-report"])
    run_cli(pa, common + ["--output", str(tmp_path / "plain.png")])
    assert sorted(os.listdir(tmp_path)) == ["f.depth.png", "f.png", "f.trips.png", "plain.png"]
    assert (tmp_path / "f.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    scene = pa.Scene.from_file(scene_file)
    r = pa.SceneRenderer(scene, device=0, flags=pa.FLAG_PASSES | pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL | pa.FLAG_QUICK_JIT)
    for k, v in (("aa_count", aa), ("render_depth", depth), ("view_angle", 90.0 / 180.0 * math.pi)):
        r.set_option(k, v)
    r.update(0.0)
    rec = r.draw_passes(w, h, rgba8=False)["passes"]
    lo, hi = float(r.uniform_value("_depth_map_min", w, h)), float(r.uniform_value("_depth_map_max", w, h))
    assert np.array_equal(ref.read_png_gray16(str(tmp_path / "f.trips.png")), ref.gray16(rec, ref.TRIPS))
    assert np.array_equal(ref.read_png_gray16(str(tmp_path / "f.depth.png")), ref.gray16(rec, ref.DEPTH, lo, hi))
    stats = ref.add_stats(ref.empty_stats(), rec)
    found = LINE.findall(out.stdout)
    assert len(found) == 1 and found[0][:8] == line_of(stats, depth) and found[0][8] == "", out.stdout
    assert stats["exhausted"] > 0 and stats["paths"] == w * h * aa
    only = run_cli(pa, common + ["--output", str(tmp_path / "g.png"), "--passes", "trips"])  # one pass, no report
    assert os.path.exists(tmp_path / "g.trips.png") and not os.path.exists(tmp_path / "g.depth.png") and not LINE.search(only.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("blur,more", [(1, []), (3, []), (3, ["--batch-subframes", "0"])])
def test_render_cli_reports_a_clip(gpu, tmp_path, blur, more):
    """`render ... --depth-report --max-frames 2` at 64x36 with one sub-frame per frame, with three in one launch, and with three drawn one by
    one: one line per clip whose totals are the sum over the same sub-frames drawn through the Python mirror, and whose worst frame is the one
    with the most exhausted paths.  The frames are the files the call writes without the option."""
    pa = gpu
    w, h, fps, depth, aa, frames = 64, 36, 2, 2, 2, 2
    scene_file = pa.scene_path("portal_in_portal")
    clip, duration = pa.Scene.from_file(scene_file).animations()[0]
    count = max(1, int(np.float32(duration) * np.float32(fps)))
    assert count >= frames
    common = ["render", scene_file, clip, "--width", str(w), "--height", str(h), "--fps", str(fps), "--asset-root", os.path.dirname(os.path.dirname(scene_file)), "--aa-count", str(aa),
              "--render-depth", str(depth), "--max-frames", str(frames), "--motion-blur-frames", str(blur)] + more
    out = run_cli(pa, common + ["--out-dir", str(tmp_path / "report"), "--depth-report"])
    run_cli(pa, common + ["--out-dir", str(tmp_path / "plain")])
    scene = pa.Scene.from_file(scene_file)
    r = pa.SceneRenderer(scene, device=0, flags=pa.FLAG_PASSES, options={"aa_count": aa, "render_depth": depth})
    scene.init_animation(clip)
    r.update(0.0)
    stats, cut = ref.empty_stats(), np.zeros(count, np.uint64)
    for i in range(frames):
        for j in range(blur):
            r.set_option("aa_start", j)
            r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
            ref.add_stats(stats, r.draw_passes(w, h, rgba8=False)["passes"], cut, i)
    found = LINE.findall(out.stdout)
    assert len(found) == 1 and found[0][:8] == line_of(stats, depth), out.stdout
    worst = int(np.argmax(cut))
    assert found[0][8] == f"; `{clip}`: {frames * blur} sub-frames, worst frame {worst} ({int(cut[worst])} paths cut)", out.stdout
    assert stats["pixels"] == w * h * frames * blur and stats["exhausted"] > 0
    written = {}
    for run in ("report", "plain"):
        for folder, _, files in os.walk(tmp_path / run):
            for f in files:
                if re.fullmatch(r"frame_\d+\.png", f):
                    written.setdefault(run, {})[f] = open(os.path.join(folder, f), "rb").read()
    assert written["report"] == written["plain"] and len(written["plain"]) == frames
