"""Trace passes on the CPU: the generator's flag, the record of the host build of the pass source against the numpy oracle, the 16-bit
greyscale writer, the parse-time refusals of the CLI.  (The gfx950 leg is tests/test_gpu_passes.py.)

The record (include/portal_amd.h `ptl_pass_record`) holds integers and one float minimum, so every comparison here is exact.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import pass_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["basics", "mobius_monoportal", "monoportal", "portal_in_portal", "triple_portal"]  # the five files of scenes/
W, H = 37, 19  # not a multiple of the 32x8 block: the last tile of every row block is partial


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------
# 1. the generator
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", SCENES)
def test_flag_is_in_the_text_and_nowhere_else(pa, scene_name):
    """Without bit 30 the source does not know the feature; with it the text differs (a renderer decides rebuilds by comparing sources)."""
    assert sorted(os.path.splitext(f)[0] for f in os.listdir(os.path.join(ROOT, "scenes")) if f.endswith(".ron")) == SCENES
    scene = pa.Scene.from_file(pa.scene_path(scene_name))
    for base in (0, pa.FLAG_SLICES, pa.FLAG_SPECIALIZE_STATIC):
        plain = scene.generate_source(base)
        assert "PTL_PASSES" not in plain and "ptl_pass" not in plain and "out_passes" not in plain
        passes = scene.generate_source(base | pa.FLAG_PASSES)
        assert passes != plain and "#define PTL_PASSES 1\n" in passes and "ptl_host_render_passes(" in passes
        assert passes.count("__restrict__ out_passes) {") == 1
        assert scene.generate_source(base) == plain  # and the flag leaves nothing behind in the scene handle
    assert pa.FLAG_PASSES == 1 << 30
    assert re.search(r"#define PTL_FLAG_PASSES \(1u << 30\)", open(os.path.join(ROOT, "include", "portal_amd.h")).read())


@pytest.mark.parametrize("other", ["FLAG_ANAGLYPH", "FLAG_REFINE", "FLAG_REFINE_SLICES", "FLAG_CHECK_AFFINE"])
def test_refused_combinations_say_why(pa, other):
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    with pytest.raises(pa.PortalError) as e:
        scene.generate_source(pa.FLAG_PASSES | getattr(pa, other))
    assert "PTL_FLAG_PASSES cannot be combined with PTL_" + other in str(e.value)
    scene.generate_source(getattr(pa, other))  # alone it is still fine


def test_renderer_option_adds_and_removes_the_flag(pa):
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    r = pa.SceneRenderer(scene, device=-1)
    plain = r.kernel_source()
    r.set_option("passes", 1)
    assert "#define PTL_PASSES 1\n" in r.kernel_source()
    r.set_option("passes", 0)
    assert r.kernel_source() == plain
    refine = pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_REFINE)
    before = refine.kernel_source()
    assert pa.lib().ptl_renderer_set_option(refine._h, b"passes", 1.0) < 0 and "PTL_FLAG_REFINE" in pa.last_error()
    assert refine.kernel_source() == before  # a refused combination leaves the renderer as it was


# ---------------------------------------------------------------------------------------------
# 2. - 4. the host build of the pass source against the oracle
# ---------------------------------------------------------------------------------------------
def host_passes(pa, scene_name, w, h, depth, aa, aa_start=0, options=(), flags=0, passes=True):
    """The host build of the scene's (pass) source, drawn with the renderer's uniform values -> dict(passes, rgba8, rgba32f, segments)."""
    from oracle import host_build as hb

    scene = pa.Scene.from_file(pa.scene_path(scene_name))
    flags |= pa.FLAG_PASSES if passes else 0
    r = pa.SceneRenderer(scene, device=-1, flags=flags)
    for k, v in (("render_depth", depth), ("aa_count", aa), ("aa_start", aa_start)) + tuple(options):
        r.set_option(k, v)
    hk = hb.host_kernel_for(r, scene, w, h, flags=flags | pa.FLAG_COUNT_SEGMENTS, count_segments=True)
    if not passes:
        return hk.render(w, h)
    fn = hk.lib.ptl_host_render_passes
    fn.restype = C.c_ulonglong
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
    rec = np.zeros((h, w), ref.RECORD)
    a8, a32 = np.zeros((h, w, 4), np.uint8), np.zeros((h, w, 4), np.float32)
    rows = np.arange(h, dtype=np.int32)
    assert rec.ctypes.data % 16 == 0
    seg = fn(a8.ctypes.data, a32.ctypes.data, rec.ctypes.data, w, h, rows.ctypes.data, h, 0, w, min(16, os.cpu_count() or 1))
    return {"passes": rec, "rgba8": a8, "rgba32f": a32, "segments": int(seg)}


@functools.lru_cache(maxsize=None)
def oracle_paths(scene_name, w, h, depth, aa, aa_start, overrides=()):
    """The numpy oracle's frame, and what its ray_tracing said about every path: a spy around Oracle.ray_tracing keeps (segments, depth,
    has_depth, colour) of each call.  Without bars or stereo a call covers the whole frame in raster order, one call per sample."""
    from oracle.portal_oracle import Oracle

    o = Oracle(os.path.join(ROOT, "scenes", scene_name + ".ron"))
    o.options.update(render_depth=depth, aa_count=aa, aa_start=aa_start)
    o.overrides.update(dict(overrides))
    calls, inner = [], o.ray_tracing

    def spy(r, camera_scale):
        out = inner(r, camera_scale)
        calls.append(tuple(np.array(x) for x in out))
        return out

    o.ray_tracing = spy
    return o.render(w, h), calls


CASES = [(s, aa, d) for s in ("basics", "monoportal", "portal_in_portal") for aa in (1, 3) for d in (1, 2, 3, 40)]


@pytest.mark.parametrize("scene_name,aa,depth", CASES, ids=[f"{s}-aa{a}-d{d}" for s, a, d in CASES])
def test_records_against_the_oracle(pa, scene_name, aa, depth):
    """37x19, `_aa_start` 2: trips per pixel are the oracle's per-pixel segments; every path is booked once; the exhausted paths are exactly the
    oracle's paths that took `depth` trips, have no depth and came back black; depth_near is the minimum of the oracle's depths over the paths
    that have one."""
    got = host_passes(pa, scene_name, W, H, depth, aa, aa_start=2)
    want, calls = oracle_paths(scene_name, W, H, depth, aa, 2)
    rec = got["passes"]
    assert np.array_equal(rec["trips"], want["segments"])
    assert got["segments"] == int(rec["trips"].sum()) == int(want["segments"].sum())  # the host build's own counter is the sum of the records
    assert np.array_equal(got["rgba8"], want["rgba8"])  # same colours as every other build
    final, escaped, exhausted, outside = (c.reshape(H, W) for c in ref.counts(rec.reshape(-1)))
    assert ((final + escaped + exhausted + outside) == aa).all() and not outside.any()
    assert len(calls) == aa and all(len(c[1]) == W * H for c in calls)
    o_final = sum(c[3].astype(np.int64) for c in calls).reshape(H, W)
    o_exhausted = sum((~c[3] & (c[1] == depth) & ~c[0].any(axis=1)).astype(np.int64) for c in calls).reshape(H, W)
    assert np.array_equal(final, o_final)
    assert np.array_equal(exhausted, o_exhausted)
    assert np.array_equal(escaped, aa - o_final - o_exhausted)
    o_depth = np.full(W * H, np.inf, np.float32)
    for c in calls:
        o_depth = np.where(c[3] & (c[2] < o_depth), c[2], o_depth).astype(np.float32)
    assert np.array_equal(bits(rec["depth_near"]), bits(o_depth.reshape(H, W)))
    assert np.isinf(rec["depth_near"][final == 0]).all() and np.isfinite(rec["depth_near"][final > 0]).all()
    if scene_name == "portal_in_portal" and depth <= 3:
        # what the issue is about: pixels drawn black because the depth ran out, found without looking at the picture
        black = ~want["rgba8"][..., :3].any(axis=2)
        assert np.array_equal(exhausted == aa, (want["segments"] == aa * depth) & black & (o_final == 0))
        if depth == 1:
            assert exhausted.any()


def test_a_path_that_ends_on_the_last_trip_is_not_exhausted(pa):
    """basics at depth 1: every path's first and only trip either hits a final material or leaves the scene, so nothing is exhausted
    although every path took exactly `depth` trips; at depth 40 the same paths are booked the same way."""
    one, deep = host_passes(pa, "basics", W, H, 1, 1)["passes"], host_passes(pa, "basics", W, H, 40, 1)["passes"]
    first_trip_ends = deep["trips"] == 1
    assert first_trip_ends.any() and (one["trips"] == 1).all()
    assert np.array_equal(one["final_escaped"][first_trip_ends], deep["final_escaped"][first_trip_ends])
    assert not (one["exhausted_outside"][first_trip_ends]).any()


def test_360_frame_books_the_bars_as_outside(pa):
    """40x40 equirectangular: the picture is 2:1, so the rows above and below it never trace.  `outside` counts exactly those samples."""
    w = h = 40
    overrides = (("_use_360_camera", np.int32(1)),)
    for aa in (1, 3):
        rec = host_passes(pa, "monoportal", w, h, 20, aa, options=(("use_360_camera", 1),))["passes"]
        want, _ = oracle_paths("monoportal", w, h, 20, aa, 0, overrides)
        assert np.array_equal(rec["trips"], want["segments"])
        final, escaped, exhausted, outside = (c.reshape(h, w) for c in ref.counts(rec.reshape(-1)))
        assert ((final + escaped + exhausted + outside) == aa).all()
        # a sample that traces takes at least one trip, so the oracle's frame of sample `a` alone has zero segments exactly in the bars
        in_bar = sum((oracle_paths("monoportal", w, h, 20, 1, a, overrides)[0]["segments"] == 0).astype(np.int64) for a in range(aa))
        assert np.array_equal(outside, in_bar)
        assert (outside > 0).any() and (outside == 0).any()
        assert (outside == outside[:, :1]).all() and outside[0, 0] == aa and outside[-1, 0] == aa and outside[h // 2, 0] == 0  # whole rows, top and bottom


def test_side_by_side_books_both_eyes(pa):
    """40x16 side by side: each half is an eye.  Offline both eye matrices are the camera's, so the halves show the same picture."""
    w, h, aa = 40, 16, 3
    rec = host_passes(pa, "monoportal", w, h, 20, aa, options=(("draw_side_by_side", 1),))["passes"]
    want, _ = oracle_paths("monoportal", w, h, 20, aa, 0, (("_draw_side_by_side", np.int32(1)),))
    assert np.array_equal(rec["trips"], want["segments"])
    final, escaped, exhausted, outside = (c.reshape(h, w) for c in ref.counts(rec.reshape(-1)))
    assert ((final + escaped + exhausted + outside) == aa).all()
    for eye in (rec[:, : w // 2], rec[:, w // 2:]):  # both eyes trace, and see the same scene from the same place
        assert (eye["trips"] >= aa).all() and (eye["final_escaped"] & 0xFFFF).any()


def test_depth_near_reproduces_the_depth_map_frame(pa):
    """Compositional: at aa 1 the existing build's depth-map frame is the oracle's inferno gradient of depth_near, gamma-encoded and packed --
    byte for byte.  (The depth map is all the tracer could say about depth so far: colourised and clamped.)"""
    from oracle import glsl_math as M
    from oracle.portal_oracle import Oracle, to_rgba8

    w, h, lo, hi = W, H, 1.0, 7.5
    options = (("draw_depth_map", 1), ("depth_map_min", lo), ("depth_map_max", hi))
    drawn = host_passes(pa, "portal_in_portal", w, h, 40, 1, options=options, passes=False)["rgba8"]
    rec = host_passes(pa, "portal_in_portal", w, h, 40, 1)["passes"].reshape(-1)
    o = Oracle(os.path.join(ROOT, "scenes", "portal_in_portal.ron"))
    o.overrides.update({"_draw_depth_map": np.int32(1), "_depth_map_min": np.float32(lo), "_depth_map_max": np.float32(hi)})
    o.build(w, h)
    M.set_active(rec.size)
    has_depth = (rec["final_escaped"] & 0xFFFF) != 0
    grad = o.sample_depth_gradient(np.where(has_depth, rec["depth_near"], np.float32(0)).astype(np.float32))
    rgb = np.where(has_depth[:, None], np.stack([np.broadcast_to(c, (rec.size,)) for c in grad.c], axis=1), np.float32(0)).astype(np.float32)
    rgba = np.concatenate([M.sqrt(np.multiply(rgb, M.div(np.float32(1.0), np.float32(1)))), np.ones((rec.size, 1), np.float32)], axis=1)
    assert np.array_equal(to_rgba8(rgba).reshape(h, w, 4), drawn)
    assert len(np.unique(drawn.reshape(-1, 4), axis=0)) > 8  # a real picture


# ---------------------------------------------------------------------------------------------
# 5. gfx950
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags_name", ["", "FLAG_SLICES"])
def test_pass_build_cross_compiles_without_scratch(pa, flags_name):
    """The headline scene's pass build for gfx950 on a compile-only handle: no scratch, and still four waves per SIMD (<= 128 VGPRs)."""
    scene = pa.Scene.from_file(pa.scene_path("portal_in_portal"))
    base = getattr(pa, flags_name) if flags_name else 0
    r = pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_PASSES | base)
    res = r.resources()
    print("pass build", flags_name or "plain", res)
    assert res["scratch_bytes"] == 0 and 0 < res["registers"] <= 128
    assert r.code_object_note(".vgpr_spill_count") == 0


# ---------------------------------------------------------------------------------------------
# 6. the greyscale writer, the references, the refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (64, 36)])
def test_png_write_gray16_files_decode(pa, tmp_path, w, h):
    rng = np.random.default_rng(w * 100 + h)
    samples = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    samples.reshape(-1)[:2] = [0, 65535][: samples.size]
    for level in (0, 6, 9):
        path = str(tmp_path / f"g{level}.png")
        pa.png_write_gray16(path, ref.gray16_bytes(samples), w, h, level)
        assert np.array_equal(ref.read_png_gray16(path), samples)
    from PIL import Image

    seen = np.array(Image.open(str(tmp_path / "g6.png")))
    assert seen.shape == (h, w) and np.array_equal(seen.astype(np.uint16), samples)  # and a third reader agrees


def test_png_write_gray16_refuses(pa, tmp_path):
    f, rows = pa.lib().ptl_png_write_gray16, np.zeros(8, np.uint8)
    path = str(tmp_path / "x.png").encode()
    for args in ((None, rows.ctypes.data, 2, 2, 6), (path, None, 2, 2, 6), (path, rows.ctypes.data, 0, 2, 6), (path, rows.ctypes.data, 2, -1, 6), (path, rows.ctypes.data, 2, 2, 10),
                 (path, rows.ctypes.data, 2, 2, -1)):
        assert f(*args) == -1
    assert not os.listdir(tmp_path)
    with pytest.raises(pa.PortalError):
        pa.png_write_gray16(str(tmp_path / "y.png"), rows, 3, 2)


def test_entry_points_refuse_before_any_gpu_call(pa):
    """No device is touched: wrong `which`, null or misaligned pointers, counts out of range, a kernel without the records."""
    lib, buf = pa.lib(), np.zeros(64, np.uint8)
    aligned = (buf.ctypes.data + 15) & ~15
    assert lib.ptl_passes_to_gray16(0, aligned, 1, aligned, 2, 0.0, 1.0, None, None) == -1 and "which" in pa.last_error()
    assert lib.ptl_passes_to_gray16(0, None, 1, aligned, 0, 0.0, 1.0, None, None) == -1
    assert lib.ptl_passes_to_gray16(0, aligned + 4, 1, aligned, 0, 0.0, 1.0, None, None) == -1
    assert lib.ptl_passes_to_gray16(0, aligned, 0, aligned, 1, 0.0, 1.0, None, None) == -1
    assert lib.ptl_pass_stats(0, None, 1, aligned, None, 0, None, None) == -1
    assert lib.ptl_pass_stats(0, aligned, 1, None, None, 0, None, None) == -1
    assert lib.ptl_pass_stats(0, aligned, 0, aligned, None, 0, None, None) == -1
    assert lib.ptl_pass_stats(0, aligned, 1, aligned, None, -1, None, None) == -1
    assert lib.ptl_pass_stats(0, aligned + 8, 1, aligned, None, 0, None, None) == -1
    assert pa.pass_record_bytes(37, 19) == 16 * 37 * 19 and pa.pass_record_bytes(0, 19) == 0
    assert pa.PASS_RECORD == ref.RECORD and pa.PASS_RECORD.itemsize == 16 and pa.PASS_STATS_BLOCK.itemsize == 80 + 8 * 256
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    frame = pa.Frame(16, 8, 0, 1, 0)
    plain = pa.SceneRenderer(scene, device=-1)
    assert lib.ptl_renderer_draw_passes(plain._h, C.byref(frame), None, None, aligned, 16 * 128, None, None, None) == -1 and "PTL_FLAG_PASSES" in pa.last_error()
    passes = pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_PASSES)
    assert lib.ptl_renderer_draw_passes(passes._h, C.byref(frame), None, None, aligned, 16 * 128 - 1, None, None, None) == -1 and "16 bytes per pixel" in pa.last_error()
    assert lib.ptl_renderer_draw_passes(passes._h, C.byref(frame), None, None, aligned + 8, 16 * 128, None, None, None) == -1
    assert lib.ptl_renderer_draw_passes(passes._h, C.byref(frame), None, None, None, 16 * 128, None, None, None) == -1


def test_reference_keys_order_like_floats(pa):
    v = np.array([-np.float32(3.5), -1e-30, -0.0, 0.0, 1e-30, 2.0, 3.0e38], np.float32)
    keys = ref.depth_key(v)
    assert (np.diff(keys.astype(np.int64)) > 0).all() and keys.min() > 0 and (keys ^ 0xFFFFFFFF).min() > 0
    stats = ref.add_stats(ref.empty_stats(), ref.records(v, 1, final=1))
    lo, hi = ref.depth_range(stats)
    assert lo == v[0] and hi == v[-1]
    assert ref.depth_range(ref.add_stats(ref.empty_stats(), ref.records([np.inf, -np.inf, np.nan], 1))) is None
    block = np.zeros(1, pa.PASS_STATS_BLOCK)
    block["depth_max_key"], block["depth_min_key_inv"] = stats["depth_max_key"], stats["depth_min_key_inv"]
    assert pa.pass_stats_depth_range(block) == (lo, hi)  # the library decodes the keys the same way


# (The command line has no anaglyph switch: that combination is refused where it can be asked for, at generation -- test_refused_combinations_say_why.)
CLI_REFUSALS = [
    ("render-frame", ["--passes", "depth", "--adaptive-aa"], "--adaptive-aa"),
    ("render-frame", ["--depth-report", "--adaptive-aa"], "--adaptive-aa"),
    ("render", ["--depth-report", "--clip-adaptive-aa"], "--clip-adaptive-aa"),
    ("render", ["--depth-report", "--adaptive-aa"], "--adaptive-aa"),
    ("render-frame", ["--passes", "trips", "--gpus", "2"], "one GPU"),
    ("render-frame", ["--depth-report", "--devices", "0,1"], "one GPU"),
    ("render-frame", ["--passes", "depth,trips", "--shard", "0/2"], "one GPU"),
    ("render", ["--depth-report", "--gpus", "2"], "one GPU"),
    ("render", ["--passes", "depth"], "--passes is an option of render-frame"),
    ("render-frame", ["--passes", "depth,normals"], "unknown pass `normals`"),
    ("render-frame", ["--passes", ""], "--passes depth,trips"),
    ("check", ["--depth-report"], "--depth-report is an option of render and render-frame"),
]


@pytest.mark.parametrize("cmd,extra,reason", CLI_REFUSALS, ids=[c + " " + " ".join(e) for c, e, _ in CLI_REFUSALS])
def test_cli_refuses_while_the_arguments_are_parsed(pa, tmp_path, cmd, extra, reason):
    """Exit status 2, one line that says why, nothing rendered or written."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    target = ["anim.4.portals", "--out-dir", str(tmp_path)] if cmd == "render" else ["--output", str(tmp_path / "f.png")] if cmd == "render-frame" else []
    out = subprocess.run([exe, cmd, pa.scene_path("basics")] + target + extra, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


def test_usage_names_the_options(pa):
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 2 and "--passes depth,trips" in out.stderr and out.stderr.count("--depth-report") == 2  # render-frame's and render's


# ---------------------------------------------------------------------------------------------
# 7. the writer under sanitizers, in a program of its own
# ---------------------------------------------------------------------------------------------
SANITIZED_MAIN = r"""
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>
#include "include/portal_amd.h"
namespace ptl { void set_last_error(const std::string& msg) { std::fprintf(stderr, "%s\n", msg.c_str()); } }
int main(int argc, char** argv) {
    const int sizes[3][2] = {{1, 1}, {5, 3}, {64, 36}};
    for (auto& s : sizes)
        for (int level : {0, 3, 9}) {
            const int w = s[0], h = s[1];
            std::vector<uint8_t> rows((size_t)2 * w * h);  // exactly the bytes the writer may read
            for (size_t i = 0; i < rows.size(); ++i) rows[i] = (uint8_t)(i * 37 + 11);
            const std::string path = std::string(argv[1]) + "/g" + std::to_string(w) + "_" + std::to_string(level) + ".png";
            if (ptl_png_write_gray16(path.c_str(), rows.data(), w, h, level) != PTL_OK) return 1;
            uint8_t* rgba = nullptr;
            int rw = 0, rh = 0;
            if (ptl_png_read(path.c_str(), &rgba, &rw, &rh) != PTL_OK || rw != w || rh != h) return 2;
            for (size_t p = 0; p < (size_t)w * h; ++p)  // the reader keeps the high byte of a 16-bit grey sample, in all three channels
                if (rgba[4 * p] != rows[2 * p] || rgba[4 * p + 1] != rows[2 * p] || rgba[4 * p + 2] != rows[2 * p] || rgba[4 * p + 3] != 255) return 3;
            std::free(rgba);
        }
    if (ptl_png_write_gray16(nullptr, nullptr, 1, 1, 6) != PTL_ERR_INVALID) return 4;
    std::puts("sanitized writer ok");
    return 0;
}
"""


def test_gray16_writer_under_sanitizers(tmp_path):
    """ptl_png_write_gray16 and ptl_png_read in a stand-alone program compiled with png_io.cpp under AddressSanitizer and
    UndefinedBehaviorSanitizer, run as a plain child process on rows of exactly 2 W H bytes, like tests/test_png16.py does for the RGB writer.
    The runtimes are linked statically and the child inherits the environment untouched.  Nothing is loaded into Python under a sanitizer."""
    (tmp_path / "main.cpp").write_text(SANITIZED_MAIN)
    exe = tmp_path / "sanitized_writer"
    build = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                            "-I", ROOT, str(tmp_path / "main.cpp"), os.path.join(ROOT, "portal_amd", "csrc", "host", "png_io.cpp"), "-lz", "-o", str(exe)],
                           capture_output=True, text=True, timeout=300)
    if build.returncode != 0 and re.search(r"cannot find.*(asan|ubsan)|libasan|libubsan", build.stderr):
        print(build.stderr)
        pytest.skip("no sanitizer runtimes to link against on this machine: " + build.stderr.strip().splitlines()[-1])
    assert build.returncode == 0, build.stderr
    files = tmp_path / "files"
    files.mkdir()
    run = subprocess.run([str(exe), str(files)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and "sanitized writer ok" in run.stdout, (run.returncode, run.stderr)
    assert "ERROR" not in run.stderr and "runtime error" not in run.stderr
    assert len(os.listdir(files)) == 9
    ref.read_png_gray16(str(files / "g64_3.png"))
