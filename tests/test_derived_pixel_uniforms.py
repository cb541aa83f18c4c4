"""Frame-uniform arithmetic of the pixel path comes from the prologue kernel's table (ptl_trace.tpl derive(): `ptl_dv_eye*`, `ptl_dv_aa_jitter`,
`ptl_dv_rcp_aa_count`, `ptl_dv_rcp_t_range`, and the pixel size in place of `/ coef`) -- and no frame changes.

CPU: the host build of the generated source with the derived uniforms against the host build of the same scene without them
(FLAG_NO_DERIVED_UNIFORMS: every expression as the pixel path spells it), float bits and RGBA8 of whole frames.  Each case names a branch and
counts the pixels that take it.  tools/isa_uniform.py then says what is left of the uniform-only VALU work in the headline kernel, against the
list it made of the parent commit (profiles/r26/isa_uniform_pip_spec_w5_parent.json).
GPU: the same cases on the device against the host build's bits, one of them through the slices entry and one through the refine entry."""
import ctypes as C
import functools
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ("basics", "monoportal", "portal_in_portal")
W, H = 64, 36
DEPTH = 12
# The darkening thresholds: the final hits of all three scenes lie between 3 and 12 units from the camera at these sizes, so `_t_start` = 5 and
# `_t_end` = 7 leave pixels below the first threshold, between the two and above the second (each count is asserted).
T_START, T_END = 5.0, 7.0
# every builtin a case touches, with the value the other cases see
NEUTRAL = {"_aa_count": 1, "_aa_start": 0, "_draw_side_by_side": 0, "_camera_scale": 1.0, "_left_eye_scale": 1.0, "_right_eye_scale": 1.0, "_darken_by_distance": 0,
           "_t_start": 10.0, "_t_end": 210.0, "_draw_depth_map": 0, "_depth_map_min": 0.0, "_depth_map_max": 10.0, "_ray_tracing_depth": DEPTH}
DARKEN = {"_darken_by_distance": 1, "_t_start": T_START, "_t_end": T_END}
INT_UNIFORMS = ("_aa_count", "_aa_start", "_draw_side_by_side", "_darken_by_distance", "_draw_depth_map", "_ray_tracing_depth")


def table_rows(pa):
    src = pa.Scene.from_file(pa.scene_path("basics")).generate_source(0)
    return int(re.search(r"^#define PTL_AA_TABLE (\d+)$", src, re.M).group(1))


def cases(rows):
    """name -> (width, height, uniforms on top of NEUTRAL)"""
    return {
        "aa1": (W, H, {}),
        "aa3_from_2": (W, H, {"_aa_count": 3, "_aa_start": 2}),                      # the sub-frame form clips use
        "aa_past_the_table": (W, H, {"_aa_count": rows + 1}),                        # the last sample takes the spelled form
        "stereo_scales": (W, H, {"_draw_side_by_side": 1, "_left_eye_scale": 0.75, "_right_eye_scale": 1.6, **DARKEN}),
        "darken": (W, H, {"_camera_scale": 1.25, "_t_start": T_START / 1.25, "_t_end": T_END / 1.25, "_darken_by_distance": 1}),
        "depth_map": (W, H, {"_draw_depth_map": 1, "_depth_map_min": 3.0, "_depth_map_max": 12.0}),
        # max(scale, 1e-6) selects 1e-6: depths come out as all_t * 1e6, the map's range is set to see them
        "tiny_scale": (W, H, {"_camera_scale": 1e-7, "_draw_depth_map": 1, "_depth_map_min": 3.0e6, "_depth_map_max": 12.0e6}),
        "portrait": (H, W, {}),                                                        # min(resolution) picks x
        "square": (H, H, {}),
    }


class HostSide:
    """The two host builds of a scene (with and without derived uniforms) and their frames, rendered once per process."""

    def __init__(self, pa, name):
        from oracle import host_build as hb

        self.kernels = {}
        for label, flags in (("derived", 0), ("spelled", pa.FLAG_NO_DERIVED_UNIFORMS)):
            scene = pa.Scene.from_file(pa.scene_path(name))
            r = pa.SceneRenderer(scene, device=-1, flags=flags)
            self.kernels[label] = hb.host_kernel_for(r, scene, W, H, flags=flags)
        self.frames = {}

    def render(self, label, w, h, uniforms):
        key = (label, w, h, tuple(sorted(uniforms.items())))
        if key not in self.frames:
            hk = self.kernels[label]
            for k, v in {**NEUTRAL, **uniforms}.items():
                assert hk.set_uniform(k, v), k
            assert hk.set_uniform("_resolution", np.array([w, h], np.float32))
            out = hk.render(w, h)
            self.frames[key] = (out["rgba32f"].copy(), out["rgba8"].copy())
        return self.frames[key]


@functools.lru_cache(maxsize=None)
def host_side(name):
    import portal_amd as pa

    return HostSide(pa, name)


def differ(a, b):
    """pixels whose float bits differ"""
    return (a.view(np.uint32) != b.view(np.uint32)).any(axis=2)


def witnesses(host, case, w, h, uniforms, rows):
    """How many pixels of the case's frame take the branch it names -> {what: count}; every count must be positive."""
    f32 = host.render("spelled", w, h, uniforms)[0]
    lit = (f32[..., :3] != 0).any(axis=2)
    if case in ("aa1", "portrait", "square"):
        return {"pixels with a colour": int(lit.sum())}
    if case == "aa3_from_2":
        first = host.render("spelled", w, h, {"_aa_count": 3, "_aa_start": 0})[0]
        return {"pixels that samples 2, 3, 4 colour differently from samples 0, 1, 2": int(differ(f32, first).sum())}
    if case == "aa_past_the_table":
        table_only = host.render("spelled", w, h, {"_aa_count": rows})[0]
        assert uniforms["_aa_count"] > rows
        return {"pixels the sample behind the table's last row changes": int(differ(f32, table_only).sum())}
    if case == "stereo_scales":
        unit = host.render("spelled", w, h, {**uniforms, "_left_eye_scale": 1.0, "_right_eye_scale": 1.0})[0]
        swapped = host.render("spelled", w, h, {**uniforms, "_left_eye_scale": uniforms["_right_eye_scale"], "_right_eye_scale": uniforms["_left_eye_scale"]})[0]
        d, s = differ(f32, unit), differ(f32, swapped)
        return {"left-eye pixels its scale changes": int(d[:, : w // 2].sum()), "right-eye pixels its scale changes": int(d[:, w // 2:].sum()),
                "left-eye pixels the right eye's scale would colour differently": int(s[:, : w // 2].sum()), "right-eye pixels likewise": int(s[:, w // 2:].sum())}
    if case == "darken":
        # depth = all_t / scale, so `all_t > _t_start * scale` is `depth > _t_start`: the depth map says on which side a pixel's final hit lies.  A
        # depth at or below the map's lower end is drawn in ONE colour (normalised depth 0), and so is every pixel when that end is out of reach.
        def deeper_than(x):
            probe = {**uniforms, "_darken_by_distance": 0, "_draw_depth_map": 1}
            at_x = host.render("spelled", w, h, {**probe, "_depth_map_min": x, "_depth_map_max": x + 10.0})[0]
            nearest = host.render("spelled", w, h, {**probe, "_depth_map_min": 1e9, "_depth_map_max": 1e9})[0]
            return differ(at_x, nearest), (nearest[..., :3] != 0).any(axis=2)

        (past_start, final), (past_end, _) = deeper_than(uniforms["_t_start"]), deeper_than(uniforms["_t_end"])
        faded = differ(f32, host.render("spelled", w, h, {**uniforms, "_darken_by_distance": 0})[0])
        return {"final hits nearer than _t_start * scale, left as they are": int((final & ~past_start & ~faded).sum()),
                "between the thresholds, faded": int((past_start & ~past_end & faded).sum()), "beyond _t_end * scale, faded": int((past_end & faded).sum())}
    if case in ("depth_map", "tiny_scale"):
        colours = len(np.unique(f32.reshape(-1, 4)[lit.reshape(-1)].view(np.uint32), axis=0))
        out = {"pixels with a depth": int(lit.sum()), "distinct depth colours beyond one": colours - 1}
        if case == "tiny_scale":
            assert max(uniforms["_camera_scale"], 1e-6) == 1e-6
            floor = host.render("spelled", w, h, {**uniforms, "_camera_scale": 1e-6})[0]
            assert not differ(f32, floor).any()  # the floor took the scale's place
            out["depths equal to those at scale 1e-6"] = int((lit & ~differ(f32, floor)).sum())
        return out
    raise AssertionError(case)


@pytest.mark.parametrize("name", SCENES)
def test_derived_and_spelled_host_builds_draw_the_same_bits(pa, name):
    rows = table_rows(pa)
    host = host_side(name)
    src = pa.Scene.from_file(pa.scene_path(name)).generate_source(0)
    spelled = pa.Scene.from_file(pa.scene_path(name)).generate_source(pa.FLAG_NO_DERIVED_UNIFORMS)
    assert "#define PTL_DERIVED_BUILTINS 1" in src and "vec2 ptl_dv_aa_jitter[PTL_AA_TABLE];" in src
    assert "#define PTL_DERIVED_BUILTINS" not in spelled and "vec2 ptl_dv_aa_jitter" not in spelled
    for case, (w, h, uniforms) in cases(rows).items():
        a32, a8 = host.render("derived", w, h, uniforms)
        b32, b8 = host.render("spelled", w, h, uniforms)
        seen = witnesses(host, case, w, h, uniforms, rows)
        print(name, case, seen)
        assert all(v > 0 for v in seen.values()), (name, case, seen)
        assert not differ(a32, b32).any(), (name, case, int(differ(a32, b32).sum()))
        assert np.array_equal(a8, b8), (name, case)


def test_uniform_only_valu_left_in_the_headline_kernel(pa, monkeypatch):
    """tools/isa_uniform.py on the headline build (everything baked, five waves: the code object the PMC record counts).  Outside the scene's
    snippets the frame-uniform VALU instructions that remain are
      * moves of literals and inline constants into VGPRs -- the initial values of per-lane state (hit records, colours, counters): nothing is computed;
      * the spelled sub-pixel offset `quasi_random(a) * pixel_size * 2.0f` of samples beyond the table, on a branch a draw with at most
        PTL_AA_TABLE samples never takes.
    Everything the parent's list has beside those -- the reciprocal chains of `coef`, `aa_count`, the camera scale and `_t_end - _t_start`, the
    threshold products, `min(resolution)` -- is gone."""
    monkeypatch.delenv("PTL_JIT_OPT", raising=False)  # the shipped optimisation level: the parent's list was made of the shipped build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_uniform

    parent = json.load(open(os.path.join(ROOT, "profiles", "r26", "isa_uniform_pip_spec_w5_parent.json")))
    now = isa_uniform.analyse(pa.scene_path("portal_in_portal"), 5 | pa.flag_waves(5))
    assert now["same_instruction_stream_as_the_shipped_build"] and parent["same_instruction_stream_as_the_shipped_build"]
    assert parent["build"].startswith(now["build"])

    def computing(doc):
        assert all(r["class"] != "valu_move" for r in doc["computing_outside_snippets"])
        return doc["computing_outside_snippets"]

    def in_the_fallback(row):
        return any(w.startswith("shade_pixel: ") and "quasi_random(a) * pixel_size * 2.0f" in w for w in row["where"])

    left = [r for r in computing(now) if not in_the_fallback(r)]
    print("parent", parent["uniform_valu_outside_snippets"], "now", now["uniform_valu_outside_snippets"], "beyond the table", len(computing(now)) - len(left))
    assert left == [], left
    assert not any(in_the_fallback(r) for r in computing(parent))  # (the parent has no such branch: its whole list is executed by every wave)
    gone = len(computing(parent)) - len(left)
    assert gone == len(computing(parent)) > 0
    moves = lambda doc: doc["uniform_valu_outside_snippets"]["by_class"].get("valu_move", 0)
    assert moves(now) <= moves(parent)
    assert now["uniform_valu_outside_snippets"]["priced_cycles"] < parent["uniform_valu_outside_snippets"]["priced_cycles"]


# ---------------------------------------------------------------------------------------------------------------------------------------------
def _kernel_frame(pa, kernel, w, h, uniforms):
    """One launch of a renderer's layer-1 kernel with `uniforms` set on top of what the renderer uploaded."""
    L = pa.lib()
    for k, v in {**NEUTRAL, **uniforms, "_resolution": (float(w), float(h))}.items():
        if k in INT_UNIFORMS:
            buf, typ = np.array([int(v)], np.int32), pa.PTL_I32
        elif k == "_resolution":
            buf, typ = np.array(v, np.float32), pa.PTL_VEC2
        else:
            buf, typ = np.array([v], np.float32), pa.PTL_F32
        assert L.ptl_kernel_set_uniform(kernel, k.encode(), typ, buf.ctypes.data) == 0, (k, pa.last_error())
    frame = pa.Frame(w, h, 0, 1)
    a8, a32, ms = np.empty((h, w, 4), np.uint8), np.empty((h, w, 4), np.float32), C.c_float()
    assert L.ptl_kernel_render_to_host(kernel, C.byref(frame), a8.ctypes.data, a32.ctypes.data, None, C.byref(ms)) == 0, pa.last_error()
    return a32, a8


@pytest.mark.gpu
def test_device_frames_have_the_host_builds_bits(pa):
    """Every case of the CPU test on the device (the un-specialised build: every mode a run-time uniform) against the host build with derived
    uniforms; then the clip form (aa 3 from sample 2, darkening on) through the slices entry and through the refine entry at T = -1, which
    shades every pixel again with all its samples."""
    rows = table_rows(pa)
    for name in SCENES:
        host = host_side(name)
        scene = pa.Scene.from_file(pa.scene_path(name))
        r = pa.SceneRenderer(scene, device=0, flags=0)
        r.set_option("render_depth", DEPTH)
        r.draw(W, H)  # the scene's uniforms and the builtins are uploaded; the cases move builtins only
        kernel = pa.lib().ptl_renderer_kernel(r._h)
        for case, (w, h, uniforms) in cases(rows).items():
            want32, want8 = host.render("derived", w, h, uniforms)
            got32, got8 = _kernel_frame(pa, kernel, w, h, uniforms)
            assert not differ(got32, want32).any(), (name, case, int(differ(got32, want32).sum()))
            assert np.array_equal(got8, want8), (name, case)
        del r
    clip = {"_aa_count": 3, "_aa_start": 2, **DARKEN}
    options = {"render_depth": DEPTH, "aa_count": 3, "aa_start": 2, "darken_by_distance": 1, "gray_t_start": T_START, "gray_t_size": T_END - T_START}
    # the slices entry: two staged slices, the second from sample 5 on
    name = "monoportal"
    want = [host_side(name).render("derived", W, H, {**clip, "_aa_start": start}) for start in (2, 5)]
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(name)), device=0, flags=pa.FLAG_REFINE_SLICES)
    for k, v in options.items():
        r.set_option(k, v)
    frame = pa.Frame(W, H, 0, 1)
    d8, d32 = pa.device_alloc(2 * W * H * 4), pa.device_alloc(2 * W * H * 16)
    try:
        for j, start in enumerate((2, 5)):
            r.set_option("aa_start", start)
            r.stage_slice(frame, j)
        r.draw_slices(frame, 2, out_rgba8=d8, out_rgba32f=d32, slice_pixels=W * H)
        got8 = pa.device_download(d8, 2 * W * H * 4).reshape(2, H, W, 4)
        got32 = pa.device_download(d32, 2 * W * H * 16).view(np.float32).reshape(2, H, W, 4)
    finally:
        pa.device_free(d8)
        pa.device_free(d32)
    for j in range(2):
        assert not differ(got32[j], want[j][0]).any() and np.array_equal(got8[j], want[j][1]), ("slices entry", j)
    assert differ(want[0][0], want[1][0]).any()
    del r
    # the refine entry
    name = "basics"
    want32, want8 = host_side(name).render("derived", W, H, clip)
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(name)), device=0, flags=pa.FLAG_REFINE)
    for k, v in options.items():
        r.set_option(k, v)
    out = r.draw_adaptive(W, H, threshold=-1, rgba32f=True)
    assert out["count"] == W * H
    assert not differ(out["rgba32f"], want32).any() and np.array_equal(out["rgba8"], want8)
