"""The always-executed exits of the template, the generator and the prelude in their thinned forms against the text `-DPTL_SPELLED_EXITS`
restores: unorm8 as v_med3 + fma + truncating convert, the first snippet's record adopted by its flag alone -- and the
select forms of the colour helpers (-DPTL_SELECT_COLOR_HELPERS: measured, not taken).  Host leg: a model of the device form of unorm8 against
the spelled form on directed inputs, the helpers field for field in both forms, frames of the host build with and without the defines.  The
GPU leg: tests/test_gpu_exit_forms.py."""
import ctypes as C

import numpy as np
import pytest

from tests.exit_forms_cases import CASE_IDS, CASES, H, SPELLED, W, host_frame, host_kernel

# ---- unorm8 -------------------------------------------------------------------------------------------------------------------------
UNORM8_PROBE = r"""
namespace {
// v_min_f32 / v_med3_f32 as the ISA documents them: v_min returns the operand that is a number; v_med3 with a NaN among its operands
// returns v_min3 of them, otherwise the median.
float ptl_model_min(float a, float b) { return a != a ? b : (b != b ? a : (b < a ? b : a)); }
float ptl_model_max(float a, float b) { return a != a ? b : (b != b ? a : (a < b ? b : a)); }
float ptl_model_med3(float a, float b, float c) {
    if (a != a || b != b || c != c) return ptl_model_min(ptl_model_min(a, b), c);
    return ptl_model_max(ptl_model_min(a, b), ptl_model_min(ptl_model_max(a, b), c));
}
}
extern "C" void ptl_exit_unorm8_probe(const unsigned* bits, long n, unsigned* spelled, unsigned* model, unsigned* alpha) {
    for (long k = 0; k < n; ++k) {
        const float v = __builtin_bit_cast(float, bits[k]);
        spelled[k] = glsl::ptl_unorm8_spelled(v);
        model[k] = (unsigned)__builtin_fmaf(ptl_model_med3(v, 0.0f, 1.0f), 255.0f, 0.5f);  // the device form, operation for operation
    }
    *alpha = glsl::pack_rgba8(glsl::vec4(0.0f, 0.0f, 0.0f, 1.0f));
}
"""


def unorm8_inputs():
    parts = [np.arange(0, 1 << 32, 1 << 12, dtype=np.uint64).astype(np.uint32)]  # every pattern whose low 12 bits are zero
    centres = [np.float32((k + 0.5) / 255.0) for k in range(255)] + [np.float32(0.0), np.float32(1.0)]
    steps = np.arange(-8, 9, dtype=np.int64)
    for c in centres:  # +-8 ulps around every rounding border, 0 and 1 (below +0: the negative numbers next to -0)
        b = int(np.array([c], np.float32).view(np.uint32)[0])
        around = b + steps
        parts.append(np.where(around < 0, 0x80000000 + (-around), around).astype(np.uint32))
    sub = np.arange(0, 1 << 23, 1 << 8, dtype=np.uint32)  # all subnormals with a stride of 2^8, both signs
    parts += [sub, sub | np.uint32(0x80000000)]
    parts.append(np.array([0x7F800000, 0xFF800000, 0x00000000, 0x80000000], np.uint32))  # +-inf, +-0
    rng = np.random.default_rng(27)
    payload = rng.integers(1, 1 << 23, size=400, dtype=np.uint32)  # NaN payloads, quiet and signalling, both signs
    parts += [np.uint32(0x7F800000) | payload, np.uint32(0xFF800000) | payload, np.array([0x7F800001, 0x7FC00000, 0xFFFFFFFF, 0x7FFFFFFF], np.uint32)]
    return np.ascontiguousarray(np.concatenate(parts))


def test_unorm8_device_form_is_the_spelled_function(pa):
    from oracle import host_build as hb

    scene = pa.Scene.from_file(pa.scene_path("basics"))
    lib = C.CDLL(hb.compile_host(scene.generate_source(0) + UNORM8_PROBE))
    bits = unorm8_inputs()
    spelled, model, alpha = np.zeros(len(bits), np.uint32), np.zeros(len(bits), np.uint32), C.c_uint(0)
    lib.ptl_exit_unorm8_probe(C.c_void_p(bits.ctypes.data), C.c_long(len(bits)), C.c_void_p(spelled.ctypes.data), C.c_void_p(model.ctypes.data), C.byref(alpha))
    bad = np.flatnonzero(spelled != model)
    assert len(bad) == 0, f"{len(bad)} of {len(bits)} inputs differ, first: {hex(int(bits[bad[0]]))} spelled {spelled[bad[0]]} model {model[bad[0]]}"
    v = bits.view(np.float32)
    assert len(bits) > (1 << 20) + 255 * 17 + 2 * (1 << 15) + 800
    assert set(np.unique(spelled)) == set(range(256))  # every code is reached ...
    assert (spelled[np.isnan(v)] == 0).all() and np.isnan(v).sum() > 800 and (spelled[v <= 0] == 0).all() and (spelled[v >= 1] == 255).all()
    for k in range(255):  # ... and every rounding border is straddled
        c = np.float32((k + 0.5) / 255.0)
        near = np.abs(v.astype(np.float64) - float(c)) < 1e-6
        assert {k, k + 1} <= set(np.unique(spelled[near]))
    assert alpha.value == 0xFF000000  # alpha = 1.0: the code 255


# ---- color_grid3, color_grid, color_normal -------------------------------------------------------------------------------------------
HELPER_PROBE = r"""
#include <cstring>
extern "C" int ptl_exit_helper_probe(const float* in, int lanes, unsigned* out) {
    using namespace glsl;
    int words = 0;
    auto put = [&](float f) { std::memcpy(out + words++, &f, 4); };
    for (int toggle = 0; toggle < 2; ++toggle) {
        _grid_disable = toggle;  // (the accessors of the uniform block)
        _angle_color_disable = toggle;
        for (int k = 0; k < lanes; ++k) {
            const float* a = in + 8 * k;
            const vec3 start(a[0], a[1], a[2]);
            const vec2 uv(a[3], a[4]);
            const vec3 g3 = color_grid3(start, uv), g = color_grid(start, uv);
            put(g3.x); put(g3.y); put(g3.z); put(g.x); put(g.y); put(g.z);
            put(color_normal(vec3(a[0], a[1], a[2]), vec4(a[5], a[6], a[7], 0.0f)));
        }
    }
    return words;
}
"""


def helper_lanes():
    def ulps(x, ks):
        b = int(np.array([x], np.float32).view(np.uint32)[0])
        return (b + np.asarray(ks, np.int64)).astype(np.uint32).view(np.float32)

    us = []
    for border in (0.94, 0.985):  # dist = max(|fract(uv / 2) - 1/2|) * 2: u - 1 on [1, 2) (exact), 1 - u on [0, 1)
        us += list(ulps(np.float32(1.0) + np.float32(border), range(-4, 5)))
        us += list(ulps(np.float32(1.0) - np.float32(border), range(-320, 321)))
        us += list(ulps(np.float32(border), range(-4, 5)))  # (and the constants themselves as coordinates)
    for border in (0.0, 2.0, 4.0, 6.0):  # color_grid: step(fract(uv / 4), 1/2)
        us += list(ulps(np.float32(border), range(0 if border == 0.0 else -4, 5)))
    special = [0.0, -0.0, np.nan, np.inf, -np.inf, 1.0, -1.0, 0.5, 1e-38, -1e-45, 3e38, 1.5, 3.0, -1.94, -1.985, 1.96]
    rng = np.random.default_rng(3)
    lanes = []
    for u in us + special:
        for uv in ((u, 1.0), (1.0, u), (u, u), (u, -u), (u, 1.96), (1.96, u)):  # border from x, from y, x == y, and inside the border band either way round
            a = rng.normal(size=8).astype(np.float32)
            a[3], a[4] = uv
            lanes.append(a)
    for s in special:  # special values in `start` / the normal and in the direction
        for j in (0, 2, 5, 7):
            a = rng.normal(size=8).astype(np.float32)
            a[j] = s
            lanes.append(a)
    a = np.zeros(8, np.float32)  # zero vectors: normalize(0)
    lanes.append(a)
    return np.ascontiguousarray(np.stack(lanes))


def test_colour_helpers_keep_their_bits_in_both_forms(pa):
    """color_grid3, color_grid and color_normal on directed lanes in the shipped text (the reference's early returns) and as selects
    (-DPTL_SELECT_COLOR_HELPERS, the forms that were measured and not taken), all three and color_grid3 alone: the same bits, both toggle values."""
    from oracle import host_build as hb

    scene = pa.Scene.from_file(pa.scene_path("basics"))
    source = scene.generate_source(0) + HELPER_PROBE
    lanes = helper_lanes()
    got = []
    for defines in ((), ("PTL_SELECT_COLOR_HELPERS",), ("PTL_SELECT_COLOR_GRID3",)):
        lib = C.CDLL(hb.compile_host(source, defines=defines))
        out = np.zeros(2 * len(lanes) * 7, np.uint32)
        lib.ptl_exit_helper_probe.restype = C.c_int
        assert lib.ptl_exit_helper_probe(C.c_void_p(lanes.ctypes.data), len(lanes), C.c_void_p(out.ctypes.data)) == len(out)
        got.append(out.reshape(2, len(lanes), 7))
    shipped, selects, select_grid3 = got
    for other, name in ((selects, "PTL_SELECT_COLOR_HELPERS"), (select_grid3, "PTL_SELECT_COLOR_GRID3")):
        bad = np.argwhere(shipped != other)
        assert len(bad) == 0, f"{name}: {len(bad)} words differ, first: toggle {bad[0][0]} lane {bad[0][1]} word {bad[0][2]} input {lanes[bad[0][1]]}"
    on, off = shipped[0].view(np.float32), shipped[1].view(np.float32)
    ordinary = np.isfinite(lanes).all(axis=1) & (np.abs(lanes[:, :3]) > 1e-30).all(axis=1)  # (-0 * 0.4 is -0 either way; the ratios below need numbers)
    factor3 = np.round(on[ordinary, 0].astype(np.float64) / lanes[ordinary, 0], 3)
    print(f"{len(lanes)} lanes; color_grid3 factors {sorted(set(factor3))}")
    assert {0.4, 1.0, 0.7, 1.2} <= set(factor3)  # every return of color_grid3 is reached
    assert len(set(np.round(on[ordinary, 3].astype(np.float64) / lanes[ordinary, 0], 3))) >= 2  # both cells of color_grid
    start_bits = np.ascontiguousarray(lanes[:, :3]).view(np.uint32)
    assert np.array_equal(shipped[1][:, :3], start_bits) and np.array_equal(shipped[1][:, 3:6], start_bits)  # toggled off: `start` itself, bit for bit
    assert (off[:, 6] == 1.0).all()


# ---- frames ----------------------------------------------------------------------------------------------------------------------------
def assert_same_frame(a, b):
    assert np.array_equal(a[0], b[0]), f"{int((a[0] != b[0]).any(axis=2).sum())} of {W * H} pixels differ"
    assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("flags", [0, 5], ids=["unspecialised", "baked"])
@pytest.mark.parametrize("name,scene_file,depth", CASES, ids=CASE_IDS)
def test_host_frames_draw_the_same_bits_with_the_spelled_exits(pa, name, scene_file, depth, flags):
    new, old = host_frame(pa, scene_file, depth, flags), host_frame(pa, scene_file, depth, flags, defines=(SPELLED,))
    assert_same_frame(new, old)
    assert len(np.unique(new[1].reshape(-1, 4), axis=0)) > 8  # (a picture, not a flat frame)


@pytest.mark.parametrize("name,scene_file,depth", [c for c in CASES if c[0] in ("monoportal", "sphere_to_plane")], ids=["monoportal", "sphere_to_plane"])
def test_host_frames_draw_the_same_bits_with_the_colour_helpers_as_selects(pa, name, scene_file, depth):
    assert_same_frame(host_frame(pa, scene_file, depth, 5), host_frame(pa, scene_file, depth, 5, defines=("PTL_SELECT_COLOR_HELPERS",)))


def test_contract_1_host_frame_draws_the_same_bits_with_the_spelled_exits(pa):
    flags = 5 | pa.FLAG_EXACT_CR
    assert_same_frame(host_frame(pa, "scenes/portal_in_portal.ron", 40, flags), host_frame(pa, "scenes/portal_in_portal.ron", 40, flags, defines=(SPELLED,)))


# Which branches the paths of such a frame take.  The probe walks the centre ray of every pixel through the bounce loop with the kernel's
# own functions and looks, trip by trip, at what the adoption sees: the first snippet's raw record, the record
# scene_intersect_material_process hands out, the plane scan's hit.
BRANCH_PROBE = r"""
extern "C" void ptl_exit_branch_probe(int w, int h, unsigned long long* n) {
    using namespace glsl;
    derive_uniforms(&ptl_u);
    ptl_tracer t{&ptl_u};
    const float th = tan(ptl_div(_view_angle, 2.0f)), px = ptl_rcp((float)(w < h ? w : h));
    for (int y = 0; y < h; ++y) for (int x = 0; x < w; ++x) {
        const vec2 ip = vec2(((float)x + 0.5f - 0.5f * (float)w) * px * 2.0f, ((float)y + 0.5f - 0.5f * (float)h) * px * 2.0f);
        Ray r{_camera * vec4(0.0f, 0.0f, 0.0f, 1.0f), normalize(_camera * vec4(ip.x * th, ip.y * th, 1.0f, 0.0f)), 1.0f, _camera_in_subspace == 1};
        vec3 colour = vec3(1.0f);
        float all_t = 0.0f;
        ptl_tracer::RayTraceResult out{vec3(0.0f), 0.0f, false};
#ifdef PTL_DERIVED_BUILTINS
        const ptl_tracer::EyeScale eye{_camera_scale, ptl_u.ptl_dv_eye};
#else
        const ptl_tracer::EyeScale eye{_camera_scale};
#endif
        bool ended = false;
        int trips = 0;
        for (; trips < _ray_tracing_depth && !ended; ++trips) {
            const Ray ra = ptl_affine(r);
            const SceneIntersection i = t.scene_intersect(ra);
            const SceneIntersectionWithMaterial raw = t.intersect_material_0(ra, __builtin_inff()), i2 = t.scene_intersect_material_process(ra);
            const bool first_adopted = raw.scene.hit.hit && raw.scene.hit.t > 0.0f;
            n[0] += 1;                                                             // trips
            n[1] += first_adopted;                                                 // the first snippet's record adopted
            n[2] += raw.scene.hit.hit && !(raw.scene.hit.t > 0.0f);                // ... reported as a hit and rejected by t > 0
            n[3] += !raw.scene.hit.hit;                                            // ... a miss
            n[4] += i2.scene.hit.hit && (!first_adopted || __builtin_bit_cast(unsigned, i2.scene.hit.t) != __builtin_bit_cast(unsigned, raw.scene.hit.t));  // a later snippet's record took over
            const bool snippet_wins = nearer(i.hit, i2.scene.hit);
            n[5] += snippet_wins && i2.scene.material == CUSTOM_MATERIAL;          // the snippet's own material
            n[6] += snippet_wins && i2.scene.material != CUSTOM_MATERIAL;          // the snippet's hit, a material by id
            n[7] += !snippet_wins && i.hit.hit;                                    // the plane scan's hit
            n[8] += !(i.hit.hit || i2.scene.hit.hit);                              // escaped
            n[9] += i2.scene.hit.hit && !(i2.scene.hit.t > 0.0f);                  // (always 0: a record whose flag is set has t > 0)
#ifdef PTL_FIRST_TRIP
            ended = t.trace_segment(r, colour, all_t, eye, vec3(0.5f), out, false);
#else
            ended = t.trace_segment(r, colour, all_t, eye, vec3(0.5f), out);
#endif
        }
        n[10] += ended && out.has_depth;                                           // paths that end on a final material ...
        n[11] += ended && out.has_depth && trips > 1;                              // ... after at least one non-final one
        n[12] += !ended;                                                           // depth exhausted
        n[13] += __builtin_bit_cast(unsigned, out.color.x) % 251u;                 // (a checksum of what the paths returned)
    }
}
"""

# a snippet in front of sphere_to_plane's two that reports a hit BEHIND the ray on the left half of the view (t <= 0: nearer() turns it down) and
# nothing on the right
REJECTED_SNIPPET = """(
            name: "behind",
            data: ((("if (r.d.x < 0.) { return SceneIntersectionWithMaterial(SceneIntersection(0, SurfaceIntersection(true, -1., 0., 0., vec3(0., 0., 1.)), false), material_final(vec3(1., 0., 1.))); } return SceneIntersectionWithMaterial(scene_intersection_none, material_empty());"))),
        ),
        """


def branch_counts(pa, scene_file, depth, defines, text_edit=None, tmp_path=None):
    if text_edit:
        import os

        from tests.exit_forms_cases import ROOT

        text = text_edit(open(os.path.join(ROOT, scene_file)).read())
        scene_file = str(tmp_path / os.path.basename(scene_file))
        open(scene_file, "w").write(text)
    hk = host_kernel(pa, scene_file, depth, 0, defines, extra_source=BRANCH_PROBE)
    n = np.zeros(14, np.uint64)
    hk.lib.ptl_exit_branch_probe(W, H, C.c_void_p(n.ctypes.data))
    return [int(v) for v in n]


@pytest.mark.parametrize("scene_file,depth", [("scenes/portal_in_portal.ron", 40), ("tests/corpus/scenes/sphere_to_plane.ron", 20)], ids=["portal_in_portal", "sphere_to_plane"])
def test_the_paths_of_the_frames_take_every_branch_of_the_adoption(pa, scene_file, depth):
    new, old = branch_counts(pa, scene_file, depth, ()), branch_counts(pa, scene_file, depth, (SPELLED,))
    print(dict(zip(("trips", "first adopted", "rejected t<=0", "first missed", "later snippet", "custom material", "material by id", "plane hit", "escaped", "flag", "final", "final after non-final", "exhausted"), new)))
    assert new == old
    trips, adopted, rejected, missed, later, custom, by_id, plane, escaped, flag, final, final_after, exhausted, _ = new
    assert trips > W * H and adopted > 100 and plane > 100 and final > 100 and final_after > 100 and custom > 100 and flag == 0
    if "sphere_to_plane" in scene_file:
        assert later > 100  # the second snippet's record replaces the first's through nearer() (the first is hit by every ray of this view)
    else:
        assert missed > 100 and by_id > 50  # the headline's snippet misses on most trips, and hands out both kinds of material


def test_a_snippet_hit_behind_the_ray_is_turned_down_by_the_flag(pa, tmp_path):
    """No scene of the corpus reports a snippet hit with t <= 0 on these frames; this one does, on half of its rays: frames and counts with
    and without the define."""
    scene_file = "tests/corpus/scenes/sphere_to_plane.ron"

    def edit(text):
        head, sep, tail = text.partition("intersection_materials: ([")
        assert sep and tail.lstrip().startswith("(")
        return head + sep + "\n        " + REJECTED_SNIPPET + tail.lstrip()

    new, old = branch_counts(pa, scene_file, 20, (), edit, tmp_path), branch_counts(pa, scene_file, 20, (SPELLED,), edit, tmp_path)
    assert new == old
    assert new[2] > 100 and new[3] > 100 and new[4] > 100 and new[9] == 0  # rejected on the left, missed on the right, the later snippets still adopted
    scene_path = str(tmp_path / "sphere_to_plane.ron")
    frames = []
    for defines in ((), (SPELLED,)):
        f = host_kernel(pa, scene_path, 20, 0, defines).render(W, H)
        frames.append((f["rgba32f"].view(np.uint32).copy(), f["rgba8"].copy()))
    assert_same_frame(*frames)
