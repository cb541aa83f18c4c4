"""The plane-hit helpers of device/ptl_library.h in select form (no early return, no conditional block) against the reference's control flow,
which `-DPTL_EARLY_RETURN_HITS` restores: the host build of the same generated source with and without the define, frame for frame and
field for field.  (The form changes what the compiler may sink into the caller's `nearer` branch, never a value.)  The GPU leg:
tests/test_gpu_hit_helpers.py."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 64, 36
BASELINE_SCENES = [("basics", 10), ("monoportal", 20), ("triple_portal", 40), ("portal_in_portal", 40), ("mobius_monoportal", 64)]
# corpus scenes whose OWN snippets call the rewritten helpers (plane_intersect, plane_intersect_normalized, process_portal_intersection)
CORPUS_SCENES = [("tests/corpus/scenes/portal_in_portal_plus_ultra.ron", 20), ("tests/corpus/scenes/trefoil.ron", 20), ("tests/corpus/scenes/triple_portal2.ron", 20)]


def host_frames(pa, scene_path, depth, flags, define, asset_root=None):
    """64x36 frame of the host build of `scene_path`'s generated source, compiled with and without `define`."""
    from oracle import host_build as hb

    scene = pa.Scene.from_file(scene_path)
    extra = {"asset_root": asset_root} if asset_root else {}
    r = pa.SceneRenderer(scene, device=-1, flags=flags, **extra)
    r.set_option("render_depth", depth)
    source = scene.generate_source(flags)
    layout, size = scene.uniform_layout()
    defines = tuple(d for d in scene.generated_defines() if d != "PTL_COUNT_SEGMENTS" and not d.startswith("PTL_WAVES_PER_EU") and d != "PTL_QUICK_JIT")
    frames = []
    for more in ((), (define,)):
        hk = hb.HostKernel(source, layout, size, defines=defines + more)
        for name, typ, _ in layout:
            if typ == pa.PTL_SAMPLER:
                continue
            v = r.uniform_value(name, W, H)
            if v is not None:
                hk.set_uniform(name, v)
        frames.append(hk.render(W, H))
    return frames


def assert_same_frame(a, b):
    assert np.array_equal(a["rgba32f"].view(np.uint32), b["rgba32f"].view(np.uint32)), f"{int((a['rgba32f'].view(np.uint32) != b['rgba32f'].view(np.uint32)).any(axis=2).sum())} of {W * H} pixels differ"
    assert np.array_equal(a["rgba8"], b["rgba8"])


@pytest.mark.parametrize("flags", [0, 5], ids=["unspecialised", "baked"])
@pytest.mark.parametrize("scene,depth", BASELINE_SCENES, ids=[s for s, _ in BASELINE_SCENES])
def test_baseline_scenes_draw_the_same_bits_with_the_early_return_helpers(pa, scene, depth, flags):
    new, old = host_frames(pa, pa.scene_path(scene), depth, flags, "PTL_EARLY_RETURN_HITS")
    assert_same_frame(new, old)
    assert len(np.unique(new["rgba8"].reshape(-1, 4), axis=0)) > 8  # (a picture, not a flat frame)


def test_a_host_kernel_does_not_inherit_the_texture_an_earlier_one_bound(pa):
    """Every `HostKernel` of one generated source gets the same dlopen'ed library, hence the same uniform block.  A kernel object of the
    same process that bound the scene's texture (`host_kernel_for`) used to leave it bound for the next one of that source -- the first of
    `host_frames`'s two, which binds none -- and the two frames differed on the textured wall whenever a worker ran the tests in that order."""
    from oracle import host_build as hb

    scene = pa.Scene.from_file(pa.scene_path("monoportal"))
    r = pa.SceneRenderer(scene, device=-1)
    r.set_option("render_depth", 20)
    textured = hb.host_kernel_for(r, scene, W, H).render(W, H)["rgba32f"].copy()
    new, old = host_frames(pa, pa.scene_path("monoportal"), 20, 0, "PTL_EARLY_RETURN_HITS")
    assert_same_frame(new, old)
    assert not np.array_equal(textured.view(np.uint32), new["rgba32f"].view(np.uint32))  # (the texture does show where it is bound)


@pytest.mark.parametrize("scene_file,depth", CORPUS_SCENES, ids=[os.path.basename(s)[:-4] for s, _ in CORPUS_SCENES])
def test_corpus_scenes_that_call_the_helpers_draw_the_same_bits(pa, scene_file, depth):
    new, old = host_frames(pa, os.path.join(ROOT, scene_file), depth, 0, "PTL_EARLY_RETURN_HITS", asset_root=os.path.join(ROOT, "tests", "corpus"))
    assert_same_frame(new, old)


# ---- field for field: every rewritten helper on directed inputs (NaN t, +-0, infinities, d.z == 0, non-hits, every `inside` verdict) -------
PROBE = r"""
#include <cstring>
extern "C" int ptl_hit_helper_probe(const float* in, int lanes, unsigned* out) {
    using namespace glsl;
    int words = 0;
    for (int k = 0; k < lanes; ++k) {
        const float* a = in + 16 * k;
        Ray r{vec4(a[0], a[1], a[2], 1.0f), vec4(a[3], a[4], a[5], 0.0f), 1.0f, false};
        mat4 m(1.0f);
        m[3] = vec4(a[6], a[7], a[8], 1.0f);
        m[0].x = a[9];
        const vec3 n(a[10], a[11], a[12]);
        const int inside = (int)a[13], teleport = (int)a[14];
        bool flipped = false, flipped_o = false;
        const vec4 o_in_plane = m * r.o;
        SurfaceIntersection s[5] = {plane_intersect_normalized(r), plane_intersect(r, m, n), plane_intersect_derived(r, m, normalize(n), flipped),
                                    plane_intersect_o(r, m, n, o_in_plane), plane_intersect_derived_o(r, m, normalize(n), flipped_o, o_in_plane)};
        SceneIntersection before{(int)a[15], s[0], a[15] > 3.0f};
        SceneIntersection p[2] = {process_plane_intersection(before, s[1], inside), process_portal_intersection(before, s[1], inside, teleport)};
        auto put = [&](float f) { std::memcpy(out + words++, &f, 4); };
        auto put_hit = [&](const SurfaceIntersection& h) { out[words++] = h.hit; put(h.t); put(h.u); put(h.v); put(h.n.x); put(h.n.y); put(h.n.z); };
        for (const auto& h : s) put_hit(h);
        out[words++] = flipped; out[words++] = flipped_o;
        for (const auto& q : p) { out[words++] = (unsigned)q.material; put_hit(q.hit); out[words++] = q.in_subspace; }
    }
    return words;
}
"""


def probe_inputs():
    rng = np.random.default_rng(7)
    special = np.array([0.0, -0.0, 1.0, -1.0, 0.5, -2.5, np.inf, -np.inf, np.nan, 1e-38, -1e-38, 3e38, 1e-45], np.float32)
    lanes = []
    for inside in (0, 1, 2, 3, 7, 41):  # NOT_INSIDE, TELEPORT, TELEPORT_SUBSPACE and plain materials (the defines of ptl_library.h: 0, 1, ...)
        for _ in range(160):
            a = rng.normal(size=16).astype(np.float32)
            for j in rng.choice(13, size=rng.integers(0, 4), replace=False):  # up to three special values per lane
                a[j] = rng.choice(special)
            a[13], a[14], a[15] = inside, 55, rng.integers(0, 6)
            lanes.append(a)
    for oz in special:  # every pairing of origin height and direction z: t = -o.z / d.z in all its corner cases
        for dz in special:
            a = np.zeros(16, np.float32)
            a[:6] = (0.25, -0.5, oz, 0.1, 0.2, dz)
            a[9], a[10:13], a[13:16] = 1.0, (0.0, 0.0, 1.0), (5, 55, 1)
            lanes.append(a)
    return np.ascontiguousarray(np.stack(lanes))


def test_every_field_of_every_rewritten_helper_keeps_its_bits(pa):
    """The probe calls the five plane tests and the two process_* functions on the same inputs in a unit compiled twice; every field of every
    result -- hit, t, u, v, n, material, in_subspace, the `flipped` verdicts -- has the same bits (NaN payloads included)."""
    import ctypes as C

    from oracle import host_build as hb

    scene = pa.Scene.from_file(pa.scene_path("basics"))
    source = scene.generate_source(0) + PROBE
    defines = tuple(d for d in scene.generated_defines() if d != "PTL_COUNT_SEGMENTS" and not d.startswith("PTL_WAVES_PER_EU") and d != "PTL_QUICK_JIT")
    lanes = probe_inputs()
    got = []
    for more in ((), ("PTL_EARLY_RETURN_HITS",)):
        lib = C.CDLL(hb.compile_host(source, defines=defines + more))
        out = np.zeros(len(lanes) * 64, np.uint32)
        lib.ptl_hit_helper_probe.restype = C.c_int
        words = lib.ptl_hit_helper_probe(C.c_void_p(lanes.ctypes.data), len(lanes), C.c_void_p(out.ctypes.data))
        assert 0 < words <= len(out)
        got.append(out[:words].reshape(len(lanes), -1))
    new, old = got
    assert new.shape == old.shape and new.shape[1] == 5 * 7 + 2 + 2 * 9
    bad = np.argwhere(new != old)
    assert len(bad) == 0, f"{len(bad)} words differ, first: lane {bad[0][0]} word {bad[0][1]} input {lanes[bad[0][0]]}"
    hits, misses, nans = int(new[:, 0].sum()), int((new[:, 0] == 0).sum()), int(np.isnan(new[:, 1].view(np.float32)).sum())
    print(f"{len(lanes)} lanes: {hits} hits, {misses} misses, {nans} NaN distances")
    assert hits > 100 and misses > 100 and nans > 10  # the directed lanes reach both verdicts and the NaN edge
    assert len(np.unique(new[:, 37])) > 3 and len(np.unique(new[:, 46])) > 3  # several materials come out of both process_* functions
    assert new[:, 54].any() and not new[:, 54].all()  # ... and in_subspace both ways
