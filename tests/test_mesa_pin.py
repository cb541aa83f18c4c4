"""The pin to a real GLSL compiler, CPU legs: fixtures only, no Mesa and no reference tree needed.

tests/golden/mesa/ holds what Mesa (llvmpipe) computed from the reference's own vertex and fragment shader
(tests/golden/make_mesa_fixtures.py, oracle/mesa.py).  Here:
  * every stored list of pixels is recomputed from reference-side data and must equal the stored one, and stays
    under the caps of tests/mesa_pin.py, so most pixels stand under the direct comparison with Mesa;
  * the product's host build (oracle/host_build.py), shipped and un-specialised, goes through the same
    `mesa_pin.check` the GPU frames go through in tests/test_gpu_mesa_pin.py;
  * a camera off by one part in 10^4 fails that check on every frame case;
  * the teleport query read back from a real 2x3 RGBA8 target agrees with reference_text/teleport.npz.
"""
import os

import numpy as np
import pytest

from tests import mesa_pin as P
from tests import reftext as T

ENTRIES = [(family, name) for family in P.FAMILIES for name in P.names(family)]
ENTRY_IDS = [f"{family}-{name}" for family, name in ENTRIES]


@pytest.fixture(autouse=True)
def _scratch_build_dirs(tmp_path_factory, monkeypatch):
    """one-off host builds and code objects: keep them out of oracle/_build and portal_amd/_cache"""
    from oracle import host_build as hb

    monkeypatch.setattr(hb, "BUILD_DIR", str(tmp_path_factory.getbasetemp() / "mesa_pin_build"))
    monkeypatch.setenv("PTL_CACHE_DIR", str(tmp_path_factory.getbasetemp() / "mesa_pin_cache"))


def test_every_entry_is_stored_and_the_exclusions_are_few():
    for family in P.FAMILIES:
        assert len(P.EXCLUDED[family]) <= P.MAX_EXCLUDED[family]
        assert all(reason.strip() for reason in P.EXCLUDED[family].values())
    assert len(P.names("frames")) == 11 and len(P.names("corpus", True)) == 82 and len(P.names("random", True)) == 30 and len(P.names("glsl", True)) == 12
    stamps = set()
    for f in sorted(os.listdir(P.MESA_DIR)):
        if f.endswith(".npz"):
            with np.load(os.path.join(P.MESA_DIR, f)) as z:
                stamps.add((str(z["gl_version"]), str(z["gl_renderer"]), str(z["text_digest"])))
            assert os.path.getsize(os.path.join(P.MESA_DIR, f)) <= 1_200_000
    assert len(stamps) == 1 and "Mesa" in next(iter(stamps))[0]
    assert sum(os.path.getsize(os.path.join(P.MESA_DIR, f)) for f in os.listdir(P.MESA_DIR)) <= 3_000_000
    for family, name in ENTRIES:
        w, h = P.frame_size(family, name)
        assert P.load(family, name)["mesa_bits"].shape == (h, w, 4)


@pytest.mark.parametrize("family,name", ENTRIES, ids=ENTRY_IDS)
def test_the_list_is_the_cpu_reference_against_mesa_and_stays_under_its_cap(family, name, tmp_path):
    """`listed` / `listed_bits` recomputed from the committed reference-text frame (frame cases) or a fresh numpy Oracle
    render (everything else): the stored list can be neither padded nor trimmed."""
    entry = P.load(family, name)
    again = P.make_entry(entry["mesa_bits"], P.cpu_reference_bits(family, name, tmp_path))
    assert np.array_equal(again["listed"], entry["listed"])
    assert np.array_equal(again["listed_bits"], entry["listed_bits"])
    assert entry["listed"].dtype == np.int32 and np.all(np.diff(entry["listed"]) > 0)
    w, h = P.frame_size(family, name)
    assert len(entry["listed"]) <= P.CAPS[family][0] * w * h, f"{len(entry['listed'])} of {w * h} pixels listed"


@pytest.mark.parametrize("family", P.FAMILIES)
def test_the_lists_of_a_family_stay_under_its_cap(family):
    listed = sum(len(P.load(family, name)["listed"]) for name in P.names(family))
    pixels = sum(int(np.prod(P.frame_size(family, name))) for name in P.names(family))
    assert listed <= P.CAPS[family][1] * pixels, f"{listed} of {pixels} pixels listed"


STEREO_CAMERA_UNIFORMS = ("_camera", "_camera_left_eye", "_camera_right_eye", "_camera_in_subspace", "_left_eye_in_subspace", "_right_eye_in_subspace",
                          "_camera_scale", "_left_eye_scale", "_right_eye_scale")


def _is_stereo(family, name):
    return family == "frames" and bool((T.FRAME_CASES[name][7] or {}).get("stereo"))


def _stereo_renderer(pa, case, flags):
    """The side-by-side case without a GPU: the product's camera step asks its GPU ray query for the eye matrices, so here the
    renderer gets the plain camera and the host kernel is handed the camera state of the oracle's rig (un-specialised build only:
    a baked build has these values compiled in)."""
    scene, w, h, depth, aa, options, overrides, camera = T.FRAME_CASES[case]
    assert flags == 0 and not options
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene)), device=-1, flags=flags)
    r.set_option("render_depth", depth)
    r.set_option("aa_count", aa)
    for k, v in overrides.items():
        r.set_option(T.PRODUCT_OPTIONS[k], float(v))
    r.set_camera(camera["look_at"], camera["alpha"], camera["beta"], camera["r"])
    return r, w, h


def _host_frame(pa, family, name, flags, scratch, perturb=None):
    from oracle import host_build as hb
    from oracle.glsl_values import Mat
    from oracle.portal_oracle import Oracle

    if _is_stereo(family, name):
        r, w, h = _stereo_renderer(pa, name, flags)
        root = None
    else:
        r, w, h, root = P.product_renderer(pa, family, name, flags=flags, device=-1, scratch=scratch)
    if perturb:
        perturb(r, w, h)
    r.uniform_value("_ray_tracing_depth", w, h)  # (evaluates the state the kernel source belongs to)
    hk = hb.host_kernel_for(r, r.scene, w, h, flags=flags, opt="-O0", **({"asset_root": root} if root else {}))  # tiny frames: compile time dominates
    if _is_stereo(family, name):
        o, _, _ = T.make_tracer(Oracle, name)
        values = o._uniform_values(w, h)
        for k in STEREO_CAMERA_UNIFORMS:
            v = values[k]
            assert hk.set_uniform(k, np.array([[np.asarray(c) for c in col.c] for col in v.cols], np.float32).T if isinstance(v, Mat) else v), k
    return hk.render(w, h, threads=2, rgba8=False)["rgba32f"]


HOST_CASES = [(family, name, build) for family, name in ENTRIES for build in ("shipped", "unspecialised")
              if not (build == "shipped" and _is_stereo(family, name))]  # (its baked build needs the GPU ray query: tests/test_gpu_mesa_pin.py runs it)


@pytest.mark.parametrize("family,name,build", HOST_CASES, ids=[f"{f}-{n}-{b}" for f, n, b in HOST_CASES])
def test_host_build_passes_the_pin(pa, family, name, build, tmp_path):
    """The rehearsal of the GPU leg: the generated kernel source compiled for the host, in the build the CLI ships (everything
    baked) and the un-specialised one, through `mesa_pin.check`."""
    flags = pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL if build == "shipped" else 0
    P.check(_host_frame(pa, family, name, flags, tmp_path), P.load(family, name), f"{family} {name} ({build})")


def _default_camera(case):
    from oracle.scene_eval import OracleScene

    cam = OracleScene(os.path.join(T.ROOT, "scenes", T.FRAME_CASES[case][0] + ".ron")).cam
    return cam["look_at"], cam["alpha"], cam["beta"], cam["r"]


@pytest.mark.parametrize("case", list(T.FRAME_CASES))
def test_a_view_angle_off_by_one_part_in_ten_thousand_fails_the_pin(pa, case, tmp_path):
    """Negative control: what `check` lets through is not wide enough for a subtly wrong frame.  The two equirectangular cameras
    never read `_view_angle` (the reference's camera branch for them takes yaw and pitch from the image position alone), so
    there the frame must not move at all, and the same relative error goes into the camera's `alpha` instead."""
    entry = P.load("frames", case)

    def view_angle(r, w, h):
        r.set_option("view_angle", float(r.uniform_value("_view_angle", w, h)) * (1.0 + 1e-4))

    def alpha(r, w, h):
        look_at, a, b, rad = _default_camera(case)
        r.set_camera(look_at, a * (1.0 + 1e-4), b, rad)

    frame = _host_frame(pa, "frames", case, 0, tmp_path, view_angle)
    if T.FRAME_CASES[case][6].get("_use_360_camera") is not None or T.FRAME_CASES[case][6].get("_use_180_camera") is not None:
        assert T.bits_equal(frame, _host_frame(pa, "frames", case, 0, tmp_path)).all()
        assert T.FRAME_CASES[case][7] is None
        frame = _host_frame(pa, "frames", case, 0, tmp_path, alpha)
    with pytest.raises(AssertionError, match="beyond|listed pixels"):
        P.check(frame, entry, case)


@pytest.mark.parametrize("scene", P.TELEPORT_SCENES)
def test_teleport_query_through_a_real_rgba8_target_agrees_with_the_reference_text(scene):
    """Entry e: Mesa drew `main()` with `_teleport_external_ray = 1` into a 2x3 RGBA8 target; the 24 bytes read back, decoded
    as the reference's host decodes them, give the flags of reference_text/teleport.npz on every segment outside the stored
    list, and positions no further from it than the stored distance -- which has to be a rounding-sized one."""
    z = P.load_teleport()
    raw, decoded, flag_diff, distance = z[scene + ".bytes"], z[scene + ".decoded"], z[scene + ".flag_diff"], float(z[scene + ".distance"])
    assert raw.shape == (len(T.teleport_segments(scene)), 24) and raw.dtype == np.uint8
    # the stored decode is the reference's decode of the stored bytes (src/main.rs:1394-1405)
    for row, want in zip(raw, decoded):
        hit = row[5] == 255 or row[13] == 255 or row[21] == 255
        sub = row[6] == 255 or row[14] == 255 or row[22] == 255
        pos = np.array([np.frombuffer(bytes([row[k], row[k + 1], row[k + 2], row[k + 4]]), "<f4")[0] for k in (0, 8, 16)], np.float32)
        teleported = not (pos == 0).all()
        assert (int(teleported), int(hit), int(sub)) == tuple(int(v) for v in want[:3])
        assert np.array_equal(pos.view(np.uint32) if teleported else np.zeros(3, np.uint32), want[3:6])
    flags, positions = P.unpack_reference_teleport(scene)
    differs = np.flatnonzero((flags != decoded[:, :3].astype(bool)).any(axis=1))
    assert np.array_equal(differs, flag_diff)
    assert len(flag_diff) <= 2  # a segment that grazes a portal's rim may flip; more would be a misreading
    same = np.setdiff1d(np.arange(len(raw)), flag_diff)
    assert decoded[same, 0].sum() >= 1  # the position comparison is not empty
    assert P.position_distance(positions[same], decoded[same, 3:6]) == distance
    assert distance <= 1e-5


def test_no_line_of_the_reference_shaders_is_in_the_runner_or_the_fixtures():
    """The runner holds no shader text and the fixtures hold outputs only.  (Runs where the texts are at hand.)"""
    from oracle import reference_shader as RS

    if not RS.available():
        pytest.skip("the reference's shader texts are not on this machine")
    texts = RS.reference_texts()
    lines = {ln.strip() for n in RS.FILES for ln in texts[n].split("\n")}
    lines = {ln for ln in lines if len(ln) >= 12 and any(c.isalpha() for c in ln)}  # `}` and `return x;` are nobody's
    assert len(lines) > 300
    runner = open(os.path.join(T.ROOT, "oracle", "mesa_runner.c"), encoding="utf-8").read()
    for ln in runner.split("\n"):
        assert ln.strip() not in lines, ln
    assert "gl_Position" not in runner and "gl_FragCoord" not in runner and "#version" not in runner
    for f in sorted(os.listdir(P.MESA_DIR)):
        if not f.endswith(".npz"):
            continue
        with np.load(os.path.join(P.MESA_DIR, f)) as z:
            for k in z.files:
                a = z[k]
                assert a.dtype in (np.uint32, np.int32, np.uint8, np.float64) or a.dtype.kind == "U", (f, k, a.dtype)
                blob = a.tobytes().decode("utf-32-le" if a.dtype.kind == "U" else "latin-1", "replace")
                hits = [ln for ln in lines if ln in blob]
                assert not hits, (f, k, hits[:3])
