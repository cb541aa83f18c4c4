"""The select-form plane-hit helpers of device/ptl_library.h on gfx950: the kernel as shipped against the same source compiled with
`-DPTL_EARLY_RETURN_HITS` (the reference's control flow), on the three kinds of build, bit for bit -- and against the frames the
reference's own shader text produced.  64x36 is two workgroups wide and four and a half row blocks high (the partial block is covered).
The CPU leg (field by field, directed inputs): tests/test_hit_helpers.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EARLY = "-DPTL_EARLY_RETURN_HITS"
SCENES = [("portal_in_portal", 40), ("triple_portal", 40)]
BUILDS = ["baked", "patterns", "unspecialised"]


def build_flags(pa, build):
    return {"baked": pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL, "patterns": pa.FLAG_SPECIALIZE_PATTERNS, "unspecialised": 0}[build]


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


def draw(pa, scene_name, depth, flags):
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene_name)), device=0, flags=flags)
    r.set_option("render_depth", depth)
    out = {}
    for w, h in ((64, 36), (96, 54)):
        f = r.draw(w, h, rgba8=True, rgba32f=True)
        out[(w, h)] = (f["rgba32f"].view(np.uint32).copy(), f["rgba8"].copy())
    return out, r.code_object_sha256()


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("scene_name,depth", SCENES, ids=[s for s, _ in SCENES])
def test_select_form_helpers_change_no_bit_on_the_gpu(gpu, monkeypatch, scene_name, depth, build):
    pa = gpu
    flags = build_flags(pa, build)
    monkeypatch.delenv("PTL_HIPRTC_FLAGS", raising=False)
    shipped, sha_shipped = draw(pa, scene_name, depth, flags)
    # the early-return build: compiled by a compile-only child process into the code-object cache (extra compile options reach one
    # compile of one process that way, as in bench.py), loaded here
    child = "import sys; sys.path.insert(0, sys.argv[1]); import portal_amd as pa; pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(sys.argv[2])), device=-1, flags=int(sys.argv[3]))"
    subprocess.run([sys.executable, "-c", child, ROOT, scene_name, str(flags)], env=dict(os.environ, PTL_HIPRTC_FLAGS=EARLY), check=True, timeout=600)
    monkeypatch.setenv("PTL_HIPRTC_FLAGS", EARLY)
    early, sha_early = draw(pa, scene_name, depth, flags)
    assert sha_early != sha_shipped  # two binaries: the define reached the compile
    for size in shipped:
        assert np.array_equal(shipped[size][0], early[size][0]), f"{build} {size}: {int((shipped[size][0] != early[size][0]).any(axis=2).sum())} pixels differ"
        assert np.array_equal(shipped[size][1], early[size][1])
    g = np.load(os.path.join(ROOT, "tests", "golden", "reference_text", f"{scene_name}_96x54_d{depth}_aa1.npz"))
    assert np.array_equal(shipped[(96, 54)][0], g["rgba32f_bits"]) and np.array_equal(shipped[(96, 54)][1], g["rgba8"])
