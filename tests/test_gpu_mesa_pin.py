"""The pin to a real GLSL compiler, GPU leg: frames of the HIP kernel against what Mesa (llvmpipe) computed from the
reference's own shaders (tests/golden/mesa/, written by tests/golden/make_mesa_fixtures.py).

Every frame goes through `tests/mesa_pin.check`: within 1e-5 per channel of Mesa's frame everywhere except on the entry's
list of pixels, where the CPU reference itself is further than that from Mesa and the frame must have the CPU reference's
bits.  Needs neither Mesa nor the reference's tree: fixtures only.
"""
import numpy as np
import pytest

from tests import mesa_pin as P
from tests import reftext as T
from tests.test_gpu_oracle_fullsize import CORPUS_BUILDS, HUNT_BUILDS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


def _pin(r, w, h, family, name, label):
    P.check(r.draw(w, h, rgba8=False, rgba32f=True)["rgba32f"], P.load(family, name), f"{family} {name} ({label})")


@pytest.mark.parametrize("build", ["dynamic", "ints_baked", "baked"])
@pytest.mark.parametrize("case", P.names("frames"))
def test_gpu_frame_cases_against_mesa(gpu, case, build):
    pa = gpu
    flags = {"dynamic": 0, "ints_baked": pa.FLAG_SPECIALIZE_INTS, "baked": pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL}[build]
    r, w, h, _ = P.product_renderer(pa, "frames", case, flags=flags)
    _pin(r, w, h, "frames", case, build)


@pytest.mark.parametrize("build", ["dynamic", "baked"])
@pytest.mark.parametrize("name", P.names("corpus"))
def test_gpu_corpus_scenes_against_mesa(gpu, name, build):
    """Every scene file of the reference, 32x18 at depth 12, un-specialised and everything baked (the code objects are the ones
    the corpus tests of tests/test_gpu_oracle_fullsize.py use)."""
    r, w, h, _ = P.product_renderer(gpu, "corpus", name, flags=CORPUS_BUILDS[build])
    _pin(r, w, h, "corpus", name, build)


@pytest.mark.parametrize("seed", P.names("random"))
def test_gpu_random_scenes_against_mesa(gpu, seed, tmp_path):
    flags = HUNT_BUILDS[int(seed) % 5]
    r, w, h, _ = P.product_renderer(gpu, "random", seed, flags=flags, scratch=tmp_path)
    _pin(r, w, h, "random", seed, f"flags {flags}")


@pytest.mark.parametrize("seed", P.names("glsl"))
def test_gpu_glsl_expression_scenes_against_mesa(gpu, seed, tmp_path):
    pa = gpu
    flags = pa.FLAG_SPECIALIZE_INTS if int(seed) % 4 == 1 else 0
    r, w, h, _ = P.product_renderer(pa, "glsl", seed, flags=flags, scratch=tmp_path)
    _pin(r, w, h, "glsl", seed, f"flags {flags}")


@pytest.mark.parametrize("scene", P.TELEPORT_SCENES)
def test_gpu_teleport_query_against_mesa(gpu, scene):
    """The renderer's GPU ray query against the query Mesa drew into a real 2x3 RGBA8 target: the same flags on every segment
    outside the stored list, positions within the distance recorded between the reference-text answer and Mesa's (no margin on
    top: GPU == reference text is the contract already)."""
    pa = gpu
    z = P.load_teleport()
    decoded, flag_diff, distance = z[scene + ".decoded"], set(int(k) for k in z[scene + ".flag_diff"]), float(z[scene + ".distance"])
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene)), device=0)
    compared = 0
    for k, ((a, b), want) in enumerate(zip(T.teleport_segments(scene), decoded)):
        if k in flag_diff:
            continue
        pos, hit, sub = r.teleport_external_ray(a, b)
        assert (int(pos is not None), int(hit), int(sub)) == tuple(int(v) for v in want[:3]), f"segment {k}"
        if pos is not None:
            got = np.asarray(pos, np.float64).astype(np.float32)
            assert np.max(np.abs(got.astype(np.float64) - want[3:6].view(np.float32).astype(np.float64))) <= distance, f"segment {k}"
            compared += 1
    assert compared >= 1
