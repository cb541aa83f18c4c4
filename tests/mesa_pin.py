"""Shared by tests/test_mesa_pin.py, tests/test_gpu_mesa_pin.py and tests/golden/make_mesa_fixtures.py: the
entries of `tests/golden/mesa/` and the one checker every leg goes through.

`tests/golden/mesa/*.npz` hold frames that Mesa's GLSL compiler and llvmpipe computed from the reference's own
vertex and fragment shader (oracle/mesa.py).  A frame under test is compared with Mesa directly, within
TOLERANCE per channel (the project's target), everywhere except on a LIST of pixels per entry:
the pixels where the CPU reference (the committed reference-text frame, or a numpy `Oracle` render) is itself
beyond the tolerance from Mesa -- silhouettes where hit / miss flips, texture filter weights, iterations that
settle on another root.  On those the frame must have the CPU reference's bits.  The list is made of
reference-side data only, so it cannot absorb an error of the code under test; CAPS keep it small.
"""
from __future__ import annotations

import glob
import os

import numpy as np

from tests import reftext as T

ROOT = T.ROOT
MESA_DIR = os.path.join(ROOT, "tests", "golden", "mesa")
CORPUS_ROOT = os.path.join(ROOT, "tests", "corpus")
TOLERANCE = 1e-5

FAMILIES = ("frames", "corpus", "random", "glsl")
# share of listed pixels: (cap per entry, cap over the family) -- conditions on the fixtures, asserted by the CPU test
CAPS = {"frames": (0.04, 0.01), "corpus": (0.04, 0.01), "random": (0.04, 0.005), "glsl": (0.02, 0.02)}
MAX_EXCLUDED = {"frames": 0, "corpus": 4, "random": 2, "glsl": 1}
# entries left out by name, each with the reason that was found for it (see tests/golden/make_mesa_fixtures.py)
_REDEFINES_BUILTINS = ("Mesa refuses to compile the reference's shader for this scene: its own library defines `transpose` and `inverse`, builtins since "
                       "GLSL ES 3.00, which forbids redefining them (the scene was written for the reference's GLSL ES 1.00 build; its native build "
                       "asks for `#version 300 es`)")
EXCLUDED = {
    "frames": {},
    "corpus": {
        "boot.dev": _REDEFINES_BUILTINS,
        "sphere_to_plane": _REDEFINES_BUILTINS,
        "sphere_to_sphere": _REDEFINES_BUILTINS,
        "inverted_surface": "561 of 576 pixels beyond 1e-5, none beyond 2.9e-3: the whole frame is the skybox, and Mesa computes the skybox colour in 16-bit "
                            "floats (99.5 % of its pixels lie on the binary16 grid; the sampler is `lowp` by GLSL ES default and no highp operand meets the "
                            "texel before the output).  A precision GLSL ES leaves to the driver, not a misreading: rounding the oracle's texture() result "
                            "to binary16 makes 163 pixels bit-equal to Mesa instead of 15",
    },
    "random": {},
    "glsl": {},
}

CORPUS_FRAME = (32, 18, 12)   # width, height, render depth
RANDOM_FRAME = (40, 24, 10)
RANDOM_SEEDS = range(300, 330)
GLSL_SEEDS = range(400, 412)
GLSL_DEPTH, GLSL_VIEW_ANGLE = 2, 1.5
TELEPORT_SCENES = ("monoportal", "triple_portal", "portal_in_portal")


def corpus_files():
    return sorted(f for f in glob.glob(os.path.join(CORPUS_ROOT, "scenes", "*.ron")) if os.path.getsize(f) > 0)


def names(family, with_excluded=False):
    if family == "frames":
        out = list(T.FRAME_CASES)
    elif family == "corpus":
        out = [os.path.basename(f)[:-4] for f in corpus_files()]
    elif family == "random":
        out = [str(s) for s in RANDOM_SEEDS]
    else:
        out = [str(s) for s in GLSL_SEEDS]
    return [n for n in out if with_excluded or n not in EXCLUDED[family]]


def frame_size(family, name):
    if family == "frames":
        return T.FRAME_CASES[name][1:3]
    if family == "corpus":
        return CORPUS_FRAME[:2]
    if family == "random":
        return RANDOM_FRAME[:2]
    from tests.test_glsl_fuzz import N_EXPR

    return 4 * N_EXPR, 12


def _scene_file(family, name, scratch):
    """The scene file of a generated entry, written under `scratch`; -> (path, camera, in_subspace)"""
    if family == "random":
        from tests.test_scene_fuzz import random_scene

        text, cam, sub = random_scene(int(name))
    else:
        from tests.test_glsl_fuzz import fuzz_scene, fuzz_scene_with_uniforms

        text, cam, sub = (fuzz_scene_with_uniforms if int(name) % 2 else fuzz_scene)(int(name))[0], None, False
    path = os.path.join(str(scratch), f"{family}_{name}.ron")
    with open(path, "w", encoding="utf-8") as f:
        f.write(text)
    return path, cam, sub


def tracer(cls, family, name, scratch=None):
    """`cls` (oracle.portal_oracle.Oracle or oracle.reference_shader.ReferenceShader) set up for the entry -> (tracer, w, h)"""
    w, h = frame_size(family, name)
    if family == "frames":
        return T.make_tracer(cls, name)
    if family == "corpus":
        o = cls(os.path.join(CORPUS_ROOT, "scenes", name + ".ron"), asset_root=CORPUS_ROOT)
        o.options["render_depth"] = CORPUS_FRAME[2]
        return o, w, h
    path, cam, sub = _scene_file(family, name, scratch)
    o = cls(path)
    if family == "random":
        o.options["render_depth"] = RANDOM_FRAME[2]
        o.camera = dict(cam, in_subspace=sub)
    else:
        o.options.update(render_depth=GLSL_DEPTH, view_angle=GLSL_VIEW_ANGLE)
    return o, w, h


def product_renderer(pa, family, name, flags=0, device=0, scratch=None):
    """The product set up for the entry through its public options -> (renderer, w, h, asset root)"""
    w, h = frame_size(family, name)
    if family == "frames":
        return (*T.make_product_renderer(pa, name, flags=flags, device=device), None)
    if family == "corpus":
        r = pa.SceneRenderer(pa.Scene.from_file(os.path.join(CORPUS_ROOT, "scenes", name + ".ron")), device=device, asset_root=CORPUS_ROOT, flags=flags)
        r.set_option("render_depth", CORPUS_FRAME[2])
        return r, w, h, CORPUS_ROOT
    path, cam, sub = _scene_file(family, name, scratch)
    r = pa.SceneRenderer(pa.Scene.from_file(path), device=device, flags=flags)
    if family == "random":
        r.set_option("render_depth", RANDOM_FRAME[2])
        r.set_option("in_subspace", 1 if sub else 0)
        r.set_camera(cam["look_at"], cam["alpha"], cam["beta"], cam["r"])
    else:
        r.set_option("render_depth", GLSL_DEPTH)
        r.set_option("view_angle", GLSL_VIEW_ANGLE)
    return r, w, h, None


def cpu_reference_bits(family, name, scratch=None):
    """The CPU reference of an entry as float bits (h, w, 4): the committed reference-text frame where one exists, else a
    fresh numpy `Oracle` render.  Never the product, its host build or a GPU frame."""
    if family == "frames":
        w, h = frame_size(family, name)
        return np.load(os.path.join(T.GOLDEN_DIR, name + ".npz"))["rgba32f_bits"].reshape(h, w, 4).astype(np.uint32)
    from oracle.portal_oracle import Oracle

    o, w, h = tracer(Oracle, family, name, scratch)
    return np.ascontiguousarray(o.render(w, h)["rgba32f"], np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------
def within(frame_bits, mesa_bits):
    """(h, w) bool: every channel within TOLERANCE of Mesa.  Equal bits (infinities) and NaN on both sides count as
    within; NaN on one side only, or an infinity against anything else, as beyond."""
    a, b = np.asarray(frame_bits, np.uint32).view(np.float32), np.asarray(mesa_bits, np.uint32).view(np.float32)
    with np.errstate(invalid="ignore"):
        close = np.abs(a.astype(np.float64) - b.astype(np.float64)) <= TOLERANCE
    ok = close | (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
    return ok.all(axis=-1)


def make_entry(mesa_bits, cpu_bits):
    """The stored form of one entry: Mesa's frame, the listed pixels (flat indices) and the CPU reference's bits there."""
    mesa_bits, cpu_bits = np.asarray(mesa_bits, np.uint32), np.asarray(cpu_bits, np.uint32)
    listed = np.flatnonzero(~within(cpu_bits, mesa_bits).reshape(-1)).astype(np.int32)
    return dict(mesa_bits=mesa_bits, listed=listed, listed_bits=cpu_bits.reshape(-1, 4)[listed])


def check(frame, entry, label=""):
    """`frame` (h, w, 4) float32 against one entry: within TOLERANCE of Mesa off the list (NaN only where Mesa has NaN),
    the CPU reference's bits on the list."""
    mesa = np.asarray(entry["mesa_bits"], np.uint32)
    bits = np.ascontiguousarray(frame, np.float32).view(np.uint32)
    assert bits.shape == mesa.shape, f"{label}: frame {bits.shape}, fixture {mesa.shape}"
    listed = np.asarray(entry["listed"], np.int64)
    off = np.ones(mesa.shape[0] * mesa.shape[1], bool)
    off[listed] = False
    bad = off & ~within(bits, mesa).reshape(-1)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        got, want = bits.reshape(-1, 4)[k].view(np.float32), mesa.reshape(-1, 4)[k].view(np.float32)
        raise AssertionError(f"{label}: {int(bad.sum())} pixels off the list are beyond {TOLERANCE} from Mesa; first at "
                             f"(x {k % mesa.shape[1]}, y {k // mesa.shape[1]}): {got} against {want}")
    on = T.bits_equal(bits.reshape(-1, 4)[listed].view(np.float32), np.asarray(entry["listed_bits"], np.uint32).view(np.float32)).all(axis=-1)
    assert on.all(), f"{label}: {int((~on).sum())} of {len(listed)} listed pixels do not have the CPU reference's bits"


# ---------------------------------------------------------------------------------------------
# the files
# ---------------------------------------------------------------------------------------------
def family_file(family, name):
    return os.path.join(MESA_DIR, (name if family == "frames" else family) + ".npz")


def store_keys(family, name):
    prefix = "" if family == "frames" else name + "."
    return {k: prefix + k for k in ("mesa_bits", "listed", "listed_bits")}


_files = {}


def load(family, name):
    path = family_file(family, name)
    if path not in _files:
        with np.load(path) as z:
            _files[path] = {k: z[k] for k in z.files}
    return {k: _files[path][full] for k, full in store_keys(family, name).items()}


def load_teleport():
    path = os.path.join(MESA_DIR, "teleport.npz")
    if path not in _files:
        with np.load(path) as z:
            _files[path] = {k: z[k] for k in z.files}
    return _files[path]


def unpack_reference_teleport(scene):
    """reference_text/teleport.npz, the framebuffer route -> (flags (n, 3) bool, position bits (n, 3) uint32)"""
    rows = np.load(os.path.join(T.GOLDEN_DIR, "teleport.npz"))[scene][:, 6:12]
    return rows[:, :3].astype(bool), rows[:, 3:6].astype(np.uint32)


def position_distance(bits_a, bits_b):
    """largest |a - b| over the components of two positions given as float bits"""
    a, b = np.asarray(bits_a, np.uint32).view(np.float32).astype(np.float64), np.asarray(bits_b, np.uint32).view(np.float32).astype(np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0
