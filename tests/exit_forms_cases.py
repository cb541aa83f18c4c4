"""What tests/test_exit_forms.py (host) and tests/test_gpu_exit_forms.py (gfx950) share: the frame cases of the `-DPTL_SPELLED_EXITS` A/B
 and the host frames they are compared with.  Not a test module."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORPUS = os.path.join(ROOT, "tests", "corpus")
W, H = 96, 54  # three workgroups wide, six and three quarter row blocks high: the partial block is covered
SPELLED = "PTL_SPELLED_EXITS"

# (id, scene file relative to the repository, render depth).  sphere_to_plane is the corpus scene with Complex (custom) materials AND two
# intersection-material snippets: the first is adopted by the flag alone, the second through nearer().
CASES = [
    ("portal_in_portal", "scenes/portal_in_portal.ron", 40),
    ("monoportal", "scenes/monoportal.ron", 20),
    ("mobius_monoportal", "scenes/mobius_monoportal.ron", 64),
    ("sphere_to_plane", "tests/corpus/scenes/sphere_to_plane.ron", 20),
]
CASE_IDS = [c[0] for c in CASES]


def asset_root(scene_file):
    """The corpus scenes find their textures beside the corpus; so does an edited copy of one (an absolute path)."""
    return CORPUS if scene_file.startswith("tests/corpus/") or os.path.isabs(scene_file) else None


def renderer(pa, scene_file, depth, flags, device, aa_count=1):
    scene = pa.Scene.from_file(os.path.join(ROOT, scene_file))
    extra = {"asset_root": asset_root(scene_file)} if asset_root(scene_file) else {}
    r = pa.SceneRenderer(scene, device=device, flags=flags, **extra)
    r.set_option("render_depth", depth)
    r.set_option("aa_count", aa_count)
    return scene, r


def host_kernel(pa, scene_file, depth, flags, defines=(), aa_count=1, extra_source=""):
    """The host build of the scene's generated source (plus `extra_source`), loaded with the uniforms a W x H draw would upload."""
    from oracle import host_build as hb

    scene, r = renderer(pa, scene_file, depth, flags, -1, aa_count)
    layout, size = scene.uniform_layout()
    generated = tuple(d for d in scene.generated_defines() if d != "PTL_COUNT_SEGMENTS" and not d.startswith("PTL_WAVES_PER_EU") and d != "PTL_QUICK_JIT")
    hk = hb.HostKernel(scene.generate_source(flags) + extra_source, layout, size, defines=generated + tuple(defines))
    for name, typ, _ in layout:
        if typ == pa.PTL_SAMPLER:
            continue
        v = r.uniform_value(name, W, H)
        if v is not None:
            hk.set_uniform(name, v)
    # ... and with the scene's textures bound, as the device draws them (decoded with PIL, like oracle.host_build.host_kernel_for)
    from PIL import Image

    root, paths = asset_root(scene_file) or ROOT, scene.textures()
    for name, typ, _ in layout:
        rel = paths.get(name[: -len("_tex")]) if typ == pa.PTL_SAMPLER else None
        if rel is not None and os.path.exists(os.path.join(root, rel)):
            hk.set_texture(name, np.array(Image.open(os.path.join(root, rel)).convert("RGBA")))
    return hk


_HOST_FRAMES = {}


def host_frame(pa, scene_file, depth, flags, defines=(), aa_count=1):
    """-> (float bits, rgba8) of the W x H host frame; computed once per process and case, handed out read-only."""
    key = (scene_file, depth, flags, tuple(defines), aa_count)
    if key not in _HOST_FRAMES:
        f = host_kernel(pa, scene_file, depth, flags, defines, aa_count).render(W, H)
        bits, rgba8 = f["rgba32f"].view(np.uint32).copy(), f["rgba8"].copy()
        bits.setflags(write=False)
        rgba8.setflags(write=False)
        _HOST_FRAMES[key] = (bits, rgba8)
    return _HOST_FRAMES[key]
