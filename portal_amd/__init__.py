"""portal_amd -- MI355X-native offline renderer for optozorax/portal scenes.

Python is only the thin host-side mirror of the reference's operator interface
(``Scene`` / ``SceneRenderer``, reference src/gui/scene.rs and src/main.rs:732-1544) over the
C ABI of ``libportal_amd.so`` (include/portal_amd.h).  All work -- .ron loading, uniform /
matrix evaluation, scene -> HIP source generation, hiprtc compilation, kernel launch --
happens in the native library; there is no Python or CPU fallback for the render path: if
the library or a GPU is missing the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libportal_amd.so")

# default code-object cache (gfx950 binaries keyed by source hash); travels with the repo
os.environ.setdefault("PTL_CACHE_DIR", os.path.join(_HERE, "_cache"))



def _share_torch_hip_runtime() -> None:
    """One HIP runtime per process: PyTorch ships its own libamdhip64 and loads it on `import torch`.  If this library
    bound /opt/rocm's copy first and torch came later, the process would hold two runtimes whose streams and device
    pointers do not mix.  So when torch is installed but not imported yet, point the C side at torch's copy by path
    (importing torch itself would cost seconds for callers that never need it)."""
    if "PTL_HIP_LIB" in os.environ:
        return
    import importlib.util

    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    for root in (spec.submodule_search_locations if spec and spec.submodule_search_locations else []):
        cand = os.path.join(root, "lib", "libamdhip64.so")
        if os.path.exists(cand):
            os.environ["PTL_HIP_LIB"] = cand  # hiprtc stays /opt/rocm's: a compiler, not shared state
            return


_share_torch_hip_runtime()

PTL_MAT4, PTL_F32, PTL_I32, PTL_VEC2, PTL_VEC3, PTL_SAMPLER = range(6)
FLAG_SPECIALIZE_INTS = 1
FLAG_COUNT_SEGMENTS = 2
FLAG_SPECIALIZE_ALL = 4
FLAG_SPECIALIZE_STATIC = 8  # bake what stays constant while a clip plays (checked before every draw, rebuilt if it moved)
FLAG_ANAGLYPH = 16  # compile the anaglyph stereo mode in (the reference's `disable_anaglyph = false`)
FLAG_NO_DERIVED_UNIFORMS = 32  # keep the per-call plane tests (default: ray-independent halves evaluated by the prologue kernel)
FLAG_NO_FIRST_TRIP = 8192  # no first-trip copies of the intersection-material snippets (round 6: the un-specialised kernel has none unless FLAG_KEEP_TRANSFORM_DODGES asks)
FLAG_NO_UNIFORM_HOIST = 4096  # scene snippets evaluate their uniform-only expressions per ray (default: once per upload, in the prologue kernel)
FLAG_NO_DEFERRED_UPDATES = 128  # translate scene snippets exactly as written (default: loop-carried ray transforms are applied lazily)
FLAG_QUICK_JIT = 262144  # compile at -O1 instead of the shipped -O3: half the JIT time, a 5-20 % slower kernel (one-off frames)
FLAG_SPECIALIZE_PATTERNS = 1048576  # compile in only what survives moving values: zero patterns of the matrices + the renderer's mode switches
FLAG_BOUNDED_SNIPPETS = 2097152  # opt-in: scene_intersect first, its hit distance bounds the intersection-material snippets (exact; measured: no gain on the headline)
FLAG_KEEP_TRANSFORM_DODGES = 16777216  # A/B, round 4's shape: the first-trip forms (snippet copies + plane tests) also in the un-specialised kernel (opt-in there since round 6), snippet copies + deferred loop updates also with affine rays; identical frames
FLAG_MATERIAL_TABLE_LDS = 1 << 26  # A/B (measured slower, off by default): the Simple materials' literals in a per-workgroup LDS table, ONE material_simple2 call
FLAG_MATERIAL_TABLE_SCALAR = 1 << 27  # A/B (measured: no gain): the same table in constant memory, a scalar load per distinct material of the wave (waterfall)
FLAG_CHECK_AFFINE = 1 << 25  # diagnostics: general products, and `segments` counts the ray halves that meet a product / the bounce loop with a w that is not 1 / 0
FLAG_NO_AFFINE_RAYS = 8388608  # A/B: matrix-times-ray products never assume o.w = 1 / d.w = 0 (default in specialised builds of affine scenes: they do; identical frames)
FLAG_REFINE = 1 << 28  # adaptive anti-aliasing: a second render entry that shades a device-side list of pixels (SceneRenderer.draw_adaptive)
FLAG_REFINE_SLICES = 1 << 29  # FLAG_SLICES (implied) plus the refine entry over the slices of a launch (SceneRenderer.draw_slices_adaptive); not with FLAG_REFINE
FLAG_PASSES = 1 << 30  # trace passes: a 16-byte record per pixel beside the colour (PASS_RECORD; SceneRenderer.draw_passes); not with FLAG_ANAGLYPH / _REFINE / _REFINE_SLICES / _CHECK_AFFINE
FLAG_SLICES = 4194304  # the render entry reads its uniform block from a buffer of blocks (one per blockIdx.z): stage_slice / draw_slices, one launch for several draws
FLAG_NO_ZERO_MASKS = 524288  # A/B: run-time matrices keep their full products although their zero pattern is known (KernelOptions::mask_zero_elements)
FLAG_ASYNC_REJIT = 131072  # a specialised renderer never stalls on a rebuild: it draws with the un-specialised kernel until a worker thread has the new one
FLAG_NO_FIRST_TRIP_PLANES = 65536  # no first-trip copy of the generated plane tests (round 6: the un-specialised kernel has none unless FLAG_KEEP_TRANSFORM_DODGES asks)
FLAG_NO_UNROLL = 32768  # keep snippet loops whose bound is a baked Int uniform as loops (default: unrolled up to 16 iterations; identical frames)
FLAG_EXACT_CR = 16384  # numerics contract 1 of rounds 1-2: IEEE correctly rounded / and sqrt on EVERY input (default: contract 2, device/ptl_glsl.h)
FLAG_FAST_MATH = 64  # tolerance mode: hardware rcp / sqrt estimates, FMA contraction (not bit-exact; exact stays the default)


def flag_waves(n: int) -> int:
    """Occupancy hint for SceneRenderer flags: build with __launch_bounds__(256, n)."""
    return (int(n) & 0xF) << 8


class PortalError(RuntimeError):
    pass


class UniformDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("type", C.c_int), ("offset", C.c_size_t)]


class CalculatedCam(C.Structure):
    """ptl_calculated_cam (CalculatedCam, src/gui/camera.rs:22-32)."""

    _fields_ = [("look_at", C.c_double * 3), ("alpha", C.c_double), ("beta", C.c_double), ("r", C.c_double), ("free_movement", C.c_int),
                ("in_subspace", C.c_int), ("override_matrix", C.c_int), ("matrix", C.c_double * 16)]


class Frame(C.Structure):
    """Row-block sharding of one frame (ptl_frame)."""

    _fields_ = [("width", C.c_int), ("height", C.c_int), ("rb_phase", C.c_int), ("rb_stride", C.c_int), ("in_place", C.c_int)]


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise PortalError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` or `make`")
    lib = C.CDLL(LIB_PATH)
    vp, cp, ci, cd, cs = C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_size_t
    P = C.POINTER
    sig = {
        "ptl_last_error": (cp, []),
        "ptl_version": (cp, []),
        "ptl_device_count": (ci, []),
        "ptl_kernel_compile": (ci, [ci, cp, P(UniformDesc), ci, cs, P(cp), ci, P(vp), cp, cs]),
        "ptl_kernel_code_object": (ci, [vp, P(vp), P(cs)]),
        "ptl_kernel_resources": (ci, [vp, P(ci), P(ci), P(ci)]),
        "ptl_kernel_set_uniform": (ci, [vp, cp, ci, vp]),
        "ptl_kernel_set_texture": (ci, [vp, cp, vp, ci, ci]),
        "ptl_frame_shard_rows": (ci, [P(Frame)]),
        "ptl_kernel_render": (ci, [vp, P(Frame), vp, vp, vp, vp, P(C.c_float)]),
        "ptl_kernel_render_to_host": (ci, [vp, P(Frame), vp, vp, P(C.c_uint64), P(C.c_float)]),
        "ptl_kernel_teleport_ray": (ci, [vp, P(C.c_float), P(C.c_float), P(C.c_float), P(ci), P(ci), P(ci)]),
        "ptl_kernel_destroy": (None, [vp]),
        "ptl_scene_load_file": (ci, [cp, P(vp)]),
        "ptl_scene_load_text": (ci, [cp, P(vp)]),
        "ptl_scene_free": (None, [vp]),
        "ptl_scene_set_uniform": (ci, [vp, cp, cd]),
        "ptl_scene_set_time": (ci, [vp, cd, cd]),
        "ptl_scene_set_trefoil": (ci, [vp, cp, cp]),
        "ptl_scene_get_trefoil": (ci, [vp, cp, cp, cs]),
        "ptl_scene_init_stage": (ci, [vp, cp, cp, cs]),
        "ptl_scene_stage_name": (ci, [vp, ci, cp, cs]),
        "ptl_scene_camera_name": (ci, [vp, ci, cp, cs]),
        "ptl_scene_set_camera_matrix": (ci, [vp, P(cd)]),
        "ptl_scene_animation": (ci, [vp, ci, cp, cs, P(cd)]),
        "ptl_scene_init_animation": (ci, [vp, cp]),
        "ptl_scene_update": (ci, [vp, cd, P(cd), P(cd), P(ci), P(CalculatedCam)]),
        "ptl_renderer_update": (ci, [vp, cd, P(ci), P(ci)]),
        "ptl_renderer_rejit_count": (ci, [vp]),
        "ptl_renderer_rejit_pending": (ci, [vp]),
        "ptl_scene_eval_uniform": (ci, [vp, cp, P(ci), P(cd)]),
        "ptl_scene_eval_matrix": (ci, [vp, cp, P(cd)]),
        "ptl_scene_cam": (ci, [vp, P(cd)]),
        "ptl_scene_texture": (ci, [vp, ci, cp, cs, cp, cs]),
        "ptl_scene_generate_source": (ci, [vp, C.c_uint, P(vp)]),
        "ptl_scene_generated_defines": (ci, [vp, cp, cs]),
        "ptl_scene_zero_mask_probes": (ci, [vp, P(ci), P(ci)]),
        "ptl_scene_uniform_layout": (ci, [vp, P(P(UniformDesc)), P(ci), P(cs)]),
        "ptl_scene_set_uniforms": (ci, [vp, vp]),
        "ptl_scene_visit_uniforms": (ci, [vp, vp, vp]),
        "ptl_scene_source_line_owner": (ci, [vp, ci, cp, cs, cp, cs, P(ci)]),
        "ptl_free": (None, [vp]),
        "ptl_renderer_create": (ci, [vp, ci, cp, C.c_uint, P(vp), cp, cs]),
        "ptl_renderer_kernel_source": (ci, [vp, P(vp)]),
        "ptl_renderer_join": (ci, [vp, vp]),
        "ptl_renderer_stage_slice": (ci, [vp, P(Frame), ci]),
        "ptl_renderer_draw_slices": (ci, [vp, P(Frame), ci, vp, vp, C.c_ulonglong, vp, P(C.c_float)]),
        "ptl_kernel_max_slices": (ci, [vp]),
        "ptl_kernel_stage_slice": (ci, [vp, ci]),
        "ptl_kernel_hold_textures": (ci, [vp, ci]),
        "ptl_renderer_affine_rays": (ci, [vp]),
        "ptl_renderer_check_affine": (ci, [vp, ci, ci, P(C.c_ulonglong)]),
        "ptl_dmath": (ci, [cp, P(cd), P(cd), P(cd), P(cd)]),
        "ptl_snippets_keep_rays_affine": (ci, [cp, cp, cs]),
        "ptl_code_object_note": (ci, [vp, cs, cp, cp]),
        "ptl_kernel_render_slices": (ci, [vp, P(Frame), ci, vp, vp, C.c_ulonglong, vp, P(C.c_float)]),
        "ptl_kernel_clone": (ci, [vp, P(vp)]),
        "ptl_kernel_copy_uniforms": (ci, [vp, vp]),
        "ptl_renderer_create_with_options": (ci, [vp, ci, cp, C.c_uint, P(cp), P(cd), ci, P(vp), cp, cs]),
        "ptl_renderer_set_option": (ci, [vp, cp, cd]),
        "ptl_renderer_set_camera": (ci, [vp, P(cd), cd, cd, cd]),
        "ptl_renderer_use_camera": (ci, [vp, cp]),
        "ptl_renderer_uniform_value": (ci, [vp, ci, ci, cp, P(C.c_float), P(ci)]),
        "ptl_renderer_draw": (ci, [vp, P(Frame), vp, vp, vp, vp, P(C.c_float)]),
        "ptl_renderer_draw_to_host": (ci, [vp, P(Frame), vp, vp, P(C.c_uint64), P(C.c_float)]),
        "ptl_renderer_teleport_ray": (ci, [vp, P(cd), P(cd), P(cd), P(ci), P(ci), P(ci)]),
        "ptl_renderer_prebuild_teleport": (ci, [vp]),
        "ptl_kernel_prebuild_teleport": (ci, [vp]),
        "ptl_renderer_move_camera": (ci, [vp, P(cd), cd, cd, cd, P(ci), P(ci)]),
        "ptl_renderer_camera_state": (ci, [vp, P(cd), P(ci), P(cd)]),
        "ptl_renderer_kernel": (vp, [vp]),
        "ptl_renderer_destroy": (None, [vp]),
        "ptl_deinterleave_rows": (ci, [vp, P(Frame), vp]),
        "ptl_average_images": (ci, [ci, P(vp), ci, vp, ci, ci, vp, P(C.c_float)]),
        "ptl_average_to_yuv420p10": (ci, [ci, P(vp), ci, vp, ci, ci, vp, P(C.c_float)]),
        "ptl_average_f32_to_yuv420p10": (ci, [ci, P(vp), ci, vp, ci, ci, vp, P(C.c_float)]),
        "ptl_yuv420p10_frame_bytes": (cs, [ci, ci]),
        "ptl_average_to_yuv10": (ci, [ci, P(vp), ci, vp, ci, ci, ci, vp, P(C.c_float)]),
        "ptl_average_f32_to_yuv10": (ci, [ci, P(vp), ci, vp, ci, ci, ci, vp, P(C.c_float)]),
        "ptl_yuv10_frame_bytes": (cs, [ci, ci, ci]),
        "ptl_average_f32_to_rgb48": (ci, [ci, P(vp), ci, vp, ci, ci, ci, vp, P(C.c_float)]),
        "ptl_rgb48_frame_bytes": (cs, [ci, ci]),
        "ptl_png_write_rgb48": (ci, [cp, vp, ci, ci, ci, ci]),
        "ptl_png_stream_bytes": (cs, [ci, ci]),
        "ptl_png_stream_band_rows": (ci, [ci]),
        "ptl_png_stream_download_bytes": (cs, [ci, ci]),
        "ptl_png_deflate_rgba8": (ci, [ci, vp, ci, ci, vp, vp, P(C.c_float)]),
        "ptl_png_deflate_rgba8_codes": (ci, [ci, vp, ci, ci, ci, vp, vp, P(C.c_float)]),
        "ptl_png_write_stream": (ci, [cp, vp, ci, ci]),
        "ptl_png_stream16_bytes": (cs, [ci, ci]),
        "ptl_png_stream16_band_rows": (ci, [ci]),
        "ptl_png_stream16_download_bytes": (cs, [ci, ci]),
        "ptl_png_deflate_rgb48": (ci, [ci, vp, ci, ci, ci, vp, vp, P(C.c_float)]),
        "ptl_png_write_stream_rgb48": (ci, [cp, vp, ci, ci]),
        "ptl_png_write_stream_gray16": (ci, [cp, vp, ci, ci]),
        "ptl_pass_record_bytes": (cs, [ci, ci]),
        "ptl_kernel_render_passes": (ci, [vp, P(Frame), vp, vp, vp, cs, vp, vp, P(C.c_float)]),
        "ptl_kernel_render_slices_passes": (ci, [vp, P(Frame), ci, vp, vp, vp, cs, C.c_ulonglong, vp, P(C.c_float)]),
        "ptl_renderer_draw_passes": (ci, [vp, P(Frame), vp, vp, vp, cs, vp, vp, P(C.c_float)]),
        "ptl_renderer_draw_slices_passes": (ci, [vp, P(Frame), ci, vp, vp, vp, cs, C.c_ulonglong, vp, P(C.c_float)]),
        "ptl_pass_stats": (ci, [ci, vp, C.c_long, vp, vp, ci, vp, P(C.c_float)]),
        "ptl_pass_stats_depth_range": (ci, [vp, P(C.c_float), P(C.c_float)]),
        "ptl_passes_to_gray16": (ci, [ci, vp, C.c_long, vp, ci, C.c_float, C.c_float, vp, P(C.c_float)]),
        "ptl_png_write_gray16": (ci, [cp, vp, ci, ci, ci]),
        "ptl_pass_slices_to_gray16": (ci, [ci, vp, ci, C.c_ulonglong, C.c_long, vp, vp, vp, C.c_float, C.c_float, vp, P(C.c_float)]),
        "ptl_aa_edges": (ci, [ci, vp, ci, ci, ci, vp, vp, vp, P(C.c_float)]),
        "ptl_kernel_render_refine": (ci, [vp, P(Frame), vp, vp, vp, vp, vp, vp, P(C.c_float)]),
        "ptl_renderer_draw_adaptive": (ci, [vp, P(Frame), vp, vp, vp, P(C.c_float)]),
        "ptl_renderer_adaptive_result": (ci, [vp, P(vp), P(vp)]),
        "ptl_renderer_adaptive_times": (ci, [vp, P(C.c_float)]),
        "ptl_aa_edges_slices": (ci, [ci, vp, C.c_ulonglong, ci, ci, ci, ci, vp, C.c_ulonglong, vp, vp, P(C.c_float)]),
        "ptl_kernel_set_staged_uniform": (ci, [vp, ci, cp, ci, vp]),
        "ptl_kernel_render_slices_refine": (ci, [vp, P(Frame), ci, vp, C.c_ulonglong, vp, vp, vp, C.c_ulonglong, vp, vp, P(C.c_float)]),
        "ptl_renderer_draw_slices_adaptive": (ci, [vp, P(Frame), ci, vp, vp, C.c_ulonglong, vp, P(C.c_float)]),
        "ptl_renderer_adaptive_slices_result": (ci, [vp, P(vp), P(C.c_ulonglong), P(vp)]),
        "ptl_y4m_header": (ci, [ci, ci, ci, cp, cs]),
        "ptl_y4m_header_chroma": (ci, [ci, ci, ci, ci, cp, cs]),
        "ptl_device_alloc": (ci, [ci, cs, P(vp)]),
        "ptl_device_free": (ci, [vp]),
        "ptl_device_download": (ci, [vp, vp, cs, vp]),
        "ptl_device_memset": (ci, [vp, ci, cs, vp]),
        "ptl_device_copy2d_async": (ci, [vp, cs, vp, cs, cs, cs, vp]),
        "ptl_ipc_export": (ci, [vp, cp]),
        "ptl_ipc_open": (ci, [ci, cp, P(vp)]),
        "ptl_ipc_close": (ci, [vp]),
        "ptl_frame_group_create": (ci, [vp, P(ci), ci, cp, C.c_uint, ci, P(vp), cp, cs]),
        "ptl_frame_group_size": (ci, [vp]),
        "ptl_frame_group_renderer": (vp, [vp, ci]),
        "ptl_frame_group_set_option": (ci, [vp, cp, cd]),
        "ptl_frame_group_use_camera": (ci, [vp, cp]),
        "ptl_frame_group_set_camera": (ci, [vp, P(cd), cd, cd, cd]),
        "ptl_frame_group_update": (ci, [vp, cd]),
        "ptl_frame_group_draw": (ci, [vp, ci, ci, P(vp), P(C.c_float)]),
        "ptl_frame_group_submit": (ci, [vp, ci, ci, P(ci)]),
        "ptl_frame_group_wait": (ci, [vp, ci, P(vp), P(C.c_float)]),
        "ptl_frame_group_download": (ci, [vp, vp]),
        "ptl_frame_group_destroy": (None, [vp]),
        "ptl_host_alloc": (ci, [cs, P(vp)]),
        "ptl_host_free": (ci, [vp]),
        "ptl_ron_format": (vp, [cp]),
        "ptl_scene_to_ron": (ci, [vp, P(vp)]),
        "ptl_png_read": (ci, [cp, P(vp), P(ci), P(ci)]),
        "ptl_png_write": (ci, [cp, vp, ci, ci]),
        "ptl_strstore_new": (vp, []),
        "ptl_strstore_free": (None, [vp]),
        "ptl_strstore_add_string": (None, [vp, cp]),
        "ptl_strstore_add_identifier_string": (None, [vp, cp, cp, cp]),
        "ptl_apply_template": (vp, [cp, P(cp), P(vp), ci]),
        "ptl_strstore_text": (cp, [vp]),
        "ptl_strstore_current_line": (ci, [vp]),
        "ptl_strstore_range": (ci, [vp, cp, cp, P(ci), P(ci)]),
        "ptl_strstore_get_identifier": (ci, [vp, ci, cp, cs, cp, cs, P(ci)]),
        "ptl_select_sections": (vp, [cp, P(cp), ci]),
        "ptl_device_source": (cp, [cp]),
        "ptl_translate_glsl": (vp, [cp]),
        "ptl_translate_library_glsl": (vp, [cp]),
        "ptl_bound_glsl": (vp, [cp, cp, P(ci)]),
        "ptl_formula_eval": (ci, [cp, P(cp), P(cd), ci, cd, P(cd)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    return lib


_lib: Optional[C.CDLL] = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        _lib = _load()
    return _lib


def _err() -> str:
    return lib().ptl_last_error().decode("utf-8", "replace")


def last_error() -> str:
    """ptl_last_error(): the message of the most recent failure -- or note, e.g. why a renderer switched affine rays off -- on this thread."""
    return _err()


def _check(rc: int, what: str) -> int:
    if rc < 0:
        raise PortalError(f"{what} failed ({rc}): {_err()}")
    return rc


def version() -> str:
    return lib().ptl_version().decode()


def device_count() -> int:
    return lib().ptl_device_count()


def shard_rows(frame: Frame) -> int:
    return lib().ptl_frame_shard_rows(C.byref(frame))


# --------------------------------------------------------------------------------------------
class Scene:
    """A loaded .ron scene (reference: Scene::from_serialized, src/gui/scene.rs:142-146)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_file(cls, path: str) -> "Scene":
        h = C.c_void_p()
        rc = lib().ptl_scene_load_file(path.encode(), C.byref(h))
        if rc != 0:
            raise PortalError(f"Failed to parse scene `{path}`: {_err()}")
        return cls(h)

    @classmethod
    def from_text(cls, text: str) -> "Scene":
        h = C.c_void_p()
        rc = lib().ptl_scene_load_text(text.encode("utf-8"), C.byref(h))
        if rc != 0:
            raise PortalError(f"Failed to parse scene: {_err()}")
        return cls(h)

    def __del__(self):
        try:
            if self._h:
                lib().ptl_scene_free(self._h)
                self._h = None
        except Exception:
            pass

    def set_uniform(self, name: str, value: float) -> bool:
        return lib().ptl_scene_set_uniform(self._h, name.encode(), float(value)) == 0

    def set_time(self, time: float, total_time: Optional[float] = None) -> None:
        lib().ptl_scene_set_time(self._h, float(time), float(time if total_time is None else total_time))

    def init_stage(self, name: str) -> str:
        """Scene::init_stage_by_name (`render-frame --stage`).  Returns the camera the stage selects ("" = original)."""
        cam = C.create_string_buffer(256)
        rc = _check(lib().ptl_scene_init_stage(self._h, name.encode("utf-8"), cam, 256), "init_stage")
        if rc != 0:
            raise PortalError(f"Scene has no stage named `{name}`")
        return cam.value.decode("utf-8")

    def set_camera_matrix(self, m) -> None:
        """What Matrix::Camera evaluates to: 4x4, m[row][col] (a renderer sends its camera's matrix itself)."""
        a = (C.c_double * 16)(*np.asarray(m, np.float64).reshape(4, 4).T.reshape(-1))
        _check(lib().ptl_scene_set_camera_matrix(self._h, a), "set_camera_matrix")

    def set_trefoil(self, name: str, text: str) -> None:
        """A Trefoil uniform from the reference's text form, e.g. "1a 2a G,1b 3b B,2a 1a S" (TrefoilSpecial::decode)."""
        if _check(lib().ptl_scene_set_trefoil(self._h, name.encode(), text.encode()), "set_trefoil") != 0:
            raise PortalError(f"`{name}` is not a Trefoil uniform, or `{text}` does not decode")

    def get_trefoil(self, name: str) -> str:
        buf = C.create_string_buffer(512)
        if _check(lib().ptl_scene_get_trefoil(self._h, name.encode(), buf, 512), "get_trefoil") != 0:
            raise PortalError(f"`{name}` is not a Trefoil uniform")
        return buf.value.decode()

    def to_ron(self) -> str:
        """The scene as a .ron document in the reference's layout (its writer: serialize_scene_new_format + pretty RON)."""
        p = C.c_void_p()
        _check(lib().ptl_scene_to_ron(self._h, C.byref(p)), "to_ron")
        try:
            return C.string_at(p).decode("utf-8")
        finally:
            lib().ptl_free(p)

    def animations(self):
        """[(name, duration seconds)] of the scene's real animations (the clips `render` turns into videos)."""
        out, i, buf, dur = [], 0, C.create_string_buffer(256), C.c_double()
        while lib().ptl_scene_animation(self._h, i, buf, 256, C.byref(dur)) == 0:
            out.append((buf.value.decode("utf-8"), dur.value))
            i += 1
        return out

    def init_animation(self, name: str) -> None:
        """Scene::init_animation_by_name (`render-frame --animation`, `render`)."""
        if _check(lib().ptl_scene_init_animation(self._h, name.encode("utf-8")), "init_animation") != 0:
            raise PortalError(f"Scene has no animation named `{name}`")

    def update(self, seconds: float) -> dict:
        """Scene::update -> {"time", "total_time", "camera": None | dict(look_at, alpha, beta, r, ...)}."""
        t, tt, has, cam = C.c_double(), C.c_double(), C.c_int(), CalculatedCam()
        _check(lib().ptl_scene_update(self._h, float(seconds), C.byref(t), C.byref(tt), C.byref(has), C.byref(cam)), "update")
        camera = None
        if has.value:
            camera = dict(look_at=list(cam.look_at), alpha=cam.alpha, beta=cam.beta, r=cam.r, free_movement=bool(cam.free_movement),
                          in_subspace=bool(cam.in_subspace), override_matrix=bool(cam.override_matrix),
                          matrix=np.array(cam.matrix, np.float64).reshape(4, 4).T.copy())
        return {"time": t.value, "total_time": tt.value, "camera": camera}

    def _names(self, fn):
        out, i, buf = [], 0, C.create_string_buffer(256)
        while fn(self._h, i, buf, 256) == 0:
            out.append(buf.value.decode("utf-8"))
            i += 1
        return out

    def stages(self):
        return self._names(lib().ptl_scene_stage_name)

    def cameras(self):
        return self._names(lib().ptl_scene_camera_name)

    def eval_uniform(self, name: str):
        """AnyUniform::get -> bool | int | float, or None if it cannot be evaluated."""
        kind, val = C.c_int(), C.c_double()
        rc = lib().ptl_scene_eval_uniform(self._h, name.encode(), C.byref(kind), C.byref(val))
        _check(rc, "eval_uniform")
        if rc != 0:
            return None
        return bool(val.value) if kind.value == 0 else int(val.value) if kind.value == 1 else val.value

    def eval_matrix(self, name: str) -> Optional[np.ndarray]:
        """Matrix::get as a 4x4 float64 array, m[row, col] (stored column-major in the ABI)."""
        out = (C.c_double * 16)()
        rc = lib().ptl_scene_eval_matrix(self._h, name.encode(), out)
        _check(rc, "eval_matrix")
        if rc != 0:
            return None
        return np.array(out, dtype=np.float64).reshape(4, 4).T.copy()

    def cam(self) -> dict:
        out = (C.c_double * 7)()
        _check(lib().ptl_scene_cam(self._h, out), "scene_cam")
        return {"look_at": tuple(out[0:3]), "alpha": out[3], "beta": out[4], "r": out[5], "offset_after_material": out[6]}

    def textures(self) -> dict:
        """name -> path of the scene's textures (src/gui/texture.rs)."""
        out, i = {}, 0
        name, path = C.create_string_buffer(256), C.create_string_buffer(1024)
        while lib().ptl_scene_texture(self._h, i, name, 256, path, 1024) == 0:
            out[name.value.decode()] = path.value.decode()
            i += 1
        return out

    def generate_source(self, flags: int = 0) -> str:
        """Scene::generate_shader_code: the complete HIP C++ translation unit."""
        p = C.c_void_p()
        _check(lib().ptl_scene_generate_source(self._h, flags, C.byref(p)), "generate_source")
        try:
            return C.string_at(p).decode("utf-8")
        finally:
            lib().ptl_free(p)

    def zero_mask_probes(self):
        """(reused, probed): generations that reused the last zero patterns / that probed the scene for them."""
        a, b = C.c_int(), C.c_int()
        _check(lib().ptl_scene_zero_mask_probes(self._h, C.byref(a), C.byref(b)), "zero_mask_probes")
        return a.value, b.value

    def generated_defines(self):
        """The preprocessor defines that go with the source generated last (``generate_source`` / a renderer's build)."""
        buf = C.create_string_buffer(4096)
        _check(lib().ptl_scene_generated_defines(self._h, buf, len(buf)), "generated_defines")
        return tuple(buf.value.decode().split())

    def uniform_layout(self):
        """[(name, type, offset)], block_size -- Scene::uniforms plus the block layout."""
        descs, n, size = C.POINTER(UniformDesc)(), C.c_int(), C.c_size_t()
        _check(lib().ptl_scene_uniform_layout(self._h, C.byref(descs), C.byref(n), C.byref(size)), "uniform_layout")
        return [(descs[i].name.decode(), descs[i].type, descs[i].offset) for i in range(n.value)], size.value

    def uniform_values(self) -> dict:
        """What Scene::set_uniforms uploads: name -> float32 array (mat4: 4x4 m[row, col]) or int."""
        out = {}
        CB = C.CFUNCTYPE(None, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p)

        def cb(_user, name, typ, value):
            if typ == PTL_MAT4:
                out[name.decode()] = np.ctypeslib.as_array(C.cast(value, C.POINTER(C.c_float)), (16,)).copy().reshape(4, 4).T.copy()
            elif typ == PTL_I32:
                out[name.decode()] = int(C.cast(value, C.POINTER(C.c_int))[0])
            else:
                out[name.decode()] = np.float32(C.cast(value, C.POINTER(C.c_float))[0])

        fn = CB(cb)
        _check(lib().ptl_scene_visit_uniforms(self._h, C.cast(fn, C.c_void_p), None), "visit_uniforms")
        return out

    def source_line_owner(self, line: int):
        kind, name, local = C.create_string_buffer(64), C.create_string_buffer(256), C.c_int()
        rc = lib().ptl_scene_source_line_owner(self._h, line, kind, 64, name, 256, C.byref(local))
        if rc != 0:
            return None
        return kind.value.decode(), name.value.decode(), local.value


class SceneRenderer:
    """Reference: SceneRenderer (src/main.rs:732-1544), the offline image path.

    ``device=-1`` builds a GPU-less renderer (source generation, hiprtc compile, uniform
    queries); drawing then raises.
    """

    def __init__(self, scene: Scene, device: int = 0, asset_root: Optional[str] = None, flags: int = 0, options: Optional[dict] = None):
        """``options``: renderer options (``set_option`` names) applied before the first build -- a specialised renderer compiles its
        mode switches in, so e.g. ``options={"draw_side_by_side": 1}`` gets the side-by-side kernel from the start."""
        self.scene = scene
        h = C.c_void_p()
        log = C.create_string_buffer(1 << 16)
        root = (asset_root if asset_root is not None else REPO_ROOT).encode()
        if options:
            names = (C.c_char_p * len(options))(*[k.encode() for k in options])
            values = (C.c_double * len(options))(*[float(v) for v in options.values()])
            rc = lib().ptl_renderer_create_with_options(scene._h, device, root, flags, names, values, len(options), C.byref(h), log, len(log))
        else:
            rc = lib().ptl_renderer_create(scene._h, device, root, flags, C.byref(h), log, len(log))
        self.compile_log = log.value.decode("utf-8", "replace")
        if rc != 0:
            raise PortalError(f"SceneRenderer::new failed ({rc}): {_err()}\n{self.compile_log}")
        self._h = h
        self.device = device

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().ptl_renderer_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def stage_slice(self, frame: Frame, index: int) -> None:
        """Everything a draw of `frame` does short of launching; the uniform block it arrives at becomes slice `index` (FLAG_SLICES renderers)."""
        _check(lib().ptl_renderer_stage_slice(self._h, C.byref(frame), index), "ptl_renderer_stage_slice")

    def draw_slices(self, frame: Frame, n: int, out_rgba8: int = 0, out_rgba32f: int = 0, slice_pixels: int = 0, stream: int = 0, timed: bool = False):
        """ONE launch for the staged slices 0 .. n-1: slice z at out_rgba8 + 4 * z * slice_pixels bytes (device addresses)."""
        ms = C.c_float()
        _check(lib().ptl_renderer_draw_slices(self._h, C.byref(frame), n, C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None), slice_pixels,
                                              C.c_void_p(stream or None), C.byref(ms) if timed else None), "ptl_renderer_draw_slices")
        return ms.value if timed else None

    def draw_slices_adaptive(self, frame: Frame, n: int, out_rgba8: int, out_rgba32f: int = 0, slice_pixels: int = 0, stream: int = 0, timed: bool = False):
        """ptl_renderer_draw_slices_adaptive (FLAG_REFINE_SLICES renderers): the staged slices 0 .. n-1 with adaptive anti-aliasing, slice z at
        out_rgba8 + 4 * z * slice_pixels bytes (device addresses; ``slice_pixels`` 0 = width * height).  The threshold is the option
        ``adaptive_aa_threshold``.  Returns the summed GPU time of the launches in ms when ``timed`` (waits), else None."""
        ms = C.c_float()
        _check(lib().ptl_renderer_draw_slices_adaptive(self._h, C.byref(frame), n, C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None),
                                                       slice_pixels or frame.width * frame.height, C.c_void_p(stream or None), C.byref(ms) if timed else None),
               "ptl_renderer_draw_slices_adaptive")
        return ms.value if timed else None

    def adaptive_slices_result(self):
        """Device addresses and stride (lists, list_stride in entries, counts) of the last draw_slices_adaptive: owned by the renderer."""
        lst, cnt, stride = C.c_void_p(), C.c_void_p(), C.c_ulonglong()
        _check(lib().ptl_renderer_adaptive_slices_result(self._h, C.byref(lst), C.byref(stride), C.byref(cnt)), "ptl_renderer_adaptive_slices_result")
        return int(lst.value), int(stride.value), int(cnt.value)

    def set_staged_uniform(self, index: int, name: str, value: int) -> int:
        """ptl_kernel_set_staged_uniform on the renderer's current kernel (layer 1): one Int uniform inside the already staged slice `index`.
        Returns the C code (0, or 1 = the kernel has no such uniform)."""
        v = C.c_int(int(value))
        rc = lib().ptl_kernel_set_staged_uniform(lib().ptl_renderer_kernel(self._h), index, name.encode(), PTL_I32, C.byref(v))
        if rc < 0:
            _check(rc, "ptl_kernel_set_staged_uniform")
        return rc

    def refine_slices_device(self, frame: Frame, n: int, lists_ptr: int, list_stride: int, counts_ptr: int, out_rgba8: int = 0, out_rgba32f: int = 0,
                             slice_pixels: int = 0, segments: int = 0, stream: int = 0, timed: bool = False):
        """ptl_kernel_render_slices_refine on the renderer's current kernel (layer 1; FLAG_REFINE_SLICES renderers): slice z of the kernel's
        staged slices shades the ``counts_ptr[z]`` pixels of the caller's list at ``lists_ptr + 4 * z * list_stride`` into
        ``out_* + z * slice_pixels`` pixels.  All pointers are DEVICE addresses; either output may be 0."""
        ms = C.c_float()
        _check(lib().ptl_kernel_render_slices_refine(lib().ptl_renderer_kernel(self._h), C.byref(frame), n, C.c_void_p(lists_ptr or None), list_stride,
                                                     C.c_void_p(counts_ptr or None), C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None),
                                                     slice_pixels or frame.width * frame.height, C.c_void_p(segments or None), C.c_void_p(stream or None),
                                                     C.byref(ms) if timed else None), "ptl_kernel_render_slices_refine")
        return ms.value if timed else None

    def join(self, stream: int = 0) -> None:
        """With ``set_option("concurrent_draws", K)``: put `stream` (0 = the default stream) behind every draw issued so far."""
        _check(lib().ptl_renderer_join(self._h, C.c_void_p(stream or None)), "ptl_renderer_join")

    def kernel_source(self) -> str:
        """The translation unit the current kernel was compiled from (mode switches compiled in where the build is specialised)."""
        p = C.c_void_p()
        _check(lib().ptl_renderer_kernel_source(self._h, C.byref(p)), "kernel_source")
        try:
            return C.string_at(p).decode("utf-8")
        finally:
            lib().ptl_free(p)

    def set_option(self, name: str, value: float) -> None:
        rc = lib().ptl_renderer_set_option(self._h, name.encode(), float(value))
        if rc != 0:
            raise PortalError(f"unknown renderer option `{name}`")

    def set_camera(self, look_at, alpha: float, beta: float, r: float) -> None:
        la = (C.c_double * 3)(*look_at)
        _check(lib().ptl_renderer_set_camera(self._h, la, alpha, beta, r), "set_camera")

    def use_camera(self, name: str) -> None:
        """`render-frame --camera NAME`; "" restores the scene's own `cam` block."""
        if _check(lib().ptl_renderer_use_camera(self._h, name.encode("utf-8")), "use_camera") != 0:
            raise PortalError(f"Scene has no camera named `{name}`")

    def uniform_value(self, name: str, width: int, height: int):
        out, n = (C.c_float * 16)(), C.c_int()
        rc = lib().ptl_renderer_uniform_value(self._h, width, height, name.encode(), out, C.byref(n))
        _check(rc, "uniform_value")
        if rc != 0:
            return None
        a = np.array(out[: n.value], dtype=np.float32)
        return a.reshape(4, 4).T.copy() if n.value == 16 else (a[0] if n.value == 1 else a)

    def teleport_external_ray(self, a, b):
        """SceneRenderer::teleport_external_ray (src/main.rs:1361-1409) -> (pos | None, encounter_object, change_subspace)."""
        pa_, pb_, out = (C.c_double * 3)(*a), (C.c_double * 3)(*b), (C.c_double * 3)()
        hit, sub, tel = C.c_int(), C.c_int(), C.c_int()
        _check(lib().ptl_renderer_teleport_ray(self._h, pa_, pb_, out, C.byref(hit), C.byref(sub), C.byref(tel)), "teleport_external_ray")
        return (tuple(out) if tel.value else None), bool(hit.value), bool(sub.value)

    def prebuild_teleport(self) -> None:
        """Compile (or load from the cache) the camera-teleport half of the current kernel now instead of at the first query."""
        _check(lib().ptl_renderer_prebuild_teleport(self._h), "prebuild_teleport")

    def resources(self) -> dict:
        """Per-lane registers / scratch bytes / LDS bytes of the loaded kernel."""
        regs, scratch, lds = C.c_int(), C.c_int(), C.c_int()
        _check(lib().ptl_kernel_resources(lib().ptl_renderer_kernel(self._h), C.byref(regs), C.byref(scratch), C.byref(lds)), "kernel_resources")
        return {"registers": regs.value, "scratch_bytes": scratch.value, "lds_bytes": lds.value}

    def move_camera(self, look_at, alpha: float, beta: float, r: float):
        """One interactive camera step incl. SceneRenderer::teleport_camera.  -> (teleported, blocked)"""
        la, tel, blk = (C.c_double * 3)(*look_at), C.c_int(), C.c_int()
        _check(lib().ptl_renderer_move_camera(self._h, la, alpha, beta, r, C.byref(tel), C.byref(blk)), "move_camera")
        return bool(tel.value), bool(blk.value)

    def update(self, seconds: float):
        """SceneRenderer::update: the per-frame step of the video pipeline.  -> (teleported, blocked)"""
        tel, blk = C.c_int(), C.c_int()
        _check(lib().ptl_renderer_update(self._h, float(seconds), C.byref(tel), C.byref(blk)), "update")
        return bool(tel.value), bool(blk.value)

    def rejit_count(self) -> int:
        return lib().ptl_renderer_rejit_count(self._h)

    def affine_rays(self) -> bool:
        """The current kernel spells o.w = 1 / d.w = 0 in its matrix-times-ray products (every scene matrix and the camera affine)."""
        lib().ptl_renderer_kernel(self._h)  # (the kernel the next draw would use)
        return lib().ptl_renderer_affine_rays(self._h) == 1

    def check_affine(self, width: int = 64, height: int = 36) -> int:
        """The dynamic belt behind the snippet scan: draws the current state with the checking build (FLAG_CHECK_AFFINE) and returns how many ray
        halves met a place where an affine-rays kernel assumes a w with another one; above zero the renderer switches affine rays off and rebuilds."""
        n = C.c_ulonglong(0)
        _check(lib().ptl_renderer_check_affine(self._h, width, height, C.byref(n)), "ptl_renderer_check_affine")
        return int(n.value)

    def rejit_pending(self) -> bool:
        """FLAG_ASYNC_REJIT: a specialised build is being compiled in the background / the un-specialised kernel is in use."""
        return lib().ptl_renderer_rejit_pending(self._h) == 1

    def camera_state(self) -> dict:
        m, sub, pos = (C.c_double * 16)(), C.c_int(), (C.c_double * 3)()
        _check(lib().ptl_renderer_camera_state(self._h, m, C.byref(sub), pos), "camera_state")
        return {"teleport_matrix": np.array(m, np.float64).reshape(4, 4).T.copy(), "in_subspace": bool(sub.value), "position": np.array(pos)}

    def code_object(self) -> bytes:
        k = lib().ptl_renderer_kernel(self._h)
        data, size = C.c_void_p(), C.c_size_t()
        _check(lib().ptl_kernel_code_object(k, C.byref(data), C.byref(size)), "code_object")
        return C.string_at(data, size.value)

    def code_object_sha256(self) -> str:
        """sha256 of the loaded gfx950 code object: what ties a bench line to the PMC passes of the same binary."""
        import hashlib

        return hashlib.sha256(self.code_object()).hexdigest()

    def code_object_note(self, key: str, kernel_prefix: str = "ptl_render") -> int:
        """Kernel metadata of the loaded code object (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".sgpr_count"):
        the largest value over the kernels whose name starts with ``kernel_prefix`` ("" = all)."""
        code = self.code_object()
        return lib().ptl_code_object_note(code, len(code), key.encode(), kernel_prefix.encode())

    # -- drawing ---------------------------------------------------------------------------
    def draw_device(self, frame: Frame, out_rgba8: int = 0, out_rgba32f: int = 0, segments: int = 0, stream: int = 0, timed: bool = False):
        """draw_texture into DEVICE buffers given as integer addresses (e.g. torch data_ptr()).
        Returns the kernel time in ms when ``timed`` (waits for completion), else None."""
        ms = C.c_float()
        rc = lib().ptl_renderer_draw(self._h, C.byref(frame), C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None),
                                     C.c_void_p(segments or None), C.c_void_p(stream or None), C.byref(ms) if timed else None)
        _check(rc, "draw_texture")
        return ms.value if timed else None

    def draw(self, width: int, height: int, rgba8: bool = True, rgba32f: bool = False, segments: bool = False, rb_phase: int = 0, rb_stride: int = 1):
        """draw_texture + read back to numpy.  Returns dict(rgba8=HxWx4 u8, rgba32f=HxWx4 f32,
        segments=int, ms=float); H = rows of the shard."""
        frame = Frame(width, height, rb_phase, rb_stride)
        rows = shard_rows(frame)
        if rows < 0:
            raise PortalError("bad frame")
        a8 = np.empty((rows, width, 4), np.uint8) if rgba8 else None
        a32 = np.empty((rows, width, 4), np.float32) if rgba32f else None
        seg, ms = C.c_uint64(0), C.c_float()
        rc = lib().ptl_renderer_draw_to_host(self._h, C.byref(frame), a8.ctypes.data if rgba8 else None, a32.ctypes.data if rgba32f else None,
                                             C.byref(seg) if segments else None, C.byref(ms))
        _check(rc, "draw_texture")
        return {"rgba8": a8, "rgba32f": a32, "segments": seg.value if segments else None, "ms": ms.value}

    def draw_passes_device(self, frame: Frame, out_passes: int, passes_bytes: int, out_rgba8: int = 0, out_rgba32f: int = 0, segments: int = 0, stream: int = 0,
                           timed: bool = False):
        """ptl_renderer_draw_passes into DEVICE buffers given as integer addresses (FLAG_PASSES renderers, or option ``passes`` = 1): the draw of
        ``draw_device`` plus a PASS_RECORD per pixel at ``out_passes`` (``passes_bytes`` bytes, 16 per pixel the launch stores, addressed like
        ``out_rgba32f``).  Returns the kernel time in ms when ``timed`` (waits for completion), else None."""
        ms = C.c_float()
        _check(lib().ptl_renderer_draw_passes(self._h, C.byref(frame), C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None), C.c_void_p(out_passes or None),
                                              passes_bytes, C.c_void_p(segments or None), C.c_void_p(stream or None), C.byref(ms) if timed else None),
               "ptl_renderer_draw_passes")
        return ms.value if timed else None

    def draw_slices_passes(self, frame: Frame, n: int, out_passes: int, passes_bytes: int, out_rgba8: int = 0, out_rgba32f: int = 0, slice_pixels: int = 0,
                           stream: int = 0, timed: bool = False):
        """ptl_renderer_draw_slices_passes: ``draw_slices`` plus the records, slice z at ``out_passes + 16 * z * slice_pixels`` bytes."""
        ms = C.c_float()
        _check(lib().ptl_renderer_draw_slices_passes(self._h, C.byref(frame), n, C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None),
                                                     C.c_void_p(out_passes or None), passes_bytes, slice_pixels, C.c_void_p(stream or None),
                                                     C.byref(ms) if timed else None), "ptl_renderer_draw_slices_passes")
        return ms.value if timed else None

    def draw_passes(self, width: int, height: int, rgba8: bool = True, rgba32f: bool = False, segments: bool = False, rb_phase: int = 0, rb_stride: int = 1):
        """A pass draw read back to numpy.  Returns dict(passes=HxW structured array of PASS_RECORD, rgba8=HxWx4 u8 or None, rgba32f=HxWx4 f32
        or None, segments=int or None, ms=float); H = rows of the shard."""
        frame = Frame(width, height, rb_phase, rb_stride)
        rows = shard_rows(frame)
        if rows < 0:
            raise PortalError("bad frame")
        n = rows * width
        bufs = [device_alloc(max(n, 1) * 16, self.device), device_alloc(n * 4, self.device) if rgba8 and n else 0, device_alloc(n * 16, self.device) if rgba32f and n else 0,
                device_alloc(8, self.device) if segments else 0]
        try:
            if segments:
                device_memset(bufs[3], 0, 8)
            ms = self.draw_passes_device(frame, bufs[0], max(n, 1) * 16, bufs[1], bufs[2], bufs[3], timed=True)
            return {"passes": device_download(bufs[0], n * 16).view(PASS_RECORD).reshape(rows, width),
                    "rgba8": device_download(bufs[1], n * 4).reshape(rows, width, 4) if bufs[1] else None,
                    "rgba32f": device_download(bufs[2], n * 16).view(np.float32).reshape(rows, width, 4) if bufs[2] else None,
                    "segments": int(device_download(bufs[3], 8).view(np.uint64)[0]) if segments else None, "ms": ms}
        finally:
            for b in bufs:
                if b:
                    device_free(b)

    def draw_adaptive_device(self, frame: Frame, out_rgba8: int, out_rgba32f: int = 0, stream: int = 0, timed: bool = False):
        """ptl_renderer_draw_adaptive into DEVICE buffers given as integer addresses (FLAG_REFINE renderers; the threshold is the option
        ``adaptive_aa_threshold``).  Returns the summed GPU time of the three launches in ms when ``timed`` (waits), else None."""
        ms = C.c_float()
        _check(lib().ptl_renderer_draw_adaptive(self._h, C.byref(frame), C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None),
                                                C.c_void_p(stream or None), C.byref(ms) if timed else None), "ptl_renderer_draw_adaptive")
        return ms.value if timed else None

    def refine_device(self, frame: Frame, list_ptr: int, count_ptr: int, out_rgba8: int = 0, out_rgba32f: int = 0, segments: int = 0, stream: int = 0,
                      timed: bool = False):
        """ptl_kernel_render_refine on the renderer's current kernel (layer 1; FLAG_REFINE renderers): shades the ``*count_ptr`` pixels of the
        caller's own list with the uniforms the last draw left behind.  All pointers are DEVICE addresses; either output may be 0.
        Returns the kernel time in ms when ``timed`` (waits for completion), else None."""
        ms = C.c_float()
        _check(lib().ptl_kernel_render_refine(lib().ptl_renderer_kernel(self._h), C.byref(frame), C.c_void_p(list_ptr or None), C.c_void_p(count_ptr or None),
                                              C.c_void_p(out_rgba8 or None), C.c_void_p(out_rgba32f or None), C.c_void_p(segments or None),
                                              C.c_void_p(stream or None), C.byref(ms) if timed else None), "ptl_kernel_render_refine")
        return ms.value if timed else None

    def adaptive_result(self):
        """Device addresses (list, count) of the last adaptive draw: owned by the renderer, valid until the next adaptive draw."""
        lst, cnt = C.c_void_p(), C.c_void_p()
        _check(lib().ptl_renderer_adaptive_result(self._h, C.byref(lst), C.byref(cnt)), "ptl_renderer_adaptive_result")
        return int(lst.value), int(cnt.value)

    def adaptive_times(self):
        """GPU times in ms of the last TIMED adaptive draw: (pass 1, classification, refine pass)."""
        ms = (C.c_float * 3)()
        _check(lib().ptl_renderer_adaptive_times(self._h, ms), "ptl_renderer_adaptive_times")
        return tuple(float(v) for v in ms)

    def draw_adaptive(self, width: int, height: int, threshold: int = 4, rgba32f: bool = False):
        """Adaptive anti-aliasing (include/portal_amd.h): one sample per pixel, then the full ``aa_count`` where a pixel differs from a
        neighbour by more than ``threshold`` codes.  Returns dict(rgba8=HxWx4 u8, rgba32f=HxWx4 f32 or None, count=int,
        list=the refined pixel indices y*W+x (uint32, in the order the GPU produced them), ms=float, ms_passes=(pass 1, classify, refine))."""
        self.set_option("adaptive_aa_threshold", threshold)
        frame = Frame(width, height, 0, 1)
        n = width * height
        d8 = device_alloc(n * 4, self.device)
        d32 = device_alloc(n * 16, self.device) if rgba32f else 0
        try:
            ms = self.draw_adaptive_device(frame, d8, d32, timed=True)
            a8 = device_download(d8, n * 4).reshape(height, width, 4)
            a32 = device_download(d32, n * 16).view(np.float32).reshape(height, width, 4) if rgba32f else None
            lst, cnt = self.adaptive_result()
            count = int(device_download(cnt, 4).view(np.uint32)[0])
            entries = device_download(lst, count * 4).view(np.uint32) if count else np.empty(0, np.uint32)
        finally:
            device_free(d8)
            if d32:
                device_free(d32)
        return {"rgba8": a8, "rgba32f": a32, "count": count, "list": entries, "ms": ms, "ms_passes": self.adaptive_times()}


GROUP_PEER_STORES, GROUP_COPY_GATHER, GROUP_RCCL_GATHER = 0, 1, 2


class FrameGroup:
    """Layer 3: one frame across several GPUs from one process (include/portal_amd.h, csrc/host/multigpu.cpp).
    `devices` may name a device more than once (rehearsal of the N-rank control flow on one GPU)."""

    def __init__(self, scene: Scene, devices, asset_root: Optional[str] = None, flags: int = 0, transport: int = GROUP_PEER_STORES):
        self.scene = scene
        self.devices = list(devices)
        h = C.c_void_p()
        log = C.create_string_buffer(1 << 16)
        arr = (C.c_int * len(self.devices))(*self.devices)
        rc = lib().ptl_frame_group_create(scene._h, arr, len(self.devices), (asset_root or REPO_ROOT).encode(), flags, transport, C.byref(h), log, len(log))
        if rc != 0:
            raise PortalError(f"ptl_frame_group_create failed ({rc}): {_err()}\n{log.value.decode(errors='replace')}")
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().ptl_frame_group_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_option(self, name: str, value: float) -> None:
        _check(lib().ptl_frame_group_set_option(self._h, name.encode(), float(value)), "ptl_frame_group_set_option")

    def set_camera(self, look_at, alpha: float, beta: float, r: float) -> None:
        la = (C.c_double * 3)(*look_at)
        _check(lib().ptl_frame_group_set_camera(self._h, la, alpha, beta, r), "ptl_frame_group_set_camera")

    def update(self, seconds: float) -> None:
        _check(lib().ptl_frame_group_update(self._h, float(seconds)), "ptl_frame_group_update")

    def submit(self, width: int, height: int) -> int:
        """Enqueue one frame (trace on every rank + its transfer to devices[0]) without waiting; returns the ticket for `wait`.
        Two frames may be in flight: the transfer of frame n overlaps the trace of frame n + 1."""
        ticket = C.c_int(-1)
        _check(lib().ptl_frame_group_submit(self._h, width, height, C.byref(ticket)), "ptl_frame_group_submit")
        self._size = (width, height)  # (one size for everything in flight: another one is refused while a frame is on its way)
        return ticket.value

    def wait(self, ticket: int) -> dict:
        """The frame of `ticket`, assembled: dict(rgba8, kernel_ms per rank, device_ptr)."""
        ptr = C.c_void_p()
        ms = (C.c_float * len(self.devices))()
        _check(lib().ptl_frame_group_wait(self._h, ticket, C.byref(ptr), ms), "ptl_frame_group_wait")
        width, height = self._size
        img = np.empty((height, width, 4), np.uint8)
        _check(lib().ptl_frame_group_download(self._h, img.ctypes.data_as(C.c_void_p)), "ptl_frame_group_download")
        return {"rgba8": img, "kernel_ms": [float(x) for x in ms], "device_ptr": ptr.value}

    def draw(self, width: int, height: int) -> dict:
        """Returns dict(rgba8 (H, W, 4) uint8, kernel_ms per rank, device_ptr of the frame on devices[0])."""
        ptr = C.c_void_p()
        ms = (C.c_float * len(self.devices))()
        _check(lib().ptl_frame_group_draw(self._h, width, height, C.byref(ptr), ms), "ptl_frame_group_draw")
        img = np.empty((height, width, 4), np.uint8)
        _check(lib().ptl_frame_group_download(self._h, img.ctypes.data_as(C.c_void_p)), "ptl_frame_group_download")
        return {"rgba8": img, "kernel_ms": [float(x) for x in ms], "device_ptr": ptr.value}


class Kernel:
    """Layer 1 of the C ABI (ptl_kernel_*): a hand-written or generated HIP source compiled with
    hiprtc -- the drop-in replacement for macroquad's load_material / set_uniform / set_texture /
    draw (reference src/gui/scene.rs:1132-1143, src/main.rs:1077-1078,1269-1358,1424-1425)."""

    def __init__(self, source: str, uniforms, block_size: int, device: int = 0, defines=()):
        self._keep = [n.encode() for n, _, _ in uniforms]
        descs = (UniformDesc * len(uniforms))(*[UniformDesc(self._keep[i], t, o) for i, (_, t, o) in enumerate(uniforms)])
        defs = (C.c_char_p * len(defines))(*[d.encode() for d in defines])
        h, log = C.c_void_p(), C.create_string_buffer(1 << 16)
        rc = lib().ptl_kernel_compile(device, source.encode("utf-8"), descs, len(uniforms), block_size, defs, len(defines), C.byref(h), log, len(log))
        self.compile_log = log.value.decode("utf-8", "replace")
        if rc != 0:
            raise PortalError(f"ptl_kernel_compile failed ({rc}): {_err()}\n{self.compile_log}")
        self._h = h

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().ptl_kernel_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_uniform(self, name: str, typ: int, value) -> int:
        if typ == PTL_I32:
            buf = np.array([value], np.int32)
        elif typ == PTL_MAT4:
            buf = np.ascontiguousarray(np.asarray(value, np.float32).T).reshape(16)  # m[row, col] -> column-major
        else:
            buf = np.atleast_1d(np.asarray(value, np.float32))
        return _check(lib().ptl_kernel_set_uniform(self._h, name.encode(), typ, buf.ctypes.data), "set_uniform")

    def set_texture(self, sampler: str, rgba8: np.ndarray) -> int:
        a = np.ascontiguousarray(rgba8, np.uint8)
        return _check(lib().ptl_kernel_set_texture(self._h, sampler.encode(), a.ctypes.data, a.shape[1], a.shape[0]), "set_texture")

    def render(self, width: int, height: int, rgba8: bool = True, rgba32f: bool = False, rb_phase: int = 0, rb_stride: int = 1):
        frame = Frame(width, height, rb_phase, rb_stride)
        rows = shard_rows(frame)
        a8 = np.empty((rows, width, 4), np.uint8) if rgba8 else None
        a32 = np.empty((rows, width, 4), np.float32) if rgba32f else None
        ms = C.c_float()
        rc = lib().ptl_kernel_render_to_host(self._h, C.byref(frame), a8.ctypes.data if rgba8 else None, a32.ctypes.data if rgba32f else None, None, C.byref(ms))
        _check(rc, "ptl_kernel_render_to_host")
        return {"rgba8": a8, "rgba32f": a32, "ms": ms.value}


def device_source(which: str) -> str:
    p = lib().ptl_device_source(which.encode())
    if p is None:
        raise PortalError(f"no device source `{which}`")
    return p.decode("utf-8")


def select_sections(text: str, names=()) -> str:
    """The conditional sections of a template (``//%if NAME``, ``//%else``, ``//%end``) resolved for ``names``; PortalError where the engine refuses the text."""
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    p = lib().ptl_select_sections(text.encode("utf-8"), arr, len(names))
    if not p:
        raise PortalError(_err())
    try:
        return C.string_at(p).decode("utf-8")
    finally:
        lib().ptl_free(p)


def deinterleave_rows(shard: np.ndarray, frame: Frame, full: np.ndarray) -> None:
    _check(lib().ptl_deinterleave_rows(shard.ctypes.data, C.byref(frame), full.ctypes.data), "deinterleave_rows")


def average_images_device(frame_ptrs, out_ptr: int, width: int, height: int, device: int = 0, stream: int = 0, timed: bool = False):
    """average_images (src/main.rs:645-722) on DEVICE buffers given as integer addresses."""
    arr = (C.c_void_p * len(frame_ptrs))(*frame_ptrs)
    ms = C.c_float()
    _check(lib().ptl_average_images(device, arr, len(frame_ptrs), C.c_void_p(out_ptr), width, height, C.c_void_p(stream or None), C.byref(ms) if timed else None),
           "average_images")
    return ms.value if timed else None


def average_to_yuv420p10_device(frame_ptrs, out_ptr: int, width: int, height: int, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_average_to_yuv420p10 on DEVICE buffers given as integer addresses: the sub-frames averaged like `average_images_device` and
    converted to one planar Y'CbCr 4:2:0 10-bit frame (`yuv420p10_frame_bytes` bytes at out_ptr) by the same kernel."""
    arr = (C.c_void_p * len(frame_ptrs))(*frame_ptrs)
    ms = C.c_float()
    _check(lib().ptl_average_to_yuv420p10(device, arr, len(frame_ptrs), C.c_void_p(out_ptr), width, height, C.c_void_p(stream or None), C.byref(ms) if timed else None),
           "average_to_yuv420p10")
    return ms.value if timed else None


def average_f32_to_yuv420p10_device(frame_ptrs, out_ptr: int, width: int, height: int, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_average_f32_to_yuv420p10 on DEVICE buffers given as integer addresses: the deep-colour form of `average_to_yuv420p10_device`.
    The sub-frames are RGBA32F (what a draw writes as `rgba32f`, 16 bytes per pixel); they are quantised once, to 16 bits, before the
    10-bit frame (`yuv420p10_frame_bytes` bytes at out_ptr, the same layout)."""
    arr = (C.c_void_p * len(frame_ptrs))(*frame_ptrs)
    ms = C.c_float()
    _check(lib().ptl_average_f32_to_yuv420p10(device, arr, len(frame_ptrs), C.c_void_p(out_ptr), width, height, C.c_void_p(stream or None), C.byref(ms) if timed else None),
           "average_f32_to_yuv420p10")
    return ms.value if timed else None


def aa_edges_slices_device(frames_ptr: int, slice_pixels: int, n: int, width: int, height: int, threshold: int, lists_ptr: int, list_stride: int, counts_ptr: int,
                           device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_aa_edges_slices on DEVICE buffers given as integer addresses: aa_edges_device over a stack of ``n`` frames in one launch, slice z
    reading ``frames_ptr + 4 * z * slice_pixels``, listing at ``lists_ptr + 4 * z * list_stride`` and counting in ``counts_ptr[z]``."""
    ms = C.c_float()
    _check(lib().ptl_aa_edges_slices(device, C.c_void_p(frames_ptr or None), slice_pixels, n, width, height, threshold, C.c_void_p(lists_ptr or None), list_stride,
                                     C.c_void_p(counts_ptr or None), C.c_void_p(stream or None), C.byref(ms) if timed else None), "aa_edges_slices")
    return ms.value if timed else None


def aa_edges_device(frame_ptr: int, width: int, height: int, threshold: int, list_ptr: int, count_ptr: int, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_aa_edges on DEVICE buffers given as integer addresses: the pixels of the RGBA8 frame that differ from one of their eight
    neighbours by more than `threshold` codes in R, G or B -> their indices y*W+x at list_ptr (room for W*H uint32) and their number
    at count_ptr (one uint32, reset by the call)."""
    ms = C.c_float()
    _check(lib().ptl_aa_edges(device, C.c_void_p(frame_ptr or None), width, height, threshold, C.c_void_p(list_ptr or None), C.c_void_p(count_ptr or None),
                              C.c_void_p(stream or None), C.byref(ms) if timed else None), "aa_edges")
    return ms.value if timed else None


def yuv420p10_frame_bytes(width: int, height: int) -> int:
    """Bytes of one frame as `average_to_yuv420p10_device` writes it = the payload of one Y4M frame."""
    return int(lib().ptl_yuv420p10_frame_bytes(width, height))


def _average_to_yuv10(entry, frame_ptrs, out_ptr, width, height, chroma, device, stream, timed):
    arr = (C.c_void_p * len(frame_ptrs))(*frame_ptrs)
    ms = C.c_float()
    _check(getattr(lib(), "ptl_" + entry)(device, arr, len(frame_ptrs), C.c_void_p(out_ptr), width, height, chroma, C.c_void_p(stream or None),
                                          C.byref(ms) if timed else None), entry)
    return ms.value if timed else None


def average_to_yuv10_device(frame_ptrs, out_ptr: int, width: int, height: int, chroma: int, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_average_to_yuv10 on DEVICE buffers given as integer addresses: `average_to_yuv420p10_device` with the chroma sampling chosen,
    `chroma` = 420, 422 or 444 (`yuv10_frame_bytes(width, height, chroma)` bytes at out_ptr).  420 is the same kernel, the same bytes."""
    return _average_to_yuv10("average_to_yuv10", frame_ptrs, out_ptr, width, height, chroma, device, stream, timed)


def average_f32_to_yuv10_device(frame_ptrs, out_ptr: int, width: int, height: int, chroma: int, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_average_f32_to_yuv10: the deep-colour form (RGBA32F sub-frames, see `average_f32_to_yuv420p10_device`) with the sampling chosen."""
    return _average_to_yuv10("average_f32_to_yuv10", frame_ptrs, out_ptr, width, height, chroma, device, stream, timed)


def yuv10_frame_bytes(width: int, height: int, chroma: int) -> int:
    """Bytes of one frame as `average_to_yuv10_device` writes it at that sampling; 0 for a sampling that is none of 420, 422, 444."""
    return int(lib().ptl_yuv10_frame_bytes(width, height, chroma))


PNG_FILTER_NONE, PNG_FILTER_SUB = 0, 1


def average_f32_to_rgb48_device(frame_ptrs, out_ptr: int, width: int, height: int, filter: int = PNG_FILTER_SUB, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_average_f32_to_rgb48 on DEVICE buffers given as integer addresses: the averaged frame of the RGBA32F sub-frames (that of
    `average_f32_to_yuv420p10_device`) as the scanlines of a 16-bit RGB PNG, `rgb48_frame_bytes(width, height)` bytes at out_ptr: big-endian
    samples, unfiltered (`PNG_FILTER_NONE`) or with PNG's Sub filter applied (`PNG_FILTER_SUB`), no filter-type bytes."""
    return _average_to_yuv10("average_f32_to_rgb48", frame_ptrs, out_ptr, width, height, filter, device, stream, timed)


def rgb48_frame_bytes(width: int, height: int) -> int:
    """Bytes of one frame as `average_f32_to_rgb48_device` writes it: 6 per pixel."""
    return int(lib().ptl_rgb48_frame_bytes(width, height))


def png_write_rgb48(path: str, rows, width: int, height: int, filter: int = PNG_FILTER_SUB, level: int = 6) -> None:
    """ptl_png_write_rgb48: a 16-bit RGB PNG from HOST rows (bytes or a uint8 array of 6 * width * height) exactly as
    `average_f32_to_rgb48_device` wrote them with the same `filter`; deflate `level` 0 .. 9."""
    a = np.ascontiguousarray(np.frombuffer(rows, dtype=np.uint8) if isinstance(rows, (bytes, bytearray, memoryview)) else rows, dtype=np.uint8)
    if width > 0 and height > 0 and a.size != 6 * width * height:
        raise PortalError(f"png_write_rgb48: {a.size} bytes are not {width} x {height} pixels of 6 bytes")
    _check(lib().ptl_png_write_rgb48(path.encode(), a.ctypes.data, width, height, filter, level), "png_write_rgb48")


PNG_STREAM_HEADER_BYTES = 64


def png_stream_bytes(width: int, height: int) -> int:
    """Bytes of the result buffer of `png_deflate_rgba8_device`: header, room for the longest stream, and the kernels' scratch behind it;
    0 for a size that is not positive or whose scanlines exceed 2^31 bytes."""
    return int(lib().ptl_png_stream_bytes(width, height))


def png_stream_download_bytes(width: int, height: int) -> int:
    """The part of the result buffer a host needs: the header and the room for the longest stream, without the kernels' scratch behind them."""
    return int(lib().ptl_png_stream_download_bytes(width, height))


def png_stream_band_rows(width: int) -> int:
    """Rows of the frame per band of the stream (each band is a deflate block of its own)."""
    return int(lib().ptl_png_stream_band_rows(width))


PNG_CODES_FIXED, PNG_CODES_DYNAMIC = 0, 1


def png_deflate_rgba8_device(frame_ptr: int, out_ptr: int, width: int, height: int, device: int = 0, stream: int = 0, timed: bool = False, codes: int = PNG_CODES_FIXED):
    """ptl_png_deflate_rgba8 on DEVICE buffers given as integer addresses: the RGBA8 frame at frame_ptr -> at out_ptr
    (`png_stream_bytes(width, height)` bytes) a 64-byte header and the deflate stream of the frame's Up-filtered scanlines (runs only; fixed
    Huffman codes, or with ``codes=PNG_CODES_DYNAMIC`` a code per band through ptl_png_deflate_rgba8_codes; the contracts are in
    include/portal_amd.h).  Returns the time of both kernels in ms when ``timed`` (waits), else None."""
    ms = C.c_float()
    if codes == PNG_CODES_FIXED:
        _check(lib().ptl_png_deflate_rgba8(device, C.c_void_p(frame_ptr or None), width, height, C.c_void_p(out_ptr or None), C.c_void_p(stream or None),
                                           C.byref(ms) if timed else None), "png_deflate_rgba8")
    else:
        _check(lib().ptl_png_deflate_rgba8_codes(device, C.c_void_p(frame_ptr or None), width, height, int(codes), C.c_void_p(out_ptr or None), C.c_void_p(stream or None),
                                                 C.byref(ms) if timed else None), "png_deflate_rgba8_codes")
    return ms.value if timed else None


def png_write_stream(path: str, result, width: int, height: int) -> None:
    """ptl_png_write_stream: an 8-bit RGBA PNG from a HOST copy of the result buffer (bytes or a uint8 array: the header and the stream it
    announces, at least); the host adds the chunk framing and CRCs, nothing else."""
    a = np.ascontiguousarray(np.frombuffer(result, dtype=np.uint8) if isinstance(result, (bytes, bytearray, memoryview)) else result, dtype=np.uint8)
    if a.size < PNG_STREAM_HEADER_BYTES or a.size < PNG_STREAM_HEADER_BYTES + int(a[12:16].view("<u4")[0]):
        raise PortalError("png_write_stream: the buffer is shorter than its header and the stream the header announces")
    _check(lib().ptl_png_write_stream(path.encode(), a.ctypes.data, width, height), "png_write_stream")


def png_stream16_bytes(width: int, height: int) -> int:
    """Bytes of the result buffer of `png_deflate_rgb48_device`: header, room for the longest stream, and the kernels' scratch behind it; 0 for
    a size that is not positive, has more than 2^28 pixels or whose scanlines exceed 2^31 bytes."""
    return int(lib().ptl_png_stream16_bytes(width, height))


def png_stream16_download_bytes(width: int, height: int) -> int:
    """The part of that result buffer a host needs: the header and the room for the longest stream."""
    return int(lib().ptl_png_stream16_download_bytes(width, height))


def png_stream16_band_rows(width: int) -> int:
    """Rows of the 16-bit frame per band of the stream."""
    return int(lib().ptl_png_stream16_band_rows(width))


def png_deflate_rgb48_device(rows_ptr: int, out_ptr: int, width: int, height: int, device: int = 0, stream: int = 0, timed: bool = False, codes: int = PNG_CODES_DYNAMIC):
    """ptl_png_deflate_rgb48 on DEVICE buffers given as integer addresses: the unfiltered rows of `average_f32_to_rgb48_device`
    (PNG_FILTER_NONE) at rows_ptr -> at out_ptr (`png_stream16_bytes(width, height)` bytes) a 64-byte header ("PTL6") and the deflate stream
    of the rows' Up-filtered scanlines: literals and matches at distance 6, a Huffman code per band, or with ``codes=PNG_CODES_FIXED`` the
    fixed block in every band (the contract is in include/portal_amd.h).  Returns the time of both kernels in ms when ``timed`` (waits),
    else None."""
    ms = C.c_float()
    _check(lib().ptl_png_deflate_rgb48(device, C.c_void_p(rows_ptr or None), width, height, int(codes), C.c_void_p(out_ptr or None), C.c_void_p(stream or None),
                                       C.byref(ms) if timed else None), "png_deflate_rgb48")
    return ms.value if timed else None


def png_write_stream_rgb48(path: str, result, width: int, height: int) -> None:
    """ptl_png_write_stream_rgb48: a 16-bit RGB PNG from a HOST copy of the result buffer of `png_deflate_rgb48_device` (bytes or a uint8
    array: the header and the stream it announces, at least); the host adds the chunk framing and CRCs, nothing else."""
    a = np.ascontiguousarray(np.frombuffer(result, dtype=np.uint8) if isinstance(result, (bytes, bytearray, memoryview)) else result, dtype=np.uint8)
    if a.size < PNG_STREAM_HEADER_BYTES or a.size < PNG_STREAM_HEADER_BYTES + int(a[12:16].view("<u4")[0]):
        raise PortalError("png_write_stream_rgb48: the buffer is shorter than its header and the stream the header announces")
    _check(lib().ptl_png_write_stream_rgb48(path.encode(), a.ctypes.data, width, height), "png_write_stream_rgb48")


def png_write_stream_gray16(path: str, result, width: int, height: int) -> None:
    """ptl_png_write_stream_gray16: a 16-bit grey PNG of ``width`` samples per row (a multiple of 3) from a HOST copy of the result buffer of
    `png_deflate_rgb48_device` over the same rows taken as width / 3 RGB pixels."""
    a = np.ascontiguousarray(np.frombuffer(result, dtype=np.uint8) if isinstance(result, (bytes, bytearray, memoryview)) else result, dtype=np.uint8)
    if a.size < PNG_STREAM_HEADER_BYTES or a.size < PNG_STREAM_HEADER_BYTES + int(a[12:16].view("<u4")[0]):
        raise PortalError("png_write_stream_gray16: the buffer is shorter than its header and the stream the header announces")
    _check(lib().ptl_png_write_stream_gray16(path.encode(), a.ctypes.data, width, height), "png_write_stream_gray16")


# ---- trace passes (include/portal_amd.h: ptl_pass_record, ptl_pass_stats_block) ------------------------------------------------------
PASS_RECORD = np.dtype([("depth_near", "<f4"), ("trips", "<u4"), ("final_escaped", "<u4"), ("exhausted_outside", "<u4")])
PASS_HIST_BINS = 256
PASS_STATS_BLOCK = np.dtype([("pixels", "<u8"), ("paths", "<u8"), ("trips", "<u8"), ("final_paths", "<u8"), ("escaped", "<u8"), ("exhausted", "<u8"), ("outside", "<u8"),
                             ("exhausted_pixels", "<u8"), ("max_trips", "<u4"), ("depth_max_key", "<u4"), ("depth_min_key_inv", "<u4"), ("reserved", "<u4"),
                             ("trips_histogram", "<u8", (PASS_HIST_BINS,))])
PASS_DEPTH, PASS_TRIPS = 0, 1


def pass_counts(records: np.ndarray) -> dict:
    """The four path counts of PASS_RECORD records, unpacked: dict(final, escaped, exhausted, outside) of uint32 arrays."""
    fe, xo = records["final_escaped"], records["exhausted_outside"]
    return {"final": fe & 0xFFFF, "escaped": fe >> 16, "exhausted": xo & 0xFFFF, "outside": xo >> 16}


def pass_record_bytes(width: int, height: int) -> int:
    return int(lib().ptl_pass_record_bytes(width, height))


def pass_stats_device(records_ptr: int, n: int, block_ptr: int, per_launch_ptr: int = 0, slot: int = 0, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_pass_stats: n records (DEVICE address) added into a PASS_STATS_BLOCK in device memory the caller zeroed; ``per_launch_ptr[slot]``
    (uint64 counters, or 0) receives this sweep's exhausted paths.  Returns the kernel time in ms when ``timed`` (waits), else None."""
    ms = C.c_float()
    _check(lib().ptl_pass_stats(device, C.c_void_p(records_ptr or None), n, C.c_void_p(block_ptr or None), C.c_void_p(per_launch_ptr or None), slot,
                                C.c_void_p(stream or None), C.byref(ms) if timed else None), "ptl_pass_stats")
    return ms.value if timed else None


def pass_stats_depth_range(block: np.ndarray):
    """(lo, hi) of the finite depth_near values a downloaded PASS_STATS_BLOCK has seen, or None."""
    b = np.ascontiguousarray(block).view(PASS_STATS_BLOCK).reshape(-1)[:1]
    lo, hi = C.c_float(), C.c_float()
    return (lo.value, hi.value) if lib().ptl_pass_stats_depth_range(b.ctypes.data, C.byref(lo), C.byref(hi)) == 1 else None


def passes_to_gray16_device(records_ptr: int, n: int, out_ptr: int, which: int, lo: float = 0.0, hi: float = 1.0, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_passes_to_gray16: n records -> 2 n bytes, the big-endian samples of a 16-bit greyscale PNG (``which``: PASS_DEPTH or PASS_TRIPS)."""
    ms = C.c_float()
    _check(lib().ptl_passes_to_gray16(device, C.c_void_p(records_ptr or None), n, C.c_void_p(out_ptr or None), which, lo, hi, C.c_void_p(stream or None),
                                      C.byref(ms) if timed else None), "ptl_passes_to_gray16")
    return ms.value if timed else None


def pass_slices_to_gray16_device(records_ptr: int, n_slices: int, slice_records: int, n: int, out_depth_ptr: int = 0, out_trips_ptr: int = 0, out_cut_ptr: int = 0,
                                 lo: float = 0.0, hi: float = 1.0, device: int = 0, stream: int = 0, timed: bool = False):
    """ptl_pass_slices_to_gray16: the records of ``n_slices`` sub-frames (slice z of pixel p at index z * slice_records + p) merged per pixel
    into up to three images of 2 n bytes each -- nearest final depth, summed trips, share of cut paths -- in one sweep; an output of 0 is not made."""
    ms = C.c_float()
    _check(lib().ptl_pass_slices_to_gray16(device, C.c_void_p(records_ptr or None), n_slices, slice_records, n, C.c_void_p(out_depth_ptr or None),
                                           C.c_void_p(out_trips_ptr or None), C.c_void_p(out_cut_ptr or None), lo, hi, C.c_void_p(stream or None),
                                           C.byref(ms) if timed else None), "ptl_pass_slices_to_gray16")
    return ms.value if timed else None


def png_write_gray16(path: str, rows, width: int, height: int, level: int = 6) -> None:
    """ptl_png_write_gray16: ``rows`` = height * width big-endian 16-bit samples (bytes or a uint8 array), colour type 0, bit depth 16."""
    a = np.ascontiguousarray(np.frombuffer(rows, np.uint8) if isinstance(rows, (bytes, bytearray)) else rows, dtype=np.uint8)
    if a.size != 2 * width * height:
        raise PortalError("png_write_gray16: rows must hold 2 * width * height bytes")
    _check(lib().ptl_png_write_gray16(path.encode(), a.ctypes.data, width, height, level), "ptl_png_write_gray16")


def y4m_header(width: int, height: int, fps: int, chroma: int = 420) -> bytes:
    """The header line of the Y4M stream those frames travel in (each frame: b"FRAME\\n" + payload)."""
    buf = C.create_string_buffer(128)
    n = _check(lib().ptl_y4m_header_chroma(width, height, fps, chroma, buf, len(buf)), "y4m_header")
    return buf.raw[:n]


def device_alloc(nbytes: int, device: int = 0) -> int:
    """A whole device allocation (hipMalloc), as an integer address.  What `ipc_export` needs."""
    p = C.c_void_p()
    _check(lib().ptl_device_alloc(device, nbytes, C.byref(p)), "device_alloc")
    return int(p.value)


def device_free(ptr: int) -> None:
    _check(lib().ptl_device_free(C.c_void_p(ptr)), "device_free")


def device_download(ptr: int, nbytes: int, stream: int = 0) -> np.ndarray:
    out = np.empty(nbytes, dtype=np.uint8)
    _check(lib().ptl_device_download(out.ctypes.data, C.c_void_p(ptr), nbytes, C.c_void_p(stream or None)), "device_download")
    return out


def device_memset(ptr: int, value: int, nbytes: int, stream: int = 0) -> None:
    _check(lib().ptl_device_memset(C.c_void_p(ptr), value, nbytes, C.c_void_p(stream or None)), "device_memset")


def device_copy2d_async(dst: int, dst_pitch: int, src: int, src_pitch: int, width_bytes: int, rows: int, stream: int = 0) -> None:
    """Strided device-to-device copy on `stream` (hipMemcpy2DAsync): one packed shard into an interleaved frame, possibly on another GPU."""
    _check(lib().ptl_device_copy2d_async(C.c_void_p(dst), dst_pitch, C.c_void_p(src), src_pitch, width_bytes, rows, C.c_void_p(stream or None)), "ptl_device_copy2d_async")


IPC_HANDLE_BYTES = 64


def ipc_export(ptr: int) -> bytes:
    """Handle of a `device_alloc` buffer for the other processes of the node (ptl_ipc_export)."""
    buf = C.create_string_buffer(IPC_HANDLE_BYTES)
    _check(lib().ptl_ipc_export(C.c_void_p(ptr), buf), "ipc_export")
    return buf.raw


def ipc_open(handle: bytes, device: int = 0) -> int:
    """Map another process's exported buffer into this process (on `device`); returns the local address."""
    if len(handle) != IPC_HANDLE_BYTES:
        raise PortalError("an IPC handle is 64 bytes")
    p = C.c_void_p()
    _check(lib().ptl_ipc_open(device, handle, C.byref(p)), "ipc_open")
    return int(p.value)


def ipc_close(ptr: int) -> None:
    _check(lib().ptl_ipc_close(C.c_void_p(ptr)), "ipc_close")


def png_write(path: str, rgba8: np.ndarray) -> None:
    a = np.ascontiguousarray(rgba8, dtype=np.uint8)
    _check(lib().ptl_png_write(path.encode(), a.ctypes.data, a.shape[1], a.shape[0]), "png_write")


def png_read(path: str) -> np.ndarray:
    p, w, h = C.c_void_p(), C.c_int(), C.c_int()
    _check(lib().ptl_png_read(path.encode(), C.byref(p), C.byref(w), C.byref(h)), "png_read")
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (h.value, w.value, 4)).copy()
    finally:
        lib().ptl_free(p)


def ron_format(text: str) -> str:
    """Parse RON and write it back in the layout of the reference's scene files (ron 0.10 pretty printer)."""
    p = lib().ptl_ron_format(text.encode("utf-8"))
    if not p:
        raise PortalError(_err())
    try:
        return C.string_at(p).decode("utf-8")
    finally:
        lib().ptl_free(p)


def bound_glsl(body: str, out_functions=()):
    """(text, n): an intersection-material snippet with the caller's distance bound in the `nearer` blocks it recognises (n of them)."""
    n = C.c_int()
    p = lib().ptl_bound_glsl(body.encode("utf-8"), ",".join(out_functions).encode(), C.byref(n))
    if not p:
        raise PortalError(lib().ptl_last_error().decode())
    try:
        return C.string_at(p).decode("utf-8"), n.value
    finally:
        lib().ptl_free(p)


def dmath(op: str, a, b=None, c=None) -> np.ndarray:
    """One binary64 primitive of the host's matrix arithmetic (ptl_dmath): 16 doubles, column-major, as a flat array."""
    arr = lambda v: (C.c_double * len(v))(*[float(x) for x in v]) if v is not None else None
    out = (C.c_double * 16)()
    _check(lib().ptl_dmath(op.encode(), arr(a), arr(b), arr(c), out), "ptl_dmath")
    return np.array(out, np.float64)


def snippets_keep_rays_affine(code: str):
    """(ok, why): does this GLSL text keep every ray's w at 1 (origin) / 0 (direction)?  (the scan behind the affine-rays builds)"""
    why = C.create_string_buffer(512)
    rc = lib().ptl_snippets_keep_rays_affine(code.encode("utf-8"), why, len(why))
    if rc < 0:
        raise PortalError(_err())
    return rc == 1, why.value.decode("utf-8", "replace")


def translate_glsl(code: str) -> str:
    p = lib().ptl_translate_glsl(code.encode("utf-8"))
    if not p:
        raise PortalError(_err())
    try:
        return C.string_at(p).decode("utf-8")
    finally:
        lib().ptl_free(p)


def translate_library_glsl(code: str) -> str:
    p = lib().ptl_translate_library_glsl(code.encode("utf-8"))
    if not p:
        raise PortalError(_err())
    try:
        return C.string_at(p).decode("utf-8")
    finally:
        lib().ptl_free(p)


def hoist_glsl(code: str, uniforms: dict, out_functions=(), body_only: bool = True, params=()):
    """glsl_hoist.h on one snippet (for tests): `uniforms` maps name -> GLSL type.  Returns (rewritten GLSL, prologue text with one
    "// member: type name" line per created member in front)."""
    L = lib()
    L.ptl_hoist_glsl.restype = C.c_void_p
    L.ptl_hoist_glsl.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.POINTER(C.c_void_p)]
    prologue = C.c_void_p()
    p = L.ptl_hoist_glsl(code.encode("utf-8"), ";".join(f"{t} {n}" for n, t in uniforms.items()).encode(), ";".join(out_functions).encode(),
                         1 if body_only else 0, ";".join(params).encode(), C.byref(prologue))
    try:
        return C.string_at(p).decode("utf-8"), C.string_at(prologue.value).decode("utf-8")
    finally:
        L.ptl_free(p)
        L.ptl_free(prologue.value)


def formula_eval(text: str, variables: Optional[dict] = None, time: float = 0.0) -> Optional[float]:
    variables = variables or {}
    names = (C.c_char_p * len(variables))(*[k.encode() for k in variables])
    vals = (C.c_double * len(variables))(*[float(v) for v in variables.values()])
    out = C.c_double()
    rc = lib().ptl_formula_eval(text.encode(), names, vals, len(variables), time, C.byref(out))
    return out.value if rc == 0 else None


def scene_path(name: str) -> str:
    """`monoportal` -> <repo>/scenes/monoportal.ron (the reference resolves names through its
    built-in registry, src/gui/scenes.rs:589-603)."""
    if os.path.exists(name):
        return name
    cand = os.path.join(REPO_ROOT, "scenes", name if name.endswith(".ron") else name + ".ron")
    if os.path.exists(cand):
        return cand
    raise PortalError(f"Unknown scene `{name}`")
