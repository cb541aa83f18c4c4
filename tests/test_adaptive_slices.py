"""Adaptive anti-aliasing of a batch of slices (`render --clip-adaptive-aa`): the classification kernel over a stack of
frames (portal_amd/csrc/kernels/aa_edges_slices.hip), the refine entry over slices of kernels generated with FLAG_REFINE_SLICES, both
layers of the C ABI, the Python mirror and the clip loop of the CLI, against tests/adaptive_reference.py and against draws one by one.
Every comparison is equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adaptive_reference as ar
from tests.adaptive_reference import bits as _bits, cuda_words as _cuda_words, exe as _exe, resource_usage as _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID, NO_DEVICE = -1, -6
SCENES = ["basics", "monoportal", "portal_in_portal", "triple_portal", "mobius_monoportal"]


def _base_flags(pa, build):
    return {"unspecialised": 0, "baked": pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL, "patterns": pa.FLAG_SPECIALIZE_PATTERNS}[build]


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene_name", SCENES)
def test_flag_adds_one_entry_to_the_slices_source_and_nothing_else(pa, scene_name):
    scene = pa.Scene.from_file(pa.scene_path(scene_name))
    entry = pa.device_source("refine_slices_entry")
    assert entry.count("ptl_render_refine_slices_kernel(") == 1
    for build in ("unspecialised", "baked", "patterns"):
        f = _base_flags(pa, build)
        with_flag = scene.generate_source(f | pa.FLAG_REFINE_SLICES)
        assert with_flag.replace(entry, "") == scene.generate_source(f | pa.FLAG_SLICES)
        assert with_flag.count("ptl_render_refine_slices_kernel(") == 1
        assert with_flag == scene.generate_source(f | pa.FLAG_REFINE_SLICES | pa.FLAG_SLICES)  # the flag implies the slices entry
        for other in (f, f | pa.FLAG_SLICES, f | pa.FLAG_REFINE, f | pa.FLAG_COUNT_SEGMENTS):
            src = scene.generate_source(other)
            assert "refine_slices" not in src and "REFINE_SLICES" not in src
        for refused in (pa.FLAG_REFINE | pa.FLAG_SLICES, pa.FLAG_REFINE | pa.FLAG_REFINE_SLICES):
            with pytest.raises(pa.PortalError):
                scene.generate_source(f | refused)
    assert pa.FLAG_REFINE_SLICES == 1 << 29
    with pytest.raises(pa.PortalError):
        pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_REFINE | pa.FLAG_REFINE_SLICES)


def _entry_notes(pa, code, entry):
    note = lambda key: pa.lib().ptl_code_object_note(code, len(code), key.encode(), entry.encode())  # noqa: E731
    return {k: note(k) for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count")}


def _compiles_with_both_entries(pa, scene_name, flags, label):
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene_name)), device=-1, flags=flags)
    assert "ptl_render_refine_slices_kernel(" in r.kernel_source() and "ptl_render_slices_kernel(" in r.kernel_source()
    code = r.code_object()
    assert b"ptl_render_refine_slices_kernel" in code and b"ptl_render_slices_kernel" in code
    render, refine = _entry_notes(pa, code, "ptl_render_slices_kernel"), _entry_notes(pa, code, "ptl_render_refine_slices_kernel")
    print(f"{scene_name} {label}: slices render entry {render}, refine entry over slices {refine}")
    assert refine[".private_segment_fixed_size"] == 0 and refine[".vgpr_spill_count"] == 0
    assert render[".private_segment_fixed_size"] == 0
    assert 0 < refine[".vgpr_count"] <= 128  # (the render entry's launch bounds: 256 threads)


@pytest.mark.parametrize("build", ["unspecialised", "baked", "patterns"])
@pytest.mark.parametrize("scene_name", ["basics", "monoportal", "portal_in_portal"])
def test_source_with_the_flag_compiles_for_gfx950_without_scratch(pa, scene_name, build):
    _compiles_with_both_entries(pa, scene_name, _base_flags(pa, build) | pa.FLAG_REFINE_SLICES, build)


def test_source_with_the_flag_and_the_segment_counter_compiles(pa):
    _compiles_with_both_entries(pa, "basics", pa.FLAG_COUNT_SEGMENTS | pa.FLAG_REFINE_SLICES, "count segments")


def test_make_kernels_builds_aa_edges_slices_without_scratch(pa, tmp_path):
    subprocess.run(["make", "kernels"], cwd=ROOT, check=True, capture_output=True)
    assert os.path.getsize(os.path.join(ROOT, "portal_amd", "kernels", "aa_edges_slices.hsaco")) > 1000
    src = os.path.join(ROOT, "portal_amd", "csrc", "kernels", "aa_edges_slices.hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-vgpr-regalloc=basic", "--genco", "--no-gpu-bundle-output",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "aa_edges_slices.hsaco")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    usage = _resource_usage(out.stderr)
    print(usage)
    assert set(usage) == {"ptl_aa_edges_slices_kernel"}
    u = usage["ptl_aa_edges_slices_kernel"]
    assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs"] <= 64 and u["LDS Size [bytes/block]"] <= 16384, u


def test_classification_over_a_stack_validates_before_any_gpu_call(pa):
    L = pa.lib()
    frames, lists, counts = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)

    def edges(fr=frames, slice_pixels=64, n=2, w=8, h=8, t=4, ls=lists, list_stride=64, cn=counts):
        return L.ptl_aa_edges_slices(-1, fr, slice_pixels, n, w, h, t, ls, list_stride, cn, None, None)

    assert edges(fr=None) == INVALID and edges(ls=None) == INVALID and edges(cn=None) == INVALID
    for k in ("fr", "ls", "cn"):
        assert edges(**{k: C.c_void_p((1 << 20) + 2)}) == INVALID  # pixels, entries and counts are 32-bit words
    assert edges(n=0) == INVALID and edges(n=17) == INVALID and edges(n=-1) == INVALID
    for w, h in ((0, 8), (8, 0), (-3, 8), (8, -1)):
        assert edges(w=w, h=h) == INVALID
    assert edges(w=1 << 16, h=(1 << 15) + 1, slice_pixels=1 << 40, list_stride=1 << 40) == INVALID  # beyond 2^31 pixels
    assert edges(slice_pixels=63) == INVALID and edges(list_stride=63) == INVALID
    assert edges(t=-2) == INVALID and edges(t=256) == INVALID
    assert edges() == NO_DEVICE and edges(n=16, t=-1) == NO_DEVICE and edges(n=1, t=255) == NO_DEVICE  # everything valid: only now the missing device is noticed


def test_layer_one_validates_before_any_gpu_call(pa):
    L = pa.lib()
    out, lists, counts = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    r = pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_REFINE_SLICES)
    k = L.ptl_renderer_kernel(r._h)

    def refine(kernel=k, f=pa.Frame(8, 8, 0, 1, 0), n=2, ls=lists, list_stride=64, cn=counts, slice_pixels=64):
        return L.ptl_kernel_render_slices_refine(kernel, C.byref(f) if f is not None else None, n, ls, list_stride, cn, out, None, slice_pixels, None, None, None)

    assert refine(kernel=None) == INVALID and refine(f=None) == INVALID and refine(ls=None) == INVALID and refine(cn=None) == INVALID
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        assert refine(f=pa.Frame(w, h, 0, 1, 0)) == INVALID
    for f in (pa.Frame(8, 64, 0, 2, 0), pa.Frame(8, 64, 1, 2, 0), pa.Frame(8, 8, 0, 1, 1)):  # sharded, in place
        assert refine(f=f, slice_pixels=512, list_stride=512) == INVALID and "whole frame" in pa.last_error()
    assert refine(f=pa.Frame(1 << 16, (1 << 15) + 1, 0, 1, 0), slice_pixels=1 << 40, list_stride=1 << 40) == INVALID
    assert refine(list_stride=63) == INVALID and "list_stride" in pa.last_error()
    assert refine(slice_pixels=63) == INVALID and "slice_pixels" in pa.last_error()
    assert refine(n=0) == INVALID and refine(n=17) == INVALID
    for flags in (0, pa.FLAG_SLICES, pa.FLAG_REFINE):  # kernels without the entry
        other = pa.SceneRenderer(scene, device=-1, flags=flags)
        assert refine(kernel=L.ptl_renderer_kernel(other._h)) == INVALID and "PTL_FLAG_REFINE_SLICES" in pa.last_error()
    # the order of the checks: a sharded frame is refused as such even with a kernel that has no entry
    assert refine(kernel=L.ptl_renderer_kernel(other._h), f=pa.Frame(8, 64, 0, 2, 0), slice_pixels=512, list_stride=512) == INVALID and "whole frame" in pa.last_error()
    # a kernel with the entry and nothing staged (a compile-only kernel cannot stage: the call never gets as far as asking for a device)
    assert refine() == INVALID and "no staged slices" in pa.last_error()

    one = C.c_int(1)
    staged = lambda kernel, index, name, typ=pa.PTL_I32, value=C.byref(one): L.ptl_kernel_set_staged_uniform(kernel, index, name, typ, value)  # noqa: E731
    assert staged(None, 0, b"_aa_count") == INVALID and staged(k, 0, None) == INVALID and staged(k, 0, b"_aa_count", value=None) == INVALID
    assert staged(k, -1, b"_aa_count") == INVALID and staged(k, 16, b"_aa_count") == INVALID
    assert staged(k, 0, b"no_such_uniform") == 1  # PTL_UNKNOWN_UNIFORM, the no-op code of ptl_kernel_set_uniform
    assert L.ptl_kernel_set_uniform(k, b"no_such_uniform", pa.PTL_I32, C.byref(one)) == 1
    assert staged(k, 0, b"_aa_count", typ=pa.PTL_F32) == L.ptl_kernel_set_uniform(k, b"_aa_count", pa.PTL_F32, C.byref(one)) < 0  # the same type error
    assert staged(k, 0, b"_aa_count") == INVALID and "no staged slices" in pa.last_error()


def test_layer_two_validates_before_any_gpu_call(pa):
    L = pa.lib()
    out = C.c_void_p(1 << 20)
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    r = pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_REFINE_SLICES)
    whole = pa.Frame(8, 8, 0, 1, 0)

    def draw(rr=r, f=whole, n=2, o=out, slice_pixels=64):
        return L.ptl_renderer_draw_slices_adaptive(rr._h if rr is not None else None, C.byref(f) if f is not None else None, n, o, None, slice_pixels, None, None)

    assert L.ptl_renderer_adaptive_slices_result(r._h, None, None, None) == INVALID and L.ptl_renderer_adaptive_slices_result(None, None, None, None) == INVALID
    for j in range(2):
        r.set_option("aa_start", j)
        r.stage_slice(whole, j)
    assert draw(rr=None) == INVALID and draw(f=None) == INVALID and draw(n=0) == INVALID and draw(n=17) == INVALID
    assert draw(o=None) == INVALID  # the classification reads the RGBA8 output: it is required
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        assert draw(f=pa.Frame(w, h, 0, 1, 0)) == INVALID
    for f in (pa.Frame(8, 64, 0, 2, 0), pa.Frame(8, 64, 1, 2, 0), pa.Frame(8, 8, 0, 1, 1)):
        assert draw(f=f, slice_pixels=512) == INVALID and "whole frame" in pa.last_error()
    assert draw(f=pa.Frame(1 << 16, (1 << 15) + 1, 0, 1, 0), slice_pixels=1 << 40) == INVALID
    assert draw(slice_pixels=63) == INVALID and "slice_pixels" in pa.last_error()
    for t in (-2, 256):
        r.set_option("adaptive_aa_threshold", t)
        assert draw() == INVALID and "adaptive_aa_threshold" in pa.last_error()
    r.set_option("adaptive_aa_threshold", 4)
    for flags in (0, pa.FLAG_SLICES, pa.FLAG_REFINE):  # a renderer without the flag
        other = pa.SceneRenderer(scene, device=-1, flags=flags)
        assert draw(rr=other) == INVALID and "PTL_FLAG_REFINE_SLICES" in pa.last_error()
    assert draw(n=3) == INVALID and "not all staged" in pa.last_error()  # slices 0 and 1 are staged, 2 is not
    assert draw() == NO_DEVICE  # everything valid: only now the missing device is noticed
    assert L.ptl_renderer_adaptive_slices_result(r._h, None, None, None) == INVALID  # still no adaptive draw


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--clip-adaptive-aa", "256"], "-1 .. 255"), ("render", ["--clip-adaptive-aa", "-2"], "-1 .. 255"),
                                              ("render-frame", ["--clip-adaptive-aa"], "render"), ("render-frame", ["--clip-adaptive-aa", "4"], "render")])
def test_cli_refuses_while_the_arguments_are_parsed(pa, tmp_path, cmd, extra, reason):
    """Exit status 2, one line of reason, nothing written."""
    target = ["--output", str(tmp_path / "f.png")] if cmd == "render-frame" else ["--out-dir", str(tmp_path)]
    out = subprocess.run([_exe(pa), cmd, pa.scene_path("basics")] + target + extra, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and "--clip-adaptive-aa" in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


def _words(t):
    return t.cpu().numpy().view(np.uint32)


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _synthetic(kind, w, h, t, rng):
    """The three frame kinds of tests/test_adaptive_aa.py (noise of amplitude about T, straight edges with steps of T and T + 1, every pixel
    different), and a flat frame.  Alpha is random throughout: it must not matter."""
    p = np.empty((h, w, 4), np.uint8)
    p[:, :, 3] = rng.integers(0, 256, (h, w))
    if kind == "flat":
        p[:, :, :3] = (90, 120, 200)
    elif kind == "noise":
        amp = min(255, max(t, 0) + max(1, t // 4))
        p[:, :, :3] = rng.integers(0, amp + 1, (h, w, 3))
    elif kind == "edges":
        step = min(max(t, 0), 254)
        p[:, :, :3] = 0
        p[h // 2:, :, 0] += step + 1
        p[:, (2 * w) // 3:, 1] += step
        ys, xs = np.mgrid[0:h, 0:w]
        p[:, :, 2][xs * h > ys * w] += step + 1
    else:  # every pixel differs from each of its neighbours, by more than 4 codes in some channel
        i = np.arange(w * h, dtype=np.int64).reshape(h, w)
        p[:, :, 0], p[:, :, 1], p[:, :, 2] = (i * 7) & 255, (i >> 8) & 255, (i * 37 >> 3) & 255
    return p


STACK_SIZES = [(1, 1), (7, 5), (65, 33), (130, 70)]
LIST_GUARD, FRAME_GUARD, FILL = 16, 8, 0xDEADBEEF


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", STACK_SIZES, ids=[f"{w}x{h}" for w, h in STACK_SIZES])
def test_classification_over_a_stack_lists_every_slice_on_its_own(gpu, w, h):
    pa = gpu
    pixels = w * h
    list_stride, slice_pixels = pixels + LIST_GUARD, pixels + FRAME_GUARD
    seen = set()
    for n in (1, 3, 16):
        for t in (-1, 4, 255):
            kinds = [("different", "flat", "noise", "edges")[(z + (t & 3)) % 4] for z in range(n)] if n > 1 else [("noise", "edges", "different")[t % 3]]
            frames = [_synthetic(kind, w, h, t, np.random.default_rng(100000 * n + 1000 * z + 10 * w + t + 1)) for z, kind in enumerate(kinds)]
            want = [ar.refined_indices(p, t) for p in frames]
            for kind, got in zip(kinds, want):
                seen.add((kind, t, got.size == 0, got.size == pixels))
                if kind == "flat":
                    assert got.size == (pixels if t == -1 else 0)
                if kind == "different" and t == 4 and pixels > 1:
                    assert got.size == pixels
            stack = np.full((n, slice_pixels), 0xA5A5A5A5, np.uint32)  # guard pixels between the frames: a halo that left its frame would read them
            for z, p in enumerate(frames):
                stack[z, :pixels] = _bits(p).reshape(-1)
            dev = _cuda_words(stack)
            lists = _cuda_words(np.full(n * list_stride + LIST_GUARD, FILL, np.uint32))
            counts = _cuda_words(np.full(n + 4, 0x12345678, np.uint32))  # stale counts: the call resets counts[0 .. n) itself
            sets = []
            for _ in range(2):  # twice on the same buffers: the reset works, the sets are the same
                pa.aa_edges_slices_device(dev.data_ptr(), slice_pixels, n, w, h, t, lists.data_ptr(), list_stride, counts.data_ptr(), stream=_stream())
                import torch

                torch.cuda.synchronize()
                got_counts, got_lists = _words(counts), _words(lists)
                assert (got_counts[n:] == 0x12345678).all() and (got_lists[n * list_stride:] == FILL).all()
                per_slice = []
                for z in range(n):
                    count = int(got_counts[z])
                    assert count == want[z].size, (n, t, z, kinds[z], count, want[z].size)
                    mine = got_lists[z * list_stride:(z + 1) * list_stride]
                    assert np.array_equal(np.sort(mine[:count]), want[z]), (n, t, z, kinds[z])  # sorted and equal: unique and in range as well
                    assert (mine[pixels:] == FILL).all(), "written between two lists"
                    per_slice.append(np.sort(mine[:count]))
                sets.append(per_slice)
            assert all(np.array_equal(a, b) for a, b in zip(*sets))
            assert np.array_equal(_words(dev).reshape(n, slice_pixels), stack)
    if pixels >= 64:  # not vacuous: at T = 4 some slice flags a part of its frame, some slices flag nothing and some everything
        assert any(t == 4 and not empty and not full for (_, t, empty, full) in seen), seen
        assert any(t == 4 and empty for (_, t, empty, full) in seen) and any(t == 4 and full for (_, t, empty, full) in seen), seen


_made = {}


def _renderer(pa, scene_name, build, entry_flags, animate):
    """One renderer per (scene, build, entry flags), on its own scene object; `animate`: taken into the scene's first clip, so update() moves it."""
    key = (scene_name, build, entry_flags, animate)
    if key not in _made:
        scene = pa.Scene.from_file(pa.scene_path(scene_name))
        if animate and scene.animations():
            scene.init_animation(scene.animations()[0][0])
        r = pa.SceneRenderer(scene, device=0, flags=_base_flags(pa, build) | entry_flags)
        r.set_option("render_depth", 12)
        _made[key] = (scene, r)
    return _made[key]


def _enter_state(r, j, n):
    """Slice j's state, as a clip sets it: its own time and its own `_aa_start` window."""
    r.set_option("aa_start", j)
    r.update(0.37 * j)


def _one_by_one(r, w, h, n, aa):
    """P_z and F_z of the contract: the frames of draws one by one with `_aa_count` 1 and `aa`, by a renderer without the slices entry."""
    p, f = [], []
    for j in range(n):
        _enter_state(r, j, n)
        r.set_option("aa_count", 1)
        p.append(r.draw(w, h, rgba8=True, rgba32f=True))
        r.set_option("aa_count", aa)
        f.append(r.draw(w, h, rgba8=True, rgba32f=True))
    return p, f


def _stage_all(r, frame, n, aa):
    r.set_option("aa_count", aa)
    for j in range(n):
        _enter_state(r, j, n)
        r.stage_slice(frame, j)


def _draw_slices_adaptive(pa, r, w, h, n, t, rgba32f=True, slice_pixels=None):
    """The staged slices through layer 2 into guarded device buffers -> (rgba8 [n, h, w, 4], float bits or None, counts [n], lists)."""
    import torch

    pixels = w * h
    slice_pixels = slice_pixels or pixels + FRAME_GUARD
    d8 = _cuda_words(np.full(n * slice_pixels, 0xA5A5A5A5, np.uint32))
    d32 = _cuda_words(np.full(4 * n * slice_pixels, 0xA5A5A5A5, np.uint32)) if rgba32f else None
    r.set_option("adaptive_aa_threshold", t)
    rejits = r.rejit_count()
    r.draw_slices_adaptive(pa.Frame(w, h, 0, 1), n, d8.data_ptr(), d32.data_ptr() if rgba32f else 0, slice_pixels, stream=_stream())
    assert r.rejit_count() == rejits  # nothing is rebuilt by the draw
    torch.cuda.synchronize()
    words8 = _words(d8).reshape(n, slice_pixels)
    assert (words8[:, pixels:] == 0xA5A5A5A5).all(), "RGBA8 written between two frames"
    out8 = np.ascontiguousarray(words8[:, :pixels]).view(np.uint8).reshape(n, h, w, 4)
    out32 = None
    if rgba32f:
        words32 = _words(d32).reshape(n, 4 * slice_pixels)
        assert (words32[:, 4 * pixels:] == 0xA5A5A5A5).all(), "RGBA32F written between two frames"
        out32 = np.ascontiguousarray(words32[:, :4 * pixels]).reshape(n, h, w, 4)
    lists_ptr, stride, counts_ptr = r.adaptive_slices_result()
    assert stride >= pixels
    counts = pa.device_download(counts_ptr, 4 * n).view(np.uint32).copy()
    lists = [pa.device_download(lists_ptr + 4 * z * stride, 4 * int(counts[z])).view(np.uint32).copy() if counts[z] else np.empty(0, np.uint32) for z in range(n)]
    return out8, out32, counts, lists


# ---- the refine entry over slices through layer 1: lists the caller made ---------------------------
def _stage_on_the_kernel(pa, r, w, h, n, aa):
    """Layer 1: a draw brings the kernel's uniforms to slice j's state (a single draw of such a module is a batch of one), ptl_kernel_stage_slice
    makes them slice j.  -> the frames those draws gave (F_z by the module's own render entry)."""
    L = pa.lib()
    drawn = []
    kernel = L.ptl_renderer_kernel(r._h)
    for j in range(n):
        _enter_state(r, j, n)
        r.set_option("aa_count", aa)
        drawn.append(r.draw(w, h, rgba8=True, rgba32f=True))
        assert L.ptl_renderer_kernel(r._h) == kernel, "the kernel was rebuilt between two stage calls: this test wants an un-specialised build"
        assert L.ptl_kernel_stage_slice(kernel, j) == 0, pa.last_error()
    return drawn


def _refine_slices_through_layer_one(pa, r, w, h, entries, counts, start8=None, start32=None, segments=False):
    """ptl_kernel_render_slices_refine on one list per slice (`entries[z]`, all uploaded, counts[z] of them valid) over device copies of the start
    frames.  Guards between and behind lists, frames and counts must survive."""
    import torch

    n, pixels = len(entries), w * h
    list_stride = max(max(e.size for e in entries), pixels) + LIST_GUARD
    slice_pixels = pixels + FRAME_GUARD
    host_lists = np.full(n * list_stride, FILL, np.uint32)
    for z, e in enumerate(entries):
        host_lists[z * list_stride:z * list_stride + e.size] = e
    lists = _cuda_words(host_lists)
    cnt = _cuda_words(np.concatenate([np.asarray(counts, np.uint32), np.full(4, 0x5A5A5A5A, np.uint32)]))

    def guarded(start, per_pixel):
        if start is None:
            return None
        host = np.full((n, per_pixel * slice_pixels), 0xA5A5A5A5, np.uint32)
        for z in range(n):
            host[z, :per_pixel * pixels] = _bits(start[z]).reshape(-1)
        return _cuda_words(host)

    d8, d32 = guarded(start8, 1), guarded(start32, 4)
    seg = torch.zeros(2, dtype=torch.int64, device="cuda") if segments else None
    r.refine_slices_device(pa.Frame(w, h, 0, 1, 0), n, lists.data_ptr(), list_stride, cnt.data_ptr(), out_rgba8=d8.data_ptr() if d8 is not None else 0,
                           out_rgba32f=d32.data_ptr() if d32 is not None else 0, slice_pixels=slice_pixels, segments=seg.data_ptr() if segments else 0, stream=_stream())
    torch.cuda.synchronize()
    assert np.array_equal(_words(lists), host_lists) and np.array_equal(_words(cnt)[n:], [0x5A5A5A5A] * 4) and np.array_equal(_words(cnt)[:n], np.asarray(counts, np.uint32))
    out8 = out32 = None
    if d8 is not None:
        words = _words(d8).reshape(n, slice_pixels)
        assert (words[:, pixels:] == 0xA5A5A5A5).all(), "RGBA8 written between two frames"
        out8 = np.ascontiguousarray(words[:, :pixels]).view(np.uint8).reshape(n, h, w, 4)
    if d32 is not None:
        words = _words(d32).reshape(n, 4 * slice_pixels)
        assert (words[:, 4 * pixels:] == 0xA5A5A5A5).all(), "RGBA32F written between two frames"
        out32 = np.ascontiguousarray(words[:, :4 * pixels]).reshape(n, h, w, 4)
    if segments:
        assert int(seg[1].item()) == 0
    return out8, out32, int(seg[0].item()) if segments else None


@pytest.mark.gpu
def test_refine_entry_over_slices_shades_exactly_the_callers_lists(gpu):
    """basics at 70x37, aa 4, three slices staged at three times with `_aa_start` 0, 1, 2, over device copies of P_z.  Slice 0: a shuffled half
    of the pixels, each twice, with W*H and 0xFFFFFFFF interleaved and a count below the buffer's length; slice 1: count 0; slice 2: a
    permutation of all pixels.  The result is where(listed_z, F_z, P_z) in bytes and float bits, with either output null as well."""
    pa = gpu
    w, h, n, aa = 70, 37, 3, 4
    pixels = w * h
    _, plain = _renderer(pa, "basics", "unspecialised", 0, True)
    p, f = _one_by_one(plain, w, h, n, aa)
    p8, f8 = [x["rgba8"] for x in p], [x["rgba8"] for x in f]
    p32, f32 = [_bits(x["rgba32f"]) for x in p], [_bits(x["rgba32f"]) for x in f]
    assert not np.array_equal(p8[0], p8[1]) and not np.array_equal(p8[1], p8[2])  # the slices differ
    _, r = _renderer(pa, "basics", "unspecialised", pa.FLAG_REFINE_SLICES, True)
    drawn = _stage_on_the_kernel(pa, r, w, h, n, aa)
    for z in range(n):  # (a single draw of the module with both entries is the plain renderer's)
        assert np.array_equal(drawn[z]["rgba8"], f8[z]) and np.array_equal(_bits(drawn[z]["rgba32f"]), f32[z])
    rng = np.random.default_rng(7037)
    half = rng.permutation(pixels)[: pixels // 2].astype(np.uint32)
    body = rng.permutation(np.concatenate([half, half]))
    outside = np.where(np.arange(body.size // 2) % 2 == 0, pixels, 0xFFFFFFFF).astype(np.uint32)
    first = np.stack([body[0::2], body[1::2], outside], axis=1).reshape(-1)  # every third entry names no pixel
    assert first.size == 3885
    entries = [first, rng.permutation(pixels).astype(np.uint32), rng.permutation(pixels).astype(np.uint32)]
    counts = [first.size * 2 // 3, 0, pixels]

    listed = []
    for z in range(n):
        named = entries[z][:counts[z]]
        m = np.zeros(pixels, bool)
        m[named[named < pixels]] = True
        listed.append(m.reshape(h, w))
    differs = [(f8[z] != p8[z]).any(axis=2) | (f32[z] != p32[z]).any(axis=2) for z in range(n)]
    stats = dict(listed=[int(m.sum()) for m in listed], listed_and_different=[int((m & d).sum()) for m, d in zip(listed, differs)],
                 unlisted_and_different=[int((~m & d).sum()) for m, d in zip(listed, differs)])
    print(stats)
    assert 0 < listed[0].sum() < pixels and not listed[1].any() and listed[2].all()
    assert stats["listed_and_different"][0] >= 10 and stats["unlisted_and_different"][0] >= 10 and stats["unlisted_and_different"][1] >= 10, stats  # shading nothing, or everything, must not pass
    all_of_first = np.zeros(pixels, bool)
    all_of_first[first[first < pixels]] = True
    assert (all_of_first.reshape(h, w) & ~listed[0] & differs[0]).sum() >= 5  # some pixel that differs is named only beyond the count: it stays P
    want8 = [ar.select(listed[z], f8[z], p8[z]) for z in range(n)]
    want32 = [ar.select(listed[z], f32[z], p32[z]) for z in range(n)]

    def check(out8, out32):
        for z in range(n):
            if out8 is not None:
                bad = np.argwhere((out8[z] != want8[z]).any(axis=2))
                assert bad.size == 0, f"slice {z}: {len(bad)} pixels differ in RGBA8, first (y, x) = {bad[0].tolist()}, listed there: {bool(listed[z][tuple(bad[0])])}"
            if out32 is not None:
                bad = np.argwhere((out32[z] != want32[z]).any(axis=2))
                assert bad.size == 0, f"slice {z}: {len(bad)} pixels differ in RGBA32F, first (y, x) = {bad[0].tolist()}, listed there: {bool(listed[z][tuple(bad[0])])}"

    out8, out32, _ = _refine_slices_through_layer_one(pa, r, w, h, entries, counts, start8=p8, start32=p32)
    check(out8, out32)
    out8, out32, _ = _refine_slices_through_layer_one(pa, r, w, h, entries, counts, start8=p8)  # RGBA8 only (the slices stay staged: the same launch again)
    assert out32 is None
    check(out8, None)
    out8, out32, _ = _refine_slices_through_layer_one(pa, r, w, h, entries, counts, start32=p32)  # float only
    assert out8 is None
    check(None, out32)
    # one uniform inside a staged slice: with `_aa_count` 1 in slice 2, its permutation of all pixels gives P_2 instead of F_2
    assert r.set_staged_uniform(2, "_aa_count", 1) == 0 and r.set_staged_uniform(2, "no_such_uniform", 1) == 1
    out8, out32, _ = _refine_slices_through_layer_one(pa, r, w, h, entries, counts, start8=f8, start32=f32)
    assert np.array_equal(out8[2], p8[2]) and np.array_equal(out32[2], p32[2]) and np.array_equal(out8[1], f8[1])


@pytest.mark.gpu
def test_refine_entry_over_slices_counts_the_segments_of_its_lists(gpu):
    """A FLAG_COUNT_SEGMENTS | FLAG_REFINE_SLICES build at 64x36, two slices, a permutation of all pixels each: the counter is the sum of what the
    render entry counts for the two aa-4 frames one by one; entries outside the frame count nothing."""
    pa = gpu
    w, h, n, aa = 64, 36, 2, 4
    pixels = w * h
    _, r = _renderer(pa, "basics", "unspecialised", pa.FLAG_COUNT_SEGMENTS | pa.FLAG_REFINE_SLICES, True)
    L = pa.lib()
    kernel = L.ptl_renderer_kernel(r._h)
    drawn = []
    for j in range(n):
        _enter_state(r, j, n)
        r.set_option("aa_count", aa)
        drawn.append(r.draw(w, h, rgba8=True, segments=True))
        assert L.ptl_renderer_kernel(r._h) == kernel and L.ptl_kernel_stage_slice(kernel, j) == 0
    total = sum(d["segments"] for d in drawn)
    assert all(d["segments"] > aa * pixels for d in drawn) and drawn[0]["segments"] != drawn[1]["segments"]
    rng = np.random.default_rng(6436)
    entries = [rng.permutation(pixels).astype(np.uint32) for _ in range(n)]
    start8 = [np.full((h, w, 4), 0x3C, np.uint8)] * n
    out8, _, counted = _refine_slices_through_layer_one(pa, r, w, h, entries, [pixels] * n, start8=start8, segments=True)
    assert counted == total, (counted, total)
    assert all(np.array_equal(out8[z], drawn[z]["rgba8"]) for z in range(n))
    padded = [np.concatenate([e, np.full(100, pixels, np.uint32), np.full(100, 0xFFFFFFFF, np.uint32)]) for e in entries]
    assert _refine_slices_through_layer_one(pa, r, w, h, padded, [pixels + 200] * n, start8=start8, segments=True)[2] == total
    only_first = _refine_slices_through_layer_one(pa, r, w, h, entries, [pixels, 0], start8=start8, segments=True)[2]
    assert only_first == drawn[0]["segments"]


# ---- layer 2 ------------------------------------------------------------------------------------------
def _refine_slices_grid(n, pixels):
    """The grid rule of the refine launcher behind ptl_kernel_render_slices_refine, read from the source so that a changed rule fails the
    second-trip test instead of leaving it vacuous."""
    src = open(os.path.join(ROOT, "portal_amd", "csrc", "host", "kernel.cpp")).read()
    m = re.findall(r"const unsigned gx = \(unsigned\)std::min<long long>\(chunks, (\d+) / n\);", src)
    assert len(m) == 1, "the refine launcher no longer spells its grid as min(chunks, N / n)"
    return min((pixels + 255) // 256, int(m[0]) // n)


def test_refine_slices_grid_is_what_the_second_trip_test_crosses():
    pixels = 256 * 130
    assert _refine_slices_grid(16, pixels) == 128 and 128 * 256 == 32768 < pixels == 33280 and (pixels - 32768) == 2 * 256  # a second trip that ends with the second workgroup's chunk ...
    assert _refine_slices_grid(2, pixels) == 130 == (pixels + 255) // 256  # ... and one trip
    assert _refine_slices_grid(1, 3840 * 2160) == 2048 and _refine_slices_grid(16, 3840 * 2160) == 128 and _refine_slices_grid(3, 3840 * 2160) == 682


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 2])
def test_refine_pass_over_slices_takes_a_second_trip(gpu, n):
    """basics at 256x130 (33 280 entries per slice), aa 2, T = -1 through layer 2.  With 16 slices a slice has 128 workgroups, a trip covers
    32 768 entries and the second trip ends inside the grid; with 2 slices 130 workgroups take one trip.  Every slice is the aa-2 frame of a
    draw one by one with `_aa_start` = j, bit for bit."""
    pa = gpu
    w, h, aa = 256, 130, 2
    _, plain = _renderer(pa, "basics", "unspecialised", 0, True)
    _, f = _one_by_one(plain, w, h, n, aa)
    _, r = _renderer(pa, "basics", "unspecialised", pa.FLAG_REFINE_SLICES, True)
    _stage_all(r, pa.Frame(w, h, 0, 1), n, aa)
    out8, out32, counts, lists = _draw_slices_adaptive(pa, r, w, h, n, -1)
    assert (counts == w * h).all() and w * h > _refine_slices_grid(16, w * h) * 256
    for z in range(n):
        assert np.array_equal(np.sort(lists[z]), np.arange(w * h, dtype=np.uint32)), z
        assert np.array_equal(out8[z], f[z]["rgba8"]) and np.array_equal(out32[z], _bits(f[z]["rgba32f"])), z
    assert not np.array_equal(out8[0], out8[1])


LAYER_TWO = [(s, b) for s in ("basics", "monoportal", "portal_in_portal") for b in ("unspecialised", "baked", "patterns")]


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,build", LAYER_TWO, ids=[f"{s}-{b}" for s, b in LAYER_TWO])
def test_adaptive_slices_are_the_reference_selection_of_draws_one_by_one(gpu, scene_name, build):
    """96x54, depth 12, aa 4, four slices with update() stepping between them: out_z = adaptive_frame(P_z, F_z, T) with P_z, F_z from a renderer
    without the flag drawing one by one, the counts are the reference's, and each slice is what draw_adaptive of a FLAG_REFINE renderer gives."""
    pa = gpu
    w, h, n, aa = 96, 54, 4, 4
    pixels = w * h
    animate = build != "baked"  # (a value-baked build is rebuilt by every value that moves: its slices step the time without a clip)
    _, plain = _renderer(pa, scene_name, build, 0, animate)
    p, f = _one_by_one(plain, w, h, n, aa)
    _, single = _renderer(pa, scene_name, build, pa.FLAG_REFINE, animate)
    _, r = _renderer(pa, scene_name, build, pa.FLAG_REFINE_SLICES, animate)
    frame = pa.Frame(w, h, 0, 1)
    if animate:
        assert not np.array_equal(p[0]["rgba8"], p[1]["rgba8"])
    for t in (-1, 4, 255):
        _stage_all(r, frame, n, aa)
        out8, out32, counts, lists = _draw_slices_adaptive(pa, r, w, h, n, t)
        for z in range(n):
            mask = ar.refine_mask(p[z]["rgba8"], t)
            assert int(counts[z]) == int(mask.sum()), (t, z)
            assert np.array_equal(np.sort(lists[z]), np.flatnonzero(mask).astype(np.uint32)), (t, z)
            if t == 4:
                assert 0 < counts[z] < pixels, (z, int(counts[z]))  # not vacuous
            want8 = ar.adaptive_frame(p[z]["rgba8"], f[z]["rgba8"], t)
            want32 = ar.select(mask, _bits(f[z]["rgba32f"]), _bits(p[z]["rgba32f"]))
            bad = np.argwhere((out8[z] != want8).any(axis=2) | (out32[z] != want32).any(axis=2))
            assert bad.size == 0, f"T {t} slice {z}: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}, refined there: {bool(mask[tuple(bad[0])])}"
            _enter_state(single, z, n)
            single.set_option("aa_count", aa)
            one = single.draw_adaptive(w, h, threshold=t, rgba32f=True)
            assert one["count"] == int(counts[z]) and np.array_equal(one["rgba8"], out8[z]) and np.array_equal(_bits(one["rgba32f"]), out32[z]), (t, z)
        if t == -1:
            assert all(np.array_equal(out8[z], f[z]["rgba8"]) for z in range(n))
        if t == 255:
            assert all(np.array_equal(out8[z], p[z]["rgba8"]) for z in range(n)) and not counts.any()
    # `_aa_count` 1 in every slice: a plain draw_slices, all counts 0
    _stage_all(r, frame, n, 1)
    out8, out32, counts, _ = _draw_slices_adaptive(pa, r, w, h, n, 4)
    assert not counts.any()
    import torch

    _stage_all(r, frame, n, 1)
    d8 = torch.zeros((n, h, w, 4), dtype=torch.uint8, device="cuda")
    d32 = torch.zeros((n, h, w, 4), dtype=torch.float32, device="cuda")
    r.draw_slices(frame, n, out_rgba8=d8.data_ptr(), out_rgba32f=d32.data_ptr(), slice_pixels=pixels)
    torch.cuda.synchronize()
    assert np.array_equal(out8, d8.cpu().numpy()) and np.array_equal(out32, _bits(d32.cpu().numpy()))
    assert all(np.array_equal(out8[z], p[z]["rgba8"]) for z in range(n))
    with pytest.raises(pa.PortalError, match="not all staged"):  # launching again without staging: refused
        r.draw_slices_adaptive(frame, n, d8.data_ptr(), slice_pixels=pixels)
    r.set_option("aa_count", aa)


@pytest.mark.gpu
def test_each_kind_of_adaptive_draw_hands_out_its_own_result_only(gpu):
    """basics, unspecialised, 64x36, aa 2, T = 4, two slices.  The renderer keeps ONE set of list buffers for both kinds of adaptive draw:
    after draw_slices_adaptive on a FLAG_REFINE_SLICES renderer adaptive_slices_result() hands them out and adaptive_result() refuses; after
    draw_adaptive on a FLAG_REFINE renderer it is the other way round."""
    pa = gpu
    w, h, n, aa, t = 64, 36, 2, 2, 4

    def fresh(flags):  # renderers of their own: no earlier adaptive draw of another test
        scene = pa.Scene.from_file(pa.scene_path("basics"))
        scene.init_animation(scene.animations()[0][0])
        r = pa.SceneRenderer(scene, device=0, flags=flags)
        r.set_option("render_depth", 12)
        for result in (r.adaptive_result, r.adaptive_slices_result):
            with pytest.raises(pa.PortalError):
                result()
        return r

    r = fresh(pa.FLAG_REFINE_SLICES)
    _stage_all(r, pa.Frame(w, h, 0, 1), n, aa)
    _, _, counts, _ = _draw_slices_adaptive(pa, r, w, h, n, t)  # (reads adaptive_slices_result itself)
    assert all(0 < c < w * h for c in counts), counts  # a refined edge in both slices
    lists_ptr, stride, counts_ptr = r.adaptive_slices_result()
    assert lists_ptr and counts_ptr and stride >= w * h
    with pytest.raises(pa.PortalError):
        r.adaptive_result()
    single = fresh(pa.FLAG_REFINE)
    _enter_state(single, 0, n)
    single.set_option("aa_count", aa)
    one = single.draw_adaptive(w, h, threshold=t)
    assert one["count"] == int(counts[0])
    list_ptr, count_ptr = single.adaptive_result()
    assert list_ptr and count_ptr
    with pytest.raises(pa.PortalError):
        single.adaptive_slices_result()


def _moving_state(k):
    """State k of the rebuild tests: the compiled-in `portal_rotate_angle` moves between k = 1 and k = 2, the camera with every k."""
    return (0.0 if k < 2 else 0.6), ((0.02 * k, 0.1 - 0.01 * k, -0.3), 0.9 + 0.05 * k, 1.2, 3.1 - 0.1 * k)


def _monoportal(pa, flags):
    scene = pa.Scene.from_file(pa.scene_path("monoportal"))
    r = pa.SceneRenderer(scene, device=0, flags=flags)
    r.set_option("render_depth", 12)
    return scene, r


@pytest.mark.gpu
@pytest.mark.parametrize("t", [-1, 4])
def test_a_rebuild_between_two_stage_calls_keeps_both_passes_on_the_slices_own_kernel(gpu, t):
    """A FLAG_SPECIALIZE_STATIC | FLAG_REFINE_SLICES renderer whose compiled-in value moves between slice 1 and slice 2 of 4, at 64x36: two
    runs of two slices, each with both passes on the kernel it was staged with.  The frames are the adaptive selection of the draws one
    by one (at T = -1: the aa-4 draws themselves)."""
    pa = gpu
    w, h, n, aa = 64, 36, 4, 4
    frame = pa.Frame(w, h, 0, 1)

    scene_a, ra = _monoportal(pa, 0)
    p, f = [], []
    for k in range(n):
        angle, cam = _moving_state(k)
        assert scene_a.set_uniform("portal_rotate_angle", angle)
        ra.set_camera(*cam)
        ra.set_option("aa_start", k)
        ra.set_option("aa_count", 1)
        p.append(ra.draw(w, h, rgba8=True, rgba32f=True))
        ra.set_option("aa_count", aa)
        f.append(ra.draw(w, h, rgba8=True, rgba32f=True))
    scene_b, rb = _monoportal(pa, pa.FLAG_SPECIALIZE_STATIC | pa.FLAG_REFINE_SLICES)
    rb.set_option("aa_count", aa)
    kernels = []
    for k in range(n):
        angle, cam = _moving_state(k)
        assert scene_b.set_uniform("portal_rotate_angle", angle)
        rb.set_camera(*cam)
        rb.set_option("aa_start", k)
        rb.stage_slice(frame, k)
        kernels.append(pa.lib().ptl_renderer_kernel(rb._h))
    assert kernels[0] == kernels[1] != kernels[2] == kernels[3] and rb.rejit_count() >= 1  # the value is compiled in: two kernels, two runs
    out8, out32, counts, _ = _draw_slices_adaptive(pa, rb, w, h, n, t)
    for z in range(n):
        mask = ar.refine_mask(p[z]["rgba8"], t)
        assert int(counts[z]) == int(mask.sum()) and (t == -1 or 0 < counts[z] < w * h), (z, int(counts[z]))
        assert np.array_equal(out8[z], ar.adaptive_frame(p[z]["rgba8"], f[z]["rgba8"], t)), z
        assert np.array_equal(out32[z], ar.select(mask, _bits(f[z]["rgba32f"]), _bits(p[z]["rgba32f"]))), z
    assert not np.array_equal(f[1]["rgba8"], f[2]["rgba8"])


@pytest.mark.gpu
def test_a_renderer_destroyed_with_staged_slices_a_parked_kernel_and_used_lanes_leaves_the_device_sound(gpu):
    """The teardown nothing else reaches: a FLAG_SPECIALIZE_STATIC | FLAG_REFINE_SLICES renderer at 64x36 whose lanes have drawn, with two
    slices staged and never launched and a rebuild between the two stage calls (the first slice's kernel is parked, both hold their texel
    buffers), is destroyed.  A fresh renderer of the same scene then draws the frame of a renderer that never staged anything."""
    import gc

    import torch

    pa = gpu
    w, h = 64, 36
    frame = pa.Frame(w, h, 0, 1)
    flags = pa.FLAG_SPECIALIZE_STATIC | pa.FLAG_REFINE_SLICES

    def enter(scene, r, k):
        angle, cam = _moving_state(k)
        assert scene.set_uniform("portal_rotate_angle", angle)
        r.set_camera(*cam)

    scene_a, ra = _monoportal(pa, 0)
    enter(scene_a, ra, 2)
    want = ra.draw(w, h, rgba8=True, rgba32f=True)

    scene_b, rb = _monoportal(pa, flags)
    rb.set_option("concurrent_draws", 2)
    targets = torch.zeros((2, h, w, 4), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    for j in range(2):  # lane 0 (the kernel itself) and lane 1 (its clone), not joined
        enter(scene_b, rb, 0)
        rb.draw_device(frame, out_rgba8=targets[j].data_ptr())
    kernels = []
    for j, k in enumerate((1, 2)):
        enter(scene_b, rb, k)
        rb.stage_slice(frame, j)
        kernels.append(pa.lib().ptl_renderer_kernel(rb._h))
    assert kernels[0] != kernels[1] and rb.rejit_count() >= 1  # slice 0's kernel is parked
    del rb, scene_b
    gc.collect()
    torch.cuda.synchronize()

    scene_c, rc = _monoportal(pa, flags)
    enter(scene_c, rc, 2)
    got = rc.draw(w, h, rgba8=True, rgba32f=True)
    assert np.array_equal(got["rgba8"], want["rgba8"])
    assert np.array_equal(_bits(got["rgba32f"]), _bits(want["rgba32f"]))


@pytest.mark.gpu
def test_adaptive_slices_read_the_video_frame_that_was_bound_when_they_were_staged(gpu, tmp_path):
    """The scene of test_gpu_round2.py's video test: a video texture steps twice inside a batch of six slices.  The adaptive batch has two
    tracing launches; the texel buffers retired while the slices were staged live until behind the SECOND (T = -1: every pixel is shaded
    again by the refine pass), so every slice shows its own video frame -- in two batches in a row."""
    import torch
    from tests import synthetic

    pa = gpu
    colours = [(255, 0, 0), (0, 255, 0), (0, 0, 255)]
    frames_dir = tmp_path / "video_png" / "clip"
    frames_dir.mkdir(parents=True)
    for k, c in enumerate(colours):
        img = np.zeros((4, 4, 4), np.uint8)
        img[..., :3] = c
        img[..., 3] = 255
        pa.png_write(str(frames_dir / f"frame_{k:03d}.png"), img)
    mat = '(name: "screen", data: Complex(code: (("MaterialProcessing result = material_simple(hit, r, vec3(1.0, 1.0, 1.0), 0.0, false, 1.0, 0.0);\\nresult.mul_to_color *= texture(vid_tex, vec2(0.5, 0.5)).rgb;\\nreturn result;")))),'
    text = synthetic.wall_scene(extra_materials=mat).replace("return wall_M; }", "return screen_M; }")
    text = text.replace('uniforms: ([', 'uniforms: ([ (name: "pos", data: Formula(("time"))),')
    text = text.replace("    textures: ([]),", '    textures: ([]),\n    videos: ([ (name: "vid", data: (path: "somewhere/clip.mov", uniform: Some(Named("pos")))) ]),')
    times = (0.1, 0.2, 0.3, 0.7, 0.8, 1.0)  # frames 0 0 1 1 2 2: two boundaries inside one batch
    w, h, aa = 16, 16, 2
    frame = pa.Frame(w, h, 0, 1)
    one = pa.SceneRenderer(pa.Scene.from_text(text), device=0, asset_root=str(tmp_path))
    one.set_option("aa_count", aa)
    want = []
    for t in times:
        one.update(t)
        want.append(one.draw(w, h)["rgba8"].copy())
    assert [tuple(int(x) for x in f[8, 8][:3]) for f in want] == [colours[k] for k in (0, 0, 1, 1, 2, 2)]
    r = pa.SceneRenderer(pa.Scene.from_text(text), device=0, asset_root=str(tmp_path), flags=pa.FLAG_REFINE_SLICES)
    r.set_option("aa_count", aa)
    r.set_option("adaptive_aa_threshold", -1)
    out = torch.zeros((len(times), h, w, 4), dtype=torch.uint8, device="cuda:0")
    for rounds in range(2):
        for j, t in enumerate(times):
            r.update(t)
            r.stage_slice(frame, j)
        r.draw_slices_adaptive(frame, len(times), out.data_ptr(), slice_pixels=w * h)
        got = out.cpu().numpy()
        for j in range(len(times)):
            assert np.array_equal(got[j], want[j]), (rounds, j)
        _, _, counts_ptr = r.adaptive_slices_result()
        assert (pa.device_download(counts_ptr, 4 * len(times)).view(np.uint32) == w * h).all()


# ---- `portal-amd render --clip-adaptive-aa`, end to end (the harness of tests/test_render_cli_forms.py) -----------------------------
W, H = 64, 36
CLIP = "anim.4.portals"  # 3 s: six frames at --fps 2


def _path_without_ffmpeg():
    return os.pathsep.join(d for d in os.environ.get("PATH", "").split(os.pathsep) if d and not os.path.exists(os.path.join(d, "ffmpeg")))


def _render(pa, out_dir, extra, aa=2):
    scene = pa.scene_path("basics")
    cmd = [_exe(pa), "render", scene, CLIP, "--width", str(W), "--height", str(H), "--aa-count", str(aa), "--render-depth", "12", "--fps", "2", "--out-dir", str(out_dir),
           "--asset-root", os.path.dirname(os.path.dirname(scene))] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, PATH=_path_without_ffmpeg()))
    assert out.returncode == 0, out.stderr + out.stdout
    return out


def _clip_files(out_dir, count=6):
    """Every file a PNG clip leaves behind, as bytes: the parked frames and both stills."""
    video = out_dir / "video" / "basics"
    assert sorted(os.listdir(video / f"{CLIP}.frames")) == sorted(f"frame_{i}.png" for i in range(count))
    files = {f"frame_{i}.png": (video / f"{CLIP}.frames" / f"frame_{i}.png").read_bytes() for i in range(count)}
    for still in ("start", "end"):
        files[still] = (video / f"{CLIP}.{still}.png").read_bytes()
    return files


def _same_files(got, want):
    assert sorted(got) == sorted(want)
    for name in got:
        assert got[name] == want[name], name


@pytest.mark.gpu
@pytest.mark.parametrize("blur", [3, 1, 17])
def test_cli_threshold_minus_one_changes_no_png_byte(gpu, tmp_path, blur):
    """T = -1 refines every pixel: the clip is the plain one, byte for byte -- batched (blur 3: the refine entry over slices) and unbatched
    (blur 1 and 17: ptl_renderer_draw_adaptive per sub-frame)."""
    _render(gpu, tmp_path / "plain", ["--motion-blur-frames", str(blur)])
    _render(gpu, tmp_path / "adaptive", ["--motion-blur-frames", str(blur), "--clip-adaptive-aa", "-1"])
    _same_files(_clip_files(tmp_path / "adaptive"), _clip_files(tmp_path / "plain"))


@pytest.mark.gpu
def test_cli_threshold_255_is_the_one_sample_clip(gpu, tmp_path):
    _render(gpu, tmp_path / "one", ["--motion-blur-frames", "3"], aa=1)
    _render(gpu, tmp_path / "adaptive", ["--motion-blur-frames", "3", "--clip-adaptive-aa", "255"])
    _same_files(_clip_files(tmp_path / "adaptive"), _clip_files(tmp_path / "one"))


@pytest.mark.gpu
def test_cli_threshold_minus_one_changes_no_stream_byte(gpu, tmp_path):
    _render(gpu, tmp_path / "plain", ["--motion-blur-frames", "3", "--frames", "y4m"])
    _render(gpu, tmp_path / "adaptive", ["--motion-blur-frames", "3", "--frames", "y4m", "--clip-adaptive-aa", "-1"])
    stream = (tmp_path / "adaptive" / "video" / "basics" / f"{CLIP}.y4m").read_bytes()
    assert stream == (tmp_path / "plain" / "video" / "basics" / f"{CLIP}.y4m").read_bytes() and len(stream) > 6 * gpu.yuv420p10_frame_bytes(W, H)


@pytest.mark.gpu
def test_cli_adaptive_clip_is_the_python_mirrors(gpu, tmp_path):
    """T = 4 with --timing: frames and stills are draw_adaptive per sub-frame on a FLAG_REFINE renderer, averaged by the oracle; the report
    has the adaptive line, with the refined entries the mirror counted."""
    from oracle import postprocess as pp

    pa = gpu
    blur = 3
    done = _render(pa, tmp_path, ["--motion-blur-frames", str(blur), "--clip-adaptive-aa", "4", "--timing"])
    scene = pa.Scene.from_file(pa.scene_path("basics"))
    r = pa.SceneRenderer(scene, device=0, flags=pa.FLAG_REFINE)
    r.set_option("aa_count", 2)
    r.set_option("render_depth", 12)
    duration = dict(scene.animations())[CLIP]
    count = max(1, int(np.float32(duration) * np.float32(2)))
    assert count == 6
    scene.init_animation(CLIP)
    r.update(0.0)
    frames, first, last, refined = [], None, None, 0
    for i in range(count):
        subs = []
        for j in range(blur):
            r.set_option("aa_start", j)
            r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
            out = r.draw_adaptive(W, H, threshold=4)
            assert 0 < out["count"] < W * H
            refined += out["count"]
            subs.append(out["rgba8"])
        first = subs[0] if first is None else first
        last = subs[-1]
        frames.append(pp.average_images(subs))
    video = tmp_path / "video" / "basics"
    assert sorted(os.listdir(video / f"{CLIP}.frames")) == sorted(f"frame_{i}.png" for i in range(count))
    for i, want in enumerate(frames):
        assert np.array_equal(pa.png_read(str(video / f"{CLIP}.frames" / f"frame_{i}.png")), want), i
    assert np.array_equal(pa.png_read(str(video / f"{CLIP}.start.png")), first) and np.array_equal(pa.png_read(str(video / f"{CLIP}.end.png")), last)
    lines = [line for line in done.stdout.splitlines() if line.startswith("adaptive aa:")]
    assert len(lines) == 1, done.stdout
    m = re.match(r"adaptive aa: threshold 4, (\d+) of (\d+) pixels refined \([\d.]+ %\); GPU ms: one-sample pass ([\d.]+), classification ([\d.]+), refine pass ([\d.]+)$", lines[0])
    assert m, lines[0]
    assert int(m.group(2)) == count * blur * W * H and int(m.group(1)) == refined <= int(m.group(2))
    assert all(float(m.group(k)) > 0 for k in (3, 4, 5))
