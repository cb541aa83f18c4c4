"""Adaptive anti-aliasing (`render-frame --adaptive-aa`): the classification kernel (portal_amd/csrc/kernels/aa_edges.hip),
the refine entry of kernels generated with FLAG_REFINE, the C ABI of both layers, the Python mirror and the CLI, against
tests/adaptive_reference.py (a numpy restatement of the contract).  Every comparison is equality."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from tests import adaptive_reference as ar
from tests.adaptive_reference import bits as _bits, cuda_words as _cuda_words, exe as _exe, resource_usage as _resource_usage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
INVALID = -1  # PTL_ERR_INVALID


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def _flat(h, w, value=(90, 120, 200, 255)):
    return np.tile(np.array(value, np.uint8), (h, w, 1))


def test_reference_helper_on_hand_made_frames():
    """Pins the fixture, not the product."""
    for t in (-1, 0, 4, 255):
        assert ar.refined_indices(_flat(5, 7), t).size == (35 if t == -1 else 0)  # a flat frame: d = 0 everywhere, only T = -1 is below it
    p = _flat(5, 5)
    p[2, 2, 1] += 1  # one odd pixel in the middle: it and its eight neighbours see a difference of 1
    want = sorted(y * 5 + x for y in (1, 2, 3) for x in (1, 2, 3))
    assert ar.refined_indices(p, 0).tolist() == want
    assert ar.refined_indices(p, 1).size == 0
    p = _flat(5, 5)
    p[0, 0, 2] -= 3  # ... in a corner: coordinates clamp, so 4 pixels
    assert ar.refined_indices(p, 0).tolist() == [0, 1, 5, 6]
    p = _flat(5, 5)
    p[4, 4, 0] = 0
    assert ar.refined_indices(p, 89).tolist() == [18, 19, 23, 24] and ar.refined_indices(p, 90).size == 0
    for t in (0, 7, 100, 254):  # d == T is not refined, d == T + 1 is
        p = _flat(3, 9, (0, 0, 0, 255))
        p[1, 2, 0] = t       # d = T around column 2
        p[1, 6, 2] = t + 1   # d = T + 1 around column 6
        mask = ar.refine_mask(p, t)
        assert not mask[:, :4].any() and mask[:, 5:8].all() and not mask[:, 8].any() and not mask[:, 4].any()
        assert ar.distance(p)[1, 2] == t and ar.distance(p)[1, 6] == t + 1
    p = _flat(4, 4)
    p[1, 1, 3] = 0  # a difference in alpha alone
    assert ar.refined_indices(p, 0).size == 0 and ar.distance(p).max() == 0
    # out = refine ? F : P, on any payload
    p, f = _flat(3, 3), _flat(3, 3, (1, 2, 3, 4))
    p[0, 0, 0] = 0
    out = ar.adaptive_frame(p, f, 4)
    assert np.array_equal(out[:2, :2], f[:2, :2]) and np.array_equal(out[2], p[2]) and np.array_equal(out[:, 2], p[:, 2])


def _refine_kernel(pa, scene="basics", flags=None):
    s = pa.Scene.from_file(pa.scene_path(scene))
    r = pa.SceneRenderer(s, device=-1, flags=pa.FLAG_REFINE if flags is None else flags)
    return s, r


def test_layer_one_validates_before_any_gpu_call(pa):
    """This machine has no GPU to ask: every refusal below comes from the argument checks (PTL_ERR_INVALID)."""
    L = pa.lib()
    frame, lst, cnt = C.c_void_p(1 << 20), C.c_void_p(2 << 20), C.c_void_p(3 << 20)
    edges = lambda *a: L.ptl_aa_edges(0, *a, None, None)  # noqa: E731
    assert edges(None, 8, 8, 4, lst, cnt) == INVALID
    assert edges(frame, 8, 8, 4, None, cnt) == INVALID
    assert edges(frame, 8, 8, 4, lst, None) == INVALID
    for w, h in ((0, 8), (8, 0), (-3, 8), (8, -1)):
        assert edges(frame, w, h, 4, lst, cnt) == INVALID
    assert edges(frame, 1 << 16, (1 << 15) + 1, 4, lst, cnt) == INVALID  # beyond 2^31 pixels
    assert edges(frame, 8, 8, -2, lst, cnt) == INVALID and edges(frame, 8, 8, 256, lst, cnt) == INVALID
    assert edges(C.c_void_p((1 << 20) + 2), 8, 8, 4, lst, cnt) == INVALID  # a pixel is a 32-bit word

    scene, r = _refine_kernel(pa)
    k = L.ptl_renderer_kernel(r._h)
    refine = lambda kernel, f, a, b: L.ptl_kernel_render_refine(kernel, C.byref(f) if f is not None else None, a, b, frame, None, None, None, None)  # noqa: E731
    whole = pa.Frame(8, 8, 0, 1, 0)
    assert refine(None, whole, lst, cnt) == INVALID
    assert refine(k, None, lst, cnt) == INVALID
    assert refine(k, whole, None, cnt) == INVALID and refine(k, whole, lst, None) == INVALID
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        assert refine(k, pa.Frame(w, h, 0, 1, 0), lst, cnt) == INVALID
    assert refine(k, pa.Frame(1 << 16, (1 << 15) + 1, 0, 1, 0), lst, cnt) == INVALID
    assert refine(k, pa.Frame(8, 64, 0, 2, 0), lst, cnt) == INVALID  # sharded
    assert refine(k, pa.Frame(8, 64, 1, 2, 0), lst, cnt) == INVALID
    assert refine(k, pa.Frame(8, 8, 0, 1, 1), lst, cnt) == INVALID  # in place
    _, plain = _refine_kernel(pa, flags=0)
    assert refine(L.ptl_renderer_kernel(plain._h), whole, lst, cnt) == INVALID  # a kernel without the refine entry
    assert "PTL_FLAG_REFINE" in pa.last_error()
    assert refine(k, whole, lst, cnt) == -6  # everything valid: only now the missing device is noticed (PTL_ERR_NO_DEVICE)


def test_layer_two_validates_before_any_gpu_call(pa):
    L = pa.lib()
    out = C.c_void_p(1 << 20)
    _, r = _refine_kernel(pa)
    draw = lambda rr, f, o: L.ptl_renderer_draw_adaptive(rr, C.byref(f) if f is not None else None, o, None, None, None)  # noqa: E731
    whole = pa.Frame(8, 8, 0, 1, 0)
    assert draw(None, whole, out) == INVALID and draw(r._h, None, out) == INVALID
    assert draw(r._h, whole, None) == INVALID  # the classification reads the RGBA8 output: it is required
    for w, h in ((0, 8), (8, 0), (-1, 8)):
        assert draw(r._h, pa.Frame(w, h, 0, 1, 0), out) == INVALID
    assert draw(r._h, pa.Frame(1 << 16, (1 << 15) + 1, 0, 1, 0), out) == INVALID
    assert draw(r._h, pa.Frame(8, 64, 0, 2, 0), out) == INVALID and draw(r._h, pa.Frame(8, 64, 1, 2, 0), out) == INVALID
    assert draw(r._h, pa.Frame(8, 8, 0, 1, 1), out) == INVALID
    for t in (-2, 256):
        r.set_option("adaptive_aa_threshold", t)
        assert draw(r._h, whole, out) == INVALID and "adaptive_aa_threshold" in pa.last_error()
    r.set_option("adaptive_aa_threshold", 4)
    _, plain = _refine_kernel(pa, flags=0)
    assert draw(plain._h, whole, out) == INVALID and "PTL_FLAG_REFINE" in pa.last_error()  # a renderer without the flag
    assert draw(r._h, whole, out) == -6  # PTL_ERR_NO_DEVICE: the arguments were fine
    assert L.ptl_renderer_adaptive_result(r._h, None, None) == INVALID  # no adaptive draw yet
    with pytest.raises(pa.PortalError):  # the refine entry reads the module's own uniform block, a slices module's draws do not fill it
        pa.SceneRenderer(pa.Scene.from_file(pa.scene_path("basics")), device=-1, flags=pa.FLAG_REFINE | pa.FLAG_SLICES)


def test_make_kernels_builds_aa_edges_without_scratch(pa, tmp_path):
    subprocess.run(["make", "kernels"], cwd=ROOT, check=True, capture_output=True)
    assert os.path.getsize(os.path.join(ROOT, "portal_amd", "kernels", "aa_edges.hsaco")) > 1000
    src = os.path.join(ROOT, "portal_amd", "csrc", "kernels", "aa_edges.hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-vgpr-regalloc=basic", "--genco", "--no-gpu-bundle-output",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / "aa_edges.hsaco")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    usage = _resource_usage(out.stderr)
    print(usage)
    assert set(usage) == {"ptl_aa_edges_kernel"}
    for entry, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0, (entry, u)
        assert u["VGPRs"] <= 64 and u["LDS Size [bytes/block]"] <= 16384, (entry, u)  # eight waves per SIMD, four workgroups per CU


@pytest.mark.parametrize("scene_name", ["basics", "monoportal", "portal_in_portal", "triple_portal", "mobius_monoportal"])
def test_source_without_the_flag_has_no_trace_of_the_refine_entry(pa, scene_name):
    for flags in (0, pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL, pa.FLAG_SPECIALIZE_PATTERNS, pa.FLAG_SLICES, pa.FLAG_COUNT_SEGMENTS):
        scene = pa.Scene.from_file(pa.scene_path(scene_name))
        src = scene.generate_source(flags)
        assert "ptl_render_refine_kernel" not in src and "REFINE" not in src and "refine_entry" not in src
        with_flag = scene.generate_source(flags | pa.FLAG_REFINE) if not flags & pa.FLAG_SLICES else None
        if with_flag is not None:  # ... and the flag adds the entry's text and changes nothing else
            entry = pa.device_source("refine_entry")
            assert with_flag.count("ptl_render_refine_kernel(") == 1 and with_flag.replace(entry, "") == src


BAKED = lambda pa: pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL  # noqa: E731


@pytest.mark.parametrize("build", ["unspecialised", "baked"])
@pytest.mark.parametrize("scene_name", ["basics", "monoportal", "portal_in_portal"])
def test_source_with_the_flag_compiles_for_gfx950_without_scratch(pa, scene_name, build):
    scene = pa.Scene.from_file(pa.scene_path(scene_name))
    r = pa.SceneRenderer(scene, device=-1, flags=pa.FLAG_REFINE | (BAKED(pa) if build == "baked" else 0))
    assert "ptl_render_refine_kernel(" in r.kernel_source()
    code = r.code_object()
    assert b"ptl_render_refine_kernel" in code and b"ptl_render_kernel" in code
    note = lambda key, entry: pa.lib().ptl_code_object_note(code, len(code), key.encode(), entry.encode())  # noqa: E731
    render = {k: note(k, "ptl_render_kernel") for k in (".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".vgpr_spill_count")}
    refine = {k: note(k, "ptl_render_refine_kernel") for k in render}
    print(f"{scene_name} {build}: render entry {render}, refine entry {refine}")
    assert refine[".private_segment_fixed_size"] == 0 and refine[".vgpr_spill_count"] == 0
    assert render[".private_segment_fixed_size"] == 0
    assert 0 < refine[".vgpr_count"] <= 128  # (the render entry's launch bounds: 256 threads)


@pytest.mark.parametrize("cmd,extra,reason", [("render-frame", ["--adaptive-aa", "-2"], "-1 .. 255"), ("render-frame", ["--adaptive-aa", "256"], "-1 .. 255"),
                                              ("render-frame", ["--adaptive-aa", "4", "--gpus", "2"], "one GPU"), ("render-frame", ["--gpus", "3", "--adaptive-aa"], "one GPU"),
                                              ("render", ["--adaptive-aa"], "render-frame"), ("render", ["--adaptive-aa", "8"], "render-frame")])
def test_cli_refuses_while_the_arguments_are_parsed(pa, tmp_path, cmd, extra, reason):
    """Exit status 2, one line of reason, nothing written (this machine has no GPU to ask)."""
    target = ["--output", str(tmp_path / "f.png")] if cmd == "render-frame" else ["--out-dir", str(tmp_path)]
    out = subprocess.run([_exe(pa), cmd, pa.scene_path("basics")] + target + extra, capture_output=True, text=True, timeout=120)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


SIZES = [(1, 1), (3, 1), (7, 5), (8, 8), (9, 9), (33, 17), (64, 36), (257, 3), (640, 360)]
THRESHOLDS = [-1, 0, 7, 254, 255]


def _synthetic(kind, w, h, t, rng):
    """Seeded frames: noise of amplitude about T (roughly half the pixels flag), a few straight edges on a flat ground with steps of
    exactly T and T + 1, every pixel different.  Alpha is random throughout: it must not matter."""
    p = np.empty((h, w, 4), np.uint8)
    p[:, :, 3] = rng.integers(0, 256, (h, w))
    if kind == "noise":
        amp = min(255, max(t, 0) + max(1, t // 4))  # a little above T: the largest of the 24 neighbour differences exceeds T for a third to a half of the pixels at the middle thresholds
        p[:, :, :3] = rng.integers(0, amp + 1, (h, w, 3))
    elif kind == "edges":
        step = min(max(t, 0), 254)
        p[:, :, :3] = 0
        p[h // 2:, :, 0] += step + 1           # a horizontal edge that flags (d = T + 1) ...
        p[:, (2 * w) // 3:, 1] += step         # ... a vertical one that does not (d = T) ...
        ys, xs = np.mgrid[0:h, 0:w]
        p[:, :, 2][xs * h > ys * w] += step + 1  # ... and a diagonal
    else:  # every pixel differs from each of its neighbours
        i = np.arange(w * h, dtype=np.int64).reshape(h, w)
        p[:, :, 0], p[:, :, 1], p[:, :, 2] = i & 255, (i >> 8) & 255, (i * 37 >> 3) & 255
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_classification_kernel_lists_exactly_the_reference_mask(gpu, w, h):
    import torch

    pa = gpu
    rng = np.random.default_rng(1000 * w + h)
    stream = torch.cuda.current_stream().cuda_stream
    lst = torch.from_numpy(np.full(w * h + 16, 0xDEADBEEF, np.uint32).view(np.int32)).cuda()  # 16 guard words behind the list's capacity
    cnt = torch.full((4,), 12345, dtype=torch.int32, device="cuda")                             # a stale count: the call resets it itself
    seen = set()
    for kind in ("noise", "edges", "different"):
        for t in THRESHOLDS:
            p = _synthetic(kind, w, h, t, rng)
            want = ar.refined_indices(p, t)
            dev = torch.from_numpy(p).cuda()
            sets = []
            for _ in range(2):  # twice on the same buffers: the reset works, the set is the same
                pa.aa_edges_device(dev.data_ptr(), w, h, t, lst.data_ptr(), cnt.data_ptr(), stream=stream)
                torch.cuda.synchronize()
                count = int(cnt[0].item()) & 0xFFFFFFFF
                got = np.sort(lst[:count].cpu().numpy().view(np.uint32))
                sets.append(got)
                assert count == want.size, (kind, t, count, want.size)
                assert np.array_equal(got, want), (kind, t)  # sorted and equal: unique and in range as well
            assert np.array_equal(sets[0], sets[1])
            assert (cnt[1:].cpu().numpy() == 12345).all() and (lst[w * h:].cpu().numpy().view(np.uint32) == 0xDEADBEEF).all()
            seen.add((kind, t, want.size == 0, want.size == w * h))
            if t == -1:
                assert want.size == w * h
            if t == 255:
                assert want.size == 0
    if w * h >= 64:  # the inputs are not vacuous: the middle thresholds flag a part of the frame
        assert any(not empty and not full for (_, t, empty, full) in seen if t in (0, 7)), seen


DRAW_CASES = [("basics", "baked"), ("monoportal", "baked"), ("portal_in_portal", "baked"), ("basics", "unspecialised"), ("monoportal", "unspecialised"),
              ("monoportal", "patterns")]
_renderers = {}


def _renderer(pa, scene_name, build, options=None, extra_flags=0):
    """One renderer per (scene, build): P, F and every adaptive frame come from the same one."""
    key = (scene_name, build, tuple(sorted((options or {}).items())), extra_flags)
    if key not in _renderers:
        flags = pa.FLAG_REFINE | extra_flags | {"baked": BAKED(pa), "unspecialised": 0, "patterns": pa.FLAG_SPECIALIZE_PATTERNS}[build]
        r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path(scene_name)), device=0, flags=flags, options=options)
        r.set_option("render_depth", 12)
        _renderers[key] = r
    return _renderers[key]


def _plain_and_full(r, w, h):
    r.set_option("aa_count", 1)
    p = r.draw(w, h, rgba8=True, rgba32f=True)
    r.set_option("aa_count", 4)
    f = r.draw(w, h, rgba8=True, rgba32f=True)
    return p, f


def _check_adaptive(r, w, h, t, p, f, vacuity):
    rejits = r.rejit_count()
    out = r.draw_adaptive(w, h, threshold=t, rgba32f=True)
    assert r.rejit_count() == rejits
    mask = ar.refine_mask(p["rgba8"], t)
    assert out["count"] == int(mask.sum())
    assert np.array_equal(np.sort(out["list"]), np.flatnonzero(mask).astype(np.uint32))
    differs = (f["rgba8"] != p["rgba8"]).any(axis=2)
    stats = dict(t=t, count=out["count"], pixels=w * h, refined_and_different=int((mask & differs).sum()), unrefined_and_different=int((~mask & differs).sum()))
    print(stats)
    if vacuity:  # writing nothing in the refine pass, or writing everywhere, must not pass
        assert 0 < out["count"] < w * h, stats
        assert stats["refined_and_different"] >= 100 and stats["unrefined_and_different"] >= 100, stats
    want8 = ar.select(mask, f["rgba8"], p["rgba8"])
    want32 = ar.select(mask, _bits(f["rgba32f"]), _bits(p["rgba32f"]))
    bad = np.argwhere((out["rgba8"] != want8).any(axis=2) | (_bits(out["rgba32f"]) != want32).any(axis=2))
    assert bad.size == 0, f"{len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}, refined there: {bool(mask[tuple(bad[0])])}"
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(64, 36), (70, 37)], ids=["64x36", "70x37"])
@pytest.mark.parametrize("scene_name,build", DRAW_CASES, ids=[f"{s}-{b}" for s, b in DRAW_CASES])
def test_adaptive_draw_is_the_reference_selection_of_the_two_plain_draws(gpu, scene_name, build, w, h):
    r = _renderer(gpu, scene_name, build)
    p, f = _plain_and_full(r, w, h)
    assert not np.array_equal(p["rgba8"], f["rgba8"])
    for t in (4, 8):
        _check_adaptive(r, w, h, t, p, f, vacuity=True)
    everything = _check_adaptive(r, w, h, -1, p, f, vacuity=False)
    assert everything["count"] == w * h and np.array_equal(everything["rgba8"], f["rgba8"]) and np.array_equal(_bits(everything["rgba32f"]), _bits(f["rgba32f"]))
    nothing = _check_adaptive(r, w, h, 255, p, f, vacuity=False)
    assert nothing["count"] == 0 and np.array_equal(nothing["rgba8"], p["rgba8"]) and np.array_equal(_bits(nothing["rgba32f"]), _bits(p["rgba32f"]))
    r.set_option("aa_count", 1)  # N = 1: a plain draw, an empty list
    rejits = r.rejit_count()
    one = r.draw_adaptive(w, h, threshold=4, rgba32f=True)
    assert r.rejit_count() == rejits
    assert one["count"] == 0 and one["list"].size == 0
    assert np.array_equal(one["rgba8"], p["rgba8"]) and np.array_equal(_bits(one["rgba32f"]), _bits(p["rgba32f"]))
    # ... and the plain draw path is what it was: F again, after all of the above
    r.set_option("aa_count", 4)
    again = r.draw(w, h, rgba8=True, rgba32f=True)
    assert np.array_equal(again["rgba8"], f["rgba8"]) and np.array_equal(_bits(again["rgba32f"]), _bits(f["rgba32f"]))


@pytest.mark.gpu
def test_adaptive_draw_with_both_eyes_in_one_wave(gpu):
    """Side by side at 64x36: an eye is 32 pixels wide, so the refined list mixes both eyes within one wave."""
    w, h = 64, 36
    r = _renderer(gpu, "monoportal", "baked", options={"draw_side_by_side": 1})
    p, f = _plain_and_full(r, w, h)
    for t in (4, 8):
        out = _check_adaptive(r, w, h, t, p, f, vacuity=False)
        assert 0 < out["count"] < w * h
        xs = np.sort(out["list"])[:] % w
        assert (xs < w // 2).any() and (xs >= w // 2).any()  # both eyes are on the list
        # ... and within one wave: a wave of the refine pass shades the 64 consecutive entries [64 c, 64 c + 64).  The list's order is free (which
        # region comes first is the atomic's business), so the mixed wave is looked for, not expected at the front.
        left = np.array([(out["list"][c:c + 64] % w < w // 2).any() for c in range(0, out["count"], 64)])
        right = np.array([(out["list"][c:c + 64] % w >= w // 2).any() for c in range(0, out["count"], 64)])
        assert (left & right).any(), "no wave of the refine pass holds pixels of both eyes"


# ---- the refine entry through layer 1: lists the caller made ---------------------------------------
def _refine_grid_cap():
    """`std::min<long long>(chunks, 2048 / n)` of the refine launcher behind ptl_kernel_render_refine (portal_amd/csrc/host/kernel.cpp), which has
    n = 1: the workgroups of a refine launch at most, 256 entries each and trip.  Read from the source, so a changed cap fails the second-trip
    test instead of leaving it vacuous."""
    src = open(os.path.join(ROOT, "portal_amd", "csrc", "host", "kernel.cpp")).read()
    m = re.findall(r"const unsigned gx = \(unsigned\)std::min<long long>\(chunks, (\d+) / n\);", src)
    assert len(m) == 1, "the refine launcher no longer spells its grid as min(chunks, N / n)"
    assert "return launch_refine(k, false, frame, 1, list, 0, count," in src, "ptl_kernel_render_refine no longer launches with n = 1"
    return int(m[0])


def test_refine_grid_cap_is_what_the_second_trip_test_crosses():
    assert _refine_grid_cap() == 2048
    assert 1024 * 513 == 525312 > 2048 * 256 == 524288 and (1024 * 513 + 255) // 256 > 2048


GUARD_PIXELS = 16  # behind both outputs: entry W*H, if it were not skipped, would land on the first of them


def _refine_through_layer_one(pa, r, w, h, entries, count, start8=None, start32=None, segments=False):
    """ptl_kernel_render_refine on `entries` (uint32, all uploaded) with *count = `count`, over device copies of the given start frames (None: that
    output is null).  -> (rgba8 or None, rgba32f bits or None, segment count or None); the guard pixels behind the outputs and the words
    behind the count must survive."""
    import torch

    lst = _cuda_words(np.concatenate([entries.astype(np.uint32), np.full(4, 0xDEADBEEF, np.uint32)]))
    cnt = _cuda_words(np.array([count, 0x5A5A5A5A, 0x5A5A5A5A, 0x5A5A5A5A], np.uint32))
    d8 = _cuda_words(np.concatenate([_bits(start8).reshape(-1), np.full(GUARD_PIXELS, 0xA5A5A5A5, np.uint32)])) if start8 is not None else None
    d32 = _cuda_words(np.concatenate([_bits(start32).reshape(-1), np.full(4 * GUARD_PIXELS, 0xA5A5A5A5, np.uint32)])) if start32 is not None else None
    seg = torch.zeros(2, dtype=torch.int64, device="cuda") if segments else None
    r.refine_device(pa.Frame(w, h, 0, 1, 0), lst.data_ptr(), cnt.data_ptr(), out_rgba8=d8.data_ptr() if d8 is not None else 0,
                    out_rgba32f=d32.data_ptr() if d32 is not None else 0, segments=seg.data_ptr() if segments else 0,
                    stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(lst.cpu().numpy().view(np.uint32)[:-4], entries) and np.array_equal(cnt.cpu().numpy().view(np.uint32)[1:], [0x5A5A5A5A] * 3)
    out8 = out32 = None
    if d8 is not None:
        words = d8.cpu().numpy().view(np.uint32)
        assert (words[w * h:] == 0xA5A5A5A5).all(), "RGBA8 written behind the frame"
        out8 = words[: w * h].view(np.uint8).reshape(h, w, 4)
    if d32 is not None:
        words = d32.cpu().numpy().view(np.uint32)
        assert (words[4 * w * h:] == 0xA5A5A5A5).all(), "RGBA32F written behind the frame"
        out32 = words[: 4 * w * h].reshape(h, w, 4)
    if segments:
        assert int(seg[1].item()) == 0
    return out8, out32, int(seg[0].item()) if segments else None


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,build", [("basics", "baked"), ("monoportal", "unspecialised")], ids=["basics-baked", "monoportal-unspecialised"])
def test_refine_entry_shades_exactly_the_callers_list(gpu, scene_name, build):
    """ptl_kernel_render_refine with lists no classification kernel wrote, at 70x37 over device copies of P: duplicates, entries outside the
    frame (W*H and 0xFFFFFFFF: skipped, as device/ptl_refine_entry.h promises), a count below the buffer's length, a count of 0, one
    output null.  The result is where(listed, F, P) in bytes and float bits.  The full list is 3 885 entries for a grid of 11
    workgroups: the stride loop takes a second trip here as well."""
    pa = gpu
    w, h = 70, 37
    pixels = w * h
    r = _renderer(pa, scene_name, build)
    p, f = _plain_and_full(r, w, h)  # F last: the kernel's `_aa_count` is 4, its resolution 70x37
    p8, f8, p32, f32 = p["rgba8"], f["rgba8"], _bits(p["rgba32f"]), _bits(f["rgba32f"])
    differs = (f8 != p8).any(axis=2) | (f32 != p32).any(axis=2)
    rng = np.random.default_rng(7037)
    half = rng.permutation(pixels)[: pixels // 2].astype(np.uint32)
    body = rng.permutation(np.concatenate([half, half]))  # a shuffled half of the pixels, each of them twice
    outside = np.where(np.arange(body.size // 2) % 2 == 0, pixels, 0xFFFFFFFF).astype(np.uint32)
    entries = np.stack([body[0::2], body[1::2], outside], axis=1).reshape(-1)  # every third entry names no pixel
    assert entries.size == 3885 > ((pixels + 255) // 256) * 256 and (entries == pixels).sum() > 600 and (entries == 0xFFFFFFFF).sum() > 600
    assert np.array_equal(np.unique(entries[entries < pixels]), np.sort(half)) and (np.bincount(entries[entries < pixels], minlength=pixels).max() == 2)

    def expect(count):
        named = entries[:count]
        listed = np.zeros(pixels, bool)
        listed[named[named < pixels]] = True
        listed = listed.reshape(h, w)
        return listed, ar.select(listed, f8, p8), ar.select(listed, f32, p32)

    for count in (entries.size, entries.size // 2, 0):
        listed, want8, want32 = expect(count)
        stats = dict(count=count, listed=int(listed.sum()), listed_and_different=int((listed & differs).sum()), unlisted_and_different=int((~listed & differs).sum()))
        print(stats)
        if count:  # shading nothing, or everything, must not pass
            assert stats["listed_and_different"] >= 10 and stats["unlisted_and_different"] >= 10, stats
            assert (entries[:count] >= pixels).any()
        else:
            assert not listed.any()
        if count == entries.size // 2:  # some pixel that differs is named only beyond the count: it stays P
            all_listed = expect(entries.size)[0]
            assert (all_listed & ~listed & differs).sum() >= 5
        out8, out32, _ = _refine_through_layer_one(pa, r, w, h, entries, count, start8=p8, start32=p32)
        bad = np.argwhere((out8 != want8).any(axis=2) | (out32 != want32).any(axis=2))
        assert bad.size == 0, f"count {count}: {len(bad)} pixels differ, first (y, x) = {bad[0].tolist()}, listed there: {bool(listed[tuple(bad[0])])}"
    listed, want8, want32 = expect(entries.size)
    out8, out32, _ = _refine_through_layer_one(pa, r, w, h, entries, entries.size, start8=p8)  # RGBA8 only
    assert out32 is None and np.array_equal(out8, want8)
    out8, out32, _ = _refine_through_layer_one(pa, r, w, h, entries, entries.size, start32=p32)  # float only
    assert out8 is None and np.array_equal(out32, want32)
    again = r.draw(w, h, rgba8=True, rgba32f=True)  # the plain draw path is what it was
    assert np.array_equal(again["rgba8"], f8) and np.array_equal(_bits(again["rgba32f"]), f32)


@pytest.mark.gpu
def test_refine_entry_takes_a_second_trip_over_a_long_list(gpu):
    """1024x513: 525 312 pixels, above the 2 048 workgroups x 256 entries of a refine launch (`std::min<long long>(chunks, 2048)` in
    ptl_kernel_render_refine), so `first += gridDim.x * 256` goes round again.  With T = -1 every pixel is listed: the adaptive frame is the
    plain aa-4 draw bit for bit; the same through layer 1 with a permuted list of all pixels over frames of another content."""
    pa = gpu
    w, h = 1024, 513
    pixels = w * h
    r = _renderer(pa, "basics", "baked")
    r.set_option("aa_count", 4)
    f = r.draw(w, h, rgba8=True, rgba32f=True)
    f8, f32 = f["rgba8"], _bits(f["rgba32f"])
    out = r.draw_adaptive(w, h, threshold=-1, rgba32f=True)
    assert out["count"] == pixels == 525312 and out["count"] > _refine_grid_cap() * 256 and _refine_grid_cap() == 2048
    assert np.array_equal(np.sort(out["list"]), np.arange(pixels, dtype=np.uint32))
    assert np.array_equal(out["rgba8"], f8) and np.array_equal(_bits(out["rgba32f"]), f32)
    entries = np.random.default_rng(513).permutation(pixels).astype(np.uint32)
    start8 = np.full((h, w, 4), 0x3C, np.uint8)
    start32 = np.full((h, w, 4), 0x7FC00000, np.uint32)
    assert (start8 != f8).any(axis=2).all() and (start32 != f32).any(axis=2).all()  # every pixel has to be written
    out8, out32, _ = _refine_through_layer_one(pa, r, w, h, entries, pixels, start8=start8, start32=start32)
    assert np.array_equal(out8, f8) and np.array_equal(out32, f32)


@pytest.mark.gpu
@pytest.mark.parametrize("scene_name,build", [("basics", "baked"), ("monoportal", "unspecialised")], ids=["basics-baked", "monoportal-unspecialised"])
def test_refine_entry_counts_the_segments_of_its_list(gpu, scene_name, build):
    """Under PTL_COUNT_SEGMENTS the refine entry reduces the lanes' trip counts with __shfl_down behind a loop whose lanes `continue`;
    ptl_renderer_draw_adaptive never passes a counter.  A pixel's trips do not depend on the lanes around it: a permutation of all pixels
    counts what the render entry counts for the aa-4 frame, two disjoint halves (lists that end inside a wave) add up to it."""
    pa = gpu
    w, h = 70, 37
    pixels = w * h
    r = _renderer(pa, scene_name, build, extra_flags=pa.FLAG_COUNT_SEGMENTS)
    r.set_option("aa_count", 4)
    f = r.draw(w, h, rgba8=True, segments=True)  # last draw: `_aa_count` 4
    total = f["segments"]
    assert total > 4 * pixels  # at least one trip per sample
    entries = np.random.default_rng(3770).permutation(pixels).astype(np.uint32)
    start8 = np.full((h, w, 4), 0x3C, np.uint8)
    out8, _, counted = _refine_through_layer_one(pa, r, w, h, entries, pixels, start8=start8, segments=True)
    assert counted == total and np.array_equal(out8, f["rgba8"])
    first, second = entries[: pixels // 2], entries[pixels // 2:]
    assert first.size % 64 and second.size % 64 and not np.intersect1d(first, second).size
    a = _refine_through_layer_one(pa, r, w, h, first, first.size, start8=start8, segments=True)[2]
    b = _refine_through_layer_one(pa, r, w, h, second, second.size, start8=start8, segments=True)[2]
    assert 0 < a < total and 0 < b < total and a + b == total, (a, b, total)
    # ... and entries that name no pixel count nothing
    padded = np.concatenate([first, np.full(100, pixels, np.uint32), np.full(100, 0xFFFFFFFF, np.uint32)])
    assert _refine_through_layer_one(pa, r, w, h, padded, padded.size, start8=start8, segments=True)[2] == a


@pytest.mark.gpu
def test_cli_adaptive_frame_is_the_python_mirrors(gpu, tmp_path):
    pa = gpu
    w, h = 64, 36
    png = str(tmp_path / "adaptive.png")
    done = subprocess.run([_exe(pa), "render-frame", pa.scene_path("basics"), "--width", str(w), "--height", str(h), "--aa-count", "4", "--render-depth", "12",
                           "--adaptive-aa", "4", "--timing", "--output", png], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert done.returncode == 0, done.stderr + done.stdout
    r = pa.SceneRenderer(pa.Scene.from_file(pa.scene_path("basics")), device=0, flags=pa.FLAG_REFINE | BAKED(pa) | pa.FLAG_QUICK_JIT)
    r.set_option("aa_count", 4)
    r.set_option("render_depth", 12)
    r.set_option("view_angle", 90.0 / 180.0 * math.pi)
    r.update(0.0)
    mirror = r.draw_adaptive(w, h, threshold=4)
    assert 0 < mirror["count"] < w * h
    assert np.array_equal(pa.png_read(png), mirror["rgba8"])
    m = re.search(r"adaptive aa: threshold 4, (\d+) of (\d+) pixels refined", done.stdout)
    assert m and int(m.group(1)) == mirror["count"] and int(m.group(2)) == w * h, done.stdout
    assert re.search(r"one-sample pass [\d.]+, classification [\d.]+, refine pass [\d.]+", done.stdout)
