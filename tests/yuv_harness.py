"""What tests/test_yuv_output.py, test_yuv_deep.py and test_yuv_chroma.py share: the `gpu` fixture, the conversion of sub-frames through the
entry points with guard bytes around the frame, the payload comparison, the grid-cap knob, the compiler's resource-usage notes, cached
cases, and the `render --frames y4m` plumbing with its stub encoder.  A plain helper module like tests/yuv_reference.py; the three numpy
references stay where they are.  Expected payloads always come from the reference of the module under test; this module uses
yuv_chroma_reference only to split planes for a failure message and to frame a stream (header, frame size), at 4:2:0 too, where
test_420_through_the_new_helper_is_the_shipped_reference pins it to yuv_reference."""
import os
import re
import stat
import subprocess

import numpy as np
import pytest

from tests import yuv_chroma_reference as cr
from tests import yuv_deep_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GUARD = 0xA5
KNOB = "PTL_AVERAGE_IMAGES_GRID_CAP"
W, H, FPS = 64, 36, 2  # the clips the CLI tests render


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


def _convert(pa, deep, chroma, frames, w, h, offset=0):
    """Sub-frames (numpy (h, w, 4) uint8 / float32, or cuda tensors; the same object may appear more than once) -> payload bytes; the 64
    guard bytes behind the frame (and `offset` before it) must survive.  chroma None: through the 4:2:0 entry points
    (ptl_average_to_yuv420p10, ptl_average_f32_to_yuv420p10); 420, 422, 444: through the ones that take the sampling."""
    import torch

    staged = {}
    for f in frames:
        if id(f) not in staged:
            staged[id(f)] = f if isinstance(f, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(f, np.float32 if deep else np.uint8)).cuda()
            assert staged[id(f)].numel() == w * h * 4 and staged[id(f)].dtype == (torch.float32 if deep else torch.uint8) and staged[id(f)].data_ptr() % 16 == 0
    nbytes = pa.yuv420p10_frame_bytes(w, h) if chroma is None else pa.yuv10_frame_bytes(w, h, chroma)
    assert nbytes == cr.frame_bytes(w, h, chroma or 420)
    buf = torch.full((offset + nbytes + 64,), GUARD, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    pointers, stream = [staged[id(f)].data_ptr() for f in frames], torch.cuda.current_stream().cuda_stream
    if chroma is None:
        (pa.average_f32_to_yuv420p10_device if deep else pa.average_to_yuv420p10_device)(pointers, buf.data_ptr() + offset, w, h, stream=stream)
    else:
        (pa.average_f32_to_yuv10_device if deep else pa.average_to_yuv10_device)(pointers, buf.data_ptr() + offset, w, h, chroma, stream=stream)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:offset] == GUARD).all() and (host[offset + nbytes:] == GUARD).all(), "written outside the frame"
    return host[offset: offset + nbytes].tobytes()


def _assert_same_payload(got: bytes, want: bytes, w, h, what, chroma=420):
    if got == want:
        return
    assert len(got) == len(want), (what, len(got), len(want))
    for name, g, r in zip(("Y", "Cb", "Cr"), cr.split_planes(got, w, h, chroma), cr.split_planes(want, w, h, chroma)):
        bad = np.argwhere(g != r)
        if len(bad):
            y, x = bad[0]
            pytest.fail(f"{what}: plane {name} differs in {len(bad)} of {g.size} samples, first at x={x} y={y}: got {g[y, x]}, want {r[y, x]}")


def _shipped_grid_cap():
    """`long cap = 256 * 16;` of launch_over_subframes (portal_amd/csrc/host/postprocess.cpp): the workgroups a post-process launch gets at
    most.  The tests that cross it read it from the source, so a changed cap fails them instead of leaving them vacuous."""
    src = open(os.path.join(ROOT, "portal_amd", "csrc", "host", "postprocess.cpp")).read()
    m = re.findall(r"long cap = (\d+) \* (\d+);", src)
    assert len(m) == 1, "launch_over_subframes no longer spells its grid cap as `long cap = A * B;`"
    return int(m[0][0]) * int(m[0][1])


def _c_getenv(name):
    """What std::getenv of the library sees (monkeypatch.setenv goes through os.environ, which calls putenv)."""
    import ctypes as C

    libc = C.CDLL(None)
    libc.getenv.restype, libc.getenv.argtypes = C.c_char_p, [C.c_char_p]
    return libc.getenv(name.encode())


def _resource_usage(notes):
    """{function: {key: value}} from the compiler's -Rpass-analysis=kernel-resource-usage notes (stderr of the build)."""
    usage, name = {}, None
    for line in notes.splitlines():
        m = re.search(r"Function Name: (\w+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"(ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|VGPRs): (\d+)", line)
        if m and name:
            usage.setdefault(name, {})[m.group(1)] = int(m.group(2))
    print(usage)
    return usage


def _compile_with_usage(source, tmp_path):
    """portal_amd/csrc/kernels/<source>.hip compiled with the Makefile's flags -> _resource_usage of its notes."""
    src = os.path.join(ROOT, "portal_amd", "csrc", "kernels", source + ".hip")
    out = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-vgpr-regalloc=basic", "--genco", "--no-gpu-bundle-output",
                          "-Rpass-analysis=kernel-resource-usage", src, "-o", str(tmp_path / (source + ".hsaco"))], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    return _resource_usage(out.stderr)


def _entries(prefix):
    """The six entries of a code object: three samplings, the pointers in the kernel arguments or in a table."""
    return {f"{prefix}{c}p10{t}_kernel" for c in cr.SAMPLINGS for t in ("", "_table")}


# ---- cases computed once and shared, never modified ---------------------------------------------
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


def _random_frames(seed, n, w, h, deep=True):
    """Float sub-frames: mostly [0, 1), a band beyond both ends.  RGBA8 ones: every byte random."""
    rng = np.random.default_rng(seed)
    if not deep:
        return [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for _ in range(n)]
    frames = [rng.random((h, w, 4), dtype=np.float32) for _ in range(n)]
    frames[0][: (h + 3) // 4] = rng.uniform(-0.25, 1.25, ((h + 3) // 4, w, 4)).astype(np.float32)
    return frames


def _averaged(deep, frames):
    """A: the averaged frame the contract starts from, by the shipped references."""
    if deep:
        return dr.encode16(frames)
    from oracle import postprocess as pp

    return pp.average_images(frames) if len(frames) > 1 else frames[0]


def _case(deep, seed, n, w, h):
    """(sub-frames, A): computed once per key."""
    def make():
        frames = _random_frames(seed, n, w, h, deep)
        return frames, _averaged(deep, frames)

    return _once(("case", deep, seed, n, w, h), make)


def _case_payload(tag, deep, seed, n, w, h, payload):
    """(sub-frames, payload(sub-frames, A)) of _case: the reference payload is computed once per (tag, key) as well."""
    frames, a = _case(deep, seed, n, w, h)
    return frames, _once(("payload", tag, deep, seed, n, w, h), lambda: payload(frames, a))


def _special_values():
    """NaN of both signs (quiet and signalling), both infinities, both zeros, negatives, denormals, 1.0 and its neighbours, values above 1,
    and for a few hundred k the floats on both sides of the rounding boundary (k + 1/2) / 65535."""
    bits = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0xff800001, 0x7fffffff, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0xbf800000, 0xb3000000, 0xff7fffff,
                     0x00000001, 0x007fffff, 0x80000001, 0x807fffff, 0x00800000, 0x3f800000, 0x3f7fffff, 0x3f800001, 0x40000000, 0x7f7fffff, 0x3f000000], np.uint32)
    k = np.unique(np.concatenate([np.arange(0, 40), np.arange(65495, 65535), np.random.default_rng(5).integers(0, 65535, 240)]))
    # where the quantisation decides: the smallest float that gives k + 1, found by bisection over the bit patterns between k / 65535 (which
    # gives k) and (k + 1) / 65535 (which gives k + 1) -- it lies next to (k + 1/2) / 65535 -- with its two neighbours
    lo, hi = (k / 65535.0).astype(np.float32).view(np.uint32).astype(np.int64), ((k + 1) / 65535.0).astype(np.float32).view(np.uint32).astype(np.int64)
    assert np.array_equal(dr.quantise16(lo.astype(np.uint32).view(np.float32)), k) and np.array_equal(dr.quantise16(hi.astype(np.uint32).view(np.float32)), k + 1)
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        up = dr.quantise16(mid.astype(np.uint32).view(np.float32)) > k
        lo, hi = np.where(up, lo, mid), np.where(up, mid, hi)
    first, last = hi.astype(np.uint32).view(np.float32), lo.astype(np.uint32).view(np.float32)  # the first float of k + 1, the last of k
    assert np.array_equal(dr.quantise16(first), k + 1) and np.array_equal(dr.quantise16(last), k) and len(k) >= 300
    assert (np.abs(first.astype(np.float64) * 65535.0 - (k + 0.5)) < 0.01).all()
    return np.concatenate([bits.view(np.float32), first, last, np.nextafter(first, np.float32(2))]).astype(np.float32)


def _frame_from_values(values, w, h, fill=0.5):
    """A float frame whose R, G, B channels hold `values` in order (alpha: NaN, which is ignored); the rest is `fill`."""
    values = np.asarray(values, np.float32)
    assert values.size <= 3 * w * h
    rgb = np.full(3 * w * h, fill, np.float32)
    rgb[: values.size] = values
    frame = np.full((h, w, 4), np.nan, np.float32)
    frame[..., :3] = rgb.reshape(h, w, 3)
    return frame


# ---- the CLI ------------------------------------------------------------------------------------
def _path_without_ffmpeg():
    return os.pathsep.join(d for d in os.environ.get("PATH", "").split(os.pathsep) if d and not os.path.exists(os.path.join(d, "ffmpeg")))


def _write_stub(directory, body):
    """An executable `ffmpeg` in `directory` -> the PATH that finds it first."""
    os.makedirs(directory, exist_ok=True)
    stub = os.path.join(directory, "ffmpeg")
    with open(stub, "w") as f:
        f.write("#!/bin/sh\n" + body)
    os.chmod(stub, os.stat(stub).st_mode | stat.S_IXUSR | stat.S_IXGRP | stat.S_IXOTH)
    return str(directory) + os.pathsep + os.environ.get("PATH", "")


def _copying_stub(directory, args_file):
    """A stub encoder that records its arguments and copies stdin to its last argument."""
    return _write_stub(directory, f'if [ "$1" = "-version" ]; then exit 0; fi\nprintf \'%s\\n\' "$@" > "{args_file}"\nfor last; do :; done\nexec cat > "$last"\n')


def _render(pa, out_dir, clip, options, path=None, check=True):
    """`portal-amd render scenes/basics.ron <clip> --frames y4m` at W x H, FPS, under a time limit of its own; PATH without an ffmpeg unless
    one is given.  -> the finished process (its status asserted unless check is False)."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    scene = pa.scene_path("basics")
    cmd = ["timeout", "-k", "10", "300", exe, "render", scene, clip, "--width", str(W), "--height", str(H), "--fps", str(FPS), "--frames", "y4m",
           "--out-dir", str(out_dir), "--asset-root", os.path.dirname(os.path.dirname(scene))] + options
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=400, env=dict(os.environ, PATH=path or _path_without_ffmpeg()))
    if check:
        assert out.returncode == 0, out.stderr + out.stdout
    return out


def _drawn_clip(pa, blur):
    """The first clip of scenes/basics.ron drawn through the Python mirror with --aa-count 2 --render-depth 12, once per blur: per frame the
    RGBA8 and the float sub-frames.  -> (frames, clip name)"""
    def draw():
        clip, duration = pa.Scene.from_file(pa.scene_path("basics")).animations()[0]
        count = max(1, int(np.float32(duration) * np.float32(FPS)))
        scene = pa.Scene.from_file(pa.scene_path("basics"))
        r = pa.SceneRenderer(scene, device=0)
        r.set_option("aa_count", 2)
        r.set_option("render_depth", 12)
        scene.init_animation(clip)
        r.update(0.0)
        frames = []
        for i in range(count):
            subs8, subs32 = [], []
            for j in range(blur):
                r.set_option("aa_start", j)
                r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
                drawn = r.draw(W, H, rgba8=True, rgba32f=True)
                subs8.append(np.array(drawn["rgba8"]))
                subs32.append(np.array(drawn["rgba32f"]))
            frames.append((subs8, subs32))
        return frames, clip

    return _once(("clip", blur), draw)


def _expected_stream(pa, blur, chroma, payload):
    """Header plus, per frame of _drawn_clip, FRAME and payload(RGBA8 sub-frames, float sub-frames).  -> (stream, frames, clip name)"""
    frames, clip = _drawn_clip(pa, blur)
    return cr.y4m_header(W, H, FPS, chroma) + b"".join(b"FRAME\n" + payload(subs8, subs32) for subs8, subs32 in frames), frames, clip


def _check_stream(got: bytes, want: bytes, count, chroma=420):
    header = cr.y4m_header(W, H, FPS, chroma)
    size = 6 + cr.frame_bytes(W, H, chroma)
    assert got[: len(header)] == header
    assert len(got) == len(header) + count * size, "not exactly `count` frames"
    for i in range(count):
        at = len(header) + i * size
        assert got[at: at + 6] == b"FRAME\n", i
        _assert_same_payload(got[at + 6: at + size], want[at + 6: at + size], W, H, f"frame {i}", chroma)
    assert got == want
