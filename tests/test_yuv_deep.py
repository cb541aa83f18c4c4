"""`render --frames y4m --deep-colour`: the kernel that makes 10-bit frames from float sub-frames (portal_amd/csrc/kernels/yuv10_f32.hip), its C
ABI, the Python mirror and the CLI option, against tests/yuv_deep_reference.py (a numpy restatement of the contract in DESIGN.md 2.3.2).
Every comparison of a payload is byte equality."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import yuv_deep_reference as dr
from tests import yuv_reference as yr
from tests.yuv_harness import (FPS, H, HIPCC, KNOB, ROOT, W, _assert_same_payload, _c_getenv, _case_payload, _convert, _entries, _frame_from_values, _random_frames, _render,
                               _resource_usage, _shipped_grid_cap, _special_values, gpu)  # noqa: F401 (gpu: a fixture)

CORNERS = [(r, g, b) for r in (0, 65535) for g in (0, 65535) for b in (0, 65535)]  # the eight corners of the RGB cube, 16 bit
BLUE, RED, YELLOW, CYAN, WHITE = (0, 0, 65535), (65535, 0, 0), (65535, 65535, 0), (0, 65535, 65535), (65535, 65535, 65535)


def _flat_columns(colours):
    """colour k fills rows 2k, 2k+1 of a two-pixel-wide frame: each chroma sample then sees one flat colour (its columns clamp to the frame)."""
    return np.repeat(np.repeat(np.asarray(colours, np.int64)[:, None, :], 2, axis=0), 2, axis=1)


def _unorm8(v):
    """pack_rgba8's quantisation: the 8-bit value of a float channel."""
    v = np.asarray(v, np.float32)
    with np.errstate(all="ignore"):
        q = np.floor(np.where((v > 0) & (v < 1), v, np.float32(0)) * np.float32(255.0) + np.float32(0.5)).astype(np.int64)
    return np.where(v >= 1, 255, np.where(v > 0, q, 0)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------
# CPU: the contract's own properties
# ---------------------------------------------------------------------------------------------
def test_coefficients_are_the_rounded_ones_and_no_accumulator_overflows():
    scale = 1023.0 / 65535.0 * (1 << 22)  # luma; a chroma coefficient meets S = 8 x a colour and is shifted by 26: 2^26 / 8 = twice this
    cb = [-dr.KR / (2 * (1 - dr.KB)), -dr.KG / (2 * (1 - dr.KB)), 0.5]
    cr = [0.5, -dr.KG / (2 * (1 - dr.KR)), -dr.KB / (2 * (1 - dr.KR))]
    assert dr.Y_COEFF == tuple(round(k * scale) for k in (dr.KR, dr.KG, dr.KB)) and sum(dr.Y_COEFF) == 65473 == round(scale)
    assert dr.CB_COEFF == tuple(round(k * 2 * scale) for k in cb) and sum(dr.CB_COEFF) == 0
    assert dr.CR_COEFF == tuple(round(k * 2 * scale) for k in cr) and sum(dr.CR_COEFF) == 0
    assert 65473 * 65535 + (1 << 21) == 4292870207 < 1 << 32
    s = 8 * 65535  # the largest weighted sum
    assert s == 524280
    lowest = min(sum(k * (s if corner[c] else 0) for c, k in enumerate(coeff)) + dr.CHROMA_BIAS for coeff in (dr.CB_COEFF, dr.CR_COEFF) for corner in CORNERS)
    assert lowest - (1 << 25) == 33553928 > 0  # before the rounding term (yellow's Cb, cyan's Cr): `>>` is a plain shift


def test_reference_against_the_real_valued_definition():
    """On flat colours (10^5 seeded 16-bit triples, a thousand greys, the cube corners) the integer contract stays within 0.53 codes of
    H.273 in real numbers: 0.5 from the final rounding, at most 3 x 0.5 x 65535 / 2^22 = 0.023 from the rounded coefficients."""
    rng = np.random.default_rng(2020)
    greys = np.repeat(rng.integers(0, 65536, 1000)[:, None], 3, axis=1)
    colours = np.concatenate([greys, np.array(CORNERS), rng.integers(0, 65536, (100000, 3))])
    y, cb, cr = dr.planes_from_e(_flat_columns(colours), clamp=False)
    ry, rcb, rcr = dr.real_valued(colours)
    worst = {name: float(np.abs(got - real).max()) for name, got, real in (("Y", y[::2, 0], ry), ("Y'", y[1::2, 1], ry), ("Cb", cb[:, 0], rcb), ("Cr", cr[:, 0], rcr))}
    print(worst)
    assert max(worst.values()) <= 0.53, worst


def test_greys_corners_and_the_clamp():
    q = np.arange(65536, dtype=np.int64)
    y, cb, cr = dr.planes_from_e(_flat_columns(np.repeat(q[:, None], 3, axis=1)))
    assert np.array_equal(y[::2, 0], (2 * 1023 * q + 65535) // (2 * 65535))  # floor(1023 q / 65535 + 1/2), in integers
    assert np.array_equal(y[::2, 0], y[1::2, 1]) and (cb == 512).all() and (cr == 512).all()
    y, cb, cr = dr.planes_from_e(_flat_columns(CORNERS))
    _, ucb, ucr = dr.planes_from_e(_flat_columns(CORNERS), clamp=False)
    for k, rgb in enumerate(CORNERS):
        assert (ucb[k, 0] == 1024) == (rgb == BLUE) and (ucr[k, 0] == 1024) == (rgb == RED), rgb  # pure blue and pure red reach 1024 before the min
        assert cb[k, 0] == min(1023, ucb[k, 0]) and cr[k, 0] == min(1023, ucr[k, 0]) and 0 <= ucb[k, 0] <= 1024 and 0 <= ucr[k, 0] <= 1024
        assert (cb[k, 0] == 0) == (rgb == YELLOW) and (cr[k, 0] == 0) == (rgb == CYAN), rgb
        if rgb == WHITE:
            assert y[2 * k, 0] == 1023 and cb[k, 0] == 512 and cr[k, 0] == 512
        if rgb == (0, 0, 0):
            assert y[2 * k, 0] == 0


def test_quantisation_and_the_root_follow_their_definitions():
    bits = np.array([0x7fc00000, 0xffc00000, 0x7f800001, 0x7f800000, 0xff800000, 0x00000000, 0x80000000, 0xbf800000, 0x00000001, 0x007fffff, 0x80000001,
                     0x3f800000, 0x3f7fffff, 0x3f800001, 0x40000000], np.uint32)
    assert dr.quantise16(bits.view(np.float32)).tolist() == [0, 0, 0, 65535, 0, 0, 0, 0, 0, 0, 0, 65535, 65535, 65535, 65535]
    below_one = np.array([0x3f7fffff], np.uint32).view(np.float32)[0]
    assert 65535.49 < float(below_one * np.float32(65535.0) + np.float32(0.5)) < 65535.5  # the result never reaches 65536
    q = np.arange(65536)
    assert np.array_equal(dr.quantise16((q / 65535.0).astype(np.float32)), q)  # every q has a float that gives it
    m = np.concatenate([np.arange(0, 70000), np.arange(65535 ** 2 - 70000, 65535 ** 2 + 1)])
    assert dr.nearest_roots(m).tolist() == [dr.nearest_root(int(v)) for v in m]
    for e in (0, 1, 2, 3, 255, 256, 65534, 65535):  # both ends of every e's interval
        assert dr.nearest_root(e * (e + 1)) == e and dr.nearest_root(e * (e + 1) + 1) == e + 1
    assert np.array_equal(dr.encode16_from_q(q[None]), q)  # n = 1: E = q, no special case


def test_one_subframe_stays_within_three_codes_of_the_8_bit_lumas():
    """n = 1: this luma against the one the 8-bit contract gives for pack_rgba8 of the same floats.  1023 (0.5 / 255 + 0.5 / 65535) = 2.01
    plus the two final roundings: at most 3 codes."""
    rng = np.random.default_rng(8)
    frame = rng.random((64, 64, 4), dtype=np.float32)
    frame[:4] = rng.uniform(-0.2, 1.2, (4, 64, 4)).astype(np.float32)
    deep, _, _ = dr.planes_from_e(dr.encode16([frame]))
    plain, _, _ = yr.yuv_planes(_unorm8(frame))
    worst = int(np.abs(deep - plain).max())
    print(worst)
    assert 1 <= worst <= 3


def test_a_1024_step_ramp_keeps_its_1024_codes():
    """What the feature is for: v = k / 1023 gives 1024 distinct luma codes through this contract and 256 through the 8-bit one."""
    ramp = (np.arange(1024) / 1023.0).astype(np.float32)
    frame = np.repeat(ramp[None, :, None], 4, axis=2)[[0, 0]]  # 2 x 1024, grey
    deep, cb, cr = dr.planes_from_e(dr.encode16([frame]))
    assert np.array_equal(deep[0], np.arange(1024)) and (cb == 512).all() and (cr == 512).all()
    plain, _, _ = yr.yuv_planes(_unorm8(frame))
    assert len(np.unique(deep[0])) == 1024 and len(np.unique(plain[0])) == 256
    for n in (2, 4, 16):  # identical sub-frames average to themselves
        assert dr.deep_reference([frame] * n) == dr.deep_reference([frame])


def test_the_kernels_mean_is_the_floor_for_every_count():
    """ptl_mean_n's argument in numbers: floor(sum / n) as (u32)(sum * (1.0 / n) + 2^-10) in binary64, at the sums where it could go wrong
    (multiples of n, one below, one above, n - 1 above) up to the largest, 256 * 65535^2, for every n."""
    rng = np.random.default_rng(40)
    for n in range(2, 257):
        m = np.concatenate([rng.integers(0, 65535 ** 2, 4000), [0, 1, 65535 ** 2 - 1, 65535 ** 2]]).astype(np.int64)
        for sums in (m * n, np.maximum(m * n - 1, 0), np.minimum(m * n + 1, n * 65535 ** 2), np.minimum(m * n + n - 1, n * 65535 ** 2)):
            got = (sums.astype(np.float64) * (np.float64(1.0) / np.float64(n)) + np.float64(2.0 ** -10)).astype(np.int64)
            assert np.array_equal(got, sums // n), n


# ---------------------------------------------------------------------------------------------
# CPU: the entry point, the build, the CLI's refusals
# ---------------------------------------------------------------------------------------------
def test_entry_point_refuses_before_any_gpu_call(pa):
    """No frames, bad counts, bad sizes, unaligned pointers, more pixels than 32-bit byte offsets reach -> PTL_ERR_INVALID; no device needed."""
    import ctypes as C

    f = pa.lib().ptl_average_f32_to_yuv420p10
    ptrs = (C.c_void_p * 2)(4096, 8192)
    out = C.c_void_p(1 << 20)
    assert f(0, None, 2, out, 4, 4, None, None) == -1
    assert f(0, ptrs, 2, None, 4, 4, None, None) == -1
    assert f(0, (C.c_void_p * 2)(4096, None), 2, out, 4, 4, None, None) == -1
    assert f(0, ptrs, 0, out, 4, 4, None, None) == -1
    many = (C.c_void_p * 257)(*([4096] * 257))
    assert f(0, many, 257, out, 4, 4, None, None) == -1
    assert f(0, (C.c_void_p * 2)(4096, 8200), 2, out, 4, 4, None, None) == -1  # 8-byte aligned only
    assert f(0, ptrs, 2, C.c_void_p((1 << 20) + 8), 4, 4, None, None) == -1
    assert f(0, ptrs, 2, out, 0, 4, None, None) == -1
    assert f(0, ptrs, 2, out, 4, -2, None, None) == -1
    assert f(0, ptrs, 2, out, 1 << 14, (1 << 14) + 1, None, None) == -1  # beyond 2^28 pixels
    assert f(0, ptrs, 2, out, (1 << 14) + 1, 1 << 14, None, None) == -1
    header = open(os.path.join(ROOT, "include", "portal_amd.h")).read()
    assert "int ptl_average_f32_to_yuv420p10(" in header and "W*H <= 2^28" in header


def test_make_builds_the_code_object_without_scratch(tmp_path):
    """`make portal_amd/kernels/yuv10_f32.hsaco` in a copy of the tree's Makefile and kernel sources: its six entries compile for gfx950
    with 0 bytes of scratch, no SGPR or VGPR spills, no LDS and at most 128 VGPRs; the numbers are printed from the compiler's own notes.
    The object holds no fused or contracted binary32 multiply-add: the quantisation is a product and a sum, each rounded (a toolchain
    that contracts them again fails here, before any GPU run), and the packed or plain multiply it is made of is there."""
    shutil.copy(os.path.join(ROOT, "Makefile"), tmp_path / "Makefile")
    shutil.copytree(os.path.join(ROOT, "portal_amd", "csrc", "kernels"), tmp_path / "portal_amd" / "csrc" / "kernels")
    target = "portal_amd/kernels/yuv10_f32.hsaco"
    out = subprocess.run(["make", target, f"HIPCC={HIPCC} -Rpass-analysis=kernel-resource-usage"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    assert os.path.getsize(tmp_path / target) > 1000
    usage = _resource_usage(out.stderr)
    assert set(usage) == _entries("ptl_average_f32_to_yuv") >= {"ptl_average_f32_to_yuv420p10_kernel", "ptl_average_f32_to_yuv420p10_table_kernel"}
    for entry, u in usage.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["LDS Size [bytes/block]"] == 0, (entry, u)
        assert u["SGPRs Spill"] == 0 and u["VGPRs Spill"] == 0, (entry, u)
        assert u["VGPRs"] <= 128, (entry, u)  # four waves per SIMD
    objdump = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "lib", "llvm", "bin", "llvm-objdump")
    listing = subprocess.run([objdump, "-d", str(tmp_path / target)], capture_output=True, text=True, timeout=120)
    assert listing.returncode == 0, listing.stderr
    mnemonics = re.findall(r"^\s+(v_\w+)", listing.stdout, re.M)
    assert len(mnemonics) > 1000
    fused = sorted({m for m in mnemonics if re.match(r"v_(pk_)?(fma|fmac|mad|mac)_(legacy_)?f32|v_(fma|mad)_mix", m)})
    assert not fused, fused
    assert any(m.startswith(("v_pk_mul_f32", "v_mul_f32")) for m in mnemonics) and any(m.startswith(("v_pk_add_f32", "v_add_f32")) for m in mnemonics)
    makefile = open(os.path.join(ROOT, "Makefile")).read()
    assert target in re.search(r"^KERNELS\s*:=(.*)$", makefile, re.M).group(1)
    assert '#include "average_common.h"' in open(os.path.join(ROOT, "portal_amd", "csrc", "kernels", "yuv10_f32.hip")).read()


@pytest.mark.parametrize("cmd,extra,reason", [("render", ["--deep-colour"], "--deep-colour needs --frames y4m"),
                                              ("render", ["--deep-colour", "--frames", "png"], "--deep-colour needs --frames y4m"),
                                              ("render-frame", ["--deep-colour", "--frames", "y4m"], "--deep-colour is an option of render"),
                                              ("precompile", ["--frames", "y4m", "--deep-colour"], "--deep-colour is an option of render")])
def test_cli_refuses_deep_colour_where_it_means_nothing(pa, tmp_path, cmd, extra, reason):
    """Refused while the arguments are parsed: exit status 2, one line that says why, nothing rendered."""
    exe = os.path.join(os.path.dirname(pa.__file__), "portal-amd")
    args = [exe, cmd, pa.scene_path("basics")] + (["anim.4.portals", "--out-dir", str(tmp_path)] if cmd == "render" else []) + extra
    out = subprocess.run(args, capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert out.returncode == 2, out.stderr + out.stdout
    assert reason in out.stderr and len(out.stderr.strip().splitlines()) == 1
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _is_fast(w, h):
    return w % 2 == 0 and h % 2 == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 16, 64, 65, 256])
@pytest.mark.parametrize("w,h", [(37, 23), (256, 6)])
def test_kernel_matches_reference_for_every_subframe_count(gpu, w, h, n):
    """37x23: the general path.  256x6: the fast path, 128 blocks = two waves per row pair.  Beyond 64 sub-frames the pointer-table entry."""
    assert _is_fast(w, h) == ((w, h) == (256, 6))
    frames = _random_frames(100 * n + w, n, w, h)
    _assert_same_payload(_convert(gpu, True, None, frames, w, h), dr.deep_reference(frames), w, h, f"{w}x{h} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (13, 11), (2, 2), (130, 6), (244, 135)])
def test_kernel_matches_reference_at_any_frame_size(gpu, w, h):
    """1x1, 5x3, 13x11: the general path with W*H odd, so the chroma planes start on odd multiples of 2 bytes.  2x2, 130x6: the fast path
    whose last wave of a row pair is partial (65 blocks per row).  244x135: the general path at a realistic shape.  Three sub-frames, and
    the frame 16 bytes into its buffer: nothing before or behind it is written."""
    assert _is_fast(w, h) == ((w, h) in ((2, 2), (130, 6)))
    frames = _random_frames(w * 1000 + h, 3, w, h)
    _assert_same_payload(_convert(gpu, True, None, frames, w, h, offset=16), dr.deep_reference(frames), w, h, f"{w}x{h}")
    _assert_same_payload(_convert(gpu, True, None, frames[:1], w, h), dr.deep_reference(frames[:1]), w, h, f"{w}x{h} n=1")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(32, 12), (33, 11)])
def test_special_inputs_as_bit_patterns(gpu, w, h):
    """NaN of both signs (quiet and signalling), both infinities, both zeros, negatives, denormals, 1.0 and its neighbours, values above 1,
    and for a few hundred k the float nearest (k + 1/2) / 65535 with both its neighbours -- as one sub-frame, and as two (with the values
    reversed in the second).  Both paths."""
    values = _special_values()
    assert values.size <= 3 * w * h and _is_fast(w, h) == (w == 32)
    frame, reversed_frame = _frame_from_values(values, w, h), _frame_from_values(values[::-1], w, h)
    for frames in ([frame], [frame, reversed_frame], [frame, frame, reversed_frame]):
        _assert_same_payload(_convert(gpu, True, None, frames, w, h), dr.deep_reference(frames), w, h, f"{w}x{h} special n={len(frames)}")


@pytest.mark.gpu
def test_every_q_once(gpu):
    """256x256, n = 1: pixel p holds p / 65535, (65535 - p) / 65535 and (7 p mod 65536) / 65535 -- every q in every channel.  E must be q."""
    w = h = 256
    p = np.arange(65536, dtype=np.int64)
    q = np.stack([p, 65535 - p, (7 * p) % 65536], axis=1).reshape(h, w, 3)
    frame = np.zeros((h, w, 4), np.float32)
    frame[..., :3] = (q / 65535.0).astype(np.float32)
    assert np.array_equal(dr.encode16([frame]), q)
    for c in range(3):
        assert np.array_equal(np.sort(q[..., c].ravel()), p)
    _assert_same_payload(_convert(gpu, True, None, [frame], w, h), dr.payload_from_e(q), w, h, "every q")


@pytest.mark.gpu
def test_rounding_boundary_of_the_root(gpu):
    """n = 2 with q pairs (a, b), 0 <= a, b < 3000, whose mean floor((a^2 + b^2) / 2) sits on an end of some e's interval: e (e - 1) + 1, the
    first value that rounds to e, or e (e + 1), the last.  Found by search here; a root that is off by one flips these."""
    b, a = np.meshgrid(np.arange(3000, dtype=np.int64), np.arange(3000, dtype=np.int64))
    m = (a * a + b * b) // 2
    e = dr.nearest_roots(m)
    hit = ((m == e * (e - 1) + 1) | (m == e * (e + 1))) & (e > 0)  # (17 371 ordered pairs)
    pairs = np.stack([a[hit], b[hit]], axis=1)
    print(len(pairs), "pairs;", int((m[hit] == (e * (e + 1))[hit]).sum()), "at the upper end")
    w, h = 128, 46
    pairs = pairs[np.random.default_rng(1).permutation(len(pairs))[: 3 * w * h]]
    assert len(pairs) >= 1000
    lower = int((m[hit] == (e * (e - 1) + 1)[hit]).sum())
    assert lower >= 100 and int(hit.sum()) - lower >= 100  # both ends
    frames = [_frame_from_values(pairs[:, 0] / 65535.0, w, h, fill=0.0), _frame_from_values(pairs[:, 1] / 65535.0, w, h, fill=0.0)]
    assert np.array_equal(dr.quantise16(frames[0][..., :3]).ravel()[: len(pairs)], pairs[:, 0])
    _assert_same_payload(_convert(gpu, True, None, frames, w, h), dr.deep_reference(frames), w, h, "root boundary")
    general = [f[:, : w - 1] for f in frames]
    _assert_same_payload(_convert(gpu, True, None, general, w - 1, h), dr.deep_reference(general), w - 1, h, "root boundary, general path")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(6, 4), (5, 3)])
def test_largest_sum(gpu, w, h):
    """n = 256 and every value >= 1: the sum is 256 * 65535^2, the largest there is; E = 65535, the frame is white."""
    frame = np.full((h, w, 4), 1.0, np.float32)
    frame[::2, :, 1] = np.inf
    frame[:, ::2, 2] = 3.5
    got = _convert(gpu, True, None, [frame] * 256, w, h)
    _assert_same_payload(got, dr.deep_reference([frame] * 256), w, h, "largest sum")
    y, cb, cr = yr.split_planes(got, w, h)
    assert (y == 1023).all() and (cb == 512).all() and (cr == 512).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [3, 7, 255])
def test_mean_boundary(gpu, n):
    """q_k chosen (by search over seeded vectors of large q) so that the sum of squares is m n - 1 and m n: the floor of the mean is m - 1
    and m.  A division that is off by one ulp flips these."""
    rng = np.random.default_rng(n)
    q = rng.integers(60000, 65536, (60000 if n < 255 else 40000, n)).astype(np.int64)
    sums = (q * q).sum(axis=1)
    exact, below = q[sums % n == 0], q[sums % n == n - 1]
    w, h = 16, 6
    half = 3 * w * h // 2  # 144 values of each kind, alternating: a frame's every row holds both
    assert len(exact) >= half and len(below) >= half and (sums // n > 1 << 31).all()
    chosen = np.stack([exact[:half], below[:half]], axis=1).reshape(2 * half, n)  # (K, n): exact, below, exact, ...
    frames = [_frame_from_values(chosen[:, k] / 65535.0, w, h, fill=1.0) for k in range(n)]
    general = [f[:5, :15] for f in frames]

    def residues(subframes):
        """How many channel values of what is sent have a sum of squares of m n, and of m n - 1."""
        q_sent = np.stack([dr.quantise16(f[..., :3]) for f in subframes])
        rest = (q_sent * q_sent).sum(axis=0) % n
        return int((rest == 0).sum()), int((rest == n - 1).sum())

    assert residues(frames) == (half, half) and min(residues(general)) >= 100, (residues(frames), residues(general))
    _assert_same_payload(_convert(gpu, True, None, frames, w, h), dr.deep_reference(frames), w, h, f"mean boundary n={n}")
    _assert_same_payload(_convert(gpu, True, None, general, 15, 5), dr.deep_reference(general), 15, 5, f"mean boundary n={n}, general path")


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(4, 2), (5, 3)])
def test_saturated_colours(gpu, w, h):
    """The eight cube corners as flat frames, on both paths, as one sub-frame and as two: 1023 where the reference before its min holds 1024
    (pure blue's Cb, pure red's Cr), and 0 is reached (yellow's Cb, cyan's Cr)."""
    reached = {"cb_clamp": 0, "cr_clamp": 0, "cb_zero": 0, "cr_zero": 0}
    for rgb in CORNERS:
        frame = np.tile(np.array([c / 65535.0 for c in rgb] + [0.25], np.float32), (h, w, 1))
        for n in (1, 2):
            got = _convert(gpu, True, None, [frame] * n, w, h)
            _assert_same_payload(got, dr.deep_reference([frame] * n), w, h, f"{rgb} n={n}")
            _, cb, cr = yr.split_planes(got, w, h)
            _, ucb, ucr = dr.planes_from_e(dr.encode16([frame] * n), clamp=False)
            assert np.array_equal(cb == 1023, ucb >= 1023) and np.array_equal(cr == 1023, ucr >= 1023) and cb.max() <= 1023 and cr.max() <= 1023
            assert (ucb == 1024).all() == (rgb == BLUE) and (ucr == 1024).all() == (rgb == RED)
            reached["cb_clamp"] += int((ucb == 1024).sum())
            reached["cr_clamp"] += int((ucr == 1024).sum())
            reached["cb_zero"] += int((cb == 0).sum())
            reached["cr_zero"] += int((cr == 0).sum())
    assert all(reached.values()), reached


def _lanes(w, h):
    return ((w + 1) // 2) * ((h + 1) // 2)


KNOB_SHAPES = {"fast-256x134": (256, 134), "general-244x135": (244, 135), "fast-136x70": (136, 70)}


def test_knob_shapes_make_the_trips_they_are_meant_to():
    assert _shipped_grid_cap() == 4096
    assert _lanes(256, 134) == 8576 and _lanes(244, 135) == 8296 and _lanes(136, 70) == 2380
    for w, h in KNOB_SHAPES.values():
        for cap in (1, 3):
            assert 2 * cap * 256 < _lanes(w, h) <= 4096 * 256  # at least three trips, all of them the knob's
    assert 2380 % 256 == 76 and 2380 % 768 == 76 and 76 % 64 == 12  # fast path: the last trip ends in the middle of a wave, under both caps
    assert 4096 * 256 < _lanes(2050, 2050) == 1050625 < 2 * 4096 * 256  # the shipped cap crossed once


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 65])
@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("kind", list(KNOB_SHAPES))
def test_grid_stride_with_the_cap_knob(gpu, monkeypatch, kind, cap, n):
    """The grid-stride loops going round more than twice, on both paths and both entries (n = 65: the pointer table), with 1 and 3
    workgroups.  136x70 is 2 380 blocks: the last trip ends after 76 lanes, in the middle of a wave, and the cross-lane move of the fast path
    still finds its lower neighbour.  Equal to the reference and to the same call with the shipped grid."""
    w, h = KNOB_SHAPES[kind]
    assert _is_fast(w, h) == kind.startswith("fast")
    frames, want = _case_payload("deep", True, 7000 + 10 * n + len(kind), n, w, h, lambda frames, a: dr.deep_reference(frames))  # once per (shape, n), shared by the caps
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None
    shipped = _convert(gpu, True, None, frames, w, h)
    monkeypatch.setenv(KNOB, str(cap))
    assert _c_getenv(KNOB) == str(cap).encode()
    got = _convert(gpu, True, None, frames, w, h)
    _assert_same_payload(got, want, w, h, f"{kind} cap={cap} n={n}")
    assert got == shipped


@pytest.mark.gpu
def test_grid_stride_at_the_shipped_cap(gpu, monkeypatch):
    """The second trip with no knob: 2050x2050 is 1 050 625 blocks against 4096 x 256 lanes; n = 1, a 67 MB input made on the card."""
    import torch

    w = h = 2050
    monkeypatch.delenv(KNOB, raising=False)
    assert _c_getenv(KNOB) is None and _lanes(w, h) > _shipped_grid_cap() * 256
    g = torch.Generator(device="cuda").manual_seed(2050)
    frame = torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=g) * 1.25 - 0.125
    got = _convert(gpu, True, None, [frame], w, h)
    _assert_same_payload(got, dr.deep_reference([frame.cpu().numpy()]), w, h, "2050x2050")


@pytest.mark.gpu
def test_elapsed_ms_and_a_stream_of_the_callers(gpu):
    """Launched on the stream it is given (a non-default torch stream, the inputs produced on it); with elapsed_ms the launch is bracketed by
    events and waited for."""
    import torch

    pa = gpu
    w, h = 640, 360
    nbytes = pa.yuv420p10_frame_bytes(w, h)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        g = torch.Generator(device="cuda").manual_seed(11)
        frames = [torch.rand((h, w, 4), dtype=torch.float32, device="cuda", generator=g) for _ in range(4)]
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        ms = pa.average_f32_to_yuv420p10_device([f.data_ptr() for f in frames], out.data_ptr(), w, h, stream=side.cuda_stream, timed=True)
        assert ms is not None and 0.0 < ms < 1000.0
        got = out.cpu().numpy().tobytes()  # the timed call has waited; the copy is ordered behind it on the same stream anyway
        out.zero_()
        assert pa.average_f32_to_yuv420p10_device([f.data_ptr() for f in frames], out.data_ptr(), w, h, stream=side.cuda_stream) is None
        side.synchronize()
        assert out.cpu().numpy().tobytes() == got
    _assert_same_payload(got, dr.deep_reference([f.cpu().numpy() for f in frames]), w, h, "side stream")


# ---- the CLI ---------------------------------------------------------------------------------
MAX_FRAMES = 2
SCENE, CLIP = "basics", "anim.4.portals"  # (scenes/monoportal.ron has no clip; this is the clip the other end-to-end tests of `render` draw)


def _render_frames(pa, out_dir, extra):
    """The first MAX_FRAMES frames of CLIP with the defaults of `render` -> the directory the clip's files are in."""
    assert SCENE == "basics"
    _render(pa, out_dir, CLIP, ["--max-frames", str(MAX_FRAMES)] + extra)
    return out_dir / "video" / SCENE


def _stream_through_the_entry_point(pa, blur, adaptive):
    """The clip's first frames drawn through the Python mirror with the float output asked for, made into payloads by the new entry point."""
    import torch

    scene = pa.Scene.from_file(pa.scene_path(SCENE))
    duration = dict(scene.animations())[CLIP]
    count = max(1, int(np.float32(duration) * np.float32(FPS)))
    assert count > MAX_FRAMES
    r = pa.SceneRenderer(scene, device=0, flags=pa.FLAG_REFINE if adaptive is not None else 0)
    r.set_option("aa_count", 4)  # the defaults of `render`
    r.set_option("render_depth", 150)
    scene.init_animation(CLIP)
    r.update(0.0)
    stream = yr.y4m_header(W, H, FPS)
    nbytes = pa.yuv420p10_frame_bytes(W, H)
    for i in range(MAX_FRAMES):
        subs = []
        for j in range(blur):
            r.set_option("aa_start", j)
            r.update((i / count + j / blur / count * 0.5) * float(np.float32(duration)))
            drawn = r.draw_adaptive(W, H, threshold=adaptive, rgba32f=True) if adaptive is not None else r.draw(W, H, rgba8=True, rgba32f=True)
            subs.append(torch.from_numpy(np.ascontiguousarray(drawn["rgba32f"])).cuda())
        out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        pa.average_f32_to_yuv420p10_device([s.data_ptr() for s in subs], out.data_ptr(), W, H, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        payload = out.cpu().numpy().tobytes()
        _assert_same_payload(payload, dr.deep_reference([s.cpu().numpy() for s in subs]), W, H, f"frame {i}")
        stream += b"FRAME\n" + payload
    return stream


@pytest.mark.gpu
@pytest.mark.parametrize("blur,adaptive,more", [(3, None, []), (1, None, []), (3, 4, []), (2, 4, ["--batch-subframes", "0"])])
def test_render_cli_streams_deep_colour_frames(gpu, tmp_path, blur, adaptive, more):
    """`portal-amd render ... --frames y4m --deep-colour` with no ffmpeg on the PATH: <clip>.y4m is the header plus, per frame, FRAME and the
    payload the library makes of the same draws' float output -- batched (blur 3), one sub-frame (blur 1: converted with n = 1), with
    --clip-adaptive-aa 4 batched and, with --batch-subframes 0, as one adaptive draw per sub-frame: the four draw calls of the clip loop.  The start still is the one a run without the option writes: the RGBA8 sub-frames are still drawn."""
    pa = gpu
    extra = ["--motion-blur-frames", str(blur)] + (["--clip-adaptive-aa", str(adaptive)] if adaptive is not None else []) + more
    video = _render_frames(pa, tmp_path / "deep", extra + ["--deep-colour"])
    got = (video / f"{CLIP}.y4m").read_bytes()
    want = _stream_through_the_entry_point(pa, blur, adaptive)
    header, size = yr.y4m_header(W, H, FPS), 6 + yr.frame_bytes(W, H)
    assert got[: len(header)] == header and len(got) == len(header) + MAX_FRAMES * size
    for i in range(MAX_FRAMES):
        at = len(header) + i * size
        assert got[at: at + 6] == b"FRAME\n", i
        _assert_same_payload(got[at + 6: at + size], want[at + 6: at + size], W, H, f"frame {i}")
    assert got == want
    plain = _render_frames(pa, tmp_path / "plain", extra)
    assert (video / f"{CLIP}.start.png").read_bytes() == (plain / f"{CLIP}.start.png").read_bytes()
    eight_bit = (plain / f"{CLIP}.y4m").read_bytes()
    assert len(eight_bit) == len(got) and eight_bit != got  # the option changes the frames, not their form
    y_deep, y_plain = yr.split_planes(got[len(header) + 6: len(header) + size], W, H)[0], yr.split_planes(eight_bit[len(header) + 6: len(header) + size], W, H)[0]
    if blur == 1:  # one quantisation against another of the same floats: at most 3 luma codes apart
        assert np.abs(y_deep.astype(int) - y_plain.astype(int)).max() <= 3
