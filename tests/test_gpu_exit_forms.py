"""The thinned exits of the trace kernel on gfx950 (the host leg and the cases: tests/test_exit_forms.py,
tests/exit_forms_cases.py): both forms of unorm8 on all 2^32 inputs, the 96x54 frames of the four cases against the host build through the
plain, the slices and the refine entry and with a passes build, and the shipped kernels against the same source compiled with
`-DPTL_SPELLED_EXITS`, bit for bit."""
import numpy as np
import pytest

from tests.exit_forms_cases import CASE_IDS, CASES, H, SPELLED, W, host_frame, renderer

pytestmark = pytest.mark.gpu

AA = 2  # two samples per pixel: the refine entry then shades something the first pass did not


@pytest.fixture(scope="module")
def gpu(pa):
    if pa.device_count() < 1:
        pytest.fail("no HIP device visible: the render path has no CPU fallback")
    return pa


def spec(pa):
    return pa.FLAG_SPECIALIZE_INTS | pa.FLAG_SPECIALIZE_ALL


_SWEEP = r"""
#define PTL_COUNT_SEGMENT() ((void)0)
#define PTL_NO_TELEPORT_ENTRY 1
namespace glsl {
struct ptl_uniform_block { int what_u; int pad_u; };
__constant__ ptl_uniform_block ptl_u;
// pixel (x, y) of a 4096 x 256 frame = one of 2^20 threads, each walking 4096 consecutive bit patterns: all 2^32 floats.
PTL_FN vec4 shade_pixel(vec2 position) {
    const unsigned base = ((unsigned)position.y * 4096u + (unsigned)position.x) << 12;
    unsigned bad = 0, first = 0, zeros = 0, full = 0;
    for (unsigned k = 0; k < 4096u; ++k) {
        float x = __builtin_bit_cast(float, base + k);
        asm volatile("" : "+v"(x));   // a run-time value: the instructions, not the compiler's constant folding
        const unsigned a = ptl_unorm8_spelled(x), b = ptl_unorm8_clamped(x);
        const bool differ = a != b;
        bad += differ;
        zeros += b == 0u;
        full += b == 255u;
        if (differ && first == 0) first = base + k;
    }
    return vec4((float)bad, __builtin_bit_cast(float, first), (float)zeros, (float)full);
}
PTL_FN unsigned int pack_rgba8(vec4 c) { return 0u; }
}  // namespace glsl
"""


def test_both_unorm8_forms_agree_on_every_input(gpu):
    """ALL 2^32 bit patterns -- normals, subnormals, zeros, infinities, every NaN -- through the spelled form and the v_med3 form on the
    device: not one mismatch, and the codes add up to what the definition gives (so the loop really ran the forms)."""
    pa = gpu
    k = pa.Kernel(pa.device_source("glsl") + _SWEEP + pa.device_source("entry"), [("what_u", 2, 0), ("pad_u", 2, 4)], 8, device=0)
    out = k.render(4096, 256, rgba8=False, rgba32f=True)
    got = out["rgba32f"].reshape(-1, 4)
    bad, first = got[:, 0].astype(np.float64).sum(), got[:, 1].view(np.uint32)
    assert not bad, f"{bad:.0f} of 2^32 inputs differ, e.g. bit pattern {hex(int(first[first != 0][0]))}"
    # ... and the loop really ran the forms: how many inputs give 0 and how many 255, counted on the host from the two borders
    def code(bits):  # the definition; v * 255 + 0.5 is exact in binary64 near both borders, so the cast rounds once like the fma
        v = np.array([bits], np.uint32).view(np.float32)[0]
        return int(np.floor(np.float32(np.float64(v) * 255.0 + 0.5))) if 0 < v < 1 else (255 if v >= 1 else 0)

    def first_with(c, near):
        b = int(np.array([near], np.float32).view(np.uint32)[0])
        while code(b) >= c:
            b -= 1
        while code(b) < c:
            b += 1
        return b

    first_1, first_255 = first_with(1, 0.5 / 255.0), first_with(255, 254.5 / 255.0)
    want_zeros = (1 << 31) + first_1 + ((1 << 23) - 1)  # every pattern with the sign bit, +0 up to the first border, the positive NaNs
    want_full = 0x7F800000 - first_255 + 1  # up to +inf
    assert got[:, 2].astype(np.float64).sum() == want_zeros and got[:, 3].astype(np.float64).sum() == want_full
    print(f"unorm8: both forms agree on all 2^32 inputs ({out['ms']:.1f} ms)")


def draw(pa, r, entry):
    """-> (float bits, rgba8) of the W x H frame through `entry` of a renderer built for it."""
    if entry == "refine":  # threshold -1: every pixel is on the refine list, the frame is the refine entry's
        f = r.draw_adaptive(W, H, threshold=-1, rgba32f=True)
        assert f["count"] == W * H
    elif entry == "passes":
        f = r.draw_passes(W, H, rgba8=True, rgba32f=True)
    else:  # plain; slices: a single draw of such a renderer is a batch of one
        f = r.draw(W, H, rgba8=True, rgba32f=True)
    return f["rgba32f"].view(np.uint32).copy(), f["rgba8"].copy(), f


def entry_flags(pa, entry):
    return spec(pa) | {"plain": 0, "slices": pa.FLAG_SLICES, "refine": pa.FLAG_REFINE, "passes": pa.FLAG_PASSES}[entry]


@pytest.mark.parametrize("entry", ["plain", "slices", "refine", "passes"])
@pytest.mark.parametrize("name,scene_file,depth", CASES, ids=CASE_IDS)
def test_frames_match_the_host_build_through_every_entry(gpu, monkeypatch, name, scene_file, depth, entry):
    pa = gpu
    monkeypatch.delenv("PTL_HIPRTC_FLAGS", raising=False)
    want = host_frame(pa, scene_file, depth, spec(pa), aa_count=AA)
    _, r = renderer(pa, scene_file, depth, entry_flags(pa, entry), 0, aa_count=AA)
    bits, rgba8, _ = draw(pa, r, entry)
    assert np.array_equal(bits, want[0]), f"{name} {entry}: {int((bits != want[0]).any(axis=2).sum())} of {W * H} pixels differ from the host build"
    assert np.array_equal(rgba8, want[1])  # (the host build packs with the spelled unorm8, the device with v_med3)


@pytest.mark.parametrize("entry", ["plain", "passes"])
@pytest.mark.parametrize("name,scene_file,depth", CASES, ids=CASE_IDS)
def test_spelled_exits_change_no_bit_on_the_gpu(gpu, monkeypatch, name, scene_file, depth, entry):
    """The shipped kernel and the same source with `-DPTL_SPELLED_EXITS`: two binaries, one frame -- and with a passes build one record per pixel."""
    pa = gpu
    monkeypatch.delenv("PTL_HIPRTC_FLAGS", raising=False)
    _, r = renderer(pa, scene_file, depth, entry_flags(pa, entry), 0, aa_count=AA)
    shipped = draw(pa, r, entry)
    monkeypatch.setenv("PTL_HIPRTC_FLAGS", "-D" + SPELLED)
    _, r_spelled = renderer(pa, scene_file, depth, entry_flags(pa, entry), 0, aa_count=AA)
    spelled = draw(pa, r_spelled, entry)
    assert r.code_object_sha256() != r_spelled.code_object_sha256()  # the define reached the compile
    assert np.array_equal(shipped[0], spelled[0]) and np.array_equal(shipped[1], spelled[1])
    if entry == "passes":
        assert np.array_equal(np.asarray(shipped[2]["passes"]).view(np.uint8), np.asarray(spelled[2]["passes"]).view(np.uint8))


@pytest.mark.parametrize("size", [(W, H), (328, 186)], ids=["96x54", "328x186"])
def test_the_headline_build_draws_the_same_frame_with_and_without_the_define(gpu, monkeypatch, size):
    pa = gpu
    flags = spec(pa) | pa.flag_waves(5)
    frames, shas = [], []
    for env in (None, "-D" + SPELLED):
        if env:
            monkeypatch.setenv("PTL_HIPRTC_FLAGS", env)
        else:
            monkeypatch.delenv("PTL_HIPRTC_FLAGS", raising=False)
        _, r = renderer(pa, "scenes/portal_in_portal.ron", 40, flags, 0)
        f = r.draw(*size, rgba8=True, rgba32f=True)
        frames.append((f["rgba32f"].view(np.uint32).copy(), f["rgba8"].copy()))
        shas.append(r.code_object_sha256())
    assert shas[0] != shas[1]
    assert np.array_equal(frames[0][0], frames[1][0]) and np.array_equal(frames[0][1], frames[1][1])
    assert len(np.unique(frames[0][1].reshape(-1, 4), axis=0)) > 8
