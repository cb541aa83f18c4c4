"""tests/contract_sweep.py -- stratified inputs for the numerics contract (beside tests/probe.py, whose functions and
input format it uses): 2^20 (a, b, c) triples aimed at the places where range-reduced polynomial kernels go wrong and where
two compilers can part ways -- every exponent field, every comparison constant of ptl_glsl.h, the trig cancellation points,
integers and half-integers, and a block built for the multi-argument functions.  Seeded and deterministic.

Also here: the kernel that evaluates four probe functions per pixel (so that a frame stays small), the table of vector
overloads against their scalar builtins, and the directed `texture()` cases.
"""
import functools
import os
import re

import numpy as np

from tests import probe

F32, U32 = np.float32, np.uint32
N_TOTAL = 1 << 20          # triples in the sweep (block 1 fills what block 2 leaves)
N_BLOCK2_MAX = 1 << 16
SEED = 20240607
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "portal_amd", "csrc", "device", "ptl_glsl.h")

# Inputs that once showed a difference or a wrong bound, kept by name (a, b, c); block 2 starts with them.
FIXED_POINTS = [
    ("atan_2.29ulp_above_the_tan_pi_8_knot", (0.41421542, 1.0, 0.0)),
    ("atan_3.23ulp_worst_of_the_middle_branch", (0.43229637, 1.0, 0.0)),      # from an exhaustive search of (tan(pi/8), tan(3pi/8)]
    # just below sqrt(1/2), where the log polynomial's argument is largest and its top coefficient decides the last bit (found by comparing the
    # host build with one whose coefficient 7.0376836292e-2 was moved by one binary32 step, over every number of [0.5, 1))
    ("log_top_coefficient_decides", (0.70668787, 1.0, 0.0)),
    ("log2_top_coefficient_decides", (0.6990319, 1.0, 0.0)),
]


def from_bits(u):
    return (np.asarray(u, np.int64) & 0xFFFFFFFF).astype(U32).view(F32)


def bits_of(x):
    return np.ascontiguousarray(x, dtype=F32).view(U32).astype(np.int64)


def around(values, ulps, both_signs=True):
    """The binary32 neighbours of |values| within +-ulps steps of the bit pattern (clipped at +0 and +inf), in both signs."""
    m = bits_of(np.abs(np.asarray(values, F32))).reshape(-1, 1) + np.arange(-ulps, ulps + 1).reshape(1, -1)
    m = np.clip(m, 0, 0x7F800000).reshape(-1)
    return from_bits(np.concatenate([m, m | 0x80000000]) if both_signs else m)


def header_comparison_constants():
    """|literal| of every floating-point literal that ptl_glsl.h compares something with (`x > 2.414213562373095f`, `m < 0x1p-126f` ...),
    rounded to binary32 as the compilers round it."""
    from oracle import glsl_math as M

    text = open(HEADER).read()
    text = re.sub(r"//[^\n]*", "", text)
    found = re.findall(r"(?:[<>]=?|[=!]=)\s*(-?(?:0x[0-9a-fA-F.]+p[+-]?\d+|\d+\.\d*(?:e[+-]?\d+)?|\.\d+))f\b", text)
    vals = sorted({float(np.abs(M.lit(t))) for t in found})
    return np.array(vals, F32)


# what the generator must find in the header at the least (the knots named when the sweep was designed)
KNOWN_KNOTS = ["2.414213562373095", "0.4142135623730950", "0.5", "1.0", "0.707106781186547524", "128.0", "150.0", "88.72283905206835",
               "103.972076416015625", "0x1p-126", "0x1p-100", "0x1p-96", "0x1p+126"]


def _exponent_fields(rng, n_random):
    fixed = np.array([0, 1, 2, 3, 0x3FFFFF, 0x400000, 0x400001, 0x7FFFFD, 0x7FFFFE, 0x7FFFFF, 0x3504F2, 0x3504F3, 0x3504F4], np.int64)
    fields = np.arange(512, dtype=np.int64).reshape(-1, 1) << 23
    out = [(fields | fixed.reshape(1, -1)).reshape(-1)]
    if n_random > 0:
        out.append((fields | rng.integers(0, 1 << 23, (512, n_random), dtype=np.int64)).reshape(-1))
    return from_bits(np.concatenate(out))


def _trig_points():
    k = np.unique(np.concatenate([np.arange(1, 4097), np.round(2.0 ** np.linspace(12, 30, 4000)).astype(np.int64)])).astype(np.float64)
    x = np.concatenate([k * (np.pi / 2), k * (np.pi / 2) + np.pi / 4]).astype(F32)
    return around(x, 4)


def _integer_points():
    n = np.arange(-152, 131, dtype=np.float64)
    # (n and n + 1/2: where exp2's rint and fract / mod's floor step; n / ln 2; n ln 2 and (n + 1/2) ln 2: where exp's floor(x log2(e) + 1/2) steps)
    return np.concatenate([around(n.astype(F32), 2), around((n + 0.5).astype(F32), 3), around((n / np.log(2.0)).astype(F32), 3),
                           around((n * np.log(2.0)).astype(F32), 3), around(((n + 0.5) * np.log(2.0)).astype(F32), 3)])


def block1_a(rng, size):
    """The `a` column of block 1: `size` values."""
    from oracle import glsl_math as M

    consts = header_comparison_constants()
    missing = [t for t in KNOWN_KNOTS if float(np.abs(M.lit(t))) not in set(consts.tolist())]
    assert not missing, f"comparison constants not found in ptl_glsl.h: {missing}"
    directed = np.concatenate([_exponent_fields(rng, 0), around(consts, 16), _trig_points(), _integer_points()])
    directed = from_bits(np.unique(bits_of(directed)))
    left = size - len(directed)
    assert left >= 512 * 64, "the directed sets leave no room for random mantissas"
    per_field = left // 512
    rand = _exponent_fields(rng, per_field)[512 * 13:]
    raw = from_bits(rng.integers(0, 1 << 32, left - len(rand), dtype=np.int64))
    a = np.concatenate([directed, rand, raw])
    assert len(a) == size
    return a


# ---- block 2: triples built for the multi-argument functions ----------------------------------------------------------------------
def _triples(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return np.stack([a.reshape(-1), b.reshape(-1), c.reshape(-1)], axis=1)


def _grid(*axes):
    return [g.reshape(-1) for g in np.meshgrid(*[np.asarray(x, F32) for x in axes], indexing="ij")]


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38,
                     3.4028235e38, -3.4028235e38, 0.5, -0.5, 2.0, -2.0, 8.5070592e37, -8.5070592e37, 1.7014118e38, -1.7014118e38, 3.0, -1e-20, 1e20], F32)


def _atan2_block(rng):
    y, x = _grid(SPECIALS, SPECIALS)
    out = [_triples(y, x, rng.choice(SPECIALS, len(y)))]
    knots = around(np.array([2.414213562373095, 0.4142135623730950, 1.0], F32), 4, both_signs=False)
    scales = np.concatenate([2.0 ** np.array([-140, -126, -100, -30, -1, 0, 1, 24, 100, 126], np.float64), 10.0 ** rng.uniform(-20, 20, 6)]).astype(F32)
    t, s, sy, sx = _grid(knots, scales, [1, -1], [1, -1])
    with np.errstate(all="ignore"):
        out.append(_triples(sy * (t * s), sx * s, t))
    return np.concatenate(out)


def _pow_block(rng):
    bases = np.concatenate([np.array([2.0, 0.5, 10.0, 0.1, 1.5, 2.7182817, 3e-5, 1e30, 1e-30, 1e-40, 1e-45, 3.4028235e38, 1.1754944e-38, 0.99999994, 1.0000001, 0.70710677,
                                      0.70710683, 1.4142135], F32), (10.0 ** rng.uniform(-38, 38, 14)).astype(F32)])
    targets = np.array([128.0, -150.0, 127.0, -126.0, -149.0, -127.0, 0.5, -0.5, 1.0], np.float64)
    a, t, d = _grid(bases, targets, np.arange(-6, 7))
    with np.errstate(all="ignore"):
        b0 = (t.astype(np.float64) / np.log2(a.astype(np.float64))).astype(F32)
    ok = np.isfinite(b0)
    b = from_bits(np.clip(bits_of(np.abs(b0[ok])) + d[ok].astype(np.int64), 0, 0x7F800000) | (bits_of(b0[ok]) & 0x80000000))
    out = [_triples(a[ok], b, d[ok]), _triples(-a[ok], b, d[ok])]
    ea, eb = _grid(np.array([0.0, -0.0, 1.0, np.inf, -np.inf, np.nan, 0.99999994, 1.0000001, 1e-45, 3.4028235e38, 2.0, 0.5], F32),
                   np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, 0.5, 2.0, -2.0, 1e-45, -1e-45, 3.4028235e38, -3.4028235e38, 127.0, 128.0, -149.0, -150.0], F32))
    out.append(_triples(ea, eb, 0.0))
    return np.concatenate(out)


def _mod_block(rng):
    ys = np.concatenate([np.array([1.0, 2.0, 0.1, 3.0, 1e-3, 3.1415927, 6.2831855, 7.5, 1e10, 1e-30, 1.1754944e-38, 1e-40, 0.33333334, 360.0], F32),
                         (10.0 ** rng.uniform(-6, 6, 10)).astype(F32)])
    ys = np.concatenate([ys, -ys])
    ms = np.concatenate([np.arange(-12, 13), rng.integers(-100000, 100000, 20), np.array([1 << 23, -(1 << 23), (1 << 24) + 2, 8388607])]).astype(np.float64)
    y, m, d = _grid(ys, ms, np.arange(-2, 3))
    x0 = (m.astype(np.float64) * y.astype(np.float64)).astype(F32)
    x = from_bits(np.clip(bits_of(np.abs(x0)) + d.astype(np.int64), 0, 0x7F800000) | (bits_of(x0) & 0x80000000))
    return _triples(x, y, m)


def _fma_block(rng):
    out = []
    n = 3000
    # products that cancel c to within a few ulps, over the whole exponent range
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)).astype(F32)
    with np.errstate(all="ignore"):
        p = (a.astype(np.float64) * b.astype(np.float64)).astype(F32)
    c = -from_bits(np.clip(bits_of(np.abs(p)) + rng.integers(-3, 4, n), 0, 0x7F800000) | (bits_of(p) & 0x80000000))
    out.append(_triples(a, b, c))
    # results in the subnormal range: product 2^-152 .. 2^-124, c zero, subnormal or a small normal of either sign
    a = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(-80, -60, n) * rng.choice([-1, 1], n)).astype(F32)
    b = (rng.uniform(1, 2, n) * 2.0 ** (rng.integers(-152, -123, n) - np.floor(np.log2(np.abs(a.astype(np.float64)))))).astype(F32)
    c = from_bits(rng.integers(0, 0x01000000, n) | (rng.integers(0, 2, n) << 31))
    c[::3] = 0.0
    c[1::9] = -0.0
    out.append(_triples(a, b, c))
    # the overflow boundary: product within a few ulps of 2^128, c pulling it back under or pushing it over
    a = (rng.uniform(1, 2, n) * 2.0 ** rng.integers(30, 90, n)).astype(F32)
    t = from_bits(0x7F7FFFFF - rng.integers(0, 4, n)).astype(np.float64) * rng.choice([1.0, 1.0 + 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -22], n)
    b = (t / a.astype(np.float64)).astype(F32)
    c = (rng.choice([0.0, 1.0, -1.0, 0.5, -0.5, 0.25, -0.25, 2.0, -2.0], n) * 2.0 ** 104).astype(F32)
    s = rng.choice([-1, 1], n).astype(F32)
    out.append(_triples(a * s, b, c * s))
    # exact ties of the sum: c = M * u with M in [2^23, 2^24), a * b = (odd) * u / 2, the sum stays in c's binade
    e = rng.integers(-100, 100, n)
    u = 2.0 ** e.astype(np.float64)
    mant = rng.integers((1 << 23) + 4096, (1 << 24) - 4096, n).astype(np.float64)
    j = (2 * rng.integers(0, 1024, n) + 1).astype(np.float64)
    k = (2 * rng.integers(0, 16, n) + 1).astype(np.float64)
    s = rng.choice([-1.0, 1.0], n)
    out.append(_triples(j * u / 2 * s, k, mant * u))
    # ... and ties missed by a tail that binary64 cannot hold beside c (the oracle's round-to-odd step decides): a * b = u / 2 * (1 - 2^-46),
    # just under the tie, or u / 2 * (1 + 2^-36), just over it -- (1 + x)(1 - x) and (1 + x)(1 - x + x^2), every factor a binary32 number
    # exact zeros: a product of two 12-bit numbers against its own negative (+0), and zero products of either sign beside zeros of either sign
    m = 900
    za = (rng.integers(1, 4096, m) * 2.0 ** rng.integers(-50, 50, m) * rng.choice([-1.0, 1.0], m)).astype(F32)
    zb = (rng.integers(1, 4096, m) * 2.0 ** rng.integers(-50, 50, m)).astype(F32)
    zc = -(za.astype(np.float64) * zb.astype(np.float64)).astype(F32)
    zero = rng.integers(0, 3, m) == 0
    za[zero] = rng.choice(np.array([0.0, -0.0], F32), int(zero.sum()))
    zc[zero] = rng.choice(np.array([0.0, -0.0], F32), int(zero.sum()))
    out.append(_triples(za, zb, zc))
    under = rng.integers(0, 2, n) == 0
    fa = np.where(under, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -12)
    fb = np.where(under, 1.0 - 2.0 ** -23, 1.0 - 2.0 ** -12 + 2.0 ** -24)
    out.append(_triples(u / 2 * s * fa, fb, mant * u * rng.choice([-1.0, 1.0], n)))
    return np.concatenate(out)


def _smoothstep_block(rng):
    v = np.array([0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 1e-45, 1.1754944e-38, 1e-30, 1e30, 3.4028235e38, -3.4028235e38, np.inf, -np.inf, np.nan, 0.1, 0.3, 7.0], F32)
    e0, e1, w = _grid(v, v, np.arange(8))
    with np.errstate(all="ignore"):
        mid = (0.5 * e0.astype(np.float64) + 0.5 * e1.astype(np.float64)).astype(F32)
        x = np.select([w == 0, w == 1, w == 2, w == 3, w == 4, w == 5, w == 6], [e0, e1, mid, np.nextafter(e0, F32(np.inf)), np.nextafter(e1, F32(-np.inf)),
                                                                                  np.nextafter(e0, F32(-np.inf)), np.nextafter(e1, F32(np.inf))], default=(e0 + e1).astype(F32))
    return _triples(e0, e1, x.astype(F32))       # every (e0, e1) pair: equal, reversed and ordered edges


def _vector_block(rng):
    mags = np.array([2.0 ** 63, 2.0 ** 64, 1.8446743e19, 1.8446744e19, 1.3043817e19, 1e19, 3e19, 2.0 ** 127, 2.0 ** -75, 2.0 ** -74, 2.0 ** -63, 1e-23, 8.8817842e-16, 8.881785e-16,
                     1.0842022e-19, 1.0], F32)
    v = np.concatenate([mags[:12], -mags[:12]])
    a, b, c = _grid(v, v, v)
    extra = _triples(*_grid(np.concatenate([mags, -mags]), [0.0, -0.0, np.inf, np.nan, 1e-45], np.concatenate([mags[::3], -mags[::3]])))
    return np.concatenate([_triples(a, b, c), extra])


def _equal_block(rng, a_col):
    x = rng.choice(a_col, 1024)
    y = rng.choice(a_col, 1024)
    return np.concatenate([_triples(x, x, x), _triples(x, x, y), _triples(x, y, x), _triples(y, x, x), _triples(x, -x, y)])


@functools.lru_cache(maxsize=None)
def _build():
    rng = np.random.default_rng(SEED)
    fixed = np.array([p for _, p in FIXED_POINTS], F32).reshape(-1, 3)
    parts = [("fixed", fixed), ("atan2", _atan2_block(rng)), ("pow", _pow_block(rng)), ("mod", _mod_block(rng)), ("fma", _fma_block(rng)),
             ("smoothstep", _smoothstep_block(rng)), ("vector", _vector_block(rng))]
    a = block1_a(rng, N_TOTAL - N_BLOCK2_MAX)
    parts.append(("equal", _equal_block(rng, a)))
    block2 = np.concatenate([p for _, p in parts]).astype(F32)
    assert len(block2) <= N_BLOCK2_MAX, len(block2)
    pad = rng.integers(0, 1 << 32, (N_BLOCK2_MAX - len(block2), 3), dtype=np.int64)
    block2 = np.concatenate([block2, from_bits(pad.reshape(-1)).reshape(-1, 3)])
    block1 = np.stack([a, a[rng.permutation(len(a))], a[rng.permutation(len(a))]], axis=1)
    out = np.ascontiguousarray(np.concatenate([block2, block1]), dtype=F32)
    assert out.shape == (N_TOTAL, 3)
    out.setflags(write=False)
    where, at = {}, 0
    for name, p in parts:
        where[name] = (at, at + len(p))
        at += len(p)
    return out, where


def sweep():
    """float32 (2^20, 3), read-only: block 2 (the multi-argument cases, 2^16 rows) followed by block 1."""
    return _build()[0]


def block(name):
    """The rows of one named part of block 2 ("fma", "pow", "atan2", "mod", "smoothstep", "vector", "equal", "fixed")."""
    lo, hi = _build()[1][name]
    return sweep()[lo:hi]


# ---- the kernel: four functions per pixel -------------------------------------------------------------------------------------------
FRAME_W = 4096
CHUNK = 1 << 18                         # samples per rendered frame: 4096 x (64 * 9) pixels x 16 B = 36 MiB of RGBA32F


def groups():
    return (len(probe.functions()) + 3 + 3) // 4      # the functions, then an echo of a, b, c


def source(pa):
    fns = probe.functions()
    cases = "\n".join(f"        case {k}: return {expr};  // {name}" for k, (name, expr, _) in enumerate(fns))
    n = len(fns)
    return (
        pa.device_source("glsl")
        + """
#define PTL_COUNT_SEGMENT() ((void)0)
#define PTL_NO_TELEPORT_ENTRY 1
namespace glsl {
struct ptl_uniform_block { sampler2D in_tex; int base_u; int count_u; };
#if PTL_DEVICE_BUILD
__constant__ ptl_uniform_block ptl_u;
#else
ptl_uniform_block ptl_u;
#endif
PTL_FN float probe(int fn, float a, float b, float c) {
    switch (fn) {
"""
        + cases
        + f"""
        case {n}: return a;
        case {n + 1}: return b;
        case {n + 2}: return c;
        default: return 0.0f;
    }}
}}
PTL_FN vec4 shade_pixel(vec2 position) {{
    const int x = (int)position.x, y = (int)position.y, g = y % {groups()};
    const int i = ptl_u.base_u + x + {FRAME_W} * (y / {groups()});
    if (i < 0 || i >= ptl_u.count_u) return vec4(0.0f);
    const float* in = reinterpret_cast<const float*>(ptl_u.in_tex.texels);
    const float a = in[3 * i], b = in[3 * i + 1], c = in[3 * i + 2];
    return vec4(probe(4 * g, a, b, c), probe(4 * g + 1, a, b, c), probe(4 * g + 2, a, b, c), probe(4 * g + 3, a, b, c));
}}
PTL_FN unsigned int pack_rgba8(vec4 c) {{ return 0u; }}
}}  // namespace glsl
"""
        + pa.device_source("entry")
    )


LAYOUT = [("in_tex", 5, 0), ("base_u", 2, 16), ("count_u", 2, 20)]
BLOCK_SIZE = 24


def run(samples, bind_texture, set_int, render):
    """Drive one compiled kernel (host build or GPU) over `samples` in chunks; -> (functions, len(samples)) float32 results.
    `render(w, h)` returns the RGBA32F frame.  The echo rows prove that the inputs arrived intact."""
    n, g, nf = len(samples), groups(), len(probe.functions())
    bind_texture(probe.as_texture(np.ascontiguousarray(samples)))
    set_int("count_u", n)
    out = np.empty((4 * g, n), F32)
    for base in range(0, n, CHUNK):
        m = min(CHUNK, n - base)
        rows = -(-m // FRAME_W)
        set_int("base_u", base)
        frame = render(FRAME_W, rows * g).reshape(rows, g, FRAME_W, 4)
        out[:, base:base + m] = frame.transpose(1, 3, 0, 2).reshape(4 * g, rows * FRAME_W)[:, :m]
    echo = out[nf:nf + 3].T
    assert np.array_equal(echo.view(U32), np.ascontiguousarray(samples).view(U32)), "the inputs did not arrive intact"
    return out[:nf]


def run_host(pa, samples, defines=()):
    from oracle import host_build as hb

    hk = hb.HostKernel(source(pa), LAYOUT, BLOCK_SIZE, defines=tuple(defines))
    return run(samples, lambda t: hk.set_texture("in_tex", t), hk.set_uniform, lambda w, h: hk.render(w, h, rgba8=False)["rgba32f"])


def run_gpu(pa, samples, defines=()):
    k = pa.Kernel(source(pa), LAYOUT, BLOCK_SIZE, device=0, defines=tuple(defines))
    return run(samples, lambda t: k.set_texture("in_tex", t), lambda name, v: k.set_uniform(name, pa.PTL_I32, v),
               lambda w, h: k.render(w, h, rgba8=False, rgba32f=True)["rgba32f"])


def numpy_results(samples, contract=2):
    from oracle import glsl_math as M

    previous = M.set_contract(contract)
    try:
        return probe.numpy_results(samples)
    finally:
        M.set_contract(previous)


def mismatches(got, want, samples, who):
    """One line per function whose results differ: name, count, the first offending input with its bit patterns."""
    lines = []
    for k, (name, _, _) in enumerate(probe.functions()):
        bad = np.nonzero(~probe.same_bits(got[k], want[k]))[0]
        if len(bad):
            i = bad[0]
            s = samples[i]
            lines.append(f"{name}: {len(bad)} of {len(samples)} differ, first at row {i}: (a, b, c) = {tuple(float(v) for v in s)} "
                         f"bits {[hex(int(v)) for v in s.view(U32)]} -> {who} {got[k][i]!r} ({hex(int(got[k][i:i + 1].view(U32)[0]))}) "
                         f"numpy {want[k][i]!r} ({hex(int(want[k][i:i + 1].view(U32)[0]))})")
    return lines


# ---- vector overloads ---------------------------------------------------------------------------------------------------------------
COMPONENTS = "xyzw"
MAP1 = ["sin", "cos", "tan", "asin", "acos", "atan", "exp", "log", "exp2", "log2", "sqrt", "inversesqrt", "abs", "sign", "floor", "ceil", "fract", "trunc", "round",
        "roundEven", "radians", "degrees"]
MAP2 = ["min", "max", "mod", "pow", "atan", "step"]
MAP2S = ["min", "max", "mod"]


def overload_rows():
    """(vector expression, its component, the scalar expression it must equal) over float p[4], q[4], r[4]: every vec2 / vec3 / vec4
    overload of the component-wise builtins that ptl_glsl.h spells out, each component on its own."""
    rows = []
    for n in (2, 3, 4):
        vec = lambda s: f"vec{n}(" + ", ".join(f"{s}[{i}]" for i in range(n)) + ")"
        P, Q, R = vec("p"), vec("q"), vec("r")
        for i in range(n):
            at = lambda s: f"{s}[{i}]"
            rows += [(f"{f}({P})", i, f"{f}({at('p')})") for f in MAP1]
            rows += [(f"{f}({P}, {Q})", i, f"{f}({at('p')}, {at('q')})") for f in MAP2]
            rows += [(f"{f}({P}, q[0])", i, f"{f}({at('p')}, q[0])") for f in MAP2S]
            rows += [(f"step(q[0], {P})", i, f"step(q[0], {at('p')})"),
                     (f"clamp({P}, q[0], r[0])", i, f"clamp({at('p')}, q[0], r[0])"),
                     (f"clamp({P}, {Q}, {R})", i, f"clamp({at('p')}, {at('q')}, {at('r')})"),
                     (f"mix({P}, {Q}, r[0])", i, f"mix({at('p')}, {at('q')}, r[0])"),
                     (f"mix({P}, {Q}, {R})", i, f"mix({at('p')}, {at('q')}, {at('r')})"),
                     (f"smoothstep(q[0], r[0], {P})", i, f"smoothstep(q[0], r[0], {at('p')})"),
                     (f"smoothstep({P}, {Q}, {R})", i, f"smoothstep({at('p')}, {at('q')}, {at('r')})")]
    return rows


def overload_source(pa):
    """Pixel (x, y): sample x, row y -> (component of the vector overload, the scalar builtin on that component, 0, 0).  The vectors are
    p = (a, b, c, d), q = (b, c, d, a), r = (c, d, a, b) with d the next sample's a: four different numbers, so a wrong component letter shows."""
    cases = "\n".join(f"        case {k}: return vec2(({v}).{COMPONENTS[i]}, {s});" for k, (v, i, s) in enumerate(overload_rows()))
    return (
        pa.device_source("glsl")
        + """
#define PTL_COUNT_SEGMENT() ((void)0)
#define PTL_NO_TELEPORT_ENTRY 1
namespace glsl {
struct ptl_uniform_block { sampler2D in_tex; int base_u; int count_u; };
#if PTL_DEVICE_BUILD
__constant__ ptl_uniform_block ptl_u;
#else
ptl_uniform_block ptl_u;
#endif
PTL_FN vec2 overload(int row, const float* p, const float* q, const float* r) {
    switch (row) {
"""
        + cases
        + """
        default: return vec2(0.0f, 1.0f);
    }
}
PTL_FN vec4 shade_pixel(vec2 position) {
    const int i = (int)position.x, row = ptl_u.base_u + (int)position.y;
    if (i < 0 || i >= ptl_u.count_u) return vec4(0.0f);
    const float* in = reinterpret_cast<const float*>(ptl_u.in_tex.texels);
    const float a = in[3 * i], b = in[3 * i + 1], c = in[3 * i + 2], d = in[3 * ((i + 1) % ptl_u.count_u)];
    const float p[4] = {a, b, c, d}, q[4] = {b, c, d, a}, r[4] = {c, d, a, b};
    const vec2 o = overload(row, p, q, r);
    return vec4(o.x, o.y, a, d);
}
PTL_FN unsigned int pack_rgba8(vec4 c) { return 0u; }
}  // namespace glsl
"""
        + pa.device_source("entry")
    )


def overload_samples(n=4096):
    """A 4096-triple slice of the sweep: block 2's directed rows and block 1's directed values, interleaved by a fixed stride."""
    s = sweep()
    idx = np.concatenate([np.arange(0, N_BLOCK2_MAX, N_BLOCK2_MAX // (n // 2))[: n // 2], N_BLOCK2_MAX + np.arange(0, 400000, 400000 // (n // 2))[: n // 2]])
    return np.ascontiguousarray(s[idx])


def check_overloads(samples, frame):
    """frame: (rows, n, 4) float32 from overload_source.  -> list of failure lines (empty when every row agrees)."""
    rows = overload_rows()
    assert frame.shape[:2] == (len(rows), len(samples))
    assert np.array_equal(frame[0, :, 2].view(U32), samples[:, 0].view(U32)) and np.array_equal(frame[0, :, 3].view(U32), np.roll(samples[:, 0], -1).view(U32))
    lines = []
    for k, (v, i, s) in enumerate(rows):
        bad = np.nonzero(~probe.same_bits(frame[k, :, 0], frame[k, :, 1]))[0]
        if len(bad):
            j = bad[0]
            lines.append(f"({v}).{COMPONENTS[i]} != {s}: {len(bad)} of {len(samples)} differ, first at sample {j} (a, b, c) = {samples[j]} "
                         f"bits {[hex(int(t)) for t in samples[j].view(U32)]}: {frame[k, j, 0]!r} vs {frame[k, j, 1]!r}")
    return lines


# ---- texture() ----------------------------------------------------------------------------------------------------------------------
TEXTURE_SHAPES = [(1, 1), (2, 3), (5, 1), (4, 4)]   # (width, height)


def texture_cases():
    """[(texels uint8 (H, W, 4) or None for an unbound sampler, uv float32 (n, 2))]"""
    rng = np.random.default_rng(SEED + 1)
    one = F32(1.0)
    common = [F32(0.0), np.nextafter(F32(0.0), F32(1.0)), -np.nextafter(F32(0.0), F32(1.0)), F32(-0.0), one, np.nextafter(one, F32(0.0)), np.nextafter(one, F32(2.0)),
              F32(-0.25), F32(1.25), F32(1e30), F32(-1e30), F32(np.inf), F32(-np.inf), F32(np.nan)]

    def axis(n):
        centres = [(i + 0.5) / n for i in range(n)]
        edges = [i / n for i in range(n + 1)]
        return np.array(centres + edges + common, F32)

    out = []
    for w, h in TEXTURE_SHAPES:
        tex = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
        us = np.concatenate([axis(w), np.array([w, h], F32)])
        vs = np.concatenate([axis(h), np.array([w, h], F32)])
        u, v = np.meshgrid(us, vs, indexing="ij")
        out.append((tex, np.ascontiguousarray(np.stack([u.reshape(-1), v.reshape(-1)], axis=1), dtype=F32)))
    out.append((None, out[-1][1][::7].copy()))
    return out


TEXTURE_LAYOUT = [("tex", 5, 0), ("in_tex", 5, 16), ("never_bound_tex", 5, 32), ("count_u", 2, 48), ("unbound_u", 2, 52)]
TEXTURE_BLOCK_SIZE = 56
# |numpy oracle - binary64 bilinear| over texture_cases(), measured on the CPU (tests/test_math_contract.py asserts the measurement): 1.34e-7
# (three binary32 mixes of values in [0, 1] and the rounding of byte / 255); twice that is what any build may differ from binary64 by.
TEXTURE_MEASURED = 1.34e-7
TEXTURE_TOLERANCE = 2 * TEXTURE_MEASURED


def texture_source(pa):
    return (
        pa.device_source("glsl")
        + """
#define PTL_COUNT_SEGMENT() ((void)0)
#define PTL_NO_TELEPORT_ENTRY 1
namespace glsl {
struct ptl_uniform_block { sampler2D tex; sampler2D in_tex; sampler2D never_bound_tex; int count_u; int unbound_u; };
#if PTL_DEVICE_BUILD
__constant__ ptl_uniform_block ptl_u;
#else
ptl_uniform_block ptl_u;
#endif
PTL_FN vec4 shade_pixel(vec2 position) {
    const int i = (int)position.x;
    if (i < 0 || i >= ptl_u.count_u) return vec4(0.0f);
    const float* in = reinterpret_cast<const float*>(ptl_u.in_tex.texels);
    const vec2 uv = vec2(in[2 * i], in[2 * i + 1]);
    return ptl_u.unbound_u != 0 ? texture(ptl_u.never_bound_tex, uv) : texture(ptl_u.tex, uv);
}
PTL_FN unsigned int pack_rgba8(vec4 c) { return 0u; }
}  // namespace glsl
"""
        + pa.device_source("entry")
    )


def texture_oracle(tex, uv):
    from oracle import glsl_values as V

    r = V.texture(None if tex is None else V.Sampler(tex), V.Vec([uv[:, 0], uv[:, 1]]))
    return np.stack([np.broadcast_to(np.asarray(c, F32), (len(uv),)) for c in r.c], axis=1)


def texture_binary64(tex, uv):
    """Bilinear, clamp-to-edge, texel centres at +0.5, NaN coordinate -> 0, in binary64 and in its own words."""
    if tex is None:
        return np.tile(np.array([0.0, 0.0, 0.0, 1.0]), (len(uv), 1))
    h, w = tex.shape[:2]
    t = tex.astype(np.float64) / 255.0
    with np.errstate(all="ignore"):
        x, y = uv[:, 0].astype(np.float64) * w - 0.5, uv[:, 1].astype(np.float64) * h - 0.5
    x, y = np.clip(np.nan_to_num(x, nan=0.0, posinf=np.inf, neginf=-np.inf), -1, w), np.clip(np.nan_to_num(y, nan=0.0, posinf=np.inf, neginf=-np.inf), -1, h)
    x0, y0 = np.floor(x).astype(int), np.floor(y).astype(int)
    fx, fy = (x - x0)[:, None], (y - y0)[:, None]
    cx = lambda k: np.clip(k, 0, w - 1)
    cy = lambda k: np.clip(k, 0, h - 1)
    top = t[cy(y0), cx(x0)] * (1 - fx) + t[cy(y0), cx(x0 + 1)] * fx
    bottom = t[cy(y0 + 1), cx(x0)] * (1 - fx) + t[cy(y0 + 1), cx(x0 + 1)] * fx
    return top * (1 - fy) + bottom * fy


def run_texture_cases(bind_texture, set_int, render):
    """Every case of texture_cases() through one compiled texture_source kernel -> list of failure lines.  Bit for bit against
    oracle.glsl_values.texture, within TEXTURE_TOLERANCE of the binary64 bilinear filter."""
    lines = []
    for tex, uv in texture_cases():
        if tex is not None:
            bind_texture("tex", tex)
        bind_texture("in_tex", uv.reshape(-1).view(np.uint8).reshape(1, -1, 4))
        set_int("count_u", len(uv))
        set_int("unbound_u", 1 if tex is None else 0)
        got = render(len(uv), 1)[0]
        what = "unbound sampler" if tex is None else f"{tex.shape[1]}x{tex.shape[0]} texture"
        want = texture_oracle(tex, uv)
        bad = np.nonzero(~probe.same_bits(got, want).all(axis=1))[0]
        if len(bad):
            lines.append(f"{what}: {len(bad)} of {len(uv)} coordinates differ from the oracle, first uv = {uv[bad[0]]} bits {[hex(int(t)) for t in uv[bad[0]].view(U32)]}: "
                         f"{got[bad[0]]} vs {want[bad[0]]}")
        err = np.abs(got.astype(np.float64) - texture_binary64(tex, uv))
        if not (err <= TEXTURE_TOLERANCE).all():
            j = int(np.nanargmax(np.where(np.isnan(err), np.inf, err).max(axis=1)))
            lines.append(f"{what}: {float(err[j].max()):.3g} from the binary64 bilinear filter at uv = {uv[j]} (allowed {TEXTURE_TOLERANCE:.3g})")
    return lines
