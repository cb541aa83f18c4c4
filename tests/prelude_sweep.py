"""tests/prelude_sweep.py -- the prelude (portal_amd/csrc/device/ptl_library.h) function by function, beside tests/contract_sweep.py
(the builtins of ptl_glsl.h) whose conventions it follows.

A table of cases (function, GLSL parameter types, the C++ call, the output leaves in the order of tests.reftext.flatten) is turned
into a probe translation unit: ptl_glsl.h, a uniform block, ptl_library.h, a `shade_pixel` that reads one lane's flattened arguments
from a buffer bound as `in_tex` and returns four output leaves per pixel row group, ptl_entry.h.  The same unit is compiled by g++
(oracle/host_build) and by hiprtc (layer 1, `pa.Kernel`); every leaf is compared bit for bit (NaN == NaN the only equivalence, bools
and ints as numbers) with

  * tests/golden/reference_text/functions.npz -- the reference text's own values -- on the 1024 committed lanes,
  * the numpy restatement `oracle.portal_oracle.Natives` on those, on 16 384 lanes of the same generator and on DIRECTED lanes
    built from geometry to reach every branch and edge.  How many directed lanes go through each branch is counted with the
    restatement's arithmetic (never with the code under test) and asserted: MIN_BRANCH for a branch, MIN_EDGE for an equality / NaN edge.

The product-only forms (plane_intersect_derived / _o / _derived_o / ptl_plane_intersect_unit, ptl_normalize_normal_unit,
ptl_is_collinear_len / _len0, ptl_mul_m / ptl_transform_m for a list of masks, ptl_cannot_be_nearer / ptl_plane_cull) are evaluated
in the same kernel as their base form and compared with the restatement of the base form.
"""
import functools
import os

import numpy as np

from tests import reftext as T

F32, U32, I32 = np.float32, np.uint32, np.int32
ROOT = T.ROOT
LIBRARY_HEADER = os.path.join(ROOT, "portal_amd", "csrc", "device", "ptl_library.h")
N_COMMITTED, N_RANDOM, N_AFFINE = 1024, 16384, 4096
MIN_BRANCH, MIN_EDGE = 256, 64
SEED = 20261019
FRAME_W = 4096

# keys of functions.npz without a case: helpers inside the trace template that the product inlines or does not have as functions of their own
# (the depth-map pieces are covered through sample_depth_gradient, the float -> RGBA8 packing of the teleport query is replaced by a float read-back)
TEMPLATE_KEYS = {"normalize_depth_value(float)", "depth_gradient_inferno(float)", "shift_right(float,float)", "shift_left(float,float)", "mask_last(float,float)",
                 "extract_bits(float,float,float)", "encode_float(float)", "Pow2(float)"}

# ---- types: leaves in the order of tests.reftext.flatten ----------------------------------------------------------------------------
FIELDS = {
    "vec2": [("float", ".x"), ("float", ".y")],
    "vec3": [("float", ".x"), ("float", ".y"), ("float", ".z")],
    "vec4": [("float", ".x"), ("float", ".y"), ("float", ".z"), ("float", ".w")],
    "mat3": [("vec3", "[0]"), ("vec3", "[1]"), ("vec3", "[2]")],
    "mat4": [("vec4", "[0]"), ("vec4", "[1]"), ("vec4", "[2]"), ("vec4", "[3]")],
    "Ray": [("vec4", ".o"), ("vec4", ".d"), ("float", ".tmul"), ("bool", ".in_subspace")],
    "SurfaceIntersection": [("bool", ".hit"), ("float", ".t"), ("float", ".u"), ("float", ".v"), ("vec3", ".n")],
    "SceneIntersection": [("int", ".material"), ("SurfaceIntersection", ".hit"), ("bool", ".in_subspace")],
    "MaterialProcessing": [("bool", ".is_final"), ("vec3", ".mul_to_color"), ("Ray", ".new_ray")],
}


def leaf_kinds(ty):
    """'f' / 'b' / 'i' per leaf of a value of GLSL type `ty`."""
    if ty in ("float", "bool", "int"):
        return [ty[0]]
    return [k for t, _ in FIELDS[ty] for k in leaf_kinds(t)]


def leaf_exprs(ty, e):
    """C++ float expressions of the leaves of expression `e` of type `ty`."""
    if ty == "float":
        return [e]
    if ty == "bool":
        return [f"(({e}) ? 1.0f : 0.0f)"]
    if ty == "int":
        return [f"(float)({e})"]
    return [x for t, s in FIELDS[ty] for x in leaf_exprs(t, f"({e}){s}")]


def decode_expr(ty, at):
    """C++ expression that builds a value of type `ty` from the input words at[0] .. ; -> (expression, words used)."""
    if ty == "float":
        return f"F({at})", 1
    if ty == "int":
        return f"(int)in[{at}]", 1
    if ty == "bool":
        return f"(in[{at}] != 0u)", 1
    parts, used = [], 0
    for t, _ in FIELDS[ty]:
        e, k = decode_expr(t, at + used)
        parts.append(e)
        used += k
    ctor = f"{ty}(" + ", ".join(parts) + ")" if ty.startswith(("vec", "mat")) else f"{ty}{{" + ", ".join(parts) + "}"
    return ctor, used


# ---- the case table -----------------------------------------------------------------------------------------------------------------
class Case:
    def __init__(self, name, ptypes, body, outputs, want, group, base=None, builds=("shipped", "O1", "contract1", "affine")):
        self.name, self.ptypes, self.body, self.outputs, self.want, self.group = name, tuple(ptypes), body, outputs, want, group
        self.base = base or name          # the reference function whose input generator it uses
        self.builds = builds
        self.kinds = [k for t, _ in outputs for k in leaf_kinds(t)]
        self.labels = [f"{e}{p}" for t, e in outputs for p in _paths(t)]

    @property
    def key(self):
        return f"{self.name}({','.join(self.ptypes)})"


def _paths(ty):
    if ty in ("float", "bool", "int"):
        return [""]
    return [s + p for t, s in FIELDS[ty] for p in _paths(t)]


def _lib(name, ptypes, ret, group="library"):
    call = f"{name}(" + ", ".join(f"a{i}" for i in range(len(ptypes))) + ")"
    return Case(name, ptypes, f"const {ret} r = {call};", [(ret, "r")], lambda nat, a, _n=name: [getattr(nat, _n)(*a)], group)


SI, RAY, SCI, MP = "SurfaceIntersection", "Ray", "SceneIntersection", "MaterialProcessing"
LIBRARY = [
    ("between", ("float", "float", "float"), "bool"), ("sqr", ("float",), "float"), ("sqrvec", ("vec3",), "vec3"), ("offset_ray", (RAY, "float"), RAY),
    ("normalize_normal", ("vec3", "vec3"), "vec3"), ("is_collinear", ("vec3", "vec3"), "bool"), ("my_reflect", ("vec3", "vec3"), "vec3"),
    ("my_refract", ("vec3", "vec3", "float"), "vec3"), ("transform", ("mat4", RAY), RAY), ("get_normal", ("mat4",), "vec3"), ("normalize_ray", (RAY,), RAY),
    ("adjugate", ("mat4",), "mat3"), ("plane_intersect_normalized", (RAY,), SI), ("plane_intersect", (RAY, "mat4", "vec3"), SI),
    ("color", ("float", "float", "float"), "vec3"), ("color_normal", ("vec3", "vec4"), "float"), ("color_grid", ("vec3", "vec2"), "vec3"),
    ("circle_sdf", ("vec2",), "float"), ("color_grid2", ("vec3", "vec2"), "vec3"), ("color_grid3", ("vec3", "vec2"), "vec3"),
    ("color_add_weighted", ("vec3", "vec3", "float"), "vec3"), ("material_empty", (), MP), ("material_final", ("vec3",), MP), ("material_next", ("vec3", RAY), MP),
    ("material_simple2", (SI, RAY, "vec3", "float", "bool", "float", "float", "bool", "bool"), MP),
    ("material_simple", (SI, RAY, "vec3", "float", "bool", "float", "float"), MP), ("material_reflect", (SI, RAY, "vec3"), MP),
    ("material_refract", (SI, RAY, "vec3", "float"), MP), ("material_teleport_transformed", (RAY, "vec3"), MP), ("material_teleport", (SI, RAY, "mat4"), MP),
    ("material_change_subspace", (RAY,), MP), ("nearer", (SI, SI), "bool"), ("nearer", (SCI, SI), "bool"), ("nearer", (SCI, SCI), "bool"),
    ("cap_normal", ("vec3", "vec3", "vec3", "float"), "vec3"), ("cap", (RAY, "vec3", "vec3", "float"), SI), ("cylinder", (RAY, "vec3", "vec3", "float"), SI),
    ("triangle", (RAY, "vec3", "vec3", "vec3"), SI), ("debug_intersect", (RAY,), SCI), ("process_plane_intersection", (SCI, SI, "int"), SCI),
    ("process_portal_intersection", (SCI, SI, "int", "int"), SCI),
]

# the masks of ptl_mul_m / ptl_transform_m: (name, may-be-non-zero bits, +1 bits, -1 bits), bit 4 * column + row
_ROW3 = (1 << 3) | (1 << 7) | (1 << 11)
MASKS = [
    ("identity", 0x8421, 0x8421, 0),
    ("translation", 0x8421 | 0x7000, 0x8421, 0),
    ("quarter_turn", (1 << 1) | (1 << 4) | (1 << 10) | 0xF000, (1 << 1) | (1 << 10) | (1 << 15), 1 << 4),
    ("one_zero", 0xFFFF & ~(1 << 6), 0, 0),
    ("dense", 0xFFFF, 0, 0),
    ("bottom_row_0001", 0xFFFF & ~_ROW3, 1 << 15, 0),
]
W_MODES = [("PTL_W_ANY", None), ("PTL_W_ONE", 1.0), ("PTL_W_ZERO", 0.0)]


def mask_literal(bits, ones, negs):
    return f"((ptl_mask_t)0x{bits:x}ull | PTL_UNIT_BITS(0x{ones:x}ull, 0x{negs:x}ull))"


def _want_plane_forms(nat, a):
    from oracle import glsl_math as M
    from oracle import glsl_values as V

    base = nat.plane_intersect(*a)
    flipped = M.gt(V.dot(V.normalize(a[2]), V.Vec(a[0].f["d"].c[:3])), F32(0))
    return [base, base, flipped, base, base, base, flipped]


def _want_derived_m(nat, a):
    from oracle import glsl_math as M
    from oracle import glsl_values as V

    inv, r, n = a
    base = nat.plane_intersect(r, inv, n)
    flipped = M.gt(V.dot(V.normalize(n), V.Vec(r.f["d"].c[:3])), F32(0))
    return [base, flipped, base, flipped, V.mat_vec(inv, r.f["o"]).c[2], V.mat_vec(inv, r.f["d"]).c[2]]


def _want_cull(nat, a):
    from oracle import glsl_values as V

    r, inv, n, best = a
    o, d = V.mat_vec(inv, r.f["o"]), V.mat_vec(inv, r.f["d"])
    hit = nat.plane_intersect(r, inv, n)
    return [o.c[2], d.c[2], hit]


def _want_mul_m(w, nat, a):
    """masked: the full chain with v.w taken for what W says (half of the lanes carry that very w: there it is the full chain m * v; the others
    pin that PTL_W_ONE / PTL_W_ZERO do not read v.w); full: m * v."""
    from oracle import glsl_values as V

    m, v = a
    forced = v if w is None else V.Vec(list(v.c[:3]) + [np.full(np.shape(v.c[3]), w, F32)])
    return [V.mat_vec(m, forced), V.mat_vec(m, v)]


@functools.lru_cache(maxsize=None)
def cases():
    from oracle import glsl_values as V

    out = [_lib(*row) for row in LIBRARY] + [_tpl(*row) for row in TEMPLATE]
    out.append(Case("plane_forms", (RAY, "mat4", "vec3"),
                    "const SurfaceIntersection base = plane_intersect(a0, a1, a2); const vec3 un = normalize(a2); bool f1 = false, f2 = false;\n"
                    "            const SurfaceIntersection der = plane_intersect_derived<0xffffu>(a0, a1, un, f1);\n"
                    "            const SurfaceIntersection unit = ptl_plane_intersect_unit(a0, a1, un);\n"
                    "            const vec4 oin = a1 * a0.o;\n"
                    "            const SurfaceIntersection with_o = plane_intersect_o(a0, a1, a2, oin);\n"
                    "            const SurfaceIntersection der_o = plane_intersect_derived_o<0xffffu>(a0, a1, un, f2, oin);",
                    [(SI, "base"), (SI, "der"), ("bool", "f1"), (SI, "unit"), (SI, "with_o"), (SI, "der_o"), ("bool", "f2")],
                    _want_plane_forms, "forms", base="plane_intersect"))
    out.append(Case("normal_forms", ("vec3", "vec3"), "const vec3 base = normalize_normal(a0, a1); const vec3 unit = ptl_normalize_normal_unit(normalize(a0), a1);",
                    [("vec3", "base"), ("vec3", "unit")], lambda nat, a: [nat.normalize_normal(*a)] * 2, "forms", base="normalize_normal"))
    out.append(Case("collinear_forms", ("vec3", "vec3"),
                    "const bool base = is_collinear(a0, a1); const bool len = ptl_is_collinear_len(a0, a1, length(a1)); const bool len0 = ptl_is_collinear_len0(a0, a1, length(a0));",
                    [("bool", "base"), ("bool", "len"), ("bool", "len0")], lambda nat, a: [nat.is_collinear(*a)] * 3, "forms", base="is_collinear"))
    out.append(Case("cull", (RAY, "mat4", "vec3", "float"),
                    "const float oz = ptl_row_m<0xffffu, 2, PTL_W_OF_ORIGIN>(a1, a0.o), dz = ptl_row_m<0xffffu, 2, PTL_W_OF_DIRECTION>(a1, a0.d);\n"
                    "            const SurfaceIntersection hit = plane_intersect(a0, a1, a2);\n"
                    "            const bool cannot = ptl_cannot_be_nearer(oz, dz, a3);\n"
                    "            const bool near = nearer(SurfaceIntersection{true, a3, 0.0f, 0.0f, vec3(0.0f)}, hit);\n"
                    "            const bool ballot = ptl_plane_cull<0xffffu>(a0, a1, a3);",
                    [("float", "oz"), ("float", "dz"), (SI, "hit"), ("bool", "cannot"), ("bool", "near"), ("bool", "ballot")], _want_cull, "forms", base="cull"))
    for mname, bits, ones, negs in MASKS:
        lit = mask_literal(bits, ones, negs)
        for wname, _w in W_MODES:
            out.append(Case(f"mul_m_{mname}_{wname[6:]}", ("mat4", "vec4"), f"const vec4 masked = ptl_mul_m<{lit}, {wname}>(a0, a1); const vec4 full = a0 * a1;",
                            [("vec4", "masked"), ("vec4", "full")], functools.partial(_want_mul_m, _w), "masks", base="mask", builds=("shipped", "O1", "affine")))
        if mname in ("translation", "quarter_turn", "bottom_row_0001"):
            out.append(Case(f"derived_m_{mname}", ("mat4", RAY, "vec3"),
                            f"bool f1 = false, f2 = false; const vec3 un = normalize(a2); const SurfaceIntersection der = plane_intersect_derived<{lit}>(a1, a0, un, f1);\n"
                            f"            const SurfaceIntersection der_o = plane_intersect_derived_o<{lit}>(a1, a0, un, f2, ptl_mul_origin<{lit}>(a0, a1.o));\n"
                            f"            const float oz = ptl_row_m<{lit}, 2, PTL_W_OF_ORIGIN>(a0, a1.o), dz = ptl_row_m<{lit}, 2, PTL_W_OF_DIRECTION>(a0, a1.d);",
                            [(SI, "der"), ("bool", "f1"), (SI, "der_o"), ("bool", "f2"), ("float", "oz"), ("float", "dz")], _want_derived_m, "masks", base="mask",
                            builds=("shipped", "O1", "affine")))
        out.append(Case(f"transform_m_{mname}", ("mat4", RAY), f"const Ray masked = ptl_transform_m<{lit}>(a0, a1); const Ray full = transform(a0, a1);",
                        [(RAY, "masked"), (RAY, "full")], lambda nat, a: [nat.transform(a[0], a[1])] * 2, "masks", base="mask", builds=("shipped", "O1", "affine")))
    return out


def case(name, ptypes=None):
    for c in cases():
        if c.name == name and (ptypes is None or c.ptypes == tuple(ptypes)):
            return c
    raise KeyError(name)


def groups_of_cases():
    return sorted({c.group for c in cases()})


def prelude_reference_functions():
    """Names that ptl_library.h defines with PTL_FN (for the test that the table covers the prelude's share of functions.npz)."""
    import re

    return set(re.findall(r"PTL_FN\s+[A-Za-z_0-9]+\s+([A-Za-z_0-9]+)\s*\(", open(LIBRARY_HEADER).read()))


# ---- the probe unit -----------------------------------------------------------------------------------------------------------------
LAYOUT = [("in_tex", 5, 0), ("fn_u", 2, 16), ("count_u", 2, 20), ("words_u", 2, 24), ("groups_u", 2, 28), ("tiled_u", 2, 32), ("group_u", 2, 36),
          ("grid_disable_u", 2, 40), ("angle_color_disable_u", 2, 44), ("offset_u", 1, 48)]
BLOCK_SIZE = 56


def case_blocks(group):
    """The `case K: { ... }` bodies of one group: decode the arguments, evaluate once, return the four leaves of row group g from registers."""
    blocks = []
    for c in [c for c in cases() if c.group == group]:
        k = cases().index(c)
        decl, at = [], 0
        for j, t in enumerate(c.ptypes):
            e, used = decode_expr(t, at)
            decl.append(f"const {t} a{j} = {e};")
            at += used
        leaves = [x for t, e in c.outputs for x in leaf_exprs(t, e)] + ["echo"]
        leaves += ["0.0f"] * (-len(leaves) % 4)
        rows = "\n".join(f"                case {g}: return vec4({', '.join(leaves[4 * g:4 * g + 4])});" for g in range(len(leaves) // 4))
        blocks.append(f"        case {k}: {{  // {c.key}\n            {' '.join(decl)}\n            {c.body}\n            switch (g) {{\n{rows}\n"
                      f"                default: return vec4(0.0f);\n            }}\n        }}")
    return "\n".join(blocks)


def source(pa, group):
    """The probe unit of one group of cases.  Pixel (x, y): lane i = x + FRAME_W * (y / groups_u), leaves 4 * (y % groups_u) .. + 3; with
    tiled_u the lanes are laid out 64 to an 8x8 tile (one wavefront) and the frame holds row group `group_u` only.  A lane outside
    [0, count_u) returns zeros before it reads anything.  Leaves are returned from registers: the unit uses no private arrays."""
    if group == "template":
        return template_unit(pa)[0]
    blocks = [case_blocks(group)]
    return (
        pa.device_source("glsl")
        + """
#define PTL_COUNT_SEGMENT() ((void)0)
#define PTL_NO_TELEPORT_ENTRY 1
namespace glsl {
struct ptl_uniform_block { sampler2D in_tex; int fn_u; int count_u; int words_u; int groups_u; int tiled_u; int group_u; int grid_disable_u; int angle_color_disable_u; float offset_u; };
#if PTL_DEVICE_BUILD
__constant__ ptl_uniform_block ptl_u;
#else
ptl_uniform_block ptl_u;
#endif
}  // namespace glsl
#define _grid_disable (ptl_u.grid_disable_u)
#define _angle_color_disable (ptl_u.angle_color_disable_u)
#define _black_border_disable 0
#define _offset_after_material (ptl_u.offset_u)
"""
        + pa.device_source("library")
        + """
namespace glsl {
#define F(k) __builtin_bit_cast(float, in[k])
PTL_FN vec4 evaluate(int fn, int g, const unsigned int* in, float echo) {
    switch (fn) {
"""
        + "\n".join(blocks)
        + f"""
        default: return vec4(0.0f);
    }}
}}
#undef F
PTL_FN vec4 shade_pixel(vec2 position) {{
    const int x = (int)position.x, y = (int)position.y;
    int i, g;
    if (ptl_u.tiled_u != 0) {{
        i = ((y >> 3) * ({FRAME_W} >> 3) + (x >> 3)) * 64 + (y & 7) * 8 + (x & 7);
        g = ptl_u.group_u;
    }} else {{
        i = x + {FRAME_W} * (y / ptl_u.groups_u);
        g = y % ptl_u.groups_u;
    }}
    if (x >= {FRAME_W} || i < 0 || i >= ptl_u.count_u) return vec4(0.0f);
    const unsigned int* in = reinterpret_cast<const unsigned int*>(ptl_u.in_tex.texels) + (long)i * ptl_u.words_u;
    unsigned int h = 0u;   // the echo leaf: a 24-bit digest of the lane's input words, exact in a float
    for (int k = 0; k < ptl_u.words_u; k++) h = h * 31u + in[k];
    return evaluate(ptl_u.fn_u, g, in, (float)((h ^ (h >> 24)) & 0xffffffu));
}}
PTL_FN unsigned int pack_rgba8(vec4 c) {{ return 0u; }}
}}  // namespace glsl
"""
        + pa.device_source("entry")
    )


TEMPLATE_HEADER_WORDS = 8
TEMPLATE_SCENE = "basics"
TEMPLATE_SAMPLER = "texture_tex"       # the scene's own sampler slot carries the input words
PACK_FN = -1                           # fn < 0: the lane's four floats go out as they came (for pack_rgba8)


def template_unit(pa):
    """The scene-independent members of the trace template (PaniniProjection, sample_depth_gradient, quasi_random, anaglyphCombineLinear) and
    pack_rgba8, which sit in or behind `ptl_tracer`: the generated source of scenes/basics.ron with the anaglyph mode compiled in, cut where the
    entry text begins, its `shade_pixel` wrapper renamed, a probe `shade_pixel` that builds `ptl_tracer t{&ptl_u}` as the wrapper does, the
    entry again.  The input words ride in the scene's sampler slot behind a header (fn, count, words per lane, row groups).
    -> (source, layout, block size, defines)"""
    scene = pa.Scene.from_file(pa.scene_path(TEMPLATE_SCENE))
    src = scene.generate_source(pa.FLAG_ANAGLYPH)
    layout, size = scene.uniform_layout()
    cut = src.index("// ptl_entry.h --")
    close = src.rindex("}  // namespace glsl", 0, cut)
    head, entry = src[:close], src[cut:]
    wrapper = "PTL_FN vec4 shade_pixel(vec2 position) {\n    ptl_tracer t{&ptl_u};"
    assert head.count(wrapper) == 1
    head = head.replace(wrapper, "PTL_FN vec4 ptl_scene_shade_pixel(vec2 position) {\n    ptl_tracer t{&ptl_u};")
    probe = (
        """
#define F(k) __builtin_bit_cast(float, in[k])
PTL_FN vec4 evaluate(ptl_tracer& t, int fn, int g, const unsigned int* in, float echo) {
    switch (fn) {
"""
        + case_blocks("template")
        + f"""
        default: return vec4(0.0f);
    }}
}}
PTL_FN vec4 shade_pixel(vec2 position) {{
    ptl_tracer t{{&ptl_u}};
    const unsigned int* hdr = reinterpret_cast<const unsigned int*>({TEMPLATE_SAMPLER}.texels);
    if (hdr == nullptr || {TEMPLATE_SAMPLER}.width < {TEMPLATE_HEADER_WORDS}) return vec4(0.0f);
    const int fn = (int)hdr[0], count = (int)hdr[1], words = (int)hdr[2], groups = (int)hdr[3];
    if (count < 0 || words < 1 || groups < 1 || (long){TEMPLATE_HEADER_WORDS} + (long)count * words > (long){TEMPLATE_SAMPLER}.width) return vec4(0.0f);
    const int x = (int)position.x, y = (int)position.y;
    const int i = x + {FRAME_W} * (y / groups), g = y % groups;
    if (x >= {FRAME_W} || i < 0 || i >= count) return vec4(0.0f);
    const unsigned int* in = hdr + {TEMPLATE_HEADER_WORDS} + (long)i * words;
    if (fn < 0) return words >= 4 ? vec4(F(0), F(1), F(2), F(3)) : vec4(0.0f);
    unsigned int h = 0u;
    for (int k = 0; k < words; k++) h = h * 31u + in[k];
    return evaluate(t, fn, g, in, (float)((h ^ (h >> 24)) & 0xffffffu));
}}
#undef F
}}  // namespace glsl

"""
    )
    return head + probe + entry, layout, size, tuple(scene.generated_defines())


@functools.lru_cache(maxsize=None)
def template_oracle():
    from oracle.portal_oracle import Oracle

    o = Oracle(os.path.join(ROOT, "scenes", TEMPLATE_SCENE + ".ron"))
    o.anaglyph_compiled_in = True
    o.build(64, 64)
    return o


TEMPLATE_UNIFORMS = ("_anaglyph_p", "_anaglyph_q", "_depth_map_min", "_depth_map_max")    # what the four members read


def _tpl(name, ptypes, ret):
    call = f"t.{name}(" + ", ".join(f"a{i}" for i in range(len(ptypes))) + ")"

    def want(nat, a, _n=name, _p=tuple(ptypes)):
        n = max([len(np.atleast_1d(leaf)) for x in a for _, leaf in T.flatten(x)])
        return [T.restated(template_oracle(), _n, _p, a, n)]

    return Case(name, ptypes, f"const {ret} r = {call};", [(ret, "r")], want, "template", builds=("shipped", "O1"))


TEMPLATE = [("PaniniProjection", ("vec2", "float", "float"), "vec3"), ("sample_depth_gradient", ("float",), "vec3"), ("quasi_random", ("int",), "vec2"),
            ("anaglyphCombineLinear", ("vec3", "vec3", "int"), "vec3")]


def words_of(args, n):
    """The flattened arguments as (n, words) uint32: floats by bit pattern, ints as int32, bools as 0 / 1."""
    from oracle import glsl_values as V

    cols = []
    for a in args:
        for _, leaf in T.flatten(V.expand(a, n)):
            leaf = np.broadcast_to(leaf, (n,))
            if leaf.dtype == F32:
                cols.append(leaf.view(U32))
            elif leaf.dtype == np.bool_:
                cols.append(leaf.astype(U32))
            else:
                cols.append(leaf.astype(I32).view(U32))
    if not cols:
        cols = [np.zeros(n, U32)]
    return np.ascontiguousarray(np.stack(cols, axis=1))


def echo_of(words):
    h = np.zeros(len(words), np.uint64)
    for k in range(words.shape[1]):
        h = (h * np.uint64(31) + words[:, k].astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return ((h ^ (h >> np.uint64(24))) & np.uint64(0xFFFFFF)).astype(F32)


def leaves_to_bits(c, leaves):
    """(n, k) float32 probe output -> the uint32 matrix of tests.reftext.leaves_array (one NaN; bools and ints widened)."""
    out = np.empty(leaves.shape, U32)
    for j, kind in enumerate(c.kinds):
        col = np.ascontiguousarray(leaves[:, j])
        if kind == "f":
            bits = col.view(U32).copy()
            bits[np.isnan(col)] = 0x7FC00000
            out[:, j] = bits
        else:
            out[:, j] = col.astype(np.int64).astype(U32)
    return out


class Runner:
    """One compiled probe kernel (host build or layer 1 on the GPU) of one group of cases.  Every set_texture / set_uniform must succeed."""

    def __init__(self, pa, group, where, defines=()):
        self.group, self.where, self.header = group, where, group == "template"
        if self.header:
            src, layout, size, own = template_unit(pa)
            defines = tuple(own) + tuple(defines)
            self.sampler = TEMPLATE_SAMPLER
        else:
            src, layout, size, self.sampler = source(pa, group), LAYOUT, BLOCK_SIZE, "in_tex"
        types = {name: typ for name, typ, _ in layout}
        if where == "host":
            from oracle import host_build as hb

            k = hb.HostKernel(src, layout, size, defines=tuple(defines))
            self._tex = lambda t: _ok(k.set_texture(self.sampler, t) is True, "set_texture")
            self._set = lambda name, v: _ok(k.set_uniform(name, v) is True, f"set_uniform {name}")
            self._render = lambda w, h, rgba8=False: k.render(w, h, rgba8=rgba8)
        else:
            k = pa.Kernel(src, layout, size, device=0, defines=tuple(defines))
            self._tex = lambda t: _ok(k.set_texture(self.sampler, t) == 0, "set_texture")
            self._set = lambda name, v: _ok(k.set_uniform(name, types[name], v) == 0, f"set_uniform {name}")
            self._render = lambda w, h, rgba8=False: k.render(w, h, rgba8=rgba8, rgba32f=True)
        self._k = k
        if self.header:
            u = template_oracle().uniforms
            for name in TEMPLATE_UNIFORMS:
                self._set(name, F32(u[name]))

    def _bind(self, fn, words, n, g):
        if self.header:
            hdr = np.zeros(TEMPLATE_HEADER_WORDS, U32)
            hdr[:4] = np.array([fn, n, words.shape[1], g], I32).view(U32)
            buf = np.concatenate([hdr, words.reshape(-1)])
        else:
            buf = words.reshape(-1)
        self._tex(np.ascontiguousarray(buf).view(np.uint8).reshape(1, -1, 4))

    def run(self, c, args, n, uniforms, tiled=False):
        """-> (n, leaves) float32.  The echo leaf proves that the lane's inputs arrived."""
        assert c.group == self.group and not (tiled and self.header)
        words = words_of(args, n)
        nl = len(c.kinds) + 1
        g = -(-nl // 4)
        self._bind(cases().index(c), words, n, g)
        if not self.header:
            for name, v in (("fn_u", cases().index(c)), ("count_u", n), ("words_u", words.shape[1]), ("groups_u", g), ("tiled_u", int(tiled)), ("group_u", 0),
                            ("grid_disable_u", int(uniforms["_grid_disable"])), ("angle_color_disable_u", int(uniforms["_angle_color_disable"])),
                            ("offset_u", F32(uniforms["_offset_after_material"]))):
                self._set(name, v)
        if tiled:
            tiles = -(-n // 64)
            rows = -(-tiles // (FRAME_W // 8)) * 8
            out = np.empty((tiles * 64, 4 * g), F32)
            for gi in range(g):
                self._set("group_u", gi)
                f = self._render(FRAME_W, rows)["rgba32f"].reshape(rows // 8, 8, FRAME_W // 8, 8, 4)
                out[:, 4 * gi:4 * gi + 4] = f.transpose(0, 2, 1, 3, 4).reshape(-1, 4)[:tiles * 64]
            out = out[:n]
        else:
            rows = -(-n // FRAME_W)
            f = self._render(FRAME_W, rows * g)["rgba32f"].reshape(rows, g, FRAME_W, 4)
            out = f.transpose(0, 2, 1, 3).reshape(rows * FRAME_W, 4 * g)[:n]
        assert np.array_equal(out[:, nl - 1].view(U32), echo_of(words).view(U32)), f"{c.key}: the inputs did not arrive intact"
        return np.ascontiguousarray(out[:, :nl - 1])

    def run_pack(self, rgba):
        """(n, 4) float32 colours through the template unit's entry -> (RGBA32F (n, 4), RGBA8 (n, 4)) of ONE launch."""
        assert self.header
        n = len(rgba)
        self._bind(PACK_FN, np.ascontiguousarray(rgba, F32).view(U32), n, 1)
        rows = -(-n // FRAME_W)
        out = self._render(FRAME_W, rows, rgba8=True)
        return out["rgba32f"].reshape(-1, 4)[:n], out["rgba8"].reshape(-1, 4)[:n]


def _ok(cond, what):
    assert cond, f"{what} failed"


def pack_inputs():
    """Channel values for pack_rgba8: every rounding boundary (k + 0.5) / 255 and one step either side, 0, -0, 1 and its neighbours, negatives, values
    above 1, inf, NaN, subnormals; four to a pixel, shifted so that every channel meets every value."""
    k = ((np.arange(255) + 0.5) / 255.0).astype(F32)
    one = F32(1.0)
    v = np.concatenate([k, np.nextafter(k, F32(2)), np.nextafter(k, F32(-1)), (np.arange(256) / 255.0).astype(F32),
                        np.array([0.0, -0.0, 1.0, np.nextafter(one, F32(2)), np.nextafter(one, F32(0)), -1.0, -1e-45, 1e-45, 1e-38, 2.0, 255.0, 1e30, -1e30,
                                  np.inf, -np.inf, np.nan, 0.5, 0.25], F32)])
    return np.ascontiguousarray(np.stack([v, np.roll(v, 1), np.roll(v, 2), np.roll(v, 3)], axis=1))


def check_pack(runner):
    """RGBA8 == oracle.portal_oracle.to_rgba8(RGBA32F) of the same launch, and RGBA32F carries the inputs unchanged.  -> failure lines"""
    from oracle.portal_oracle import to_rgba8

    rgba = pack_inputs()
    f32, u8 = runner.run_pack(rgba)
    lines = []
    same = (f32.view(U32) == rgba.view(U32)) | (np.isnan(f32) & np.isnan(rgba))
    if not same.all():
        lines.append(f"pack_rgba8: {int((~same).sum())} float channels did not come back as they went in")
    want = to_rgba8(f32)
    bad = np.flatnonzero((u8 != want).any(axis=1))
    if len(bad):
        i = int(bad[0])
        lines.append(f"pack_rgba8: {len(bad)} of {len(rgba)} pixels differ from to_rgba8, first {[hex(int(w)) for w in rgba[i].view(U32)]} -> {u8[i]} want {want[i]}")
    return lines


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def basics_uniforms():
    """What `Oracle("scenes/basics.ron").build(64, 64)` uploads: the values the committed vectors were made with."""
    from oracle.portal_oracle import Oracle

    o = Oracle(os.path.join(ROOT, "scenes", "basics.ron"))
    o.build(64, 64)
    return {k: o.uniforms[k] for k in ("_grid_disable", "_angle_color_disable", "_offset_after_material")}


def natives(uniforms=None):
    from oracle.portal_oracle import Natives

    return Natives(dict(uniforms or basics_uniforms()))


def vcat(values):
    from oracle.glsl_values import Mat, Struct, Vec

    a = values[0]
    if isinstance(a, Vec):
        return Vec([np.concatenate([np.asarray(v.c[i], F32) for v in values]) for i in range(a.n)])
    if isinstance(a, Mat):
        return Mat([vcat([v.cols[i] for v in values]) for i in range(a.n)])
    if isinstance(a, Struct):
        return Struct(a.tname, {k: vcat([v.f[k] for v in values]) for k in a.f})
    return np.concatenate([np.asarray(v) for v in values])


def cat_args(sets):
    """[(args, n)] -> (args, n) with the lanes one after the other."""
    from oracle import glsl_values as V

    sets = [s for s in sets if s[1] > 0]
    n = sum(m for _, m in sets)
    if not sets[0][0]:
        return [], n
    return [vcat([V.expand(a[j], m) for a, m in sets]) for j in range(len(sets[0][0]))], n


def v3(x, y, z):
    from oracle.glsl_values import Vec

    return Vec([np.asarray(x, F32), np.asarray(y, F32), np.asarray(z, F32)])


def v4(x, y, z, w):
    from oracle.glsl_values import Vec

    return Vec([np.asarray(x, F32), np.asarray(y, F32), np.asarray(z, F32), np.asarray(w, F32)])


def mk_ray(o, d, n, tmul=1.0, sub=False):
    from oracle.portal_oracle import Ray

    o4 = v4(o[0], o[1], o[2], np.ones(n)) if len(o) == 3 else v4(*o)
    d4 = v4(d[0], d[1], d[2], np.zeros(n)) if len(d) == 3 else v4(*d)
    return Ray(o4, d4, np.broadcast_to(F32(tmul), (n,)).copy(), np.broadcast_to(np.bool_(sub), (n,)).copy())


def mat_from(m):
    """(n, 4, 4) array m[lane, row, col] -> Mat"""
    from oracle.glsl_values import Mat

    m = np.asarray(m, F32)
    return Mat([v4(*(m[:, r, c] for r in range(4))) for c in range(4)])


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, a):
    """unit vectors perpendicular to the rows of a (float64)"""
    p = np.cross(a, rng.standard_normal(a.shape))
    return _unit(p)


def _cols(a):
    return a[:, 0], a[:, 1], a[:, 2]


def rigid(rng, n, scale=False):
    """(n, 4, 4) float64 affine matrices: a rotation, a translation of O(1), optionally a scale in [0.5, 2]."""
    q = _unit(rng.standard_normal((n, 4)))
    w, x, y, z = q.T
    r = np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], 1),
                  np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], 1),
                  np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1)], 1)
    if scale:
        r = r * rng.uniform(0.5, 2.0, (n, 1, 1))
    m = np.zeros((n, 4, 4))
    m[:, :3, :3] = r
    m[:, :3, 3] = rng.uniform(-2, 2, (n, 3))
    m[:, 3, 3] = 1.0
    return m


# -- directed families: each returns (args, n, {branch: (boolean lanes by the restatement's arithmetic, minimum)}) -----------------------
def _segment_geometry(rng, n):
    pa_ = rng.uniform(-1, 1, (n, 3))
    axis = _unit(rng.standard_normal((n, 3)))
    length = rng.uniform(0.5, 2.0, (n, 1))
    ra = rng.uniform(0.1, 0.5, (n, 1))
    return pa_, axis, length, ra


def _cyl_like_lanes(rng, per):
    """Rays against segments pa -> pb of radius ra, by geometry: side hits from outside, origins inside, rays entering through an end (the near
    root lies beyond the end), rays along the axis into each end, misses beside the body, misses of the infinite cylinder."""
    o, d, A, B, R = [], [], [], [], []

    def emit(pa_, pb, ra, ro, rd):
        o.append(ro), d.append(rd), A.append(pa_), B.append(pb), R.append(ra[:, 0])

    # side hits from outside
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    s = rng.uniform(0.1, 0.9, (per, 1))
    rad = _perp(rng, ax)
    target = pa_ + ax * ln * s
    ro = target + rad * ra * rng.uniform(2, 6, (per, 1)) + ax * rng.uniform(-0.3, 0.3, (per, 1))
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(target + _perp(rng, ax) * ra * rng.uniform(0, 0.7, (per, 1)) - ro))
    # origin inside the body
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    ro = pa_ + ax * ln * rng.uniform(0.2, 0.8, (per, 1)) + _perp(rng, ax) * ra * rng.uniform(0, 0.9, (per, 1))
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(rng.standard_normal((per, 3))))
    # entering through an end: origin beyond pa (or pb) within the radius, heading inwards and outwards enough to reach the wall inside
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    end_b = rng.random((per, 1)) < 0.5
    rad = _perp(rng, ax)
    ro = np.where(end_b, pa_ + ax * ln * 1.3, pa_ - ax * ln * 0.3) + rad * ra * rng.uniform(0, 0.5, (per, 1))
    wall = pa_ + ax * ln * rng.uniform(0.2, 0.8, (per, 1)) + _perp(rng, ax) * ra
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(wall - ro))
    # along the axis into each end (a little tilted)
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    end_b = rng.random((per, 1)) < 0.5
    ro = np.where(end_b, pa_ + ax * (ln + 2.0), pa_ - ax * 2.0) + _perp(rng, ax) * ra * rng.uniform(0, 0.8, (per, 1))
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(np.where(end_b, -ax, ax) + rng.standard_normal((per, 3)) * 0.02))
    # beside the body: hits the infinite cylinder beyond an end, far from the end sphere
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    rad = _perp(rng, ax)
    target = pa_ + ax * ln * rng.choice([-1.0, 2.0], (per, 1)) * rng.uniform(1.5, 3, (per, 1))
    ro = target + rad * ra * 5
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(target - ro))
    # misses of the infinite cylinder
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    rad = _perp(rng, ax)
    ro = pa_ + ax * ln * 0.5 + rad * ra * 4
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(np.cross(ax, rad) + ax * rng.uniform(-1, 1, (per, 1))))
    # leaving: the body lies behind the ray (negative roots)
    pa_, ax, ln, ra = _segment_geometry(rng, per)
    rad = _perp(rng, ax)
    ro = pa_ + ax * ln * 0.5 + rad * ra * 3
    emit(pa_, pa_ + ax * ln, ra, ro, _unit(rad + rng.standard_normal((per, 3)) * 0.1))
    cat = lambda parts: np.concatenate(parts).astype(F32)
    return cat(o), cat(d), cat(A), cat(B), cat(R)


def _exact_axis_lanes():
    """Exactly representable set-ups on the z axis (pa = 0, pb = (0, 0, L), radius 1): rays perpendicular to the axis at heights 0 and L
    (y == 0, y == baba), tangent rays (h == 0), rays parallel to the axis (k2 == 0), radius 0."""
    L = np.array([1.0, 2.0, 4.0, 0.5])
    x0 = np.array([2.0, 3.0, 4.0, 8.0, -2.0, -3.0, -4.0, -8.0])
    sy = np.array([0.0, 0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 0.125])
    Lg, xg, yg = (g.reshape(-1) for g in np.meshgrid(L, x0, sy, indexing="ij"))
    n = len(Lg)
    zero, one = np.zeros(n), np.ones(n)
    sets = []
    for z in (zero, Lg, Lg * 0.5):                       # y == 0, y == baba, a plain body hit
        sets.append((np.stack([xg, yg, z], 1), np.stack([-np.sign(xg), zero, zero], 1), Lg, one))
    tz = np.tile(np.array([0.25, 0.5, 0.75, 0.125]), n // 4) * Lg
    sets.append((np.stack([np.sign(xg), -np.abs(xg), tz], 1), np.stack([zero, one, zero], 1), Lg, one))      # tangent at x = +-1: h == 0
    sets.append((np.stack([yg, yg * 0.5, -xg], 1), np.stack([zero, zero, np.sign(xg)], 1), one, one))      # parallel to a unit axis: k2 == 0
    sets.append((np.stack([xg, yg, Lg * 0.5], 1), np.stack([-np.sign(xg), zero, zero], 1), Lg, zero))        # radius 0
    o = np.concatenate([s[0] for s in sets]).astype(F32)
    d = np.concatenate([s[1] for s in sets]).astype(F32)
    Lc = np.concatenate([s[2] for s in sets]).astype(F32)
    R = np.concatenate([s[3] for s in sets]).astype(F32)
    z = np.zeros(len(o), F32)
    return o, d, np.stack([z, z, z], 1), np.stack([z, z, Lc], 1), R


def _segment_args(rng, per):
    parts = [_cyl_like_lanes(rng, per), _exact_axis_lanes()]
    o, d, A, B, R = (np.concatenate([p[k] for p in parts]) for k in range(5))
    n = len(o)
    return [mk_ray(_cols(o), _cols(d), n), v3(*_cols(A)), v3(*_cols(B)), R.astype(F32)], n


def directed_cylinder(rng):
    from oracle import glsl_math as M
    from oracle import glsl_values as V
    from oracle.portal_oracle import sub, xyz

    args, n = _segment_args(rng, 1024)
    r, pa_, pb, ra = args
    ro, rd = xyz(r.f["o"]), xyz(r.f["d"])
    ba, oc = sub(pb, pa_), sub(ro, pa_)
    baba, bard, baoc = V.dot(ba, ba), V.dot(ba, rd), V.dot(ba, oc)
    k2 = M.sub(baba, M.mul(bard, bard))
    k1 = M.sub(M.mul(baba, V.dot(oc, rd)), M.mul(baoc, bard))
    k0 = M.sub(M.sub(M.mul(baba, V.dot(oc, oc)), M.mul(baoc, baoc)), M.mul(M.mul(ra, ra), baba))
    h = M.sub(M.mul(k1, k1), M.mul(k2, k0))
    hs = M.sqrt(h)
    yn = M.add(baoc, M.mul(M.div(M.sub(M.neg(k1), hs), k2), bard))
    yf = M.add(baoc, M.mul(M.div(M.add(M.neg(k1), hs), k2), bard))
    ok = ~M.lt(h, F32(0))
    near = ok & M.gt(yn, F32(0)) & M.lt(yn, baba)
    far = ok & ~near & M.gt(yf, F32(0)) & M.lt(yf, baba)
    cover = {"near side": (near, MIN_BRANCH), "far side only": (far, MIN_BRANCH), "h < 0": (~ok, MIN_BRANCH), "neither side": (ok & ~near & ~far, MIN_BRANCH),
             "y == 0": (ok & (yn == 0), MIN_EDGE), "y == baba": (ok & (yn == baba), MIN_EDGE), "k2 == 0": (k2 == 0, MIN_EDGE), "ra == 0": (ra == 0, MIN_EDGE)}
    return args, n, cover


def directed_cap(rng):
    from oracle import glsl_math as M
    from oracle import glsl_values as V
    from oracle.portal_oracle import sub, xyz

    args, n = _segment_args(rng, 1024)
    r, pa_, pb, radius = args
    ro, rd = xyz(r.f["o"]), xyz(r.f["d"])
    ba, oa = sub(pb, pa_), sub(ro, pa_)
    baba, bard, baoa, rdoa, oaoa = V.dot(ba, ba), V.dot(ba, rd), V.dot(ba, oa), V.dot(rd, oa), V.dot(oa, oa)
    a = M.sub(baba, M.mul(bard, bard))
    b = M.sub(M.mul(baba, rdoa), M.mul(baoa, bard))
    c = M.sub(M.sub(M.mul(baba, oaoa), M.mul(baoa, baoa)), M.mul(M.mul(radius, radius), baba))
    h = M.sub(M.mul(b, b), M.mul(a, c))
    y = M.add(baoa, M.mul(M.div(M.sub(M.neg(b), M.sqrt(h)), a), bard))
    ok = M.ge(h, F32(0))
    body = ok & M.gt(y, F32(0)) & M.lt(y, baba)
    end_a = M.le(y, F32(0))
    oc = V.select(end_a, oa, sub(ro, pb))
    b2 = V.dot(rd, oc)
    h2 = M.sub(M.mul(b2, b2), M.sub(V.dot(oc, oc), M.mul(radius, radius)))
    caps = ok & ~body & M.gt(h2, F32(0))
    inside = M.lt(c, F32(0)) & M.gt(baoa, F32(0)) & M.lt(baoa, baba)
    cover = {"body": (body, MIN_BRANCH), "cap at pa": (caps & end_a, MIN_BRANCH), "cap at pb": (caps & ~end_a, MIN_BRANCH), "h < 0": (~ok, MIN_BRANCH),
             "miss after the body test": (ok & ~body & ~caps, MIN_BRANCH), "origin inside": (inside, MIN_BRANCH), "h == 0": (h == 0, MIN_EDGE)}
    return args, n, cover


def directed_debug_intersect(rng):
    """Rays aimed at points of each of the three axis capsules (0 -> e_k, radius 0.03), and some that miss them all."""
    per = 512
    o, d = [], []
    for k in range(3):
        p = np.zeros((per, 3))
        p[:, k] = rng.uniform(-0.05, 1.05, per)
        ro = p + _unit(rng.standard_normal((per, 3))) * rng.uniform(0.5, 3, (per, 1))
        o.append(ro), d.append(_unit(p + rng.standard_normal((per, 3)) * 0.01 - ro))
    ro = rng.uniform(-2, 2, (per, 3))
    o.append(ro), d.append(_unit(rng.standard_normal((per, 3))))
    o, d = np.concatenate(o).astype(F32), np.concatenate(d).astype(F32)
    n = len(o)
    args = [mk_ray(_cols(o), _cols(d), n)]
    m = np.asarray(natives().debug_intersect(*args).f["material"])
    cover = {"red": (m == 3, MIN_BRANCH), "green": (m == 4, MIN_BRANCH), "blue": (m == 5, MIN_BRANCH), "none": (m == 0, MIN_BRANCH)}
    return args, n, cover


def directed_triangle(rng):
    from oracle import glsl_math as M
    from oracle import glsl_values as V
    from oracle.portal_oracle import sub, xyz

    up = lambda x: np.nextafter(F32(x), F32(np.inf))
    dn = lambda x: np.nextafter(F32(x), F32(-np.inf))
    # the unit right triangle scaled by a power of two, a ray straight down from height s: u = px, v = py exactly
    k = np.arange(1, 64) / 64.0
    pts = [(0.0, q) for q in k] + [(-0.0, q) for q in k] + [(up(0), q) for q in k] + [(dn(0), q) for q in k]                      # u == 0 and either side
    pts += [(q, 0.0) for q in k] + [(q, -0.0) for q in k] + [(q, up(0)) for q in k] + [(q, dn(0)) for q in k]                     # v == 0
    pts += [(q, 1.0 - q) for q in k] + [(F32(q), up(1.0 - q)) for q in k] + [(F32(q), dn(1.0 - q)) for q in k]                    # u + v == 1
    pts += [(0.0, 0.0), (1.0, 0.0), (0.0, 1.0), (up(1), 0.0), (0.0, up(1))] * 8
    pts = np.array(pts, F32)
    scales = np.array([1.0, 2.0, 0.5, 4.0], F32)
    px, py, s = np.tile(pts[:, 0], 4), np.tile(pts[:, 1], 4), np.repeat(scales, len(pts))
    m = len(px)
    zero = np.zeros(m, F32)
    exact = dict(o=np.stack([px * s, py * s, s], 1), d=np.stack([zero, zero, -np.ones(m, F32)], 1), v0=np.zeros((m, 3), F32),
                 v1=np.stack([s, zero, zero], 1), v2=np.stack([zero, s, zero], 1))
    # general position: front, back-facing, behind the origin (negative t), in the triangle's plane
    per = 512
    parts = [exact]
    for kind in ("front", "back", "behind", "in_plane", "outside"):
        v0, e1, e2 = rng.uniform(-1, 1, (per, 3)), rng.standard_normal((per, 3)), rng.standard_normal((per, 3))
        nrm = _unit(np.cross(e1, e2))
        uv = rng.dirichlet([1, 1, 1], per)[:, :2]
        if kind == "outside":
            uv = uv + rng.choice([-1.0, 1.0], (per, 1)) * rng.uniform(0.6, 2, (per, 2))
        p = v0 + e1 * uv[:, :1] + e2 * uv[:, 1:]
        if kind == "in_plane":
            ro = v0 + e1 * 3.0
            rd = _unit(p - ro)
        else:
            side = -1.0 if kind == "back" else 1.0
            ro = p + nrm * side * rng.uniform(0.5, 3, (per, 1)) + _perp(rng, nrm) * rng.uniform(0, 1, (per, 1))
            rd = _unit(p - ro) * (-1.0 if kind == "behind" else 1.0)
        parts.append(dict(o=ro, d=rd, v0=v0, v1=v0 + e1, v2=v0 + e2))
    # exactly in the plane: the xy triangle, rays with d.z = 0 from z = 0
    ang = rng.uniform(0, 6.28, per)
    zed = np.zeros(per)
    parts.append(dict(o=np.stack([rng.uniform(-2, 2, per), rng.uniform(-2, 2, per), zed], 1), d=np.stack([np.cos(ang), np.sin(ang), zed], 1),
                      v0=np.zeros((per, 3)), v1=np.tile([1.0, 0, 0], (per, 1)), v2=np.tile([0, 1.0, 0], (per, 1))))
    g = {key: np.concatenate([np.asarray(p[key], np.float64) for p in parts]).astype(F32) for key in ("o", "d", "v0", "v1", "v2")}
    n = len(g["o"])
    args = [mk_ray(_cols(g["o"]), _cols(g["d"]), n), v3(*_cols(g["v0"])), v3(*_cols(g["v1"])), v3(*_cols(g["v2"]))]
    r, v0, v1, v2 = args
    ro, rd = xyz(r.f["o"]), xyz(r.f["d"])
    v1v0, v2v0, rov0 = sub(v1, v0), sub(v2, v0), sub(ro, v0)
    nn = V.cross(v1v0, v2v0)
    q = V.cross(rov0, rd)
    dot = V.dot(rd, nn)
    dd = M.div(F32(1.0), dot)
    u, v, t = M.mul(dd, V.dot(V.neg(q), v2v0)), M.mul(dd, V.dot(q, v1v0)), M.mul(dd, V.dot(V.neg(nn), rov0))
    with np.errstate(all="ignore"):
        miss = M.lt(u, F32(0)) | M.lt(v, F32(0)) | M.gt(M.add(u, v), F32(1))
        uv1 = M.add(u, v)
    tiny = np.abs(F32(1e-45))
    cover = {"hit": (~miss, MIN_BRANCH), "u < 0": (M.lt(u, F32(0)), MIN_BRANCH), "v < 0": (~M.lt(u, F32(0)) & M.lt(v, F32(0)), MIN_BRANCH),
             "u + v > 1": (~M.lt(u, F32(0)) & ~M.lt(v, F32(0)) & M.gt(uv1, F32(1)), MIN_BRANCH),
             "back-facing hit": (~miss & (dot > 0), MIN_BRANCH), "hit with t < 0": (~miss & (t < 0), MIN_BRANCH),
             "u == 0": (u == 0, MIN_EDGE), "u one step above 0": (u == tiny, MIN_EDGE), "u one step below 0": (u == -tiny, MIN_EDGE),
             "v == 0": (v == 0, MIN_EDGE), "v one step above 0": (v == tiny, MIN_EDGE), "v one step below 0": (v == -tiny, MIN_EDGE),
             "u + v == 1": (uv1 == 1, MIN_EDGE), "u + v one step above 1": (uv1 == up(1), MIN_EDGE), "u + v one step below 1": (uv1 == dn(1), MIN_EDGE),
             "dot(rd, n) == 0": (dot == 0, MIN_EDGE)}
    return args, n, cover


def _plane_lanes(rng):
    """(o (n,4), d (n,4), inv (n,4,4), normal (n,3)) float32 for the plane tests: rays by geometry in the frames of affine matrices, and exact
    set-ups under identity / translation matrices for the zeros."""
    per = 512
    O, D, INV, N = [], [], [], []

    def emit(o, d, inv, nrm):
        m = len(o)
        o = np.concatenate([o, np.ones((m, 1))], 1) if o.shape[1] == 3 else o
        d = np.concatenate([d, np.zeros((m, 1))], 1) if d.shape[1] == 3 else d
        O.append(o), D.append(d), INV.append(inv), N.append(nrm)

    def world(inv, p_local):
        fwd = np.linalg.inv(inv)
        return np.einsum("nij,nj->ni", fwd[:, :3, :3], p_local) + fwd[:, :3, 3]

    for kind in ("hit", "away", "parallel_general"):
        inv = rigid(rng, per, scale=True)
        fwd = np.linalg.inv(inv)
        nrm = fwd[:, :3, 2] * rng.uniform(0.5, 2, (per, 1))
        target = world(inv, np.concatenate([rng.uniform(-2, 2, (per, 2)), np.zeros((per, 1))], 1))
        ro = world(inv, np.concatenate([rng.uniform(-2, 2, (per, 2)), rng.uniform(0.3, 3, (per, 1)) * rng.choice([-1, 1], (per, 1))], 1))
        rd = _unit(target - ro)
        if kind == "away":
            rd = -rd
        if kind == "parallel_general":
            rd = _unit(np.einsum("nij,nj->ni", fwd[:, :3, :3], np.concatenate([rng.standard_normal((per, 2)), np.zeros((per, 1))], 1)))
        emit(ro, rd, inv, nrm)
    # exact: identity with a dyadic translation; heights 0, -0, +-h; directions with d.z 0, +-1, tilted
    ident = np.tile(np.eye(4), (per, 1, 1))
    tz = rng.choice([0.0, 0.5, -0.5, 2.0], per)
    ident[:, 2, 3] = tz
    oz = rng.choice([0.0, -0.0, 1.0, -1.0, 0.25], per) - tz
    oz = np.where(rng.random(per) < 0.25, -0.0, oz)
    ident[:, 2, 3] = np.where(np.signbit(oz) & (oz == 0), 0.0, ident[:, 2, 3])
    dzs = rng.choice([0.0, -0.0, 1.0, -1.0, 0.5], per)
    dxy = np.round(rng.uniform(-2, 2, (per, 2)) * 4) / 4
    emit(np.stack([dxy[:, 0], dxy[:, 1], oz], 1), np.stack([dxy[:, 1], dxy[:, 0], dzs], 1), ident, np.tile([0, 0, 1.0], (per, 1)))
    # -0 in o'.z.  The product chain starts from +0, so a zero sum is +0 unless it UNDERFLOWED from a negative value: z row (-2^-80, -0, -0, -0) against
    # an origin with x <= 2^-72 (the first term rounds to -0) and y, z > 0 (each further term adds -0); rows 0 and 1 take y and z, the direction's
    # x = +-2^79 gives d'.z = -+0.5
    q = per // 2
    inv = np.zeros((q, 4, 4))
    inv[:, 0, 1], inv[:, 1, 2], inv[:, 3, 3] = 1.0, 1.0, 1.0
    inv[:, 2, :] = [-(2.0 ** -80), -0.0, -0.0, -0.0]
    ro = np.stack([2.0 ** -75 * rng.integers(1, 9, q), rng.uniform(0.25, 2, q), rng.uniform(0.25, 2, q)], 1)
    rd = np.stack([2.0 ** 79 * rng.choice([-1.0, 1.0], q), rng.uniform(-1, 1, q), rng.uniform(-1, 1, q)], 1)
    emit(ro, rd, inv, np.tile([1.0, 0.0, 0.0], (q, 1)))
    # degenerate: zero-length and subnormal directions, an all-NaN matrix, an inf element
    q = per // 2
    for kind in ("zero_dir", "subnormal_dir", "nan_matrix", "inf_element"):
        inv = rigid(rng, q)
        ro = rng.uniform(-2, 2, (q, 3))
        rd = _unit(rng.standard_normal((q, 3)))
        if kind == "zero_dir":
            rd = np.zeros((q, 3)) * rng.choice([-1.0, 1.0], (q, 3))
        if kind == "subnormal_dir":
            rd = rd * 2.0 ** rng.integers(-148, -120, (q, 1))
        if kind == "nan_matrix":
            inv = np.full((q, 4, 4), np.nan)
        if kind == "inf_element":
            inv[np.arange(q), rng.integers(0, 3, q), rng.integers(0, 4, q)] = rng.choice([np.inf, -np.inf], q)
        emit(ro, rd, inv, np.linalg.inv(rigid(rng, q))[:, :3, 2])
    with np.errstate(all="ignore"):
        return tuple(np.concatenate(x).astype(F32) for x in (O, D, INV, N))


def directed_plane_intersect(rng):
    from oracle import glsl_math as M
    from oracle import glsl_values as V

    o, d, inv, nrm = _plane_lanes(rng)
    n = len(o)
    args = [mk_ray(tuple(o.T), tuple(d.T), n), mat_from(inv), v3(*_cols(nrm))]
    with np.errstate(all="ignore"):
        op, dp = V.mat_vec(args[1], args[0].f["o"]), V.mat_vec(args[1], args[0].f["d"])
        ln = V.length(dp)
        t = M.div(M.neg(op.c[2]), V.normalize(dp).c[2])
        finite = np.isfinite(t)
        nan_m = np.isnan(inv).all(axis=(1, 2))
        inf_m = np.isinf(inv).any(axis=(1, 2))
    cover = {"hit": (finite & (t > 0), MIN_BRANCH), "t < 0": (t < 0, MIN_BRANCH), "d'.z == 0": (dp.c[2] == 0, MIN_EDGE), "o'.z == 0": (op.c[2] == 0, MIN_EDGE), "-0 in o'.z": ((op.c[2] == 0) & np.signbit(op.c[2]), MIN_EDGE),
             "t == 0": (t == 0, MIN_EDGE), "zero-length direction": (ln == 0, MIN_EDGE), "all-NaN matrix": (nan_m, MIN_EDGE),
             "inf element": (inf_m, MIN_EDGE), "direction of subnormal length": ((np.abs(d[:, :3]).max(axis=1) > 0) & (np.linalg.norm(d[:, :3].astype(np.float64), axis=1) < 2.0 ** -126), MIN_EDGE)}
    return args, n, cover


def directed_plane_intersect_normalized(rng):
    per = 128
    z = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, np.inf, np.nan], F32)
    oz, dz = (g.reshape(-1) for g in np.meshgrid(z, z, indexing="ij"))
    oz, dz = np.tile(oz, per // 8), np.tile(dz, per // 8)
    n = len(oz)
    xy = (np.round(rng.uniform(-2, 2, (n, 4)) * 8) / 8).astype(F32)
    args = [mk_ray((xy[:, 0], xy[:, 1], oz), (xy[:, 2], xy[:, 3], dz), n)]
    neg0 = (oz == 0) & np.signbit(oz)
    cover = {"-0 in o.z": (neg0, MIN_EDGE), "o.z == +0": ((oz == 0) & ~neg0, MIN_EDGE), "d.z == 0": (dz == 0, MIN_EDGE), "NaN": (np.isnan(oz) | np.isnan(dz), MIN_EDGE)}
    return args, n, cover


def directed_my_refract(rng):
    from oracle import glsl_math as M
    from oracle import glsl_values as V

    per = 768
    D, N, RI = [], [], []
    for kind in ("outside", "inside"):
        nrm = _unit(rng.standard_normal((per, 3))) * np.where(rng.random((per, 1)) < 0.5, 1.0, rng.uniform(0.5, 2, (per, 1)))   # (the function expects a unit normal)
        ang = rng.uniform(0.02, 1.55, per)
        t = _perp(rng, nrm)
        sgn = 1.0 if kind == "outside" else -1.0
        dr = (_unit(nrm) * np.cos(ang)[:, None] * sgn + t * np.sin(ang)[:, None]) * rng.uniform(0.5, 2, (per, 1))
        ri = rng.choice([0.0, 1.0, np.inf, 1.5, 0.6, 2.4, 1.0 / 1.5], per, p=[0.1, 0.1, 0.1, 0.2, 0.2, 0.15, 0.15])
        D.append(dr), N.append(nrm), RI.append(ri)
    # d == 0 exactly: ri 1 with the direction at right angles (c = 0, from inside) or a hair off it (c = 2^-13: 1 - c c rounds to 1, from outside)
    e = np.eye(3)
    for k in range(3):
        for j in range(3):
            if j == k:
                continue
            for s in (1.0, -1.0):
                for tilt in (0.0, 2.0 ** -13, 2.0 ** -14, 2.0 ** -20):
                    for scale in (1.0, 2.0, 0.5, 4.0, 0.25, 8.0, 0.125, 16.0):
                        D.append((e[k] * s + e[j] * tilt)[None, :]), N.append((e[j] * scale)[None, :]), RI.append(np.array([1.0]))
    dr, nrm, ri = np.concatenate(D).astype(F32), np.concatenate(N).astype(F32), np.concatenate(RI).astype(F32)
    n = len(dr)
    args = [v3(*_cols(dr)), v3(*_cols(nrm)), ri]
    with np.errstate(all="ignore"):
        outside = M.gt(V.dot(args[1], args[0]), F32(0))
        r = V.select(outside, ri, M.div(F32(1.0), ri))
        nn = V.select(outside, V.neg(args[1]), args[1])
        c = M.neg(V.dot(nn, V.normalize(args[0])))
        dd = M.sub(F32(1.0), M.mul(M.mul(r, r), M.sub(F32(1.0), M.mul(c, c))))
    cover = {"from outside, d > 0": (outside & (dd > 0), MIN_BRANCH), "from inside, d > 0": (~outside & (dd > 0), MIN_BRANCH),
             "total internal reflection (d < 0)": (dd < 0, MIN_BRANCH), "d == 0 from outside": (outside & (dd == 0), MIN_EDGE),
             "d == 0 from inside": (~outside & (dd == 0), MIN_EDGE), "refractive_index 0": (ri == 0, MIN_EDGE), "refractive_index 1": (ri == 1, MIN_EDGE),
             "refractive_index inf": (np.isinf(ri), MIN_EDGE)}
    return args, n, cover


# |dot / (|a| |b|) - 1| against 0.01f: the difference is a multiple of 2^-24 (the quotient lies in [0.5, 1)), 0.01f is 167772.16 of them, so
# equality cannot happen; the nearest values either side are 167772 and 167773 steps
COLLINEAR_BELOW, COLLINEAR_ABOVE = 167772 * 2.0 ** -24, 167773 * 2.0 ** -24


def directed_collinear(rng):
    from oracle import glsl_math as M
    from oracle import glsl_values as V

    per = 512
    a = _unit(rng.standard_normal((per, 3))) * rng.uniform(0.5, 2, (per, 1))
    A = [a, a, a, np.zeros((64, 3)), a[:64], np.round(a * 4) / 4]
    B = [a * rng.uniform(0.5, 2, (per, 1)), -a * rng.uniform(0.5, 2, (per, 1)), _perp(rng, a), a[:64], np.zeros((64, 3)), None]
    p = np.round(a * 4) / 4          # dot exactly 0: (x, y, z) . (y, -x, 0) with quarter-integers
    B[5] = np.stack([p[:, 1], -p[:, 0], np.zeros(per)], 1)
    # around the threshold: a = e_x, b = (c, s, 0) with c near 0.99 -- a search over candidates for quotients exactly one step either side
    m = 1 << 16
    c = (0.99 + rng.uniform(-3e-6, 3e-6, m))
    cand_b = np.stack([c, np.sqrt(1 - c * c), np.zeros(m)], 1).astype(F32)
    cand_a = np.tile(np.array([1.0, 0, 0], F32), (m, 1))
    with np.errstate(all="ignore"):
        e = M.absf(M.sub(M.div(V.dot(v3(*_cols(cand_a)), v3(*_cols(cand_b))), M.mul(V.length(v3(*_cols(cand_a))), V.length(v3(*_cols(cand_b))))), F32(1.0)))
    for target in (COLLINEAR_BELOW, COLLINEAR_ABOVE):
        idx = np.flatnonzero(e == F32(target))[:96]
        A.append(cand_a[idx]), B.append(cand_b[idx])
    idx = rng.integers(0, m, 1024)
    A.append(cand_a[idx]), B.append(cand_b[idx])
    a, b = np.concatenate(A).astype(F32), np.concatenate(B).astype(F32)
    n = len(a)
    args = [v3(*_cols(a)), v3(*_cols(b))]
    with np.errstate(all="ignore"):
        dot = V.dot(args[0], args[1])
        q = M.div(dot, M.mul(V.length(args[0]), V.length(args[1])))
        e = M.absf(M.sub(q, F32(1.0)))
    zero_len = (np.abs(a).max(axis=1) == 0) | (np.abs(b).max(axis=1) == 0)
    cover = {"collinear": (e < M.lit("0.01"), MIN_BRANCH), "not collinear": (~(e < M.lit("0.01")), MIN_BRANCH), "dot == 0": ((dot == 0) & ~zero_len, MIN_EDGE),
             "zero-length vector": (zero_len, MIN_EDGE), "parallel (q == 1)": (q == 1, MIN_EDGE), "antiparallel (q == -1)": (q == -1, MIN_EDGE),
             "one step below 0.01": (e == F32(COLLINEAR_BELOW), MIN_EDGE), "one step above 0.01": (e == F32(COLLINEAR_ABOVE), MIN_EDGE)}
    return args, n, cover


def directed_normalize_normal(rng):
    from oracle import glsl_values as V

    args, n, _ = directed_collinear(rng)
    with np.errstate(all="ignore"):
        dot = V.dot(V.normalize(args[0]), args[1])
    a = np.stack([np.asarray(c) for c in args[0].c], 1)
    cover = {"flipped": (dot > 0, MIN_BRANCH), "kept": (dot < 0, MIN_BRANCH), "dot == 0": (dot == 0, MIN_EDGE), "zero-length normal": (np.abs(a).max(axis=1) == 0, MIN_EDGE)}
    return args, n, cover


def _uv_lanes(rng):
    gx = np.arange(-8 * 32, 8 * 32 + 1) / 32.0            # cell borders of every pattern (multiples of 1/32), negative halves included
    gy = np.arange(-2 * 16, 2 * 16 + 1) / 8.0 + 1.0 / 64
    u, v = (g.reshape(-1) for g in np.meshgrid(gx, gy, indexing="ij"))
    big = np.concatenate([2.0 ** rng.integers(24, 40, 256) * rng.choice([-1, 1], 256), [np.inf, -np.inf, np.nan, 2.0 ** 24, -(2.0 ** 24)]])
    rnd = rng.uniform(-6, 6, (4096, 2))
    # the thin bands of color_grid3 (0.94 <= dist <= 0.985): points near the cell border on either side of the diagonal
    edge = rng.uniform(0.47, 0.4925, 2048) * rng.choice([-1, 1], 2048)
    other = rng.uniform(-0.45, 0.45, 2048)
    swap = rng.random(2048) < 0.5
    band = (np.stack([np.where(swap, edge, other), np.where(swap, other, edge)], 1) + 0.5 + rng.integers(-3, 3, (2048, 2))) * 2.0
    # color_grid3's two thresholds met exactly (and one step either side): uv.x = 1 + 0.985f gives fract(uv.x / 2) - 0.5 = 0.985f / 2, uv.x = 1 - 0.94f
    # gives -(0.94f / 2), both without a rounding; the other coordinate stays well inside
    thr = np.array([F32(1) + F32(0.985), F32(1) - F32(0.94)], F32)
    thr = np.concatenate([thr, np.nextafter(thr, F32(4)), np.nextafter(thr, F32(-4))])
    tx, ty = (g.reshape(-1) for g in np.meshgrid(thr, (1.0 + np.arange(-48, 48) / 128.0).astype(F32), indexing="ij"))
    uu = np.concatenate([u, v, big, rng.uniform(-4, 4, len(big)), rnd[:, 0], band[:, 0], tx, ty])
    vv = np.concatenate([v, u, rng.uniform(-4, 4, len(big)), big, rnd[:, 1], band[:, 1], ty, tx])
    return uu.astype(F32), vv.astype(F32)


def directed_grid(name):
    def make(rng):
        from oracle import glsl_math as M
        from oracle import glsl_values as V
        from oracle.glsl_values import Vec
        from oracle.portal_oracle import mul, sub

        u, v = _uv_lanes(rng)
        n = len(u)
        uv = Vec([u, v])
        start = v3(*(rng.uniform(0.1, 1, n).astype(F32) for _ in range(3)))
        with np.errstate(all="ignore"):
            common = {"negative uv": ((u < 0) | (v < 0), MIN_BRANCH), "|uv| >= 2^24": ((np.abs(u) >= 2.0 ** 24) | (np.abs(v) >= 2.0 ** 24), MIN_EDGE)}
            if name == "circle_sdf":
                d = natives().circle_sdf(uv)
                return [uv], n, dict(common, **{"inside a disc (d < -0.2)": (d < M.lit("-0.2"), MIN_BRANCH), "outside": (~(d < M.lit("-0.2")), MIN_BRANCH)})
            if name == "color_grid2":
                d = natives().circle_sdf(uv)
                return [start, uv], n, dict(common, **{"band 1.1": (d < M.lit("-0.2"), MIN_BRANCH), "band 0.7": (~(d < M.lit("-0.2")), MIN_BRANCH)})
            if name == "color_grid":
                f = V.map1(M.fract, mul(uv, F32(0.25)))
                sx, sy = M.step(f.c[0], F32(0.5)) == 1, M.step(f.c[1], F32(0.5)) == 1
                return [start, uv], n, dict(common, **{"x low, y low": (sx & sy, MIN_BRANCH), "x low, y high": (sx & ~sy, MIN_BRANCH), "x high, y low": (~sx & sy, MIN_BRANCH),
                                                       "x high, y high": (~sx & ~sy, MIN_BRANCH), "on a cell border (fract == 0.5 or 0)": ((f.c[0] == 0.5) | (f.c[0] == 0), MIN_EDGE)})
            f = sub(V.map1(M.fract, mul(uv, F32(0.5))), Vec([F32(0.5), F32(0.5)]))
            dist = M.mul(M.fmax(M.absf(f.c[0]), M.absf(f.c[1])), F32(2.0))
            b1, b2 = M.gt(dist, M.lit("0.985")), M.lt(dist, M.lit("0.94"))
            b3 = ~b1 & ~b2 & M.gt(f.c[0], f.c[1])
            return [start, uv], n, dict(common, **{"border (0.4)": (b1, MIN_BRANCH), "middle": (b2, MIN_BRANCH), "band 0.7": (b3, MIN_BRANCH), "band 1.2": (~b1 & ~b2 & ~b3, MIN_BRANCH),
                                                   "on a cell border (dist == 1)": (dist == 1, MIN_EDGE), "dist == 0.985f": (dist == M.lit("0.985"), MIN_EDGE),
                                                   "dist == 0.94f": (dist == M.lit("0.94"), MIN_EDGE)})
    return make


def directed_material_simple2(rng):
    per = 320
    n = per * 8
    ptypes = case("material_simple2").ptypes
    args = T.make_args("material_simple2.directed", ptypes, n, _structs(), special=False)
    combo = np.repeat(np.arange(8), per)
    args[4], args[7], args[8] = (combo & 1) != 0, (combo & 2) != 0, (combo & 4) != 0
    coef = args[3].copy()
    coef[0::4], coef[1::4] = 0.0, 1.0
    args[3] = coef
    cover = {f"grid {int(k & 1)} grid2 {int(k >> 1 & 1)} grid3 {int(k >> 2)}": (combo == k, MIN_BRANCH) for k in range(8)}
    cover.update({"normal_coef 0": (coef == 0, MIN_BRANCH), "normal_coef 1": (coef == 1, MIN_BRANCH)})
    return args, n, cover


def _structs():
    from oracle.portal_oracle import STRUCTS

    return dict(STRUCTS)


def directed_nearer(ptypes):
    def make(rng):
        from oracle.portal_oracle import SceneI, Surf

        ts = np.array([0.0, -0.0, 1.0, -1.0, 1e-45, 1e-10, 2.5, np.inf, -np.inf, np.nan, 1e10, 3.0], F32)
        rt, ct, rh, ch, rep = (g.reshape(-1) for g in np.meshgrid(ts, ts, [False, True], [False, True], np.arange(4), indexing="ij"))
        n = len(rt)
        z = np.zeros(n, F32)

        def wrap(ty, hit, t):
            s = Surf(hit.astype(bool), t.astype(F32), rng.uniform(-1, 1, n).astype(F32), z, v3(z, z, z + 1))
            return s if ty == SI else SceneI(rng.integers(0, 12, n).astype(I32), s, rng.random(n) < 0.5)

        args = [wrap(ptypes[0], rh, rt), wrap(ptypes[1], ch, ct)]
        with np.errstate(all="ignore"):
            cover = {"nearer": (ch & (ct > 0) & (~rh | (ct < rt)), MIN_BRANCH), "not nearer": (~(ch & (ct > 0) & (~rh | (ct < rt))), MIN_BRANCH),
                     "t == +0": ((ct == 0) & ~np.signbit(ct), MIN_EDGE), "t == -0": ((ct == 0) & np.signbit(ct), MIN_EDGE), "equal t": (ct == rt, MIN_EDGE),
                     "NaN t": (np.isnan(ct) | np.isnan(rt), MIN_EDGE), "inf t": (np.isinf(ct) | np.isinf(rt), MIN_EDGE),
                     "result.hit false with a small result.t": (~rh & ch & (ct > rt) & (ct > 0), MIN_EDGE)}
        return args, n, cover
    return make


def directed_process(name):
    def make(rng):
        c = case(name)
        n = 14 * 64
        args = T.make_args(name + ".directed", c.ptypes, n, _structs())
        inside = np.tile(np.arange(-1, 13), 64).astype(I32)
        args[2] = inside
        return args, n, {f"inside {k}": (inside == k, MIN_EDGE) for k in range(-1, 13)}
    return make


def directed_anaglyph(rng):
    """Both colour modes (any non-zero mode is the hue mode), channels outside [0, 1], and the green + blue sum of the right eye exactly on the 1e-6f
    threshold of the hue mode and one step either side."""
    from oracle import glsl_math as M

    n = 1536
    left = rng.uniform(-0.2, 1.2, (n, 3)).astype(F32)
    right = rng.uniform(-0.2, 1.2, (n, 3)).astype(F32)
    mode = rng.integers(-1, 3, n).astype(I32)
    e = M.lit("1e-6")
    edge = np.array([e, np.nextafter(e, F32(1)), np.nextafter(e, F32(0)), 0.0], F32)
    k = np.arange(768)
    right[k, 1] = np.where(k % 2 == 0, edge[k // 2 % 4], 0.0)
    right[k, 2] = np.where(k % 2 == 0, 0.0, edge[k // 2 % 4])
    mode[k] = 1
    mode[768::2] = 0
    args = [v3(*left.T), v3(*right.T), mode]
    with np.errstate(all="ignore"):
        sum_gb = M.add(M.clamp(right[:, 1], F32(0), F32(1)), M.clamp(right[:, 2], F32(0), F32(1)))
    cover = {"mode 0": (mode == 0, MIN_BRANCH), "hue mode": (mode != 0, MIN_BRANCH), "green + blue == 1e-6f": ((mode != 0) & (sum_gb == e), MIN_EDGE),
             "one step above": ((mode != 0) & (sum_gb == edge[1]), MIN_EDGE), "one step below": ((mode != 0) & (sum_gb == edge[2]), MIN_EDGE),
             "green + blue == 0": ((mode != 0) & (sum_gb == 0), MIN_EDGE)}
    return args, n, cover


DIRECTED = {
    "anaglyphCombineLinear(vec3,vec3,int)": directed_anaglyph,
    "cylinder(Ray,vec3,vec3,float)": directed_cylinder, "cap(Ray,vec3,vec3,float)": directed_cap, "triangle(Ray,vec3,vec3,vec3)": directed_triangle,
    "plane_intersect(Ray,mat4,vec3)": directed_plane_intersect, "plane_intersect_normalized(Ray)": directed_plane_intersect_normalized,
    "my_refract(vec3,vec3,float)": directed_my_refract, "is_collinear(vec3,vec3)": directed_collinear, "normalize_normal(vec3,vec3)": directed_normalize_normal,
    "color_grid(vec3,vec2)": directed_grid("color_grid"), "color_grid2(vec3,vec2)": directed_grid("color_grid2"), "color_grid3(vec3,vec2)": directed_grid("color_grid3"),
    "circle_sdf(vec2)": directed_grid("circle_sdf"), "material_simple2(SurfaceIntersection,Ray,vec3,float,bool,float,float,bool,bool)": directed_material_simple2,
    "nearer(SurfaceIntersection,SurfaceIntersection)": directed_nearer((SI, SI)), "nearer(SceneIntersection,SurfaceIntersection)": directed_nearer((SCI, SI)),
    "nearer(SceneIntersection,SceneIntersection)": directed_nearer((SCI, SCI)), "process_plane_intersection(SceneIntersection,SurfaceIntersection,int)": directed_process("process_plane_intersection"),
    "process_portal_intersection(SceneIntersection,SurfaceIntersection,int,int)": directed_process("process_portal_intersection"), "debug_intersect(Ray)": directed_debug_intersect,
}
# the directed lanes that run once more with a display toggle set (a uniform, so a render of their own)
TOGGLED = {"color_grid(vec3,vec2)": "_grid_disable", "color_grid3(vec3,vec2)": "_grid_disable", "color_normal(vec3,vec4)": "_angle_color_disable",
           "material_simple2(SurfaceIntersection,Ray,vec3,float,bool,float,float,bool,bool)": "both"}


@functools.lru_cache(maxsize=None)
def directed(key):
    """-> (args, n, cover) of a reference function's directed lanes, or None."""
    import zlib

    fn = DIRECTED.get(key)
    if fn is None:
        return None
    with np.errstate(all="ignore"):
        return fn(np.random.default_rng(SEED ^ zlib.crc32(key.encode())))


def _reference_key(c):
    base = case(c.base) if c.base not in ("mask", "cull") else None
    return base.key if base is not None and c.base != c.name else c.key


# -- masks and the cull -----------------------------------------------------------------------------------------------------------------
def mask_inputs(c, affine=False):
    """Matrices that conform to the mask (0 where a bit is clear, +-1 where a unit bit is set), finite vectors with magnitudes in 2^-40 .. 2^40
    (outside the deviation the header states for non-finite operands and underflowing partial sums), v.w as W says."""
    import zlib

    mname = next(m for m in MASKS if c.name in (f"transform_m_{m[0]}", f"derived_m_{m[0]}") or c.name.startswith(f"mul_m_{m[0]}_"))
    _, bits, ones, negs = mname
    rng = np.random.default_rng(SEED ^ zlib.crc32(c.name.encode()))
    n = 2048
    mag = lambda shape: (rng.uniform(1, 2, shape) * 2.0 ** rng.integers(-40, 41, shape) * rng.choice([-1.0, 1.0], shape)).astype(F32)
    small = lambda shape: (rng.uniform(-2, 2, shape)).astype(F32)
    pick = lambda shape: np.where(rng.random(shape) < 0.5, mag(shape), small(shape)).astype(F32)
    m = pick((n, 4, 4))
    for col in range(4):
        for row in range(4):
            k = 4 * col + row
            if not (bits >> k) & 1:
                m[:, row, col] = 0.0
            if (ones >> k) & 1:
                m[:, row, col] = 1.0
            if (negs >> k) & 1:
                m[:, row, col] = -1.0
    if affine:
        m[:, 3, :] = [0.0, 0.0, 0.0, 1.0]          # (a set bit says "may be non-zero": every mask of the list admits this row)
    if c.name.startswith("mul_m_"):
        v = pick((n, 4))
        w = dict(W_MODES)["PTL_W_" + c.name.rsplit("_", 1)[1]]
        if w is not None:
            v[: n // 2, 3] = w          # (the other half keeps an arbitrary w, which the W modes must not read)
        return [mat_from(m), v4(*v.T)], n
    o, d = pick((n, 4)), pick((n, 4))
    aff = np.ones(n, bool) if affine else rng.random(n) < 0.5
    o[:, 3], d[:, 3] = np.where(aff, 1.0, o[:, 3]), np.where(aff, 0.0, d[:, 3])
    from oracle.portal_oracle import Ray

    args = [mat_from(m), Ray(v4(*o.T), v4(*d.T), pick(n), rng.random(n) < 0.3)]
    if c.name.startswith("derived_m_"):
        args.append(v3(*small((n, 3)).T))
    return args, n


CULL_SPECIALS = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, 2.0 ** -126, -(2.0 ** -126), 2.0 ** -100, 2.0 ** -64, -(2.0 ** -64), 1e-20, -1e-20, 1e-6, -1e-6, 0.5, -0.5,
                          1.0, -1.0, 3.0, -3.0, 1e6, -1e6, 1e19, -1e19, 2.0 ** 63, 2.0 ** 64, -(2.0 ** 64), 2.0 ** 126, 2.0 ** 127, -(2.0 ** 127), 3.4e38, -3.4e38, np.inf,
                          -np.inf, np.nan], F32)
CULL_TILE_KINDS = ("all culled", "mixed", "none culled")


@functools.lru_cache(maxsize=None)
def cull_inputs():
    """Rays, plane matrices and bounds for the cull, 64 lanes to a tile: the adversarial families of tests/test_cull_property.py in the plane's
    frame (specials, crossings a hair either side of the bound, random bit patterns; best_t 1e10, inf, tiny), rays by geometry, and tiles
    that are culled throughout, mixed, or not at all.  -> (args, n, kind per tile, must_not_cull lanes)"""
    rng = np.random.default_rng(SEED ^ 0xC011)
    O, D, INV, N, BEST, KIND, KEEP = [], [], [], [], [], [], []

    def emit(oz, dxyz, best, inv=None, kind="free", keep=None):
        m = len(oz)
        assert m % 64 == 0
        o = np.stack([rng.uniform(-1, 1, m), rng.uniform(-1, 1, m), oz, np.ones(m)], 1)
        O.append(o), D.append(np.concatenate([dxyz, np.zeros((m, 1))], 1)), BEST.append(best)
        INV.append(np.tile(np.eye(4), (m, 1, 1)) if inv is None else inv)
        N.append(np.tile([0.0, 0.0, 1.0], (m, 1)))
        KIND.extend([kind] * (m // 64)), KEEP.append(np.zeros(m, bool) if keep is None else keep)

    with np.errstate(all="ignore"):
        s = CULL_SPECIALS.astype(np.float64)
        oz, dz, best = (g.reshape(-1) for g in np.meshgrid(s, s, np.concatenate([s[s >= 0], [1e10]]), indexing="ij"))
        m = len(oz) // 64 * 64
        oz, dz, best = oz[:m], dz[:m], best[:m]
        dxy = rng.choice([0.0, 1e-20, 1.0, 1e19], (m, 2))
        emit(oz, np.concatenate([dxy, dz[:, None]], 1), best, keep=(oz == 0) | np.isnan(oz) | np.isnan(dz) | np.isnan(best))
        # near the bound
        m = 64 * 128
        mag = lambda lo, hi: np.exp2(rng.uniform(lo, hi, m)) * rng.choice([-1.0, 1.0], m)
        dz3 = np.stack([mag(-30, 30), mag(-30, 30), mag(-30, 30)], 1)
        t_true = np.exp2(rng.uniform(-20, 20, m))
        rel = rng.choice([-1.0, 1.0], m) * np.exp2(rng.uniform(-24, -12, m)) * rng.choice([0.0, 1.0], m, p=[0.1, 0.9])
        emit(-(t_true * dz3[:, 2]), dz3, t_true * (1.0 + rel))
        # random bit patterns
        bits = lambda: rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(U32).view(F32).astype(np.float64)
        best = np.abs(bits())
        best = np.where(rng.random(m) < 0.2, np.inf, best)
        emit(bits(), np.stack([bits(), bits(), bits()], 1), best)
        # underflowing and zero products: must not be culled
        m2 = 64 * 8
        tiny = np.exp2(rng.uniform(-149, -100, m2)) * rng.choice([-1.0, 1.0], m2)
        emit(tiny, np.stack([np.ones(m2), np.zeros(m2), tiny[::-1].copy()], 1), np.exp2(rng.uniform(-60, -50, m2)), keep=np.ones(m2, bool))
        # by geometry: affine frames, the bound before / beyond the crossing, tile by tile
        for kind in CULL_TILE_KINDS:
            tiles = 24
            m3 = tiles * 64
            inv = rigid(rng, m3, scale=True)
            fwd = np.linalg.inv(inv)
            lo = np.concatenate([rng.uniform(-2, 2, (m3, 2)), rng.uniform(0.5, 3, (m3, 1))], 1)
            target = np.concatenate([rng.uniform(-2, 2, (m3, 2)), np.zeros((m3, 1))], 1)
            ro = np.einsum("nij,nj->ni", fwd[:, :3, :3], lo) + fwd[:, :3, 3]
            tw = np.einsum("nij,nj->ni", fwd[:, :3, :3], target) + fwd[:, :3, 3]
            dist = np.linalg.norm(tw - ro, axis=1)
            rd = (tw - ro) / dist[:, None]
            lane, odd = np.arange(m3) % 64, np.arange(m3) // 64 % 2 == 1
            # mixed tiles: every fifth lane's bound lies beyond its crossing; in every other one a single lane's does (lane 17)
            culled = {"all culled": np.ones(m3, bool), "none culled": np.zeros(m3, bool), "mixed": np.where(odd, lane != 17, lane % 5 != 3)}[kind]
            best = np.where(culled, dist * rng.uniform(0.2, 0.9, m3), dist * rng.uniform(1.1, 3, m3))
            O.append(np.concatenate([ro, np.ones((m3, 1))], 1)), D.append(np.concatenate([rd, np.zeros((m3, 1))], 1)), BEST.append(best), INV.append(inv)
            N.append(fwd[:, :3, 2]), KIND.extend([kind] * tiles), KEEP.append(np.zeros(m3, bool))
        o, d, inv, nrm, best, keep = (np.concatenate(x).astype(F32) if x is not KEEP else np.concatenate(x) for x in (O, D, INV, N, BEST, KEEP))
    n = len(o)
    assert n % 64 == 0 and len(KIND) == n // 64
    args = [mk_ray(tuple(o.T), tuple(d.T), n), mat_from(inv), v3(*_cols(nrm)), best]
    return args, n, np.array(KIND), keep


def cannot_be_nearer_model(oz, dz, best):
    """The three instructions of ptl_cannot_be_nearer on given (oz, dz): oz * fma(best * (1 + 2^-16), dz, oz) > 0, each step rounded to binary32 (the fma through
    binary64: a double rounding can move it by one binary32 step next to a tie, never in sign, and the sign is all that is read)."""
    oz, dz, best = (np.asarray(x, F32) for x in (oz, dz, best))
    with np.errstate(all="ignore"):
        far = (best * F32(1.0 + 2.0 ** -16)).astype(F32)
        z_far = (far.astype(np.float64) * dz.astype(np.float64) + oz.astype(np.float64)).astype(F32)
        return (oz * z_far).astype(F32) > 0


def affine_args(c):
    """Family for the PTL_AFFINE_RAYS + PTL_DROP_ZERO_TERMS build: finite values, matrices with the bottom row 0 0 0 1, rays with o.w = 1 and d.w = 0."""
    from oracle.glsl_values import Mat, Struct, Vec

    if c.base == "mask":
        return mask_inputs(c, affine=True)
    args = T.make_args(c.base + ".affine", c.ptypes, N_AFFINE, _structs(), special=False)

    def fix(v):
        if isinstance(v, Mat) and v.n == 4:
            return Mat([Vec(list(col.c[:3]) + [np.full(N_AFFINE, 1.0 if j == 3 else 0.0, F32)]) for j, col in enumerate(v.cols)])
        if isinstance(v, Struct):
            f = {k: fix(x) for k, x in v.f.items()}
            if v.tname == "Ray":
                f["o"] = Vec(list(f["o"].c[:3]) + [np.ones(N_AFFINE, F32)])
                f["d"] = Vec(list(f["d"].c[:3]) + [np.zeros(N_AFFINE, F32)])
            return Struct(v.tname, f)
        return v

    return [fix(a) for a in args], N_AFFINE


# ---- checks -------------------------------------------------------------------------------------------------------------------------
def want_bits(c, nat, args, n):
    from oracle import glsl_values as V

    with np.errstate(all="ignore"):
        vals = c.want(nat, args)
    return np.concatenate([T.leaves_array(V.expand(v, n), n) for v in vals], axis=1)


def report(c, got, want, words, who, against, columns=None):
    """One line per differing leaf: function, leaf, count, the first offending lane with its input bit patterns."""
    lines = []
    cols = range(want.shape[1]) if columns is None else columns
    for j, k in enumerate(cols):
        bad = np.flatnonzero(got[:, k] != want[:, j])
        if len(bad):
            i = int(bad[0])
            lines.append(f"{c.key} leaf {c.labels[k]}: {len(bad)} of {len(got)} lanes differ from {against}, first at lane {i}: inputs {[hex(int(w)) for w in words[i]]} -> "
                         f"{who} {hex(int(got[i, k]))} {against} {hex(int(want[i, j]))}")
    return lines


def inputs_for(c, families):
    """-> [(family, args, n, uniforms)] for one case."""
    base = basics_uniforms()
    out = []
    ref = _reference_key(c)
    ref_case = next(x for x in cases() if x.key == ref) if c.base not in ("mask", "cull") else None
    if c.base == "mask":
        if "directed" in families:
            out.append(("directed", *mask_inputs(c), base))
        return out
    if c.base == "cull":
        if "directed" in families:
            a, n, _, _ = cull_inputs()
            out.append(("directed", a, n, base))
        return out
    if "committed" in families:
        out.append(("committed", T.make_args(ref_case.name, ref_case.ptypes, N_COMMITTED, _structs()), N_COMMITTED, base))
    if "random" in families:
        out.append(("random", T.make_args(ref_case.name, ref_case.ptypes, N_RANDOM, _structs()), N_RANDOM, base))
    d = directed(ref)
    if "directed" in families and d is not None:
        out.append(("directed", d[0], d[1], base))
    if "directed" in families and ref in TOGGLED and c.key == ref:
        a, n = (d[0], d[1]) if d is not None else (T.make_args(ref_case.name, ref_case.ptypes, N_COMMITTED, _structs()), N_COMMITTED)
        which = TOGGLED[ref]
        out.append(("toggled", a, n, dict(base, **({"_grid_disable": I32(1)} if which in ("_grid_disable", "both") else {}),
                                          **({"_angle_color_disable": I32(1)} if which in ("_angle_color_disable", "both") else {}))))
    return out


@functools.lru_cache(maxsize=None)
def committed_vectors():
    store = np.load(os.path.join(T.GOLDEN_DIR, "functions.npz"))
    return {k: store[k] for k in store.files if k != "text_digest"}


def check_case(runner, c, contract=2, families=("committed", "random", "directed"), with_npz=True):
    """Run one case over its input families and compare every leaf.  -> (failure lines, lanes compared, {family: (n, leaves float32, words)})"""
    from oracle import glsl_math as M

    lines, lanes, raw = [], 0, {}
    for family, args, n, uniforms in inputs_for(c, families):
        tiled = c.base == "cull"
        got_f = runner.run(c, args, n, uniforms, tiled=tiled)
        got = leaves_to_bits(c, got_f)
        words = words_of(args, n)
        raw[family] = (n, got_f, words)
        prev = M.set_contract(contract)
        try:
            want = want_bits(c, natives(uniforms), args, n)
        finally:
            M.set_contract(prev)
        if c.base == "cull":
            lines += check_cull(c, got, got_f, want, words, runner.where)
        else:
            assert want.shape == got.shape, (c.key, want.shape, got.shape)
            lines += report(c, got, want, words, runner.where, "the restatement")
        if family == "committed" and with_npz and c.key in committed_vectors():
            lines += report(c, got, committed_vectors()[c.key], words, runner.where, "functions.npz")
        lanes += n
    return lines, lanes, raw


def check_cull(c, got, got_f, want, words, where):
    """oz, dz and the full plane test == the restatement; the device function's verdict == the model of its three instructions on the device's own
    (oz, dz); wherever it says "cannot be nearer" the full test of that lane is not nearer() than a hit at best_t, by the device's plane test and by
    the restatement's; lanes with zero / NaN / underflowing products are not culled; ptl_plane_cull is true exactly on the tiles (wavefronts) where
    all 64 lanes say so (host build: lane by lane)."""
    args, n, kinds, keep = cull_inputs()
    lines = report(c, got, want, words, where, "the restatement", columns=range(9))
    oz, dz, best = got_f[:, 0], got_f[:, 1], np.asarray(args[3], F32)
    cannot, near, ballot = got[:, 9] == 1, got[:, 10] == 1, got[:, 11] == 1
    model = cannot_be_nearer_model(oz, dz, best)
    if not np.array_equal(cannot, model):
        i = int(np.flatnonzero(cannot != model)[0])
        lines.append(f"ptl_cannot_be_nearer: {int((cannot != model).sum())} lanes differ from its three instructions, first lane {i}: oz {oz[i]!r} dz {dz[i]!r} best {best[i]!r}")
    with np.errstate(all="ignore"):
        wt = want[:, 3].view(F32)
        near_restated = (want[:, 2] == 1) & (wt > 0) & (wt < best)
    for what, bad in (("the device's own plane test", cannot & near), ("the restatement's plane test", cannot & near_restated), ("a lane that must not be culled", cannot & keep)):
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            lines.append(f"ptl_cannot_be_nearer culls {int(bad.sum())} lanes against {what}, first lane {i}: inputs {[hex(int(w)) for w in words[i]]}")
    expect = cannot.reshape(-1, 64).all(axis=1).repeat(64) if where != "host" else cannot
    if not np.array_equal(ballot, expect):
        i = int(np.flatnonzero(ballot != expect)[0])
        lines.append(f"ptl_plane_cull: {int((ballot != expect).sum())} lanes differ from the all-64-lanes verdict, first lane {i} (tile {i // 64}, {kinds[i // 64]})")
    tiles = cannot.reshape(-1, 64)
    for kind, ok in (("all culled", tiles.all(axis=1)), ("mixed", tiles.any(axis=1) & ~tiles.all(axis=1)), ("none culled", ~tiles.any(axis=1))):
        sel = kinds == kind
        if not ok[sel].all():
            lines.append(f"cull tiles laid out as `{kind}`: {int((~ok[sel]).sum())} of {int(sel.sum())} are not")
    if not (cannot.sum() > 1000 and (tiles.all(axis=1)).sum() >= 24):
        lines.append("the cull inputs no longer exercise the cull")
    return lines


def coverage_lines():
    """[(key, branch, lanes, minimum)] over every directed family (counted with the restatement's arithmetic)."""
    out = []
    for key in DIRECTED:
        _, n, cover = directed(key)
        for branch, (mask, minimum) in cover.items():
            out.append((key, branch, int(np.asarray(mask).sum()), minimum))
    return out


# ---- accuracy: the distance of the contract from real geometry -------------------------------------------------------------------------
# Largest binary64 residual of the RESTATEMENT's results on accuracy_lanes() (the hit point o + t d against the surface; Snell's law for
# my_refract), measured on the CPU on 2026-10-19 by tests/test_prelude_contract.py::test_accuracy_constants_are_the_restatements_residuals,
# which asserts that these are still what the restatement gives.  Any build may be twice that far from the geometry (the rule of
# tests/contract_sweep.TEXTURE_TOLERANCE); the builds equal the restatement bit for bit anyway.
ACCURACY_MEASURED = {"plane_intersect": 8.04e-7, "cap": 4.67e-6, "cylinder": 7.53e-6, "triangle": 6.53e-7, "my_refract": 3.25e-7}
ACCURACY_FUNCTIONS = ("plane_intersect", "cap", "cylinder", "triangle", "my_refract")


@functools.lru_cache(maxsize=None)
def accuracy_lanes(name):
    """Well-conditioned lanes of the directed family: a hit exists (by the restatement), the ray is not within 1e-3 of grazing, sizes are O(1).
    -> (args, n)"""
    from oracle import glsl_values as V

    c = case(name)
    args, n, _ = directed(c.key)
    nat = natives()
    with np.errstate(all="ignore"):
        res = nat.my_refract(*args) if name == "my_refract" else getattr(nat, name)(*args)
        f64 = lambda v: np.stack([np.asarray(x, np.float64) for x in V.expand(v, n).c[:3]], 1)
        if name == "my_refract":
            d, nr, ri = f64(args[0]), f64(args[1]), np.asarray(args[2], np.float64)
            cosi = np.abs((_unit(d) * _unit(nr)).sum(1))
            eff = np.where((d * nr).sum(1) > 0, ri, 1.0 / ri)
            ok = np.isfinite(ri) & (ri > 0.3) & (ri < 3) & (cosi > 1e-3) & (1 - eff ** 2 * (1 - cosi ** 2) > 1e-3) & (np.linalg.norm(d, axis=1) > 0.1) & (np.abs(np.linalg.norm(nr, axis=1) - 1) < 1e-6)
        else:
            t = np.asarray(res.f["t"], np.float64)
            d, o = f64(args[0].f["d"]), f64(args[0].f["o"])
            nrm = f64(res.f["n"])
            graze = np.abs((_unit(d) * _unit(nrm)).sum(1))
            ok = np.asarray(res.f["hit"]) & np.isfinite(t) & (t > 1e-2) & (t < 20) & (graze > 1e-3) & (np.abs(o).max(1) < 10) & (np.abs(np.linalg.norm(d, axis=1) - 1) < 1e-3)
            if name == "plane_intersect":
                ok &= np.isfinite(np.stack([f64(col) for col in args[1].cols], 1)).all(axis=(1, 2))
            if name in ("cap", "cylinder"):
                ok &= np.asarray(args[3]) > 0.05
    idx = np.flatnonzero(ok)
    return [V.take(V.expand(a, n), idx) for a in args], len(idx)


def residuals(name, args, n, leaves):
    """binary64 residual per lane of a result given as float32 leaves (n, k) in the case's output order."""
    from oracle import glsl_values as V

    f64 = lambda v: np.stack([np.asarray(x, np.float64) for x in V.expand(v, n).c[:3]], 1)
    leaves = np.asarray(leaves, np.float64)
    with np.errstate(all="ignore"):
        if name == "my_refract":
            d, nr, ri = _unit(f64(args[0])), _unit(f64(args[1])), np.asarray(args[2], np.float64)
            out = leaves[:, :3]
            eff = np.where((d * nr).sum(1) > 0, ri, 1.0 / ri)
            sin_i = np.linalg.norm(np.cross(d, nr), axis=1)
            sin_t = np.linalg.norm(np.cross(_unit(out), nr), axis=1)
            coplanar = np.abs((_unit(out) * _unit(np.cross(d, nr))).sum(1))
            return np.maximum(np.abs(sin_t - eff * sin_i), np.where(sin_i > 1e-6, coplanar, 0.0))
        o, d = f64(args[0].f["o"]), f64(args[0].f["d"])
        p = o + d * leaves[:, 1:2]
        if name == "plane_intersect":
            inv = np.stack([np.stack([np.asarray(x, np.float64) for x in V.expand(col, n).c], 1) for col in args[1].cols], 2)     # [lane, row, col]
            return np.abs(np.einsum("nj,nj->n", inv[:, 2, :3], p) + inv[:, 2, 3]) / np.linalg.norm(inv[:, 2, :3], axis=1)
        if name == "triangle":
            v0, v1, v2 = f64(args[1]), f64(args[2]), f64(args[3])
            return np.linalg.norm(p - (v0 + (v1 - v0) * leaves[:, 2:3] + (v2 - v0) * leaves[:, 3:4]), axis=1)
        a, b, ra = f64(args[1]), f64(args[2]), np.asarray(args[3], np.float64)
        ba = b - a
        s = ((p - a) * ba).sum(1) / (ba * ba).sum(1)
        if name == "cap":
            s = np.clip(s, 0, 1)
        return np.abs(np.linalg.norm(p - (a + ba * s[:, None]), axis=1) - ra)


def restatement_residual(name):
    from oracle import glsl_values as V

    args, n = accuracy_lanes(name)
    c = case(name)
    leaves = want_bits(c, natives(), args, n)
    as_float = np.stack([leaves[:, j].view(F32) if k == "f" else leaves[:, j].astype(F32) for j, k in enumerate(c.kinds)], 1)
    return float(residuals(name, args, n, as_float).max()), n


# ---- one build of one group, every check ------------------------------------------------------------------------------------------------
BUILDS = {"shipped": (), "O1": (), "contract1": ("PTL_CONTRACT_V1",), "affine": ("PTL_AFFINE_RAYS", "PTL_DROP_ZERO_TERMS")}


def run_build(pa, where, build, group, shipped=None):
    """Every case of `group` in one build (host build or GPU) -> (failure lines, [(case key, lanes compared)]).
    shipped / O1: functions.npz, the restatement, the equivalences, the accuracy leg.  contract1: the restatement under contract 1.
    affine (PTL_AFFINE_RAYS + PTL_DROP_ZERO_TERMS): against the shipped build's results (`shipped`: its Runner) on affine_args()."""
    runner = Runner(pa, group, where, BUILDS[build])
    lines, counts = [], []
    if group == "template":
        lines += check_pack(runner)
        counts.append(("pack_rgba8", len(pack_inputs())))
    for c in cases():
        if c.group != group or build not in c.builds:
            continue
        if build == "affine":
            if c.base == "cull":
                continue          # (its inputs are the non-finite and underflowing ones the two defines exclude)
            args, n = affine_args(c)
            got = leaves_to_bits(c, runner.run(c, args, n, basics_uniforms()))
            ref = leaves_to_bits(c, shipped.run(c, args, n, basics_uniforms()))
            lines += report(c, got, ref, words_of(args, n), f"{where} affine build", "the shipped build")
            counts.append((c.key, n))
            continue
        bad, lanes, _ = check_case(runner, c, contract=1 if build == "contract1" else 2, with_npz=build != "contract1")
        lines += bad
        counts.append((c.key, lanes))
        if build != "contract1" and c.group == "library" and c.name in ACCURACY_FUNCTIONS:
            args, n = accuracy_lanes(c.name)
            got = runner.run(c, args, n, basics_uniforms())
            worst = float(residuals(c.name, args, n, got).max())
            if not worst <= 2 * ACCURACY_MEASURED[c.name]:
                lines.append(f"{c.key}: binary64 residual {worst:.3g} on {n} well-conditioned lanes, allowed {2 * ACCURACY_MEASURED[c.name]:.3g}")
    return lines, counts
