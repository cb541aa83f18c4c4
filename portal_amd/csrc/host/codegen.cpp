// codegen.cpp -- see codegen.h.
#include "codegen.h"
#include "glsl_hoist.h"
#include "glsl_tokens.h"

#include <cstdlib>
#include <cstring>

#include <algorithm>
#include <charconv>
#include <cmath>
#include <cstdio>
#include <set>
#include <sstream>
#include <tuple>

namespace ptl {

// ------------------------------------------------------------------------------------------
// template engine (src/code_generation.rs)
// ------------------------------------------------------------------------------------------
void LineNumbersByKey::offset(int lines) {
    for (auto& kv : ranges) {
        kv.second.start += lines;
        kv.second.end += lines;
    }
}
void LineNumbersByKey::add(const ElementKey& key, LineRange r) {
    if (ranges.count(key)) throw std::logic_error("LineNumbersByKey: duplicate key " + key.kind + ":" + key.name);
    ranges[key] = r;
}
void LineNumbersByKey::extend(const LineNumbersByKey& other) {
    for (auto& kv : other.ranges) add(kv.first, kv.second);
}
bool LineNumbersByKey::get_identifier(int line_no, ElementKey* key, int* local_line) const {
    for (auto& kv : ranges) {
        if (line_no >= kv.second.start && line_no < kv.second.end) {
            if (key) *key = kv.first;
            if (local_line) *local_line = line_no - kv.second.start + 1;
            return true;
        }
    }
    return false;
}

void StringStorage::add_string(const std::string& s) {
    current_line_no += (int)std::count(s.begin(), s.end(), '\n');
    storage += s;
}
void StringStorage::add_identifier_string(const ElementKey& id, const std::string& s) {
    int start = current_line_no;
    add_string(s);
    line_numbers.add(id, LineRange{start, current_line_no + 1});
}
void StringStorage::add_string_storage(StringStorage other) {
    other.line_numbers.offset(current_line_no - 1);
    add_string(other.storage);
    line_numbers.extend(other.line_numbers);
}

StringStorage apply_template(const std::string& tmpl, std::map<std::string, StringStorage> storages) {
    StringStorage result;
    size_t pos = 0;
    bool is_name = false;
    for (;;) {
        size_t next = tmpl.find("//%", pos);
        std::string piece = tmpl.substr(pos, next == std::string::npos ? std::string::npos : next - pos);
        if (is_name) {
            auto it = storages.find(piece);
            if (it == storages.end()) throw std::logic_error("apply_template: no storage for slot `" + piece + "`");
            result.add_string_storage(std::move(it->second));
            storages.erase(it);
        } else {
            result.add_string(piece);
        }
        if (next == std::string::npos) break;
        pos = next + 3;
        is_name = !is_name;
    }
    return result;
}

const std::set<std::string>& section_names() {
    static const std::set<std::string> known = {"slices", "passes", "refine", "refine_slices"};
    return known;
}

std::string select_sections(const std::string& text, const std::set<std::string>& names) {
    auto known = [](const std::string& name) {
        if (!section_names().count(name)) throw std::logic_error("select_sections: unknown section name `" + name + "`");
    };
    for (const std::string& n : names) known(n);
    struct Section {
        bool outer, condition, in_else;  // the enclosing sections are selected; what `if` asked for held; behind its `else`
    };
    std::vector<Section> open;
    bool selected = true;
    std::string out;
    for (size_t pos = 0, line_no = 1; pos < text.size(); ++line_no) {
        const size_t eol = text.find('\n', pos);
        const size_t next = eol == std::string::npos ? text.size() : eol + 1;
        size_t b = pos, e = eol == std::string::npos ? text.size() : eol;
        while (b < e && (text[b] == ' ' || text[b] == '\t')) ++b;
        while (e > b && (text[e - 1] == ' ' || text[e - 1] == '\t' || text[e - 1] == '\r')) --e;
        const std::string line = text.substr(b, e - b);
        auto fail = [&](const char* what) { throw std::logic_error("select_sections: line " + std::to_string(line_no) + ": " + what); };
        if (line.compare(0, 6, "//%if ") == 0) {
            std::string name = line.substr(6);
            const bool negated = !name.empty() && name[0] == '!';
            if (negated) name.erase(0, 1);
            known(name);
            open.push_back({selected, (names.count(name) != 0) != negated, false});
            selected = open.back().outer && open.back().condition;
        } else if (line == "//%else") {
            if (open.empty()) fail("`else` without an `if`");
            if (open.back().in_else) fail("a second `else`");
            open.back().in_else = true;
            selected = open.back().outer && !open.back().condition;
        } else if (line == "//%end") {
            if (open.empty()) fail("`end` without an `if`");
            selected = open.back().outer;
            open.pop_back();
        } else if (selected) {
            out.append(text, pos, next - pos);
        }
        pos = next;
    }
    if (!open.empty()) throw std::logic_error("select_sections: " + std::to_string(open.size()) + " section(s) not closed");
    return out;
}

// ------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------
std::string format_lower_exp(double v) {
    if (std::isnan(v)) return "NaN";
    if (std::isinf(v)) return v > 0 ? "inf" : "-inf";
    char buf[64];
    auto res = std::to_chars(buf, buf + sizeof buf, v, std::chars_format::scientific);
    std::string s(buf, res.ptr);  // d.ddde[+-]XX
    size_t e = s.find('e');
    std::string mant = s.substr(0, e), exp = s.substr(e + 1);
    bool neg = !exp.empty() && exp[0] == '-';
    if (!exp.empty() && (exp[0] == '-' || exp[0] == '+')) exp.erase(0, 1);
    while (exp.size() > 1 && exp[0] == '0') exp.erase(0, 1);
    return mant + "e" + (neg ? "-" : "") + exp;
}

size_t uniform_type_size(UniformType t) {
    switch (t) {
        case UniformType::Mat4: return 64;
        case UniformType::Float1: return 4;
        case UniformType::Int1: return 4;
        case UniformType::Float2: return 8;
        case UniformType::Float3: return 12;
        case UniformType::Sampler: return 16;
    }
    return 0;
}

namespace {

const char* cxx_type(UniformType t) {
    switch (t) {
        case UniformType::Mat4: return "mat4";
        case UniformType::Float1: return "float";
        case UniformType::Int1: return "int";
        case UniformType::Float2: return "vec2";
        case UniformType::Float3: return "vec3";
        case UniformType::Sampler: return "sampler2D";
    }
    return "?";
}

const std::string& matrix_name(const Scene& s, int idx, const Object& o) {
    if (idx < 0 || idx >= (int)s.matrices.size()) throw SceneError("object `" + o.name + "` refers to no matrix");
    return s.matrices[idx].name;
}
std::string normal_name(const std::string& m) { return m + "_mat"; }
std::string inverse_name(const std::string& m) { return m + "_mat_inv"; }
std::string teleport_name(const std::string& from, const std::string& to) { return from + "_to_" + to + "_mat_teleport"; }

std::string f32_literal(double v) { return format_lower_exp(v) + "f"; }
const char* bool_lit(bool b) { return b ? "true" : "false"; }

}  // namespace

// ------------------------------------------------------------------------------------------
// uniforms (scene.rs:424-543)
// ------------------------------------------------------------------------------------------
std::vector<std::string> scene_texture_list(const Scene& scene) {
    std::set<std::string> names;
    for (auto& t : scene.textures) names.insert(t.name);
    for (auto& v : scene.videos) names.insert(v);
    std::vector<std::string> out;
    for (auto& n : names) out.push_back(n + "_tex");
    return out;
}

std::vector<UniformDesc> scene_uniform_list(const Scene& scene) {
    std::set<std::string> mats;  // BTreeSet: sorted, unique
    for (const Object& o : scene.objects) {
        if (o.kind == Object::DebugMatrix || !o.portal) {
            const std::string& m = matrix_name(scene, o.m0, o);
            mats.insert(normal_name(m));
            mats.insert(inverse_name(m));
        } else {
            const std::string& a = matrix_name(scene, o.m0, o);
            const std::string& b = matrix_name(scene, o.m1, o);
            mats.insert(normal_name(a));
            mats.insert(inverse_name(a));
            mats.insert(normal_name(b));
            mats.insert(inverse_name(b));
            mats.insert(teleport_name(a, b));
            if (a != b) mats.insert(teleport_name(b, a));
        }
    }
    for (const MatrixEntry& m : scene.matrices) {
        if (!m.named) continue;
        mats.insert(normal_name(m.name));
        mats.insert(inverse_name(m.name));
    }
    std::vector<UniformDesc> out;
    for (auto& n : mats) out.push_back({n, UniformType::Mat4, 0});
    for (size_t k = 0; k < scene.uniforms.size(); ++k) {
        const UniformEntry& u = scene.uniforms[k];
        if (u.name.empty()) continue;  // inline uniforms are not visible
        const Uniform* now = scene.resolved_uniform((int)k);
        if (now && now->kind == Uniform::Trefoil) {  // 18 packed ints `ts_<i>_<name>_u` (scene.rs:488-492)
            for (int i = 0; i < 18; ++i) out.push_back({"ts_" + std::to_string(i) + "_" + u.name + "_u", UniformType::Int1, 0});
            continue;
        }
        auto v = scene.eval_uniform((int)k);
        if (!v) continue;
        out.push_back({u.name + "_u", v->kind == UniformValue::Float ? UniformType::Float1 : UniformType::Int1, 0});
    }
    static const std::pair<const char*, UniformType> builtins[] = {
        {"_camera", UniformType::Mat4},
        {"_camera_left_eye", UniformType::Mat4},
        {"_camera_right_eye", UniformType::Mat4},
        {"_camera_mul_inv", UniformType::Mat4},
        {"_camera_in_subspace", UniformType::Int1},
        {"_left_eye_in_subspace", UniformType::Int1},
        {"_right_eye_in_subspace", UniformType::Int1},
        {"_resolution", UniformType::Float2},
        {"_ray_tracing_depth", UniformType::Int1},
        {"_aa_count", UniformType::Int1},
        {"_aa_start", UniformType::Int1},
        {"_draw_side_by_side", UniformType::Int1},
        {"_offset_after_material", UniformType::Float1},
        {"_draw_anaglyph", UniformType::Int1},
        {"_anaglyph_p", UniformType::Float1},
        {"_anaglyph_q", UniformType::Float1},
        {"_anaglyph_mode", UniformType::Int1},
        {"_draw_depth_map", UniformType::Int1},
        {"_depth_map_min", UniformType::Float1},
        {"_depth_map_max", UniformType::Float1},
        {"_camera_scale", UniformType::Float1},
        {"_left_eye_scale", UniformType::Float1},
        {"_right_eye_scale", UniformType::Float1},
        {"_t_start", UniformType::Float1},
        {"_t_end", UniformType::Float1},
        {"_view_angle", UniformType::Float1},
        {"_use_panini_projection", UniformType::Int1},
        {"_use_360_camera", UniformType::Int1},
        {"_use_180_camera", UniformType::Int1},
        {"_angle_color_disable", UniformType::Int1},
        {"_darken_by_distance", UniformType::Int1},
        {"_grid_disable", UniformType::Int1},
        {"_black_border_disable", UniformType::Int1},
        {"_panini_param", UniformType::Float1},
        {"_teleport_external_ray", UniformType::Int1},
        {"_external_ray_a", UniformType::Float3},
        {"_external_ray_b", UniformType::Float3},
    };
    for (auto& b : builtins) out.push_back({b.first, b.second, 0});
    return out;
}

bool UniformUpload::same_value(const UniformUpload& o) const {
    if (type != o.type) return false;
    if (type == UniformType::Int1) return i == o.i;
    return std::memcmp(f, o.f, uniform_type_size(type)) == 0;  // bit patterns: NaN == NaN, -0 != +0
}

std::vector<UniformUpload> evaluate_scene_uniforms(const Scene& scene, std::vector<std::string>* errors) {
    std::vector<UniformUpload> out;
    std::map<int, bool> matrix_animated;
    auto put_mat = [&](const std::string& name, const DMat4& m) {
        UniformUpload u;
        u.name = name;
        u.type = UniformType::Mat4;
        m.to_f32(u.f);
        out.push_back(u);
    };
    // matrices used by objects, then all named matrices (scene.rs:551-592)
    std::vector<int> passed;
    for (const Object& o : scene.objects) {
        if (o.m0 >= 0) passed.push_back(o.m0);
        if (o.kind != Object::DebugMatrix && o.portal && o.m1 >= 0) passed.push_back(o.m1);
    }
    for (size_t k = 0; k < scene.matrices.size(); ++k)
        if (scene.matrices[k].named) passed.push_back((int)k);
    for (int idx : passed) {
        const std::string& name = scene.matrices[idx].name;
        scene.take_frame_input_mark();
        auto m = scene.eval_matrix(idx);
        bool animated = scene.take_frame_input_mark();
        matrix_animated[idx] = animated;
        if (m) {
            put_mat(normal_name(name), *m);
            out.back().animated = animated;
            put_mat(inverse_name(name), m->inverse());
            out.back().animated = animated;
        } else if (errors) {
            errors->push_back("matrix `" + name + "` can't be getted");
        }
    }
    // teleport matrices (scene.rs:594-635)
    for (const Object& o : scene.objects) {
        if (o.kind == Object::DebugMatrix || !o.portal || o.m0 < 0 || o.m1 < 0) continue;
        auto a = scene.eval_matrix(o.m0);
        auto b = scene.eval_matrix(o.m1);
        if (!a || !b) continue;
        const std::string& na = scene.matrices[o.m0].name;
        const std::string& nb = scene.matrices[o.m1].name;
        bool animated = matrix_animated[o.m0] || matrix_animated[o.m1];
        put_mat(teleport_name(na, nb), *b * a->inverse());
        out.back().animated = animated;
        if (na != nb) {
            put_mat(teleport_name(nb, na), *a * b->inverse());
            out.back().animated = animated;
        }
    }
    // user uniforms (scene.rs:637-656)
    for (size_t k = 0; k < scene.uniforms.size(); ++k) {
        const UniformEntry& e = scene.uniforms[k];
        if (e.name.empty()) continue;
        const Uniform* now = scene.resolved_uniform((int)k);
        if (now && now->kind == Uniform::Trefoil) {  // value + enabled * 10000 + color * 1000 (scene.rs:644-650)
            for (int i = 0; i < 18; ++i) {
                UniformUpload u;
                u.name = "ts_" + std::to_string(i) + "_" + e.name + "_u";
                u.type = UniformType::Int1;
                u.i = now->trefoil[i][1] + now->trefoil[i][0] * 10000 + now->trefoil[i][2] * 1000;
                out.push_back(u);
            }
            continue;
        }
        scene.take_frame_input_mark();
        auto v = scene.eval_uniform((int)k);
        bool animated = scene.take_frame_input_mark();
        if (!v) {
            if (errors) errors->push_back("Error getting `" + e.name + "` uniform");
            continue;
        }
        UniformUpload u;
        u.animated = animated;
        u.name = e.name + "_u";
        if (v->kind == UniformValue::Float) {
            u.type = UniformType::Float1;
            u.f[0] = (float)v->f;
        } else {
            u.type = UniformType::Int1;
            u.i = v->kind == UniformValue::Bool ? (v->b ? 1 : 0) : v->i;
        }
        out.push_back(u);
    }
    return out;
}

MatrixPattern matrix_pattern(const float e[16]) {
    MatrixPattern p = 0;
    for (int k = 0; k < 16; ++k) {
        if (e[k] != 0.0f) p |= 1ull << k;  // (column-major: k = 4 * column + row; a NaN element counts as non-zero)
        if (e[k] == 1.0f) p |= 1ull << (16 + k);
        if (e[k] == -1.0f) p |= 1ull << (32 + k);
    }
    return p;
}

bool matrix_breaks_short_chains(const float m[16]) {
    int nan = 0, inf = 0;
    for (int k = 0; k < 16; ++k) {
        nan += std::isnan(m[k]) ? 1 : 0;
        inf += std::isinf(m[k]) ? 1 : 0;
    }
    return inf > 0 || (nan > 0 && nan < 16);
}

bool matrix_is_affine(const float m[16]) { return m[3] == 0.0f && m[7] == 0.0f && m[11] == 0.0f && m[15] == 1.0f; }

bool matrix_keeps_rays_affine(const float m[16]) {
    return matrix_is_affine(m) || std::all_of(m, m + 16, [](float e) { return std::isnan(e); });
}

// ------------------------------------------------------------------------------------------
// the plan of one build: every decision, no text
// ------------------------------------------------------------------------------------------
namespace {

// One GLSL text of the scene on its way into the kernel: tag filter, (optionally) the caller's distance bound, (optionally) uniform-only work
// moved to the prologue kernel (glsl_hoist.h; planned for all snippets at once, because the members it creates belong into the uniform block
// that is emitted before any snippet), GLSL -> C++ (translate_snippet).
struct SceneSnippet {
    enum Kind { Library, MaterialBody, FlatObject, ComplexObject, IntersectionMaterial };
    Kind kind;
    const std::string* code;    // the scene's text as written; its address names the snippet
    bool portal;                // (objects) the generated function has the extra parameter `first`
    std::string filtered;       // the text behind the tag filter
    std::string bounded;        // ... with the caller's distance bound in its `nearer` conditions ("": as written; KernelOptions::bound_snippets)
    std::string hoisted;        // ... with its uniform-only work replaced by reads of block members ("": nothing hoisted)
    std::string hoisted_first;  // the first-trip variant of an intersection material: parameter `r` starts at the camera ("": none; KernelOptions::first_trip)
    const std::string& source() const { return bounded.empty() ? filtered : bounded; }
    const std::string& glsl() const { return hoisted.empty() ? source() : hoisted; }
};

// Every snippet of the scene, in the order the affine scan reports and the hoister numbers its members by: library, Complex materials,
// Flat / Complex objects, intersection materials.
std::vector<SceneSnippet> scene_snippets(const Scene& scene, const CodegenFlags& flags) {
    std::vector<SceneSnippet> out;
    auto add = [&](SceneSnippet::Kind kind, const std::string& code, bool portal) { out.push_back({kind, &code, portal, filter_tagged_lines(code, flags), {}, {}, {}}); };
    for (const NamedCode& lib : scene.library) add(SceneSnippet::Library, lib.code, false);
    for (const Material& m : scene.materials)
        if (m.kind == Material::Complex) add(SceneSnippet::MaterialBody, m.code, false);
    for (const Object& o : scene.objects)
        if (o.kind == Object::Flat || o.kind == Object::Complex) add(o.kind == Object::Flat ? SceneSnippet::FlatObject : SceneSnippet::ComplexObject, o.code, o.portal);
    for (const NamedCode& im : scene.intersection_materials) add(SceneSnippet::IntersectionMaterial, im.code, false);
    return out;
}

struct BuildPlan {
    std::vector<UniformDesc> uniforms;  // the block's layout: samplers first, then Scene::uniforms() order, with offsets
    size_t uniform_block_size = 0;
    std::map<std::string, std::string> baked;  // uniforms compiled in: name -> literal
    std::vector<UniformUpload> baked_values;   // ... the scene's among them, with the values (GeneratedKernel::baked)
    // Int uniforms baked into this build, with their values: a counting loop `for (int k = 0; k < NAME_u; k++)` of a snippet whose bound
    // is one of them (and small) is unrolled.  The same operations in the same order -- identical frames -- but every iteration
    // then has its own constants: the loop counter (`size` of scenes/portal_in_portal.ron:1144 drives an inner loop and a material
    // index) and, with the matrices baked too, whatever the iteration does to loop-carried uniform values.  Measured on the headline
    // (profiles/r03/stub_profile.jsonl `pip_unrolled`, variants5_unroll.jsonl): 0.409 -> 0.350 ms, same frame hash.
    std::map<std::string, int> unroll_bounds;
    bool full_chains = false;  // no matrix product is shortened (GeneratedKernel::full_chains)
    std::vector<std::pair<std::string, MatrixPattern>> masked;
    std::set<std::string> masked_names;  // ... their names: what every text that multiplies by one of them is written by (masked_call, translate_snippet)
    bool affine_rays = false;
    std::string affine_rays_refused_because;
    bool cheap_transforms = false;     // affine rays: a transform is a few additions, and the two dodges of it are dropped (plan_build):
    bool defer_loop_updates = true;    // ... translate_glsl's deferred loop-carried ray transforms
    bool first_trip_snippets = false;  // ... first-trip copies of the intersection-material snippets
    std::vector<DerivedPlane> derived;
    int first_trip_plane_tests = 0;  // > 0: the generated plane tests get their first-trip form (ptl_dvo_<object>_<side> members), this many
    std::vector<SceneSnippet> snippets;
    int bounded_snippet_blocks = 0;
    std::vector<HoistedMember> hoisted_members;  // block members that hold uniform-only work of the snippets ...
    std::string hoisted_prologue;                // ... and the GLSL that fills them

    const SceneSnippet& snippet(const std::string& code) const {
        for (const SceneSnippet& s : snippets)
            if (s.code == &code) return s;
        throw std::logic_error("BuildPlan: a scene text that is no snippet");
    }
    bool any_first_snippet() const {
        return std::any_of(snippets.begin(), snippets.end(), [](const SceneSnippet& s) { return !s.hoisted_first.empty(); });
    }
};

// "this build may shorten matrix products at all" (masks, or literal matrices whose zero terms are dropped) ...
bool may_shorten_products(const KernelOptions& opts) { return opts.mask_zero_elements || opts.specialize_all || opts.specialize_static; }
// ... and "what it shortens stays exact": contract 2, no tolerance mode, every matrix finite
bool short_chains_exact(const KernelOptions& opts, bool full_chains) { return !opts.exact_cr && !opts.fast_math && !full_chains; }

void plan_uniform_layout(const Scene& scene, BuildPlan& plan) {
    std::vector<UniformDesc>& list = plan.uniforms;
    for (auto& tex : scene_texture_list(scene)) list.push_back({tex, UniformType::Sampler, 0});
    for (auto& u : scene_uniform_list(scene)) list.push_back(u);
    size_t off = 0;
    for (auto& u : list) {
        u.offset = off;
        off += uniform_type_size(u.type);
    }
    bool has_sampler = !list.empty() && list[0].type == UniformType::Sampler;  // pointer member -> 8-byte struct alignment
    plan.uniform_block_size = has_sampler ? ((off + 7) & ~(size_t)7) : off;
}

// JIT-time specialisation: current values baked in as literals (same arithmetic, the
// compiler folds branches on mode switches / ray-independent subexpressions)
void plan_baked_values(const std::vector<UniformUpload>& values, const KernelOptions& opts, BuildPlan& plan) {
    if (!(opts.specialize_ints || opts.specialize_all || opts.specialize_static || opts.specialize_static_ints)) return;
    auto hexf = [](float v) -> std::string {
        if (std::isnan(v)) return "__builtin_nanf(\"\")";
        if (std::isinf(v)) return v > 0 ? "__builtin_inff()" : "(-__builtin_inff())";
        char buf[48];
        std::snprintf(buf, sizeof buf, "%af", (double)v);
        return buf;
    };
    for (auto& up : values) {
        if (up.name == "teleport_light_u") continue;  // forced to 1 by the camera-teleport query (src/main.rs:1367)
        if (opts.keep_dynamic.count(up.name)) continue;
        if (opts.specialize_static && up.animated) continue;  // changes every frame: stays a run-time uniform
        const bool switches_only = opts.specialize_static_ints && !(opts.specialize_ints || opts.specialize_all || opts.specialize_static);
        if (switches_only && (up.animated || up.type != UniformType::Int1)) continue;  // the patterns build: only the Bool / Int uniforms that hold still
        bool all = opts.specialize_all || opts.specialize_static;
        if (up.type == UniformType::Int1) {
            plan.baked[up.name] = std::to_string(up.i);
            if (opts.unroll_baked_loops) plan.unroll_bounds[up.name] = up.i;
        } else if (all && up.type == UniformType::Float1) {
            plan.baked[up.name] = hexf(up.f[0]);
        } else if (all && up.type == UniformType::Mat4) {
            std::string m = "mat4(";
            for (int k = 0; k < 16; ++k) m += (k ? ", " : "") + hexf(up.f[k]);
            plan.baked[up.name] = m + ")";
        } else {
            continue;
        }
        plan.baked_values.push_back(up);
    }
}

// Shortened products are exact for finite vectors (device/ptl_glsl.h, "the deviation, stated"): a skipped `0 * x` would have been NaN
// for an infinite or NaN x.  Where such vectors come from is known at generation time -- a matrix with non-finite elements (the
// inverse of a zero scale, 1/0 in a formula) -- so it is decided here, for the whole kernel:
//   * a matrix that is NaN in EVERY element (glam's inverse of a matrix scaled to zero on all axes: how the reference's scenes switch
//     an object off, scenes/portal_in_portal.ron `c0`) turns every vector into all-NaN, and NaN times a retained non-zero element is
//     NaN in the short chain as in the full one: allowed;
//   * any other non-finite matrix (infinities, or NaN beside numbers) produces +-inf components, for which the two chains do differ
//     (inf * 1 against inf * 1 + 0 * inf = NaN): the kernel keeps every full chain (GeneratedKernel::full_chains).
bool plan_full_chains(const std::vector<UniformUpload>& values, const KernelOptions& opts) {
    if (opts.full_chains || !may_shorten_products(opts)) return opts.full_chains;
    for (auto& up : values)
        if (up.type == UniformType::Mat4 && matrix_breaks_short_chains(up.f)) return true;
    return false;
}

// the state the zero patterns depend on: stage / clip, every value that is not animated (the probes move the animated ones themselves)
std::string zero_mask_cache_key(const Scene& scene, const std::vector<UniformUpload>& values, const std::map<std::string, std::string>& baked, const KernelOptions& opts) {
    std::string key;
    auto put = [&key](const void* p, size_t n) { key.append(static_cast<const char*>(p), n); };
    const int stage[3] = {(int)scene.current_stage.kind, scene.current_stage.index, scene.run_animations ? 1 : 0};
    put(stage, sizeof stage);
    for (auto& up : values) {
        key += up.name;
        key += up.animated ? '~' : '=';
        if (!up.animated) {
            put(up.f, sizeof up.f);
            put(&up.i, sizeof up.i);
        }
        key += baked.count(up.name) ? 'b' : (opts.keep_unmasked.count(up.name) ? 'k' : 'r');
    }
    return key;
}

// The patterns in `found` of the matrices that move, taken over the whole clip.  A matrix that reads the formulas' `time` is identity-like
// exactly when a clip starts -- the moment a clip-constant kernel is generated: the union over probes of `time` in [0, 1] (a copy of the scene;
// the pattern of an animation changes at its end points or nowhere, a probe that misses something costs one rebuild, not a pixel).
void probe_animated_patterns(const Scene& scene, const std::vector<UniformUpload>& values, std::vector<std::pair<std::string, MatrixPattern>>& found) {
    auto take = [&](const Scene& probe) {
        for (auto& up : evaluate_scene_uniforms(probe, nullptr))
            if (up.type == UniformType::Mat4 && up.animated)
                for (auto& f : found)
                    if (f.first == up.name) f.second = combine_patterns(f.second, matrix_pattern(up.f));
    };
    Scene probe = scene;
    const bool in_clip = !scene.run_animations && scene.current_stage.kind == StageRef::RealAnimation && scene.current_stage.index >= 0 &&
                         scene.current_stage.index < (int)scene.animations.size() && scene.animations[scene.current_stage.index].duration > 0.0;
    if (in_clip) {
        // inside a clip: the video pipeline's own step (Scene::update) at 33 moments of the clip.  On the reference's corpus (471 clips,
        // patterns taken on a 240-point grid) 7 probes miss something in 16 clips, 16 in 10, 32 in none: elements like cos(pi/2)
        // flicker between 0 and 1e-17, and every miss is a rebuild in the middle of a clip
        const double duration = scene.animations[scene.current_stage.index].duration;
        try {
            for (int k = 0; k <= 32; ++k) {
                probe.update(duration * (k < 32 ? k / 32.0 : 0.999999));
                take(probe);
            }
        } catch (const std::exception&) {  // a clip whose cameras cannot be evaluated fails where it is played, not here: no pattern for what moves
            for (auto& up : values)
                if (up.type == UniformType::Mat4 && up.animated)
                    for (auto& f : found)
                        if (f.first == up.name) f.second = 0xffffu;
        }
    } else {
        for (double t : {0.0, 0.0625, 0.271, 0.5, 0.729, 0.9375, 1.0}) {
            probe.time = t;
            take(probe);
        }
    }
    // The other per-frame input is the camera (Matrix::Camera): one probe gives it a matrix without a single zero, so that
    // nothing that follows the camera is ever masked (a renderer is even created before its camera is known).
    probe = scene;
    probe.camera_matrix = DMat4::from_cols(DVec4(0.36, 0.48, -0.8, 0.013), DVec4(-0.8, 0.6, 0.017, 0.011), DVec4(0.48, 0.64, 0.6, 0.019), DVec4(0.37, -1.21, 2.53, 1.0));
    take(probe);
}

// KernelOptions::mask_zero_elements: the zero / unit pattern of every matrix that stays a run-time value, from the cache while the state it
// was probed in still holds.
std::vector<std::pair<std::string, MatrixPattern>> plan_zero_patterns(const Scene& scene, const std::vector<UniformUpload>& values, const std::map<std::string, std::string>& baked,
                                                                      bool full_chains, const KernelOptions& opts) {
    if (!opts.mask_zero_elements || !short_chains_exact(opts, full_chains)) return {};
    auto run_time = [&](const UniformUpload& up) { return up.type == UniformType::Mat4 && !baked.count(up.name) && !opts.keep_unmasked.count(up.name); };
    const std::string key = opts.mask_cache ? zero_mask_cache_key(scene, values, baked, opts) : std::string();
    // (a hit must still cover what the animated matrices hold NOW: their values are not part of the key, and a build with baked Bool /
    // Int uniforms has nothing but this generation between a moved value and the draw)
    bool hit = opts.mask_cache && !key.empty() && key == opts.mask_cache->key;
    if (hit)
        for (auto& up : values) {
            if (!run_time(up) || !up.animated) continue;
            MatrixPattern mask = 0xffffu;
            for (auto& m : opts.mask_cache->masked)
                if (m.first == up.name) mask = m.second;
            if (!pattern_holds(mask, up.f)) hit = false;
        }
    if (hit) {
        ++opts.mask_cache->hits;
        return opts.mask_cache->masked;
    }
    std::vector<std::pair<std::string, MatrixPattern>> found, masked;
    bool any_animated = false;
    for (auto& up : values) {
        if (!run_time(up)) continue;
        found.emplace_back(up.name, matrix_pattern(up.f));
        any_animated = any_animated || up.animated;
    }
    if (any_animated) probe_animated_patterns(scene, values, found);
    for (auto& f : found)
        if (f.second != 0xffffu) masked.push_back(f);
    if (opts.mask_cache) {
        ++opts.mask_cache->misses;
        opts.mask_cache->key = key;
        opts.mask_cache->masked = masked;
    }
    return masked;
}

// Affine rays (KernelOptions::affine_rays): every matrix of the scene maps w = 1 to 1 and w = 0 to 0 (bottom row 0 0 0 1) -- or is NaN in
// every element (a switched-off object: its products are NaN whatever the w) -- and no scene snippet writes a ray's w.  Only in builds
// that may shorten products at all (the same deviation for non-finite rays, the same guard), i.e. never in the un-specialised build.
// (the tolerance mode gets them too: it is not bit-exact anyway, and without them it was SLOWER than the exact kernel -- 0.217 against 0.191 ms)
bool plan_affine_rays(const std::vector<UniformUpload>& values, const std::vector<SceneSnippet>& snippets, bool full_chains, const KernelOptions& opts, std::string* refused_because) {
    if (!opts.affine_rays || opts.check_affine || opts.exact_cr || full_chains || !may_shorten_products(opts)) return false;
    // (a matrix that stays a run-time value: what holds now is checked again by the renderer before every upload that could change it
    // -- renderer_builds.cpp `zero_patterns_broken` for the builds that keep their kernel across scene states; the others come back here)
    for (auto& up : values)
        if (up.type == UniformType::Mat4 && !matrix_keeps_rays_affine(up.f)) return false;
    if (opts.skip_affine_scan) return true;
    std::vector<std::string> codes;
    for (const SceneSnippet& s : snippets) codes.push_back(s.filtered);
    return snippets_keep_rays_affine(codes, refused_because);
}

// first-trip plane tests (KernelOptions::first_trip_planes): `plane_inv * camera origin` per generated plane test, only where some Flat
// object's matrix is a run-time value
// (not with every scene uniform baked in: with the zero terms of the literal matrices skipped the origin half of a plane test
// is a couple of FMAs, and the second copy of scene_intersect measured no gain there -- profiles/r03/variants7_first_trip_planes.jsonl)
int plan_first_trip_planes(const Scene& scene, const std::map<std::string, std::string>& baked, const KernelOptions& opts) {
    if (!(opts.derived_uniforms && opts.first_trip_planes)) return 0;
    bool wanted = false;
    int tests = 0;
    for (const Object& o : scene.objects) {
        if (o.kind != Object::Flat) continue;
        wanted = wanted || !baked.count(inverse_name(matrix_name(scene, o.m0, o))) || (o.portal && !baked.count(inverse_name(matrix_name(scene, o.m1, o))));
        tests += o.portal ? 2 : 1;
    }
    return wanted ? tests : 0;
}

// derived uniforms: one entry per plane test of a Flat object whose matrix is a run-time uniform
std::vector<DerivedPlane> plan_derived_planes(const Scene& scene, const std::map<std::string, std::string>& baked, const KernelOptions& opts) {
    std::vector<DerivedPlane> derived;
    if (!opts.derived_uniforms) return derived;
    for (size_t pos = 0; pos < scene.objects.size(); ++pos) {
        const Object& o = scene.objects[pos];
        if (o.kind != Object::Flat) continue;
        auto add = [&](int midx, int side, const std::string& normal_expr, const std::string& arg_expr) {
            const std::string& m = matrix_name(scene, midx, o);
            if (baked.count(normal_name(m))) return;  // literal matrix: the compiler folds all of this
            DerivedPlane d;
            d.object = (int)pos;
            d.side = side;
            d.member = "ptl_dv_" + std::to_string(pos) + "_" + std::to_string(side);
            d.normal_expr = normal_expr + normal_name(m) + ")";
            d.arg_expr = arg_expr + normal_name(m) + ")";
            derived.push_back(d);
        };
        if (!o.portal) {
            add(o.m0, 0, "-get_normal(", "get_normal(");
        } else {
            add(o.m0, 0, "-get_normal(", "-get_normal(");
            add(o.m1, 1, "get_normal(", "get_normal(");
        }
    }
    return derived;
}

// out / inout arguments are lowered to references: refuse the scenes for which that is not GLSL's copy in / copy out
void check_snippet_out_arguments(const std::vector<SceneSnippet>& snippets) {
    std::vector<std::string> file_scope, bodies;
    for (const SceneSnippet& s : snippets) (s.kind == SceneSnippet::Library ? file_scope : bodies).push_back(s.filtered);
    check_out_argument_aliasing(file_scope, bodies);
}

// the caller's distance bound inside the intersection-material snippets (KernelOptions::bound_snippets)
void plan_bounded_snippets(BuildPlan& plan, const KernelOptions& opts) {
    if (!opts.bound_snippets) return;
    // process_portal_intersection never resets SceneIntersection::in_subspace (library.glsl:571-589): with subspace portals a skipped
    // candidate could leave that flag behind, so a scene whose GLSL names them keeps its snippets as written
    std::set<std::string> with_out;
    for (const SceneSnippet& s : plan.snippets) {
        if (s.kind == SceneSnippet::Library) functions_with_out_params(*s.code, with_out);
        if (names_identifier(*s.code, {"TELEPORT_SUBSPACE", "in_subspace"})) return;
    }
    for (SceneSnippet& s : plan.snippets) {
        if (s.kind != SceneSnippet::IntersectionMaterial) continue;
        int n = 0;
        std::string bounded = bound_nearer_blocks(s.filtered, with_out, &n);
        if (n > 0) {
            s.bounded = bounded;
            plan.bounded_snippet_blocks += n;
        }
    }
}

// uniform-only work of the scene snippets: members behind the derived planes, filled by the same prologue kernel
void plan_hoisted_work(BuildPlan& plan, const KernelOptions& opts) {
    if (!(opts.derived_uniforms && opts.hoist_uniform_work)) return;
    HoistParams base;
    for (auto& u : plan.uniforms) {
        if (u.type == UniformType::Sampler) continue;
        if (plan.baked.count(u.name)) base.constants[u.name] = cxx_type(u.type);
        else base.uniforms[u.name] = cxx_type(u.type);
    }
    for (const SceneSnippet& s : plan.snippets)
        if (s.kind == SceneSnippet::Library) {
            functions_with_out_params(*s.code, base.functions_with_out_params);
            defined_functions(*s.code, base.scene_functions);
        }
    int next_member = 0;
    auto hoist = [&](const SceneSnippet& s, const HoistParams& hp, std::string& into) {
        HoistResult r = hoist_uniform_work(s.source(), hp, next_member);
        if (r.members.empty()) return;
        into = r.glsl;
        plan.hoisted_members.insert(plan.hoisted_members.end(), r.members.begin(), r.members.end());
        plan.hoisted_prologue += r.prologue;
    };
    for (SceneSnippet& s : plan.snippets) {
        HoistParams hp = base;
        hp.body_only = s.kind != SceneSnippet::Library;
        switch (s.kind) {
            case SceneSnippet::Library: break;
            case SceneSnippet::MaterialBody: hp.body_params = {"hit", "r", "i"}; break;
            case SceneSnippet::FlatObject: hp.body_params = {"pos", "x", "y", "back"}; break;
            case SceneSnippet::ComplexObject: hp.body_params = {"r"}; break;
            case SceneSnippet::IntersectionMaterial: hp.body_params = {"r", "ptl_far"}; break;
        }
        if (s.portal) hp.body_params.push_back("first");
        hoist(s, hp, s.hoisted);
    }
    if (!plan.first_trip_snippets) return;
    for (SceneSnippet& s : plan.snippets) {  // the first-trip variant of an intersection-material snippet: parameter `r` starts at the camera
        if (s.kind != SceneSnippet::IntersectionMaterial) continue;
        HoistParams hp = base;
        hp.body_only = true;
        hp.body_params = {"r", "ptl_far"};
        hp.origin_uniform_rays = {"r"};
        hp.origin_expr = "PTL_DV_OUT.ptl_dv_origin";
        hoist(s, hp, s.hoisted_first);
    }
}

// The decisions of one build, in the order in which they depend on each other.
BuildPlan plan_build(const Scene& scene, const CodegenFlags& flags, const KernelOptions& opts, const std::vector<UniformUpload>& values) {
    BuildPlan plan;
    plan_uniform_layout(scene, plan);
    plan_baked_values(values, opts, plan);
    plan.full_chains = plan_full_chains(values, opts);
    plan.masked = plan_zero_patterns(scene, values, plan.baked, plan.full_chains, opts);
    for (auto& m : plan.masked) plan.masked_names.insert(m.first);
    plan.snippets = scene_snippets(scene, flags);
    plan.affine_rays = plan_affine_rays(values, plan.snippets, plan.full_chains, opts, &plan.affine_rays_refused_because);
    // Deferred loop updates (glsl_translate.h) and the first-trip copies of the intersection-material snippets (ptl_trace.tpl PTL_FIRST_TRIP)
    // both exist to dodge `transform(uniform matrix, ray)` -- 32 FMAs in the un-specialised kernel.  In a kernel with affine rays the matrices
    // are literals or carry their patterns, a transform of the reference's portal matrices is a handful of additions, and the bookkeeping
    // around it (pending counters and their flush loops; a second copy of every snippet and a wave-level choice between the two) costs more
    // than it saves: measured on the headline, same frames, baked 0.2305 -> 0.2046 ms, Int-baked 0.272 -> 0.239, patterns 0.274 -> 0.239
    // (profiles/r05/ab_flags2.jsonl; the un-specialised kernel: 0.70 -> 0.89 without the deferral, so it keeps both).
    plan.cheap_transforms = plan.affine_rays && !opts.keep_transform_dodges;
    plan.defer_loop_updates = flags.defer_loop_updates && !plan.cheap_transforms;
    plan.first_trip_snippets = opts.first_trip && !plan.cheap_transforms;
    // (KernelOptions::baked_options is only filled in for builds that may compile the switches in: any specialisation, patterns-only included)
    for (auto& [name, value] : opts.baked_options)
        for (auto& u : plan.uniforms)
            if (u.name == name && u.type == UniformType::Int1) plan.baked[name] = std::to_string(value);
    plan.first_trip_plane_tests = plan_first_trip_planes(scene, plan.baked, opts);
    plan.derived = plan_derived_planes(scene, plan.baked, opts);
    check_snippet_out_arguments(plan.snippets);
    plan_bounded_snippets(plan, opts);
    plan_hoisted_work(plan, opts);
    return plan;
}

// ------------------------------------------------------------------------------------------
// slot generators (scene.rs:693-1063): one per slot of the kernel template, text only
// ------------------------------------------------------------------------------------------

// GLSL -> C++ as this build wants it.  `file_scope`: a library text, whose function definitions become PTL_FN (force-inlined) like the rest of the kernel.
// Then what the build compiles in (specialize_translated): the masked forms of the products with plan.masked, the unrolled counting loops.
std::string translate_snippet(const BuildPlan& plan, const std::string& glsl, bool file_scope = false, int* unrolled = nullptr) {
    return specialize_translated(translate_glsl(glsl, plan.defer_loop_updates, file_scope), plan.masked_names, plan.unroll_bounds, unrolled);
}
std::string translate_snippet(const BuildPlan& plan, const SceneSnippet& s) { return translate_snippet(plan, s.glsl(), s.kind == SceneSnippet::Library); }

// The statements the generator writes itself: a callee that multiplies by matrix `m` / the product `m * operand`, in the masked form where
// the build knows the matrix's zero / unit pattern (KernelOptions::mask_zero_elements).
std::string masked_call(const BuildPlan& plan, const std::string& callee, const std::string& m) { return plan.masked_names.count(m) ? masked_callee(callee, m) : callee; }
std::string masked_product(const BuildPlan& plan, const std::string& m, const std::string& operand) {
    return plan.masked_names.count(m) ? masked_callee("ptl_mul_m", m) + "(" + m + ", " + operand + ")" : m + " * " + operand;
}

// The entry variants of a build as the names the device files' sections go by (select_sections); the entry over slices brings the slices entry along.
// (No section asks for one of the two refine names today -- their text is a whole file, and fills a slot: emit_refine_entry.)
bool sliced(const KernelOptions& opts) { return opts.slices_entry || opts.refine_slices_entry; }
std::set<std::string> variant_sections(const KernelOptions& opts) {
    std::set<std::string> names;
    if (sliced(opts)) names.insert("slices");
    if (opts.passes) names.insert("passes");
    if (opts.refine_entry) names.insert("refine");
    if (opts.refine_slices_entry) names.insert("refine_slices");
    return names;
}

StringStorage emit_uniforms(const Scene& scene, const BuildPlan& plan, const KernelOptions& opts) {
    StringStorage s;
    // (in the TEXT as well as among the defines: a renderer tells "nothing compiled in changed" by comparing sources, and a kernel with and
    // one without affine rays differ in nothing else)
    if (plan.affine_rays) s.add_string("#define PTL_AFFINE_RAYS 1\n");
    if (opts.check_affine) s.add_string("#define PTL_CHECK_AFFINE 1\n");  // (implies PTL_COUNT_SEGMENTS: the counter counts rays whose w is not 1 / 0)
    // (PTL_AA_TABLE: rows of the table of sub-pixel offsets, one per sample of a draw from `_aa_start` on.  The CLI's defaults are 1 and 4 samples per
    // draw, a clip moves `_aa_start` and keeps the count (cli_video.cpp), the benchmark's workloads take 1 and 4; `--aa-count` has no upper bound, and a
    // draw with more samples evaluates those beyond the table as written.  16 rows = 128 bytes of the block.)
    if (opts.derived_uniforms) s.add_string("#define PTL_DERIVED_BUILTINS 1\n#define PTL_AA_TABLE 16\n");
    // (trace passes: the define in the text for the same reason, and the record the tracer fills per pixel -- include/portal_amd.h has its contract)
    if (opts.passes)
        s.add_string("#define PTL_PASSES 1\nstruct alignas(16) ptl_pass_record {\n    float depth_near;\n    unsigned int trips;\n    unsigned int final_escaped;\n    unsigned int exhausted_outside;\n};\n");
    if (plan.first_trip_plane_tests > 0) s.add_string("#define PTL_FIRST_TRIP_PLANES 1\n#ifndef PTL_FIRST_TRIP\n#define PTL_FIRST_TRIP 1\n#endif\n");
    if (plan.any_first_snippet()) s.add_string("#define PTL_FIRST_TRIP_SNIPPETS 1\n#ifndef PTL_FIRST_TRIP\n#define PTL_FIRST_TRIP 1\n#endif\n");
    s.add_string("struct ptl_uniform_block {\n");
    for (auto& u : plan.uniforms) s.add_string(std::string("    ") + cxx_type(u.type) + " " + u.name + ";\n");
    // written by ptl_derive_kernel (never by the host: uploads stop at uniform_block_size)
    if (opts.derived_uniforms)  // the per-pixel work that depends on the frame's builtins alone (ptl_trace.tpl derive())
        s.add_string("    vec4 ptl_dv_origin;\n    vec4 ptl_dv_origin_left;\n    vec4 ptl_dv_origin_right;\n    vec2 ptl_dv_half_resolution;\n"
                     "    float ptl_dv_tan_half_view;\n    float ptl_dv_pixel_size;\n"
                     "    vec4 ptl_dv_eye;\n    vec4 ptl_dv_eye_left;\n    vec4 ptl_dv_eye_right;\n    vec2 ptl_dv_aa_jitter[PTL_AA_TABLE];\n"
                     "    float ptl_dv_rcp_aa_count;\n    float ptl_dv_rcp_t_range;\n");
    for (auto& d : plan.derived) s.add_string("    vec3 " + d.member + "_nrm;\n    int " + d.member + "_col;\n");
    if (plan.first_trip_plane_tests > 0)
        for (size_t pos = 0; pos < scene.objects.size(); ++pos) {
            const Object& o = scene.objects[pos];
            if (o.kind != Object::Flat) continue;
            s.add_string("    vec4 ptl_dvo_" + std::to_string(pos) + "_0;\n");
            if (o.portal) s.add_string("    vec4 ptl_dvo_" + std::to_string(pos) + "_1;\n");
        }
    for (auto& m : plan.hoisted_members) s.add_string("    " + m.type + " " + m.name + (m.length ? "[" + std::to_string(m.length) + "]" : "") + ";\n");
    s.add_string("};\n");
    s.add_string("#if PTL_DEVICE_BUILD\n__constant__ ptl_uniform_block ptl_u;\n#else\nptl_uniform_block ptl_u;\n#endif\n");
    // where the kernel reads uniforms from: the __constant__ block through the scalar cache
    // (default), or a per-workgroup LDS copy (-DPTL_UNIFORMS_IN_LDS, staged in ptl_entry.h)
    s.add_string("#if PTL_DEVICE_BUILD && defined(PTL_UNIFORMS_IN_LDS)\n__shared__ ptl_uniform_block ptl_lds_u;\n#define PTL_U ptl_lds_u\n"
                 "#elif PTL_DEVICE_BUILD && defined(PTL_UNIFORM_RELOAD)\n"
                 "// every access goes through a pointer the optimiser cannot see through: scalar loads stay where they are\n"
                 "// used instead of being hoisted out of the bounce loop and spilled (SGPR -> VGPR lanes)\n"
                 "PTL_FN const ptl_uniform_block& ptl_ublock() { const ptl_uniform_block* p = &ptl_u; asm volatile(\"\" : \"+s\"(p)); return *p; }\n"
                 "#define PTL_U (ptl_ublock())\n"
                 "#else\n#define PTL_U ptl_u\n#endif\n");
    for (auto& u : plan.uniforms)
        s.add_string("static_assert(__builtin_offsetof(ptl_uniform_block, " + u.name + ") == " + std::to_string(u.offset) + ", \"uniform layout\");\n");
    for (auto& u : plan.uniforms) {
        auto it = plan.baked.find(u.name);
        if (it != plan.baked.end()) s.add_string("#define " + u.name + " (" + it->second + ")\n");
        else s.add_string("#define " + u.name + " (PTL_U." + u.name + ")\n");
    }
    for (auto& [name, mask] : plan.masked) {
        char hex[96];
        const unsigned ones = (unsigned)((mask >> 16) & 0xffffu), negs = (unsigned)((mask >> 32) & 0xffffu);
        if (ones | negs) std::snprintf(hex, sizeof hex, "0x%04xu | PTL_UNIT_BITS(0x%04x, 0x%04x)", (unsigned)(mask & 0xffffu), ones, negs);
        else std::snprintf(hex, sizeof hex, "0x%04xu", (unsigned)(mask & 0xffffu));
        s.add_string("#define PTL_MASK_" + name + " " + hex + "\n");
    }
    return s;
}

// Round 6 -- table-driven Simple materials (KernelOptions::material_table).  The reference prints one `else if (i.material == X_M) return
// material_simple2(hit, r, <nine literals>)` per material (scene.rs:736-760): 30 of the headline's 34, each an inlined copy of the same body
// behind its own compare-and-branch, and a wave that straddles two materials runs two copies.  Here the nine literals of every Simple material
// (and of the three DEBUG_* system materials) sit in a table indexed by the material id -- staged in LDS per workgroup by the kernel entries,
// read back per lane with two ds_read_b128 -- and ONE call of material_simple2 serves all of them.  Same function, same argument values, same
// operation order: no bit moves (a literal `1.0f - 0.5f` folded by the compiler is the value the instruction computes).
struct MaterialTableEntry { float color[3], normal_coef, grid_scale, grid_coef; unsigned flags; };  // flags: 1 grid, 2 grid2, 4 grid3, 8 present

std::string material_table_text(const std::map<int, MaterialTableEntry>& table, int mode) {
    const int entries = table.rbegin()->first + 1;
    auto bits = [](float v) {
        unsigned u;
        std::memcpy(&u, &v, 4);
        char buf[16];
        std::snprintf(buf, sizeof buf, "0x%08xu", u);
        return std::string(buf);
    };
    std::string init, masks;
    for (int id = 0; id < entries; ++id) {
        auto it = table.find(id);
        const MaterialTableEntry e = it == table.end() ? MaterialTableEntry{{0, 0, 0}, 0, 0, 0, 0u} : it->second;
        init += "    " + bits(e.color[0]) + ", " + bits(e.color[1]) + ", " + bits(e.color[2]) + ", " + bits(e.normal_coef) + ", " + bits(e.grid_scale) + ", " +
                bits(e.grid_coef) + ", " + std::to_string(e.flags) + "u, 0u,\n";
    }
    for (int w = 0; w * 64 < entries; ++w) {
        unsigned long long mask = 0;
        for (int b = 0; b < 64; ++b)
            if (table.count(w * 64 + b)) mask |= 1ull << b;
        char buf[48];
        std::snprintf(buf, sizeof buf, "0x%016llxull", mask);
        masks += std::string(w ? ", " : "") + buf;
    }
    return "#define PTL_MATERIAL_TABLE " + std::to_string(mode) + "\n#define PTL_MATERIAL_TABLE_WORDS " + std::to_string(entries * 8) + "\n"
           "// per material id: colour x y z, normal_coef | grid_scale, grid_coef, flags (1 grid, 2 grid2, 4 grid3, 8 = a Simple material), 0 -- binary32 bit patterns\n"
           "#if PTL_DEVICE_BUILD && PTL_MATERIAL_TABLE == 1\n__constant__ const unsigned int ptl_material_table_init[PTL_MATERIAL_TABLE_WORDS] = {\n" + init + "};\n"
           "__shared__ __attribute__((aligned(16))) unsigned int ptl_material_table[PTL_MATERIAL_TABLE_WORDS];  // filled by the kernel entries (ptl_entry.h)\n"
           "#elif PTL_DEVICE_BUILD\n__constant__ const unsigned int ptl_material_table[PTL_MATERIAL_TABLE_WORDS] __attribute__((aligned(32))) = {\n" + init + "};\n"
           "#else\nstatic const unsigned int ptl_material_table[PTL_MATERIAL_TABLE_WORDS] __attribute__((aligned(16))) = {\n" + init + "};\n#endif\n"
           "PTL_FN bool ptl_material_in_table(int id) {\n"
           "    const unsigned long long masks[] = {" + masks + "};\n"
           "    return (unsigned)id < " + std::to_string(entries) + "u && ((masks[(unsigned)id >> 6] >> ((unsigned)id & 63u)) & 1ull) != 0;\n}\n";
}

// materials (scene.rs:720-845): the slots `material_processing` and `materials_defines`, which share the numbering of the materials
std::pair<StringStorage, StringStorage> emit_materials(const Scene& scene, const BuildPlan& plan, const KernelOptions& opts) {
    StringStorage processing, defines;
    int counter = 0;
    std::map<int, MaterialTableEntry> table;
    if (opts.material_table != 0) {
        const float hi = 0.9f, lo = 0.2f;  // src/library.glsl:387-398 via ptl_trace.tpl: color(0.9, 0.2, 0.2) = the squares, one binary32 multiplication each
        const float hh = hi * hi, ll = lo * lo;
        table[3] = MaterialTableEntry{{hh, ll, ll}, 0.5f, 1.0f, 0.0f, 8u};  // DEBUG_RED / GREEN / BLUE
        table[4] = MaterialTableEntry{{ll, hh, ll}, 0.5f, 1.0f, 0.0f, 8u};
        table[5] = MaterialTableEntry{{ll, ll, hh}, 0.5f, 1.0f, 0.0f, 8u};
    }
    for (const Material& m : scene.materials) {
        std::string name_m = m.name + "_M";
        defines.add_string("#define " + name_m + " (USER_MATERIAL_OFFSET + " + std::to_string(counter++) + ")\n");
        if (opts.material_table != 0 && m.kind == Material::Simple) {
            table[10 + counter - 1] = MaterialTableEntry{{(float)m.color[0], (float)m.color[1], (float)m.color[2]}, (float)m.normal_coef, (float)m.grid_scale, (float)m.grid_coef,
                                                         8u | (m.grid ? 1u : 0u) | (m.grid2 ? 2u : 0u) | (m.grid3 ? 4u : 0u)};
            continue;
        }
        processing.add_string("} else if (i.material == " + name_m + ") {\n");
        switch (m.kind) {
            case Material::Simple:
                processing.add_string("return material_simple2(hit, r, vec3(" + f32_literal(m.color[0]) + ", " + f32_literal(m.color[1]) + ", " +
                                      f32_literal(m.color[2]) + "), " + f32_literal(m.normal_coef) + ", " + bool_lit(m.grid) + ", " +
                                      f32_literal(m.grid_scale) + ", " + f32_literal(m.grid_coef) + ", " + bool_lit(m.grid2) + ", " + bool_lit(m.grid3) + ");\n");
                break;
            case Material::Reflect:
                processing.add_string("return material_reflect(hit, r, vec3(" + f32_literal(m.color[0]) + ", " + f32_literal(m.color[1]) + ", " +
                                      f32_literal(m.color[2]) + "));\n");
                break;
            case Material::Refract:
                processing.add_string("return material_refract(hit, r, vec3(" + f32_literal(m.color[0]) + ", " + f32_literal(m.color[1]) + ", " +
                                      f32_literal(m.color[2]) + "), " + f32_literal(m.refractive_index) + ");\n");
                break;
            case Material::Complex:
                processing.add_identifier_string({"material", m.name}, translate_snippet(plan, plan.snippet(m.code)));
                processing.add_string("\n");
                break;
        }
    }
    for (size_t pos = 0; pos < scene.objects.size(); ++pos) {
        const Object& o = scene.objects[pos];
        if (o.kind == Object::DebugMatrix || !o.portal) continue;
        if (o.m0 < 0 || o.m1 < 0) continue;
        const std::string& a = matrix_name(scene, o.m0, o);
        const std::string& b = matrix_name(scene, o.m1, o);
        std::string m1 = "teleport_" + std::to_string(pos) + "_1_M", m2 = "teleport_" + std::to_string(pos) + "_2_M";
        defines.add_string("#define " + m1 + " (USER_MATERIAL_OFFSET + " + std::to_string(counter++) + ")\n");
        defines.add_string("#define " + m2 + " (USER_MATERIAL_OFFSET + " + std::to_string(counter++) + ")\n");
        // material_teleport(hit, r, M) (library.glsl:366-379) spelled as its body: behind the function parameter the product with M is out of
        // reach of the zero / unit patterns (a masked form names the uniform: masked_call) -- the same two calls, same values
        auto teleport = [&](const std::string& m) { return "return material_teleport_transformed(" + masked_call(plan, "transform", m) + "(" + m + ", r), hit.n);"; };
        processing.add_string("} else if (i.material == " + m1 + ") {\n");
        processing.add_string(teleport(teleport_name(a, b)));
        processing.add_string("} else if (i.material == " + m2 + ") {\n");
        processing.add_string(teleport(teleport_name(b, a)));
    }
    if (opts.material_table != 0) defines.add_string(material_table_text(table, opts.material_table));
    // The prelude needs the uniform accessors, so the library header goes after the uniform
    // block: splice it at the head of the `materials_defines` slot (order in the reference:
    // predefined library -> uniforms -> textures -> material defines -> library -> ...).
    // (With the slices entry the prelude is in the tracer struct instead: emit_prelude_in_tracer.)
    StringStorage spliced;
    spliced.add_string("}  // namespace glsl\n");
    if (!sliced(opts)) spliced.add_string(plain_library_source());
    spliced.add_string("\nnamespace glsl {\n");
    spliced.add_string_storage(std::move(defines));
    return {std::move(processing), std::move(spliced)};
}

// is_inside_N / intersect_N (scene.rs:847-883)
StringStorage emit_intersection_functions(const Scene& scene, const BuildPlan& plan, const KernelOptions&) {
    StringStorage s;
    for (size_t pos = 0; pos < scene.objects.size(); ++pos) {
        const Object& o = scene.objects[pos];
        std::string p = std::to_string(pos);
        if (o.kind == Object::Flat) {
            if (o.portal) s.add_string("PTL_FN int is_inside_" + p + "(vec4 pos, float x, float y, bool back, bool first) {\n");
            else s.add_string("PTL_FN int is_inside_" + p + "(vec4 pos, float x, float y, bool back) {\n");
        } else if (o.kind == Object::Complex) {
            if (o.portal) s.add_string("PTL_FN SceneIntersection intersect_" + p + "(Ray r, bool first) {\n");
            else s.add_string("PTL_FN SceneIntersection intersect_" + p + "(Ray r) {\n");
        } else {
            continue;
        }
        s.add_identifier_string({"object", o.name}, translate_snippet(plan, plan.snippet(o.code)));
        s.add_string("\n}\n");
    }
    return s;
}

// One generated plane test of Flat object `p`: side 0 is the object's (first) matrix `m`, side 1 a portal's second; `material` names the
// teleport material of a portal's side ("": a plain plane).  With a derived entry `d` the unit normal and both is_collinear verdicts come
// from the prologue kernel (emit_derive evaluates exactly the expressions of the plain form).  The first form takes the transformed origin
// of this test from the prologue too, through the `_o` variants of the cull and the plane test.
void emit_plane_test(StringStorage& s, const BuildPlan& plan, const std::string& p, const std::string& m, int side, const std::string& material, const DerivedPlane* d, bool first_form) {
    const bool portal = !material.empty();
    const std::string inv = inverse_name(m), o = first_form ? "_o" : "";
    const std::string origin = first_form ? ", PTL_U.ptl_dvo_" + p + "_" + std::to_string(side) : "";
    s.add_string("if (!" + masked_call(plan, "ptl_plane_cull" + o, inv) + "(r, " + inv + origin + ", PTL_BEST_T(i))) {\n");
    std::string back;  // is_inside's `back`: the plane is seen from behind
    if (d) {
        s.add_string("hit = " + masked_call(plan, "plane_intersect_derived" + o, inv) + "(r, " + inv + ", PTL_U." + d->member + "_nrm, flipped" + origin + ");\n");
        back = "((PTL_U." + d->member + "_col >> (flipped ? 1 : 0)) & 1) != 0";
    } else {
        s.add_string(std::string("normal = ") + (side == 0 ? "-" : "") + "get_normal(" + normal_name(m) + ");\n");
        s.add_string("hit = plane_intersect" + o + "(r, " + inv + ", " + (portal ? "normal" : "get_normal(" + normal_name(m) + ")") + origin + ");\n");
        back = "is_collinear(hit.n, normal)";
    }
    s.add_string(std::string("if (nearer(i, hit)) { i = ") + (portal ? "process_portal_intersection" : "process_plane_intersection") + "(i, hit, is_inside_" + p +
                 "(r.o + r.d * hit.t, hit.u, hit.v, " + back + (portal ? std::string(", ") + bool_lit(side == 0) : "") + ")" + (portal ? ", " + material : "") + "); }\n}\n\n");
}

// Per-object intersection statements (scene.rs:885-1009).  Emitted once in the general form and, with KernelOptions::first_trip_planes, once
// more for the trip on which every ray of the wave still starts at the camera: there `plane_inv * r.o` of a Flat object is the prologue's
// `ptl_dvo_<object>_<side>` (emit_derive evaluates the very product on the very origin), and the plane test / the cull take it instead of
// transforming the origin per lane.
StringStorage emit_intersections(const Scene& scene, const BuildPlan& plan, const KernelOptions&, bool first_form) {
    StringStorage s;
    for (size_t pos = 0; pos < scene.objects.size(); ++pos) {
        const Object& o = scene.objects[pos];
        std::string p = std::to_string(pos);
        auto transformed = [&](const std::string& inv) {
            s.add_string("transformed_ray = " + masked_call(plan, "transform", inv) + "(" + inv + ", r);\nlen = length(transformed_ray.d);\ntransformed_ray = normalize_ray(transformed_ray);");
        };
        if (o.kind != Object::DebugMatrix) {
            if (o.in_subspace == Subspace::Normal) s.add_string("if (r.in_subspace == false) {");
            else if (o.in_subspace == Subspace::Subspace) s.add_string("if (r.in_subspace == true) {");
        }
        if (o.kind == Object::DebugMatrix) {
            const std::string& m = matrix_name(scene, o.m0, o);
            transformed(inverse_name(m));
            s.add_string("ihit = debug_intersect(transformed_ray);\nihit.hit.t = ptl_div(ihit.hit.t, len);\n");
            // quirk kept from the reference: the normal uses adjugate of the *inverse* matrix here
            s.add_string("if (nearer(i, ihit)) { i = ihit; i.hit.n = normalize(adjugate(" + inverse_name(m) + ") * i.hit.n); }\n\n");
        } else if (o.kind == Object::Flat) {
            auto test = [&](int side, const std::string& material) {
                const DerivedPlane* derived = nullptr;
                for (auto& d : plan.derived)
                    if (d.object == (int)pos && d.side == side && !derived) derived = &d;
                emit_plane_test(s, plan, p, matrix_name(scene, side == 0 ? o.m0 : o.m1, o), side, material, derived, first_form);
            };
            if (!o.portal) {
                test(0, "");
            } else {
                test(0, "teleport_" + p + "_1_M");
                test(1, "teleport_" + p + "_2_M");
            }
        } else if (!o.portal) {  // Complex
            const std::string& m = matrix_name(scene, o.m0, o);
            transformed(inverse_name(m));
            s.add_string("ihit = intersect_" + p + "(transformed_ray);\nihit.hit.t = ptl_div(ihit.hit.t, len);\n");
            s.add_string("if (nearer(i, ihit)) { i = ihit; i.hit.n = normalize(adjugate(" + normal_name(m) + ") * i.hit.n); }\n\n");
        } else {
            auto side = [&](const std::string& m, bool first, const std::string& material) {
                transformed(inverse_name(m));
                s.add_string("ihit = intersect_" + p + "(transformed_ray, " + bool_lit(first) + ");\nihit.hit.t = ptl_div(ihit.hit.t, len);\n");
                s.add_string("if (nearer(i, ihit) && ihit.material != NOT_INSIDE) { if (ihit.material == TELEPORT) { ihit.material = " + material +
                             "; } if (ihit.material == TELEPORT_SUBSPACE) { ihit.material = " + material +
                             "; ihit.in_subspace = true; } i = ihit; i.hit.n = normalize(adjugate(" + normal_name(m) + ") * i.hit.n); }\n\n");
            };
            side(matrix_name(scene, o.m0, o), true, "teleport_" + p + "_1_M");
            side(matrix_name(scene, o.m1, o), false, "teleport_" + p + "_2_M");
        }
        if (o.kind != Object::DebugMatrix && o.in_subspace != Subspace::Both) s.add_string("}");
        s.add_string("\n");
    }
    return s;
}

// prologue: the ray-independent part of every derived plane test, once per uniform upload
StringStorage emit_derive(const Scene& scene, const BuildPlan& plan, const KernelOptions&) {
    StringStorage s;
    if (plan.first_trip_plane_tests > 0) {
        s.add_string("    // first-trip plane tests: plane_inv * (origin of every primary ray), the product transform() would evaluate per lane\n");
        for (size_t pos = 0; pos < scene.objects.size(); ++pos) {
            const Object& o = scene.objects[pos];
            if (o.kind != Object::Flat) continue;
            s.add_string("    out->ptl_dvo_" + std::to_string(pos) + "_0 = " + masked_product(plan, inverse_name(matrix_name(scene, o.m0, o)), "out->ptl_dv_origin") + ";\n");
            if (o.portal) s.add_string("    out->ptl_dvo_" + std::to_string(pos) + "_1 = " + masked_product(plan, inverse_name(matrix_name(scene, o.m1, o)), "out->ptl_dv_origin") + ";\n");
        }
    }
    for (auto& d : plan.derived) {
        s.add_string("    {\n        vec3 normal = " + d.normal_expr + ";\n        vec3 unit = normalize(" + d.arg_expr + ");\n");
        s.add_string("        out->" + d.member + "_nrm = unit;\n");
        s.add_string("        out->" + d.member + "_col = (is_collinear(unit, normal) ? 1 : 0) | (is_collinear(unit * -1.0f, normal) ? 2 : 0);\n    }\n");
    }
    if (!plan.hoisted_prologue.empty()) {
        s.add_string("    // uniform-only work of the scene snippets (host/glsl_hoist.h)\n");
        s.add_string(specialize_translated(translate_glsl(plan.hoisted_prologue, false), plan.masked_names, {}));  // (its loops stay rolled)
    }
    return s;
}

// intersection materials (scene.rs:1011-1035): the functions, with the first-trip copies of those that have one ...
StringStorage emit_intersection_material_functions(const Scene& scene, const BuildPlan& plan, const KernelOptions&) {
    StringStorage fns;
    for (size_t pos = 0; pos < scene.intersection_materials.size(); ++pos) {
        const NamedCode& im = scene.intersection_materials[pos];
        const SceneSnippet& snippet = plan.snippet(im.code);
        fns.add_string("PTL_FN SceneIntersectionWithMaterial intersect_material_" + std::to_string(pos) + "(Ray r, float ptl_far) {\n(void)ptl_far; ");
        fns.add_identifier_string({"intersection_material", im.name}, translate_snippet(plan, snippet));
        fns.add_string("\n}\n");
        if (snippet.hoisted_first.empty()) continue;
        fns.add_string("PTL_FN SceneIntersectionWithMaterial intersect_material_" + std::to_string(pos) + "_first(Ray r, float ptl_far) {\n(void)ptl_far; ");
        fns.add_string(translate_snippet(plan, snippet.hoisted_first));
        fns.add_string("\n}\n");
    }
    return fns;
}
// ... and their calls; in the first form only when some snippet has a first-trip copy
// (a snippet without ray chains has none: its general form serves the first trip too)
StringStorage emit_intersection_material_processing(const Scene& scene, const BuildPlan& plan, const KernelOptions&, bool first_form) {
    StringStorage calls;
    if (first_form && !plan.any_first_snippet()) return calls;
    for (size_t pos = 0; pos < scene.intersection_materials.size(); ++pos) {
        const bool own = first_form && !plan.snippet(scene.intersection_materials[pos].code).hoisted_first.empty();
        const std::string call = "intersect_material_" + std::to_string(pos) + (own ? "_first" : "") + "(r, ptl_far)";
        if (pos == 0) {
            // The first snippet meets `result` = none, for which nearer() is `hit.hit && hit.t > 0`: its record is adopted as it stands, and only the
            // flag takes the verdict -- one select instead of one per field of the record (15 on every trip of every lane).  A record whose
            // flag is false is a record nobody reads.  The readers of the returned record (`i2`) in ptl_trace.tpl, and what guards them:
            //   trace_segment   ptl_bound (-DPTL_SNIPPETS_FIRST)           `.scene.hit.t` behind `.scene.hit.hit &&`
            //                   nearer(i.hit, i2.scene.hit)                 `.t` behind `current.hit &&` (ptl_library.h)
            //                   `.scene.hit.t`, `.scene.material`, `.material`, material_process(r, i2.scene): inside that nearer() branch
            //                   the escape test                             `.scene.hit.hit` alone
            //   teleport_external_ray: the same nearer() and the same uses inside its branch
            // (the passes sections of the template read `out` and the trip count, never `i2`), and the snippets after this one:
            // nearer(result.scene.hit, ..) reads `result.t` behind `!result.hit ||`, and `result = hit` replaces every field.
            calls.add_string("#if defined(PTL_SPELLED_ADOPTION)\n");
            calls.add_string("hit = " + call + ";\n");
            calls.add_string("if (nearer(result.scene.hit, hit.scene.hit)) { result = hit; }\n");
            calls.add_string("#else\n");
            calls.add_string("result = " + call + ";\n");
            calls.add_string("result.scene.hit.hit = result.scene.hit.hit && (result.scene.hit.t > 0.0f);\n");
            calls.add_string("#endif\n\n");
            continue;
        }
        calls.add_string("hit = " + call + ";\n");
        calls.add_string("if (nearer(result.scene.hit, hit.scene.hit)) { result = hit; }\n\n");
    }
    return calls;
}

// library (scene.rs:1037-1044)
StringStorage emit_library(const Scene& scene, const BuildPlan& plan, const KernelOptions&) {
    StringStorage s;
    // scene functions are plain GLSL functions: the translation puts PTL_FN in front of every definition
    for (const NamedCode& lib : scene.library) s.add_identifier_string({"library", lib.name}, translate_snippet(plan, plan.snippet(lib.code)));
    return s;
}

StringStorage emit_predefined_library(const Scene&, const BuildPlan&, const KernelOptions&) {
    StringStorage s;
    s.add_string(device_source_glsl());
    s.add_string("\n");
    return s;
}

// The slices entry: three functions of the prelude (device/ptl_library.h) read renderer uniforms (`_grid_disable`, `_angle_color_disable`,
// `_offset_after_material`) -- as free functions through the module's global block, which a slice does not use.  So the prelude goes INTO
// the tracer struct, in front of the scene snippets (the template's `prelude_in_tracer` slot): member functions read the block the tracer
// points at, like everything else.  The same text without its namespace wrapper (its `slices` sections), as many lines as emit_materials leaves out.
StringStorage emit_prelude_in_tracer(const Scene&, const BuildPlan&, const KernelOptions&) {
    StringStorage s;
    s.add_string(select_sections(device_source_library(), {"slices"}));
    return s;
}

// The list-driven render entry of the adaptive anti-aliasing, for the slot in front of the host half of device/ptl_entry.h: device/ptl_refine_common.h
// followed by the entry's own header, as ONE text (embed_sources.py joins them), or nothing.
StringStorage emit_refine_entry(const KernelOptions& opts) {
    StringStorage s;
    if (opts.refine_entry) s.add_string(device_source_refine_entry());
    if (opts.refine_slices_entry) s.add_string(device_source_refine_slices_entry());
    return s;
}

StringStorage emit_skybox_processing(const Scene& scene, const BuildPlan&, const KernelOptions&) {
    StringStorage s;
    if (scene.skybox) {
        s.add_string("vec4 rd2 = ptl_mul_runtime(_camera_mul_inv, r.d);");
        s.add_string("float u = atan(rd2.z, rd2.x);");
        s.add_string("float v = atan(sqrt(rd2.x * rd2.x + rd2.z * rd2.z), rd2.y);");
        s.add_string("vec3 not_found_color = sqrvec(texture(" + *scene.skybox + "_tex, vec2(ptl_div(ptl_div(u, PI) + 1.0f, 2.0f), ptl_div(v, PI))).sw<0,1,2>());");
    } else {
        s.add_string("vec3 not_found_color = color(0.6f, 0.6f, 0.6f);");
    }
    return s;
}

// A loop in an intersection-material snippet (portal_in_portal's ten nested copies) puts the deepest call chain of the kernel inside a
// loop nest; unrolled -- its bound a baked Int (translate_snippet) -- it multiplies the body that LLVM's bottom-up inliner pipeline
// re-simplifies at every call level: the kernels whose hiprtc time that pipeline dominates (kernel.cpp compile_options;
// tools/jit_inliner_survey.py).  The JIT switches to the module inliner for them.  Only for them: it needs ~10 more VGPRs, which the
// baked builds have (115 -> 125 of 128) and the others do not (patterns build with the slices entry: 120 -> 139, a wave per SIMD lost).
bool has_unrolled_snippet_loop(const BuildPlan& plan) {
    for (const SceneSnippet& s : plan.snippets) {
        if (s.kind != SceneSnippet::IntersectionMaterial) continue;
        int unrolled = 0;
        if (names_identifier(s.filtered, {"for", "while"})) translate_snippet(plan, s.glsl(), false, &unrolled);
        if (unrolled > 0) return true;
    }
    return false;
}

// what the plan says about the kernel, for the renderer ...
GeneratedKernel describe_kernel(const BuildPlan& plan, const KernelOptions& opts) {
    GeneratedKernel gk;
    gk.uniforms = plan.uniforms;
    gk.uniform_block_size = plan.uniform_block_size;
    gk.baked = plan.baked_values;
    gk.first_trip_plane_tests = plan.first_trip_plane_tests;
    gk.first_trip_variants = plan.any_first_snippet();
    gk.looped_snippets = has_unrolled_snippet_loop(plan);
    gk.hoisted_members = (int)plan.hoisted_members.size();
    gk.derived = plan.derived;
    gk.masked = plan.masked;
    gk.bounded_snippet_blocks = plan.bounded_snippet_blocks;
    gk.full_chains = plan.full_chains;
    gk.affine_rays_refused_because = plan.affine_rays_refused_because;
    gk.affine_rays = plan.affine_rays;
    // matrices baked into the source: a matrix product skips the terms whose matrix element is zero (device/ptl_glsl.h `ptl_mterm`)
    const bool drop_zero_terms = (opts.specialize_all || opts.specialize_static) && short_chains_exact(opts, plan.full_chains);
    gk.shortened = drop_zero_terms || !plan.masked.empty();
    // ... and for the compiler
    if (opts.count_segments || opts.check_affine) gk.defines.push_back("PTL_COUNT_SEGMENTS");
    if (opts.check_affine) gk.defines.push_back("PTL_CHECK_AFFINE");
    if (opts.anaglyph) gk.defines.push_back("PTL_ANAGLYPH");
    if (opts.fast_math) gk.defines.push_back("PTL_FAST_MATH");
    if (opts.exact_cr) gk.defines.push_back("PTL_CONTRACT_V1");
    if (opts.quick_jit) gk.defines.push_back("PTL_QUICK_JIT");
    if (drop_zero_terms) gk.defines.push_back("PTL_DROP_ZERO_TERMS");
    if (gk.affine_rays) gk.defines.push_back("PTL_AFFINE_RAYS");
    if (gk.first_trip_variants) gk.defines.push_back("PTL_FIRST_TRIP");
    if (gk.looped_snippets) gk.defines.push_back("PTL_JIT_MODULE_INLINER");
    if (gk.bounded_snippet_blocks > 0) gk.defines.push_back("PTL_BOUNDED_SNIPPETS");
    return gk;
}

}  // namespace

const std::string& plain_library_source() {
    static const std::string text = select_sections(device_source_library(), {});
    return text;
}
const std::string& plain_entry_source() {
    static const std::string text = apply_template(select_sections(device_source_entry(), {}), {{"refine_entry", StringStorage()}}).storage;
    return text;
}

GeneratedKernel generate_kernel_source(const Scene& scene, const CodegenFlags& flags, const KernelOptions& opts) {
    if (opts.refine_slices_entry && opts.refine_entry)
        throw SceneError("PTL_FLAG_REFINE and PTL_FLAG_REFINE_SLICES cannot be combined: a module has the refine entry over its own uniform block or the one over slices");
    if (opts.slices_entry && opts.refine_entry) throw SceneError("PTL_FLAG_REFINE and PTL_FLAG_SLICES cannot be combined: the refine entry reads the module's own uniform block (PTL_FLAG_REFINE_SLICES has the entry over slices)");
    if (opts.passes && (opts.anaglyph || opts.refine_entry || opts.refine_slices_entry || opts.check_affine))
        throw SceneError(std::string("PTL_FLAG_PASSES cannot be combined with ") + (opts.anaglyph ? "PTL_FLAG_ANAGLYPH: an anaglyph sample traces two paths, a pass record books one per sample"
                                                                                    : opts.check_affine ? "PTL_FLAG_CHECK_AFFINE: that build counts ray halves where the record counts trips"
                                                                                    : opts.refine_entry ? "PTL_FLAG_REFINE: the list-driven entry stores no records"
                                                                                                        : "PTL_FLAG_REFINE_SLICES: the list-driven entry stores no records"));
    const std::vector<UniformUpload> values = evaluate_scene_uniforms(scene, nullptr);
    const BuildPlan plan = plan_build(scene, flags, opts, values);

    std::map<std::string, StringStorage> slots;
    slots["uniforms"] = emit_uniforms(scene, plan, opts);
    std::tie(slots["material_processing"], slots["materials_defines"]) = emit_materials(scene, plan, opts);
    slots["intersection_functions"] = emit_intersection_functions(scene, plan, opts);
    slots["intersections"] = emit_intersections(scene, plan, opts, false);
    slots["intersections_first"] = plan.first_trip_plane_tests > 0 ? emit_intersections(scene, plan, opts, true) : StringStorage();
    slots["derive"] = emit_derive(scene, plan, opts);
    slots["intersection_material_functions"] = emit_intersection_material_functions(scene, plan, opts);
    slots["intersection_material_processing"] = emit_intersection_material_processing(scene, plan, opts, false);
    slots["intersection_material_processing_first"] = emit_intersection_material_processing(scene, plan, opts, true);
    slots["library"] = emit_library(scene, plan, opts);
    slots["predefined_library"] = emit_predefined_library(scene, plan, opts);
    slots["skybox_processing"] = emit_skybox_processing(scene, plan, opts);
    if (sliced(opts)) slots["prelude_in_tracer"] = emit_prelude_in_tracer(scene, plan, opts);
    slots["refine_entry"] = emit_refine_entry(opts);

    // the trace template and the entries behind it as one text: the sections of this build's variants, then the slots
    const std::string tmpl = select_sections(std::string(device_source_trace_template()) + "\n" + device_source_entry(), variant_sections(opts));
    StringStorage body = apply_template(tmpl, std::move(slots));
    GeneratedKernel gk = describe_kernel(plan, opts);
    gk.source = std::move(body.storage);
    gk.line_numbers = std::move(body.line_numbers);
    return gk;
}

}  // namespace ptl
