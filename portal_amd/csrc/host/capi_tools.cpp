// capi_tools.cpp -- entry points that are no part of a renderer: hooks for the tests and the tools into the template engine, the GLSL passes,
// the RON writer, the formula evaluator, the binary64 matrix primitives and the embedded device sources.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <map>
#include <set>

#include "formula.h"
#include "glsl_hoist.h"
#include "glsl_translate.h"
#include "renderer.h"

using namespace ptl;

// ---- the binary64 primitives behind the scene's constants, one by one (test hooks: tests/test_matrix_exact.py checks each against exact
// arithmetic).  Matrices are 16 doubles, column-major like glam's to_cols_array.
extern "C" int ptl_dmath(const char* op, const double* a, const double* b, const double* c, double* out) {
    if (!op || !a || !out) return PTL_ERR_INVALID;
    auto load = [](const double* v) {
        return DMat4::from_cols({v[0], v[1], v[2], v[3]}, {v[4], v[5], v[6], v[7]}, {v[8], v[9], v[10], v[11]}, {v[12], v[13], v[14], v[15]});
    };
    auto store = [&](const DMat4& m) {
        m.to_cols_array(out);
        return (int)PTL_OK;
    };
    const std::string what = op;
    if (what == "inverse") return store(load(a).inverse());  // glam DMat4::inverse (src/gui/scene.rs:587-588, matrix.rs:537-547)
    if (what == "mul" && b) return store(load(a) * load(b));
    if (what == "teleport" && b) return store(load(b) * load(a).inverse());  // a_to_b = B * A^-1 (src/gui/scene.rs:624-632)
    if (what == "srt" && b && c)  // Simple / Parametrized: T * (Rx * Ry * Rz) * S (src/gui/matrix.rs:555-569); a = scale xyz, b = rotate xyz, c = offset xyz
        return store(DMat4::from_scale_rotation_translation(DVec3(a[0], a[1], a[2]), DQuat::rotation_x(b[0]) * DQuat::rotation_y(b[1]) * DQuat::rotation_z(b[2]), DVec3(c[0], c[1], c[2])));
    if (what == "lerp" && b && c) {  // Matrix::Lerp (src/gui/matrix.rs:614-627): a = first, b = second, c[0] = t -- the very statements scene.cpp evaluates
        DVec3 fs, ft, ss, st;
        DQuat fr, sr;
        load(a).to_scale_rotation_translation(&fs, &fr, &ft);
        load(b).to_scale_rotation_translation(&ss, &sr, &st);
        return store(DMat4::from_scale_rotation_translation(fs.lerp(ss, c[0]), fr.lerp(sr, c[0]), ft.lerp(st, c[0])));
    }
    if (what == "camera" && b) {  // RotateAroundCam::get_matrix (src/main.rs:278-304): a = look_at xyz, alpha, beta, r; b = the teleport matrix
        Camera cam;
        cam.look_at = DVec3(a[0], a[1], a[2]);
        cam.alpha = a[3];
        cam.beta = a[4];
        cam.r = a[5];
        cam.teleport_matrix = load(b);
        return store(cam.matrix());
    }
    set_last_error(std::string("ptl_dmath: unknown operation `") + what + "`");
    return PTL_ERR_INVALID;
}

extern "C" int ptl_snippets_keep_rays_affine(const char* glsl, char* why, size_t why_cap) {
    if (!glsl) return -1;
    try {
        std::string reason;
        const bool ok = snippets_keep_rays_affine({glsl}, &reason);
        if (why && why_cap) {
            std::snprintf(why, why_cap, "%s", ok ? "" : reason.c_str());
        }
        return ok ? 1 : 0;
    } catch (const std::exception& e) {
        set_last_error(std::string("ptl_snippets_keep_rays_affine: ") + e.what());
        return -1;
    }
}

// ---- template engine hooks ----------------------------------------------------------------------
struct ptl_strstore {
    StringStorage s;
};
extern "C" ptl_strstore* ptl_strstore_new(void) { return new ptl_strstore(); }
extern "C" void ptl_strstore_free(ptl_strstore* s) { delete s; }
extern "C" void ptl_strstore_add_string(ptl_strstore* s, const char* text) {
    if (s && text) s->s.add_string(text);
}
extern "C" void ptl_strstore_add_identifier_string(ptl_strstore* s, const char* kind, const char* name, const char* text) {
    if (s && kind && name && text) s->s.add_identifier_string({kind, name}, text);
}
extern "C" ptl_strstore* ptl_apply_template(const char* tmpl, const char* const* slot_names, ptl_strstore* const* storages, int n) {
    std::map<std::string, StringStorage> m;
    for (int k = 0; k < n; ++k) {
        m[slot_names[k]] = std::move(storages[k]->s);
        delete storages[k];
    }
    try {
        auto* out = new ptl_strstore();
        out->s = apply_template(tmpl, std::move(m));
        return out;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return nullptr;
    }
}
// select_sections on a text of the caller's: malloc'd (ptl_free), or NULL + ptl_last_error() where the engine throws
extern "C" char* ptl_select_sections(const char* text, const char* const* names, int n) {
    if (!text || (n > 0 && !names)) return nullptr;
    try {
        const std::string out = select_sections(text, std::set<std::string>(names, names + std::max(n, 0)));
        char* p = (char*)std::malloc(out.size() + 1);
        std::memcpy(p, out.c_str(), out.size() + 1);
        return p;
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return nullptr;
    }
}
extern "C" const char* ptl_strstore_text(const ptl_strstore* s) { return s ? s->s.storage.c_str() : ""; }
extern "C" int ptl_strstore_current_line(const ptl_strstore* s) { return s ? s->s.current_line_no : 0; }
extern "C" int ptl_strstore_range(const ptl_strstore* s, const char* kind, const char* name, int* start, int* end) {
    if (!s) return PTL_ERR_INVALID;
    auto it = s->s.line_numbers.ranges.find(ElementKey{kind, name});
    if (it == s->s.line_numbers.ranges.end()) return 1;
    if (start) *start = it->second.start;
    if (end) *end = it->second.end;
    return PTL_OK;
}
extern "C" int ptl_strstore_get_identifier(const ptl_strstore* s, int line, char* kind, size_t kind_cap, char* name, size_t name_cap,
                                           int* local_line) {
    if (!s) return PTL_ERR_INVALID;
    ElementKey key;
    int local = 0;
    if (!s->s.line_numbers.get_identifier(line, &key, &local)) return 1;
    copy_str(kind, kind_cap, key.kind);
    copy_str(name, name_cap, key.name);
    if (local_line) *local_line = local;
    return PTL_OK;
}

extern "C" const char* ptl_device_source(const char* which) {
    if (!which) return nullptr;
    std::string w = which;
    if (w == "glsl") return device_source_glsl();
    if (w == "library") return plain_library_source().c_str();  // (no section selected: what a hand-written kernel pastes in)
    if (w == "trace") return device_source_trace_template();     // the template as embedded, conditional sections included
    if (w == "entry") return plain_entry_source().c_str();      // (no section selected, the refine slot empty)
    if (w == "refine_entry") return device_source_refine_entry();
    if (w == "refine_slices_entry") return device_source_refine_slices_entry();
    return nullptr;
}

static char* translated(const char* glsl, bool library) {
    if (!glsl) return nullptr;
    std::string out;
    try {
        out = translate_glsl(glsl, true, library);
    } catch (const std::exception& e) {  // e.g. a struct field that spells a swizzle: NULL + ptl_last_error()
        set_last_error(e.what());
        return nullptr;
    }
    char* p = (char*)std::malloc(out.size() + 1);
    std::memcpy(p, out.c_str(), out.size() + 1);
    return p;
}
extern "C" char* ptl_translate_glsl(const char* glsl) { return translated(glsl, false); }
extern "C" char* ptl_translate_library_glsl(const char* glsl) { return translated(glsl, true); }  // a file-scope library text: function definitions get PTL_FN

extern "C" char* ptl_bound_glsl(const char* glsl_body, const char* out_functions, int* bounded) {
    if (!glsl_body) return nullptr;
    std::set<std::string> with_out;
    std::string cur;
    for (const char* c = out_functions ? out_functions : ""; ; ++c) {
        if (*c == ',' || *c == '\0') {
            if (!cur.empty()) with_out.insert(cur);
            cur.clear();
            if (*c == '\0') break;
        } else {
            cur += *c;
        }
    }
    try {
        std::string out = bound_nearer_blocks(glsl_body, with_out, bounded);
        char* p = (char*)std::malloc(out.size() + 1);
        if (!p) {
            set_last_error("ptl_bound_glsl: out of memory");
            return nullptr;
        }
        std::memcpy(p, out.c_str(), out.size() + 1);
        return p;
    } catch (const std::exception& e) {  // malformed input (the tokenizer throws): an error, never an exception across the C boundary
        set_last_error(std::string("ptl_bound_glsl: ") + e.what());
        return nullptr;
    }
}

static std::vector<std::string> split(const char* text) {  // "a;b;c", empty parts dropped
    std::vector<std::string> parts;
    std::string cur;
    for (const char* c = text ? text : ""; *c; ++c) {
        if (*c == ';') {
            if (!cur.empty()) parts.push_back(cur);
            cur.clear();
        } else {
            cur += *c;
        }
    }
    if (!cur.empty()) parts.push_back(cur);
    return parts;
}

extern "C" char* ptl_specialize_translated(const char* cxx, const char* masked, const char* unroll_bounds, int* unrolled) {
    if (!cxx) return nullptr;
    try {
        std::set<std::string> matrices;
        for (const std::string& m : split(masked)) matrices.insert(m);
        std::map<std::string, int> bounds;
        for (const std::string& b : split(unroll_bounds)) {
            const size_t eq = b.find('=');
            if (eq != std::string::npos) bounds[b.substr(0, eq)] = std::atoi(b.c_str() + eq + 1);
        }
        return strdup(specialize_translated(cxx, matrices, bounds, unrolled).c_str());
    } catch (const std::exception& e) {
        set_last_error(std::string("ptl_specialize_translated: ") + e.what());
        return nullptr;
    }
}

extern "C" char* ptl_hoist_glsl(const char* glsl, const char* uniforms, const char* out_functions, int body_only, const char* params, char** prologue) {
    if (!glsl) return nullptr;
    HoistParams hp;
    for (const std::string& u : split(uniforms)) {
        size_t sp = u.find(' ');
        if (sp != std::string::npos) hp.uniforms[u.substr(sp + 1)] = u.substr(0, sp);
    }
    for (const std::string& f : split(out_functions)) {  // "name" may write through an argument; "=name" is merely defined by the scene
        if (f[0] == '=') hp.scene_functions.insert(f.substr(1));
        else hp.functions_with_out_params.insert(f);
    }
    hp.body_only = body_only != 0;
    for (const std::string& name : split(params)) {  // "@r": a ray parameter whose origin is the camera's (first-trip variant)
        if (name[0] == '@') {
            hp.origin_uniform_rays.push_back(name.substr(1));
            hp.body_params.push_back(name.substr(1));
        } else {
            hp.body_params.push_back(name);
        }
    }
    hp.origin_expr = "PTL_DV_OUT.ptl_dv_origin";
    int counter = 0;
    HoistResult r = hoist_uniform_work(glsl, hp, counter);
    if (prologue) {
        std::string text;
        for (auto& m : r.members) text += "// member: " + m.type + " " + m.name + (m.length ? "[" + std::to_string(m.length) + "]" : "") + "\n";
        text += r.prologue;
        *prologue = strdup(text.c_str());
    }
    return strdup(r.glsl.c_str());
}

extern "C" int ptl_scene_to_ron(ptl_scene* s, char** text) {
    if (!s || !text) return PTL_ERR_INVALID;
    return guarded([&] {
        *text = strdup(s->scene->to_ron().c_str());
        return PTL_OK;
    });
}

extern "C" char* ptl_ron_format(const char* text) {
    if (!text) return nullptr;
    try {
        std::string out = ron::to_string(ron::parse(text));
        return strdup(out.c_str());
    } catch (const std::exception& e) {
        set_last_error(e.what());
        return nullptr;
    }
}

extern "C" int ptl_formula_eval(const char* text, const char* const* names, const double* values, int n, double time, double* out) {
    if (!text || !out) return PTL_ERR_INVALID;
    std::string err;
    auto f = Formula::compile(text, &err);
    if (!f) {
        set_last_error(err);
        return 1;
    }
    FormulaNamespace ns = [&](const std::string& name, const std::vector<double>& args) -> std::optional<double> {
        bool known = false;
        auto r = formula_custom_function(name, args, &known);
        if (known) return r;
        if (name == "time" || name == "total_time") return time;
        for (int k = 0; k < n; ++k)
            if (name == names[k]) return values[k];
        return std::nullopt;
    };
    auto v = f->eval(ns);
    if (!v) return 1;
    *out = *v;
    return PTL_OK;
}
