// glsl_binding.cpp -- see glsl_binding.h.
#include "glsl_binding.h"

#include <algorithm>

namespace ptl {
namespace {

bool float_type(const std::string& t) { return t == "float" || t == "vec2" || t == "vec3" || t == "vec4" || t == "mat2" || t == "mat3" || t == "mat4"; }
int vec_size(const std::string& t) { return t == "vec2" ? 2 : t == "vec3" ? 3 : t == "vec4" ? 4 : 0; }
int mat_size(const std::string& t) { return t == "mat2" ? 2 : t == "mat3" ? 3 : t == "mat4" ? 4 : 0; }
std::string vec_of(int n) { return n == 1 ? "float" : n == 2 ? "vec2" : n == 3 ? "vec3" : n == 4 ? "vec4" : ""; }
bool type_name(const std::string& t) {
    static const std::set<std::string> names = {"float", "int", "uint", "bool", "vec2", "vec3", "vec4", "ivec2", "ivec3", "ivec4", "uvec2", "uvec3",
                                                "uvec4", "bvec2", "bvec3", "bvec4", "mat2", "mat3", "mat4"};
    return names.count(t) != 0;
}

// GLSL built-ins (and the two pure helpers of the reference's library every scene uses) with the rule that types their result
enum class Ret { Arg0, Arg1, Arg2, Float, Vec3 };
const std::map<std::string, Ret>& pure_functions() {
    static const std::map<std::string, Ret> f = {
        {"normalize", Ret::Arg0}, {"abs", Ret::Arg0},   {"sign", Ret::Arg0},    {"floor", Ret::Arg0},       {"ceil", Ret::Arg0},     {"fract", Ret::Arg0},
        {"sqrt", Ret::Arg0},      {"inversesqrt", Ret::Arg0}, {"sin", Ret::Arg0}, {"cos", Ret::Arg0},       {"tan", Ret::Arg0},      {"asin", Ret::Arg0},
        {"acos", Ret::Arg0},      {"atan", Ret::Arg0},  {"exp", Ret::Arg0},     {"log", Ret::Arg0},         {"exp2", Ret::Arg0},     {"log2", Ret::Arg0},
        {"radians", Ret::Arg0},   {"degrees", Ret::Arg0}, {"pow", Ret::Arg0},   {"mod", Ret::Arg0},         {"min", Ret::Arg0},      {"max", Ret::Arg0},
        {"clamp", Ret::Arg0},     {"mix", Ret::Arg0},   {"step", Ret::Arg1},    {"smoothstep", Ret::Arg2},  {"length", Ret::Float},  {"distance", Ret::Float},
        {"dot", Ret::Float},      {"cross", Ret::Vec3}, {"reflect", Ret::Arg0}, {"transpose", Ret::Arg0},   {"inverse", Ret::Arg0},  {"determinant", Ret::Float},
        {"get_normal", Ret::Vec3}, {"sqr", Ret::Arg0},
    };
    return f;
}

void combine(Binding& bd, const Binding& kid) {
    bd.leaf = bd.leaf || kid.leaf;
    bd.op = bd.op || kid.op;
    bd.cost += kid.cost;
    if (kid.loop > 0) {
        if (bd.loop == 0) {
            bd.loop = kid.loop;
            bd.phase = kid.phase;
        } else if (bd.loop != kid.loop || bd.phase != kid.phase) {
            bd.phase = -1;
        }
    }
}

}  // namespace

bool Binding::hoistable() const { return placeable() && op && cost >= 3 && float_type(type); }

BindingTimes::BindingTimes(const TokenView& s, const ParsedBody& body, const HoistParams& params, const std::vector<std::string>& param_names, size_t body_e)
    : s_(s), body_(body), P(params), body_e_(body_e), bindings_(body.nodes.size()) {
    for (const std::string& p : param_names) {
        declared_.insert(p);
        ++writes_[p];
    }
    for (const Site& site : body_.sites) {
        if (site.kind != Site::Expr) {  // (a declaration is the first write of its name)
            declared_.insert(site.decl_name);
            ++writes_[site.decl_name];
        }
        if (site.root >= 0) count_writes(site.root);
    }
    // locals that are uniform values (written once: their declaration) or uniform sequences (once more: their update in a loop), in the
    // order of their declarations: each is judged by what is known of the ones before it
    for (size_t si = 0; si < body_.sites.size(); ++si) {
        const Site& site = body_.sites[si];
        if (site.kind != Site::DeclInit || site.depth != 0 || site.loop != 0) continue;
        const bool ray = site.decl_type == "Ray" && !P.origin_uniform_rays.empty();
        if (ray || type_name(site.decl_type)) top_level_local(si, ray);
    }
    drop_chains_that_read_a_dropped_one();
}

int BindingTimes::writes(const std::string& name) const {
    auto it = writes_.find(name);
    return it == writes_.end() ? 0 : it->second;
}

void BindingTimes::count_writes(int id) {
    const Node& nd = body_.nodes[id];
    if (nd.kind == Node::Assign) ++writes_[body_.base_identifier(nd.kids[0])];
    if (nd.kind == Node::Post || (nd.kind == Node::Unary && (nd.text == "++" || nd.text == "--"))) ++writes_[body_.base_identifier(nd.kids[0])];
    // ... and the GLSL built-ins that write through an argument (GLSL ES 3.00 8.3, 8.8): `float ip = 0.0; f = modf(x, ip);` leaves
    // `ip` written twice, not a write-once uniform local (the prelude has no modf / frexp today; the day it gets one this must hold)
    static const std::set<std::string> builtin_out = {"modf", "frexp", "umulExtended", "imulExtended", "uaddCarry", "usubBorrow"};
    if (nd.kind == Node::Call && (P.functions_with_out_params.count(nd.text) || builtin_out.count(nd.text)))
        for (int k : nd.kids) ++writes_[body_.base_identifier(k)];
    for (int k : nd.kids) count_writes(k);
}

bool BindingTimes::is_update(size_t site) const {
    for (auto& c : carried_)
        if (c.second.update_site == (int)site) return true;
    return false;
}

// `T V = <uniform>;` / `Ray V = <ray with a uniform origin>;` at the top level of the function: V keeps that property if nothing else
// writes it, or if the one other write is its update in a canonical loop.
void BindingTimes::top_level_local(size_t si, bool ray) {
    const Site& decl = body_.sites[si];
    const int w = writes(decl.decl_name);
    if (w != 1 && w != 2) return;
    const Binding init = classify(decl.root);
    if (!(ray ? init.half : init.uniform) || init.loop != 0) return;
    if (!ray && !init.type.empty() && init.type != decl.decl_type) return;  // (an implicit conversion we do not model)
    const Local local{decl.decl_type, decl.name_at, ray || init.leaf, ray};
    if (w == 1) {
        locals_[decl.decl_name] = local;
        return;
    }
    const int ui = update_in_canonical_loop(si, ray);
    if (ui < 0) return;
    const Site& update = body_.sites[ui];
    const int rhs_id = body_.nodes[update.root].kids[1];
    // The update is classified with V itself already carried -- a uniform chain at first without `leaf`: does it read a run-time uniform
    // besides itself? -- and, between its declaration and the loop, an ordinary local.
    carried_[decl.decl_name] = {decl.decl_type, update.loop, ui, ray, ray};
    locals_[decl.decl_name] = local;
    const Binding rhs = classify(rhs_id);
    // what the two kinds ask of the update's right-hand side: a uniform chain its own type and some run-time uniform in it, a ray its origin
    const bool kind_ok = ray ? rhs.half : rhs.uniform && rhs.type == decl.decl_type && (init.leaf || rhs.leaf);
    if (kind_ok && (rhs.loop == 0 || rhs.loop == update.loop) && rhs.phase >= 0 && !body_.mentions(rhs_id, body_.loops[update.loop - 1].var)) {
        carried_[decl.decl_name].leaf = true;
    } else {
        carried_.erase(decl.decl_name);
        locals_.erase(decl.decl_name);
    }
}

// For the twice-written local declared at site `si`: the site of `V = ...;` if that is a statement directly in the body of a canonical
// loop at the function's top level from which V can be tabulated, else -1.  The FIRST assignment to V decides.
int BindingTimes::update_in_canonical_loop(size_t si, bool ray) const {
    const std::string& name = body_.sites[si].decl_name;
    for (size_t ui = si + 1; ui < body_.sites.size(); ++ui) {
        const Site& u = body_.sites[ui];
        if (u.kind != Site::Expr || u.header || u.loop == 0 || u.stmt_e == 0) continue;
        const Node& root = body_.nodes[u.root];
        if (root.kind != Node::Assign || root.text != "=" || body_.nodes[root.kids[0]].kind != Node::Ident || body_.nodes[root.kids[0]].text != name) continue;
        const LoopInfo& L = body_.loops[u.loop - 1];
        if (!L.canonical || !L.braced || L.outer != 0 || L.depth != 0 || L.has_continue || u.depth != L.depth + 1) return -1;
        if (writes(L.var) != 2 || (declared_.count(L.bound) && writes(L.bound) != 1)) return -1;
        // the guard's declaration is inserted in front of the keyword: that must be the start of a statement.  (V's declaration at depth
        // 0 stands in front of the loop, so the keyword is never the body's first token and there is always a token to look at.)
        if (!(s_.is(L.kw - 1, ";") || s_.is(L.kw - 1, "{") || s_.is(L.kw - 1, "}"))) return -1;
        if (tokens_mention(s_, L.header_open, L.header_close, name) || tokens_mention(s_, L.body_e, body_e_, name)) return -1;
        if (ray) {
            // A ray chain must also be READ directly in the loop's body, outside its update: one that is only read in nested blocks is left
            // to the translator's deferred updates, which skip it altogether.  (A uniform chain is not asked this.)
            bool read_in_the_body = false;
            for (size_t k = 0; k < body_.sites.size(); ++k) {
                const Site& r = body_.sites[k];
                read_in_the_body = read_in_the_body || (k != ui && r.root >= 0 && !r.header && r.loop == u.loop && r.depth == L.depth + 1 && body_.mentions(r.root, name));
            }
            if (!read_in_the_body) return -1;
        }
        return (int)ui;
    }
    return -1;
}

// An update may read another carried variable: every one of them has to have survived.  ASYMMETRY, kept as it was found: only the
// uniform chains are looked at again.  A ray chain `V = transform(M, V)` whose matrix M is a uniform chain that this loop drops would
// stay carried, with M varying in its update.  No input is known that gets here: locals are judged in the order of their declarations
// (top_level_local), an update that reads a local declared later fails on the spot, and one that reads an earlier local reads one
// whose fate was settled -- so by induction nothing accepted is dropped here, and the loop never erases.  DESIGN.md has the note.
void BindingTimes::drop_chains_that_read_a_dropped_one() {
    for (bool again = true; again;) {
        again = false;
        for (auto it = carried_.begin(); it != carried_.end(); ++it) {
            if (it->second.ray) continue;
            if (!classify(body_.nodes[body_.sites[it->second.update_site].root].kids[1]).uniform) {
                locals_.erase(it->first);
                carried_.erase(it);
                again = true;
                break;
            }
        }
    }
}

void BindingTimes::classify_identifier(const Node& nd, Binding& bd) const {
    auto known = [&](const std::string& type, bool leaf, bool ray) {
        bd.type = type;
        bd.leaf = leaf;
        bd.uniform = !ray;
        bd.half = ray;
    };
    if (nd.text == "true" || nd.text == "false") return known("bool", false, false);
    auto c = carried_.find(nd.text);
    if (c != carried_.end()) {
        const LoopInfo& L = body_.loops[c->second.loop - 1];
        if (nd.b >= L.body_b && nd.b < L.body_e) {  // inside its loop: the value of this trip, before or after the update
            const Site& upd = body_.sites[c->second.update_site];
            bd.loop = c->second.loop;
            bd.phase = nd.b < upd.stmt_b ? 0 : (nd.b >= upd.stmt_e ? 1 : 0);
            return known(c->second.type, c->second.leaf, c->second.ray);
        }
    }
    auto l = locals_.find(nd.text);
    if (l != locals_.end() && nd.b > l->second.name_at) return known(l->second.type, l->second.leaf, l->second.ray);
    // a parameter whose origin is the camera's (written once: a local of that name would be a second write)
    if (std::find(P.origin_uniform_rays.begin(), P.origin_uniform_rays.end(), nd.text) != P.origin_uniform_rays.end() && writes(nd.text) == 1) return known("Ray", true, true);
    if (declared_.count(nd.text)) return;
    auto g = P.uniforms.find(nd.text);
    if (g != P.uniforms.end()) return known(g->second, true, false);
    auto k = P.constants.find(nd.text);
    if (k != P.constants.end()) return known(k->second, false, false);
}

const Binding& BindingTimes::classify(int id) {
    const Node& nd = body_.nodes[id];
    for (int k : nd.kids) classify(k);
    Binding bd;
    auto kid = [&](size_t i) -> const Binding& { return bindings_[nd.kids[i]]; };
    switch (nd.kind) {
        case Node::Lit:
            bd.uniform = true;
            bd.type = is_float_typed_literal(nd.text) ? "float" : ((nd.text.back() == 'u' || nd.text.back() == 'U') ? "uint" : "int");
            break;
        case Node::Ident:
            classify_identifier(nd, bd);
            break;
        case Node::Paren:
            bd.uniform = kid(0).uniform;
            bd.half = kid(0).half;
            bd.type = kid(0).type;
            combine(bd, kid(0));
            break;
        case Node::Unary:
            if (nd.text == "++" || nd.text == "--") break;
            bd.uniform = kid(0).uniform;
            bd.type = nd.text == "!" ? "bool" : kid(0).type;
            combine(bd, kid(0));
            break;
        case Node::Post:
        case Node::Assign:
            break;
        case Node::Binary: {
            const Binding &a = kid(0), &b = kid(1);
            bd.uniform = a.uniform && b.uniform;
            combine(bd, a);
            combine(bd, b);
            const std::string& op = nd.text;
            if (op == "*" || op == "/" || op == "+" || op == "-") {
                if (a.type == b.type) bd.type = a.type;
                else if (a.type == "float" && (vec_size(b.type) || mat_size(b.type))) bd.type = b.type;
                else if (b.type == "float" && (vec_size(a.type) || mat_size(a.type))) bd.type = a.type;
                else if (op == "*" && mat_size(a.type) && mat_size(a.type) == vec_size(b.type)) bd.type = b.type;
                else if (op == "*" && mat_size(b.type) && mat_size(b.type) == vec_size(a.type)) bd.type = a.type;
                if (float_type(bd.type)) {
                    bd.op = true;
                    const int ma = mat_size(a.type), mb = mat_size(b.type), width = vec_size(bd.type) ? vec_size(bd.type) : (mat_size(bd.type) ? mat_size(bd.type) * mat_size(bd.type) : 1);
                    bd.cost += (op == "*" && ma && mb) ? ma * ma * ma : (op == "*" && (ma || mb) && vec_size(bd.type)) ? width * width : (op == "/" ? 10 : 1) * width;
                } else if (op == "/") bd.uniform = false;  // an integer quotient may trap where the snippet guards it
            } else if (op == "%" || op == "<<" || op == ">>" || op == "&" || op == "|" || op == "^") {
                bd.type = a.type == b.type ? a.type : "";
                if (op == "%") bd.uniform = false;
            } else {
                bd.type = "bool";
            }
            break;
        }
        case Node::Ternary:
            bd.uniform = kid(0).uniform && kid(1).uniform && kid(2).uniform;
            for (int i = 0; i < 3; ++i) combine(bd, kid(i));
            bd.type = kid(1).type == kid(2).type ? kid(1).type : "";
            break;
        case Node::Call: {
            bool all = true;
            for (size_t i = 0; i < nd.kids.size(); ++i) {
                all = all && kid(i).uniform;
                combine(bd, kid(i));
            }
            if (nd.text == "transform" && nd.kids.size() == 2 && library_function("transform") && kid(0).uniform && kid(0).type == "mat4" && kid(1).half) {
                bd.half = true;  // (combine() above has merged leaf / loop / phase / cost of both arguments)
                bd.type = "Ray";
                bd.op = true;
                bd.cost += 16;
                break;
            }
            if (type_name(nd.text)) {
                bd.uniform = all && !nd.kids.empty();
                bd.type = nd.text;
                break;
            }
            auto f = pure_functions().find(nd.text);
            if (f == pure_functions().end() || !library_function(nd.text) || nd.kids.empty()) break;  // (not uniform: wiped below)
            bd.uniform = all;
            bd.op = true;
            bd.cost += 8;
            const size_t want = f->second == Ret::Arg1 ? 1 : f->second == Ret::Arg2 ? 2 : 0;
            if (f->second == Ret::Float) bd.type = "float";
            else if (f->second == Ret::Vec3) bd.type = "vec3";
            else if (want < nd.kids.size()) bd.type = kid(want).type;
            if (!float_type(bd.type)) bd.type.clear();  // (an integer overload: not ours to type)
            break;
        }
        case Node::Member:
            if (kid(0).half && nd.text == "o") {
                bd.uniform = true;
                bd.type = "vec4";
                combine(bd, kid(0));
            } else if (kid(0).uniform && vec_size(kid(0).type) && !component_indices(nd.text).empty()) {
                bd.uniform = true;
                bd.type = vec_of((int)nd.text.size());
                combine(bd, kid(0));
            }
            break;
        case Node::Index:
            if (kid(0).uniform && kid(1).uniform && (mat_size(kid(0).type) || vec_size(kid(0).type))) {
                bd.uniform = true;
                bd.type = mat_size(kid(0).type) ? vec_of(mat_size(kid(0).type)) : "float";
                combine(bd, kid(0));
                combine(bd, kid(1));
            }
            break;
    }
    if (!bd.uniform && !bd.half) {  // varying: what it is made of is of no interest (its type is kept)
        bd.leaf = bd.op = false;
        bd.loop = 0;
        bd.phase = 0;
        bd.cost = 0;
    }
    return bindings_[id] = bd;
}

}  // namespace ptl
