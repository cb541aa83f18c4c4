// glsl_affine.cpp -- snippets_keep_rays_affine (glsl_translate.h): what the text of a scene's snippets may do to a ray while every origin keeps
// w = 1 and every direction w = 0 (KernelOptions::affine_rays).
//
// Round 6: a WHITELIST over every occurrence of a ray half, not a list of known offenders (VERDICT r5 / ADVICE r5: `r.o[3] = 2.;`, `r.o += r.d * t +
// vec4(0., 0., 0., 5.);`, `mat4 m = mat4(2.); r.o += r.d * m;`, a macro and a builtin's out parameter all passed the round-5 scan).  The invariant to keep:
// every Ray value has o.w == 1 and d.w == 0.  A Ray value comes from (1) the camera and the library (checked once, by hand and by the A/B tests), (2) the
// constructor `Ray(...)`, (3) a write to `.o` / `.d` of an existing one, (4) `transform` / `material_teleport` by some matrix.  So:
//   * nothing a token scan cannot see through: no preprocessor directive, no `out` / `inout` parameter of any type, no builtin with an out parameter
//     (modf, frexp), no use of the library's one non-affine ray constant (`ray_none`);
//   * (2) both halves spelled as `vec4(.., 1.)` / `vec4(.., 0.)`;
//   * (3) EVERY `.o` / `.d` followed (after its member / index chain) by an assignment operator or `++` / `--`, or preceded by a prefix `++` / `--`, is a
//     write: allowed to x / y / z alone (a swizzle out of xyz / rgb / stp, a literal index 0..2), or to the whole half in five spelled forms
//     (`= vec4(.., w)`, `d = normalize(same.d)`, `o += same.d * S`, `o = same.o + same.d * S` with S a product of factors none of which names a matrix);
//     anything else -- `.w`, `[i]`, `[3]`, a deeper chain, another right-hand side -- switches the optimisation off;
//   * (4) the matrix is a scene uniform by name (those the generator and the renderer check for the bottom row 0 0 0 1).
// What the scan cannot prove it refuses; what it accepts is hunted by tests/test_affine_guard_fuzz.py (random legal ray writes, frames with and without
// affine rays) and, on the device, checked by the PTL_CHECK_AFFINE build (ptl_renderer_check_affine).
#include <cctype>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "glsl_tokens.h"
#include "glsl_translate.h"

namespace ptl {

static bool ends_with(const std::string& x, const char* tail) {
    const size_t n = std::strlen(tail);
    return x.size() > n && x.compare(x.size() - n, n, tail) == 0;
}

bool is_scene_matrix_name(const std::string& name) { return ends_with(name, "_mat") || ends_with(name, "_mat_inv") || ends_with(name, "_mat_teleport"); }

namespace {

// The scan sees identifiers, numbers and punctuation.  (Directives and inserted text are looked for on the stream itself, before any rule runs.)
constexpr unsigned kNoCode = token_kinds({Token::Space, Token::Comment, Token::Preproc, Token::Raw});

bool matrix_type(const std::string& x) { return x.size() >= 4 && x.compare(0, 3, "mat") == 0 && std::isdigit((unsigned char)x[3]); }

// every name some snippet declares with a matrix type: locals, parameters, functions that return a matrix (too many names only refuse more)
void collect_matrix_names(const TokenView& t, std::set<std::string>& names) {
    for (size_t i = 0; i + 1 < t.n(); ++i) {
        if (!t.ident(i) || !matrix_type(t[i].text) || !t.ident(i + 1)) continue;
        names.insert(t[i + 1].text);
        int depth = 0;  // `mat4 a = .., b = ..;`
        for (size_t k = i + 2; k < t.n() && depth >= 0 && !t.is(k, ";") && !t.is(k, "{"); ++k) {
            if (t.is(k, "(") || t.is(k, "[")) ++depth;
            else if (t.is(k, ")") || t.is(k, "]")) --depth;
            else if (depth == 0 && t.is(k, ",") && t.ident(k + 1) && k + 2 < t.n() && !t.ident(k + 2)) names.insert(t[k + 1].text);
        }
    }
}

bool names_a_matrix(const std::string& x, const std::set<std::string>& matrix_names) {
    return matrix_type(x) || x == "inverse" || x == "transpose" || x == "outerProduct" || x == "matrixCompMult" || is_scene_matrix_name(x) || matrix_names.count(x) != 0;
}

// t[from, to) is `vec4(<three components in one or three arguments>, <the literal w>)`
bool is_vec4_with_w(const TokenView& t, size_t from, size_t to, double w) {
    if (to < from + 4 || !t.ident(from, "vec4") || !t.is(from + 1, "(") || t.close_of(from + 1) != to - 1) return false;
    const auto parts = t.split_top_level(from + 2, to - 1, ",");
    if (parts.size() != 2 && parts.size() != 4) return false;
    const auto [a, b] = parts.back();
    if (b != a + 1 || !t.number(a)) return false;
    char* end = nullptr;
    const double v = std::strtod(t[a].text.c_str(), &end);
    return end != t[a].text.c_str() && (*end == '\0' || *end == 'f' || *end == 'F') && v == w;
}

// the argument [part.first, part.second) is one name: a scene matrix that no snippet declares as something else
bool is_uniform_matrix_argument(const TokenView& t, std::pair<size_t, size_t> part, const std::set<std::string>& matrix_names) {
    return part.second == part.first + 1 && t.ident(part.first) && is_scene_matrix_name(t[part.first].text) && matrix_names.count(t[part.first].text) == 0;
}

// ---- the rules: each looks at token i and says why the snippet is refused (and from which token on to quote it), or nothing ----------------------
struct Refusal {
    const char* what = nullptr;
    size_t at = 0;
    explicit operator bool() const { return what != nullptr; }
};
using MatrixNames = std::set<std::string>;

Refusal stray_hash(const TokenView& t, size_t i, const MatrixNames&) {  // (a `#` that does not start its line: the lexer makes no directive of it)
    return t.is(i, "#") ? Refusal{"a preprocessor directive (a macro hides what it expands to from the scan)", i} : Refusal{};
}
// out / inout parameters (of any type: `f(r.o.w)` into an `out float`), and the builtins that have one
Refusal out_parameter(const TokenView& t, size_t i, const MatrixNames&) {
    return t.ident(i, "out") || t.ident(i, "inout") ? Refusal{"an out parameter (it could carry a ray half)", i} : Refusal{};
}
Refusal out_parameter_builtin(const TokenView& t, size_t i, const MatrixNames&) {
    return (t.ident(i, "modf") || t.ident(i, "frexp")) && !(i > 0 && t.is(i - 1, ".")) ? Refusal{"a builtin with an out parameter", i} : Refusal{};
}
Refusal ray_none_constant(const TokenView& t, size_t i, const MatrixNames&) {
    return t.ident(i, "ray_none") && !(i > 0 && t.is(i - 1, ".")) ? Refusal{"the library's ray constant whose origin has w = 0", i} : Refusal{};
}

// Ray( origin, direction, ... ): both halves spelled with their w
Refusal ray_constructor(const TokenView& t, size_t i, const MatrixNames&) {
    if (!(t.ident(i, "Ray") && t.is(i + 1, "("))) return {};
    const size_t close = t.close_of(i + 1);
    if (close == t.n()) return {"an unbalanced Ray constructor", i};
    const auto parts = t.split_top_level(i + 2, close, ",");
    if (parts.size() < 2 || !is_vec4_with_w(t, parts[0].first, parts[0].second, 1.0) || !is_vec4_with_w(t, parts[1].first, parts[1].second, 0.0))
        return {"a Ray built from halves whose w is not spelled", i};
    return {};
}

// A call of `name` (not its definition, which has `result_type` in front: anything else there, `return` included, is a call) with `args` arguments of
// which number `matrix` is one the affinity checks see -- a scene uniform by name, not a matrix the snippet computed
Refusal call_by_uniform_matrix(const TokenView& t, size_t i, const MatrixNames& matrix_names, const char* name, const char* result_type, size_t args, size_t matrix,
                               const char* unbalanced, const char* not_a_uniform) {
    if (!(t.ident(i, name) && t.is(i + 1, "(") && !(i > 0 && t.ident(i - 1, result_type)))) return {};
    const size_t close = t.close_of(i + 1);
    if (close == t.n()) return {unbalanced, i};
    const auto parts = t.split_top_level(i + 2, close, ",");
    if (!(parts.size() == args && is_uniform_matrix_argument(t, parts[matrix], matrix_names))) return {not_a_uniform, i};
    return {};
}
// transform(<matrix>, ray) (`Ray transform(mat4 m, Ray r) {` is the library's definition)
Refusal transform_call(const TokenView& t, size_t i, const MatrixNames& matrix_names) {
    return call_by_uniform_matrix(t, i, matrix_names, "transform", "Ray", 2, 0, "an unbalanced transform call", "transform() by a matrix that is not a scene uniform");
}
// material_teleport(hit, r, <matrix>) (library.glsl:376-379: it transforms r by the matrix and hands the result back to be traced): the same rule
Refusal material_teleport_call(const TokenView& t, size_t i, const MatrixNames& matrix_names) {
    return call_by_uniform_matrix(t, i, matrix_names, "material_teleport", "MaterialProcessing", 3, 2, "an unbalanced material_teleport call",
                                  "material_teleport() by a matrix that is not a scene uniform");
}

// every occurrence of <owner>.o / <owner>.d: t[i] is the `.`
Refusal ray_half_write(const TokenView& t, size_t i, const MatrixNames& matrix_names) {
    if (!(t.is(i, ".") && (t.ident(i + 1, "o") || t.ident(i + 1, "d")))) return {};
    const bool origin = t[i + 1].text == "o";
    const char* const unknown_form = "a ray half assigned in a form that is not known to keep its w";
    // what follows the half: a chain of `.member` and `[index]`
    size_t j = i + 2;
    int links = 0;
    bool xyz_only = false;
    while (j < t.n()) {
        if (t.is(j, ".") && t.ident(j + 1)) {
            bool inside = !t[j + 1].text.empty() && t[j + 1].text.size() <= 4;
            for (char c : t[j + 1].text) inside = inside && std::strchr("xyzrgbstp", c) != nullptr;  // (no w / a / q; anything that is no swizzle at all counts as unknown)
            xyz_only = inside;
            ++links;
            j += 2;
        } else if (t.is(j, "[")) {
            const size_t close = t.close_of(j);
            if (close == t.n()) return {"an unbalanced index", i};
            xyz_only = close == j + 2 && t.number(j + 1) && (t[j + 1].text == "0" || t[j + 1].text == "1" || t[j + 1].text == "2");
            ++links;
            j = close + 1;
        } else break;
    }
    // the owner of the member, as written: `a.b[c]` in front of `.o`
    size_t own = i;
    while (own > 0) {
        if (t.ident(own - 1) || t.is(own - 1, ".")) --own;
        else if (t.is(own - 1, "]")) {
            own = t.open_of(own - 1);
            if (own == t.n()) return {"an unbalanced index", i};
        } else break;
    }
    const bool prefix_write = own > 0 && (t.is(own - 1, "++") || t.is(own - 1, "--"));
    // (the lexer knows `+= -= *= /= ++ --`; the integer forms reach here as two tokens: `% =`, `<< =`, `& =` ... -- not legal on a float vector, refused all the same)
    const bool two_token_assignment = t.is(j + 1, "=") && (t.is(j, "%") || t.is(j, "<<") || t.is(j, ">>") || t.is(j, "&") || t.is(j, "|") || t.is(j, "^"));
    if (two_token_assignment) return {unknown_form, own};
    const bool postfix_write = j < t.n() && is_assignment_op(t[j]);
    if (!prefix_write && !postfix_write) return {};  // a read (there are no out parameters it could be bound to)
    if (links > 0) {
        if (links == 1 && xyz_only) return {};  // x / y / z alone
        return {"a write that may reach the w of a ray half", own};
    }
    if (prefix_write || j >= t.n()) return {unknown_form, own};
    size_t end = j + 1;  // the statement's right-hand side: up to the `;` at this nesting level
    int depth = 0;
    while (end < t.n() && !(depth == 0 && t.is(end, ";"))) {
        if (t.is(end, "(") || t.is(end, "[")) ++depth;
        else if ((t.is(end, ")") || t.is(end, "]")) && --depth < 0) break;  // (`for (..; ..; r.o += r.d * s)`, an argument: the expression ends with the group it stands in)
        ++end;
    }
    const auto spells = [&](size_t from, const std::vector<std::string>& words) { return from + words.size() <= end && t.spells(from, words); };
    const auto member = [&](const char* half) {  // the same owner's `.o` / `.d`, as words
        std::vector<std::string> w;
        for (size_t k = own; k < i; ++k) w.push_back(t[k].text);
        w.push_back(".");
        w.push_back(half);
        return w;
    };
    // t[from, end) is a product of factors -- names, numbers, member chains, calls, parenthesised groups, joined by `*` and `/`, one leading `-` --
    // with nothing else at the top level (no `+`, no `,`, no `?`), and no factor names a matrix (`X.d * <matrix>` is GLSL too: a row vector times
    // a matrix, with whatever w comes out).  Then `X.d * S` has the w `0 * S.w`-or-`0 * S`: 0.
    const auto scalar_factors = [&](size_t from) {
        if (from >= end) return false;
        int depth = 0;
        for (size_t k = from; k < end; ++k) {
            if (t.ident(k) && names_a_matrix(t[k].text, matrix_names)) return false;
            if (t.is(k, "(") || t.is(k, "[")) ++depth;
            else if (t.is(k, ")") || t.is(k, "]")) --depth;
            else if (depth == 0 && !(t.ident(k) || t.number(k) || t.is(k, "*") || t.is(k, "/") || t.is(k, ".") || (t.is(k, "-") && k == from))) return false;
        }
        return depth == 0;
    };
    if (origin && t.is(j, "+=")) {  // X.o += X.d * S
        std::vector<std::string> lead = member("d");
        lead.push_back("*");
        if (spells(j + 1, lead) && scalar_factors(j + 1 + lead.size())) return {};
    }
    if (t.is(j, "=")) {
        if (is_vec4_with_w(t, j + 1, end, origin ? 1.0 : 0.0)) return {};  // X.o = vec4(.., 1.) / X.d = vec4(.., 0.)
        if (!origin) {  // X.d = normalize(X.d)
            std::vector<std::string> call = {"normalize", "("};
            for (auto& w : member("d")) call.push_back(w);
            call.push_back(")");
            if (spells(j + 1, call) && j + 1 + call.size() == end) return {};
        } else {  // X.o = X.o + X.d * S
            std::vector<std::string> lead = member("o");
            lead.push_back("+");
            for (auto& w : member("d")) lead.push_back(w);
            lead.push_back("*");
            if (spells(j + 1, lead) && scalar_factors(j + 1 + lead.size())) return {};
        }
    }
    return {unknown_form, own};
}

using Rule = Refusal (*)(const TokenView&, size_t, const MatrixNames&);
constexpr Rule kRules[] = {stray_hash, out_parameter, out_parameter_builtin, ray_none_constant, ray_constructor, transform_call, material_teleport_call, ray_half_write};

}  // namespace

bool snippets_keep_rays_affine(const std::vector<std::string>& codes, std::string* why) {
    std::vector<std::vector<Token>> streams;
    for (const std::string& code : codes) streams.push_back(tokenize_glsl(code));
    std::vector<TokenView> views;  // (built once every stream stands where it stays)
    for (const auto& stream : streams) views.emplace_back(stream, kNoCode);
    MatrixNames matrix_names;
    for (const TokenView& t : views) collect_matrix_names(t, matrix_names);
    for (size_t c = 0; c < codes.size(); ++c) {
        for (const Token& raw : streams[c])
            if (raw.kind == Token::Preproc || raw.kind == Token::Raw) {
                if (why) *why = "a preprocessor directive (a macro hides what it expands to from the scan): " + raw.text.substr(0, 60);
                return false;
            }
        const TokenView& t = views[c];
        for (size_t i = 0; i < t.n(); ++i)
            for (Rule rule : kRules)
                if (const Refusal refusal = rule(t, i, matrix_names)) {
                    if (why) {
                        *why = std::string(refusal.what) + ":";
                        for (size_t k = refusal.at; k < t.n() && k < refusal.at + 12; ++k) *why += " " + t[k].text;
                    }
                    return false;
                }
    }
    return true;
}

}  // namespace ptl
