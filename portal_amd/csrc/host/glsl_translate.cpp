// glsl_translate.cpp -- see glsl_translate.h.
#include "glsl_translate.h"
#include "glsl_syntax.h"
#include "glsl_tokens.h"

#include <stdexcept>

#include <algorithm>
#include <set>
#include <vector>

namespace ptl {

std::string filter_tagged_lines(const std::string& text, const CodegenFlags& f) {
    std::string out;
    out.reserve(text.size());
    size_t pos = 0;
    while (pos <= text.size()) {
        size_t eol = text.find('\n', pos);
        bool last = eol == std::string::npos;
        std::string line = text.substr(pos, last ? std::string::npos : eol - pos);
        auto has = [&](const char* tag) { return line.find(tag) != std::string::npos; };
        bool skip = (has("!FOR_NUMBER!") && f.for_prefer_variable) || (has("!FOR_VARIABLE!") && !f.for_prefer_variable) ||
                    (has("!ANTIALIASING!") && f.disable_antialiasing) || (has("!ANAGLYPH!") && f.disable_anaglyph) ||
                    (has("!CAMERA_TELEPORTATION!") && f.disable_camera_teleportation) || (has("!GLSL100!") && f.use_300_version) ||
                    (has("!GLSL300!") && !f.use_300_version);
        if (!skip) out += line;
        if (last) break;
        out += '\n';
        pos = eol + 1;
    }
    return out;
}

namespace {

const std::set<std::string>& cpp_only_keywords() {
    static const std::set<std::string> k = {
        "alignas", "alignof", "and", "and_eq", "asm", "auto", "bitand", "bitor", "catch", "char", "class", "compl", "concept",
        "const_cast", "consteval", "constexpr", "constinit", "co_await", "co_return", "co_yield", "decltype", "delete",
        "dynamic_cast", "enum", "explicit", "export", "extern", "friend", "goto", "inline", "long", "mutable", "namespace", "new",
        "noexcept", "not", "not_eq", "nullptr", "operator", "or", "or_eq", "private", "protected", "public", "register",
        "reinterpret_cast", "requires", "short", "signed", "sizeof", "static", "static_assert", "static_cast", "template", "this",
        "thread_local", "throw", "try", "typedef", "typeid", "typename", "union", "unsigned", "using", "virtual", "volatile",
        "wchar_t", "xor", "xor_eq", "double"};
    return k;
}

bool looks_like_a_uniform(const std::string& name) {
    const bool float_uniform = name.size() > 2 && name.compare(name.size() - 2, 2, "_u") == 0;
    return is_scene_matrix_name(name) || float_uniform || (name.size() > 1 && name[0] == '_');
}

// See glsl_translate.h (`defer_loop_updates`).  Works on the significant tokens; every check that fails leaves the loop untouched.
void defer_loop_carried_updates(std::vector<Token>& toks) {
    const TokenView s(toks);  // the edits are collected and applied once the scan is over: the view never sees a changed stream
    const size_t n = s.n();
    // identifiers the snippet assigns or declares somewhere: never treated as loop-invariant
    std::set<std::string> written;
    for (size_t i = 0; i < n; ++i) {
        if (s[i].kind != Token::Ident) continue;
        bool target = (i + 1 < n && is_assignment_op(s[i + 1])) || (i > 0 && (s.is(i - 1, "++") || s.is(i - 1, "--")));
        bool declared = i > 0 && s[i - 1].kind == Token::Ident && i + 1 < n && (s.is(i + 1, "=") || s.is(i + 1, ";") || s.is(i + 1, ",") || s.is(i + 1, ")") || s.is(i + 1, "["));
        if (target || declared) written.insert(s[i].text);
    }
    for (size_t i = 0; i < n; ++i)
        if (s.ident(i, "do") || s.ident(i, "goto")) return;  // do-while bodies are not tracked as loops: leave such code alone
    struct Loop {
        size_t kw, header_open, header_close, body_open, body_close;
    };
    std::vector<Loop> loops;  // every loop with a braced body, `for` and `while`
    for (size_t i = 0; i + 1 < n; ++i) {
        if (!(s.ident(i, "for") || s.ident(i, "while")) || !s.is(i + 1, "(")) continue;
        size_t close = s.close_of(i + 1);
        if (close >= n || !s.is(close + 1, "{")) continue;
        size_t end = s.close_of(close + 1);
        if (end >= n) continue;
        loops.push_back({i, i + 1, close, close + 1, end});
    }
    TokenEdits edits(toks);  // every text goes in front of a significant token; the update statement itself is dropped
    int counter = 0;
    for (const Loop& L : loops) {
        if (!s.ident(L.kw, "for")) continue;
        bool nested = false;
        for (const Loop& O : loops) nested = nested || (O.body_open < L.kw && L.kw < O.body_close);
        if (nested) continue;
        if (L.kw > 0 && !(s.is(L.kw - 1, ";") || s.is(L.kw - 1, "{") || s.is(L.kw - 1, "}"))) continue;  // `if (c) for ...`: nowhere to declare the counter
        // the enclosing function: for a body-only snippet (loop at brace depth 0) the whole text, else from the brace that opens the
        // function body to the one that closes it
        size_t fn_begin = 0, fn_end = n;
        {
            int depth = 0;
            for (size_t i = 0; i < L.kw; ++i) {
                if (s.is(i, "{") && depth++ == 0) fn_begin = i + 1;
                else if (s.is(i, "}")) --depth;
            }
            if (depth == 0) fn_begin = 0;
            if (depth > 0) {
                int d = depth;
                for (size_t i = L.body_close + 1; i < n; ++i) {
                    d += s.is(i, "{") ? 1 : s.is(i, "}") ? -1 : 0;
                    if (d == 0) {
                        fn_end = i;
                        break;
                    }
                }
            }
        }
        // statement starts inside the body, by paren depth 0 delimiters
        int brace = 0, paren = 0;
        size_t stmt_start = L.body_open + 1;
        std::vector<size_t> start_of(n, 0);
        std::vector<int> depth_of(n, 0);
        for (size_t i = L.body_open + 1; i < L.body_close; ++i) {
            start_of[i] = stmt_start;
            depth_of[i] = brace;
            if (s.is(i, "(")) ++paren;
            else if (s.is(i, ")")) --paren;
            else if (s.is(i, "{")) { ++brace; if (paren == 0) stmt_start = i + 1; }
            else if (s.is(i, "}")) { --brace; if (paren == 0) stmt_start = i + 1; }
            else if (s.is(i, ";") && paren == 0) stmt_start = i + 1;
        }
        for (size_t i = L.body_open + 1; i < L.body_close; ++i) {
            if (depth_of[i] != 0 || start_of[i] != i || s[i].kind != Token::Ident || !s.is(i + 1, "=")) continue;
            const std::string X = s[i].text;
            size_t semi = i + 2;
            int p = 0, x_in_rhs = 0;
            bool ok = true;
            for (; semi < L.body_close && !(s.is(semi, ";") && p == 0); ++semi) {
                const Token& t = s[semi];
                if (s.is(semi, "(")) ++p;
                else if (s.is(semi, ")")) --p;
                else if (s.is(semi, ",") || s.is(semi, "*")) {}
                else if (t.kind == Token::Ident && t.text == X) ++x_in_rhs;
                else if (t.kind == Token::Ident && t.text == "transform" && s.is(semi + 1, "(")) {}
                else if (t.kind == Token::Ident && looks_like_a_uniform(t.text) && !written.count(t.text) && !(semi > 0 && s.is(semi - 1, "."))) {}
                else ok = false;
            }
            if (!ok || x_in_rhs != 1 || semi >= L.body_close || p != 0) continue;
            // X elsewhere: not in the header, only in nested blocks of the body, never written, never a member name
            std::vector<size_t> uses;
            for (size_t j = L.header_open; j <= L.header_close && ok; ++j) ok = !(s[j].kind == Token::Ident && s[j].text == X);
            for (size_t j = L.body_open + 1; j < L.body_close && ok; ++j) {
                if (j >= i && j <= semi) continue;
                if (s[j].kind != Token::Ident || s[j].text != X) continue;
                if (j > 0 && s.is(j - 1, ".")) { ok = false; break; }
                bool target = is_assignment_op(s[j + 1]) || s.is(j - 1, "++") || s.is(j - 1, "--");
                if (depth_of[j] < 1 || target) { ok = false; break; }
                if (s.ident(start_of[j], "else") || s.ident(start_of[j], "case") || s.ident(start_of[j], "default")) { ok = false; break; }
                uses.push_back(start_of[j]);
            }
            if (!ok || uses.empty()) continue;
            // X must be a LOCAL of this function, declared before the loop: an `out` / `inout` parameter or a global would have to carry
            // its final value out of the function, which a deferred update does not guarantee
            bool local = false;
            for (size_t j = fn_begin + 1; j + 1 < L.kw && !local; ++j)
                local = s[j].kind == Token::Ident && s[j].text == X && s[j - 1].kind == Token::Ident && (s.is(j + 1, "=") || s.is(j + 1, ";") || s.is(j + 1, ","));
            if (!local) continue;
            bool used_after = false;
            for (size_t j = L.body_close + 1; j < fn_end; ++j) used_after = used_after || (s[j].kind == Token::Ident && s[j].text == X);
            // the update statement as text, the counter, the flush
            std::string update;
            for (size_t j = i; j <= semi; ++j) update += s[j].text + (j < semi && s[j].kind == Token::Ident && s[j + 1].kind == Token::Ident ? " " : "");
            const std::string pend = "ptl_pend_" + std::to_string(counter++);
            const std::string flush = "for (; " + pend + " > 0; --" + pend + ") " + update + " ";
            edits.before(s, L.kw, "int " + pend + " = 0; ");
            edits.before(s, i, "++" + pend + ";");
            edits.drop(s, i, semi);
            std::sort(uses.begin(), uses.end());
            uses.erase(std::unique(uses.begin(), uses.end()), uses.end());
            for (size_t u : uses) edits.before(s, u, flush);
            if (used_after) edits.before(s, L.body_close + 1, flush);
            i = semi;
        }
    }
    if (!edits.empty()) toks = edits.tokens();
}

// `a / b` -> `ptl_div(a, b)`, `a /= b` -> `ptl_div_assign(a, b)` (device/ptl_glsl.h, "CONTRACT 2"): C++ cannot overload the division
// of two scalars, and the numerics contract defines it (a * (1/b) with the contract's reciprocal), so every division of a snippet
// becomes a call; the overload set of ptl_div keeps int / int an integer division and sends vector operands to the vector operators.
// Operand extents follow GLSL's grammar: the right operand is ONE unary expression (prefix operators, a primary, its postfix chain),
// the left operand the whole multiplicative chain in front (`a * b / c` is `(a * b) / c`; `*`, `/`, `%` associate to the left --
// earlier divisions of the chain have already been rewritten when a later one is reached, so their text is part of that operand).
// `x.yz /= e` (a multi-component swizzle as target) stays: the swizzle proxy's own operator/= does the same arithmetic.
void rewrite_divisions(std::vector<Token>& toks) {
    const TokenView s(toks);  // the edits are collected and applied once the scan is over: the view never sees a changed stream
    const size_t n = s.n();
    auto operand_end = [&](size_t i) {  // can a (sub)expression end with this token?
        if (i >= n) return false;
        const Token& t = s[i];
        if (t.kind == Token::Ident) {
            static const std::set<std::string> kw = {"return", "if", "else", "for", "while", "do", "case", "in", "out", "inout", "const"};
            return kw.count(t.text) == 0;
        }
        if (t.kind == Token::Number) return true;
        return t.kind == Token::Punct && (t.text == ")" || t.text == "]");
    };
    auto is_prefix_op = [&](size_t i) {  // a unary operator: one of - + ! ~ ++ -- that does not follow an operand
        if (i >= n || s[i].kind != Token::Punct) return false;
        const std::string& t = s[i].text;
        if (!(t == "-" || t == "+" || t == "!" || t == "~" || t == "++" || t == "--")) return false;
        return i == 0 || !operand_end(i - 1);
    };
    // start of the unary expression that ends at `e` (inclusive); n when the text is not understood
    auto unary_start = [&](size_t e) -> size_t {
        size_t p = e;
        if ((s.is(p, "++") || s.is(p, "--")) && p > 0 && operand_end(p - 1)) --p;  // postfix increment
        for (;;) {
            if (p >= n) return n;
            const Token& t = s[p];
            if (t.kind == Token::Punct && (t.text == ")" || t.text == "]")) {
                const size_t o = s.open_of(p);
                if (o == n) return n;
                if (t.text == "]") {  // base[...]: go on with the base
                    if (o == 0) return n;
                    p = o - 1;
                    continue;
                }
                p = o;
                if (o > 0 && s[o - 1].kind == Token::Ident && operand_end(o - 1)) p = o - 1;  // a call or a constructor
                else break;  // a parenthesised expression
            } else if (t.kind != Token::Ident && t.kind != Token::Number) {
                return n;
            }
            if (p > 0 && s.is(p - 1, ".")) {  // member of something: go on with the object
                if (p < 2) return n;
                p -= 2;
                continue;
            }
            break;
        }
        while (p > 0 && is_prefix_op(p - 1)) --p;
        return p;
    };
    // end (inclusive) of the unary expression that starts at `b`
    auto unary_end = [&](size_t b) -> size_t {
        size_t p = b;
        while (is_prefix_op(p)) ++p;
        if (p >= n) return n;
        if (s.is(p, "(")) {
            p = s.close_of(p);
            if (p == n) return n;
        } else if (s[p].kind != Token::Ident && s[p].kind != Token::Number) {
            return n;
        }
        for (;;) {  // postfix chain
            if (s.is(p + 1, "(") || s.is(p + 1, "[")) {
                p = s.close_of(p + 1);
                if (p == n) return n;
            } else if (s.is(p + 1, ".") && p + 2 < n && s[p + 2].kind == Token::Ident) {
                p += 2;
            } else if ((s.is(p + 1, "++") || s.is(p + 1, "--"))) {
                p += 1;
            } else {
                return p;
            }
        }
    };
    TokenEdits edits(toks);
    // `)` belongs right behind the last token of its operand, in front of the white space and comments that follow it -- only where that
    // token is the last of the text it goes behind those as well
    auto close_behind = [&](size_t last) { last + 1 < n ? edits.behind(s.raw(last), ")") : edits.before(s, n, ")"); };
    for (size_t k = 0; k < n; ++k) {
        auto fail = [&](const char* what) {
            std::string near;
            for (size_t i = k > 4 ? k - 4 : 0; i < n && i < k + 5; ++i) near += s[i].text + " ";
            throw std::runtime_error(std::string("GLSL -> HIP translation: cannot find the ") + what + " operand of the division near `" + near + "`");
        };
        auto ends_operand = [&](size_t i) { return operand_end(i) || ((s.is(i, "++") || s.is(i, "--")) && i > 0 && operand_end(i - 1)); };
        if (s.is(k, "/")) {
            if (k == 0 || !ends_operand(k - 1)) fail("left");
            size_t left = unary_start(k - 1);
            if (left == n) fail("left");
            while (left > 1 && (s.is(left - 1, "*") || s.is(left - 1, "/") || s.is(left - 1, "%")) && operand_end(left - 2)) {
                const size_t prev = unary_start(left - 2);
                if (prev == n) break;
                left = prev;
            }
            const size_t right = unary_end(k + 1);
            if (right == n) fail("right");
            edits.before(s, left, "ptl_div(");
            edits.replace(s.raw(k), ",");
            close_behind(right);
        } else if (s.is(k, "/=")) {
            if (k == 0 || !operand_end(k - 1)) fail("left");
            if (s[k - 1].kind == Token::Ident && k >= 2 && s.is(k - 2, ".") && !swizzle_indices(s[k - 1].text).empty()) continue;  // v.xy /= e
            const size_t left = unary_start(k - 1);
            if (left == n) fail("left");
            size_t end = k + 1;  // the assignment expression: up to the `;`, `,` or closing bracket of this nesting level
            int depth = 0;
            for (; end < n; ++end) {
                if (s.is(end, "(") || s.is(end, "[")) ++depth;
                else if (s.is(end, ")") || s.is(end, "]")) {
                    if (depth == 0) break;
                    --depth;
                } else if (depth == 0 && (s.is(end, ";") || s.is(end, ","))) break;
            }
            if (end == k + 1) fail("right");
            edits.before(s, left, "ptl_div_assign(");
            edits.replace(s.raw(k), ",");
            close_behind(end - 1);
        }
    }
    if (!edits.empty()) toks = edits.tokens();
}

}  // namespace

std::string translate_glsl(const std::string& glsl, bool defer_loop_updates, bool force_inline_definitions) {
    std::vector<Token> toks = tokenize_glsl(glsl);
    if (defer_loop_updates) defer_loop_carried_updates(toks);  // (each pass builds its own view: the one before it has changed the stream)
    rewrite_divisions(toks);
    // The return types (by index in the stream) of the function definitions of a file-scope text.  A `#define` head keeps what follows it on
    // its line from being one: that is a macro's replacement text, not a function of the kernel.
    std::set<size_t> heads;
    if (force_inline_definitions) {
        const TokenView s(toks, TokenView::kLayout);
        auto follows_define = [&](size_t k) {
            while (k-- > 0 && !(toks[k].kind == Token::Space && toks[k].text.find('\n') != std::string::npos))
                if (toks[k].kind == Token::Preproc) return true;
            return false;
        };
        for (const FunctionSpan& fn : function_definitions(s))
            if (!follows_define(s.raw(fn.type_at))) heads.insert(s.raw(fn.type_at));
    }
    std::string out;
    out.reserve(glsl.size() + glsl.size() / 8);

    // the code token in front of / behind toks[k] on the stream (the emitter below walks every token of it), or nullptr
    auto prev_sig = [&](size_t k) { const size_t p = prev_code(toks, k); return p < toks.size() ? &toks[p] : nullptr; };
    auto next_sig = [&](size_t k) { const size_t p = next_code(toks, k + 1); return p < toks.size() ? &toks[p] : nullptr; };

    // The translation works on tokens, not on types: `.xy` after ANY expression becomes a swizzle call.  A user struct with a field
    // that spells a swizzle (`struct S { vec2 st; }` ... `s.st`) would silently turn into s.sw<0,1>(): refuse it with a message
    // that names the field instead of leaving the scene author with a hiprtc error (or none).  The reference's corpus has no such field.
    {
        int brace = 0, struct_brace = -1;
        bool struct_head = false;
        for (size_t k = 0; k < toks.size(); ++k) {
            const Token& t = toks[k];
            if (t.kind == Token::Ident && t.text == "struct") struct_head = true;
            if (t.kind != Token::Punct && t.kind != Token::Ident) continue;
            if (t.kind == Token::Punct && t.text == "{") {
                ++brace;
                if (struct_head) {
                    struct_brace = brace;
                    struct_head = false;
                }
            } else if (t.kind == Token::Punct && t.text == "}") {
                if (brace == struct_brace) struct_brace = -1;
                --brace;
            } else if (t.kind == Token::Punct && t.text == ";") {
                struct_head = false;  // `struct S;` or a variable of struct type: no body
            } else if (t.kind == Token::Ident && struct_brace == brace && brace > 0) {
                const Token* nx = next_sig(k);
                if (nx && nx->kind == Token::Punct && (nx->text == ";" || nx->text == "," || nx->text == "[") && !swizzle_indices(t.text).empty())
                    throw std::runtime_error("struct field `" + t.text + "` spells a vector swizzle (xyzw / rgba / stpq): the GLSL -> HIP translation "
                                             "cannot tell `value." + t.text + "` from a swizzle; rename the field");
            }
        }
    }

    int paren_depth = 0;
    bool pending_ref = false;  // an `out` / `inout` qualifier was seen: next type name gets `&`
    for (size_t k = 0; k < toks.size(); ++k) {
        const Token& t = toks[k];
        switch (t.kind) {
            case Token::Space:
            case Token::Comment:
            case Token::Preproc:
            case Token::Raw:
                out += t.text;
                break;
            case Token::Number: {
                std::string s = t.text;
                if (is_float_literal(s)) {
                    char last = s.back();
                    if (last == 'F') s.back() = 'f';
                    else if (last != 'f') s += 'f';
                }
                out += s;
                break;
            }
            case Token::Punct:
                if (t.text == "(") ++paren_depth;
                if (t.text == ")") --paren_depth;
                out += t.text;
                break;
            case Token::Ident: {
                if (heads.count(k)) out += "PTL_FN ";  // on the line of the definition: the scene's line numbers stay what they are
                const Token* p = prev_sig(k);
                const Token* nx = next_sig(k);
                bool after_dot = p && p->kind == Token::Punct && p->text == ".";
                if (after_dot) {
                    std::vector<int> idx = swizzle_indices(t.text);
                    if (!idx.empty()) {
                        bool lvalue = nx && nx->kind == Token::Punct &&
                                      (nx->text == "=" || nx->text == "+=" || nx->text == "-=" || nx->text == "*=" || nx->text == "/=");
                        out += lvalue ? "swr<" : "sw<";
                        for (size_t c = 0; c < idx.size(); ++c) {
                            if (c) out += ',';
                            out += std::to_string(idx[c]);
                        }
                        out += ">()";
                        break;
                    }
                    out += t.text;  // ordinary member (or single component)
                    break;
                }
                // parameter qualifiers: only meaningful right after `(` or `,` inside parentheses
                bool param_pos = paren_depth > 0 && p && ((p->kind == Token::Punct && (p->text == "(" || p->text == ",")) ||
                                                          (p->kind == Token::Ident && p->text == "const"));  // `const in vec3 v`
                bool next_is_type = nx && nx->kind == Token::Ident;
                if (param_pos && next_is_type && (t.text == "in" || t.text == "out" || t.text == "inout")) {
                    if (t.text != "in") pending_ref = true;
                    break;  // drop the qualifier
                }
                if (t.text == "highp" || t.text == "mediump" || t.text == "lowp") break;
                if (cpp_only_keywords().count(t.text)) {
                    out += t.text + "_";
                    break;
                }
                out += t.text;
                if (pending_ref && next_is_type) {  // this identifier is the parameter's type
                    out += "&";
                    pending_ref = false;
                }
                break;
            }
        }
    }
    return out;
}

}  // namespace ptl
