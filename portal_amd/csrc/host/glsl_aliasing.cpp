// glsl_aliasing.cpp -- check_out_argument_aliasing (glsl_translate.h): the one thing about a scene's GLSL that is refused, not translated.
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "glsl_syntax.h"
#include "glsl_tokens.h"
#include "glsl_translate.h"

namespace ptl {

// GLSL passes `out` / `inout` arguments by value-result: copied in at the call, copied out at the return (GLSL ES 3.00 section 6.1.1).
// The translation passes C++ references.  The two agree unless the callee can reach the argument under another name while it runs:
//   (a) the argument is a mutable global that the callee (or something it calls) also names -- GLSL keeps the global's old value
//       until the return, a reference changes it at once;
//   (b) the same variable is given to two out / inout parameters of one call -- GLSL leaves the order of the copies back undefined, so
//       the reference's picture would depend on its GL driver.
// Neither occurs in the reference's scenes (tests/test_host_logic.py runs the corpus through this).  A scene that does either is
// refused here instead of silently drawing something the reference might not: VERDICT r2 "semantic gaps" #8.
void check_out_argument_aliasing(const std::vector<std::string>& sources, const std::vector<std::string>& bodies) {
    struct Function {
        std::vector<char> out;          // per parameter: out / inout?
        std::set<std::string> names;    // identifiers of the body
        std::set<std::string> calls;
    };
    static const std::set<std::string> not_a_type = {"return", "if", "else", "for", "while", "do", "switch", "case", "in", "out", "inout", "const", "uniform", "struct", "break", "continue", "discard"};
    std::multimap<std::string, Function> functions;
    std::set<std::string> globals;
    std::vector<std::vector<Token>> streams;
    for (const std::string& text : sources) streams.push_back(tokenize_glsl(text));
    for (const std::string& text : bodies) streams.push_back(tokenize_glsl(text));  // statements of a generated function: calls, no definitions
    const std::vector<TokenView> views(streams.begin(), streams.end());  // (built once every stream stands where it stays)
    std::vector<std::set<size_t>> definitions(streams.size());         // positions (in the views) of function names at their definition
    // pass 1: what is defined at file scope
    for (size_t f = 0; f < sources.size(); ++f) {
        const TokenView& s = views[f];
        std::map<size_t, FunctionSpan> defined;  // by the position of the return type
        for (const FunctionSpan& fn : function_definitions(s)) defined.emplace(fn.type_at, fn);
        for (size_t k = 0; k < s.n();) {
            if (s.is(k, "{")) {  // a struct body (or anything else braced at file scope)
                k = s.close_of(k) + 1;
                continue;
            }
            bool decl = s[k].kind == Token::Ident && !not_a_type.count(s[k].text) && k + 2 < s.n() && s[k + 1].kind == Token::Ident && s[k + 2].kind == Token::Punct;
            if (!decl) {
                ++k;
                continue;
            }
            bool qualified = false;  // `const float x`, `uniform ...`: nothing a function could write
            for (size_t b = k; b-- > 0;) {
                if (s[b].kind == Token::Punct && (s[b].text == ";" || s[b].text == "}")) break;
                if (s[b].kind == Token::Ident && (s[b].text == "const" || s[b].text == "uniform" || s[b].text == "in")) qualified = true;
            }
            const std::string& name = s[k + 1].text;
            const std::string& after = s[k + 2].text;
            if (after == "(") {
                const auto def = defined.find(k);
                if (def == defined.end()) {  // a prototype
                    k = s.close_of(k + 2) + 1;
                    continue;
                }
                const FunctionSpan& span = def->second;
                Function fn;
                const bool only_void = span.params.size() == 1 && span.params[0].e == span.params[0].b + 1 && s[span.params[0].b].text == "void";
                for (const FunctionSpan::Param& p : span.params)
                    if (!only_void) fn.out.push_back(p.out);
                for (size_t a = span.body_b; a < span.body_e; ++a)
                    if (s[a].kind == Token::Ident) {
                        fn.names.insert(s[a].text);
                        if (a + 1 < span.body_e && s.is(a + 1, "(")) fn.calls.insert(s[a].text);
                    }
                definitions[f].insert(span.name_at);
                functions.emplace(name, std::move(fn));
                k = span.body_e + 1;
                continue;
            }
            if (!qualified && (after == ";" || after == "=" || after == "[" || after == ",")) {
                // `float a, b = 1.0, c;` : every declarator up to the `;`
                globals.insert(name);
                int depth = 0;
                size_t a = k + 2;
                for (; a < s.n(); ++a) {
                    const Token& t = s[a];
                    if (t.kind != Token::Punct) continue;
                    if (t.text == "(" || t.text == "[" || t.text == "{") ++depth;
                    else if (t.text == ")" || t.text == "]" || t.text == "}") --depth;
                    else if (t.text == ";" && depth == 0) break;
                    else if (t.text == "," && depth == 0 && a + 1 < s.n() && s[a + 1].kind == Token::Ident) globals.insert(s[a + 1].text);
                }
                k = a + 1;
                continue;
            }
            ++k;
        }
    }
    bool any_out = false;
    for (auto& [name, fn] : functions)
        for (char o : fn.out) any_out = any_out || o;
    if (!any_out) return;
    // which mutable globals can a call of `name` touch (through anything it calls)
    auto reach = [&](const std::string& name) {
        std::set<std::string> seen_fn, found;
        std::vector<std::string> todo = {name};
        while (!todo.empty()) {
            std::string cur = todo.back();
            todo.pop_back();
            if (!seen_fn.insert(cur).second) continue;
            auto range = functions.equal_range(cur);
            for (auto it = range.first; it != range.second; ++it) {
                for (const std::string& g : globals)
                    if (it->second.names.count(g)) found.insert(g);
                for (const std::string& c : it->second.calls) todo.push_back(c);
            }
        }
        return found;
    };
    // may two lvalues name the same storage?  `v.x` / `v.y` and `s.a` / `s.b` do not; `v` / `v.x`, `v.xy` / `v.yz`, anything indexed may
    auto overlap = [](const std::string& a, const std::string& b) {
        if (a == b) return true;
        if (a.find('[') != std::string::npos || b.find('[') != std::string::npos) return true;
        auto parts = [](const std::string& t) {
            std::vector<std::string> out(1);
            for (char c : t)
                if (c == '.') out.emplace_back();
                else out.back() += c;
            return out;
        };
        std::vector<std::string> pa = parts(a), pb = parts(b);
        for (size_t c = 0;; ++c) {
            if (c == pa.size() || c == pb.size()) return true;  // one is the whole of which the other is a part
            if (pa[c] == pb[c]) continue;
            std::vector<int> ia = swizzle_indices(pa[c]), ib = swizzle_indices(pb[c]);
            if (ia.empty() || ib.empty()) return false;         // two different fields
            for (int x : ia)
                for (int y : ib)
                    if (x == y) return true;
            return false;
        }
    };
    // pass 2: every call of a function with out / inout parameters
    for (size_t f = 0; f < streams.size(); ++f) {
        const TokenView& s = views[f];
        for (size_t k = 0; k + 1 < s.n(); ++k) {
            if (s[k].kind != Token::Ident || !functions.count(s[k].text) || definitions[f].count(k)) continue;
            if (!(s.is(k + 1, "("))) continue;
            if (k > 0 && s.is(k - 1, ".")) continue;
            const size_t close = s.close_of(k + 1);
            std::vector<std::string> roots, whole;  // first identifier of every argument; the argument without white space
            if (close > k + 2)
                for (const auto& [b, e] : s.split_top_level(k + 2, close, ",")) {
                    std::string root, text;
                    for (size_t a = b; a < e; ++a) {
                        text += s[a].text;
                        if (root.empty() && s[a].kind == Token::Ident) root = s[a].text;
                    }
                    roots.push_back(root);
                    whole.push_back(text);
                }
            auto range = functions.equal_range(s[k].text);
            for (auto it = range.first; it != range.second; ++it) {
                const Function& fn = it->second;
                if (fn.out.size() != roots.size()) continue;
                std::set<std::string> touched;
                bool computed = false;
                for (size_t j = 0; j < roots.size(); ++j) {
                    if (!fn.out[j] || roots[j].empty()) continue;
                    for (size_t j2 = j + 1; j2 < roots.size(); ++j2)
                        if (fn.out[j2] && roots[j2] == roots[j] && overlap(whole[j], whole[j2]))
                            throw std::runtime_error("`" + s[k].text + "(...)`: `" + roots[j] + "` is given to two out / inout parameters of one call; GLSL leaves the order "
                                                     "in which they are copied back undefined, so the picture would depend on the GL driver");
                    if (!globals.count(roots[j])) continue;
                    if (!computed) {
                        touched = reach(s[k].text);
                        computed = true;
                    }
                    if (touched.count(roots[j]))
                        throw std::runtime_error("`" + s[k].text + "(...)`: the global `" + roots[j] + "` is an out / inout argument of a function that also names it; "
                                                 "GLSL copies the argument back at the return, this translation passes a reference -- the two would differ.  Pass a local "
                                                 "and assign it afterwards");
                }
            }
        }
    }
}

}  // namespace ptl
