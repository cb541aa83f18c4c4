// glsl_masks.cpp -- specialize_translated (glsl_translate.h): what the values a build compiles in do to a translated snippet.
#include <map>
#include <set>
#include <string>
#include <vector>

#include "glsl_tokens.h"
#include "glsl_translate.h"

namespace ptl {

std::string masked_callee(const std::string& callee, const std::string& matrix) {
    return (callee == "transform" ? "ptl_transform_m" : callee) + "<PTL_MASK_" + matrix + ">";
}

namespace {

constexpr int kUnrollLimit = 16;

bool blank(const Token& t) { return t.kind == Token::Space && t.text != "\n"; }

// The right operand of a product, from its first token q to its last (returned; s.n(): none that is rewritten).  One unary expression: a
// parenthesised group, or a name with its call / index / member suffixes -- never one that starts with a sign or a digit.
size_t operand_end(const TokenView& s, size_t q) {
    if (s.is(q, "(")) return s.close_of(q);
    if (!s.ident(q)) return s.n();
    for (size_t end = q;;) {
        if (s.is(end + 1, "(") || s.is(end + 1, "[")) {
            end = s.close_of(end + 1);
        } else if (s.is(end + 1, ".") && s.ident(end + 2)) {
            end += 2;
            if ((s[end].text == "sw" || s[end].text == "swr") && s.is(end + 1, "<"))  // a translated swizzle, .sw<0,1,2>(): up to its `>`, the call is the next suffix
                while (end < s.n() && !s.is(end, ">")) ++end;
        } else if (s.is(end + 1, "-") && s.is(end + 2, ">") && s.raw(end + 2) == s.raw(end + 1) + 1 && s.ident(end + 3)) {
            end += 3;  // (the generated prologue: `X_mat_inv * out->ptl_dv_origin`)
        } else {
            return end;
        }
        if (end >= s.n()) return s.n();  // a bracket that is not closed
    }
}

// `for ( int I = 0 ; I < B ; I ++ ) {` at i, B a baked Int of 2 .. kUnrollLimit
bool counts_to_small_bound(const TokenView& s, size_t i, const std::map<std::string, int>& bounds) {
    if (!(s.spells(i, {"for", "(", "int"}) && s.ident(i + 3) && s.spells(i + 4, {"=", "0", ";"}) && s.is(i + 8, "<") && s.ident(i + 9) && s.is(i + 10, ";") &&
          s.spells(i + 12, {"++", ")", "{"})))
        return false;
    const std::string& counter = s[i + 3].text;
    const auto b = bounds.find(s[i + 9].text);
    return s.ident(i + 7, counter) && s.ident(i + 11, counter) && b != bounds.end() && b->second >= 2 && b->second <= kUnrollLimit;
}

}  // namespace

// See glsl_translate.h.  The walk reads the tokens as written (TokenEdits), so a product inside an operand is judged by its own neighbours.
std::string specialize_translated(const std::string& cxx, const std::set<std::string>& masked, const std::map<std::string, int>& unroll_bounds, int* unrolled) {
    if (unrolled) *unrolled = 0;
    if (masked.empty() && unroll_bounds.empty()) return cxx;
    const std::vector<Token> toks = tokenize_glsl(cxx);
    const TokenView s(toks);
    TokenEdits edits(toks);
    for (size_t i = 0; i < s.n(); ++i) {
        if (!s.ident(i) || s.is(i - 1, ".")) continue;  // (a member is never the uniform)
        const std::string& word = s[i].text;
        if (word == "for" && counts_to_small_bound(s, i, unroll_bounds)) {
            edits.before(s, i, "_Pragma(\"unroll\") ");
            if (unrolled) ++*unrolled;
        } else if (word == "transform" && s.is(i + 1, "(") && s.ident(i + 2) && masked.count(s[i + 2].text) && s.is(i + 3, ",")) {
            edits.replace(s.raw(i), masked_callee(word, s[i + 2].text));
        } else if (masked.count(word) && s.is(i + 1, "*")) {
            // `word` must be the whole left operand: nothing multiplicative in front of it, and no unary sign (which binds tighter than the
            // product: (-M) * v stays).  A sign is binary behind a name, a literal, `)` or `]`.
            if (s.is(i - 1, "*") || s.is(i - 1, "/") || s.is(i - 1, "%") || s.is(i - 1, "++") || s.is(i - 1, "--")) continue;
            if ((s.is(i - 1, "-") || s.is(i - 1, "+")) && !(s.ident(i - 2) || s.number(i - 2) || s.is(i - 2, ")") || s.is(i - 2, "]"))) continue;
            const size_t end = operand_end(s, i + 2);
            if (end == s.n()) continue;
            // M * v -> ptl_mul_m<PTL_MASK_M>(M, v): the blanks around `*` go, comments and line breaks stay where they are
            const size_t star = s.raw(i + 1);
            edits.before(s, i, masked_callee("ptl_mul_m", word) + "(");
            for (size_t k = s.raw(i) + 1; k < star; ++k)
                if (blank(toks[k])) edits.replace(k, "");
            size_t next = star + 1;
            if (blank(toks[next])) edits.replace(next++, "");
            edits.replace(star, toks[next].text == "\n" ? "," : ", ");
            edits.behind(s.raw(end), ")");
        }
    }
    return edits.text();
}

}  // namespace ptl
