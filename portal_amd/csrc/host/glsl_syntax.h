// glsl_syntax.h -- the shape of a GLSL function body, as far as the uniform-work hoister (glsl_hoist.h) needs it: expressions as trees,
// the statements around them as a list of sites, `for` / `while` loops with what makes one canonical.  Nothing here knows what a
// uniform is (glsl_binding.h decides that) and nothing rewrites a token (glsl_hoist.cpp does).
#pragma once
#include <string>
#include <vector>

#include "glsl_tokens.h"

namespace ptl {

struct Node {
    enum Kind { Lit, Ident, Paren, Unary, Binary, Ternary, Assign, Call, Member, Index, Post } kind = Lit;
    size_t b = 0, e = 0;  // significant-token span [b, e)
    std::vector<int> kids;
    std::string text;  // operator, identifier, function or member name
};

struct Site {  // one parsed expression and where it stands
    enum Kind { Expr, DeclInit, Decl } kind = Expr;
    int root = -1;
    int depth = 0;        // blocks / controlled statements around it inside the function body
    int loop = 0;         // innermost loop it is in (its header included), 0 = none
    bool header = false;  // part of a loop header
    size_t stmt_b = 0, stmt_e = 0;  // for expression statements: the whole statement with its `;`
    std::string decl_type, decl_name;
    size_t name_at = 0;   // Decl / DeclInit: significant-token index of the declared name
};

struct LoopInfo {
    int id = 0, outer = 0, depth = 0;
    size_t kw = 0, header_open = 0, header_close = 0, body_b = 0, body_e = 0;  // body_b/e: first token of the body, one past its last
    bool canonical = false, has_continue = false, braced = false;  // canonical: `for (int I = 0; I < BOUND; I++)`, token for token
    std::string var, bound;
};

struct ParsedBody {
    bool ok = false;  // false: something in the body is not understood (do / switch / struct / arrays / a method call / a stray token ...)
    std::vector<Node> nodes;
    std::vector<Site> sites;      // in source order; the names the body declares are those of its Decl / DeclInit sites, in that order
    std::vector<LoopInfo> loops;  // loop `id` is loops[id - 1]

    std::string base_identifier(int id) const;              // `v` of `v`, `v.x`, `v[i]`, `(v)`; "" for anything else
    bool mentions(int id, const std::string& name) const;   // does the expression name the variable?
};

// The statements of [b, e) -- a function's body without its braces.
ParsedBody parse_body(const TokenView& s, size_t b, size_t e);

// do the tokens of [b, e) name the variable (a member of that name after a `.` is not it)?
bool tokens_mention(const TokenView& s, size_t b, size_t e, const std::string& name);

struct FunctionSpan {
    struct Param {
        size_t b, e;       // its tokens [b, e)
        std::string name;  // the last identifier among them ("" if there is none; `void` of `f(void)` is one)
        bool out;          // `out` / `inout` stands among them
    };
    size_t type_at = 0, name_at = 0;  // return type and name
    std::vector<Param> params;        // the list between the parentheses, cut at its top-level commas; none for `()`
    size_t body_b = 0, body_e = 0;    // the tokens between its braces; body_e == s.n(): the body is never closed
    std::vector<std::string> param_names() const;  // of the parameters that have one
};
// The function definitions of a file-scope text: identifier, identifier, `( ... ) {` outside all braces.  That is all the scan asks: the
// word in front of the name may be `return` or `else`, what follows a `#define` on its line is code like any other, and the last
// definition may lack its `}` -- whoever minds looks at the span.
std::vector<FunctionSpan> function_definitions(const TokenView& s);

}  // namespace ptl
