// glsl_tokens.h -- the lexer, the token view and the token edit list shared by every pass over the GLSL snippets of a scene: the GLSL -> C++
// rewrite (glsl_translate.cpp), the out-argument check (glsl_aliasing.cpp), the distance bound (glsl_bound.cpp), the uniform-work hoister
// (glsl_syntax.cpp, glsl_hoist.cpp), the affine-rays scan (glsl_affine.cpp), the masked forms and unroll pragmas of a build (glsl_masks.cpp) and
// the generator's "does it name X" questions (codegen.cpp).  A pass reads through a TokenView and writes through a TokenEdits.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <map>
#include <set>
#include <string>
#include <utility>
#include <vector>

namespace ptl {

struct Token {
    enum Kind { Space, Comment, Ident, Number, Punct, Preproc, Raw } kind;  // Raw: text inserted by a rewrite, emitted verbatim
    std::string text;
};

// Every character of the input ends up in exactly one token (concatenating the texts gives the input back).
std::vector<Token> tokenize_glsl(const std::string& s);

// `= += -= *= /= ++ --`: the operators the lexer knows that write their operand.
bool is_assignment_op(const Token& t);

// Does a Number token spell a float (never a hexadecimal one)?  The two passes that ask disagree on digits with a bare suffix, `1f`:
//   is_float_literal        a point or an exponent (the translator: what gets an `f` appended; `1f` is left for the compiler to refuse);
//   is_float_typed_literal  ... or an `f` / `F` suffix (the hoister: the type it gives the literal; `1f` is a float there).
bool is_float_literal(const std::string& number);
bool is_float_typed_literal(const std::string& number);

// `.xyzw` / `.rgba` / `.stpq` selectors -> component indices, all letters from one set; empty if `name` is none.
//   component_indices   one to four components (the hoister: `v.x` selects like `v.xy` does);
//   swizzle_indices     two to four (the translator: a single component is an ordinary member of the C++ vector, only more become a swizzle call).
std::vector<int> component_indices(const std::string& name);
std::vector<int> swizzle_indices(const std::string& name);

// Is one of `names` an identifier of `glsl` (not part of a comment, a directive or a longer name)?
bool names_identifier(const std::string& glsl, std::initializer_list<const char*> names);

// The names of the functions a GLSL text defines (`type name(` outside all braces), and of those it defines with an `out` / `inout`
// parameter (the qualifier in front of a type; the name in front of the `(` that opens its list).  Comments and directives are not code.
// A looser question than glsl_syntax.h's function_definitions answers: a prototype counts as well, and the names are all there is.
void defined_functions(const std::string& glsl, std::set<std::string>& names);
void functions_with_out_params(const std::string& glsl, std::set<std::string>& names);

constexpr unsigned token_kinds(std::initializer_list<Token::Kind> kinds) {  // a set of kinds, for TokenView to drop
    unsigned bits = 0;
    for (Token::Kind k : kinds) bits |= 1u << k;
    return bits;
}

// The tokens of a stream that a pass looks at, by position: white space, comments and (by default) directives are stepped over.  Holds
// indices into the stream, no tokens: the stream must outlive the view, and a view built before tokens were inserted or removed is stale.
// Every predicate takes any index: at or past n() it is false, never a read.
class TokenView {
  public:
    static constexpr unsigned kLayout = token_kinds({Token::Space, Token::Comment});  // what the hoister drops: it bails out on a directive it sees
    static constexpr unsigned kLayoutAndDirectives = token_kinds({Token::Space, Token::Comment, Token::Preproc});

    explicit TokenView(const std::vector<Token>& stream, unsigned dropped_kinds = kLayoutAndDirectives);

    size_t n() const { return at_.size(); }
    const Token& operator[](size_t i) const { return (*stream_)[at_[i]]; }
    size_t raw(size_t i) const { return at_[i]; }  // index in the stream (where a rewrite inserts or replaces)

    bool is(size_t i, const char* punct) const { return i < n() && (*this)[i].kind == Token::Punct && (*this)[i].text == punct; }
    bool ident(size_t i) const { return i < n() && (*this)[i].kind == Token::Ident; }
    bool ident(size_t i, const std::string& text) const { return ident(i) && (*this)[i].text == text; }
    bool number(size_t i) const { return i < n() && (*this)[i].kind == Token::Number; }
    // do the tokens from i on spell `words`, one each (by text alone: identifiers and punctuation as given)?
    bool spells(size_t i, const std::vector<std::string>& words) const;

    // The bracket matching the one at `open` / `close` -- `(`, `[` or `{`, as the token itself says; only its own kind is counted -- or n().
    size_t close_of(size_t open) const;
    size_t open_of(size_t close) const;

    // source text of [b, e) on one line: every comment and every run of white space between the two ends is one space each
    std::string text_of(size_t b, size_t e) const;
    // [from, to) cut at every `separator` that stands outside all brackets opened in the range (always at least one part)
    std::vector<std::pair<size_t, size_t>> split_top_level(size_t from, size_t to, const char* separator) const;

  private:
    const std::vector<Token>* stream_;
    std::vector<size_t> at_;
};

// What one pass changes in one stream: text in front of a token, behind it, in its place, and tokens dropped.  Recorded by index in the
// stream while the pass reads the tokens as written, applied once by text() / tokens(); the stream itself is never touched, and nothing
// is tokenised again.  Where several texts meet in one slot between two tokens they come out in this order: what stands behind token k,
// then what stands in front of token k + 1, each in the order it was recorded -- so text put in front of a token that is also replaced
// or dropped stands in front of the replacement.  Inserted text comes out whether or not the token it is tied to is dropped.
class TokenEdits {
  public:
    explicit TokenEdits(const std::vector<Token>& stream) : stream_(&stream) {}

    void before(size_t k, const std::string& text) { inserts_.push_back({2 * std::min(k, stream_->size()), text}); }  // k at or past the size: the end
    void behind(size_t k, const std::string& text) { inserts_.push_back({2 * k + 1, text}); }
    void replace(size_t k, const std::string& text) { replaced_[k] = text; }  // the token keeps its kind; replaced by "" it is gone
    void drop(size_t first, size_t last);  // [first, last] go, but for the line breaks among them (the text keeps its lines) and for what replace() names
    // ... by significant-token index of a view of the same stream; at or past s.n() is the end of the stream
    void before(const TokenView& s, size_t i, const std::string& text) { before(i < s.n() ? s.raw(i) : stream_->size(), text); }
    void drop(const TokenView& s, size_t first, size_t last) { drop(s.raw(first), s.raw(last)); }

    bool empty() const { return inserts_.empty() && replaced_.empty(); }
    std::vector<Token> tokens() const;  // every inserted text a Token::Raw of its own: a significant token for the pass that comes next
    std::string text() const;

  private:
    const std::vector<Token>* stream_;
    std::vector<std::pair<size_t, std::string>> inserts_;  // (slot, text): slot 2k in front of token k, 2k + 1 behind it
    std::map<size_t, std::string> replaced_;  // (a dropped token: replaced by "")
};

// For the walks that emit every token of a stream and so stay on it: the first index at or after k / the last one before k whose token is code
// (neither white space nor a comment), or stream.size().
size_t next_code(const std::vector<Token>& stream, size_t k);
size_t prev_code(const std::vector<Token>& stream, size_t k);

}  // namespace ptl
