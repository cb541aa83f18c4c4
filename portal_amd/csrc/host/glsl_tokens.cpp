// glsl_tokens.cpp -- see glsl_tokens.h.
#include "glsl_tokens.h"

#include <algorithm>
#include <cctype>
#include <cstring>

namespace ptl {

std::vector<Token> tokenize_glsl(const std::string& s) {
    std::vector<Token> out;
    size_t i = 0, n = s.size();
    bool line_start = true;
    while (i < n) {
        char c = s[i];
        if (c == '\n') {
            out.push_back({Token::Space, "\n"});
            ++i;
            line_start = true;
            continue;
        }
        if (c == ' ' || c == '\t' || c == '\r') {
            size_t j = i;
            while (j < n && (s[j] == ' ' || s[j] == '\t' || s[j] == '\r')) ++j;
            out.push_back({Token::Space, s.substr(i, j - i)});
            i = j;
            continue;
        }
        if (c == '#' && line_start) {  // preprocessor directive: keep the line verbatim ...
            size_t j = s.find('\n', i);
            if (j == std::string::npos) j = n;
            // ... except the replacement text of a `#define`, which is GLSL like any other: its float literals need their suffix and its
            // divisions are the contract's (rewrite_divisions), e.g. the reference's own `#define PI2 (acos(-1.) / 2.0)`.  The head
            // (`#define NAME` or `#define NAME(params)`) stays one verbatim token, the rest of the line is tokenised as code.
            size_t h = i + 1;
            while (h < j && (s[h] == ' ' || s[h] == '\t')) ++h;
            if (s.compare(h, 6, "define") == 0 && h + 6 < j && (s[h + 6] == ' ' || s[h + 6] == '\t') && s.find('\\', i) >= j) {
                h += 6;
                while (h < j && (s[h] == ' ' || s[h] == '\t')) ++h;
                while (h < j && (std::isalnum((unsigned char)s[h]) || s[h] == '_')) ++h;
                if (h < j && s[h] == '(') {  // function-like: the parameter list belongs to the head
                    size_t close = s.find(')', h);
                    h = (close == std::string::npos || close >= j) ? j : close + 1;
                }
                out.push_back({Token::Preproc, s.substr(i, h - i)});
                i = h;
                line_start = false;
                continue;
            }
            out.push_back({Token::Preproc, s.substr(i, j - i)});
            i = j;
            continue;
        }
        line_start = false;
        if (c == '/' && i + 1 < n && s[i + 1] == '/') {
            size_t j = s.find('\n', i);
            if (j == std::string::npos) j = n;
            out.push_back({Token::Comment, s.substr(i, j - i)});
            i = j;
            continue;
        }
        if (c == '/' && i + 1 < n && s[i + 1] == '*') {
            size_t j = s.find("*/", i + 2);
            j = j == std::string::npos ? n : j + 2;
            out.push_back({Token::Comment, s.substr(i, j - i)});
            i = j;
            continue;
        }
        if (std::isalpha((unsigned char)c) || c == '_') {
            size_t j = i;
            while (j < n && (std::isalnum((unsigned char)s[j]) || s[j] == '_')) ++j;
            out.push_back({Token::Ident, s.substr(i, j - i)});
            i = j;
            continue;
        }
        if (std::isdigit((unsigned char)c) || (c == '.' && i + 1 < n && std::isdigit((unsigned char)s[i + 1]))) {
            size_t j = i;
            if (c == '0' && j + 1 < n && (s[j + 1] == 'x' || s[j + 1] == 'X')) {
                j += 2;
                while (j < n && std::isxdigit((unsigned char)s[j])) ++j;
            } else {
                while (j < n && std::isdigit((unsigned char)s[j])) ++j;
                if (j < n && s[j] == '.') {
                    ++j;
                    while (j < n && std::isdigit((unsigned char)s[j])) ++j;
                }
                if (j < n && (s[j] == 'e' || s[j] == 'E')) {
                    size_t k = j + 1;
                    if (k < n && (s[k] == '+' || s[k] == '-')) ++k;
                    if (k < n && std::isdigit((unsigned char)s[k])) {
                        while (k < n && std::isdigit((unsigned char)s[k])) ++k;
                        j = k;
                    }
                }
            }
            while (j < n && (s[j] == 'f' || s[j] == 'F' || s[j] == 'u' || s[j] == 'U')) ++j;  // suffixes
            out.push_back({Token::Number, s.substr(i, j - i)});
            i = j;
            continue;
        }
        // two-character operators that matter for the lvalue-swizzle test
        static const char* two[] = {"==", "!=", "<=", ">=", "+=", "-=", "*=", "/=", "&&", "||", "++", "--", "<<", ">>"};
        bool matched = false;
        for (const char* t : two) {
            if (s.compare(i, 2, t) == 0) {
                out.push_back({Token::Punct, t});
                i += 2;
                matched = true;
                break;
            }
        }
        if (matched) continue;
        out.push_back({Token::Punct, std::string(1, c)});
        ++i;
    }
    return out;
}

bool is_assignment_op(const Token& t) {
    if (t.kind != Token::Punct) return false;
    return t.text == "=" || t.text == "+=" || t.text == "-=" || t.text == "*=" || t.text == "/=" || t.text == "++" || t.text == "--";
}

static bool float_spelling(const std::string& t, const char* marks) {
    if (t.size() > 1 && t[0] == '0' && (t[1] == 'x' || t[1] == 'X')) return false;
    return t.find_first_of(marks) != std::string::npos;
}
bool is_float_literal(const std::string& number) { return float_spelling(number, ".eE"); }
bool is_float_typed_literal(const std::string& number) { return float_spelling(number, ".eEfF"); }

std::vector<int> component_indices(const std::string& name) {
    if (name.empty() || name.size() > 4) return {};
    for (const char* set : {"xyzw", "rgba", "stpq"}) {
        std::vector<int> idx;
        for (char c : name) {
            const char* p = std::strchr(set, c);
            if (!p) break;
            idx.push_back((int)(p - set));
        }
        if (idx.size() == name.size()) return idx;
    }
    return {};
}
std::vector<int> swizzle_indices(const std::string& name) { return name.size() < 2 ? std::vector<int>() : component_indices(name); }

bool names_identifier(const std::string& glsl, std::initializer_list<const char*> names) {
    for (const Token& t : tokenize_glsl(glsl))
        if (t.kind == Token::Ident && std::any_of(names.begin(), names.end(), [&](const char* name) { return t.text == name; })) return true;
    return false;
}

TokenView::TokenView(const std::vector<Token>& stream, unsigned dropped_kinds) : stream_(&stream) {
    for (size_t k = 0; k < stream.size(); ++k)
        if (!(dropped_kinds >> stream[k].kind & 1u)) at_.push_back(k);
}

bool TokenView::spells(size_t i, const std::vector<std::string>& words) const {
    for (const std::string& w : words) {
        if (i >= n() || (*this)[i].text != w) return false;
        ++i;
    }
    return true;
}

static const char* const kOpening[] = {"(", "[", "{"};
static const char* const kClosing[] = {")", "]", "}"};
static const char* partner_of(const Token& bracket, const char* const* own, const char* const* other) {
    for (int k = 0; k < 3 && bracket.kind == Token::Punct; ++k)
        if (bracket.text == own[k]) return other[k];
    return nullptr;
}

size_t TokenView::close_of(size_t open) const {
    const char* closing = open < n() ? partner_of((*this)[open], kOpening, kClosing) : nullptr;
    if (!closing) return n();
    const std::string opening = (*this)[open].text;
    int depth = 0;
    for (size_t i = open; i < n(); ++i) {
        if (is(i, opening.c_str())) ++depth;
        else if (is(i, closing) && --depth == 0) return i;
    }
    return n();
}

size_t TokenView::open_of(size_t close) const {
    const char* opening = close < n() ? partner_of((*this)[close], kClosing, kOpening) : nullptr;
    if (!opening) return n();
    const std::string closing = (*this)[close].text;
    int depth = 0;
    for (size_t i = close + 1; i-- > 0;) {
        if (is(i, closing.c_str())) ++depth;
        else if (is(i, opening) && --depth == 0) return i;
    }
    return n();
}

std::string TokenView::text_of(size_t b, size_t e) const {
    std::string s;
    if (b >= e) return s;
    for (size_t k = raw(b); k <= raw(e - 1); ++k) {
        const Token& t = (*stream_)[k];
        s += t.kind == Token::Comment || t.kind == Token::Space ? std::string(" ") : t.text;
    }
    return s;
}

std::vector<std::pair<size_t, size_t>> TokenView::split_top_level(size_t from, size_t to, const char* separator) const {
    std::vector<std::pair<size_t, size_t>> parts;
    int depth = 0;
    size_t start = from;
    for (size_t i = from; i < to; ++i) {
        if (is(i, "(") || is(i, "[") || is(i, "{")) ++depth;
        else if (is(i, ")") || is(i, "]") || is(i, "}")) --depth;
        else if (depth == 0 && is(i, separator)) {
            parts.emplace_back(start, i);
            start = i + 1;
        }
    }
    parts.emplace_back(start, to);
    return parts;
}

void TokenEdits::drop(size_t first, size_t last) {
    for (size_t k = first; k <= last && k < stream_->size(); ++k)
        if (!((*stream_)[k].kind == Token::Space && (*stream_)[k].text == "\n")) replaced_.emplace(k, "");
}

std::vector<Token> TokenEdits::tokens() const {
    std::vector<std::pair<size_t, std::string>> inserts = inserts_;
    std::stable_sort(inserts.begin(), inserts.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<Token> out;
    out.reserve(stream_->size() + inserts.size());
    size_t next = 0;
    auto insert_up_to = [&](size_t slot) {
        while (next < inserts.size() && inserts[next].first <= slot) out.push_back({Token::Raw, inserts[next++].second});
    };
    for (size_t k = 0; k < stream_->size(); ++k) {
        insert_up_to(2 * k);
        const auto r = replaced_.find(k);
        if (r == replaced_.end()) out.push_back((*stream_)[k]);
        else if (!r->second.empty()) out.push_back({(*stream_)[k].kind, r->second});
        insert_up_to(2 * k + 1);
    }
    insert_up_to(2 * stream_->size());
    return out;
}

std::string TokenEdits::text() const {
    std::string out;
    for (const Token& t : tokens()) out += t.text;
    return out;
}

void defined_functions(const std::string& glsl, std::set<std::string>& names) {
    const std::vector<Token> toks = tokenize_glsl(glsl);
    const TokenView s(toks);
    int depth = 0;
    for (size_t i = 0; i < s.n(); ++i) {
        if (s.is(i, "{")) ++depth;
        else if (s.is(i, "}")) --depth;
        else if (depth == 0 && s.is(i, "(") && s.ident(i - 1) && s.ident(i - 2)) names.insert(s[i - 1].text);
    }
}

void functions_with_out_params(const std::string& glsl, std::set<std::string>& names) {
    const std::vector<Token> toks = tokenize_glsl(glsl);
    const TokenView s(toks);
    for (size_t i = 0; i < s.n(); ++i) {
        if (!((s.ident(i, "out") || s.ident(i, "inout")) && s.ident(i + 1))) continue;
        int depth = 0;
        size_t open = i;  // back to the `(` that opens this parameter list
        while (open-- > 0 && !(s.is(open, "(") && depth == 0)) depth += s.is(open, ")") ? 1 : s.is(open, "(") ? -1 : 0;
        if (s.ident(open - 1)) names.insert(s[open - 1].text);  // (no such `(`: `open` is past every index, and nothing is one)
    }
}

static bool is_code(const Token& t) { return t.kind != Token::Space && t.kind != Token::Comment; }

size_t next_code(const std::vector<Token>& stream, size_t k) {
    while (k < stream.size() && !is_code(stream[k])) ++k;
    return std::min(k, stream.size());
}

size_t prev_code(const std::vector<Token>& stream, size_t k) {
    while (k-- > 0)
        if (is_code(stream[k])) return k;
    return stream.size();
}

}  // namespace ptl
