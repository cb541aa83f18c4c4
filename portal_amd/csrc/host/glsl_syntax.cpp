// glsl_syntax.cpp -- see glsl_syntax.h.
#include "glsl_syntax.h"

#include <map>

namespace ptl {
namespace {

struct ParseError {};  // thrown and caught in this file alone: parse_body() turns it into ParsedBody::ok == false

class Parser {
  public:
    Parser(const TokenView& s, ParsedBody& out) : s_(s), out_(out) {}

    void block(size_t pos, size_t end, int depth, int loop) {
        while (pos < end) statement(pos, end, depth, loop);
    }

  private:
    const TokenView& s_;
    ParsedBody& out_;

    // ---- expressions ---------------------------------------------------------------------------------------------------------
    int add(Node nd) {
        out_.nodes.push_back(std::move(nd));
        return (int)out_.nodes.size() - 1;
    }
    static int precedence(const std::string& op) {
        static const std::map<std::string, int> p = {{"*", 12}, {"/", 12}, {"%", 12}, {"+", 11}, {"-", 11}, {"<<", 10}, {">>", 10}, {"<", 9},  {">", 9},
                                                     {"<=", 9}, {">=", 9}, {"==", 8}, {"!=", 8}, {"&", 7},  {"^", 6},   {"|", 5},   {"&&", 4}, {"||", 3},
                                                     {"?", 2},  {"=", 1},  {"+=", 1}, {"-=", 1}, {"*=", 1}, {"/=", 1}};
        auto it = p.find(op);
        return it == p.end() ? 0 : it->second;
    }
    void expect(size_t& pos, const char* punct) {
        if (!s_.is(pos, punct)) throw ParseError{};
        ++pos;
    }
    int parse_expr(size_t& pos, size_t end, int min_prec) {
        int lhs = parse_unary(pos, end);
        while (pos < end && s_[pos].kind == Token::Punct) {
            const std::string op = s_[pos].text;
            const int prec = precedence(op);
            if (prec == 0 || prec < min_prec) break;
            ++pos;
            Node nd;
            nd.b = out_.nodes[lhs].b;
            nd.text = op;
            if (op == "?") {
                int mid = parse_expr(pos, end, 1);
                expect(pos, ":");
                nd.kind = Node::Ternary;
                nd.kids = {lhs, mid, parse_expr(pos, end, 2)};
            } else {
                nd.kind = prec == 1 ? Node::Assign : Node::Binary;  // (assignments associate to the right)
                nd.kids = {lhs, parse_expr(pos, end, prec == 1 ? 1 : prec + 1)};
            }
            nd.e = pos;
            lhs = add(nd);
        }
        return lhs;
    }
    int parse_unary(size_t& pos, size_t end) {
        if (pos >= end) throw ParseError{};
        if (s_[pos].kind == Token::Punct) {
            const std::string op = s_[pos].text;
            if (op == "-" || op == "+" || op == "!" || op == "~" || op == "++" || op == "--") {
                Node nd;
                nd.kind = Node::Unary;
                nd.b = pos;
                nd.text = op;
                ++pos;
                nd.kids = {parse_unary(pos, end)};
                nd.e = pos;
                return add(nd);
            }
        }
        return parse_postfix(pos, end);
    }
    int parse_postfix(size_t& pos, size_t end) {
        int cur = parse_primary(pos, end);
        while (pos < end) {
            Node nd;
            nd.b = out_.nodes[cur].b;
            if (s_.is(pos, ".")) {
                if (!s_.ident(pos + 1) || s_.is(pos + 2, "(")) throw ParseError{};  // (a method call: .length())
                nd.kind = Node::Member;
                nd.text = s_[pos + 1].text;
                nd.kids = {cur};
                pos += 2;
            } else if (s_.is(pos, "[")) {
                ++pos;
                int idx = parse_expr(pos, end, 1);
                expect(pos, "]");
                nd.kind = Node::Index;
                nd.kids = {cur, idx};
            } else if (s_.is(pos, "++") || s_.is(pos, "--")) {
                nd.kind = Node::Post;
                nd.text = s_[pos].text;
                nd.kids = {cur};
                ++pos;
            } else {
                break;
            }
            nd.e = pos;
            cur = add(nd);
        }
        return cur;
    }
    int parse_primary(size_t& pos, size_t end) {
        if (pos >= end) throw ParseError{};
        Node nd;
        nd.b = pos;
        const Token& t = s_[pos];
        if (t.kind == Token::Number) {
            nd.kind = Node::Lit;
            nd.text = t.text;
            nd.e = ++pos;
            return add(nd);
        }
        if (t.kind == Token::Ident) {
            nd.text = t.text;
            if (s_.is(pos + 1, "(")) {
                nd.kind = Node::Call;
                pos += 2;
                if (s_.is(pos, ")")) {
                    ++pos;
                } else {
                    for (;;) {
                        nd.kids.push_back(parse_expr(pos, end, 1));
                        if (s_.is(pos, ",")) {
                            ++pos;
                            continue;
                        }
                        expect(pos, ")");
                        break;
                    }
                }
                nd.e = pos;
                return add(nd);
            }
            nd.kind = Node::Ident;
            nd.e = ++pos;
            return add(nd);
        }
        if (s_.is(pos, "(")) {
            ++pos;
            nd.kind = Node::Paren;
            nd.kids = {parse_expr(pos, end, 1)};
            expect(pos, ")");
            nd.e = pos;
            return add(nd);
        }
        throw ParseError{};
    }

    // ---- statements ----------------------------------------------------------------------------------------------------------
    // parses one expression that must end exactly at `stop` (a `;`, `)` ... the caller has found)
    int expression_until(size_t b, size_t stop) {
        size_t pos = b;
        int root = parse_expr(pos, stop, 1);
        if (pos != stop) throw ParseError{};
        return root;
    }
    static Site site(int depth, int loop, bool header, int root = -1) {
        Site s;
        s.depth = depth;
        s.loop = loop;
        s.header = header;
        s.root = root;
        return s;
    }
    size_t statement_end(size_t pos, size_t end) const {  // the `;` that ends the statement starting at pos (brackets balanced)
        int depth = 0;
        for (size_t i = pos; i < end; ++i) {
            if (s_.is(i, "(") || s_.is(i, "[")) ++depth;
            else if (s_.is(i, ")") || s_.is(i, "]")) --depth;
            else if (s_.is(i, "{") || s_.is(i, "}")) throw ParseError{};
            else if (s_.is(i, ";") && depth == 0) return i;
        }
        throw ParseError{};
    }
    size_t close_before(size_t open, const char* bracket, size_t end) const {  // what closes the `(` or `{` that must stand at `open`, inside the range
        if (!s_.is(open, bracket)) throw ParseError{};
        const size_t close = s_.close_of(open);
        if (close >= end) throw ParseError{};
        return close;
    }
    void controlled(size_t& pos, size_t end, int depth, int loop) {  // the statement an if / else / for / while governs
        if (s_.is(pos, "{")) {
            const size_t close = close_before(pos, "{", end);
            block(pos + 1, close, depth + 1, loop);
            pos = close + 1;
        } else {
            statement(pos, end, depth + 1, loop);
        }
    }
    void declaration_or_expression(size_t& pos, size_t end, int depth, int loop, bool header) {
        size_t p = pos;
        while (s_.ident(p, "const") || s_.ident(p, "highp") || s_.ident(p, "mediump") || s_.ident(p, "lowp")) ++p;
        const bool declares = s_.ident(p) && s_.ident(p + 1) && (s_.is(p + 2, "=") || s_.is(p + 2, ";") || s_.is(p + 2, ",") || s_.is(p + 2, "["));
        const size_t semi = statement_end(pos, end);
        if (!declares) {
            Site s = site(depth, loop, header, expression_until(pos, semi));
            s.stmt_b = pos;
            s.stmt_e = semi + 1;
            out_.sites.push_back(s);
        }
        for (size_t q = p + 1; declares;) {  // one site per declarator
            if (!s_.ident(q)) throw ParseError{};
            Site s = site(depth, loop, header);
            s.kind = Site::Decl;
            s.decl_type = s_[p].text;
            s.decl_name = s_[q].text;
            s.name_at = q;
            ++q;
            if (s_.is(q, "[")) throw ParseError{};  // arrays: not handled
            if (s_.is(q, "=")) {
                ++q;
                s.kind = Site::DeclInit;
                s.root = parse_expr(q, semi, 1);
            }
            out_.sites.push_back(s);
            if (s_.is(q, ",")) {
                ++q;
                continue;
            }
            if (q != semi) throw ParseError{};
            break;
        }
        pos = semi + 1;
    }
    void loop_statement(size_t& pos, size_t end, int depth, int loop) {
        const bool is_for = s_[pos].text == "for";
        const size_t close = close_before(pos + 1, "(", end);
        LoopInfo L;
        L.id = (int)out_.loops.size() + 1;
        L.outer = loop;
        L.depth = depth;
        L.kw = pos;
        L.header_open = pos + 1;
        L.header_close = close;
        size_t p = pos + 2;
        // `for (int I = 0; I < BOUND; I++)`, token for token: the only loop shape whose trip number is known to be I
        if (is_for && s_.ident(p, "int") && s_.ident(p + 1) && s_.is(p + 2, "=") && s_.number(p + 3) && s_[p + 3].text == "0" && s_.is(p + 4, ";") &&
            s_.ident(p + 5, s_[p + 1].text) && s_.is(p + 6, "<") && (s_.ident(p + 7) || s_.number(p + 7)) && s_.is(p + 8, ";") && s_.ident(p + 9, s_[p + 1].text) &&
            s_.is(p + 10, "++") && p + 11 == close) {
            L.canonical = true;
            L.var = s_[p + 1].text;
            L.bound = s_[p + 7].text;
        }
        out_.loops.push_back(L);
        const size_t slot = out_.loops.size() - 1;  // (by index: loops nested in the body are appended behind it)
        if (is_for) {
            if (s_.is(p, ";")) ++p;
            else declaration_or_expression(p, close, depth + 1, L.id, true);  // init (ends at its `;`)
            const size_t semi = statement_end(p, close);
            if (semi > p) out_.sites.push_back(site(depth + 1, L.id, true, expression_until(p, semi)));
            if (semi + 1 < close) out_.sites.push_back(site(depth + 1, L.id, true, expression_until(semi + 1, close)));
        } else {
            out_.sites.push_back(site(depth + 1, L.id, true, expression_until(p, close)));
        }
        pos = close + 1;
        out_.loops[slot].braced = s_.is(pos, "{");
        out_.loops[slot].body_b = pos;
        controlled(pos, end, depth, L.id);
        out_.loops[slot].body_e = pos;
    }
    void statement(size_t& pos, size_t end, int depth, int loop) {
        if (s_.is(pos, ";")) {
            ++pos;
        } else if (s_.is(pos, "{")) {
            const size_t close = close_before(pos, "{", end);
            block(pos + 1, close, depth + 1, loop);
            pos = close + 1;
        } else if (s_.ident(pos, "if")) {
            const size_t close = close_before(pos + 1, "(", end);
            out_.sites.push_back(site(depth, loop, false, expression_until(pos + 2, close)));
            pos = close + 1;
            controlled(pos, end, depth, loop);
            if (s_.ident(pos, "else")) {
                ++pos;
                controlled(pos, end, depth, loop);
            }
        } else if (s_.ident(pos, "for") || s_.ident(pos, "while")) {
            loop_statement(pos, end, depth, loop);
        } else if (s_.ident(pos, "return")) {
            const size_t semi = statement_end(pos, end);
            if (semi > pos + 1) out_.sites.push_back(site(depth, loop, false, expression_until(pos + 1, semi)));
            pos = semi + 1;
        } else if (s_.ident(pos, "break") || s_.ident(pos, "continue") || s_.ident(pos, "discard")) {
            if (s_[pos].text == "continue")
                for (int l = loop; l > 0; l = out_.loops[l - 1].outer) out_.loops[l - 1].has_continue = true;  // (only the innermost is skipped, but be strict)
            if (!s_.is(pos + 1, ";")) throw ParseError{};
            pos += 2;
        } else if (s_.ident(pos, "do") || s_.ident(pos, "switch") || s_.ident(pos, "case") || s_.ident(pos, "default") || s_.ident(pos, "struct") ||
                   s_.ident(pos, "goto") || s_.ident(pos, "else")) {
            throw ParseError{};
        } else {
            declaration_or_expression(pos, end, depth, loop, false);
        }
    }
};

}  // namespace

std::string ParsedBody::base_identifier(int id) const {
    const Node& nd = nodes[id];
    if (nd.kind == Node::Ident) return nd.text;
    if (nd.kind == Node::Member || nd.kind == Node::Index || nd.kind == Node::Paren) return base_identifier(nd.kids[0]);
    return "";
}

bool ParsedBody::mentions(int id, const std::string& name) const {
    const Node& nd = nodes[id];
    if (nd.kind == Node::Ident && nd.text == name) return true;
    for (int k : nd.kids)
        if (mentions(k, name)) return true;
    return false;
}

ParsedBody parse_body(const TokenView& s, size_t b, size_t e) {
    ParsedBody out;
    try {
        Parser(s, out).block(b, e, 0, 0);
        out.ok = true;
    } catch (const ParseError&) {
    }
    return out;
}

bool tokens_mention(const TokenView& s, size_t b, size_t e, const std::string& name) {
    for (size_t i = b; i < e && i < s.n(); ++i)
        if (s.ident(i, name) && !(i > 0 && s.is(i - 1, "."))) return true;
    return false;
}

std::vector<FunctionSpan> function_definitions(const TokenView& s) {
    std::vector<FunctionSpan> fns;
    int depth = 0;
    for (size_t i = 0; i < s.n(); ++i) {
        if (s.is(i, "{")) ++depth;
        else if (s.is(i, "}")) --depth;
        else if (depth == 0 && s.ident(i) && s.ident(i + 1) && s.is(i + 2, "(")) {
            const size_t close = s.close_of(i + 2);
            if (!s.is(close + 1, "{")) continue;
            FunctionSpan f;
            f.type_at = i, f.name_at = i + 1, f.body_b = close + 2, f.body_e = s.close_of(close + 1);
            if (close > i + 3)
                for (const auto& [b, e] : s.split_top_level(i + 3, close, ",")) {
                    FunctionSpan::Param p{b, e, "", false};
                    for (size_t j = b; j < e; ++j) {
                        if (s.ident(j)) p.name = s[j].text;
                        p.out = p.out || s.ident(j, "out") || s.ident(j, "inout");
                    }
                    f.params.push_back(p);
                }
            fns.push_back(f);
            for (size_t j = i + 3; j < close; ++j) depth += s.is(j, "{") ? 1 : s.is(j, "}") ? -1 : 0;  // (a brace astray in the list counts like any other)
            i = f.body_e;  // (the body leaves the depth as it is; past an open one there is nothing at depth 0)
        }
    }
    return fns;
}

std::vector<std::string> FunctionSpan::param_names() const {
    std::vector<std::string> names;
    for (const Param& p : params)
        if (!p.name.empty()) names.push_back(p.name);
    return names;
}

}  // namespace ptl
