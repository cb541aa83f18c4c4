// glsl_hoist.cpp -- see glsl_hoist.h.  The shape of the text is glsl_syntax.h's business, what is uniform glsl_binding.h's; here the
// hoistable expressions of each function become members of the uniform block, statements of the prologue and a rewritten text.
#include "glsl_hoist.h"

#include <algorithm>

#include "glsl_binding.h"
#include "glsl_syntax.h"
#include "glsl_tokens.h"

namespace ptl {
namespace {

struct PrologueItem {
    size_t at = 0;
    int loop = 0;  // > 0: belongs into the table loop of that loop; < 0: likewise, behind the tables (the update of a carried local)
    std::string text;
};

struct FunctionOutcome {  // what hoisting did to one function
    std::vector<HoistedMember> members;
    std::string prologue;  // its block
    int ids_used = 0;      // of the kernel-wide member numbers, from the one it was given on
};

// One function's block of the prologue: source order; the items of a loop inside one table loop at the loop's place, updates last.
std::string prologue_block(std::vector<PrologueItem> items) {
    std::stable_sort(items.begin(), items.end(), [](const PrologueItem& a, const PrologueItem& b) { return a.at < b.at; });
    std::string text = "{\n";
    std::set<int> emitted;
    for (const PrologueItem& it : items) {
        if (it.loop == 0) {
            text += "    " + it.text + "\n";
            continue;
        }
        const int l = it.loop > 0 ? it.loop : -it.loop;
        if (!emitted.insert(l).second) continue;
        text += "    for (int ptl_k = 0; ptl_k < " + std::to_string(kTableEntries) + "; ptl_k++) {\n";
        for (int sign : {1, -1})
            for (const PrologueItem& in : items)
                if (in.loop == sign * l) text += "        " + in.text + "\n";
        text += "    }\n";
    }
    return text + "}\n";
}

// Hoists the work of one parsed function.  Member numbers are taken in this order, which the generated text shows: the guards of the
// loops that carry something, the members as the sites are walked, one table per carried local; wherever carried locals are listed,
// the uniform chains come before the rays, each by name.
class FunctionHoist {
  public:
    FunctionHoist(const TokenView& s, const ParsedBody& body, const HoistParams& params, const FunctionSpan& fn, int first_id, TokenEdits& edits)
        : s_(s), body_(body), P(params), fn_(fn), first_id_(first_id), edits_(edits), bt_(s, body, params, fn.param_names(), fn.body_e) {}

    FunctionOutcome run() {
        for (bool ray : {false, true})
            for (auto& c : bt_.carried())
                if (c.second.ray == ray && !loop_tags_.count(c.second.loop)) loop_tags_[c.second.loop] = first_id_ + out_.ids_used++;  // (a number unique in the kernel)
        for (size_t si = 0; si < body_.sites.size(); ++si) {
            const Site& site = body_.sites[si];
            if (site.root < 0 || site.header || bt_.is_update(si)) continue;
            bt_.classify(site.root);
            hoist_in(site.root);
        }
        if (out_.members.empty() && bt_.carried().empty()) return out_;  // nothing to do here (and nothing was numbered or replaced)
        for (bool ray : {false, true})
            for (auto& c : bt_.carried())
                if (c.second.ray == ray) tabulate(c.first, c.second);
        guard_the_loops();
        declare_for_the_prologue();
        out_.prologue = prologue_block(items_);
        return out_;
    }

  private:
    const TokenView& s_;
    const ParsedBody& body_;
    const HoistParams& P;
    const FunctionSpan& fn_;
    const int first_id_;
    TokenEdits& edits_;  // of the whole text: the significant tokens [b, e) become `text`, line for line (b == e: `text` goes in front of b)
    BindingTimes bt_;
    FunctionOutcome out_;
    std::vector<PrologueItem> items_;
    std::map<int, int> loop_tags_;  // loop id (per function) -> number unique in the kernel
    bool rays_used_ = false;        // members hold ray origins: the prologue needs the rays themselves

    std::string guard_name(int loop) const { return "ptl_tab_ok_" + std::to_string(loop_tags_.at(loop)); }
    std::string text_of(int id) const { return s_.text_of(body_.nodes[id].b, body_.nodes[id].e); }

    // A new member of the block: a table if it belongs to a loop.  The prologue stores `value` in it where `at` stands (as entry ptl_k of
    // a table); returns the expression that reads it (a table's entry `index`).
    std::string make_member(const std::string& type, size_t at, int loop, const std::string& value, const std::string& index) {
        const HoistedMember m{type, "ptl_hv" + std::to_string(first_id_ + out_.ids_used++), loop > 0 ? kTableEntries : 0};
        out_.members.push_back(m);
        items_.push_back({at, loop, "PTL_DV_OUT." + m.name + (loop > 0 ? "[ptl_k]" : "") + " = " + value + ";"});
        return "PTL_U." + m.name + (loop > 0 ? "[" + index + "]" : "");
    }
    // What a member has to hold of a local or an expression of either kind, and the value that the member stands for in the snippet:
    // of a ray only the origin is uniform, the rest of `expr` stays where it is.
    static std::string stored(bool ray, const std::string& expr, bool a_name) { return !ray ? expr : a_name ? expr + ".o" : "(" + expr + ").o"; }
    static std::string loaded(bool ray, const std::string& expr, const std::string& read) { return ray ? "ptl_ray_o(" + expr + ", " + read + ")" : read; }

    // a new member holding `expr` (evaluated where node `like` stands); returns the expression that stands for `expr` there
    std::string member_for(const std::string& type, int like, const std::string& expr, bool ray = false) {
        const Binding& bd = bt_.of(like);
        const std::string index = bd.loop > 0 ? body_.loops[bd.loop - 1].var + (bd.phase == 1 ? " + 1" : "") : "";
        const std::string value = loaded(ray, expr, make_member(type, body_.nodes[like].b, bd.loop, stored(ray, expr, false), index));
        rays_used_ = rays_used_ || ray;
        return bd.loop > 0 ? "(" + guard_name(bd.loop) + " ? " + value + " : (" + expr + "))" : value;
    }
    void replace(size_t b, size_t e, const std::string& text) {
        if (b == e) return edits_.before(s_, b, text);
        edits_.replace(s_.raw(b), text);
        edits_.drop(s_.raw(b) + 1, s_.raw(e - 1));
    }

    void hoist_in(int id) {
        const Node& nd = body_.nodes[id];
        const Binding& bd = bt_.of(id);
        if (bd.ray_hoistable() || bd.hoistable()) {
            const bool ray = bd.ray_hoistable();
            return replace(nd.b, nd.e, member_for(ray ? "vec4" : bd.type, id, text_of(id), ray));
        }
        if (nd.kind == Node::Call && bt_.library_function(nd.text)) {
            auto staged_arg = [&](size_t k) { return k < nd.kids.size() && bt_.of(nd.kids[k]).placeable() && bt_.of(nd.kids[k]).type == "vec3"; };
            if ((nd.text == "normalize_normal" && nd.kids.size() == 2 && staged_arg(0)) || (nd.text == "plane_intersect" && nd.kids.size() == 3 && staged_arg(2))) {
                const size_t which = nd.text == "normalize_normal" ? 0 : 2;
                const Node& arg = body_.nodes[nd.kids[which]];
                replace(nd.b, nd.b + 1, nd.text == "normalize_normal" ? "ptl_normalize_normal_unit" : "ptl_plane_intersect_unit");
                replace(arg.b, arg.e, member_for("vec3", nd.kids[which], "normalize(" + text_of(nd.kids[which]) + ")"));
                for (size_t k = 0; k < nd.kids.size(); ++k)
                    if (k != which) hoist_in(nd.kids[k]);
                return;
            }
            if (nd.text == "is_collinear" && nd.kids.size() == 2 && (staged_arg(1) || staged_arg(0))) {
                const size_t which = staged_arg(1) ? 1 : 0;
                replace(nd.b, nd.b + 1, which == 1 ? "ptl_is_collinear_len" : "ptl_is_collinear_len0");
                replace(nd.e - 1, nd.e - 1, ", " + member_for("float", nd.kids[which], "length(" + text_of(nd.kids[which]) + ")"));
            }
        }
        for (int k : nd.kids) hoist_in(k);
    }

    // a carried local: its table (first in the table loop: the value each trip starts with), the update as the prologue's step (last),
    // and in the snippet the update guarded: from the table, or as written
    void tabulate(const std::string& name, const Carried& c) {
        const Site& update = body_.sites[c.update_site];
        const LoopInfo& L = body_.loops[c.loop - 1];
        const std::string rhs = text_of(body_.nodes[update.root].kids[1]);
        const std::string read = make_member(c.ray ? "vec4" : c.type, L.body_b, c.loop, stored(c.ray, name, true), L.var + " + 1");
        rays_used_ = rays_used_ || c.ray;
        items_.push_back({update.stmt_b, -c.loop, name + " = " + rhs + ";"});
        replace(update.stmt_b, update.stmt_e, "if (" + guard_name(c.loop) + ") " + name + " = " + loaded(c.ray, rhs, read) + "; else " + name + " = " + rhs + ";");
    }
    void guard_the_loops() {  // every loop that got a table: is it short enough for it?
        std::set<int> used;
        for (const PrologueItem& it : items_)
            if (it.loop != 0) used.insert(it.loop > 0 ? it.loop : -it.loop);
        for (int l : used) {
            const LoopInfo& L = body_.loops[l - 1];
            replace(L.kw, L.kw, "const bool " + guard_name(l) + " = (" + L.bound + ") <= " + std::to_string(kTableLoop) + "; ");
        }
    }
    void declare_locals(bool ray) {  // as the snippet declares them
        for (auto& l : bt_.locals())
            for (const Site& site : body_.sites)
                if (l.second.ray == ray && site.kind == Site::DeclInit && site.decl_name == l.first && site.name_at == l.second.name_at)
                    items_.push_back({site.name_at, 0, site.decl_type + " " + site.decl_name + " = " + text_of(site.root) + ";"});
    }
    void declare_for_the_prologue() {
        declare_locals(false);  // uniform locals: the prologue needs them wherever a hoisted expression names one
        // The rays themselves: the parameters as dummies with the right origin, the locals as declared.  Not only when a ray
        // expression was rewritten (rays_used_): a plain uniform expression or uniform local may read `r.o` -- or `q.o` of a copy
        // `Ray q = r;` -- of an origin-uniform ray (Member-on-half is classed uniform), and then the prologue names the ray too.
        if (!rays_used_ && (P.origin_uniform_rays.empty() || items_.empty())) return;
        for (const std::string& p : P.origin_uniform_rays) items_.push_back({fn_.body_b, 0, "Ray " + p + " = Ray(" + P.origin_expr + ", vec4(0.0), 1.0, false);"});
        declare_locals(true);
    }
};

}  // namespace

HoistResult hoist_uniform_work(const std::string& glsl, const HoistParams& params, int& next_member) {
    HoistResult out;
    out.glsl = glsl;
    try {
        const std::vector<Token> toks = tokenize_glsl(glsl);
        const TokenView s(toks, TokenView::kLayout);  // keeps directives: a text that has one is left as it is
        for (size_t i = 0; i < s.n(); ++i)
            if (s[i].kind == Token::Preproc || s[i].kind == Token::Raw) return out;  // macros: the text is not what the compiler will see
        std::vector<FunctionSpan> fns;
        if (params.body_only) {  // all of the text, with the parameters the caller names
            fns.emplace_back();
            fns[0].body_e = s.n();
            for (const std::string& name : params.body_params) fns[0].params.push_back({0, 0, name, false});
        } else {
            for (const FunctionSpan& fn : function_definitions(s))
                if (fn.body_e < s.n() && s[fn.type_at].text != "return") fns.push_back(fn);  // whole functions, and `return f(x) {` opens none
        }
        TokenEdits edits(toks);
        HoistResult hoisted;
        int next = next_member;
        for (const FunctionSpan& fn : fns) {
            const ParsedBody body = parse_body(s, fn.body_b, fn.body_e);
            if (!body.ok) continue;  // leave this function exactly as written
            const FunctionOutcome f = FunctionHoist(s, body, params, fn, next, edits).run();
            hoisted.members.insert(hoisted.members.end(), f.members.begin(), f.members.end());
            hoisted.prologue += f.prologue;
            next += f.ids_used;
        }
        if (hoisted.members.empty()) return out;
        hoisted.glsl = edits.text();
        next_member = next;
        return hoisted;
    } catch (...) {  // (never throws: on anything unexpected the text comes back unchanged)
        HoistResult unchanged;
        unchanged.glsl = glsl;
        return unchanged;
    }
}

}  // namespace ptl
