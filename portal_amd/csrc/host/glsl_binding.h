// glsl_binding.h -- the binding-time analysis of ONE parsed function body (glsl_syntax.h) for the uniform-work hoister (glsl_hoist.h): which
// expressions depend on nothing but run-time uniforms, which locals hold such values, and which of those a canonical loop carries from
// trip to trip.  An object of this class is made for one function and dies with it: nothing it learns can reach the next function.
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

#include "glsl_hoist.h"
#include "glsl_syntax.h"

namespace ptl {

struct Binding {  // of one node, parallel to ParsedBody::nodes
    std::string type;  // GLSL type, "" = unknown
    bool uniform = false;
    bool leaf = false;  // reads at least one run-time uniform (directly or through a local)
    bool op = false;    // does arithmetic
    int cost = 0;       // ... roughly this many VALU instructions of it
    bool half = false;  // a Ray whose origin is uniform and whose direction is not (first-trip variants); then `uniform` is false
    int loop = 0;       // > 0: depends on the carried variables of that loop ...
    int phase = 0;      // ... 0 as they are before their updates in the iteration, 1 after, -1 mixed

    bool placeable() const { return uniform && leaf && (loop == 0 || phase >= 0); }
    // worth a member: a scalar load replaces it, so one multiplication alone is not
    bool hoistable() const;
    // a Ray with a uniform origin that is more than a name: its origin arithmetic can come from the prologue
    bool ray_hoistable() const { return half && leaf && op && (loop == 0 || phase >= 0); }
};

// A local declared at the top level of the function whose value -- or, `ray`, whose origin: `Ray V = <ray with a uniform origin>;` -- is
// uniform from its declaration on: written once, or once more by its update in a loop (Carried).
struct Local {
    std::string type;
    size_t name_at = 0;  // significant-token index of the declared name
    bool leaf = false;   // its value depends on a run-time uniform (not just on literals)
    bool ray = false;
};

struct Carried {  // a Local that a canonical loop advances by `V = f(V, uniforms);`: inside the loop a function of the trip number alone
    std::string type;
    int loop = 0;
    int update_site = -1;
    bool leaf = false;  // ... and of at least one run-time uniform (a chain of baked constants is the compiler's business)
    bool ray = false;
};

class BindingTimes {
  public:
    // `body_e`: one past the last token of the body; `params`: the function's parameter names
    BindingTimes(const TokenView& s, const ParsedBody& body, const HoistParams& P, const std::vector<std::string>& params, size_t body_e);

    // Classifies the expression anew (bottom-up, by what is known of the locals NOW) and returns its root's binding; of() reads what
    // the last classify() of a tree left at one of its nodes.
    const Binding& classify(int id);
    const Binding& of(int id) const { return bindings_[id]; }

    const std::map<std::string, Local>& locals() const { return locals_; }
    const std::map<std::string, Carried>& carried() const { return carried_; }  // by name: the order in which members are numbered
    bool is_update(size_t site) const;  // the update statement of a carried local
    // is `name` the library's function of that name (neither a local nor a function of the scene)?
    bool library_function(const std::string& name) const { return !declared_.count(name) && !P.scene_functions.count(name); }

  private:
    const TokenView& s_;
    const ParsedBody& body_;
    const HoistParams& P;
    const size_t body_e_;
    std::vector<Binding> bindings_;
    std::set<std::string> declared_;
    std::map<std::string, int> writes_;
    std::map<std::string, Local> locals_;
    std::map<std::string, Carried> carried_;

    int writes(const std::string& name) const;
    void count_writes(int id);
    void classify_identifier(const Node& nd, Binding& bd) const;
    void top_level_local(size_t si, bool ray);
    int update_in_canonical_loop(size_t si, bool ray) const;
    void drop_chains_that_read_a_dropped_one();
};

}  // namespace ptl
