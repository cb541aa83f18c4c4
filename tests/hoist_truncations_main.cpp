// hoist_truncations_main.cpp -- the uniform-work hoister on texts that stop anywhere, as a program of its own (built and run by
// tests/test_host_logic.py::test_hoister_on_truncated_snippets_under_sanitizers with the host units of the hoister, under sanitizers).
//
//   hoist_truncations SNIPPETS CUTS
//
// SNIPPETS holds texts, each as a decimal length, a newline and that many bytes.  Every text is cut behind each of its first CUTS tokens
// and taken whole; every cut goes through hoist_uniform_work as a function body and as a file-scope text, each with and without the ray
// parameter `r` having a uniform origin.  Prints the number of runs and a digest (FNV-1a, 64 bits) of everything that came back.
// A second line does the same for the other passes that write through TokenEdits: every cut through translate_glsl (as a body and as a
// file-scope text, with and without deferred updates), through bound_nearer_blocks, and the translation through specialize_translated with
// the cut's matrix names as masked and every identifier of the cut as a loop bound of 4; and, beside them, through
// check_out_argument_aliasing as a file-scope text and as a body at once.  A refusal counts with its message.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "portal_amd/csrc/host/glsl_hoist.h"
#include "portal_amd/csrc/host/glsl_tokens.h"
#include "portal_amd/csrc/host/glsl_translate.h"

namespace {

struct Digest {
    uint64_t value = 1469598103934665603ull;
    void fold(const std::string& text) {
        for (unsigned char c : text) value = (value ^ c) * 1099511628211ull;
        value = (value ^ 0xff) * 1099511628211ull;  // (a separator no text holds)
    }
};

bool ends_with(const std::string& s, const char* tail) {
    const std::string t(tail);
    return s.size() >= t.size() && s.compare(s.size() - t.size(), t.size(), t) == 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    std::ifstream in(argv[1], std::ios::binary);
    const size_t cuts = (size_t)std::atoi(argv[2]);
    std::vector<std::string> snippets;
    for (size_t length; in >> length;) {
        in.get();
        std::string text(length, '\0');
        if (!in.read(text.data(), (std::streamsize)length)) return 3;
        snippets.push_back(text);
    }
    size_t runs = 0, changed = 0, edit_runs = 0, edit_changed = 0, refused = 0;
    Digest hoisted, edited;
    for (const std::string& snippet : snippets) {
        const std::vector<ptl::Token> toks = ptl::tokenize_glsl(snippet);
        ptl::HoistParams base;
        for (const ptl::Token& t : toks) {  // the scene's uniforms by their names, as tools/source_matrix.py guesses them
            if (t.kind != ptl::Token::Ident) continue;
            if (ends_with(t.text, "_mat") || ends_with(t.text, "_mat_inv") || ends_with(t.text, "_mat_teleport")) base.uniforms[t.text] = "mat4";
            else if (ends_with(t.text, "_u")) base.uniforms[t.text] = "float";
        }
        ptl::defined_functions(snippet, base.scene_functions);
        ptl::functions_with_out_params(snippet, base.functions_with_out_params);
        base.body_params = {"r", "pos", "x", "y", "back", "first", "hit", "i"};
        base.origin_expr = "PTL_DV_OUT.ptl_dv_origin";
        std::string text;
        std::set<std::string> masked;
        std::map<std::string, int> unroll_bounds;
        for (size_t k = 0; k <= toks.size(); ++k) {
            if (k > 0) text += toks[k - 1].text;
            if (k > 0 && toks[k - 1].kind == ptl::Token::Ident) {
                unroll_bounds[toks[k - 1].text] = 4;
                if (ptl::is_scene_matrix_name(toks[k - 1].text)) masked.insert(toks[k - 1].text);
            }
            if (k == 0 || (k > cuts && k < toks.size())) continue;
            for (int variant = 0; variant < 4; ++variant) {
                ptl::HoistParams p = base;
                p.body_only = (variant & 1) != 0;
                if (variant & 2) p.origin_uniform_rays = {"r"};
                int counter = 7;
                const ptl::HoistResult r = ptl::hoist_uniform_work(text, p, counter);
                hoisted.fold(r.glsl);
                hoisted.fold(r.prologue);
                for (const ptl::HoistedMember& m : r.members) hoisted.fold(m.type + " " + m.name + " " + std::to_string(m.length));
                hoisted.fold(std::to_string(counter));
                ++runs;
                changed += r.glsl != text;
            }
            auto edit = [&](auto&& pass) {  // one run of a pass: what it returns, or what it says when it refuses
                std::string made;
                try {
                    made = pass();
                    edit_changed += made != text;
                } catch (const std::runtime_error& e) {
                    made = std::string("refused: ") + e.what();
                    ++refused;
                }
                edited.fold(made);
                ++edit_runs;
                return made;
            };
            std::string translated;
            for (int variant = 0; variant < 4; ++variant) {
                const std::string made = edit([&] { return ptl::translate_glsl(text, (variant & 1) == 0, (variant & 2) != 0); });
                if (variant == 0) translated = made;
            }
            edit([&] {
                int bounded = 0;
                const std::string made = ptl::bound_nearer_blocks(text, base.functions_with_out_params, &bounded);
                return made + " " + std::to_string(bounded);
            });
            edit([&] {
                ptl::check_out_argument_aliasing({text}, {text});
                return text;
            });
            if (translated.compare(0, 9, "refused: ") != 0)
                edit([&] {
                    int unrolled = 0;
                    const std::string made = ptl::specialize_translated(translated, masked, unroll_bounds, &unrolled);
                    return made + " " + std::to_string(unrolled);
                });
        }
    }
    std::printf("snippets %zu, runs %zu, texts changed %zu, digest %016llx\n", snippets.size(), runs, changed, (unsigned long long)hoisted.value);
    std::printf("edits: runs %zu, refused %zu, texts changed %zu, digest %016llx\n", edit_runs, refused, edit_changed, (unsigned long long)edited.value);
    return 0;
}
