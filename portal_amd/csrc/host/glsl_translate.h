// glsl_translate.h -- token-level rewrite of the GLSL ES 3.00 snippets stored in scene files
// into C++ that compiles against device/ptl_glsl.h (for hiprtc and for the host build).
//
// The reference hands these snippets verbatim to the GL driver's GLSL compiler
// (src/gui/scene.rs:776,865,877,1020,1041).  A HIP kernel has no GLSL front end, so the
// differences between the two languages are bridged here, lexically and line-preserving
// (the output has exactly as many lines as the input, so compiler diagnostics still point
// at the right snippet line -- the job of src/code_generation.rs's LineNumbersByKey):
//   * floating literals get an `f` suffix (GLSL literals are binary32, C++'s are binary64)
//   * multi-component swizzles  v.xyz -> v.sw<0,1,2>(),  v.xy = e -> v.swr<0,1>() = e
//   * `in` / `out` / `inout` / precision qualifiers in parameter lists
//   * identifiers that are C++ keywords are renamed
//   * the tagged-line filter of src/gui/scene.rs:1065-1107 (!FOR_NUMBER! etc.)
#pragma once
#include <map>
#include <set>
#include <string>
#include <vector>

namespace ptl {

// Feature switches of the reference's `Data` (src/gui/common.rs:63-86) with the native
// (non-wasm) defaults of src/main.rs:935-941.
struct CodegenFlags {
    bool for_prefer_variable = true;
    bool disable_antialiasing = false;
    bool disable_anaglyph = true;
    bool disable_camera_teleportation = false;
    bool use_300_version = true;
    bool defer_loop_updates = true;  // translate_glsl's deferred loop-carried ray transforms (KernelOptions can switch it off)
};

// Drops (blanks) the lines whose tags are switched off; keeps the line count.
std::string filter_tagged_lines(const std::string& text, const CodegenFlags& flags);

// GLSL snippet -> C++ (line-preserving).
//
// `defer_loop_updates` (default on): one optimisation on the way, exact by construction.  Scene snippets advance rays through a
// pair of portal matrices on EVERY iteration of a loop -- `X = transform(A_mat, transform(B_mat_inv, X));` -- but read X only inside
// nested blocks that few rays enter (where a portal hit is recorded: scenes/portal_in_portal.ron:1146-1147,1157,1178).  Such an
// update is replaced by a counter increment, and the pending updates are applied right before every statement that reads X (and
// behind the loop, if X is read there): the same operations on the same values in the same order for every ray that reads X,
// none for the rays that never do.  Applied only when all of this holds -- otherwise the code is left exactly as written:
//   * the update is a statement of a `for` body (not nested deeper, loop not inside another loop), of the form above: `transform`
//     calls and `*` over X (once) and identifiers that name uniforms (`*_mat`, `*_mat_inv`, `*_mat_teleport`, `*_u`, `_*`) which the
//     snippet never assigns or declares;
//   * every other occurrence of X in the loop body sits in a nested block, is not an assignment target, and X does not appear in
//     the loop header.
// `force_inline_definitions`: the text is a file-scope library (scene.rs:1037-1044) -- its function definitions get PTL_FN like every other function
// of the kernel.  Without it they are plain inline members that LLVM's bottom-up inliner happens to inline and its module inliner does not
// (a call with `this` then keeps the tracer object in scratch).
std::string translate_glsl(const std::string& glsl, bool defer_loop_updates = true, bool force_inline_definitions = false);

// (glsl_masks.cpp)  What the values a build compiles in do to a snippet, on the output of translate_glsl and line-preserving like it.
// Token shapes, so white space, comments and line breaks between their tokens do not matter, and comment text is never touched.
//   * `masked`: the matrix uniforms whose zero / unit pattern the build knows (KernelOptions::mask_zero_elements).  The calls that multiply
//     by one of them get their masked forms (device/ptl_glsl.h):
//       transform ( M ,    -> ptl_transform_m<PTL_MASK_M>(M,                  (`transform` a name of its own, not a member)
//       M * <operand>      -> ptl_mul_m<PTL_MASK_M>(M, <operand>)            (`(b0_mat_inv * pos).z`; the deferred loop updates' own text)
//     M is the whole left operand: not a member, nothing multiplicative (`*`, `/`, `%`) and no unary sign in front of it, and `*` is not
//     `*=`.  The operand is one unary expression -- a parenthesised group, or a name with its call `(..)`, index `[..]`, member `.m`
//     (`.sw<..>()`) and `->m` suffixes -- that starts with neither a sign nor a digit; the walk goes on inside it, so `A * (B * v)` nests.
//     ptl_mul_m falls back to the plain product for anything but a vec4.  Every other use of the matrix (behind a sign, copied into a
//     local, handed to a function) keeps the full chain: correct, just not shortened.
//   * `unroll_bounds`: the Int uniforms baked into the build.  `for (int I = 0; I < B; I++) {` with one of them, 2 <= B <= 16, as its
//     bound gets `_Pragma("unroll")` in front; `*unrolled` receives how many loops did.
std::string specialize_translated(const std::string& cxx, const std::set<std::string>& masked, const std::map<std::string, int>& unroll_bounds, int* unrolled = nullptr);
// The masked spelling of a callee that multiplies by matrix M: `callee<PTL_MASK_M>`, and `ptl_transform_m<PTL_MASK_M>` for `transform`.
std::string masked_callee(const std::string& callee, const std::string& matrix);

// Refuses (std::runtime_error) a scene in which passing `out` / `inout` arguments by reference could differ from GLSL's copy in /
// copy out: a mutable global handed to a function that also names it, or one variable handed to two out parameters of a call.
// `sources`: file-scope GLSL (the scene's library); `bodies`: statement lists that call into it (material / object / intersection snippets).
void check_out_argument_aliasing(const std::vector<std::string>& sources, const std::vector<std::string>& bodies);

// The caller's distance bound inside an intersection-material snippet (KernelOptions::bound_snippets).  The bounce loop takes the nearest
// of scene_intersect() and the scene's snippets (src/frag.glsl:114-125); a snippet candidate farther than the hit scene_intersect() has
// already found can never be that nearest hit, yet the snippets of the reference's scenes spend most of their time deciding whether such
// candidates lie inside a portal (scenes/portal_in_portal.ron:1133-1191: ten nested copies of two portals, each with an O(copy) walk).
// For a snippet of the shape
//     SceneIntersectionWithMaterial R = SceneIntersectionWithMaterial(scene_intersection_none, material_empty());
//     ... if (nearer(R.scene.hit, H)) { ... R.scene = process_portal_intersection(R.scene, H, ...); ... R.material = ...; } ...
//     return R;
// every such condition becomes `nearer(R.scene.hit, H) && !(H.t > ptl_far)` (`ptl_far`: a new parameter of the snippet function).
// Exact by construction: with S_k the accumulator of the snippet as written after block k and T_k the bounded one's, T_k = S_k whenever
// S_k.t <= ptl_far and "no hit" otherwise (induction over the blocks: a candidate within the bound meets the same `nearer` verdict in
// both, one beyond it is accepted as written only when the accumulator holds no nearer hit -- and a hit beyond the bound loses against
// scene_intersect()'s in the caller either way).  Applied only when the token stream shows that nothing else can carry a skipped block's
// effect out of it: R appears only in the declaration, the conditions, `R.scene = process_{portal,plane}_intersection(R.scene, H, ..)`,
// `R.scene.material ==/!=`, `R.material =` and the final `return R;`; a block assigns only R and its own locals, calls no function with
// out / inout parameters, and stores R.material itself whenever it may leave CUSTOM_MATERIAL behind (the one case in which the caller reads
// it).  The caller additionally requires that no GLSL of the scene names TELEPORT_SUBSPACE / in_subspace: process_portal_intersection never
// resets SceneIntersection::in_subspace, so with subspace portals a skipped candidate could leave that flag behind.  Returns the text
// unchanged (and *bounded = 0) when any of this fails.
std::string bound_nearer_blocks(const std::string& glsl_body, const std::set<std::string>& functions_with_out_params, int* bounded);

// (glsl_affine.cpp)  A scene uniform that holds a matrix, by its name: `X_mat`, `X_mat_inv`, `A_to_B_mat_teleport` (scene.rs:424-543).
bool is_scene_matrix_name(const std::string& name);

// Do the scene's GLSL snippets keep rays affine?  True unless one of them builds a Ray from parts that are not spelled `vec4(.., 1.)` /
// `vec4(.., 0.)`, assigns a ray's `.o` / `.d` in another than a whitelisted form, calls transform() with a matrix that is not a scene uniform
// (`X_mat`, `X_mat_inv`, `A_to_B_mat_teleport`: the ones whose values are checked), or has an out / inout parameter of type Ray or vec4
// (KernelOptions::affine_rays; conservative: a refusal only costs the optimisation).  `why` receives the offending text.
bool snippets_keep_rays_affine(const std::vector<std::string>& codes, std::string* why);

}  // namespace ptl
