/* portal_amd.h -- C ABI of libportal_amd.so, the MI355X backend for optozorax/portal scenes.
 *
 * Two layers, both plain C (pointers and sizes only):
 *
 *  1. ptl_kernel_*  -- the drop-in boundary.  Replaces exactly what the reference asks of
 *     macroquad/miniquad for its trace shader:
 *         load_material(ShaderSource::Glsl{..}, MaterialParams{uniforms, textures})
 *                                                   src/gui/scene.rs:1132-1143  -> ptl_kernel_compile
 *         material.set_uniform(name, value)         src/gui/scene.rs:587-588,624-632,641-649,
 *                                                   src/main.rs:1269-1358      -> ptl_kernel_set_uniform
 *         material.set_texture(name, texture)       src/main.rs:1077-1078      -> ptl_kernel_set_texture
 *         render_target(w,h) + gl_use_material + draw_rectangle(0,0,w,h)
 *                                                   src/main.rs:1041-1042,1424-1425 -> ptl_kernel_render
 *         texture.get_texture_data()                src/main.rs:2939-2943      -> ptl_kernel_render_to_host
 *     A Rust host binds these with `extern "C"` (INTEGRATION.md shows the stub).
 *
 *  2. ptl_scene_* / ptl_renderer_*  -- the host side above that boundary, written in C++
 *     because no Rust toolchain exists in the build image: .ron loader, uniform/matrix
 *     evaluator, scene -> HIP source generator, and the SceneRenderer driver
 *     (src/main.rs:934-1064,1266-1359,1411-1428).  Python (portal_amd/__init__.py), the CLI and
 *     the tests call this layer through ctypes.
 *
 * Threading: a handle is not thread-safe; different handles may be used from different threads
 * (one per GPU).  Every function returns 0 on success unless stated otherwise.
 */
#ifndef PORTAL_AMD_H
#define PORTAL_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ---------------------------------------------------------------------- */
#define PTL_OK 0
#define PTL_UNKNOWN_UNIFORM 1 /* set_uniform: the kernel has no such uniform; ignored, like macroquad */
#define PTL_ERR_INVALID (-1)
#define PTL_ERR_COMPILE (-2) /* hiprtc diagnostics are in the log buffer */
#define PTL_ERR_HIP (-3)     /* HIP runtime call failed; see ptl_last_error() */
#define PTL_ERR_TYPE (-4)    /* set_uniform: type differs from the declared one */
#define PTL_ERR_SCENE (-5)   /* scene file / evaluation error */
#define PTL_ERR_NO_DEVICE (-6)

/* Last error message of the calling thread ("" if none). */
const char* ptl_last_error(void);

/* Library / toolchain description: "portal_amd <ver>; hip=<path>; hiprtc=<path>". */
const char* ptl_version(void);

/* Number of HIP devices visible (0 when the HIP runtime cannot be loaded). */
int ptl_device_count(void);

/* ---- layer 1: kernel handle ---------------------------------------------------------------- */
typedef struct ptl_kernel ptl_kernel;

typedef enum { PTL_MAT4 = 0, PTL_F32 = 1, PTL_I32 = 2, PTL_VEC2 = 3, PTL_VEC3 = 4, PTL_SAMPLER = 5 } ptl_type;

typedef struct {
    const char* name;
    ptl_type type;
    size_t offset; /* byte offset in the kernel's `ptl_uniform_block` (see ptl_scene_uniform_layout) */
} ptl_uniform_desc;

/* Compile `hip_source` (a translation unit produced by ptl_scene_generate_source, or written
 * by hand against the same conventions) for `device` with hiprtc and load it.
 *   uniforms/n_uniforms : every uniform of the block incl. samplers, with offsets
 *   defines/n_defines   : preprocessor symbols, e.g. "PTL_COUNT_SEGMENTS"
 *   log/log_cap         : receives the hiprtc log (NUL-terminated, truncated to fit)
 * device = -1 compiles only (no GPU needed): the handle can then only be queried with
 * ptl_kernel_code_object. */
int ptl_kernel_compile(int device, const char* hip_source, const ptl_uniform_desc* uniforms, int n_uniforms,
                       size_t uniform_block_size, const char* const* defines, int n_defines, ptl_kernel** out, char* log,
                       size_t log_cap);

/* A second instance of a compiled kernel on the same device: the code object loaded once more, so it has a uniform block of its own and
 * can be in flight on another stream with other uniform values (one module's block is a single global: consecutive launches of ONE handle
 * with different uniforms serialise on the upload).  Nothing is compiled.  ptl_kernel_copy_uniforms hands the original's current values
 * (sampler records included: the clone reads the original's texel buffers, so the original must outlive it) to the clone.  What
 * ptl_renderer_set_option("concurrent_draws", K) is built on. */
int ptl_kernel_clone(ptl_kernel* src, ptl_kernel** out);
int ptl_kernel_copy_uniforms(ptl_kernel* dst, const ptl_kernel* src);
/* The compiled gfx950 code object (valid until ptl_kernel_destroy). */
int ptl_kernel_code_object(ptl_kernel* k, const void** data, size_t* size);

/* Kernel metadata of a gfx950 code object (ptl_kernel_code_object, or a file of the code-object cache) without a device: the largest value of
 * `key` (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".sgpr_count") over the kernels whose name starts with
 * `kernel_prefix` (NULL or "": every kernel of the module); -1 when the key does not occur -- and, with a prefix, for a key that sorts before
 * ".name" (".kernarg_segment_size", ".group_segment_fixed_size" ...: the per-kernel attribution reads the metadata map in its alphabetical key
 * order and is only right behind ".name").  The JIT's occupancy retry decides on the render
 * entries alone ("ptl_render"): the one-wave teleport and prologue entries of a one-module build say nothing about the render kernel. */
int ptl_code_object_note(const void* code, size_t size, const char* key, const char* kernel_prefix);
/* Per-lane resources of the loaded render kernel (hipFuncGetAttribute): vector registers, scratch
 * (private segment) bytes -- non-zero means register spills that travel through the memory hierarchy --
 * and static LDS bytes per workgroup.  -1 where the runtime cannot tell.  A compile-only handle (device -1) answers from the
 * code object's metadata: the largest values over its render entries. */
int ptl_kernel_resources(ptl_kernel* k, int* registers, int* scratch_bytes, int* lds_bytes);

/* value points at 16 floats (column-major) / 1 float / 1 int32 / 2 floats / 3 floats. */
int ptl_kernel_set_uniform(ptl_kernel* k, const char* name, ptl_type type, const void* value);

/* RGBA8 texels, row 0 first, are copied to device memory; sampled bilinear, clamp-to-edge. */
int ptl_kernel_set_texture(ptl_kernel* k, const char* sampler, const uint8_t* rgba8, int width, int height);

/* Row-block sharding of one frame: the frame is cut into blocks of 8 pixel rows; this launch
 * renders blocks phase, phase+stride, phase+2*stride, ...  (1 GPU: phase 0, stride 1). */
typedef struct {
    int width, height;       /* full frame, used for the pixel -> ray mapping */
    int rb_phase, rb_stride; /* row-block interleave */
    int in_place;            /* 0: the shard's rows are stored packed, in block order (out = shard_rows*width pixels);
                              * 1: the out pointers address a FULL frame (height*width pixels) and every row is stored at its
                              *    own position -- N launches with phase 0..N-1 fill one buffer between them, which may be
                              *    another GPU's memory mapped with ptl_ipc_open */
} ptl_frame;

/* Rows rendered by a shard (with in_place = 0 they are stored packed, in block order, in the output buffers). */
int ptl_frame_shard_rows(const ptl_frame* f);

/* Launch on `stream` (a hipStream_t, NULL = default stream).  Outputs are DEVICE pointers, either
 * may be NULL: out_rgba8 = shard_rows*width*4 bytes, out_rgba32f = shard_rows*width*16 bytes
 * (frame->in_place: height*width*4 and height*width*16 bytes).
 * segments (DEVICE pointer to one uint64, may be NULL) accumulates bounce-loop trips when the
 * kernel was compiled with PTL_COUNT_SEGMENTS.  If elapsed_ms is non-NULL the launch is bracketed
 * by HIP events on `stream` and the call waits for completion. */
int ptl_kernel_render(ptl_kernel* k, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* segments,
                      void* stream, float* elapsed_ms);

/* Convenience: render the shard and copy it to HOST buffers (either may be NULL). */
int ptl_kernel_render_to_host(ptl_kernel* k, const ptl_frame* frame, uint8_t* host_rgba8, float* host_rgba32f,
                              uint64_t* host_segments, float* elapsed_ms);
/* Slices: ONE launch for several frames that differ in their uniforms only (the motion-blur sub-frames of a clip frame, src/main.rs:1798).
 * A source generated with flag bit 22 (PTL_FLAG_SLICES) has the render entry `ptl_render_slices_kernel`, which reads the uniform block of
 * slice blockIdx.z from a device buffer of blocks instead of the module's one global -- through the same scalar loads -- and writes slice z's
 * frame behind slice z - 1's.  ptl_kernel_stage_slice(k, j) makes the values set so far (ptl_kernel_set_uniform ...) slice j of the next
 * batch; ptl_kernel_render_slices uploads slices 0 .. n-1 with one copy, runs the prologue of every slice and launches once with
 * grid.z = n: slice z lands at out_rgba8 + z * slice_pixels pixels (out_rgba32f + 4 * z * slice_pixels floats; either may be NULL).  The
 * ramp and tail of a small frame (~10 us of a 50 us 1080p launch) overlap with its neighbours' instead of adding up.  A single
 * ptl_kernel_render of such a module is a batch of one; the camera-teleport query keeps using the module's own block.
 * ptl_kernel_max_slices: 16 for such a module, 0 otherwise. */
int ptl_kernel_max_slices(ptl_kernel* k);
int ptl_kernel_stage_slice(ptl_kernel* k, int index);
/* ... or a block saved earlier (ptl_kernel_snapshot_uniforms: the host copy of the uniform block, ptl_kernel_uniform_block_size bytes), also one
 * saved from ANOTHER kernel of the same scene -- every build of a scene has the same block layout.  A sampler record that names a texel buffer
 * of `k` itself (bound now, or bound when the block was taken) is kept; any other record is replaced by `k`'s current one.
 * Textures and slices: a staged slice names the texel buffers that were bound when it was staged.  Re-binding a sampler
 * (ptl_kernel_set_texture: a video texture stepping to its next frame) between two stage calls does NOT free the buffer the earlier slice
 * reads: it is retired and freed behind the launch.  A caller that keeps snapshots instead of staging at once brackets them with
 * ptl_kernel_hold_textures(k, 1) ... (k, 0) for the same guarantee.
 * A block is only meaningful for a kernel whose compiled-in values agree with it: a value-baked build (flag bits 0 / 2 / 3 / 20) that had to
 * be rebuilt between two stage calls must not trace the earlier blocks -- layer 2 (ptl_renderer_stage_slice / _draw_slices) launches each
 * slice on the kernel it was staged with; a layer-1 caller that rebuilds has to do the same. */
int ptl_kernel_stage_slice_from(ptl_kernel* k, int index, const void* block, size_t size);
int ptl_kernel_hold_textures(ptl_kernel* k, int hold);
size_t ptl_kernel_uniform_block_size(ptl_kernel* k);
int ptl_kernel_snapshot_uniforms(ptl_kernel* k, void* dst, size_t cap);
int ptl_kernel_render_slices(ptl_kernel* k, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels,
                             void* stream, float* elapsed_ms);

/* SceneRenderer::teleport_external_ray (src/main.rs:1361-1409): where does point b end up when the
 * segment a -> b is carried through the scene's portals (at most 10)?  One-thread launch of the
 * kernel's second entry point; synchronous.  teleported = 0 means "no portal crossed" (the
 * reference's `None`), out_pos is then (0,0,0).  Uses whatever uniforms are currently set. */
int ptl_kernel_teleport_ray(ptl_kernel* k, const float a[3], const float b[3], float out_pos[3], int* hit_object,
                            int* changed_subspace, int* teleported);
/* Split builds.  A source compiled with the define PTL_RENDER_MODULE has no teleport entry: that entry is a second copy of the whole
 * tracer, a fifth of every hiprtc build, and a camera that stands still never asks for it.  ptl_kernel_teleport_ray on such a kernel
 * compiles the other half on demand -- the same source with PTL_TELEPORT_MODULE: teleport entry + prologue, no render entry; its code
 * object is cached like any other -- and runs the query there with this kernel's uniform values.  ptl_kernel_prebuild_teleport does the
 * compile ahead of time (on a compile-only handle, device -1: fills the code-object cache).  Kernels compiled without either define
 * have every entry in one module, as before.  ptl_renderer_* builds split (environment PTL_ONE_MODULE=1: one module). */
int ptl_kernel_prebuild_teleport(ptl_kernel* k);

void ptl_kernel_destroy(ptl_kernel* k);

/* ---- layer 2: scene + renderer ------------------------------------------------------------- */
typedef struct ptl_scene ptl_scene;
typedef struct ptl_renderer ptl_renderer;

/* Scene::from_serialized(ron::from_str(..)) -- src/main.rs:2882, src/gui/scene.rs:142-146 */
int ptl_scene_load_file(const char* path, ptl_scene** out);
int ptl_scene_load_text(const char* ron_text, ptl_scene** out);
void ptl_scene_free(ptl_scene* s);

/* Override a named uniform's stored value (what a GUI slider / stage does). 1 = no such uniform. */
int ptl_scene_set_uniform(ptl_scene* s, const char* name, double value);
/* Trefoil uniforms in the reference's text form (TrefoilSpecial::decode / encode, src/gui/uniform.rs:23-98; its unit test:
 * "1a 2a G,1b 3b B,2a 1a S" round-trips): part 1a teleports to part 2a and is drawn in colour G, ...  Returns
 * PTL_UNKNOWN_UNIFORM (1) for an unknown name, a uniform of another kind, or text that does not decode. */
int ptl_scene_set_trefoil(ptl_scene* s, const char* name, const char* text);
int ptl_scene_get_trefoil(ptl_scene* s, const char* name, char* text, size_t cap);
/* Formula time inputs (FormulasCache::set_time / set_total_time). */
int ptl_scene_set_time(ptl_scene* s, double time, double total_time);

/* Scene::init_stage_by_name (src/gui/scene.rs:1237-1250, `render-frame --stage`): apply the named
 * animation stage's uniform / matrix overrides.  camera receives the name of the camera the stage
 * selects ("" = the scene's original camera; an inline stage camera is reported as "#<index>").
 * Returns 1 if the scene has no such stage. */
int ptl_scene_init_stage(ptl_scene* s, const char* stage, char* camera, size_t camera_cap);
/* Number of stages / cameras and their names (index past the end: returns 1). */
int ptl_scene_stage_name(ptl_scene* s, int index, char* name, size_t cap);
int ptl_scene_camera_name(ptl_scene* s, int index, char* name, size_t cap);

/* FormulasCache::set_camera_matrix (src/gui/uniform.rs:625-697): what Matrix::Camera evaluates to (column-major
 * binary64).  A renderer sets it to its camera's matrix before every draw (send_camera_object_matrix). */
int ptl_scene_set_camera_matrix(ptl_scene* s, const double m16[16]);
/* Real animations = the clips of the video pipeline (RealAnimation, src/gui/animation.rs:1014-1043).
 * ptl_scene_animation: name and duration (seconds) of clip `index`, 1 past the end.
 * ptl_scene_init_animation: Scene::init_animation_by_name (src/gui/scene.rs:1254-1267): the clip's base stage,
 * then its own replacements, then its start camera becomes the scene's current camera.  1 = no such clip. */
int ptl_scene_animation(ptl_scene* s, int index, char* name, size_t cap, double* duration);
int ptl_scene_init_animation(ptl_scene* s, const char* animation);
/* CalculatedCam (src/gui/camera.rs:22-32); matrix is column-major binary64 */
typedef struct ptl_calculated_cam {
    double look_at[3], alpha, beta, r;
    int free_movement, in_subspace, override_matrix;
    double matrix[16];
} ptl_calculated_cam;
/* Scene::update (src/gui/scene.rs:1353-1493): map wall-clock `seconds` to the formulas' `time` (fraction of the
 * current clip) and `total_time`, and compute the clip's interpolated camera ("OverrideCam") when it has a start
 * and an end camera (*has_cam = 1). */
int ptl_scene_update(ptl_scene* s, double seconds, double* time, double* total_time, int* has_cam, ptl_calculated_cam* cam);

/* AnyUniform::get: kind 0 = bool, 1 = int, 2 = float.  Returns 1 if the uniform cannot be evaluated. */
int ptl_scene_eval_uniform(ptl_scene* s, const char* name, int* kind, double* value);
/* Matrix::get as binary64, column-major.  Returns 1 if it cannot be evaluated. */
int ptl_scene_eval_matrix(ptl_scene* s, const char* name, double out16[16]);
/* Scene `cam` block: look_at xyz, alpha, beta, r, offset_after_material. */
int ptl_scene_cam(ptl_scene* s, double out7[7]);

/* Texture `index` of the scene: name ("monoportal") and path ("scenes/img/monoportal.png").
 * Returns 1 when index is past the end. */
int ptl_scene_texture(ptl_scene* s, int index, char* name, size_t name_cap, char* path, size_t path_cap);

/* ---- generation / renderer flags (the bits are described below, at ptl_scene_generate_source) ---- */
#define PTL_FLAG_SPECIALIZE_INTS (1u << 0)
#define PTL_FLAG_COUNT_SEGMENTS (1u << 1)
#define PTL_FLAG_SPECIALIZE_ALL (1u << 2)
#define PTL_FLAG_SPECIALIZE_STATIC (1u << 3)
#define PTL_FLAG_ANAGLYPH (1u << 4)
#define PTL_FLAG_NO_DERIVED_UNIFORMS (1u << 5)
#define PTL_FLAG_FAST_MATH (1u << 6)
#define PTL_FLAG_NO_DEFERRED_UPDATES (1u << 7)
#define PTL_FLAG_WAVES_SHIFT 8 /* bits 8-11: occupancy hint n, (n & 0xF) << PTL_FLAG_WAVES_SHIFT */
#define PTL_FLAG_NO_UNIFORM_HOIST (1u << 12)
#define PTL_FLAG_NO_FIRST_TRIP (1u << 13)
#define PTL_FLAG_EXACT_CR (1u << 14)
#define PTL_FLAG_NO_UNROLL (1u << 15)
#define PTL_FLAG_NO_FIRST_TRIP_PLANES (1u << 16)
#define PTL_FLAG_ASYNC_REJIT (1u << 17)
#define PTL_FLAG_QUICK_JIT (1u << 18)
#define PTL_FLAG_NO_ZERO_MASKS (1u << 19)
#define PTL_FLAG_SPECIALIZE_PATTERNS (1u << 20)
#define PTL_FLAG_BOUNDED_SNIPPETS (1u << 21)
#define PTL_FLAG_SLICES (1u << 22)
#define PTL_FLAG_NO_AFFINE_RAYS (1u << 23)
#define PTL_FLAG_KEEP_TRANSFORM_DODGES (1u << 24)
#define PTL_FLAG_CHECK_AFFINE (1u << 25)
#define PTL_FLAG_MATERIAL_TABLE_LDS (1u << 26)
#define PTL_FLAG_MATERIAL_TABLE_SCALAR (1u << 27)
#define PTL_FLAG_REFINE (1u << 28)
#define PTL_FLAG_REFINE_SLICES (1u << 29)
#define PTL_FLAG_PASSES (1u << 30)

/* Scene::generate_shader_code: returns a malloc'ed NUL-terminated HIP C++ source (free with
 * ptl_free).  flags: bit0 = bake Bool/Int scene uniforms as literals, bit1 = count segments,
 * bit2 = bake every scene uniform (ints, floats, matrices; camera and other builtins stay dynamic),
 * bit3 = clip-constant specialisation: bake every scene uniform whose evaluation reads no per-frame input (time,
 * total_time, the camera matrix) -- what stays fixed while a clip plays; a renderer checks the compiled-in values before
 * every draw and rebuilds (demoting what moved) if one no longer holds, so results never depend on the guess.
 * A RENDERER built with bit0, bit2 or bit3 also compiles its own mode switches in -- "use_panini_projection", "use_360_camera",
 * "use_180_camera", "draw_depth_map", "draw_anaglyph", "draw_side_by_side": the camera models and output modes a frame does not use
 * are then not in the kernel at all (7-10 % of the kernel time) -- and rebuilds when ptl_renderer_set_option flips one (counted by
 * ptl_renderer_rejit_count; the code-object cache keeps both).  ptl_scene_generate_source leaves them run-time values,
 * bit4 = compile the anaglyph stereo mode in (the reference's `disable_anaglyph = false`, src/main.rs:939),
 * bit5 = NO derived uniforms: by default the ray-independent half of every generated plane test whose matrix is a run-time
 * uniform (normalize(get_normal(X_mat)), both possible is_collinear verdicts) is evaluated once per uniform upload by the
 * module's prologue kernel `ptl_derive_kernel` and read back as extra uniforms -- same operations, identical frames;
 * this bit keeps the reference's per-call form (A/B measurements, tests),
 * bit14 = EXACT CR (`--exact-cr`): numerics contract 1 of rounds 1-2 -- `/`, 1/x and sqrt IEEE correctly rounded on every input --
 * instead of contract 2 (device/ptl_glsl.h: 1/x correctly rounded with the extremes flushed, a / b = a * (1/b), sqrt correctly rounded
 * with |x| < 2^-100 flushed); both are bit-exact against the oracle run with the same contract,
 * bit6 = FAST MATH, the tolerance mode (`--fast`): hardware rcp / sqrt / rsq estimates (1 ulp), a / b = a * rcp(b), FMA
 * contraction, plane tests as t = -o'.z * rcp(d'.z) without normalising the transformed direction, products with a literal zero folded
 * (-fno-signed-zeros -fno-honor-nans: with the scene state baked in, most portal matrices are mostly zeros).  Frames agree with the exact kernel to ~1e-6 per channel except at pixels where the last bit decides a path
 * (object edges); the exact kernel stays the default and the parity reference.
 * bit7 = NO deferred loop updates: by default a loop-carried ray transform in a scene snippet (`X = transform(A_mat, transform(B_mat_inv, X));`
 * on every iteration, X read only where a hit is recorded) is replaced by a counter and applied right before X is read -- the same
 * operations on the same values for the rays that read X, none for the others; identical frames (glsl_translate.h has the conditions).
 * bit12 = NO hoisted uniform work: by default every expression of a scene snippet that depends on run-time uniforms alone
 * (`b0_mat * (a_mat_inv * normal_b)`, `d_mat * c_mat_inv`, normalize() of such a normal ...), loop-carried chains of them
 * included, is computed by the prologue kernel of bit5 into members behind the derived uniforms, and the snippet reads it
 * from there -- the same expression text compiled in the same module, identical frames (host/glsl_hoist.h).  Off with bit5.
 * bit13 = NO first-trip variants: with the first-trip forms (below: every specialised build; the un-specialised kernel with bit24) every intersection-material snippet is compiled twice, and
 * the copy that runs while a ray still starts at the camera (the first trip of the bounce loop: nine trips in ten) takes the ORIGIN half of its
 * `transform(uniform matrix, ray)` chains from the prologue kernel -- the origin of every primary ray is the same uniform value --
 * while the direction half stays per ray; same operations on the same values, identical frames.  Off with bit5 / bit12.
 * bit16 = NO first-trip form of the generated plane tests: with the first-trip forms, where the scene's matrices are
 * run-time uniforms, a second copy of scene_intersect serves the trip on which every ray of a wave still starts at the camera and takes
 * `plane_inv * r.o` of every Flat object from the prologue kernel (ptl_dvo_<object>_<side>) -- the same product of the same values, identical frames.
 * Round 6: in the UN-SPECIALISED kernel (none of bit0 / bit2 / bit3 / bit20) both first-trip forms are opt-in (bit24).  Rounds 3-5 built them in
 * every kernel; the un-specialised one loses with either -- headline 0.697 -> 0.664 ms without them (-3 ... -9 % over five views), triple_portal
 * 0.445 -> 0.434, mobius 1.108 -> 1.046, monoportal equal (profiles/r06/ab_unspec_code_size*.jsonl) -- and is 12 535 instead of 17 090 instructions
 * and compiles in a quarter of the time.  The specialised builds keep them as before (the plane form still gains 1 ... 4 % in the patterns and
 * Int-baked builds, profiles/r06/ab_first_trip_planes.jsonl; the snippet copies go where rays are affine, bit24).
 * bit17 = ASYNC REJIT (read by ptl_renderer_create only; the "specialize_static" option may be switched on such a renderer: the pair
 * of kernels is rebuilt synchronously, like at creation): see ptl_renderer_rejit_pending.
 * bit18 = QUICK JIT: compile at -O1 instead of the shipped -O3 without SLP: half the hiprtc time for a 5-20 % slower kernel, identical
 * frames -- for a build that is wanted now and used briefly (the CLI's render-frame; the kernel a clip starts on).  Implies bit15;
 * ignored together with bit3 (a clip-constant build is asked for because many frames follow).
 * bit19 = NO ZERO MASKS: by default a build with bit0, bit2 or bit3 compiles in the ZERO PATTERN of every matrix uniform that stays a
 * run-time value (only Bool / Int baked; animated within the clip -- its pattern then taken over probes of the clip's `time`; demoted):
 * `transform(X_mat, ..)` of the scene snippets and the generated plane tests skip the terms whose element is zero, as a baked matrix's do
 * (same results for finite operands); a renderer rebuilds when a masked element stops being zero.  Since round 4 the pattern also names the
 * elements that are exactly +1 or -1 (their terms become `x + acc` / `acc - x`: the same operation, no bit moves), with the same rebuild rule.
 * This bit keeps the full products (A/B),
 * bit20 = SPECIALIZE PATTERNS: no animated VALUE of the scene is compiled in, only what survives while the values move -- the zero / unit
 * patterns of the matrix uniforms (as with bit19 clear), in a renderer its mode switches, and (round 5) the scene's own switches: the Bool /
 * Int uniforms whose evaluation reads no per-frame input (GUI toggles and counters such as `filter_teleported`, `show_teleported`; dead
 * branches, constant loop bounds and unrolled snippet loops follow: headline 0.50 -> 0.30 ms).  The kernel for scenes whose uniforms move
 * every frame (the reference uploads them every frame and never recompiles, src/main.rs:1266-1359): a renderer rebuilds only when a matrix
 * element leaves its pattern (then without masks, at most once per stage), a switch flips (the one that moved becomes a run-time uniform)
 * or a matrix stops being affine (bit23); with bit17 the un-specialised kernel draws meanwhile.
 * bit21 = BOUNDED SNIPPETS (opt-in): the bounce loop evaluates scene_intersect() first and hands its hit distance to the scene's
 * intersection-material snippets; a snippet of the usual shape (an accumulator filled in `if (nearer(result.scene.hit, H)) { ... }` blocks)
 * then skips the candidates beyond it, which could never be the nearest hit -- exact by construction (host/glsl_translate.h
 * `bound_nearer_blocks` has the proof and the conditions), identical frames.  Off by default: on the headline scene it measures -2 ... +13 %
 * kernel time over five views (profiles/r04/ab_bounded_snippets.jsonl),
 * bit22 = SLICES: the render entry takes its uniform block from a buffer of blocks, one per blockIdx.z (ptl_kernel_render_slices /
 * ptl_renderer_draw_slices: one launch for the blur sub-frames of a clip frame).  Same arithmetic, same scalar loads, identical frames; a
 * single draw is a batch of one,
 * bit23 = NO AFFINE RAYS: by default (round 5) a build that may shorten products (bit0, bit2, bit3 or bit20; not with bit14 / bit6) whose scene
 * matrices all have the bottom row 0 0 0 1 -- or are NaN throughout: a switched-off object -- and whose snippets never write a ray's w says in
 * its matrix-times-ray products what every ray of the reference satisfies anyway: an origin has w = 1, a direction w = 0.  The translation
 * column then costs a direction nothing and the w row folds to a constant (headline kernel -16 %); the same operations on the same values
 * for finite rays, identical frames.  A renderer rebuilds without it when a matrix -- the camera's included -- stops being affine.
 * This bit keeps the general products (A/B measurements, tests),
 * bit26 = MATERIAL TABLE IN LDS, bit27 = MATERIAL TABLE BEHIND SCALAR LOADS (round 6, A/B; both measured and left off): the reference prints one
 * `else if (i.material == X_M) return material_simple2(hit, r, <nine literals>);` per Simple material (src/gui/scene.rs:736-760).  With one of these bits
 * the nine literals of every Simple material (and of DEBUG_RED / GREEN / BLUE) sit in a table indexed by the material id and ONE call of
 * material_simple2 serves them all -- bit26: the table staged in LDS per workgroup, two ds_read_b128 per lane; bit27: the table in constant memory,
 * one scalar load per DISTINCT material of the wave (a readfirstlane loop), the grid flags on the scalar unit.  Same function, same argument
 * values: identical frames.  Headline 0.1869 ms without, 0.1905 (LDS) / 0.1872 (scalar); C2 0.0369 / 0.0383 / 0.0376; C3 0.2133 / 0.2118 / 0.2086
 * (profiles/r06/ab_material_table2.jsonl): a wave usually holds ONE material and its own copy with the literals folded beats a generic body.
 * bit25 = CHECK AFFINE (round 6, diagnostics): never affine rays; the kernel is generated with PTL_CHECK_AFFINE and its `segments` counter (bit1 is
 * implied) counts, instead of bounce-loop trips, the ray halves that reach a matrix-times-ray product or the bounce loop with a w that is
 * not 1 (origin) / 0 (direction) -- what a kernel with affine rays would have assumed wrongly.  Same frames as bit23.  See ptl_renderer_check_affine.
 * bit24 = KEEP TRANSFORM DODGES (A/B): round 4's shape of a kernel.  (a) The un-specialised kernel gets the first-trip forms of bit13 / bit16 (opt-in there
 * since round 6, see there), a kernel with affine rays its first-trip snippet copies.  (b) A kernel with affine rays (bit23 clear and everything affine) is by default generated WITHOUT the deferred loop updates (bit7) --
 * they dodge `transform(uniform matrix, ray)`, which is a handful of additions there and cheaper than the bookkeeping around it (headline baked
 * 0.2305 -> 0.2046 ms, Int-baked 0.272 -> 0.239, patterns 0.274 -> 0.239; identical frames); this bit keeps them.  Kernels without affine rays (the
 * un-specialised one above all: 0.70 against 0.89 ms) keep the deferral anyway,
 * bit28 = REFINE: the module gets a second render entry, `ptl_render_refine_kernel`, which shades a device-side list of pixels instead of a
 * rectangle (ptl_kernel_render_refine, ptl_renderer_draw_adaptive below).  A source generated without it is byte for byte what it was.  Not with bit22,
 * bit30 = PASSES: the tracer keeps a 16-byte record per pixel -- nearest final depth, bounce-loop trips, how its paths ended -- and the render
 * entries store it through one more pointer (ptl_pass_record, ptl_kernel_render_passes below).  Same colours.  A source generated without it is byte
 * for byte what it was.  Not with bit4, bit25, bit28 or bit29 (PTL_ERR_SCENE and a message),
 * bit15 = NO unrolling of baked loops: by default (with bit0) a counting loop of a scene snippet whose bound is a baked Int uniform
 * (<= 16 iterations) is unrolled -- the same operations in the same order, identical frames; every iteration then has its own
 * constants (scenes/portal_in_portal.ron's `size` drives an inner loop and a material index).
 * ptl_renderer_create additionally reads bits 8-11 as an occupancy hint n (0 = none):
 * the kernel is built with __launch_bounds__(256, n), i.e. at least n waves per SIMD. */
int ptl_scene_generate_source(ptl_scene* s, unsigned flags, char** source);
/* The preprocessor defines that belong to the source generated last (ptl_scene_generate_source / ptl_renderer_*), space separated: what
 * ptl_kernel_compile has to be given with it ("PTL_FIRST_TRIP", "PTL_DROP_ZERO_TERMS" -- absent when a matrix of the scene is infinite or
 * NaN: shortened products are exact for finite vectors only, so such a scene keeps every full chain -- "PTL_COUNT_SEGMENTS" ...). */
int ptl_scene_generated_defines(ptl_scene* s, char* out, size_t cap);
/* Diagnostics: how often a generation with zero patterns (bit0 / bit2 / bit3 without bit19) probed the scene for them (copies of the scene
 * stepped through the clip) and how often it reused the last result because the state the patterns depend on had not changed -- a renderer
 * with baked Bool / Int uniforms regenerates on every camera move. */
int ptl_scene_zero_mask_probes(ptl_scene* s, int* reused, int* probed);
/* Scene::uniforms + layout: descs are owned by the scene handle and stay valid until the next
 * call of this function or ptl_scene_free. */
int ptl_scene_uniform_layout(ptl_scene* s, const ptl_uniform_desc** descs, int* n, size_t* block_size);
/* Scene::set_uniforms: evaluate and upload X_mat / X_mat_inv / *_mat_teleport / user uniforms. */
int ptl_scene_set_uniforms(ptl_scene* s, ptl_kernel* k);
/* The same values without a kernel (tests): callback per uniform. */
typedef void (*ptl_uniform_cb)(void* user, const char* name, ptl_type type, const void* value);
int ptl_scene_visit_uniforms(ptl_scene* s, ptl_uniform_cb cb, void* user);
/* Which scene element produced generated line `line` (1-based) of the last generated source:
 * kind/name are written into caller buffers.  Returns 1 if the line is template text. */
int ptl_scene_source_line_owner(ptl_scene* s, int line, char* kind, size_t kind_cap, char* name, size_t name_cap,
                                int* local_line);
void ptl_free(void* p);

/* SceneRenderer::new (src/main.rs:934-1064): generate + compile + upload scene uniforms and
 * textures (paths are resolved against `asset_root`).  device = -1: no GPU, only
 * ptl_renderer_uniform_* queries work. */
int ptl_renderer_create(ptl_scene* s, int device, const char* asset_root, unsigned flags, ptl_renderer** out, char* log,
                        size_t log_cap);
/* The same with renderer options (ptl_renderer_set_option names, "specialize_static" excluded) applied BEFORE the first build: a
 * specialised renderer (flags bit0 / bit2 / bit3) compiles its mode switches in, so a caller that draws side by side, with Panini, a
 * 360 camera ... gets the kernel it will draw with from the start -- and a compile-only handle (device = -1) warms the code-object cache
 * with exactly that kernel (`portal-amd render --stereoimage` prefetches its clips' kernels this way).  An unknown name is
 * PTL_ERR_INVALID. */
int ptl_renderer_create_with_options(ptl_scene* s, int device, const char* asset_root, unsigned flags, const char* const* option_names,
                                     const double* option_values, int n_options, ptl_renderer** out, char* log, size_t log_cap);
/* CLI / GUI knobs of SceneRenderer, by the reference's field names: "render_depth", "aa_count",
 * "aa_start", "view_angle", "use_panini_projection", "panini_param", "use_360_camera",
 * "use_180_camera", "darken_by_distance", "gray_t_start", "gray_t_size", "draw_depth_map",
 * "depth_map_min", "depth_map_max", "angle_color_disable", "grid_disable",
 * "black_border_disable", "offset_after_material", "draw_side_by_side"; "adaptive_aa_threshold" (ptl_renderer_draw_adaptive). */
/* The translation unit the renderer's current kernel was compiled from (malloc'ed, free with ptl_free): ptl_scene_generate_source's text
 * with the renderer's own mode switches compiled in where it is a specialised build -- what tools/isa_hist.py attributes instructions to. */
int ptl_renderer_kernel_source(ptl_renderer* r, char** source);
int ptl_renderer_set_option(ptl_renderer* r, const char* name, double value);
/* "concurrent_draws" K (1 = off, up to 8; round 4): draws issued with stream = NULL / the caller's stream and without a request for the
 * kernel time go round-robin to K internal streams, each with its own instance of the kernel (ptl_kernel_clone), so consecutive draws with
 * DIFFERENT uniforms -- the motion-blur sub-frames of a clip frame (src/main.rs:1798) -- overlap on the GPU instead of serialising on the one
 * uniform block a module has.  Each launch waits for what the caller's stream had queued when it was issued; nothing waits for the launches
 * until ptl_renderer_join(r, stream), which puts `stream` (NULL = the default stream) behind all of them -- call it before the frames are
 * consumed (averaged, downloaded).  Timed draws, counting draws, draws to host memory and the teleport query join by themselves.
 * Identical frames (tests/test_gpu_round2.py); measured on one MI355X it buys nothing (profiles/r04/concurrent_draws.jsonl: 1080p
 * 0.0519 ms per sub-frame with one instance, 0.0522 with two, 0.0559 with four) -- the cross-stream waits cost what the overlap saves --
 * so nothing switches it on by default.
 * "lane_fence" 0 (round 6; default 1): a draw on a lane is the kernel's packet and nothing else -- the launch does NOT wait for what the
 * caller's stream holds, and no event is recorded behind it (a lane's completion event is recorded when ptl_renderer_join or a host-side
 * wait asks for it).  The caller orders the reuse of a target itself: ptl_renderer_join before a target is read or drawn into again.
 * With two lanes and a target per lane this is two frames in flight -- frame n + 1's ramp under frame n's tail -- for a caller that queues
 * frames and looks at them later (`bench.py`'s timed region at one GPU; profiles/r06/two_streams.jsonl: headline 4K 0.187 -> 0.177 ms per
 * frame, monoportal 1080p 0.035 -> 0.027, identical bytes).
 * "lane_stagger_us" T (default 0): lanes that start together stay together -- two launches queued at the same moment share the chip evenly and
 * drain at the same moment, so only one drain per PAIR is hidden.  With T > 0 the first draw of every lane but the first, counted from the last
 * ptl_renderer_join (or host-side wait), is issued T x 2 / K microseconds after the previous lane's: a host-side spin while the GPU is busy with
 * the first launch.  Half a launch is the natural T (bench.py sets it; profiles/r06/stagger.jsonl: 20-frame batches 0.1823 -> 0.180 ms per 4K frame). */
int ptl_renderer_join(ptl_renderer* r, void* stream);
/* One launch for several draws of a renderer created with flag bit 22 (PTL_FLAG_SLICES): ptl_renderer_stage_slice does everything a draw
 * does short of launching -- camera, rebuild checks, uniform evaluation for `frame` -- and keeps the resulting uniform block as slice `index`;
 * ptl_renderer_draw_slices launches slices 0 .. n-1 at once (ptl_kernel_render_slices).  Between two stage calls: ptl_renderer_update,
 * ptl_renderer_set_option("aa_start", j), camera moves ... as between two draws.  A slice is a snapshot of the uniform block TOGETHER WITH the
 * kernel it was staged with: when the kernel is rebuilt between two stage calls (a value-baked build whose value moved, a mode switch, an
 * adopted background build) the earlier slices are still traced by the earlier kernel -- draw_slices then issues one launch per run of
 * slices that share a kernel, same frames as draws one by one -- and the texel buffers a slice names (a video texture that steps between
 * two sub-frames) live until its launch.  draw_slices without slices 0 .. n-1 staged since the last launch is PTL_ERR_INVALID.
 * draw_slices is asynchronous like a draw EXCEPT when a kernel was rebuilt or a video texture stepped between two stage calls: it then releases
 * the parked kernels and retired texel buffers behind its launches, which waits for those launches (hipFree / the kernels' completion events);
 * on an error return `elapsed_ms` covers only the runs launched so far. */
int ptl_renderer_stage_slice(ptl_renderer* r, const ptl_frame* frame, int index);
int ptl_renderer_draw_slices(ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels,
                             void* stream, float* elapsed_ms);
/* Camera (RotateAroundCam): look_at xyz, alpha, beta, r. */
int ptl_renderer_set_camera(ptl_renderer* r, const double look_at[3], double alpha, double beta, double radius);
/* `render-frame --camera NAME` (src/main.rs:2918-2926, 1442-1478): take look_at / alpha / beta / r /
 * in_subspace / free_movement / teleport matrix from a named scene camera ("#<index>" for an inline stage
 * camera); "" restores the scene's `cam` block.  Returns 1 if there is no such camera. */
int ptl_renderer_use_camera(ptl_renderer* r, const char* camera);
/* The value draw_texture would upload for a builtin or scene uniform (floats; ints as 1 float). */
int ptl_renderer_uniform_value(ptl_renderer* r, int width, int height, const char* name, float out16[16], int* n_values);
/* SceneRenderer::draw_texture (src/main.rs:1411-1428): scene.set_uniforms + set_uniforms(w,h) +
 * one launch.  Same output conventions as ptl_kernel_render. */
int ptl_renderer_draw(ptl_renderer* r, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* segments,
                      void* stream, float* elapsed_ms);
int ptl_renderer_draw_to_host(ptl_renderer* r, const ptl_frame* frame, uint8_t* host_rgba8, float* host_rgba32f,
                              uint64_t* host_segments, float* elapsed_ms);
/* The same through the renderer: uploads scene + builtin uniforms as teleport_external_ray does
 * (set_uniforms(0,0), teleport_light_u = 1), then ptl_kernel_teleport_ray. */
int ptl_renderer_teleport_ray(ptl_renderer* r, const double a[3], const double b[3], double out_pos[3], int* hit_object,
                              int* changed_subspace, int* teleported);
/* Build (or load from the cache) the teleport half of the renderer's current kernel now instead of at the first query. */
int ptl_renderer_prebuild_teleport(ptl_renderer* r);
/* Move the camera the way the interactive reference does every frame: set the new orbit parameters, then
 * SceneRenderer::teleport_camera (src/main.rs:1217-1264): if the straight segment from the previous camera
 * position to the new one crosses a portal, the camera's teleport matrix becomes the portal map's
 * finite-difference Jacobian (teleport_matrix, src/main.rs:1174-1215; four ray queries) so that the view
 * continues seamlessly on the other side.  *teleported = 1 if that happened, *blocked = 1 if the move was
 * undone (stop_at_objects, or no Jacobian could be formed).  ptl_renderer_set_camera, by contrast, *places*
 * the camera without looking for a crossing. */
int ptl_renderer_move_camera(ptl_renderer* r, const double look_at[3], double alpha, double beta, double radius, int* teleported,
                             int* blocked);
/* SceneRenderer::update (src/main.rs:1430-1538), the per-frame step of `render` and `render-frame`:
 * ptl_scene_update(seconds); Matrix::Camera := the camera's matrix; switch to / follow the scene's current
 * camera; apply the clip's interpolated camera; if the camera matrix moved, teleport_camera (portal crossing). */
int ptl_renderer_update(ptl_renderer* r, double seconds, int* teleported, int* blocked);

/* Current teleport matrix (binary64, column-major), subspace flag and world position of the camera. */
int ptl_renderer_camera_state(ptl_renderer* r, double teleport16[16], int* in_subspace, double position[3]);
ptl_kernel* ptl_renderer_kernel(ptl_renderer* r);
/* The binary64 primitives behind the scene's constants, exposed one by one for tests (tests/test_matrix_exact.py compares each with exact
 * arithmetic): op = "inverse" (a), "mul" (a * b), "teleport" (b * a^-1: `A_to_B_mat_teleport`, src/gui/scene.rs:624-632), "srt" (a = scale
 * xyz, b = rotate xyz, c = offset xyz: Matrix::Simple / Parametrized, src/gui/matrix.rs:555-569), "camera" (a = look_at xyz, alpha, beta, r;
 * b = the teleport matrix: RotateAroundCam::get_matrix, src/main.rs:278-304).  Matrices are 16 doubles, column-major. */
int ptl_dmath(const char* op, const double* a, const double* b, const double* c, double* out);
/* 1 when the renderer's current kernel was generated with affine rays (flag bit23 clear, a build that may shorten products, every scene
 * matrix and the camera affine, no snippet that writes a ray's w): its matrix-times-ray products spell o.w = 1 / d.w = 0.  A matrix or a
 * camera that stops being affine makes the next draw rebuild without it (counted by ptl_renderer_rejit_count); 0 then, and for every other build. */
int ptl_renderer_affine_rays(ptl_renderer* r);
/* Round 6 -- the dynamic belt behind that decision (the reference has nothing to check: `transform` multiplies all four components,
 * /root/reference/src/library.glsl:95-120).  Builds the checking kernel of the renderer's CURRENT state (flag bit25: general products, every
 * place an affine-rays kernel assumes a w counts the ray halves that arrive with another one), draws width x height with the renderer's camera
 * and options, and reports the count.  A count above zero on a renderer whose kernel has affine rays switches them off for the stage and
 * rebuilds (ptl_renderer_rejit_count goes up, ptl_last_error says why); its frames were and stay those of the general products only from then on.
 * Needs a device.  The renderer option "check_affine" = 1 (or PTL_CHECK_AFFINE=1 in the environment) runs this at 64 x 36 before the first
 * draw with every new affine-rays source; `portal-amd check` runs it when a GPU is present. */
int ptl_renderer_check_affine(ptl_renderer* r, int width, int height, unsigned long long* violations);
/* The scan behind that decision, exposed for tests: 1 when the GLSL text keeps rays affine (no Ray built from halves whose w is not spelled
 * `vec4(.., 1.)` / `vec4(.., 0.)`, no `.o` / `.d` assigned in another than the whitelisted forms, no out / inout parameter of type Ray or
 * vec4, no transform() by a matrix that is not a scene uniform), 0 with the offending text in `why`, -1 on malformed input (ptl_last_error).
 * Round 6: a whitelist over EVERY write to a ray half (x / y / z alone, or the whole half in five spelled forms), no preprocessor directive, no
 * out / inout parameter of any type, no modf / frexp, no `ray_none` (codegen.cpp; hunted by tests/test_affine_guard_fuzz.py). */
int ptl_snippets_keep_rays_affine(const char* glsl, char* why, size_t why_cap);
/* how many times a draw had to rebuild a specialised kernel since the renderer was created: a clip-constant value that moved (flags bit3),
 * a mode switch that was flipped (flags bit0 / bit2 / bit3) */
int ptl_renderer_rejit_count(ptl_renderer* r);
/* flags bit17 (ASYNC REJIT) on a specialised renderer (bits 0/2 or 3): a draw that finds its compiled-in values stale does not wait for
 * the rebuild (1-3 s of hiprtc) -- it draws with the un-specialised kernel of the scene (every build draws the same bits) while a worker
 * thread compiles the specialised source of the current state; the first draw that finds it finished and still matching loads it and
 * switches (counted by ptl_renderer_rejit_count).  Returns 1 while such a build is in flight or the un-specialised kernel is in use.
 * Reference seam: the reference recompiles its shader synchronously when the scene changes (src/gui/scene.rs:1112-1176). */
int ptl_renderer_rejit_pending(ptl_renderer* r);
void ptl_renderer_destroy(ptl_renderer* r);

/* Place the packed rows of shard (phase, stride) into a full-frame RGBA8 image (host memory). */
int ptl_deinterleave_rows(const uint8_t* shard_rgba8, const ptl_frame* frame, uint8_t* full_rgba8);

/* average_images (src/main.rs:645-722), the motion-blur step of the video pipeline, on the GPU: N RGBA8
 * sub-frames (DEVICE pointers, 16-byte aligned, any width x height) -> one RGBA8 frame:
 * per channel mean of c*c over the sub-frames (integer division), then (u8)(sqrt(mean) + 0.5); alpha = 255.
 * HBM-bound: reads 4*N bytes and writes 4 bytes per pixel.  1 <= n_frames <= 256 (up to 64 the pointers travel in the kernel
 * arguments, beyond in a device table; 256 is where the exact one-multiply integer mean ends: 65025 * 256 * 256 < 2^32).  (For one image the reference
 * hands it back untouched; callers skip the call then -- the kernel would still force alpha to 255.)  Launched on `stream`;
 * with elapsed_ms != NULL it is bracketed by HIP events and the call waits. */
int ptl_average_images(int device, const void* const* frames_rgba8, int n_frames, void* out_rgba8, int width, int height, void* stream,
                       float* elapsed_ms);

/* The same averaging fused with the conversion to what a video encoder consumes: N RGBA8 sub-frames -> one planar Y'CbCr 4:2:0
 * 10-bit frame (BT.709 matrix on the gamma-encoded values, full range), the payload of one Y4M frame.  The averaged RGBA8 frame is
 * never written: the kernel reads 4*N bytes and writes 3 bytes per pixel.
 * Contract: let A(x, y) = (R, G, B) be the RGBA8 frame ptl_average_images would have written for n_frames >= 2; for n_frames == 1
 * (a plain RGBA8 -> YUV conversion) the input's own RGB.  Alpha is ignored.  All arithmetic is 32-bit integer:
 *   Y  = (55896 R + 188037 G + 18982 B + 32768) >> 16                                        per pixel
 *   S_c = sum over dy = 0, 1 of A_c(2i-1, 2j+dy) + 2 A_c(2i, 2j+dy) + A_c(2i+1, 2j+dy)        coordinates clamped to the frame
 *   Cb = min(1023, (-30123 S_R - 101335 S_G + 131458 S_B + (512 << 19) + (1 << 18)) >> 19)
 *   Cr = min(1023, (131458 S_R - 119404 S_G -  12054 S_B + (512 << 19) + (1 << 18)) >> 19)
 * i.e. H.273 Y = round(1023 E'y), C = round(1023 E'pb) + 512 with coefficients round(K * 1023 / 255 * 2^16), chroma sited like
 * MPEG-2 ("left": co-sited with luma column 2i, weights 1-2-1; the mean of rows 2j and 2j+1).
 * Layout of out_yuv (DEVICE pointer, 16-byte aligned, ptl_yuv420p10_frame_bytes(w, h) = 2 (W H + 2 cw ch) bytes): the Y plane, W*H
 * little-endian uint16, row 0 on top; then Cb and Cr, cw*ch each, cw = (W+1)/2, ch = (H+1)/2.  Any width, height >= 1 (W*H <= 2^29).
 * Validation, stream and timing are those of ptl_average_images.  There is no host-side conversion. */
int ptl_average_to_yuv420p10(int device, const void* const* frames_rgba8, int n_frames, void* out_yuv, int width, int height, void* stream,
                             float* elapsed_ms);
size_t ptl_yuv420p10_frame_bytes(int width, int height);
/* Deep colour: the same frame made from the UN-QUANTISED sub-frames, so that its 10 bits carry 10 bits of signal (the frame above is a
 * function of 8-bit values: a 1024-step grey ramp gives 256 luma codes there, 1024 here).  Input: n_frames (1 .. 256) RGBA32F sub-frames
 * (DEVICE pointers, 16-byte aligned, W*H pixels of four binary32 values) as the out_rgba32f argument of any render call writes them:
 * gamma-2 encoded values, alpha ignored.  ONE quantisation, to 16 bits, per channel value v of a sub-frame (unorm8's rule at 16 bits):
 *   q(v) = 0 if !(v > 0) (NaN, -0, negatives), 65535 if v >= 1 (+inf), else (u32) floor(v * 65535.0f + 0.5f)
 * with the product and the sum each rounded to binary32 (no fused multiply-add).  Integers from there on, per pixel and channel:
 *   M = floor((sum over the sub-frames of q^2) / n)           (64-bit: the sum stays below 2^40)
 *   E = the integer e with e (e - 1) < M <= e (e + 1)         (= floor(sqrt(M) + 1/2); E = 0 for M = 0; for n = 1, E = q)
 * A(x, y) = (E_R, E_G, E_B), 16-bit gamma-encoded.  BT.709 on these, full range, 10 bit, siting and layout as above:
 *   Y  = (13920 E_R + 46826 E_G + 4727 E_B + (1 << 21)) >> 22                                 per pixel, unsigned 32-bit
 *   S_c = sum over dy = 0, 1 of A_c(2i-1, 2j+dy) + 2 A_c(2i, 2j+dy) + A_c(2i+1, 2j+dy)         coordinates clamped (0 .. 524 280)
 *   Cb = min(1023, (-15003 S_R - 50470 S_G + 65473 S_B + (512 << 26) + (1 << 25)) >> 26)      64-bit; both accumulators stay positive
 *   Cr = min(1023, ( 65473 S_R - 59470 S_G -  6003 S_B + (512 << 26) + (1 << 25)) >> 26)
 * (coefficients round(K * 1023 / 65535 * 2^22); every grey q gives Y = round(1023 q / 65535) and Cb = Cr = 512; within 0.53 codes of the
 * real-valued H.273 definition).  out_yuv: ptl_yuv420p10_frame_bytes(w, h) bytes, the layout above; the Y4M header is the same.
 * Any width, height >= 1 with W*H <= 2^28 (a sub-frame is addressed with 32-bit byte offsets).  Validation, stream and timing are
 * those of ptl_average_to_yuv420p10.  (`portal-amd render --frames y4m --deep-colour`.) */
int ptl_average_f32_to_yuv420p10(int device, const void* const* frames_rgba32f, int n_frames, void* out_yuv, int width, int height, void* stream,
                                 float* elapsed_ms);
/* The same two frames with another chroma sampling, `chroma` = PTL_CHROMA_420, _422 or _444.  The averaged frame A(x, y),
 * the luma formula, the plane order and the full-range 10-bit coding stay what they are above: for RGBA8 sub-frames those of
 * ptl_average_to_yuv420p10, for RGBA32F sub-frames those of ptl_average_f32_to_yuv420p10 (q, M, E).  Only the chroma planes change:
 *   chroma  cw       ch       S_c
 *   422     (W+1)/2  H        A_c(2i-1, y) + 2 A_c(2i, y) + A_c(2i+1, y)     co-sited with luma column 2i (as 4:2:0 is horizontally), columns
 *                                                                            clamped to the frame, nothing vertical
 *   444     W        H        A_c(x, y)
 * RGBA8 sub-frames, 32-bit integers, k = 18 for 422 and 16 for 444 (the 4:2:0 form above is k = 19):
 *   Cb = min(1023, (-30123 S_R - 101335 S_G + 131458 S_B + (512 << k) + (1 << (k-1))) >> k)
 *   Cr = min(1023, (131458 S_R - 119404 S_G -  12054 S_B + (512 << k) + (1 << (k-1))) >> k)
 * RGBA32F sub-frames, 64-bit integers, k = 25 for 422 and 23 for 444 (the 4:2:0 form above is k = 26):
 *   Cb = min(1023, (-15003 S_R - 50470 S_G + 65473 S_B + (512 << k) + (1 << (k-1))) >> k)
 *   Cr = min(1023, ( 65473 S_R - 59470 S_G -  6003 S_B + (512 << k) + (1 << (k-1))) >> k)
 * Every accumulator stays positive (minima 261 640 and 65 410, 33 554 180 and 8 388 545), so >> is a plain shift; pure blue and pure red
 * reach exactly 1024 before the min and nothing exceeds it; every grey gives 512; within 0.51 codes of the real-valued H.273 definition.
 * out_yuv: the Y plane (W*H little-endian uint16), then Cb, then Cr (cw*ch each) = ptl_yuv10_frame_bytes(w, h, chroma) =
 * 2 (W H + 2 cw ch) bytes: 4 bytes per pixel at 422 and 6 at 444 for even W.  The stream header names the sampling
 * (ptl_y4m_header_chroma).  chroma == PTL_CHROMA_420 IS the entry above: same kernel, same bytes.  Validation, limits (W*H <= 2^29 for
 * RGBA8, <= 2^28 for float sub-frames), stream and timing are those of ptl_average_to_yuv420p10; any other `chroma` is PTL_ERR_INVALID.
 * (`portal-amd render --frames y4m --chroma 420|422|444 [--deep-colour]`.) */
#define PTL_CHROMA_420 420
#define PTL_CHROMA_422 422
#define PTL_CHROMA_444 444
int ptl_average_to_yuv10(int device, const void* const* frames_rgba8, int n_frames, void* out_yuv, int width, int height, int chroma, void* stream,
                         float* elapsed_ms);
int ptl_average_f32_to_yuv10(int device, const void* const* frames_rgba32f, int n_frames, void* out_yuv, int width, int height, int chroma, void* stream,
                             float* elapsed_ms);
size_t ptl_yuv10_frame_bytes(int width, int height, int chroma); /* 0 for an unknown chroma */
/* The same averaged frame as RGB: N RGBA32F sub-frames -> the scanlines of one 16-bit PNG (colour type 2, bit depth 16), unfiltered or with
 * PNG's Sub filter already applied, so that the host only deflates them (ptl_png_write_rgb48 below).  Unfiltered 16-bit rows
 * hardly compress (a 1080p frame: 8.1 MB at deflate level 3, 2.1 MB with Sub), so the filter is part of the hot path, and the kernel applies
 * it, with the byte order, while the values are in registers.
 * Contract (tests/png16_reference.py restates it in numpy).  A(x, y) = (E_R, E_G, E_B) is exactly the averaged frame of
 * ptl_average_f32_to_yuv420p10 above: q per channel value of a sub-frame, M = floor(sum q^2 / n), E = floor(sqrt(M) + 1/2); for n = 1,
 * E = q.  Alpha is ignored.  Raw row y, bytes 6x .. 6x+5:
 *   E_R >> 8, E_R & 255, E_G >> 8, E_G & 255, E_B >> 8, E_B & 255                    big-endian samples
 * `filter` selects the transform of the raw rows:
 *   PTL_PNG_FILTER_NONE (0)  out = raw
 *   PTL_PNG_FILTER_SUB  (1)  out[y][i] = (raw[y][i] - (i >= 6 ? raw[y][i - 6] : 0)) mod 256     per byte, no borrow between bytes; every
 *                                                                                                row starts from zero
 * out_rows: DEVICE pointer, 16-byte aligned, H rows of 6 W bytes, packed = ptl_rgb48_frame_bytes(w, h) = 6 W H bytes.  There are no
 * filter-type bytes: the writer adds them (rows stay 8-byte aligned for W % 4 == 0).  Any width, height >= 1 with W*H <= 2^28 (a sub-frame
 * is addressed with 32-bit byte offsets).  HBM-bound: reads 16 N and writes 6 bytes per pixel, the traffic of the 4:4:4 form above.
 * 1 <= n_frames <= 256; validation, stream and timing are those of ptl_average_f32_to_yuv10; any other `filter` is PTL_ERR_INVALID before
 * any GPU call.  (`portal-amd render --png-depth 16`, `portal-amd render-frame --png-depth 16`.) */
#define PTL_PNG_FILTER_NONE 0
#define PTL_PNG_FILTER_SUB 1
int ptl_average_f32_to_rgb48(int device, const void* const* frames_rgba32f, int n_frames, void* out_rows, int width, int height, int filter, void* stream,
                             float* elapsed_ms);
size_t ptl_rgb48_frame_bytes(int width, int height); /* 6 W H; 0 for a size that is not positive */

/* ---- trace passes: what the tracer knows about a pixel beside its colour (opt-in, flag bit 30) ------------------------------------------
 * A source generated with PTL_FLAG_PASSES keeps one record per pixel while it traces and stores it through one more pointer of the render
 * entry, `out_passes`, addressed exactly like out_rgba32f (16 bytes per pixel, one 16-byte store per lane; rb_phase / rb_stride / in_place are
 * honoured; in the slices entry slice z lands behind slice z - 1, at out_passes + z * slice_pixels records).  A "path" is one call of the
 * tracer's bounce loop: one per anti-aliasing sample of the window `_aa_start` .. `_aa_start + _aa_count - 1`.  Every path of a pixel ends in
 * exactly one of four ways, so final + escaped + exhausted + outside = `_aa_count`:
 *   final      a final material ended it (the result has a depth),
 *   escaped    it left the scene (the sky colour; black inside a subspace),
 *   exhausted  it was still alive when the bounce loop reached `_ray_tracing_depth` trips -- the pixel is drawn black for this sample, and
 *              nothing else says so; a path that ends ON trip `_ray_tracing_depth` is final or escaped, never exhausted,
 *   outside    the sample never traced: it lies in the black bars of a 360 / 180 degree frame.
 * The four counts saturate at 65 535.  depth_near is a minimum (taken with `<`, so a NaN depth never enters it) and the rest are integers:
 * every field is exact, the host build of the same source (ptl_host_render_passes) gives the same bytes, and with PTL_FLAG_COUNT_SEGMENTS also
 * on, the launch's segment sum equals the sum of `trips`.  Colours are those of the build without the flag.  Generation refuses bit 30
 * together with PTL_FLAG_ANAGLYPH (two paths per sample), PTL_FLAG_REFINE / _REFINE_SLICES (the list-driven entries store no records) and
 * PTL_FLAG_CHECK_AFFINE.  Without the flag, sources and code objects are byte for byte what they were. */
typedef struct ptl_pass_record {
    float depth_near;           /* min over the pixel's FINAL paths of path length / max(camera scale, 1e-6); +inf if it has none */
    uint32_t trips;             /* bounce-loop trips over all paths of the pixel (what PTL_FLAG_COUNT_SEGMENTS sums per launch) */
    uint32_t final_escaped;     /* low 16 bits: final paths; high 16: escaped paths */
    uint32_t exhausted_outside; /* low 16 bits: exhausted paths; high 16: outside samples */
} ptl_pass_record;
size_t ptl_pass_record_bytes(int width, int height); /* 16 W H; 0 for a size that is not positive */
/* ptl_kernel_render and ptl_kernel_render_slices with the records: out_passes is a DEVICE pointer, 16-byte aligned, of passes_bytes bytes --
 * at least 16 bytes per pixel the launch stores: shard_rows * width records (frame->in_place: height * width), for slices
 * (n - 1) * slice_pixels more.  Refused before any GPU call (PTL_ERR_INVALID, ptl_last_error): a kernel generated without bit 30, a null or
 * misaligned pointer, a buffer that is too small.  The plain calls still work on such a kernel and store no records. */
int ptl_kernel_render_passes(ptl_kernel* k, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes, void* segments,
                             void* stream, float* elapsed_ms);
int ptl_kernel_render_slices_passes(ptl_kernel* k, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes,
                                    unsigned long long slice_pixels, void* stream, float* elapsed_ms);
/* Layer 2: ptl_renderer_draw and ptl_renderer_draw_slices with the records, for a renderer created with PTL_FLAG_PASSES or switched with the
 * option "passes" = 1 (ptl_renderer_set_option: the flag joins the next build, which happens at once; 0 takes it out again; a combination the
 * generator refuses leaves the renderer as it was).  A pass draw goes on the caller's stream after joining the lanes ("concurrent_draws"), as
 * a timed draw does.  Frame groups draw no records: ptl_frame_group_create refuses the flag and ptl_frame_group_set_option the option. */
int ptl_renderer_draw_passes(ptl_renderer* r, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes, void* segments,
                             void* stream, float* elapsed_ms);
int ptl_renderer_draw_slices_passes(ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes,
                                    unsigned long long slice_pixels, void* stream, float* elapsed_ms);
/* ptl_pass_stats: one sweep over n records (DEVICE pointer, 16-byte aligned) added into a ptl_pass_stats_block in DEVICE memory that the
 * caller zeroed once (hipMemset) -- a clip keeps one block on the card, adds the launch behind every draw and downloads it at its end.
 * per_launch (DEVICE pointer to uint64 counters the caller zeroed, or NULL): per_launch[slot] receives the exhausted paths of THIS sweep,
 * so the worst frame of a clip can be named.  Integers only; the result does not depend on the order of the adds.  Launched on `stream`;
 * with elapsed_ms the call waits.  HBM-bound: 16 bytes per record in.  n <= 2^31. */
#define PTL_PASS_HIST_BINS 256
typedef struct ptl_pass_stats_block {
    uint64_t pixels, paths, trips;                   /* records seen, their paths (the four counts added up), their trips */
    uint64_t final_paths, escaped, exhausted, outside;
    uint64_t exhausted_pixels;                       /* records with at least one exhausted path */
    uint32_t max_trips;                              /* the largest `trips` of a record */
    /* the range of depth_near over the records where it is finite, as order-preserving keys (depths need not be positive): zero = none yet.
     * key(bits) = bits has the sign bit ? ~bits : bits | 0x80000000; depth_max_key = the largest key, depth_min_key_inv = the largest ~key.
     * ptl_pass_stats_depth_range decodes both. */
    uint32_t depth_max_key, depth_min_key_inv;
    uint32_t reserved;
    uint64_t trips_histogram[PTL_PASS_HIST_BINS];    /* records by `trips`; the last bin collects trips >= 255 */
} ptl_pass_stats_block;
int ptl_pass_stats(int device, const void* records, long n, void* stats_block, void* per_launch, int slot, void* stream, float* elapsed_ms);
/* HOST copy of a block -> the smallest and largest finite depth_near; returns 1, or 0 (and leaves lo / hi alone) when no record had one */
int ptl_pass_stats_depth_range(const ptl_pass_stats_block* block, float* lo, float* hi);
/* ptl_passes_to_gray16: n records -> the scanlines of a 16-bit greyscale PNG (colour type 0, bit depth 16, filter None: 2 n bytes, big-endian
 * samples, rows packed without filter-type bytes), `which`:
 *   PTL_PASS_DEPTH  a record without a final path gives 0; otherwise q((depth_near - lo) / max(1e-6f, hi - lo)): difference, divisor and ONE
 *                   IEEE division in binary32, then q of ptl_average_f32_to_yuv420p10 (0 if !(v > 0), 65535 if v >= 1, else
 *                   (u32) floor(v * 65535.0f + 0.5f), product and sum each rounded to binary32) -- round(65535 clamp(., 0, 1)).
 *                   The renderer's defaults for lo / hi are its "depth_map_min" / "depth_map_max" options.
 *   PTL_PASS_TRIPS  min(trips, 65535): lossless up to there; lo and hi are ignored.
 * records, out_rows: DEVICE pointers, 16-byte aligned.  Any other `which`: PTL_ERR_INVALID before any GPU call.  HBM-bound: 16 bytes in,
 * 2 out.  ptl_png_write_gray16 adds the filter-type bytes and deflates (`level` 0 .. 9), like ptl_png_write_rgb48.
 * (`portal-amd render-frame --passes depth,trips`.) */
#define PTL_PASS_DEPTH 0
#define PTL_PASS_TRIPS 1
int ptl_passes_to_gray16(int device, const void* records, long n, void* out_rows, int which, float lo, float hi, void* stream, float* elapsed_ms);
int ptl_png_write_gray16(const char* path, const uint8_t* rows, int width, int height, int level);
/* ptl_pass_slices_to_gray16: the pass images of ONE output frame of a clip from the records of its n_slices blur sub-frames, in one sweep.
 * records: DEVICE pointer, 16-byte aligned; slice z of pixel p is the ptl_pass_record at index z * slice_records + p -- the layout
 * ptl_renderer_draw_slices_passes writes.  out_depth, out_trips, out_cut: DEVICE pointers, 16-byte aligned, 2 n bytes each, the packed
 * big-endian samples ptl_passes_to_gray16 writes and ptl_png_write_gray16 reads; any of them may be NULL (that image is not made), not all.
 * Per pixel, over the slices z = 0 .. n_slices - 1, exact integers unless said otherwise:
 *   depth  F_z = final paths of slice z (low 16 bits of final_escaped).  0 where every F_z is 0.  Otherwise D starts as depth_near of the
 *          lowest-numbered slice with F_z > 0, and every later slice with F_z > 0 replaces D where its depth_near < D (so a NaN that came
 *          first stays); a slice without a final path is never read for depth.  Sample = q((D - lo) / max(1e-6f, hi - lo)), the binary32
 *          difference, divisor, ONE IEEE division and quantisation of PTL_PASS_DEPTH.  With n_slices = 1: ptl_passes_to_gray16(PTL_PASS_DEPTH)
 *          for every bit pattern.
 *   trips  min(sum of trips_z, 65535), the sum exact.  With n_slices = 1: ptl_passes_to_gray16(PTL_PASS_TRIPS).
 *   cut    E = sum of exhausted_z, P = sum of final_z + escaped_z + exhausted_z (outside samples do not count).  0 where P = 0, else
 *          ceil(65535 E / P): 0 exactly where no path was cut, at least 1 wherever one was, 65535 where every traced path was (and, being
 *          a ceiling, where fewer than P / 65535 survived: only beyond 65 535 paths per pixel).
 * Refused before any GPU call (PTL_ERR_INVALID, ptl_last_error): null records, all three outputs NULL, a pointer that is not 16-byte
 * aligned, n_slices outside 1 .. 256, n outside 1 .. 2^31, slice_records < n with n_slices > 1.  Launched on `stream`; with elapsed_ms the
 * call waits.  HBM-bound: 16 n_slices bytes in, 2 per image out.  (`portal-amd render --clip-passes depth,trips,cut`,
 * `render-frame --passes cut`.) */
int ptl_pass_slices_to_gray16(int device, const void* records, int n_slices, unsigned long long slice_records, long n, void* out_depth, void* out_trips,
                              void* out_cut, float lo, float hi, void* stream, float* elapsed_ms);
/* ---- adaptive anti-aliasing: supersample only the pixels that sit on an edge (opt-in, approximate by design) ------------------------
 * Every anti-aliasing sample costs a full trace, and most pixels of a frame are flat walls and smooth gradients whose centre sample is
 * already the final 8-bit colour.  An adaptive draw traces ONE sample per pixel, classifies the frame it got, and traces the full
 * `aa_count` only where a pixel differs from a neighbour.  Contract, integers only (tests/adaptive_reference.py restates it in numpy):
 *   P = the RGBA8 frame ptl_renderer_draw writes for the current state with `_aa_count` = 1,
 *   F = the frame it writes with `_aa_count` = N, the renderer's "aa_count" option (`_aa_start` and everything else unchanged),
 *   T = an integer in -1 .. 255, the renderer option "adaptive_aa_threshold" (default 4),
 *   d(x, y)      = max over dx, dy in {-1, 0, 1}, c in {R, G, B} of | P(clamp(x+dx), clamp(y+dy)).c - P(x, y).c |
 *   refine(x, y) = d(x, y) > T
 *   out(x, y)    = refine(x, y) ? F(x, y) : P(x, y)
 * Coordinates clamp to the frame; alpha is ignored; `out` covers the RGBA8 bytes and, where asked for, the RGBA32F bits (byte for byte
 * those of F and P: a pixel's value does not depend on which lanes share its wave).  T = -1 refines everything (out == F), T = 255
 * nothing (out == P); with N = 1 the call is a plain draw and the list is empty.  What the method cannot see: a feature thinner than a
 * pixel that the centre samples of a whole 3x3 neighbourhood miss stays at its one-sample colour (DESIGN.md 2.6 has the measured counts).
 *
 * ptl_aa_edges: the classification alone.  frame_rgba8 = W*H RGBA8 pixels, list = room for W*H uint32, count = one uint32 -- all DEVICE
 * pointers, 4-byte aligned.  Writes the indices y*W + x of the refined pixels as a dense list and their number; the count is reset on
 * `stream` by the call itself.  The order of the list is free, but entries produced together are spatial neighbours (a 64x32 region per
 * workgroup, 8x8 tile after 8x8 tile), so 64 consecutive entries still make a compact bundle of rays.  W*H <= 2^31.
 * ptl_kernel_render_refine: the kernel's second render entry (sources generated with PTL_FLAG_REFINE, bit 28) shades the *count pixels of
 * `list` with the uniforms set now and stores each into the FULL frame at out_rgba8 / out_rgba32f (either may be NULL).  The count is
 * read on the device: no host read-back, no synchronisation.  `segments` as in ptl_kernel_render.
 * Both validate their arguments before any GPU call (PTL_ERR_INVALID): null pointers, sizes <= 0, W*H > 2^31, T outside -1 .. 255, a
 * sharded or in-place frame (rb_stride != 1, rb_phase != 0, in_place), a kernel without the refine entry.  Stream and timing as in
 * ptl_average_images / ptl_kernel_render. */
int ptl_aa_edges(int device, const void* frame_rgba8, int width, int height, int threshold, void* list, void* count, void* stream,
                 float* elapsed_ms);
int ptl_kernel_render_refine(ptl_kernel* k, const ptl_frame* frame, const void* list, const void* count, void* out_rgba8, void* out_rgba32f,
                             void* segments, void* stream, float* elapsed_ms);
/* ptl_renderer_draw_adaptive: one adaptive draw of a renderer created with PTL_FLAG_REFINE (without it: PTL_ERR_INVALID and a message).
 * Everything a draw does before its launch runs ONCE; then pass 1 with `_aa_count` 1, the classification of out_rgba8 (required), and
 * the refine pass with `_aa_count` N go on the caller's stream, behind a join of the lanes.  One kernel serves both passes -- `_aa_count`
 * is a run-time builtin in every build -- so no rebuild falls between them; a background rebuild (PTL_FLAG_ASYNC_REJIT) is adopted before
 * or after the draw, never in between.  elapsed_ms: the sum of the three launches' GPU times (the call then waits after each;
 * ptl_renderer_adaptive_times hands out the three).  Whole frames only; frame groups and slices (PTL_FLAG_SLICES cannot be combined
 * with PTL_FLAG_REFINE) are out of scope.
 * ptl_renderer_adaptive_result: the list and the count of the last adaptive draw, DEVICE pointers owned and reused by the renderer,
 * ordered on that draw's stream and valid until the next adaptive draw or destroy.
 * (Adaptive draws of a batch of slices: PTL_FLAG_REFINE_SLICES and ptl_renderer_draw_slices_adaptive below.) */
int ptl_renderer_draw_adaptive(ptl_renderer* r, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* stream, float* elapsed_ms);
int ptl_renderer_adaptive_result(ptl_renderer* r, void** list, void** count);
int ptl_renderer_adaptive_times(ptl_renderer* r, float ms3[3]); /* pass 1, classification, refine pass of the last TIMED adaptive draw */

/* ---- adaptive anti-aliasing of a batch of slices: the motion-blur sub-frames of a clip frame (opt-in, approximate by design) --------
 * A source generated with flag bit 29 (PTL_FLAG_REFINE_SLICES) is the PTL_FLAG_SLICES source (the flag implies the slices entry) plus ONE
 * more entry, `ptl_render_refine_slices_kernel`: the refine entry over the slices of a launch.  Bit 29 cannot be combined with bit 28.
 * Contract, integers only, PER SLICE: for slice z of a batch of n (1 .. 16) take the state staged for it (uniforms, camera, `_aa_start`,
 * textures as bound when it was staged).  P_z = the RGBA8 frame ptl_renderer_draw_slices writes for slice z with `_aa_count` = 1, F_z =
 * the one it writes with the staged `_aa_count` = N, T = the option "adaptive_aa_threshold";  out_z = where(refine(P_z), F_z, P_z) with
 * `refine` the rule above applied to each slice ON ITS OWN (a frame's border clamps to that frame).  RGBA8 bytes and, where asked for,
 * RGBA32F bits.  T = -1: out_z == F_z; T = 255: out_z == P_z; every staged N = 1: a plain ptl_renderer_draw_slices with all counts 0.
 * The averaging kernels (ptl_average_images, ptl_average_to_yuv420p10) consume out_z unchanged.
 *
 * ONE LIST PER SLICE (lists + z * list_stride entries, counts[z] entries used), not one merged list with the slice packed into the
 * entry: every lane of a workgroup then shades with the same uniform block, the block pointer stays workgroup-uniform and the uniform
 * reads stay scalar loads -- what the slices entry exists for.
 *
 * ptl_aa_edges_slices: the classification of ptl_aa_edges over a stack of n frames in one launch, grid (ceil(W/64), ceil(H/32), n).
 * Slice z reads frames_rgba8 + z * slice_pixels pixels, appends to lists + z * list_stride and counts in counts[z]; counts[0 .. n) are
 * reset on `stream` by the call itself.  PTL_ERR_INVALID before any GPU call: null pointers or pointers that are not 4-byte aligned, n
 * outside 1 .. 16, sizes <= 0, W*H > 2^31, slice_pixels < W*H, list_stride < W*H, T outside -1 .. 255.
 * ptl_kernel_set_staged_uniform: one uniform inside the ALREADY STAGED slice `index` (the codes of ptl_kernel_set_uniform; an unknown
 * name is the same no-op code, PTL_UNKNOWN_UNIFORM); PTL_ERR_INVALID for an index outside 0 .. 15 or when nothing is staged.
 * ptl_kernel_render_slices_refine: uploads the staged slices 0 .. n-1 and runs their prologue exactly as ptl_kernel_render_slices does,
 * then launches the entry: slice z shades the counts[z] pixels of lists + z * list_stride (counts read on the device; an entry >= W*H
 * is skipped) into out_* + z * slice_pixels pixels (either output may be NULL).  Grid (gx, 1, n) with gx = min(ceil(W*H / 256), 2048 / n)
 * (integer division): at most 2 048 workgroups per launch, the single-frame entry's 8 per CU, shared evenly by the slices -- a starting
 * rule (profiles/r09).  PTL_ERR_INVALID, in this order: null pointers / sizes <= 0, a sharded or in-place frame, W*H > 2^31,
 * list_stride or slice_pixels < W*H, n outside 1 .. 16, a kernel without the entry, nothing staged; only then PTL_ERR_NO_DEVICE. */
int ptl_aa_edges_slices(int device, const void* frames_rgba8, unsigned long long slice_pixels, int n, int width, int height, int threshold, void* lists,
                        unsigned long long list_stride, void* counts, void* stream, float* elapsed_ms);
int ptl_kernel_set_staged_uniform(ptl_kernel* k, int index, const char* name, ptl_type type, const void* value);
int ptl_kernel_render_slices_refine(ptl_kernel* k, const ptl_frame* frame, int n, const void* lists, unsigned long long list_stride, const void* counts,
                                    void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels, void* segments, void* stream, float* elapsed_ms);
/* ptl_renderer_draw_slices_adaptive: ptl_renderer_draw_slices with adaptive anti-aliasing, for renderers created with
 * PTL_FLAG_REFINE_SLICES (without it: PTL_ERR_INVALID and a message that names the flag).  Three launches per run of slices on the caller's
 * stream, behind a join of the lanes: pass 1 (every slice with `_aa_count` 1), ptl_aa_edges_slices on the sub-frames it wrote, the refine
 * pass (the slices re-staged with their own `_aa_count`).  Nothing is read back and no kernel is rebuilt or adopted between the passes
 * (ptl_renderer_stage_slice did that); consecutive slices staged with the same kernel form a run, and BOTH passes of a run go to the
 * kernel its slices were staged with.  Texel buffers a staged slice names live until behind the refine launch.  PTL_ERR_INVALID before any
 * GPU call: a null out_rgba8 (the classification reads it), anything but a whole frame, slice_pixels < W*H, a threshold outside
 * -1 .. 255, slices 0 .. n-1 not all staged.  elapsed_ms: the sum of all launches; ptl_renderer_adaptive_times then reports the three
 * passes summed over the runs.
 * ptl_renderer_adaptive_slices_result: the lists (n * W*H uint32, list z at z * *list_stride entries) and the counts (16 words) of the
 * last such draw, DEVICE pointers owned and reused by the renderer, ordered on that draw's stream; PTL_ERR_INVALID before the first. */
int ptl_renderer_draw_slices_adaptive(ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels,
                                      void* stream, float* elapsed_ms);
int ptl_renderer_adaptive_slices_result(ptl_renderer* r, void** lists, unsigned long long* list_stride, void** counts);

/* The Y4M stream such frames travel in: "YUV4MPEG2 W<w> H<h> F<fps>:1 Ip A1:1 C420p10 XYSCSS=420P10 XCOLORRANGE=FULL\n" once, then
 * "FRAME\n" + payload per frame.  Writes the header (NUL-terminated) into buf and returns its length; PTL_ERR_INVALID when it does not fit. */
int ptl_y4m_header(int width, int height, int fps, char* buf, size_t cap);
/* The same with the sampling of ptl_average_to_yuv10 named: "... C422p10 XYSCSS=422P10 XCOLORRANGE=FULL\n", "... C444p10 XYSCSS=444P10
 * XCOLORRANGE=FULL\n"; chroma == PTL_CHROMA_420 gives the line above.  PTL_ERR_INVALID for any other chroma. */
int ptl_y4m_header_chroma(int width, int height, int fps, int chroma, char* buf, size_t cap);

/* Device frame buffers for callers that keep frames on the GPU between kernels (sub-frames -> ptl_average_images ->
 * one download); the reference's counterpart is the macroquad render target + Texture2D::get_texture_data()
 * (src/main.rs:1041-1042,1803-1816).  ptl_device_download waits for `stream` first (it is a stream-ordered copy). */
int ptl_device_alloc(int device, size_t bytes, void** out);
int ptl_device_free(void* p);
int ptl_device_download(void* host_dst, const void* device_src, size_t bytes, void* stream);
/* hipMemsetAsync on `stream`: every byte of the range becomes `value` (a ptl_pass_stats_block and its per-launch counters start as zeros). */
int ptl_device_memset(void* device_dst, int value, size_t bytes, void* stream);
/* Streams and events, 1:1 over HIP, for callers that overlap the download of frame i (on its own non-blocking stream, into
 * page-locked memory) with the tracing of frame i+1: record an event behind the producer, make the copy stream wait for it,
 * ptl_device_download_async, record a second event behind the copy and ptl_event_synchronize on it where the pixels are
 * consumed.  (`portal-amd render` does exactly this.) */
int ptl_stream_create(int device, void** stream);
int ptl_stream_destroy(void* stream);
int ptl_event_create(int device, void** event);
int ptl_event_destroy(void* event);
int ptl_event_record(void* event, void* stream);
int ptl_event_synchronize(void* event);
int ptl_stream_wait_event(void* stream, void* event);
int ptl_device_download_async(void* host_dst, const void* device_src, size_t bytes, void* stream);
/* Strided device-to-device copy on `stream` (1:1 over hipMemcpy2DAsync, pitches in bytes).  A rank's packed shard (source pitch =
 * one 8-row block) into another GPU's frame (destination pitch = G blocks; a pointer from ptl_ipc_open or a peer-accessible one):
 * the gather of that shard and its de-interleave in ONE transfer over the rank's own xGMI link. */
int ptl_device_copy2d_async(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t rows, void* stream);
/* A frame buffer shared by the processes of one node (one process per GPU; the reference is single-GPU): the
 * destination rank exports a ptl_device_alloc'ed buffer, the others map it and render into it with ptl_frame.in_place = 1
 * (stores go over xGMI into the destination's HBM).  A handle is PTL_IPC_HANDLE_BYTES opaque bytes to hand to the other
 * processes by any means; it cannot be opened in the exporting process.  Completion is the caller's business (a barrier
 * behind the launches). */
#define PTL_IPC_HANDLE_BYTES 64
int ptl_ipc_export(void* device_ptr, unsigned char handle[PTL_IPC_HANDLE_BYTES]);
int ptl_ipc_open(int device, const unsigned char handle[PTL_IPC_HANDLE_BYTES], void** device_ptr);
int ptl_ipc_close(void* device_ptr);
/* ---- layer 3: ONE frame across the GPUs of one node from ONE host process -------------------------------
 * The draw it shards is SceneRenderer::draw_texture (src/main.rs:1411-1428): rank g of n renders the 8-row blocks b with
 * b % n == g, with its own renderer (same scene, same flags) on devices[g]; the frame is assembled in devices[0]'s memory by
 *   PTL_GROUP_PEER_STORES  the kernels' own row stores over xGMI (peer access, ptl_frame.in_place = 1): no staging, no gather;
 *   PTL_GROUP_COPY_GATHER  a packed shard per rank + ONE strided peer copy per rank (hipMemcpy2DAsync) that gathers and
 *                          de-interleaves in the same transfer -- what an RCCL gather to one root decomposes into;
 *   PTL_GROUP_RCCL_GATHER  the packed shards gathered by RCCL itself (ONE group of ncclSend x n / ncclRecv x n into devices[0], the
 *                          "single RCCL gather" of BASELINE.json's north star), then one strided device-local copy per shard.
 *                          librccl is bound at run time (dlopen; PTL_RCCL_LIB overrides the search): create fails with
 *                          PTL_ERR_NO_DEVICE when it is absent.  Devices must be distinct for this transport.
 * No torch, no second process: a Rust host binds exactly these.  One thread drives all ranks;
 * the handle is not thread-safe.  A device may be listed more than once with the first two transports (rehearsal on a one-GPU machine).
 * Options / camera / update are forwarded to every rank's renderer (ptl_frame_group_renderer gives the individual ones;
 * keep them in step).  ptl_frame_group_draw returns after every rank has finished; *device_rgba8 is the width x height
 * RGBA8 frame on devices[0] (owned by the group, valid until the next draw with another size or destroy);
 * kernel_ms (n floats, may be NULL) receives each rank's trace-kernel time. */
typedef struct ptl_frame_group ptl_frame_group;
enum { PTL_GROUP_PEER_STORES = 0, PTL_GROUP_COPY_GATHER = 1, PTL_GROUP_RCCL_GATHER = 2 };
int ptl_frame_group_create(ptl_scene* s, const int* devices, int n_devices, const char* asset_root, unsigned flags, int transport,
                           ptl_frame_group** out, char* log, size_t log_cap);
int ptl_frame_group_size(const ptl_frame_group* g);
ptl_renderer* ptl_frame_group_renderer(ptl_frame_group* g, int rank);
int ptl_frame_group_set_option(ptl_frame_group* g, const char* name, double value);
int ptl_frame_group_use_camera(ptl_frame_group* g, const char* camera);
int ptl_frame_group_set_camera(ptl_frame_group* g, const double look_at[3], double alpha, double beta, double radius);
int ptl_frame_group_update(ptl_frame_group* g, double seconds);
int ptl_frame_group_draw(ptl_frame_group* g, int width, int height, void** device_rgba8, float* kernel_ms);
/* The pipelined form for clips ("gather of frame n overlaps tracing of frame n+1 on a second stream"): _submit enqueues the
 * trace of one frame on every rank's compute stream and its transfer to devices[0] behind it on the rank's second stream, and returns at
 * once with a ticket; _wait blocks until THAT frame is assembled and hands out its buffer (valid until the frame after the next is
 * submitted).  Two frames may be in flight -- shards, gather buffer and frame are double-buffered -- so while frame n travels over xGMI
 * the compute streams already trace frame n + 1 (set the camera / options / update for it between the two calls: uniform uploads are
 * stream-ordered behind the previous frame's kernel).  A third _submit before the oldest _wait is PTL_ERR_INVALID, and so is a _submit with
 * another frame size while a frame is in flight (the buffers are re-allocated); ptl_frame_group_draw is _submit + _wait and finishes
 * whatever is in flight first. */
int ptl_frame_group_submit(ptl_frame_group* g, int width, int height, int* ticket);
int ptl_frame_group_wait(ptl_frame_group* g, int ticket, void** device_rgba8, float* kernel_ms);
int ptl_frame_group_download(ptl_frame_group* g, uint8_t* host_rgba8);
void ptl_frame_group_destroy(ptl_frame_group* g);

/* Page-locked host memory for those downloads (PCIe-rate copies; pageable memory works too, several times slower). */
int ptl_host_alloc(size_t bytes, void** out);
int ptl_host_free(void* p);

/* The scene writer (serialize_scene_new_format + ron::ser::to_string_pretty, src/gui/scene_serialized.rs:22-24,654-1100):
 * the scene as a .ron document in the reference's own layout, malloc'ed (ptl_free).  The document the scene was loaded from is
 * kept whole and edited in step with the model (uniform values set through ptl_scene_set_uniform, the current stage, the cam
 * block), so an unmodified scene comes back byte for byte -- checked on every scene file of the reference.
 * ptl_ron_format: parse any RON text and write it back in that layout (NULL + ptl_last_error() on a syntax error). */
int ptl_scene_to_ron(ptl_scene* s, char** text);
char* ptl_ron_format(const char* text);

/* PNG I/O (RGBA8): the reference's Texture2D::from_file_with_format / Image::export_png. */
int ptl_png_read(const char* path, uint8_t** rgba8, int* width, int* height); /* free with ptl_free */
int ptl_png_write(const char* path, const uint8_t* rgba8, int width, int height); /* deflate level 6 */
/* the same with an explicit deflate level 0..9 (frame sequences that an encoder consumes and deletes: level 3 is 2.3x faster) */
int ptl_png_write_level(const char* path, const uint8_t* rgba8, int width, int height, int level);
/* A 16-bit RGB file (IHDR: bit depth 16, colour type 2) from HOST rows exactly as ptl_average_f32_to_rgb48 wrote them with the same
 * `filter` (PTL_PNG_FILTER_NONE or _SUB): per row the filter-type byte `filter`, then the row's 6 W bytes; one zlib stream at `level`
 * 0 .. 9; IEND.  No per-pixel work on the host.  ptl_png_read opens such a file by its high bytes. */
int ptl_png_write_rgb48(const char* path, const uint8_t* rows, int width, int height, int filter, int level);

/* ---- GPU deflate of an 8-bit PNG frame: run-length fixed-Huffman streams (opt-in: `--png-encoder gpu`) ------------------
 * ptl_png_deflate_rgba8 turns an RGBA8 frame that is already on the card into the deflate stream of its filtered scanlines, so that the host's
 * part of the file is a CRC and an fwrite (ptl_png_write_stream).  The stream is stated bit for bit; tests/png_deflate_reference.py restates it
 * in numpy, and any inflater returns `raw` from it.
 * Input.  frame_rgba8: DEVICE pointer, W x H pixels of 4 bytes, packed.  Its raw scanlines `raw`, H (4 W + 1) bytes, are what
 *   ptl_png_write_level deflates: per row a filter-type byte, 0 for row 0 and 2 (Up) for every other row, then the row's 4 W bytes, each minus
 *   the byte above it mod 256 (row 0 unchanged).
 * Bands.  `raw` is cut into bands of whole rows, ptl_png_stream_band_rows(W) = max(1, floor(16384 / (4 W + 1))) rows each (the last band may
 *   have fewer); inside a band `raw` is cut into segments of 4096 bytes (the last of a band may be shorter).  Runs never cross a segment
 *   boundary: the parse stays local, and a segment's Adler-32 partial sums stay within 32 bits (255 * 4096 * 4097 / 2 < 2^32).
 * Tokens of a segment.  For every maximal run of L equal bytes v: literal v; m = L - 1; while m >= 3, a match of length min(m, 258) at
 *   distance 1, m less that length; the remaining m (0, 1 or 2) bytes as literals v.
 * Bits of a band (RFC 1951 3.2.5 - 3.2.6, fixed codes): block header BFINAL = 0, BTYPE = 01; the tokens (Huffman codes most-significant bit
 *   first, extra bits least-significant bit first, distance code 0 without extra bits); end-of-block (seven 0 bits); an empty stored block
 *   (three 0 bits, zero padding to the byte, 00 00 FF FF).  Every band is a whole number of bytes, and bands concatenate.
 * The zlib stream of the file: 78 01, the bands in order, 03 00 (an empty final fixed block), Adler-32 of `raw`, big-endian.
 * Capacity.  A token never costs more than 9 bits per raw byte it covers (a match: at most 18 bits for at least 3 bytes), so a band of n raw
 *   bytes needs at most ceil((9 n + 20) / 8) + 4 bytes.  Every band's slot is sized from that bound (rounded up to 16): no input overruns it.
 * out: DEVICE pointer, 16-byte aligned, ptl_png_stream_bytes(W, H) bytes:
 *   bytes 0 .. 63   header, little-endian uint32: "PTLZ" (0x5a4c5450), W, H, the stream's byte count n, Adler-32 of `raw`, rows per band,
 *                   number of bands, nine zero words
 *   bytes 64 .. 64 + n   the bands in order (without 78 01 / 03 00 / Adler-32: the writer adds them); room for the sum of the band bounds
 *   behind it       scratch: a 16-byte table entry per band (bytes used, Adler s1, s2, raw bytes) and the bands' slots.  Nothing in `out` has
 *                   to be cleared between calls.
 * Refused before any GPU call (PTL_ERR_INVALID): null or not 16-byte aligned pointers, sizes <= 0, H (4 W + 1) > 2^31 (the kernels address
 * `raw` with 32-bit offsets; ptl_png_stream_bytes is 0 for such a size).  Stream and timing as for ptl_average_images: two kernels
 * (portal_amd/csrc/kernels/png_deflate.hip) on `stream`, elapsed_ms != NULL waits and reports both. */
#define PTL_PNG_STREAM_HEADER_BYTES 64 /* the stream starts this far into the result buffer; its byte count is header word 3 */
size_t ptl_png_stream_bytes(int width, int height);
/* What a host needs of the result buffer: the header and the room for the longest stream (rounded up to 16), without the scratch behind them;
 * 0 where ptl_png_stream_bytes is 0. */
size_t ptl_png_stream_download_bytes(int width, int height);
int ptl_png_stream_band_rows(int width); /* rows per band; 0 for a width that is not positive */
int ptl_png_deflate_rgba8(int device, const void* frame_rgba8, int width, int height, void* out, void* stream, float* elapsed_ms);
/* ---- The same with per-band dynamic Huffman codes (opt-in: `--png-codes dynamic`) -----------------------------------------
 * ptl_png_deflate_rgba8_codes(codes = PTL_PNG_CODES_FIXED) IS ptl_png_deflate_rgba8: the same kernels, the same bytes.  With
 * PTL_PNG_CODES_DYNAMIC every band is emitted as a dynamic block (RFC 1951 3.2.7) or as the fixed block above, whichever has fewer bits.
 * Unchanged: `raw`, the bands and segments, the tokens, the Adler-32, the band's trailing empty stored block, 78 01 ... 03 00, the 64-byte
 * header (its reserved words zero), the layout of `out` and ptl_png_stream_bytes; ptl_png_write_stream reads either.
 * tests/png_huffman_reference.py restates what follows.  Per band:
 * Histogram.  count[s], s = 0 .. 285: how often literal/length symbol s occurs among the band's tokens; end-of-block (256) counts once.
 * Literal/length code.  The used symbols (count > 0; at least two) sorted by (count, symbol) are the leaves of a Huffman tree built with two
 *   queues: the leaves in that order, and the merged nodes in the order they are made.  Each merge takes, twice, the lighter of the two queue
 *   heads -- the leaf where the weights are equal -- and appends a node of the summed weight.  A leaf's depth is its number of edges to the
 *   root.  n[d] = number of leaves of depth d, depths beyond 15 counted as 15.  Repair: while sum n[d] 2^(15 - d) > 2^15: n[15] -= 1; for the
 *   largest d < 15 with n[d] > 0: n[d] -= 1, n[d + 1] += 2 (each round takes one unit off the sum and keeps the number of leaves).  Lengths go
 *   to the symbols in the sorted order: the first n[15] symbols (the rarest) get 15, the next n[14] get 14, and so on.  Codes: the canonical
 *   assignment of RFC 1951 3.2.2.
 * Distance code.  One code, distance code 0, of length 1 (a 0 bit behind every match).  HDIST = 0.
 * Block header.  BFINAL = 0, BTYPE = 10, HLIT = (last used symbol + 1) - 257, HDIST = 0, HCLEN = 15; the 19 lengths of the code-length code in
 *   the order 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15.  The code-length code is ONE fixed complete code, symbol 0 .. 18:
 *       lengths   3 7 4 4 4 4 4 4 4 4 5 5 6 6 6 7 4 4 3          (canonical codes, RFC 1951 3.2.2)
 *   Then the HLIT + 257 literal/length lengths followed by the one distance length (1), as one sequence, greedily per maximal run of r equal
 *   lengths v.  v = 0: while r >= 138, symbol 18 with 138; then 18 with r if r >= 11, 17 with r if r >= 3, else r times symbol 0.
 *   v > 0: symbol v; m = r - 1; while m >= 6, symbol 16 with 6; then 16 with m if m >= 3, else m times symbol v.
 * Choice.  dynamic bits = header + sum count[s] (length[s] + extra bits) + 1 per match; fixed bits = 3 + sum count[s] (fixed length[s] + extra
 *   bits) + 5 per match, end-of-block in both.  The band is the dynamic block where dynamic bits < fixed bits, else the fixed block: a band
 *   never exceeds ceil((9 n + 20) / 8) + 4 bytes, and slots and capacities stay as they are.
 * Any other `codes` is PTL_ERR_INVALID before anything else is looked at; every refusal of ptl_png_deflate_rgba8 carries over.  Two kernels on
 * `stream`: the bands kernel of portal_amd/csrc/kernels/png_huffman.hip and the pack kernel of png_deflate.hip. */
#define PTL_PNG_CODES_FIXED 0
#define PTL_PNG_CODES_DYNAMIC 1
int ptl_png_deflate_rgba8_codes(int device, const void* frame_rgba8, int width, int height, int codes, void* out, void* stream, float* elapsed_ms);
/* The file from a HOST copy of that buffer (the header and the stream's n bytes are read, nothing behind them): signature, IHDR (bit depth 8,
 * colour type 6), ONE IDAT = 78 01 + stream + 03 00 + Adler-32, IEND.  No per-pixel work and no zlib call but crc32.  A header that does not
 * match -- the magic word, W, H, the band cut, or a byte count beyond the room ptl_png_stream_bytes leaves for the stream -- is
 * PTL_ERR_INVALID, and nothing is written. */
int ptl_png_write_stream(const char* path, const uint8_t* result, int width, int height);

/* ---- GPU deflate of a 16-bit PNG frame: matches at pixel distance (opt-in: `--png16-encoder gpu`) -------------------------
 * ptl_png_deflate_rgb48 turns the rows of a 16-bit RGB frame that are already on the card into the deflate stream of its filtered scanlines;
 * ptl_png_write_stream_rgb48 frames it.  In such a row neighbouring samples lie 6 bytes apart, so a run of equal pixels, or a vertical
 * gradient after the Up filter, repeats with period 6, not 1: every match is at distance 6.  tests/png16_deflate_reference.py restates what
 * follows, and any inflater returns `raw16` from the stream.
 * Input.  rows_rgb48: DEVICE pointer, the UNFILTERED rows of ptl_average_f32_to_rgb48(..., PTL_PNG_FILTER_NONE, ...): H rows of 6 W bytes,
 *   big-endian samples, packed.  Its raw scanlines `raw16`, H (6 W + 1) bytes: per row a filter-type byte, 0 for row 0 and 2 (Up) for every
 *   other row, then the row's 6 W bytes, each minus the byte above it mod 256 (row 0 unchanged).
 * Bands.  `raw16` is cut into bands of whole rows, ptl_png_stream16_band_rows(W) = max(1, floor(16384 / (6 W + 1))) rows each (the last band
 *   may have fewer); inside a band `raw16` is cut into segments of 4096 bytes (the last of a band may be shorter).  No match reaches before
 *   its segment: the parse stays local, and a segment's Adler-32 partial sums stay within 32 bits.
 * Tokens of a segment.  Byte i, counted from the segment's start, is covered when i >= 6 and s[i] == s[i - 6].  Every byte that is not covered
 *   is a literal.  It is followed by the maximal stretch of m covered bytes behind it: while m >= 3, a match of length min(m, 258) at distance
 *   6, m less that length; the remaining m (0, 1 or 2) bytes as literals.  The first six bytes of a segment are literals.  (With "covered"
 *   read as "equal to the previous byte" this is the rule of ptl_png_deflate_rgba8.)
 * Distance code.  Distance 6 is distance symbol 4 with one extra bit of value 1.  Fixed block: the five bits 00100 (most-significant bit
 *   first, like every Huffman code), then the extra bit.  Dynamic block: HDIST = 4, distance code lengths 0 0 0 0 1 (one code, one bit, sent
 *   as 0), then the extra bit.
 * Bits of a band.  As ptl_png_deflate_rgba8_codes states them -- the histogram, the two-queue builder with limit 15 and its repair, the
 *   canonical codes, the contract's one code-length code, HCLEN = 15 -- with HDIST = 4 in the block header, and the sequence that the greedy
 *   16 / 17 / 18 rule codes being the HLIT + 257 literal/length lengths followed by the five distance lengths, as one sequence.  Then the
 *   tokens, end-of-block and an empty stored block (three 0 bits, zero padding to the byte, 00 00 FF FF).
 * Choice.  dynamic bits = header + sum count[s] (length[s] + extra bits) + 2 per match; fixed bits = 3 + sum count[s] (fixed length[s] + extra
 *   bits) + 6 per match, end-of-block in both.  With PTL_PNG_CODES_DYNAMIC the band is the dynamic block where dynamic bits < fixed bits, else
 *   the fixed block; PTL_PNG_CODES_FIXED forces the fixed block in every band, through the same kernel.
 * The zlib stream of the file: 78 01, the bands in order, 03 00 (an empty final fixed block), Adler-32 of `raw16`, big-endian.
 * Capacity.  A fixed match costs at most 8 + 5 + 5 + 1 bits for at least 3 bytes, still under 9 per byte, so a band of n raw bytes needs at
 *   most ceil((9 n + 20) / 8) + 4 bytes, and every band's slot is sized from that bound (rounded up to 16).
 * out: DEVICE pointer, 16-byte aligned, ptl_png_stream16_bytes(W, H) bytes, laid out as the result buffer of ptl_png_deflate_rgba8: the
 *   64-byte header, room for the stream, a 16-byte table entry per band, the bands' slots.  The header's magic word is "PTL6" (0x364c5450), so
 *   that neither writer takes the other's buffer; words 1 .. 6 are W, H, the stream's byte count n, Adler-32 of `raw16`, rows per band, number
 *   of bands; the remaining nine words are zero.  Nothing in `out` has to be cleared between calls.
 * Refused before any GPU call (PTL_ERR_INVALID): any `codes` but the two (before anything else is looked at), null or not 16-byte aligned
 * pointers, sizes <= 0, W H > 2^28 (the rows' own limit), H (6 W + 1) > 2^31; the size functions are 0 for such a size.  Two kernels on
 * `stream` (the 16-bit bands kernel of portal_amd/csrc/kernels/png_huffman.hip and the pack kernel of png_deflate.hip), elapsed_ms != NULL
 * waits and reports both. */
size_t ptl_png_stream16_bytes(int width, int height);
size_t ptl_png_stream16_download_bytes(int width, int height); /* the header and the room for the longest stream (rounded up to 16) */
int ptl_png_stream16_band_rows(int width);                     /* rows per band; 0 for a width that is not positive */
int ptl_png_deflate_rgb48(int device, const void* rows_rgb48, int width, int height, int codes, void* out, void* stream, float* elapsed_ms);
/* The file from a HOST copy of that buffer (the header and the stream's n bytes are read, nothing behind them): signature, IHDR (bit depth 16,
 * colour type 2), ONE IDAT = 78 01 + stream + 03 00 + Adler-32, IEND.  No per-pixel work and no zlib call but crc32.  The header checks are
 * those of ptl_png_write_stream, against the magic word, the band cut and the room of THIS format (an 8-bit "PTLZ" buffer is refused): a
 * mismatch is PTL_ERR_INVALID, and nothing is written. */
int ptl_png_write_stream_rgb48(const char* path, const uint8_t* result, int width, int height);
/* The same stream framed as a 16-bit GREY file (colour type 0) of `width` samples per row: a grey row of W samples is byte for byte an RGB48 row of
 * W / 3 pixels with the filter-type byte in the same place, so ptl_png_deflate_rgb48(rows, W / 3, H, codes, out) over grey rows (what
 * ptl_passes_to_gray16 and ptl_pass_slices_to_gray16 write) is a valid stream for the grey image.  `result`: a HOST copy of that buffer's first
 * ptl_png_stream16_download_bytes(W / 3, H) bytes.  Requires width % 3 == 0 and the "PTL6" header of a (width / 3) x height frame; writes IHDR
 * with bit depth 16 and colour type 0 and ONE IDAT; anything else: PTL_ERR_INVALID, nothing written.  (`portal-amd render --pass-encoder gpu`.) */
int ptl_png_write_stream_gray16(const char* path, const uint8_t* result, int width, int height);

/* ---- template engine test hooks (src/code_generation.rs) ----------------------------------- */
typedef struct ptl_strstore ptl_strstore;
ptl_strstore* ptl_strstore_new(void);
void ptl_strstore_free(ptl_strstore* s);
void ptl_strstore_add_string(ptl_strstore* s, const char* text);
void ptl_strstore_add_identifier_string(ptl_strstore* s, const char* kind, const char* name, const char* text);
/* consumes (frees) the storages it is given */
ptl_strstore* ptl_apply_template(const char* tmpl, const char* const* slot_names, ptl_strstore* const* storages, int n);
const char* ptl_strstore_text(const ptl_strstore* s);
int ptl_strstore_current_line(const ptl_strstore* s);
/* range of element (kind, name): 0 found, 1 missing; [start, end) 1-based */
int ptl_strstore_range(const ptl_strstore* s, const char* kind, const char* name, int* start, int* end);
int ptl_strstore_get_identifier(const ptl_strstore* s, int line, char* kind, size_t kind_cap, char* name, size_t name_cap,
                                int* local_line);
/* The conditional sections of a template (`//%if NAME` or `//%if !NAME`, `//%else`, `//%end`, each on a line of its own, nesting) resolved for
 * the n names given: malloc'ed (ptl_free).  NULL + ptl_last_error() for a section left open, an else / end without an if, a second else, or a
 * name -- in the text or among `names` -- other than slices, passes, refine, refine_slices. */
char* ptl_select_sections(const char* text, const char* const* names, int n);

/* The fixed device sources embedded in the library: "glsl" (types + numerics contract),
 * "library" (prelude), "trace" (kernel template), "entry" (launchable entry points),
 * "refine_entry" (the list-driven render entry of PTL_FLAG_REFINE builds), "refine_slices_entry" (the one over slices of PTL_FLAG_REFINE_SLICES builds).
 * "library" and "entry" are the texts of a build without PTL_FLAG_SLICES / _PASSES / _REFINE / _REFINE_SLICES (their conditional sections
 * resolved for no name, no marker left); "trace" is the template as embedded, its conditional sections and slot markers included.
 * Returns NULL for an unknown name.  Lets a caller write its own kernel against the same
 * conventions and hand it to ptl_kernel_compile. */
const char* ptl_device_source(const char* which);

/* GLSL snippet -> C++ (malloc'ed, ptl_free) and the formula evaluator, exposed for tests. */
char* ptl_translate_glsl(const char* glsl);
/* The same for a file-scope library text (scene.rs:1037-1044): every function DEFINITION gets the kernel's force-inline attribute PTL_FN. */
char* ptl_translate_library_glsl(const char* glsl);
/* The distance-bound rewrite of an intersection-material snippet on its own (host/glsl_translate.h `bound_nearer_blocks`; tests): the GLSL
 * body with `&& !(H.t > ptl_far)` added to the conditions it recognises (malloc'ed, ptl_free), *bounded = how many; `out_functions`:
 * comma-separated names of scene functions with out / inout parameters.  Unchanged text and 0 when the snippet's shape does not allow it. */
char* ptl_bound_glsl(const char* glsl_body, const char* out_functions, int* bounded);
/* The uniform-work hoister on one snippet, exposed for tests (the code generator runs it on every scene snippet unless flags
 * bit12 / bit5 say otherwise).  `uniforms` lists the run-time uniforms as "type name;type name;..." (GLSL types), `out_functions`
 * the functions that write through an argument ("f;g"; "=f" marks a function the scene merely defines itself, which is then never
 * taken for the built-in of that name), `body_only` != 0 says the text is a function BODY whose parameters are
 * `params` ("r;first"; "@r" marks a ray whose origin is the camera's, as in the first-trip variant of a snippet).  Returns the rewritten GLSL (malloc'ed, ptl_free; the input itself when nothing was hoisted) and, in
 * *prologue (may be NULL), the GLSL statements for the prologue kernel, one line per created member in front as
 * "// member: type name[count]". */
char* ptl_hoist_glsl(const char* glsl, const char* uniforms, const char* out_functions, int body_only, const char* params, char** prologue);
/* What a build's compiled-in values do to a TRANSLATED snippet (host/glsl_translate.h `specialize_translated`), exposed for tests and tools:
 * `masked` "M;N" names the matrix uniforms whose products get their masked forms, `unroll_bounds` "n=4;m=16" the baked Int uniforms whose
 * loops get `_Pragma("unroll")`; *unrolled (may be NULL) receives how many did.  malloc'ed (ptl_free). */
char* ptl_specialize_translated(const char* cxx, const char* masked, const char* unroll_bounds, int* unrolled);
/* names/values: free variables; returns 0 and *out, 1 if the formula is invalid or unresolvable */
int ptl_formula_eval(const char* text, const char* const* names, const double* values, int n, double time, double* out);

#ifdef __cplusplus
}
#endif
#endif /* PORTAL_AMD_H */
