// cli_common.h -- what cli.cpp (argument parsing, the single-frame commands) and cli_video.cpp (`render`: the clip pipeline) share:
// the parsed command line, the build flags of a frame's and a clip's kernel, path helpers, and the scene / renderer / PNG steps every
// command repeats, each with the message it has always printed.  Everything goes through the C ABI (include/portal_amd.h).
#pragma once

#include <sys/stat.h>

#include <chrono>
#include <cstdio>
#include <initializer_list>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/portal_amd.h"

struct Options {
    std::string scene, clips, output = "frame.png", asset_root = ".", stage, animation, camera, scenes_dir = "scenes", out_dir = ".", starts_with;
    bool have_camera = false, stereo = false, skip_existing = true;
    bool y4m = false;     // render --frames y4m: frames leave as one Y4M stream instead of PNG files
    bool deep_colour = false;  // render --frames y4m --deep-colour: the stream's frames are made from the float sub-frames (ptl_average_f32_to_yuv420p10)
    int chroma = PTL_CHROMA_420;  // render --frames y4m --chroma 420|422|444: the chroma sampling of the stream's frames (ptl_average_to_yuv10)
    bool have_chroma = false;     // --chroma was given
    int png_depth = 8;            // render / render-frame --png-depth 8|16: 16 makes the PNG frames, or the frame, from the float output (ptl_average_f32_to_rgb48)
    bool have_png_depth = false;  // --png-depth was given
    bool png_gpu = false;         // render / render-frame --png-encoder host|gpu: gpu deflates the 8-bit frames on the card (ptl_png_deflate_rgba8), the host only frames the stream
    bool have_png_encoder = false;  // --png-encoder was given
    int png_codes = 0;              // render / render-frame --png-codes fixed|dynamic, with --png-encoder gpu: PTL_PNG_CODES_FIXED or _DYNAMIC (ptl_png_deflate_rgba8_codes)
    bool have_png_codes = false;    // --png-codes was given
    bool png16_gpu = false;         // render / render-frame --png16-encoder host|gpu, with --png-depth 16: gpu deflates the 16-bit frames on the card (ptl_png_deflate_rgb48)
    bool have_png16_encoder = false;  // --png16-encoder was given
    int batch = -1;       // render --batch-subframes 0|1: one launch for a frame's blur sub-frames (default: on where 2 <= blur <= 16)
    std::vector<std::pair<std::string, double>> sets;  // --set name=value
    bool timing = false;  // --timing: wait for every kernel and report GPU milliseconds (serialises host and GPU)
    int specialize = -1;  // -1 auto: clip-constant specialisation when the clip has enough sub-frames to repay the extra JIT
    int width = 1920, height = 1080, aa = 1, depth = 100, device = 0, fps = 60, blur = 1, shard = 0, shards = 1, max_frames = -1;
    double time = 0.0, panini = -1.0, fov = 90.0;
    // render-frame across GPUs: --gpus N (devices 0..N-1) or --devices a,b,.. ; --transport stores|copy|rccl ; --multi-process
    int gpus = 1, rank = 0, world = 1;
    std::string devices, transport = "stores", ipc_handle;
    bool multi_process = false, fast = false, exact_cr = false, opt3 = false;
    bool adaptive = false;   // render-frame --adaptive-aa [T]: one sample per pixel, the full --aa-count only where a pixel differs from a neighbour by more than T codes
    int adaptive_t = 4;
    bool clip_adaptive = false;  // render --clip-adaptive-aa [T]: the same for every sub-frame of a clip (batched: the refine entry over slices)
    int clip_adaptive_t = 4;
    bool pass_depth = false, pass_trips = false;  // render-frame --passes depth,trips: <output stem>.depth.png / .trips.png, 16-bit grey, from the tracer's pass records
    bool pass_cut = false;                        // render-frame --passes cut: <output stem>.cut.png, the share of the pixel's traced paths that --render-depth cut (ptl_pass_slices_to_gray16)
    bool have_passes = false;                     // --passes was given
    // render --clip-passes depth,trips,cut: anim/depth_<i>.png / trips_<i>.png / cut_<i>.png beside every frame of a clip, 16-bit grey, merged on
    // the card from the records of the frame's blur sub-frames (ptl_pass_slices_to_gray16)
    bool clip_pass_depth = false, clip_pass_trips = false, clip_pass_cut = false;
    bool have_clip_passes = false;                // --clip-passes was given
    bool pass_gpu = false;                        // render --pass-encoder host|gpu, with --clip-passes: gpu deflates the pass images on the card (ptl_png_deflate_rgb48 on rows of W / 3 pixels)
    bool have_pass_encoder = false;               // --pass-encoder was given
    bool depth_report = false;                    // render-frame / render --depth-report: one line on the paths that --render-depth cut short
    std::vector<std::string> argv;  // the command line as given (handed on to shard processes)
};

int render(const Options& o);  // cli_video.cpp

inline std::vector<std::string> split_list(const std::string& s) {  // "a, b,,c" -> {a, b, c}
    std::vector<std::string> out;
    size_t pos = 0;
    while (pos <= s.size()) {
        size_t comma = s.find(',', pos);
        if (comma == std::string::npos) comma = s.size();
        std::string item = s.substr(pos, comma - pos);
        size_t b = item.find_first_not_of(" \t"), e = item.find_last_not_of(" \t");
        if (b != std::string::npos) out.push_back(item.substr(b, e - b + 1));
        pos = comma + 1;
    }
    return out;
}

inline void make_dirs(const std::string& path) {  // mkdir -p
    for (size_t p = 1; p <= path.size(); ++p)
        if (p == path.size() || path[p] == '/') ::mkdir(path.substr(0, p).c_str(), 0777);
}

inline std::string dir_of(const std::string& path) {
    size_t p = path.rfind('/');
    return p == std::string::npos ? "" : path.substr(0, p);
}

inline int fail(const char* what) {
    std::fprintf(stderr, "%s: %s\n", what, ptl_last_error());
    return 1;
}

inline int scene_has_no(const std::string& scene, const char* what, const std::string& name) {  // the reference's words (src/main.rs:2900-2926)
    std::fprintf(stderr, "Scene `%s` has no %s named `%s`\n", scene.c_str(), what, name.c_str());
    return 1;
}

inline double seconds_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }

// ---- build flags ------------------------------------------------------------------------------
// No occupancy hint: with the basic VGPR allocator (kernel.cpp) a 4-waves bound makes the un-specialised portal_in_portal kernel
// spill (128 VGPRs + 240 B scratch: 2.19 ms against 1.52 ms at 4K, profiles/r02/variants1_prologue_waveloop_fast.jsonl); the
// other scenes do not care.  (Round 1, greedy allocator: the hint was a 18 % gain on that kernel.)
constexpr unsigned kRenderFlags = 0u;
// `render` (clips): the kernel a clip runs on when it gets no clip-constant build of its own still has the zero patterns of the scene's
// matrices and the mode switches compiled in (PTL_FLAG_SPECIALIZE_PATTERNS, bit 20: no value baked, so nothing moves under it but a
// pattern -- one rebuild per stage at most): 0.58 against 0.83 ms on the headline frame (profiles/r04/ab_bounded_snippets.jsonl `patterns`)
constexpr unsigned kClipFlags = kRenderFlags | PTL_FLAG_SPECIALIZE_PATTERNS;
// ... and, for a clip with motion blur, the slices entry (bit 22): the blur sub-frames of an output frame differ in their uniforms only and are
// traced by ONE launch (grid.z = sub-frame, a uniform block per slice), so the ramp and tail of a small frame overlap with its neighbours' instead
// of adding up: 1080p monoportal 0.0526 -> 0.0415 ms per sub-frame, 720p 0.0319 -> 0.0213, 4K aa 4 0.885 -> 0.861 (profiles/r04/concurrent_draws.jsonl)
constexpr unsigned kSlicesFlag = PTL_FLAG_SLICES;
inline bool batch_subframes(const Options& o) { return o.batch != 0 && o.blur >= 2 && o.blur <= 16; }

// --fast: tolerance mode; --exact-cr: numerics contract 1
inline unsigned numerics_flags(const Options& o) { return (o.fast ? PTL_FLAG_FAST_MATH : 0u) | (o.exact_cr ? PTL_FLAG_EXACT_CR : 0u); }
// A kernel that is wanted NOW gets the quick build (bit 18): the wall time of one frame, or of a clip's start, is the JIT's, not the kernel's
// (profiles/r03/render_frame_e2e.log: 2.4 s of -O3 hiprtc for a 0.33 ms kernel, 1.2 s of -O1 for a 0.36 ms one) -- unless the caller wants the
// shipped optimisation level (--opt3), e.g. to fill the cache for a bench.  The library ignores the bit for clip-constant kernels, which stay at -O3.
inline unsigned quick_jit_flag(const Options& o) { return o.opt3 ? 0u : PTL_FLAG_QUICK_JIT; }

// The build of a clip's kernel, the same wherever it is asked for -- `precompile`, the renderer `render` creates, the workers that compile
// the clips to come: a difference is a miss in the code-object cache and a clip that waits for the JIT the others were meant to hide.
// `clip_constant`: with what is constant within the clip baked in ("specialize_static").  A renderer that starts drawing on the build
// right away adds quick_jit_flag().
// --clip-adaptive-aa: where the sub-frames are batched the module has the slices entry AND the refine entry over slices (bit 29, which implies
// bit 22), else the single-frame refine entry (bit 28) and every sub-frame is a ptl_renderer_draw_adaptive.  Without the option: what it was.
// --depth-report, --clip-passes: the kernel also stores the pass records (bit 30) the report and the pass images are made from.
inline bool clip_records(const Options& o) { return o.depth_report || o.have_clip_passes; }
inline unsigned clip_flags(const Options& o, bool clip_constant) {
    const unsigned entries = o.clip_adaptive ? (batch_subframes(o) ? PTL_FLAG_REFINE_SLICES : PTL_FLAG_REFINE) : (batch_subframes(o) ? kSlicesFlag : 0u);
    return kClipFlags | entries | numerics_flags(o) | (clip_constant ? PTL_FLAG_SPECIALIZE_STATIC : 0u) | (clip_records(o) ? PTL_FLAG_PASSES : 0u);
}

// --depth-report: the one line a downloaded statistics block makes (ptl_pass_stats).  "traced" are the paths that entered the bounce loop
// (the samples in the bars of a 360 / 180 degree frame never do); `tail`: what a clip adds about its worst frame.
inline void print_depth_report(const ptl_pass_stats_block& b, int render_depth, const std::string& tail = "") {
    const unsigned long long traced = b.paths - b.outside;
    float lo = 0.0f, hi = 0.0f;
    char range[64] = "none";
    if (ptl_pass_stats_depth_range(&b, &lo, &hi) == 1) std::snprintf(range, sizeof range, "%g \xe2\x80\xa6 %g", lo, hi);
    std::printf("Paths: %llu traced, %llu cut at depth %d (%.2f %%) in %llu pixels; deepest pixel %u trips; depth %s%s\n", traced, (unsigned long long)b.exhausted, render_depth,
                traced ? 100.0 * (double)b.exhausted / (double)traced : 0.0, (unsigned long long)b.exhausted_pixels, b.max_trips, range, tail.c_str());
}
// the `_ray_tracing_depth` a draw of `r` uploads (--render-depth, or what a clip's override made of it)
inline int render_depth_of(ptl_renderer* r, int width, int height) {
    float v[16] = {};
    int n = 0;
    return ptl_renderer_uniform_value(r, width, height, "_ray_tracing_depth", v, &n) == PTL_OK ? (int)v[0] : -1;
}

// SceneRenderer::update_inner_variables (src/main.rs:1688-1756): per-clip settings the reference hard-codes for its
// published videos.  Data, not logic: clip name -> what changes.
struct ClipOverride {
    const char* clip;
    int subspace_degree;  // 0 = leave
    int render_depth;     // 0 = leave
    int fps;              // 0 = leave
};
inline constexpr ClipOverride kClipOverrides[] = {
    {"v2.face.2", 500, 0, 0},     {"v2.face.3", 500, 0, 0},     {"v2.face.4", 500, 0, 0},      {"v2.face.5", 500, 0, 0},
    {"v2.inside.1", 500, 0, 0},   {"v2.inside.3", 500, 0, 0},   {"v2.intro.1", 500, 0, 0},     {"v2.normal.2", 500, 0, 0},
    {"v2.normal.3", 500, 0, 0},   {"v2.rod.2", 500, 0, 0},      {"v2.rod.3", 500, 0, 0},       {"v2.spiral.3", 500, 0, 0},
    {"v2.spiral.4", 1000, 0, 0},  {"v2.spiral.5", 1000, 0, 0},  {"v2.spiral.6", 1000, 0, 0},   {"v2.spiral.7", 500, 0, 0},
    {"v2.spiral.9", 500, 0, 0},   {"v2.spaaaace.0", 500, 0, 0}, {"v4.golden.0", 500, 0, 0},    {"v4.golden.1", 500, 0, 0},
    {"v4.golden.2", 500, 0, 0},   {"v4.thumbnail.2", 500, 0, 0}, {"v2.rotated.0", 0, 100, 0},  {"v2.spiral.0", 0, 100, 0},
    {"v2.screenshot.5", 0, 100, 0}, {"v2.screenshot.6", 0, 100, 0}, {"v2.screenshot.3", 0, 0, 600},
};

inline void apply_clip_overrides(ptl_scene* scene, ptl_renderer* r, const std::string& clip, int* fps) {
    for (const ClipOverride& o : kClipOverrides) {
        if (clip != o.clip) continue;
        if (o.subspace_degree && scene) ptl_scene_set_uniform(scene, "subspace_degree", o.subspace_degree);  // no such uniform: nothing happens
        if (o.render_depth && r) ptl_renderer_set_option(r, "render_depth", o.render_depth);
        if (o.fps && fps) *fps = o.fps;
    }
}

// ---- scene, renderer, PNG: owned handles and the steps every command repeats -------------------
struct HandleFree {
    void operator()(ptl_scene* s) const { ptl_scene_free(s); }
    void operator()(ptl_renderer* r) const { ptl_renderer_destroy(r); }
    void operator()(void* device_memory) const { ptl_device_free(device_memory); }
};
using ScenePtr = std::unique_ptr<ptl_scene, HandleFree>;
using RendererPtr = std::unique_ptr<ptl_renderer, HandleFree>;  // (declare it behind its scene: it goes first)
using DevicePtr = std::unique_ptr<void, HandleFree>;

inline DevicePtr device_alloc(int device, size_t bytes, const char* what) {  // null after "<what>: <error>"
    void* memory = nullptr;
    if (ptl_device_alloc(device, bytes, &memory) != PTL_OK) fail(what);
    return DevicePtr(memory);
}

inline ScenePtr open_scene(const std::string& path) {  // null: ptl_last_error() says why, the caller says it in its own words
    ptl_scene* scene = nullptr;
    return ScenePtr(ptl_scene_load_file(path.c_str(), &scene) == PTL_OK ? scene : nullptr);
}

inline ScenePtr load_scene(const std::string& path, const std::string& shown) {
    ScenePtr scene = open_scene(path);
    if (!scene) std::fprintf(stderr, "Failed to parse scene `%s`: %s\n", shown.c_str(), ptl_last_error());
    return scene;
}
inline ScenePtr load_scene(const Options& o) { return load_scene(o.scene, o.scene); }

// --stage NAME, where there is one: false after the reference's message (src/main.rs:2900-2904)
inline bool init_stage(const Options& o, ptl_scene* scene) {
    char stage_cam[256] = "";
    if (o.stage.empty() || ptl_scene_init_stage(scene, o.stage.c_str(), stage_cam, sizeof stage_cam) == PTL_OK) return true;
    scene_has_no(o.scene, "stage", o.stage);
    return false;
}

// null after "<what>: <error>" and the build log on stderr.  `options`: set before the first build (a baked kernel has its mode switches compiled in)
inline RendererPtr create_renderer(ptl_scene* scene, int device, const Options& o, unsigned flags, const char* what = "renderer",
                                   std::initializer_list<std::pair<const char*, double>> options = {}) {
    std::vector<const char*> names;
    std::vector<double> values;
    for (const auto& option : options) {
        names.push_back(option.first);
        values.push_back(option.second);
    }
    std::vector<char> log(1 << 16);
    ptl_renderer* r = nullptr;
    if (ptl_renderer_create_with_options(scene, device, o.asset_root.c_str(), flags, names.data(), values.data(), (int)names.size(), &r, log.data(), log.size()) != PTL_OK)
        std::fprintf(stderr, "%s: %s\n%s\n", what, ptl_last_error(), log.data());
    return RendererPtr(r);
}

inline int write_png(const std::string& path, const uint8_t* rgba8, int width, int height) {  // 0, or 1 after "png: <error>"
    if (!dir_of(path).empty()) make_dirs(dir_of(path));
    return ptl_png_write(path.c_str(), rgba8, width, height) == PTL_OK ? 0 : fail("png");
}
