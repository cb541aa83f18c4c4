// renderer_builds.cpp -- which kernel a renderer draws with (renderer.h `Builds`): what a build compiles in, when the current kernel is stale,
// the rebuild on the calling thread and the one in the background, and what happens to the kernel that is replaced.
//   generate + compile + load textures: the JIT step of SceneRenderer::new (main.rs:946-1010,1066-1083)
#include <algorithm>
#include <cstdlib>
#include <dirent.h>

#include "renderer.h"

extern "C" int ptl_kernel_compile_prebuilt(int device, const char* hip_source, const ptl_uniform_desc* uniforms, int n_uniforms, size_t uniform_block_size,
                                           const char* const* defines, int n_defines, const void* code, size_t code_size, ptl_kernel** out, char* log,
                                           size_t log_cap);  // kernel.cpp

namespace ptl {

// The kinds of build a renderer tells apart.  Specialised: compiles in something a later state can invalidate -- values (bits 0 / 2 / 3) or, with
// PTL_FLAG_SPECIALIZE_PATTERNS, only what survives while values move (the zero patterns of the matrices, the mode switches, the scene's switches).
constexpr unsigned kSpecialisation = PTL_FLAG_SPECIALIZE_INTS | PTL_FLAG_SPECIALIZE_ALL | PTL_FLAG_SPECIALIZE_STATIC | PTL_FLAG_SPECIALIZE_PATTERNS;
static bool specialised(unsigned flags) { return (flags & kSpecialisation) != 0; }
// the current values as literals: every change of the scene is a rebuild
static bool bakes_values(unsigned flags) { return (flags & (PTL_FLAG_SPECIALIZE_INTS | PTL_FLAG_SPECIALIZE_ALL)) != 0; }
// what stays constant while a clip plays: valid while every compiled-in value and zero pattern still holds (checked before every draw)
static bool clip_constant(unsigned flags) {
    return (flags & (PTL_FLAG_SPECIALIZE_STATIC | PTL_FLAG_SPECIALIZE_PATTERNS)) != 0 && !bakes_values(flags);
}
// PTL_FLAG_ASYNC_REJIT on a specialised renderer with a device: rebuilds are compiled by a worker thread (Job)
bool async_rejit(const ptl_renderer& r) { return (r.flags & PTL_FLAG_ASYNC_REJIT) != 0 && specialised(r.flags) && r.device >= 0; }

static KernelOptions options_from_flags(unsigned flags) {
    auto on = [flags](unsigned bit) { return (flags & bit) != 0; };
    KernelOptions o;
    o.specialize_ints = on(PTL_FLAG_SPECIALIZE_INTS);
    o.count_segments = on(PTL_FLAG_COUNT_SEGMENTS);
    o.specialize_all = on(PTL_FLAG_SPECIALIZE_ALL);
    o.anaglyph = on(PTL_FLAG_ANAGLYPH);
    o.specialize_static = on(PTL_FLAG_SPECIALIZE_STATIC);
    o.specialize_static_ints = on(PTL_FLAG_SPECIALIZE_PATTERNS);  // + the scene's own switches (Bool / Int uniforms that read no per-frame input)
    o.derived_uniforms = !on(PTL_FLAG_NO_DERIVED_UNIFORMS);  // the plain plane tests (A/B measurements, tests)
    o.fast_math = on(PTL_FLAG_FAST_MATH);  // tolerance mode
    o.exact_cr = on(PTL_FLAG_EXACT_CR);  // numerics contract 1 (IEEE / and sqrt on every input), `--exact-cr`
    // PTL_FLAG_QUICK_JIT: -O1 instead of -O3 (a build that is wanted now and used briefly).  Not for a clip-constant build (bit 3 /
    // "specialize_static"): that one is asked for because many frames will run on it, so it keeps the full optimisation level
    o.quick_jit = on(PTL_FLAG_QUICK_JIT) && !o.specialize_static;
    // zero patterns of the matrices that stay run-time values: with any specialisation (the un-specialised kernel has to be valid for every
    // state of the scene -- the background re-JIT draws with it meanwhile); PTL_FLAG_NO_ZERO_MASKS (bit 19) for A/B measurements and tests
    o.mask_zero_elements = specialised(flags) && !on(PTL_FLAG_NO_ZERO_MASKS);
    o.slices_entry = on(PTL_FLAG_SLICES);  // the render entry reads its uniform block from a buffer of blocks, one per blockIdx.z
    o.refine_entry = on(PTL_FLAG_REFINE);  // a second render entry over a device-side list of pixels (ptl_renderer_draw_adaptive)
    o.refine_slices_entry = on(PTL_FLAG_REFINE_SLICES);  // the slices entry plus the list-driven entry over slices (ptl_renderer_draw_slices_adaptive)
    o.slices_entry = o.slices_entry || o.refine_slices_entry;
    o.passes = on(PTL_FLAG_PASSES);  // a 16-byte record per pixel beside the colour: nearest depth, trips, how the paths ended (ptl_renderer_draw_passes)
    o.bound_snippets = on(PTL_FLAG_BOUNDED_SNIPPETS);  // scene_intersect first, its distance bounds the intersection-material snippets (opt-in: measured, no gain)
    // Round 6: the first-trip forms -- a second copy of scene_intersect and of every intersection-material snippet for the trip on which all rays of a
    // wave still start at the camera -- are OPT-IN IN THE UN-SPECIALISED KERNEL (bit 24, PTL_FLAG_KEEP_TRANSFORM_DODGES) and stay the default of the
    // specialised builds (where a kernel with affine rays drops the snippet copies by itself, codegen.cpp).  Round 3 measured +4 % for them on kernels
    // whose transforms were 32 FMAs.  Today: the un-specialised headline 0.697 -> 0.664 ms without them (five views: -3 ... -9 %), triple_portal 0.445 ->
    // 0.434, mobius 1.108 -> 1.046, monoportal equal (profiles/r06/ab_unspec_code_size*.jsonl) -- and that kernel is 12 535 instead of 17 090
    // instructions, compiles in 3.5 s instead of 15.8 on this container's cores and needs no occupancy retry; the specialised builds that keep run-time
    // matrices (patterns, Int-baked) still gain 1 ... 4 % from the plane form (profiles/r06/ab_first_trip_planes.jsonl).  Identical frames either way.
    const bool first_trip_forms = on(PTL_FLAG_KEEP_TRANSFORM_DODGES) || specialised(flags);
    o.first_trip_planes = first_trip_forms && !on(PTL_FLAG_NO_FIRST_TRIP_PLANES);  // one scene_intersect for every trip
    if (const char* ab = std::getenv("PTL_AB_FIRST_TRIP_PLANES"); ab && (ab[0] == '0' || ab[0] == '1')) o.first_trip_planes = ab[0] == '1' && !on(PTL_FLAG_NO_FIRST_TRIP_PLANES);  // (A/B hook)
    if (const char* skip = std::getenv("PTL_AFFINE_RAYS_SKIP_SCAN")) o.skip_affine_scan = skip[0] == '1';  // (test hook: KernelOptions::skip_affine_scan)
    // PTL_FLAG_NO_UNROLL: keep snippet loops with baked bounds as loops (A/B measurements).  The quick build keeps them too: unrolling
    // is half of its hiprtc time for the headline scene (3.4 -> 1.8 s on this container's cores) and buys 0.05 ms of kernel
    o.unroll_baked_loops = !on(PTL_FLAG_NO_UNROLL) && !o.quick_jit;
    o.keep_transform_dodges = on(PTL_FLAG_KEEP_TRANSFORM_DODGES);  // deferred updates + first-trip snippet copies also with affine rays (A/B)
    // the Simple materials' literals from a table instead of one inlined material_simple2 per material (A/B: measured slower, off by default -- codegen.h):
    // PTL_FLAG_MATERIAL_TABLE_LDS (bit 26) staged in LDS, PTL_FLAG_MATERIAL_TABLE_SCALAR (bit 27) in constant memory behind scalar loads
    o.material_table = on(PTL_FLAG_MATERIAL_TABLE_SCALAR) ? 2 : (on(PTL_FLAG_MATERIAL_TABLE_LDS) ? 1 : 0);
    o.check_affine = on(PTL_FLAG_CHECK_AFFINE);  // general products, and `segments` counts the ray halves whose w is not 1 / 0
    o.affine_rays = !on(PTL_FLAG_NO_AFFINE_RAYS);  // matrix-times-ray products never assume o.w = 1 / d.w = 0 (A/B measurements, tests)
    o.first_trip = first_trip_forms && !on(PTL_FLAG_NO_FIRST_TRIP);  // no first-trip copies of the intersection-material snippets
    o.hoist_uniform_work = !on(PTL_FLAG_NO_UNIFORM_HOIST);  // snippets evaluate their uniform-only expressions per ray
    return o;
}

// The renderer's mode switches that a specialised build compiles in (KernelOptions::baked_options): the camera models and output modes.
static std::map<std::string, int> mode_switches(const ptl_renderer& r) {
    // (Round 6 measured the four display toggles -- `_grid_disable`, `_black_border_disable`, `_angle_color_disable`, `_darken_by_distance` -- and the scene's
    // `teleport_light_u` compiled in as well: 10 % fewer static instructions (every scalar load with its address arithmetic and wait inside the headline's ~20
    // inlined portal tests gone), 0.1873 -> 0.1869 ms: nothing -- the kernel is bound by VALU issue, scalar work hides behind it.  profiles/r06/README.md)
    return {{"_use_panini_projection", r.cam.use_panini_projection ? 1 : 0}, {"_use_360_camera", r.cam.use_360_camera ? 1 : 0},
            {"_use_180_camera", r.cam.use_180_camera ? 1 : 0},               {"_draw_depth_map", r.opt.draw_depth_map ? 1 : 0},
            {"_draw_anaglyph", r.opt.draw_anaglyph ? 1 : 0},                 {"_draw_side_by_side", r.opt.draw_side_by_side ? 1 : 0}};
}

// Generates the scene's source for `flags` into s->last; a renderer's build also passes what its stage has learnt and its mode switches.
void refresh_generated(ptl_scene* s, unsigned flags, const StageMemory* stage, const std::map<std::string, int>* switches) {
    KernelOptions opts = options_from_flags(flags);
    opts.mask_cache = &s->mask_cache;
    if (stage) {
        opts.full_chains = stage->full_chains;
        if (stage->no_affine) opts.affine_rays = false;
        opts.keep_dynamic = stage->keep_dynamic;
        opts.keep_unmasked = stage->keep_unmasked;
    }
    if (switches && specialised(flags)) opts.baked_options = *switches;
    CodegenFlags cg;
    cg.defer_loop_updates = (flags & PTL_FLAG_NO_DEFERRED_UPDATES) == 0;  // the snippets exactly as written (A/B measurements, tests)
    s->last = generate_kernel_source(*s->scene, cg, opts);
    s->desc_names.clear();
    s->descs.clear();
    for (auto& u : s->last.uniforms) s->desc_names.push_back(u.name);
    for (size_t k = 0; k < s->last.uniforms.size(); ++k)
        s->descs.push_back(ptl_uniform_desc{s->desc_names[k].c_str(), to_c_type(s->last.uniforms[k].type), s->last.uniforms[k].offset});
}

// VideoRuntime::update (src/main.rs:849-924): frame index = round((count - 1) * clamp(uniform, 0, 1)); a changed index loads
// that PNG and binds it to the video's sampler.  IO errors are ignored like there (the sampler keeps its previous frame).
int update_videos(ptl_renderer* r) {
    const Scene& scene = *r->scene;
    if (scene.video_sources.empty() || r->device < 0) return PTL_OK;
    r->videos.resize(scene.video_sources.size());
    for (size_t k = 0; k < scene.video_sources.size(); ++k) {
        const Scene::Video& v = scene.video_sources[k];
        VideoState& st = r->videos[k];
        if (v.path.empty() || v.uniform < 0) continue;
        if (!st.scanned) {  // video_collect_frame_files: video_png/<file stem>/*.png, sorted
            st.scanned = true;
            std::string base = v.path.substr(v.path.rfind('/') == std::string::npos ? 0 : v.path.rfind('/') + 1);
            std::string stem = base.substr(0, base.rfind('.') == std::string::npos ? base.size() : base.rfind('.'));
            std::string dir = (r->asset_root.empty() ? std::string() : r->asset_root + "/") + "video_png/" + stem;
            if (DIR* d = opendir(dir.c_str())) {
                while (dirent* e = readdir(d)) {
                    std::string name = e->d_name;
                    if (name.size() > 4 && name.compare(name.size() - 4, 4, ".png") == 0) st.frames.push_back(dir + "/" + name);
                }
                closedir(d);
            }
            std::sort(st.frames.begin(), st.frames.end());
        }
        if (st.frames.empty()) continue;
        auto value = scene.eval_uniform(v.uniform);
        if (!value) continue;
        double x = value->as_f64();
        x = x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x);  // f64::clamp; NaN stays NaN and ends up as index 0 below
        double last = (double)(st.frames.size() - 1);
        double target = std::round(last * x);
        long index = std::isnan(target) ? 0 : (long)(target < 0.0 ? 0.0 : (target > last ? last : target));
        if (index == st.bound) continue;
        uint8_t* px = nullptr;
        int w = 0, h = 0;
        if (ptl_png_read(st.frames[index].c_str(), &px, &w, &h) != PTL_OK) continue;
        int rc = ptl_kernel_set_texture(r->builds.kernel, (v.name + "_tex").c_str(), px, w, h);
        std::free(px);
        if (rc < 0) return rc;
        st.bound = index;
    }
    return PTL_OK;
}

// reload_textures (main.rs:1066-1083) into a freshly built kernel
static int bind_textures(ptl_renderer* r, ptl_kernel* k) {
    if (r->device < 0) return PTL_OK;
    for (const Texture& t : r->scene->textures) {
        std::string path = r->asset_root.empty() ? t.path : r->asset_root + "/" + t.path;
        uint8_t* px = nullptr;
        int w = 0, h = 0;
        // like the reference (data.texture_errors, src/main.rs:1082-1084): keep going, the sampler stays unbound and reads as (0, 0, 0, 1);
        // the message remains available through ptl_last_error()
        if (ptl_png_read(path.c_str(), &px, &w, &h) != PTL_OK) continue;
        int trc = ptl_kernel_set_texture(k, (t.name + "_tex").c_str(), px, w, h);
        std::free(px);
        if (trc < 0) return trc;
    }
    return PTL_OK;
}

// The renderer's kernels are built in two halves (kernel.cpp `ptl_kernel::split`): the render module now, the camera-teleport module when a
// query first asks for it -- a fifth of every build that a still camera never needs.  PTL_ONE_MODULE=1: one module with every entry (A/B).
static bool split_builds() {
    const char* e = std::getenv("PTL_ONE_MODULE");
    return !(e && e[0] == '1');
}

// What a renderer's build adds to the defines that belong to the generated source: the occupancy hint of the flags (bits 8-11:
// __launch_bounds__(256, waves)) and the split.
static std::vector<std::string> build_defines(const GeneratedKernel&, unsigned flags) {
    std::vector<std::string> d;
    unsigned waves = (flags >> PTL_FLAG_WAVES_SHIFT) & 0xFu;
    if (waves) d.push_back("PTL_WAVES_PER_EU=" + std::to_string(waves));
    if (split_builds()) d.push_back("PTL_RENDER_MODULE");
    return d;
}

static Build snapshot_build(ptl_scene* s, unsigned flags) {
    Build b;
    b.source = s->last.source;
    b.defines = s->last.defines;
    for (auto& d : build_defines(s->last, flags)) b.defines.push_back(d);
    b.desc_names = s->desc_names;
    b.descs = s->descs;
    for (size_t k = 0; k < b.descs.size(); ++k) b.descs[k].name = b.desc_names[k].c_str();
    b.block_size = s->last.uniform_block_size;
    b.baked = s->last.baked;
    return b;
}

static int compile_build(const Build& b, int device, const std::vector<char>* prebuilt, ptl_kernel** out, char* log, size_t log_cap) {
    std::vector<const char*> defines;
    for (auto& d : b.defines) defines.push_back(d.c_str());
    // (the desc names point into b.desc_names: re-seat them, `b` may have been moved since the snapshot)
    std::vector<ptl_uniform_desc> descs = b.descs;
    for (size_t k = 0; k < descs.size(); ++k) descs[k].name = b.desc_names[k].c_str();
    if (prebuilt)
        return ptl_kernel_compile_prebuilt(device, b.source.c_str(), descs.data(), (int)descs.size(), b.block_size, defines.data(), (int)defines.size(), prebuilt->data(),
                                           prebuilt->size(), out, log, log_cap);
    return ptl_kernel_compile(device, b.source.c_str(), descs.data(), (int)descs.size(), b.block_size, defines.data(), (int)defines.size(), out, log, log_cap);
}

// The renderer lets go of kernel `k` (replaced by a rebuild): destroyed, unless a staged slice still has to be traced by it.
static void retire_kernel(ptl_renderer* r, ptl_kernel* k) {
    if (!k) return;
    if (r->slices.names(k))
        r->slices.park(k);
    else
        ptl_kernel_destroy(k);
}

// Zero patterns compiled into the current kernel (r->builds.masked) against the values a draw is about to upload: a matrix with a non-zero where
// the pattern says zero is demoted (keep_unmasked) and reported.
static bool zero_patterns_broken(ptl_renderer* r, const std::vector<UniformUpload>& values) {
    StageMemory& m = r->builds.stage;
    bool broken = false;
    // a kernel with shortened products is exact for finite vectors: a matrix that got infinite elements, or NaN beside numbers, since the kernel was generated
    // (the generator checks the values it sees, codegen.cpp `full_chains`) asks for the full chains from here on
    if (r->builds.shortened && !m.full_chains)
        for (const UniformUpload& v : values)
            if (v.type == UniformType::Mat4 && matrix_breaks_short_chains(v.f)) m.full_chains = broken = true;
    // ... and a kernel with affine rays is exact while every scene matrix maps w = 1 to 1 and w = 0 to 0 (or is NaN throughout: a switched-off object)
    if (r->builds.affine_rays && !m.no_affine)
        for (const UniformUpload& v : values)
            if (v.type == UniformType::Mat4 && !matrix_keeps_rays_affine(v.f)) m.no_affine = m.no_affine_just_set = broken = true;
    for (auto& [name, mask] : r->builds.masked)
        for (const UniformUpload& v : values) {
            if (v.name != name || v.type != UniformType::Mat4) continue;
            if (!pattern_holds(mask, v.f)) {  // a non-zero where the kernel skips a term, or a +-1 the kernel has as a literal and the matrix no longer holds
                m.keep_unmasked.insert(name);
                broken = true;
            }
            break;
        }
    // one broken pattern says the probes did not see this clip's motion: every mask goes, so that a clip costs at most ONE extra rebuild
    if (!m.keep_unmasked.empty())
        for (auto& mk : r->builds.masked) m.keep_unmasked.insert(mk.first);
    return broken;
}

// Clip-constant values compiled into the current kernel (r->builds.baked) against the values a draw is about to upload: one that moved after all is
// demoted to a run-time uniform (keep_dynamic).
static bool baked_values_moved(ptl_renderer* r, const std::vector<UniformUpload>& values) {
    bool moved = false;
    size_t at = 0;
    for (const UniformUpload& b : r->builds.baked) {
        while (at < values.size() && values[at].name != b.name) ++at;  // same order as at generation time
        if (at == values.size()) return true;
        if (!values[at].same_value(b)) {
            r->builds.stage.keep_dynamic.insert(b.name);
            moved = true;
        }
    }
    return moved;
}

// The one answer to "does the current kernel still fit the renderer's state, and if not, what replaces it?", for the draws (with and without
// PTL_FLAG_ASYNC_REJIT), ptl_renderer_kernel and the synchronous rebuilds (rebuild_now: `forced`, the triggers are not looked at).  The scene's
// values are examined only when the caller passes them (`values`: what a draw is about to upload).  When a rebuild is due, the specialised
// source of the current state is generated and r->builds.want holds its build; the caller compiles it (build_kernel, or the worker thread).
static Rebuild decide_rebuild(ptl_renderer* r, const std::vector<UniformUpload>* values, Rebuild forced = Rebuild::none) {
    StageMemory& m = r->builds.stage;
    Rebuild why = forced;
    if (why == Rebuild::none) {
        // the camera went through something that is not an affine map: the kernel's w = 1 / w = 0 no longer holds for primary rays
        const bool left_affine_maps = r->builds.affine_rays && !m.no_affine && !camera_is_affine(*r);
        if (left_affine_maps) m.no_affine = m.no_affine_just_set = true;
        if (left_affine_maps || (specialised(r->flags) && mode_switches(*r) != r->builds.kernel_switches)) {
            why = Rebuild::counted;  // (a camera model / output mode was switched: the kernel has the old one compiled in and the new one compiled out)
        } else if (values && bakes_values(r->flags) && r->builds.kernel_scene_version != r->scene->version) {
            why = Rebuild::quiet;  // values are baked in and the scene changed (cached by source hash)
        } else if (values && clip_constant(r->flags)) {
            // the kernel stays valid as long as every compiled-in value and zero pattern still holds; what moved after all is demoted
            const bool stage_changed = !(r->builds.kernel_stage == r->scene->current_stage);
            const bool moved = baked_values_moved(r, *values);
            const bool broken = zero_patterns_broken(r, *values);  // an animated matrix left the zero pattern its products were shortened for
            if (stage_changed || moved || broken) why = Rebuild::counted;
        }
    }
    if (why == Rebuild::none) return why;
    const bool camera_affine = camera_is_affine(*r);
    if (!(r->builds.kernel_stage == r->scene->current_stage)) {  // another stage / clip: judge afresh what is constant
        m = StageMemory{};
        m.no_affine = !camera_affine || r->affine_violations_seen > 0;
    } else if (m.no_affine && r->affine_violations_seen == 0 && m.affine_returns < 1 && camera_affine && !m.no_affine_just_set) {
        // one transient non-affine camera or matrix state cost the rest of the stage ~16 % of kernel time.  A rebuild that happens for another
        // reason may return to affine rays ONCE per stage when the camera is affine again (the generator re-checks the scene's matrices itself); a second
        // break keeps them off, so a state that flickers cannot rebuild per frame.  A violation the checking build counted keeps them off for good.
        m.no_affine = false;
        ++m.affine_returns;
    }
    m.no_affine = m.no_affine || !camera_affine;  // (no build assumes w = 1 / 0 of a camera that does not keep them)
    m.no_affine_just_set = false;
    r->builds.kernel_switches = mode_switches(*r);
    ptl_scene* s = r->owner;
    refresh_generated(s, r->flags, &m, &r->builds.kernel_switches);
    r->builds.baked = s->last.baked;
    r->builds.masked = s->last.masked;
    r->builds.affine_rays = s->last.affine_rays;
    r->builds.shortened = s->last.shortened;
    r->builds.kernel_stage = r->scene->current_stage;
    r->builds.want = snapshot_build(s, r->flags);
    return why;
}

// The kernel the draws use from now on: a different one starts from a blank uniform block and blank samplers.
static int activate_kernel(ptl_renderer* r, ptl_kernel* k) {
    if (r->builds.kernel == k) return PTL_OK;
    r->builds.kernel = k;
    r->uploaded_scene = 0;  // upload everything again ...
    r->uploaded_options = 0;
    r->uploaded_w = r->uploaded_h = -1;
    for (auto& v : r->videos) v.bound = -1;  // ... and bind the current video frames again
    return update_videos(r);
}

// The only place where a newly built kernel `k` replaces one of the renderer's: `old` -- the active kernel, or with PTL_FLAG_ASYNC_REJIT the
// specialised one that an adopted build supersedes -- loses its lane clones and is retired (parked while a staged slice names it).
static int install_kernel(ptl_renderer* r, ptl_kernel* k, ptl_kernel* old) {
    if (r->lanes.lanes_of == old) r->lanes.drop_clones();
    r->lanes.wait();
    retire_kernel(r, old);
    return activate_kernel(r, k);
}

// compile + load textures, the JIT step of SceneRenderer::new (main.rs:946-1010,1066-1083): r->builds.want, now, on the calling thread
static int build_kernel(ptl_renderer* r, char* log, size_t log_cap) {
    if (r->builds.kernel && r->builds.want.source == r->builds.kernel_source) {  // nothing compiled in changed
        r->builds.kernel_scene_version = r->scene->version;
        return PTL_OK;
    }
    ptl_kernel* k = nullptr;
    int rc = compile_build(r->builds.want, r->device, nullptr, &k, log, log_cap);
    if (rc == PTL_OK && (rc = bind_textures(r, k)) < 0) ptl_kernel_destroy(k);
    if (rc != PTL_OK) return rc;
    r->builds.kernel_source = r->builds.want.source;
    r->builds.kernel_scene_version = r->scene->version;
    return install_kernel(r, k, r->builds.kernel);
}

// With PTL_FLAG_ASYNC_REJIT `kernel` aliases `spec_kernel` or `dyn_kernel`: before a synchronous rebuild the pair is dropped as a whole (the
// worker joined first), and the freshly built specialised kernel seeds it again afterwards.
static void drop_async_kernels(ptl_renderer* r) {
    r->builds.join_worker();
    r->builds.job.reset();
    if (r->builds.spec_kernel || r->builds.dyn_kernel) {
        r->lanes.drop_clones();
        r->slices.drop();  // (a switch of the specialisation bits between stage calls: what was staged is gone with its kernels)
        ptl_kernel_destroy(r->builds.spec_kernel);
        ptl_kernel_destroy(r->builds.dyn_kernel);
        r->builds.spec_kernel = r->builds.dyn_kernel = r->builds.kernel = nullptr;
        r->builds.kernel_source.clear();
    }
    r->builds.spec_source.clear();
    r->builds.failed_source.clear();
    r->builds.want = Build{};
}
static void seed_async_kernels(ptl_renderer* r) {
    if (async_rejit(*r)) {  // the first kernel is the specialised one of this state
        r->builds.spec_kernel = r->builds.kernel;
        r->builds.spec_source = r->builds.kernel_source;
    }
}

void Builds::join_worker() {
    if (job && job->worker.joinable()) job->worker.join();
}
Builds::~Builds() {
    if (spec_kernel || dyn_kernel) {  // background re-JIT: `kernel` is one of these two
        ptl_kernel_destroy(spec_kernel);
        ptl_kernel_destroy(dyn_kernel);
    } else {
        ptl_kernel_destroy(kernel);
    }
}

// A rebuild that is due, compiled on the calling thread: the draws of a renderer without PTL_FLAG_ASYNC_REJIT, ptl_renderer_kernel, rebuild_now.
int update_kernel(ptl_renderer* r, const std::vector<UniformUpload>* values, Rebuild forced, char* log, size_t log_cap) {
    const Rebuild why = decide_rebuild(r, values, forced);
    if (why == Rebuild::none) return PTL_OK;
    int rc = build_kernel(r, log, log_cap);
    if (rc == PTL_OK && why == Rebuild::counted) ++r->rejit_count;
    return rc;
}

// A rebuild on the calling thread also under PTL_FLAG_ASYNC_REJIT: renderer creation, a switch of the specialisation bits, the check-affine belt.
int rebuild_now(ptl_renderer* r, Rebuild why, char* log, size_t log_cap) {
    drop_async_kernels(r);
    if (int rc = update_kernel(r, nullptr, why, log, log_cap); rc != PTL_OK) return rc;
    seed_async_kernels(r);
    return PTL_OK;
}

// Options that are flag bits of the build: "specialize_static" (clip-constant specialisation, bit 3) and "passes" (pass records, bit 30), on or
// off for what follows.  A combination the generator refuses (passes with anaglyph or a refine entry) leaves the renderer as it was.
// (with PTL_FLAG_ASYNC_REJIT a worker may be compiling for the old flags: rebuilt synchronously like at creation)
int set_build_flag(ptl_renderer* r, unsigned bit, bool on) {
    const unsigned before = r->flags, want = on ? (before | bit) : (before & ~bit);
    if (want == before) return PTL_OK;
    return guarded([&] {
        r->flags = want;
        if (bit == PTL_FLAG_SPECIALIZE_STATIC) r->builds.stage.keep_dynamic.clear();
        int rc = PTL_OK;
        try {
            rc = rebuild_now(r, Rebuild::quiet, nullptr, 0);
        } catch (...) {
            r->flags = before;
            throw;
        }
        if (rc != PTL_OK) {
            r->flags = before;
            return rc;
        }
        ++r->options_version;
        return (int)PTL_OK;
    });
}

// The check-affine belt counted a violation under a kernel with affine rays: off for this stage, one counted rebuild.
int rebuild_without_affine_rays(ptl_renderer* r) {
    r->builds.stage.no_affine = r->builds.stage.no_affine_just_set = true;
    return rebuild_now(r, Rebuild::counted, nullptr, 0);
}

// PTL_FLAG_ASYNC_REJIT: pick the kernel for this draw without ever waiting for a compile of the specialised source (see Job):
// the wanted build is compiled by a worker thread, and the draws use `dyn_kernel` until it is done.
int async_select_kernel(ptl_renderer* r, const std::vector<UniformUpload>* values) {
    ptl_scene* s = r->owner;
    const bool changed = decide_rebuild(r, values) != Rebuild::none;
    if (changed) r->builds.kernel_scene_version = r->scene->version;
    if (!changed && !r->builds.job && r->builds.kernel == r->builds.spec_kernel) return PTL_OK;
    if (r->builds.spec_kernel && r->builds.spec_source == r->builds.want.source)  // (also: the state moved back to what the specialised kernel was built for)
        return activate_kernel(r, r->builds.spec_kernel);
    if (r->builds.job && r->builds.job->state.load() != 1) {  // the worker has finished
        std::shared_ptr<Job> job = r->builds.job;
        if (job->worker.joinable()) job->worker.join();
        r->builds.job.reset();
        if (job->state.load() == 2 && job->build.source == r->builds.want.source) {
            ptl_kernel* k = nullptr;
            int rc = compile_build(job->build, r->device, &job->code, &k, nullptr, 0);  // module load only: the code object is there
            if (rc == PTL_OK && (rc = bind_textures(r, k)) < 0) ptl_kernel_destroy(k);
            if (rc == PTL_OK) {
                ptl_kernel* old = r->builds.spec_kernel;
                r->builds.spec_kernel = k;
                r->builds.spec_source = r->builds.kernel_source = job->build.source;
                ++r->rejit_count;
                return install_kernel(r, k, old);
            }
            r->builds.failed_source = job->build.source;
        } else if (job->state.load() == 3) {
            r->builds.failed_source = job->build.source;  // does not compile: stay on the un-specialised kernel, do not try this source again
        }
    }
    if (!r->builds.job && r->builds.want.source != r->builds.failed_source) {
        auto job = std::make_shared<Job>();
        job->build = r->builds.want;
        job->worker = std::thread([job] {
            ptl_kernel* k = nullptr;
            if (compile_build(job->build, -1, nullptr, &k, nullptr, 0) == PTL_OK) {
                const void* data = nullptr;
                size_t size = 0;
                ptl_kernel_code_object(k, &data, &size);
                job->code.assign(static_cast<const char*>(data), static_cast<const char*>(data) + size);
                ptl_kernel_destroy(k);
                job->state.store(2);
            } else {
                job->state.store(3);
            }
        });
        r->builds.job = job;
    }
    if (!r->builds.dyn_kernel) {  // first need: built here, once (a cached code object makes it a module load)
        refresh_generated(s, r->flags & ~kSpecialisation);
        Build dyn = snapshot_build(s, r->flags);
        ptl_kernel* k = nullptr;
        int rc = compile_build(dyn, r->device, nullptr, &k, nullptr, 0);
        if (rc == PTL_OK && (rc = bind_textures(r, k)) < 0) ptl_kernel_destroy(k);
        if (rc != PTL_OK) return rc;
        r->builds.dyn_kernel = k;
    }
    return activate_kernel(r, r->builds.dyn_kernel);
}

}  // namespace ptl

