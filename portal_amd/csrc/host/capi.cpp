// capi.cpp -- layer 2 of the C ABI: the entry points of the scene handles and of the renderer's lifetime and options.
//
// Host-side mirror of SceneRenderer (src/main.rs:732-1544) for the offline image path:
//   SceneRenderer::new          src/main.rs:934-1064   -> ptl_renderer_create
// The renderer's parts are in renderer.h; which kernel it draws with is renderer_builds.cpp, the draws renderer_draw.cpp, the camera
// renderer_camera.cpp, and the hooks for tests and tools capi_tools.cpp.
#include <cstdlib>
#include <cstring>

#include "renderer.h"

using namespace ptl;

namespace ptl {

int guarded(const std::function<int()>& fn) {
    try {
        return fn();
    } catch (const ron::ParseError& e) {
        set_last_error(e.what());
        return PTL_ERR_SCENE;
    } catch (const SceneError& e) {
        set_last_error(e.what());
        return PTL_ERR_SCENE;
    } catch (const std::exception& e) {
        set_last_error(std::string("internal error: ") + e.what());
        return PTL_ERR_INVALID;
    }
}
void copy_str(char* dst, size_t cap, const std::string& s) {
    if (!dst || !cap) return;
    std::strncpy(dst, s.c_str(), cap - 1);
    dst[cap - 1] = '\0';
}

}  // namespace ptl

// ---- scenes -----------------------------------------------------------------------------------
extern "C" int ptl_scene_load_file(const char* path, ptl_scene** out) {
    if (!path || !out) return PTL_ERR_INVALID;
    return guarded([&] {
        auto s = std::make_unique<ptl_scene>();
        s->scene = Scene::from_file(path);
        *out = s.release();
        return PTL_OK;
    });
}
extern "C" int ptl_scene_load_text(const char* text, ptl_scene** out) {
    if (!text || !out) return PTL_ERR_INVALID;
    return guarded([&] {
        auto s = std::make_unique<ptl_scene>();
        s->scene = Scene::from_ron_text(text);
        *out = s.release();
        return PTL_OK;
    });
}
extern "C" void ptl_scene_free(ptl_scene* s) { delete s; }
extern "C" void ptl_free(void* p) { std::free(p); }

extern "C" int ptl_scene_set_uniform(ptl_scene* s, const char* name, double value) {
    if (!s || !name) return PTL_ERR_INVALID;
    return s->scene->set_uniform_value(name, value) ? PTL_OK : PTL_UNKNOWN_UNIFORM;
}
extern "C" int ptl_scene_set_trefoil(ptl_scene* s, const char* name, const char* text) {
    if (!s || !name || !text) return PTL_ERR_INVALID;
    return guarded([&] { return s->scene->set_trefoil(name, text) ? PTL_OK : PTL_UNKNOWN_UNIFORM; });
}
extern "C" int ptl_scene_get_trefoil(ptl_scene* s, const char* name, char* text, size_t cap) {
    if (!s || !name) return PTL_ERR_INVALID;
    return guarded([&] {
        auto t = s->scene->get_trefoil(name);
        if (!t) return (int)PTL_UNKNOWN_UNIFORM;
        copy_str(text, cap, *t);
        return (int)PTL_OK;
    });
}
extern "C" int ptl_scene_set_time(ptl_scene* s, double time, double total_time) {
    if (!s) return PTL_ERR_INVALID;
    if (s->scene->time != time || s->scene->total_time != total_time) ++s->scene->version;
    s->scene->time = time;
    s->scene->total_time = total_time;
    return PTL_OK;
}
extern "C" int ptl_scene_set_camera_matrix(ptl_scene* s, const double m16[16]) {
    if (!s || !m16) return PTL_ERR_INVALID;
    DMat4 m = DMat4::from_cols({m16[0], m16[1], m16[2], m16[3]}, {m16[4], m16[5], m16[6], m16[7]}, {m16[8], m16[9], m16[10], m16[11]},
                               {m16[12], m16[13], m16[14], m16[15]});
    s->scene->camera_matrix = m;
    ++s->scene->version;
    return PTL_OK;
}
extern "C" int ptl_scene_init_stage(ptl_scene* s, const char* stage, char* camera, size_t camera_cap) {
    if (!s || !stage) return PTL_ERR_INVALID;
    return guarded([&] {
        int cam = -1;
        if (!s->scene->init_stage_by_name(stage, &cam)) return 1;
        std::string name;
        if (cam >= 0) name = s->scene->cameras[cam].name.empty() ? "#" + std::to_string(cam) : s->scene->cameras[cam].name;
        copy_str(camera, camera_cap, name);
        return PTL_OK;
    });
}
extern "C" int ptl_scene_stage_name(ptl_scene* s, int index, char* name, size_t cap) {
    if (!s || index < 0) return PTL_ERR_INVALID;
    if (index >= (int)s->scene->stages.size()) return 1;
    copy_str(name, cap, s->scene->stages[index].name);
    return PTL_OK;
}
extern "C" int ptl_scene_camera_name(ptl_scene* s, int index, char* name, size_t cap) {
    if (!s || index < 0) return PTL_ERR_INVALID;
    if (index >= (int)s->scene->cameras.size()) return 1;
    copy_str(name, cap, s->scene->cameras[index].name.empty() ? "#" + std::to_string(index) : s->scene->cameras[index].name);
    return PTL_OK;
}

extern "C" int ptl_scene_animation(ptl_scene* s, int index, char* name, size_t cap, double* duration) {
    if (!s || index < 0) return PTL_ERR_INVALID;
    if (index >= (int)s->scene->animations.size()) return 1;
    copy_str(name, cap, s->scene->animations[index].name);
    if (duration) *duration = s->scene->animations[index].duration;
    return PTL_OK;
}
extern "C" int ptl_scene_init_animation(ptl_scene* s, const char* animation) {
    if (!s || !animation) return PTL_ERR_INVALID;
    return guarded([&] { return s->scene->init_animation_by_name(animation) ? PTL_OK : 1; });
}
static void fill_cam(const CalculatedCam& c, ptl_calculated_cam* out) {
    out->look_at[0] = c.look_at.x;
    out->look_at[1] = c.look_at.y;
    out->look_at[2] = c.look_at.z;
    out->alpha = c.alpha;
    out->beta = c.beta;
    out->r = c.r;
    out->in_subspace = c.in_subspace;
    out->free_movement = c.free_movement;
    out->override_matrix = c.override_matrix;
    c.matrix.to_cols_array(out->matrix);
}
extern "C" int ptl_scene_update(ptl_scene* s, double seconds, double* time, double* total_time, int* has_cam, ptl_calculated_cam* cam) {
    if (!s) return PTL_ERR_INVALID;
    return guarded([&] {
        auto c = s->scene->update(seconds);
        if (time) *time = s->scene->time;
        if (total_time) *total_time = s->scene->total_time;
        if (has_cam) *has_cam = c ? 1 : 0;
        if (c && cam) fill_cam(*c, cam);
        return PTL_OK;
    });
}

extern "C" int ptl_scene_eval_uniform(ptl_scene* s, const char* name, int* kind, double* value) {
    if (!s || !name) return PTL_ERR_INVALID;
    return guarded([&] {
        auto v = s->scene->eval_uniform(s->scene->find_uniform(name));
        if (!v) return 1;
        if (kind) *kind = (int)v->kind;
        if (value) *value = v->as_f64();
        return PTL_OK;
    });
}
extern "C" int ptl_scene_eval_matrix(ptl_scene* s, const char* name, double out16[16]) {
    if (!s || !name || !out16) return PTL_ERR_INVALID;
    return guarded([&] {
        auto m = s->scene->eval_matrix(s->scene->find_matrix(name));
        if (!m) return 1;
        m->to_cols_array(out16);
        return PTL_OK;
    });
}
extern "C" int ptl_scene_cam(ptl_scene* s, double out7[7]) {
    if (!s || !out7) return PTL_ERR_INVALID;
    const CamSettings& c = s->scene->cam;
    double v[7] = {c.look_at.x, c.look_at.y, c.look_at.z, c.alpha, c.beta, c.r, c.offset_after_material};
    std::memcpy(out7, v, sizeof v);
    return PTL_OK;
}

extern "C" int ptl_scene_texture(ptl_scene* s, int index, char* name, size_t name_cap, char* path, size_t path_cap) {
    if (!s || index < 0) return PTL_ERR_INVALID;
    if (index >= (int)s->scene->textures.size()) return 1;
    copy_str(name, name_cap, s->scene->textures[index].name);
    copy_str(path, path_cap, s->scene->textures[index].path);
    return PTL_OK;
}
extern "C" int ptl_scene_generate_source(ptl_scene* s, unsigned flags, char** source) {
    if (!s || !source) return PTL_ERR_INVALID;
    return guarded([&] {
        refresh_generated(s, flags);
        *source = (char*)std::malloc(s->last.source.size() + 1);
        std::memcpy(*source, s->last.source.c_str(), s->last.source.size() + 1);
        return PTL_OK;
    });
}
extern "C" int ptl_scene_zero_mask_probes(ptl_scene* s, int* reused, int* probed) {
    if (!s) return PTL_ERR_INVALID;
    if (reused) *reused = s->mask_cache.hits;
    if (probed) *probed = s->mask_cache.misses;
    return PTL_OK;
}
extern "C" int ptl_scene_generated_defines(ptl_scene* s, char* out, size_t cap) {
    if (!s || !out || cap == 0) return PTL_ERR_INVALID;
    std::string joined;
    for (const std::string& d : s->last.defines) joined += (joined.empty() ? "" : " ") + d;
    if (joined.size() + 1 > cap) return PTL_ERR_INVALID;
    std::memcpy(out, joined.c_str(), joined.size() + 1);
    return PTL_OK;
}
extern "C" int ptl_scene_uniform_layout(ptl_scene* s, const ptl_uniform_desc** descs, int* n, size_t* block_size) {
    if (!s) return PTL_ERR_INVALID;
    return guarded([&] {
        if (s->last.source.empty()) refresh_generated(s, 0);
        if (descs) *descs = s->descs.data();
        if (n) *n = (int)s->descs.size();
        if (block_size) *block_size = s->last.uniform_block_size;
        return PTL_OK;
    });
}
extern "C" int ptl_scene_set_uniforms(ptl_scene* s, ptl_kernel* k) {
    if (!s || !k) return PTL_ERR_INVALID;
    return guarded([&] {
        std::vector<std::string> errors;
        int rc = upload(k, evaluate_scene_uniforms(*s->scene, &errors));
        if (!errors.empty()) set_last_error(errors[0]);
        return rc;
    });
}
extern "C" int ptl_scene_visit_uniforms(ptl_scene* s, ptl_uniform_cb cb, void* user) {
    if (!s || !cb) return PTL_ERR_INVALID;
    return guarded([&] {
        for (const UniformUpload& u : evaluate_scene_uniforms(*s->scene, nullptr))
            cb(user, u.name.c_str(), to_c_type(u.type), u.type == UniformType::Int1 ? (const void*)&u.i : (const void*)u.f);
        return PTL_OK;
    });
}
extern "C" int ptl_scene_source_line_owner(ptl_scene* s, int line, char* kind, size_t kind_cap, char* name, size_t name_cap, int* local_line) {
    if (!s) return PTL_ERR_INVALID;
    ElementKey key;
    int local = 0;
    if (!s->last.line_numbers.get_identifier(line, &key, &local)) return 1;
    copy_str(kind, kind_cap, key.kind);
    copy_str(name, name_cap, key.name);
    if (local_line) *local_line = local;
    return PTL_OK;
}
static int set_plain_option(ptl_renderer* r, const std::string& n, double v);

extern "C" int ptl_renderer_create_with_options(ptl_scene* s, int device, const char* asset_root, unsigned flags, const char* const* option_names,
                                                const double* option_values, int n_options, ptl_renderer** out, char* log, size_t log_cap) {
    if (!s || !out || n_options < 0 || (n_options > 0 && (!option_names || !option_values))) return PTL_ERR_INVALID;
    if (log && log_cap) log[0] = '\0';
    return guarded([&] {
        auto r = std::make_unique<ptl_renderer>();
        r->owner = s;
        r->scene = s->scene;
        r->device = device;
        r->flags = flags;
        r->asset_root = asset_root ? asset_root : "";
        if ((flags & PTL_FLAG_REFINE) && (flags & PTL_FLAG_SLICES)) {
            set_last_error("ptl_renderer_create: PTL_FLAG_REFINE and PTL_FLAG_SLICES cannot be combined (the refine entry reads the module's own uniform block; PTL_FLAG_REFINE_SLICES has the entry over slices)");
            return (int)PTL_ERR_INVALID;
        }
        if ((flags & PTL_FLAG_REFINE) && (flags & PTL_FLAG_REFINE_SLICES)) {
            set_last_error("ptl_renderer_create: PTL_FLAG_REFINE and PTL_FLAG_REFINE_SLICES cannot be combined (one refine entry per module)");
            return (int)PTL_ERR_INVALID;
        }
        if (const char* e = std::getenv("PTL_CHECK_AFFINE"); e && e[0] == '1') r->check_affine_on_new_source = true;
        // options first: a specialised build compiles the mode switches in (mode_switches), so the FIRST build is already the one the
        // caller will draw with (`render --stereoimage`: draw_side_by_side) instead of a build nothing runs on plus a rebuild
        for (int k = 0; k < n_options; ++k) {
            if (!option_names[k]) return (int)PTL_ERR_INVALID;
            int orc = set_plain_option(r.get(), option_names[k], option_values[k]);
            if (orc != PTL_OK) {
                set_last_error(std::string("ptl_renderer_create_with_options: unknown option `") + option_names[k] + "`");
                return (int)PTL_ERR_INVALID;
            }
        }
        int rc = rebuild_now(r.get(), Rebuild::quiet, log, log_cap);
        if (rc != PTL_OK) return rc;
        // cam.set_cam(scene.cam); offset_after_material from the scene (main.rs:1057-1059)
        r->cam.take(calculated_of(s->scene->cam), false);  // (option "in_subspace" stays as given)
        r->opt.offset_after_material = s->scene->cam.offset_after_material;
        r->cam.prev_cam_pos = cam_pos(r->cam);  // main.rs:1058
        r->original_cam = calculated_of(r->cam);  // render_frame inserts "OriginalCam" up front (main.rs:2893-2896)
        *out = r.release();
        return PTL_OK;
    });
}
extern "C" int ptl_renderer_create(ptl_scene* s, int device, const char* asset_root, unsigned flags, ptl_renderer** out, char* log,
                                   size_t log_cap) {
    return ptl_renderer_create_with_options(s, device, asset_root, flags, nullptr, nullptr, 0, out, log, log_cap);
}

// every option that is a plain field (no rebuild): PTL_OK, or PTL_UNKNOWN_UNIFORM for a name that is not one
static int set_plain_option(ptl_renderer* r, const std::string& n, double v) {
    bool b = v > 0.5;
    if (n == "check_affine") {
        r->check_affine_on_new_source = b;
        return PTL_OK;
    }
    if (n == "render_depth") r->opt.render_depth = (int)v;
    else if (n == "aa_count") r->opt.aa_count = (int)v;
    else if (n == "aa_start") r->opt.aa_start = (int)v;
    else if (n == "view_angle") r->cam.view_angle = v;
    else if (n == "use_panini_projection") r->cam.use_panini_projection = b;
    else if (n == "panini_param") r->cam.panini_param = v;
    else if (n == "use_360_camera") r->cam.use_360_camera = b;
    else if (n == "use_180_camera") r->cam.use_180_camera = b;
    else if (n == "darken_by_distance") r->opt.darken_by_distance = b;
    else if (n == "gray_t_start") r->opt.gray_t_start = v;
    else if (n == "gray_t_size") r->opt.gray_t_size = v;
    else if (n == "draw_depth_map") r->opt.draw_depth_map = b;
    else if (n == "depth_map_min") r->opt.depth_map_min = v;
    else if (n == "depth_map_max") r->opt.depth_map_max = v;
    else if (n == "angle_color_disable") r->opt.angle_color_disable = b;
    else if (n == "grid_disable") r->opt.grid_disable = b;
    else if (n == "black_border_disable") r->opt.black_border_disable = b;
    else if (n == "offset_after_material") r->opt.offset_after_material = v;
    else if (n == "draw_side_by_side") r->opt.draw_side_by_side = b;
    else if (n == "in_subspace") r->cam.in_subspace = b;
    else if (n == "draw_anaglyph") r->opt.draw_anaglyph = b;
    else if (n == "anaglyph_mode") r->opt.anaglyph_mode = b;
    else if (n == "anaglyph_p") r->opt.anaglyph_p = v;
    else if (n == "anaglyph_q") r->opt.anaglyph_q = v;
    else if (n == "eye_distance") r->opt.eye_distance = v;
    else if (n == "swap_eyes") r->opt.swap_eyes = b;
    else if (n == "allow_teleport") r->cam.allow_teleport = b;    // RotateAroundCam toggles, src/main.rs:136-137
    else if (n == "stop_at_objects") r->cam.stop_at_objects = b;
    else if (n == "adaptive_aa_threshold") {  // T of ptl_renderer_draw_adaptive (-1 .. 255; the draw refuses anything else): no uniform depends on it
        r->adaptive_threshold = (int)v;
        return PTL_OK;
    }
    else return r->lanes.set_option(n, v);  // "concurrent_draws", "lane_stagger_us", "lane_fence", or PTL_UNKNOWN_UNIFORM
    ++r->options_version;
    return PTL_OK;
}

extern "C" int ptl_renderer_set_option(ptl_renderer* r, const char* name, double v) {
    if (!r || !name) return PTL_ERR_INVALID;
    std::string n = name;
    if (n == "specialize_static") return set_build_flag(r, PTL_FLAG_SPECIALIZE_STATIC, v > 0.5);
    if (n == "passes") return set_build_flag(r, PTL_FLAG_PASSES, v > 0.5);  // pass records beside the colour from the next build on (ptl_renderer_draw_passes)
    return set_plain_option(r, n, v);
}

extern "C" ptl_kernel* ptl_renderer_kernel(ptl_renderer* r) {
    if (!r) return nullptr;
    // the kernel the next draw would use: a specialised build follows the mode switches and the camera (also on a handle without a device, which
    // never draws); the scene's values are the draw's to examine
    if (!async_rejit(*r) && guarded([&] { return update_kernel(r, nullptr); }) != PTL_OK) return nullptr;  // ptl_last_error() says why
    return r->builds.kernel;
}
extern "C" int ptl_renderer_kernel_source(ptl_renderer* r, char** source) {
    if (!r || !source) return PTL_ERR_INVALID;
    *source = (char*)std::malloc(r->builds.kernel_source.size() + 1);
    if (!*source) return PTL_ERR_INVALID;
    std::memcpy(*source, r->builds.kernel_source.c_str(), r->builds.kernel_source.size() + 1);
    return PTL_OK;
}
extern "C" int ptl_renderer_rejit_count(ptl_renderer* r) { return r ? r->rejit_count : -1; }
extern "C" int ptl_renderer_affine_rays(ptl_renderer* r) { return r ? (r->builds.affine_rays ? 1 : 0) : -1; }
extern "C" int ptl_renderer_rejit_pending(ptl_renderer* r) {
    if (!r) return -1;
    return (r->builds.job || (r->builds.spec_kernel != nullptr && r->builds.kernel != r->builds.spec_kernel)) ? 1 : 0;
}
extern "C" void ptl_renderer_destroy(ptl_renderer* r) { delete r; }  // (~ptl_renderer and the order of its members: renderer.h)
