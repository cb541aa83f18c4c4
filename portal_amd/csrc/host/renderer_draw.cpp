// renderer_draw.cpp -- what a draw uploads and the draws themselves; the device buffers of the adaptive draws (renderer.h `AdaptiveLists`).
//   SceneRenderer::set_uniforms src/main.rs:1266-1359  -> builtin_uniforms()
//   SceneRenderer::draw_texture src/main.rs:1411-1428  -> ptl_renderer_draw
#include <algorithm>
#include <cstring>

#include "renderer.h"

using namespace ptl;

namespace ptl {

static std::vector<UniformUpload> builtin_uniforms(const ptl_renderer& r, int width, int height) {
    std::vector<UniformUpload> out;
    auto f1 = [&](const char* n, double v) {
        UniformUpload u;
        u.name = n;
        u.type = UniformType::Float1;
        u.f[0] = (float)v;
        out.push_back(u);
    };
    auto i1 = [&](const char* n, int v) {
        UniformUpload u;
        u.name = n;
        u.type = UniformType::Int1;
        u.i = v;
        out.push_back(u);
    };
    auto m4 = [&](const char* n, const DMat4& m) {
        UniformUpload u;
        u.name = n;
        u.type = UniformType::Mat4;
        m.to_f32(u.f);
        out.push_back(u);
    };
    {
        UniformUpload u;
        u.name = "_resolution";
        u.type = UniformType::Float2;
        u.f[0] = (float)width;
        u.f[1] = (float)height;
        out.push_back(u);
    }
    DMat4 cam = r.cam.matrix();
    m4("_camera", cam);
    m4("_camera_left_eye", r.cam.left_eye_matrix);
    m4("_camera_right_eye", r.cam.right_eye_matrix);
    i1("_left_eye_in_subspace", r.cam.left_eye_in_subspace ? 1 : 0);
    i1("_right_eye_in_subspace", r.cam.right_eye_in_subspace ? 1 : 0);
    m4("_camera_mul_inv", r.cam.teleport_matrix.inverse());
    i1("_camera_in_subspace", r.cam.in_subspace ? 1 : 0);
    f1("_view_angle", r.cam.view_angle);
    f1("_panini_param", r.cam.panini_param);
    i1("_use_panini_projection", r.cam.use_panini_projection ? 1 : 0);
    i1("_use_360_camera", r.cam.use_360_camera ? 1 : 0);
    i1("_use_180_camera", r.cam.use_180_camera ? 1 : 0);
    const RenderOptions& o = r.opt;
    i1("_ray_tracing_depth", o.render_depth);
    i1("_aa_count", o.aa_count);
    i1("_aa_start", o.aa_start);
    i1("_draw_side_by_side", o.draw_side_by_side ? 1 : 0);
    i1("_draw_anaglyph", o.draw_anaglyph ? 1 : 0);
    f1("_anaglyph_p", o.anaglyph_p);
    f1("_anaglyph_q", o.anaglyph_q);
    i1("_anaglyph_mode", o.anaglyph_mode ? 1 : 0);
    i1("_draw_depth_map", o.draw_depth_map ? 1 : 0);
    f1("_depth_map_min", o.depth_map_min);
    f1("_depth_map_max", o.depth_map_max);
    f1("_offset_after_material", o.offset_after_material);
    f1("_t_start", o.gray_t_start);
    f1("_t_end", o.gray_t_start + o.gray_t_size);
    f1("_camera_scale", calc_scale(cam));
    f1("_left_eye_scale", calc_scale(r.cam.left_eye_matrix));
    f1("_right_eye_scale", calc_scale(r.cam.right_eye_matrix));
    i1("_angle_color_disable", o.angle_color_disable ? 1 : 0);
    i1("_grid_disable", o.grid_disable ? 1 : 0);
    i1("_black_border_disable", o.black_border_disable ? 1 : 0);
    i1("_darken_by_distance", o.darken_by_distance ? 1 : 0);
    i1("_teleport_external_ray", 0);
    return out;
}

int upload(ptl_kernel* k, const std::vector<UniformUpload>& ups) {
    for (const UniformUpload& u : ups) {
        const void* v = u.type == UniformType::Int1 ? (const void*)&u.i : (const void*)u.f;
        int rc = ptl_kernel_set_uniform(k, u.name.c_str(), to_c_type(u.type), v);
        if (rc < 0) return rc;  // unknown names are tolerated (macroquad looks names up at upload time)
    }
    return PTL_OK;
}

static int prepare_draw(ptl_renderer* r, const ptl_frame* frame) {
    send_camera_matrix(r);
    // the scene's values (scene.set_uniforms): evaluated when a draw has to upload them anyway -- a draw of an unchanged state evaluates nothing
    std::vector<std::string> errors;
    std::vector<UniformUpload> values;
    const bool scene_moved = r->uploaded_scene != r->scene->version;
    if (scene_moved) values = evaluate_scene_uniforms(*r->scene, &errors);
    int rc = async_rejit(*r) ? async_select_kernel(r, scene_moved ? &values : nullptr) : update_kernel(r, scene_moved ? &values : nullptr);
    if (rc != PTL_OK) return rc;
    if (r->uploaded_scene != r->scene->version) {  // (also after a rebuild: a fresh uniform block)
        if (!scene_moved) values = evaluate_scene_uniforms(*r->scene, &errors);
        if (rc = upload(r->builds.kernel, values); rc < 0) return rc;
        r->uploaded_scene = r->scene->version;
    }
    if (r->uploaded_options != r->options_version || r->uploaded_w != frame->width || r->uploaded_h != frame->height) {
        rc = upload(r->builds.kernel, builtin_uniforms(*r, frame->width, frame->height));  // self.set_uniforms(w, h)
        if (rc < 0) return rc;
        r->uploaded_options = r->options_version;
        r->uploaded_w = frame->width;
        r->uploaded_h = frame->height;
    }
    return PTL_OK;
}

}  // namespace ptl

extern "C" int ptl_renderer_uniform_value(ptl_renderer* r, int width, int height, const char* name, float out16[16], int* n_values) {
    if (!r || !name || !out16) return PTL_ERR_INVALID;
    return guarded([&] {
        send_camera_matrix(r);  // Matrix::Camera uniforms: the value a draw would upload (prepare_draw does the same)
        auto all = builtin_uniforms(*r, width, height);
        auto scene_vals = evaluate_scene_uniforms(*r->scene, nullptr);
        all.insert(all.end(), scene_vals.begin(), scene_vals.end());
        for (const UniformUpload& u : all) {
            if (u.name != name) continue;
            int n = u.type == UniformType::Mat4 ? 16 : u.type == UniformType::Float2 ? 2 : u.type == UniformType::Float3 ? 3 : 1;
            if (u.type == UniformType::Int1) out16[0] = (float)u.i;
            else std::memcpy(out16, u.f, sizeof(float) * n);
            if (n_values) *n_values = n;
            return PTL_OK;
        }
        return (int)PTL_UNKNOWN_UNIFORM;
    });
}

extern "C" int ptl_renderer_stage_slice(ptl_renderer* r, const ptl_frame* frame, int index) {
    if (!r || !frame || index < 0 || index >= 16) return PTL_ERR_INVALID;
    return guarded([&] {
        int rc = prepare_draw(r, frame);
        if (rc < 0) return rc;
        return r->slices.stage(index, r->builds.kernel, r->opt.aa_count);
    });
}

// A batch of staged slices: one launch per run of slices staged with the same kernel, on the caller's stream.  `out_passes`: the slices' pass
// records (slice z at out_passes + z * slice_pixels records, `passes_bytes` in all), or null for the launch without them.  `entry`: who says so
static int draw_staged_slices(const char* entry, ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes,
                              unsigned long long slice_pixels, void* stream, float* elapsed_ms) {
    return guarded([&] {
        if (!r->slices.all_staged(n)) {
            set_last_error(std::string(entry) + ": slices 0 .. n-1 are not all staged (ptl_renderer_stage_slice) since the last launch");
            return (int)PTL_ERR_INVALID;
        }
        if (int jrc = r->lanes.join(stream); jrc != PTL_OK) return jrc;
        float total_ms = 0.0f;
        const int rc = r->slices.for_each_run(n, [&](ptl_kernel* k, int j0, int j1) {
            int rc = r->slices.stage_run(k, j0, j1);
            float ms = 0.0f;
            void* out8 = out_rgba8 ? static_cast<unsigned char*>(out_rgba8) + (size_t)j0 * slice_pixels * 4 : nullptr;
            void* out32 = out_rgba32f ? static_cast<float*>(out_rgba32f) + (size_t)j0 * slice_pixels * 4 : nullptr;
            if (rc == PTL_OK && !out_passes) rc = ptl_kernel_render_slices(k, frame, j1 - j0, out8, out32, slice_pixels, stream, elapsed_ms ? &ms : nullptr);
            if (rc == PTL_OK && out_passes) {
                void* outp = static_cast<ptl_pass_record*>(out_passes) + (size_t)j0 * slice_pixels;
                const size_t left = passes_bytes - sizeof(ptl_pass_record) * (size_t)j0 * slice_pixels;
                rc = ptl_kernel_render_slices_passes(k, frame, j1 - j0, out8, out32, outp, left, slice_pixels, stream, elapsed_ms ? &ms : nullptr);
            }
            total_ms += ms;
            return rc;
        });
        if (elapsed_ms) *elapsed_ms = total_ms;
        r->slices.drop();
        return rc;
    });
}

extern "C" int ptl_renderer_draw_slices(ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels,
                                        void* stream, float* elapsed_ms) {
    if (!r || !frame || n < 1 || n > 16) return PTL_ERR_INVALID;
    return draw_staged_slices("ptl_renderer_draw_slices", r, frame, n, out_rgba8, out_rgba32f, nullptr, 0, slice_pixels, stream, elapsed_ms);
}

// The same batch with the slices' pass records (renderers with PTL_FLAG_PASSES / option "passes"): slice z at out_passes + z * slice_pixels records.
extern "C" int ptl_renderer_draw_slices_passes(ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes,
                                               unsigned long long slice_pixels, void* stream, float* elapsed_ms) {
    if (!r || !frame || n < 1 || n > 16) return PTL_ERR_INVALID;
    if (!out_passes || passes_bytes < sizeof(ptl_pass_record) * (unsigned long long)(n - 1) * slice_pixels) return PTL_ERR_INVALID;  // (layer 1 checks the last run's share)
    return draw_staged_slices("ptl_renderer_draw_slices_passes", r, frame, n, out_rgba8, out_rgba32f, out_passes, passes_bytes, slice_pixels, stream, elapsed_ms);
}

extern "C" int ptl_renderer_join(ptl_renderer* r, void* stream) {
    if (!r) return PTL_ERR_INVALID;
    return guarded([&] { return r->lanes.join(stream); });
}

// The dynamic belt behind `snippets_keep_rays_affine` (VERDICT r5 #2c).  A sibling renderer of the same scene handle and the same specialisation is
// built with PTL_FLAG_CHECK_AFFINE (general products; the assumption sites count what arrives with another w), gets this renderer's camera and
// options, and draws the current state once at width x height.  A count above zero means: a kernel that ASSUMES w = 1 / 0 would have computed with
// other values for this very state -- the renderer then switches affine rays off for its stage and rebuilds (one re-JIT, the frames stay right).
static int check_affine_now(ptl_renderer* r, int width, int height, unsigned long long* violations) {
    if (r->device < 0) return PTL_ERR_NO_DEVICE;
    const unsigned flags = (r->flags & ~(PTL_FLAG_ASYNC_REJIT | PTL_FLAG_SLICES | PTL_FLAG_REFINE | PTL_FLAG_REFINE_SLICES | PTL_FLAG_NO_AFFINE_RAYS)) | PTL_FLAG_CHECK_AFFINE | PTL_FLAG_COUNT_SEGMENTS |
                           PTL_FLAG_QUICK_JIT;  // not async, no slices entry; checking + counting, quick JIT
    std::vector<char> log(1 << 16);
    ptl_renderer* sib = nullptr;
    int rc = ptl_renderer_create(r->owner, r->device, r->asset_root.c_str(), flags, &sib, log.data(), log.size());
    if (rc != PTL_OK) return rc;
    sib->cam = r->cam;
    sib->opt = r->opt;
    ++sib->options_version;
    ptl_frame f{};
    f.width = width;
    f.height = height;
    f.rb_phase = 0;
    f.rb_stride = 1;
    std::vector<uint8_t> pixels((size_t)width * height * 4);
    uint64_t count = 0;
    rc = ptl_renderer_draw_to_host(sib, &f, pixels.data(), nullptr, &count, nullptr);
    ptl_renderer_destroy(sib);
    if (rc != PTL_OK) return rc;
    if (violations) *violations = count;
    r->affine_violations_seen = std::max<unsigned long long>(r->affine_violations_seen, count);  // (a later clean check -- another view -- clears nothing)
    r->checked_source = r->builds.kernel_source;
    if (count > 0 && r->builds.affine_rays && !r->builds.stage.no_affine) {
        if (rc = rebuild_without_affine_rays(r); rc != PTL_OK) return rc;
        r->checked_source = r->builds.kernel_source;
        set_last_error("check_affine: " + std::to_string(count) + " ray halves met a product with a w that is not 1 / 0: affine rays switched off for this stage");
    }
    return PTL_OK;
}
extern "C" int ptl_renderer_check_affine(ptl_renderer* r, int width, int height, unsigned long long* violations) {
    if (!r || width < 1 || height < 1) return PTL_ERR_INVALID;
    return guarded([&] {
        ptl_frame f{};
        f.width = width;
        f.height = height;
        f.rb_stride = 1;
        int rc = prepare_draw(r, &f);  // (the state a draw would see: pending rebuilds done, so that `kernel_source` is what would be launched)
        if (rc < 0) return rc;
        return check_affine_now(r, width, height, violations);
    });
}
// (before a draw: option "check_affine" / PTL_CHECK_AFFINE=1 -- once per new source that has affine rays)
static int check_affine_if_asked(ptl_renderer* r, const ptl_frame* frame) {
    if (!r->check_affine_on_new_source || !r->builds.affine_rays || r->builds.stage.no_affine || r->device < 0 || r->checked_source == r->builds.kernel_source) return PTL_OK;
    int rc = check_affine_now(r, 64, 36, nullptr);
    if (rc != PTL_OK) return rc;
    return prepare_draw(r, frame);  // (the rebuilt kernel, if any, wants its uniforms)
}

extern "C" int ptl_renderer_draw(ptl_renderer* r, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* segments, void* stream,
                                 float* elapsed_ms) {
    if (!r || !frame) return PTL_ERR_INVALID;
    return guarded([&] {
        int rc = prepare_draw(r, frame);
        if (rc < 0) return rc;
        if (rc = check_affine_if_asked(r, frame); rc < 0) return rc;
        if (r->lanes.concurrent > 1 && r->device >= 0 && !elapsed_ms && !segments) return r->lanes.draw(r->builds.kernel, r->device, frame, out_rgba8, out_rgba32f, stream);
        // (a timed or counting draw, and every draw of a renderer without lanes: on the caller's stream, behind what the lanes still hold)
        if (int jrc = r->lanes.join(stream); jrc != PTL_OK) return jrc;
        return ptl_kernel_render(r->builds.kernel, frame, out_rgba8, out_rgba32f, segments, stream, elapsed_ms);
    });
}
// A draw with the pass records (renderers with PTL_FLAG_PASSES / option "passes"): on the caller's stream behind what the lanes still hold,
// like a timed draw.  Layer 1 refuses a kernel without the records and a buffer that is too small.
extern "C" int ptl_renderer_draw_passes(ptl_renderer* r, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes, void* segments,
                                        void* stream, float* elapsed_ms) {
    if (!r || !frame) return PTL_ERR_INVALID;
    return guarded([&] {
        int rc = prepare_draw(r, frame);
        if (rc < 0) return rc;
        if (rc = check_affine_if_asked(r, frame); rc < 0) return rc;
        if (int jrc = r->lanes.join(stream); jrc != PTL_OK) return jrc;
        return ptl_kernel_render_passes(r->builds.kernel, frame, out_rgba8, out_rgba32f, out_passes, passes_bytes, segments, stream, elapsed_ms);
    });
}
// ---- adaptive anti-aliasing (include/portal_amd.h has the contract) ------------------------------------------------------------------
// What both adaptive draws refuse, in this order: a frame that is not whole or has more than 2^31 pixels, room for less than a frame
// between two slices (`slice_pixels`; null for a single frame), a threshold outside its range, a renderer without the draw's flag
// (`without_flag`: the rest of that sentence).
static int check_adaptive_draw(const char* who, const ptl_renderer* r, const ptl_frame* frame, const unsigned long long* slice_pixels, unsigned flag, const char* without_flag) {
    auto refuse = [&](const std::string& why) {
        set_last_error(std::string(who) + ": " + why);
        return (int)PTL_ERR_INVALID;
    };
    if (frame->rb_stride != 1 || frame->rb_phase != 0 || frame->in_place) return refuse("a whole frame only (rb_phase 0, rb_stride 1, not in_place)");
    if ((long long)frame->width * frame->height > (1LL << 31)) return PTL_ERR_INVALID;
    if (slice_pixels && *slice_pixels < (unsigned long long)frame->width * (unsigned long long)frame->height) return refuse("slice_pixels is smaller than width * height");
    if (r->adaptive_threshold < -1 || r->adaptive_threshold > 255) return refuse("option adaptive_aa_threshold is outside -1 .. 255");
    if (!(r->flags & flag)) return refuse(std::string("the renderer was created without ") + without_flag);
    return PTL_OK;
}
int AdaptiveLists::reserve(int device, size_t pixels, int n, AdaptiveDraw kind) {
    if (capacity < pixels * (size_t)n) {
        if (lists) ptl_device_free(lists);
        lists = nullptr;
        capacity = 0;
        if (int rc = ptl_device_alloc(device, pixels * (size_t)n * 4, &lists); rc != PTL_OK) return rc;
        capacity = pixels * (size_t)n;
    }
    if (!counts)
        if (int rc = ptl_device_alloc(device, 16 * 4, &counts); rc != PTL_OK) return rc;
    stride = pixels;
    filled = kind;
    return PTL_OK;
}
AdaptiveLists::~AdaptiveLists() {
    if (lists) ptl_device_free(lists);
    if (counts) ptl_device_free(counts);
}
static void report_adaptive_times(ptl_renderer* r, const float ms[3], float* elapsed_ms) {
    if (!elapsed_ms) return;
    *elapsed_ms = ms[0] + ms[1] + ms[2];
    std::copy(ms, ms + 3, r->adaptive.ms);
}

// One frame: the frame with one sample per pixel, the classification of its RGBA8 bytes, and the flagged pixels again with the full
// `_aa_count` -- three launches on the caller's stream, nothing read back in between.  `_aa_count` is a run-time builtin in every build, so
// ONE kernel serves both passes: prepare_draw runs once, in front of pass 1, and is the only place where a kernel is rebuilt or a
// background build adopted -- never between the passes.
extern "C" int ptl_renderer_draw_adaptive(ptl_renderer* r, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* stream, float* elapsed_ms) {
    if (!r || !frame || !out_rgba8 || frame->width <= 0 || frame->height <= 0) return PTL_ERR_INVALID;
    if (int rc = check_adaptive_draw("ptl_renderer_draw_adaptive", r, frame, nullptr, PTL_FLAG_REFINE, "PTL_FLAG_REFINE: its kernel has no refine entry"); rc != PTL_OK) return rc;
    if (r->device < 0) return PTL_ERR_NO_DEVICE;
    return guarded([&] {
        int rc = prepare_draw(r, frame);
        if (rc < 0) return rc;
        if (rc = check_affine_if_asked(r, frame); rc < 0) return rc;
        if (int jrc = r->lanes.join(stream); jrc != PTL_OK) return jrc;
        if (rc = r->adaptive.reserve(r->device, (size_t)frame->width * (size_t)frame->height, 1, AdaptiveDraw::frame); rc != PTL_OK) return rc;
        float ms[3] = {0.0f, 0.0f, 0.0f};
        const int full = r->opt.aa_count, one = 1;
        // With N = 1 the call is a plain draw and the list is empty: T = 255 flags nothing, and the refine pass is not launched.
        const bool plain = full <= 1;
        if (!plain) ptl_kernel_set_uniform(r->builds.kernel, "_aa_count", PTL_I32, &one);
        rc = ptl_kernel_render(r->builds.kernel, frame, out_rgba8, out_rgba32f, nullptr, stream, elapsed_ms ? &ms[0] : nullptr);
        if (!plain) ptl_kernel_set_uniform(r->builds.kernel, "_aa_count", PTL_I32, &full);  // (the host copy is again what prepare_draw left; uploaded in front of the refine pass)
        if (rc == PTL_OK)
            rc = ptl_aa_edges(r->device, out_rgba8, frame->width, frame->height, plain ? 255 : r->adaptive_threshold, r->adaptive.lists, r->adaptive.counts, stream,
                              elapsed_ms ? &ms[1] : nullptr);
        if (rc == PTL_OK && !plain)
            rc = ptl_kernel_render_refine(r->builds.kernel, frame, r->adaptive.lists, r->adaptive.counts, out_rgba8, out_rgba32f, nullptr, stream, elapsed_ms ? &ms[2] : nullptr);
        report_adaptive_times(r, ms, elapsed_ms);
        return rc;
    });
}
extern "C" int ptl_renderer_adaptive_result(ptl_renderer* r, void** list, void** count) {
    if (!r || r->adaptive.filled != AdaptiveDraw::frame) return PTL_ERR_INVALID;
    if (list) *list = r->adaptive.lists;
    if (count) *count = r->adaptive.counts;
    return PTL_OK;
}
extern "C" int ptl_renderer_adaptive_times(ptl_renderer* r, float ms3[3]) {
    if (!r || !ms3) return PTL_ERR_INVALID;
    std::copy(r->adaptive.ms, r->adaptive.ms + 3, ms3);
    return PTL_OK;
}
// A batch of staged slices: per run of slices staged with the same kernel, pass 1 with every slice's `_aa_count` set to 1, the
// classification of the sub-frames it wrote, and the refine pass with the slices re-staged from the snapshots -- their own `_aa_count` --
// on the kernel the run was staged with.  Nothing is read back, nothing is rebuilt.  The texture holds of ptl_renderer_stage_slice stay
// until StagedSlices::drop at the end: pass 1's launch releases no texel buffer.
extern "C" int ptl_renderer_draw_slices_adaptive(ptl_renderer* r, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels,
                                                 void* stream, float* elapsed_ms) {
    if (!r || !frame || !out_rgba8 || n < 1 || n > 16 || frame->width <= 0 || frame->height <= 0) return PTL_ERR_INVALID;
    if (int rc = check_adaptive_draw("ptl_renderer_draw_slices_adaptive", r, frame, &slice_pixels, PTL_FLAG_REFINE_SLICES,
                                     "PTL_FLAG_REFINE_SLICES: its kernel has no refine entry over slices");
        rc != PTL_OK)
        return rc;
    if (!r->slices.all_staged(n)) {
        set_last_error("ptl_renderer_draw_slices_adaptive: slices 0 .. n-1 are not all staged (ptl_renderer_stage_slice) since the last launch");
        return PTL_ERR_INVALID;
    }
    if (r->device < 0) return PTL_ERR_NO_DEVICE;
    return guarded([&] {
        if (int jrc = r->lanes.join(stream); jrc != PTL_OK) return jrc;
        if (int arc = r->adaptive.reserve(r->device, (size_t)frame->width * (size_t)frame->height, n, AdaptiveDraw::slices); arc != PTL_OK) return arc;
        const unsigned long long stride = r->adaptive.stride;
        // With N = 1 in every slice the call is a plain draw_slices and the lists are empty: T = 255 flags nothing, no refine launch.
        bool plain = true;
        for (int j = 0; j < n; ++j) plain = plain && r->slices.aa_count[j] <= 1;
        float ms[3] = {0.0f, 0.0f, 0.0f};
        const int one = 1;
        const int rc = r->slices.for_each_run(n, [&](ptl_kernel* k, int j0, int j1) {
            const int count = j1 - j0;
            void* out8 = static_cast<unsigned char*>(out_rgba8) + (size_t)j0 * slice_pixels * 4;
            void* out32 = out_rgba32f ? static_cast<float*>(out_rgba32f) + (size_t)j0 * slice_pixels * 4 : nullptr;
            void* lists = static_cast<unsigned int*>(r->adaptive.lists) + (size_t)j0 * stride;
            void* counts = static_cast<unsigned int*>(r->adaptive.counts) + j0;
            float t[3] = {0.0f, 0.0f, 0.0f};
            int rc = r->slices.stage_run(k, j0, j1);
            for (int j = j0; j < j1 && rc == PTL_OK && !plain; ++j) rc = ptl_kernel_set_staged_uniform(k, j - j0, "_aa_count", PTL_I32, &one);
            if (rc == PTL_OK) rc = ptl_kernel_render_slices(k, frame, count, out8, out32, slice_pixels, stream, elapsed_ms ? &t[0] : nullptr);
            if (rc == PTL_OK)
                rc = ptl_aa_edges_slices(r->device, out8, slice_pixels, count, frame->width, frame->height, plain ? 255 : r->adaptive_threshold, lists, stride, counts, stream,
                                         elapsed_ms ? &t[1] : nullptr);
            if (rc == PTL_OK && !plain) {
                rc = r->slices.stage_run(k, j0, j1);  // the snapshots again: every slice's own `_aa_count`
                if (rc == PTL_OK) rc = ptl_kernel_render_slices_refine(k, frame, count, lists, stride, counts, out8, out32, slice_pixels, nullptr, stream, elapsed_ms ? &t[2] : nullptr);
            }
            for (int p = 0; p < 3; ++p) ms[p] += t[p];
            return rc;
        });
        report_adaptive_times(r, ms, elapsed_ms);
        r->slices.drop();
        return rc;
    });
}
extern "C" int ptl_renderer_adaptive_slices_result(ptl_renderer* r, void** lists, unsigned long long* list_stride, void** counts) {
    if (!r || r->adaptive.filled != AdaptiveDraw::slices) return PTL_ERR_INVALID;
    if (lists) *lists = r->adaptive.lists;
    if (list_stride) *list_stride = r->adaptive.stride;
    if (counts) *counts = r->adaptive.counts;
    return PTL_OK;
}
extern "C" int ptl_renderer_draw_to_host(ptl_renderer* r, const ptl_frame* frame, uint8_t* host_rgba8, float* host_rgba32f,
                                         uint64_t* host_segments, float* elapsed_ms) {
    if (!r || !frame) return PTL_ERR_INVALID;
    return guarded([&] {
        int rc = prepare_draw(r, frame);
        if (rc < 0) return rc;
        if (rc = check_affine_if_asked(r, frame); rc < 0) return rc;
        r->lanes.wait();
        return ptl_kernel_render_to_host(r->builds.kernel, frame, host_rgba8, host_rgba32f, host_segments, elapsed_ms);
    });
}
extern "C" int ptl_renderer_prebuild_teleport(ptl_renderer* r) {
    if (!r || !r->builds.kernel) return PTL_ERR_INVALID;
    return guarded([&] { return ptl_kernel_prebuild_teleport(r->builds.kernel); });
}
extern "C" int ptl_renderer_teleport_ray(ptl_renderer* r, const double a[3], const double b[3], double out_pos[3], int* hit_object,
                                         int* changed_subspace, int* teleported) {
    if (!r || !a || !b) return PTL_ERR_INVALID;
    return guarded([&] {
        ptl_frame zero{0, 0, 0, 1, 0};  // the reference calls self.set_uniforms(0., 0.) here
        int rc = prepare_draw(r, &zero);
        if (rc < 0) return rc;
        r->lanes.wait();  // (the query runs on the primary kernel's block, on the default stream)
        int one = 1;
        ptl_kernel_set_uniform(r->builds.kernel, "teleport_light_u", PTL_I32, &one);  // src/main.rs:1367 (a scene without it: no-op)
        float fa[3] = {(float)a[0], (float)a[1], (float)a[2]}, fb[3] = {(float)b[0], (float)b[1], (float)b[2]}, pos[3] = {0, 0, 0};
        rc = ptl_kernel_teleport_ray(r->builds.kernel, fa, fb, pos, hit_object, changed_subspace, teleported);
        r->uploaded_scene = 0;  // teleport_light_u was overridden: the next draw re-uploads the scene values
        r->uploaded_w = -1;
        if (rc == PTL_OK && out_pos)
            for (int k = 0; k < 3; ++k) out_pos[k] = (double)pos[k];
        return rc;
    });
}
