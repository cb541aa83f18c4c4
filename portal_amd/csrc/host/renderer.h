// renderer.h -- the two handle types of layer 2 of the C ABI and the parts a renderer is made of (internal).
//
// Each component struct holds its own fields, has its functions in ONE file (named at the struct) and tears itself down in its destructor; no
// other file writes its fields (plain reads are fine).  ptl_renderer holds the components by value.
#pragma once
#include <atomic>
#include <cmath>
#include <functional>
#include <map>
#include <memory>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "../../../include/portal_amd.h"
#include "codegen.h"
#include "internal.h"
#include "scene.h"

namespace ptl {

constexpr double kPi = 3.14159265358979323846264338327950288;
inline double deg2rad(double deg) { return deg / 180.0 * kPi; }  // src/gui/common.rs:23-25

struct NoCopy {  // a component owns device resources: one instance, where it was made
    NoCopy() = default;
    NoCopy(const NoCopy&) = delete;
    NoCopy& operator=(const NoCopy&) = delete;
};

// RotateAroundCam (src/main.rs:35-340), the fields the offline path reads.  renderer_camera.cpp
struct Camera {
    DVec3 look_at;
    double alpha = deg2rad(81.0), beta = deg2rad(64.0), r = 3.5;
    double view_angle = deg2rad(90.0);
    bool use_panini_projection = false;
    double panini_param = 1.0;
    bool use_360_camera = false, use_180_camera = false;
    DMat4 teleport_matrix = DMat4::identity();
    bool in_subspace = false, free_movement = false;
    bool allow_teleport = true, stop_at_objects = false;  // src/main.rs:136-137
    DVec3 prev_cam_pos;
    bool do_not_teleport_one_frame = false;  // src/main.rs:86,1218-1222
    int from = -1;                           // RotateAroundCam::from: scene camera in use, -1 = original
    DMat4 left_eye_matrix = DMat4::identity(), right_eye_matrix = DMat4::identity();  // src/main.rs:87-90,149-152
    bool left_eye_in_subspace = false, right_eye_in_subspace = false;

    DVec3 pos_vec() const { return DVec3(std::sin(beta) * std::cos(alpha), std::cos(beta), std::sin(beta) * std::sin(alpha)) * r; }
    DMat4 matrix() const {  // src/main.rs:286-304
        DVec3 pos = pos_vec() + look_at;
        DVec3 k = (look_at - pos).normalize();
        DVec3 i = k.cross(DVec3(0.0, 1.0, 0.0)).normalize();
        DVec3 j = k.cross(i).normalize();
        DVec3 p = free_movement ? look_at : pos;
        return teleport_matrix * DMat4::from_cols({i.x, i.y, i.z, 0.0}, {j.x, j.y, j.z, 0.0}, {k.x, k.y, k.z, 0.0}, {p.x, p.y, p.z, 1.0});
    }
    // The pose of `c`: angles, radius, look_at and free_movement; the teleport matrix and the subspace with `with_matrix`.  (What follows a
    // switch of cameras -- the free_movement fix-up of look_at, do_not_teleport_one_frame -- is the caller's: not every taker has both.)
    void take(const CalculatedCam& c, bool with_matrix = true) {
        alpha = c.alpha;
        beta = c.beta;
        r = c.r;
        look_at = c.look_at;
        free_movement = c.free_movement;
        if (with_matrix) {
            teleport_matrix = c.matrix;
            in_subspace = c.in_subspace;
        }
    }
};

// The renderer's plain options (set_plain_option): SceneRenderer defaults, src/main.rs:1021-1040
struct RenderOptions {
    double offset_after_material = 0.005, gray_t_start = 10.0, gray_t_size = 200.0;
    int render_depth = 100, aa_count = 1, aa_start = 0;
    bool draw_side_by_side = false, draw_depth_map = false, angle_color_disable = false, grid_disable = false,
         black_border_disable = false, darken_by_distance = true;
    double depth_map_min = 0.0, depth_map_max = 10.0, anaglyph_p = 0.29, anaglyph_q = 0.06;
    bool draw_anaglyph = false, anaglyph_mode = false;  // anaglyph_mode = "colorful" (src/main.rs:1551-1556)
    double eye_distance = 0.07;  // src/main.rs:1028-1029
    bool swap_eyes = false;
};

// What a specialised renderer has learnt about the states of the current stage / clip; another stage judges afresh (decide_rebuild).
struct StageMemory {
    std::set<std::string> keep_dynamic;   // clip-constant values that moved after all: run-time uniforms
    std::set<std::string> keep_unmasked;  // run-time matrices whose zero pattern did not hold: full products
    bool full_chains = false;             // a run-time matrix turned non-finite under a kernel with shortened products: keep the full chains
    // Affine rays (codegen.h KernelOptions::affine_rays) hold while every matrix that meets a ray -- the scene's (checked where the zero patterns
    // are, and by the generator) and the CAMERA's (a run-time value in every build: checked before every draw) -- has the bottom row 0 0 0 1.
    // One that does not switches the assumption off for this stage.
    bool no_affine = false;
    int affine_returns = 0;           // returns to affine rays in this stage (at most one: decide_rebuild)
    bool no_affine_just_set = false;  // the rebuild in progress is the one that switches them off
};

enum class Rebuild { none, quiet, counted };  // (quiet: a rebuild that ptl_renderer_rejit_count does not count)

// The current and the wanted build of a renderer, and its kernels.  renderer_builds.cpp
// PTL_FLAG_ASYNC_REJIT (bit 17): a specialised renderer whose baked values went stale does not stall the draw for the 1-3 s of a rebuild.
// It keeps two kernels -- `spec_kernel` (the specialised build of some scene state) and `dyn_kernel` (the un-specialised build: valid
// for every state) -- `kernel` points at the one in use, and a worker thread compiles the specialised source of the current state
// (hiprtc, no device); the draw that finds it finished, still matching the scene, loads the code object and switches.  Every
// build draws the same bits, so the pictures do not change with the switch -- only the kernel time does.
struct Build {  // everything a compile needs, detached from the scene handle (which the caller keeps changing)
    std::string source;
    std::vector<std::string> defines, desc_names;
    std::vector<ptl_uniform_desc> descs;
    size_t block_size = 0;
    std::vector<UniformUpload> baked;
};
struct Job {
    Build build;
    std::atomic<int> state{1};  // 1 running, 2 done, 3 failed
    std::vector<char> code;
    std::thread worker;
};
struct Builds : NoCopy {
    ptl_kernel* kernel = nullptr;
    ptl_kernel* spec_kernel = nullptr;
    ptl_kernel* dyn_kernel = nullptr;
    // how the kernel was built (needed to re-JIT a specialised kernel when the scene changes)
    unsigned long long kernel_scene_version = 0;
    std::string kernel_source, spec_source, failed_source;
    // What the wanted specialised build (the current kernel's, without PTL_FLAG_ASYNC_REJIT) has compiled in, and for which stage:
    std::map<std::string, int> kernel_switches;  // the mode switches (KernelOptions::baked_options)
    std::vector<std::pair<std::string, MatrixPattern>> masked;  // run-time matrices whose pattern (zeros, +-1) is compiled in (GeneratedKernel::masked)
    bool shortened = false;    // it skips zero terms of matrix products (PTL_DROP_ZERO_TERMS and / or masks): exact for finite vectors
    bool affine_rays = false;  // it was generated with PTL_AFFINE_RAYS
    std::vector<UniformUpload> baked;  // the scene values it has as literals
    StageRef kernel_stage;
    StageMemory stage;
    Build want;  // the build decide_rebuild generated last: compiled at once without PTL_FLAG_ASYNC_REJIT, by the worker with it
    std::shared_ptr<Job> job;

    void join_worker();  // (the worker owns nothing of ours, but a thread must be joined)
    ~Builds();           // spec_kernel and dyn_kernel (`kernel` is one of the two), or `kernel`
};

// "concurrent_draws" K > 1: draws on the caller's default stream go round-robin to K internal streams, each with its OWN instance of the
// kernel (ptl_kernel_clone: the same code object, another uniform block), so that consecutive draws with different uniforms -- the blur
// sub-frames of a clip frame -- overlap on the GPU (tail of one under the ramp of the next) instead of serialising on the one uniform
// block a module has.  Lane 0 draws with the active kernel itself.  ptl_renderer_join orders a stream behind everything issued so far.
// "lane_fence" 0 (round 6): a draw on a lane is the kernel's packet and nothing else -- no event on the caller's stream for the lane to
// wait on.  The caller then orders the reuse of a target buffer itself (ptl_renderer_join before it reads or overwrites one); what it
// gets is two frames in flight: frame n + 1's ramp under frame n's tail (tools/two_streams.py: headline 0.187 -> 0.177 ms, 1080p 0.035 -> 0.027).
// renderer_lanes.cpp
struct Lane {
    ptl_kernel* clone = nullptr;
    void* stream = nullptr;  // of the process-wide pool: never destroyed
    void* done = nullptr;
    bool busy = false;
};
struct Lanes : NoCopy {
    int concurrent = 1;
    bool lane_fence = true;
    // "lane_stagger_us" (round 6): lanes that start together stay together -- two launches queued at the same moment share the chip evenly, end at the
    // same moment, and their drains coincide (one drain per PAIR hidden instead of one per frame).  With this option the first draw of every lane but the
    // first, counted from the last join / host-side wait, is issued that many microseconds (x 2 / K) after the previous lane's: a host-side spin while the GPU
    // is busy with the first launch.  Half a launch is the natural value (bench.py sets it; profiles/r06/stagger.jsonl: 20-frame batches 0.1823 -> 0.180 ms).
    double lane_stagger_us = 0.0;
    unsigned lane_draws_since_join = 0;
    std::vector<Lane> lanes;
    ptl_kernel* lanes_of = nullptr;  // the kernel the clones were made from
    unsigned next_lane = 0;
    void* fence = nullptr;

    int set_option(const std::string& name, double v);  // "concurrent_draws", "lane_stagger_us", "lane_fence"; PTL_UNKNOWN_UNIFORM for another name
    void wait();                                        // host-side: everything issued on the lanes has finished
    int join(void* stream);                             // GPU-side: `stream` continues behind every draw issued so far
    void drop_clones();                                 // before the kernel they were cloned from goes away (they read its texel buffers)
    int draw(ptl_kernel* active, int device, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* stream);
    ~Lanes();  // waits, then the clones, the `done` events and the fence
};

// ptl_renderer_stage_slice: snapshots of the uniform block, one per slice, and which of them are staged since the last launch.
// A slice is traced by the kernel it was staged with: a rebuild between two stage calls (a value-baked build whose value moved, a mode
// switch, an adopted background build) compiles ANOTHER state in, and the earlier blocks are only right for the earlier kernel.
// A kernel that is replaced while staged slices name it is parked here (with its texel buffers) until those slices are launched.
// renderer_slices.cpp
struct StagedSlices : NoCopy {
    std::vector<std::vector<unsigned char>> blocks;
    unsigned mask = 0;
    std::vector<ptl_kernel*> kernels, parked;
    int aa_count[16] = {};  // `_aa_count` of each staged slice

    int stage(int index, ptl_kernel* kernel, int aa_count_now);
    bool all_staged(int n) const { return (mask & ((1u << n) - 1u)) == (1u << n) - 1u; }
    bool names(const ptl_kernel* k) const;  // a staged slice still has to be traced by `k`
    void park(ptl_kernel* k) { parked.push_back(k); }
    // The staged slices 0 .. n-1 as runs [j0, j1) of consecutive slices staged with the same kernel: each run goes out on the kernel it was
    // staged with -- one run for all n unless a rebuild fell between two stage calls (then the earlier slices keep the state THEIR kernel has
    // compiled in).  `run(k, j0, j1)` for one after the other, until one fails.
    template <typename Run>
    int for_each_run(int n, Run run) {
        int rc = PTL_OK;
        for (int j0 = 0; j0 < n && rc == PTL_OK;) {
            ptl_kernel* k = kernels[j0];
            int j1 = j0 + 1;
            while (j1 < n && kernels[j1] == k) ++j1;
            rc = run(k, j0, j1);
            j0 = j1;
        }
        return rc;
    }
    int stage_run(ptl_kernel* k, int j0, int j1);  // the snapshots of the run's slices become slices 0 .. j1-j0-1 of its kernel
    void drop();  // forget what was staged (after the launch; when the builds are torn down): holds released, parked kernels destroyed
    ~StagedSlices() { drop(); }

private:
    void release_hold(size_t j);
};

// The adaptive draws: the lists of refined pixels (list z at z * stride entries; a single frame has list 0 alone) and 16 counts, in device
// memory; owned here, reused from draw to draw.  A renderer has bit 28 or bit 29, so one kind of draw fills them.  renderer_draw.cpp
enum class AdaptiveDraw { none, frame, slices };
struct AdaptiveLists : NoCopy {
    void* lists = nullptr;
    void* counts = nullptr;
    size_t capacity = 0;            // entries, all lists together
    unsigned long long stride = 0;  // entries between two lists of the last draw
    AdaptiveDraw filled = AdaptiveDraw::none;  // the kind of draw they were last made ready for
    float ms[3] = {0.0f, 0.0f, 0.0f};          // the last timed adaptive draw: pass 1, classification, refine pass

    int reserve(int device, size_t pixels, int n, AdaptiveDraw kind);  // grown when they are too small, reused otherwise
    ~AdaptiveLists();  // (hipFree waits for the device: the last adaptive draw has finished)
};

// VideoRuntime (src/main.rs:771-925): per video, the sorted frame files and the frame currently bound
struct VideoState {
    bool scanned = false;
    std::vector<std::string> frames;
    long bound = -1;
};

}  // namespace ptl

struct ptl_scene {
    std::shared_ptr<ptl::Scene> scene;
    ptl::GeneratedKernel last;  // most recent generate_kernel_source() result
    std::vector<ptl_uniform_desc> descs;
    std::vector<std::string> desc_names;
    ptl::ZeroMaskCache mask_cache;  // zero patterns of the run-time matrices as probed last, and the scene state they belong to (codegen.h)
};

struct ptl_renderer {
    ptl_scene* owner = nullptr;
    std::shared_ptr<ptl::Scene> scene;
    ptl::Camera cam;
    ptl::RenderOptions opt;
    // draw-to-draw caching of the uploads: the reference re-evaluates and re-uploads every uniform on
    // every draw (src/main.rs:1413-1414); the values only change when the scene, an option, the camera
    // or the frame size does, so a draw of an unchanged state is just the kernel launch
    unsigned long long options_version = 1, uploaded_scene = 0, uploaded_options = 0;
    int uploaded_w = -1, uploaded_h = -1;
    int device = -1;
    unsigned flags = 0;
    std::string asset_root;
    // Round 6: option "check_affine" (or PTL_CHECK_AFFINE=1 in the environment): the first draw with every NEW affine-rays source first runs the
    // checking build of the same state at 64 x 36 (ptl_renderer_check_affine); a ray that met a product with another w switches the assumption off.
    bool check_affine_on_new_source = false;
    std::string checked_source;
    unsigned long long affine_violations_seen = 0;  // the most any check counted: above zero, affine rays stay off in every later stage
    // SceneRenderer::update state (src/main.rs:1430-1538)
    ptl::Camera prev_cam;
    bool has_prev_cam = false;
    ptl::CalculatedCam original_cam;  // egui memory "OriginalCam"
    int rejit_count = 0;
    std::vector<ptl::VideoState> videos;
    int adaptive_threshold = 4;  // option "adaptive_aa_threshold"

    // Teardown is the destructor's body, then these four in REVERSE order of declaration.  ptl_kernel_destroy waits on the kernel's own
    // ev_done and clones read their parent's texel buffers, so: the worker joined; the lanes waited for, their clones, events and fence
    // destroyed; the staged holds released, then the parked kernels destroyed; the adaptive buffers freed; spec_kernel and dyn_kernel (or
    // kernel) destroyed.
    ptl::Builds builds;
    ptl::AdaptiveLists adaptive;
    ptl::StagedSlices slices;
    ptl::Lanes lanes;
    ~ptl_renderer() { builds.join_worker(); }
};

namespace ptl {

// capi.cpp
int guarded(const std::function<int()>& fn);  // exceptions -> error codes + ptl_last_error()
void copy_str(char* dst, size_t cap, const std::string& s);
inline ptl_type to_c_type(UniformType t) { return (ptl_type)(int)t; }

// renderer_camera.cpp
DVec3 cam_pos(const Camera& c);
double calc_scale(const DMat4& m);
bool camera_is_affine(const ptl_renderer& r);
CalculatedCam calculated_of(const Camera& c);
CalculatedCam calculated_of(const CamSettings& c);
void send_camera_matrix(ptl_renderer* r);

// renderer_builds.cpp
bool async_rejit(const ptl_renderer& r);
void refresh_generated(ptl_scene* s, unsigned flags, const StageMemory* stage = nullptr, const std::map<std::string, int>* switches = nullptr);
int update_videos(ptl_renderer* r);
int update_kernel(ptl_renderer* r, const std::vector<UniformUpload>* values, Rebuild forced = Rebuild::none, char* log = nullptr, size_t log_cap = 0);
int async_select_kernel(ptl_renderer* r, const std::vector<UniformUpload>* values);
int rebuild_now(ptl_renderer* r, Rebuild why, char* log, size_t log_cap);
int set_build_flag(ptl_renderer* r, unsigned bit, bool on);   // options "specialize_static" (PTL_FLAG_SPECIALIZE_STATIC) and "passes" (PTL_FLAG_PASSES)
int rebuild_without_affine_rays(ptl_renderer* r);      // the check-affine belt counted a violation

// renderer_draw.cpp
int upload(ptl_kernel* k, const std::vector<UniformUpload>& ups);

}  // namespace ptl
