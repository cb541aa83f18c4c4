// kernel.cpp -- layer 1 of the C ABI: compile / set_uniform / set_texture / render.
// The MI355X replacement for the macroquad material API the reference calls at
// src/gui/scene.rs:1132-1143 and src/main.rs:1077-1078,1269-1358,1424-1425.
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <fstream>
#include <iterator>
#include <memory>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/portal_amd.h"
#include "hip_api.h"
#include "internal.h"

using namespace ptl;

static constexpr int kMaxSlices = 16;

static size_t type_size(ptl_type t) {
    switch (t) {
        case PTL_MAT4: return 64;
        case PTL_F32: case PTL_I32: return 4;
        case PTL_VEC2: return 8;
        case PTL_VEC3: return 12;
        case PTL_SAMPLER: return 16;
    }
    return 0;
}

struct ptl_kernel {
    int device = -1;
    std::vector<char> code;
    hip::hipModule_t module = nullptr;
    hip::hipFunction_t fn = nullptr;
    hip::hipFunction_t teleport_fn = nullptr;  // optional: ptl_teleport_kernel
    hip::hipFunction_t derive_fn = nullptr;    // optional: ptl_derive_kernel, the uniform prologue (runs after every upload)
    hip::hipFunction_t refine_fn = nullptr;    // optional: ptl_render_refine_kernel, the list-driven render entry (sources generated with PTL_FLAG_REFINE)
    bool has_refine = false;                   // the source names that entry (known without a device)
    hip::hipFunction_t refine_slices_fn = nullptr;  // optional: ptl_render_refine_slices_kernel, the list-driven entry over slices (PTL_FLAG_REFINE_SLICES)
    bool has_refine_slices = false;                 // the source names that entry (known without a device); such a source has the slices entry too
    bool has_passes = false;                        // the source was generated with PTL_FLAG_PASSES: its render entry takes `out_passes` behind `in_place`
    void* dev_block = nullptr;  // address of __constant__ ptl_u
    size_t dev_block_size = 0;
    std::vector<unsigned char> shadow;  // host copy of the uniform block
    bool dirty = true;
    struct Slot {
        ptl_type type;
        size_t offset;
    };
    std::map<std::string, Slot> slots;
    std::map<std::string, void*> textures;  // sampler -> device texel buffer
    // Staged slices carry sampler records: a texel buffer that a staged slice may still name is not freed by a re-bind of its sampler (a video
    // texture that steps to its next frame between two sub-frames of one launch) but retired, and freed behind the next launch.
    std::vector<void*> retired_textures;
    bool staged_since_launch = false;  // ptl_kernel_stage_slice* since the last launch: its sampler records are live
    int texture_holds = 0;             // ptl_kernel_hold_textures: a caller keeps snapshots of the block that name texel buffers
    hip::hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hip::hipEvent_t ev_done = nullptr;  // recorded behind every render launch: what destroy / a teleport query wait for.  Owned here, so it
                                        // stays valid when the caller has already destroyed the stream it launched on (a torch stream, a
                                        // user stream freed before the renderer: Python __del__ order is unspecified).
    // A module generated with the slices entry (the `slices` sections of device/ptl_entry.h): its render entry `ptl_render_slices_kernel` reads the uniform
    // block of slice blockIdx.z from a device buffer of blocks, so one launch can trace several frames with different uniforms.  The module's
    // own global block stays what the camera-teleport query uses.
    bool sliced = false;
    bool affine_rays = false;  // compiled with PTL_AFFINE_RAYS: its products assume o.w = 1 / d.w = 0, which a matrix with another bottom row than 0 0 0 1 breaks
    hip::hipFunction_t derive_slices_fn = nullptr;
    void* dev_slices = nullptr;           // kMaxSlices blocks of dev_block_size bytes
    std::vector<unsigned char> staged;    // host side of it: slice j at j * dev_block_size (ptl_kernel_stage_slice)
    bool slice0_dirty = true;             // slice 0 of the buffer no longer holds `shadow` (a single draw uses slice 0)
    // A module compiled with -DPTL_RENDER_MODULE has no camera-teleport entry (ptl_entry.h): that entry is a second copy of the whole tracer
    // and a fifth of every build, and only a camera that moves asks for it.  Such a kernel keeps what its build was made from and compiles
    // the other half -- the same source with -DPTL_TELEPORT_MODULE: the teleport entry and the prologue, no render entry -- at the first query
    // (ptl_kernel_teleport_ray / ptl_kernel_prebuild_teleport).  The companion has a uniform block of its own; a query copies this kernel's.
    bool split = false;
    std::string source;
    std::vector<std::string> defines;
    ptl_kernel* companion = nullptr;
    unsigned block_waves = 4;       // PTL_BLOCK_WAVES (experiments with narrower workgroups), read once at compile time
    void* last_stream = nullptr;    // the stream of the most recent render launch ...
    bool launched = false;          // ... which may still be reading the uniform block
};

namespace ptl {
thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }
}  // namespace ptl

namespace {

using Options = std::vector<std::string>;

struct Destroy {
    void operator()(ptl_kernel* p) const { ptl_kernel_destroy(p); }  // error paths: unload the module, free events and textures
};
using KernelPtr = std::unique_ptr<ptl_kernel, Destroy>;

bool hip_ok(const hip::Runtime* rt, int err, const char* what) {
    if (err == 0) return true;
    set_last_error(std::string(what) + ": " + (rt ? rt->hipGetErrorString(err) : "?") + " (" + std::to_string(err) + ")");
    if (rt) rt->hipGetLastError();  // reported through our own status code: do not leave it sticky in the shared runtime
    return false;
}

unsigned long long fnv1a(const std::string& s, unsigned long long h = 1469598103934665603ull) {
    for (unsigned char c : s) {
        h ^= c;
        h *= 1099511628211ull;
    }
    return h;
}

std::string opt_level(bool quick) {
    const char* e = std::getenv("PTL_JIT_OPT");  // "-O1" (rounds 1-2), "-O2", "-Os" ...: A/B measurements
    if (e && e[0] == '-' && e[1] == 'O') return e;
    // PTL_QUICK_JIT (flags bit 18): the build is wanted NOW and used briefly -- one frame from the CLI (2.4 s of -O3 hiprtc for a 0.33 ms kernel
    // that -O1 gives as a 0.36 ms one in 1.2 s), the un-specialised kernel a clip starts on while its specialised one compiles
    return quick ? "-O1" : "-O3";
}

// The largest value a key of the code object's kernel metadata (msgpack in the AMDGPU note: ".vgpr_count", ".vgpr_spill_count",
// ".private_segment_fixed_size" ...) takes over the kernels of the module; -1 when the key does not occur.  A scan for the key's bytes
// followed by a msgpack unsigned integer -- enough for a decision about an occupancy hint, no msgpack reader.
// `kernel_prefix`: only the kernels whose name starts with it (the render entries "ptl_render": a one-module build also holds the one-wave
// teleport and prologue entries, whose registers say nothing about the render kernel's occupancy); when no kernel of the module has such a
// name -- a hand-written layer-1 source -- every kernel counts.  A kernel's map lists its keys in alphabetical order, so the most recent
// ".name" string in front of ".private_segment_fixed_size" / ".vgpr_count" / ".vgpr_spill_count" is the kernel's own (its arguments' names
// sit inside ".args", ahead of it).
int code_object_note_max(const std::vector<char>& code, const char* key, const char* kernel_prefix = nullptr) {
    const size_t n = std::strlen(key);
    if (kernel_prefix && *kernel_prefix) {
        const std::string prefix = kernel_prefix;
        bool any = false;
        for (size_t i = 0; i + 6 + prefix.size() < code.size() && !any; ++i)
            if (std::memcmp(code.data() + i, "\xa5.name", 6) == 0) {
                const unsigned char h = (unsigned char)code[i + 6];
                const size_t at = (h & 0xe0) == 0xa0 ? i + 7 : (h == 0xd9 ? i + 8 : 0);
                any = at != 0 && at + prefix.size() <= code.size() && std::memcmp(code.data() + at, prefix.data(), prefix.size()) == 0;
            }
        if (!any) kernel_prefix = nullptr;
    }
    int best = -1;
    bool wanted = !kernel_prefix;
    for (size_t i = 0; i + n + 1 < code.size(); ++i) {
        if (kernel_prefix && i + 8 < code.size() && std::memcmp(code.data() + i, "\xa5.name", 6) == 0) {
            const unsigned char h = (unsigned char)code[i + 6];
            const size_t at = (h & 0xe0) == 0xa0 ? i + 7 : (h == 0xd9 ? i + 8 : 0);
            const size_t len = std::strlen(kernel_prefix);
            wanted = at != 0 && at + len <= code.size() && std::memcmp(code.data() + at, kernel_prefix, len) == 0;
        }
        if (!wanted || std::memcmp(code.data() + i, key, n) != 0) continue;
        const unsigned char* p = reinterpret_cast<const unsigned char*>(code.data()) + i + n;
        const size_t left = code.size() - (i + n);
        long v = -1;
        if (p[0] <= 0x7f) v = p[0];
        else if (p[0] == 0xcc && left >= 2) v = p[1];
        else if (p[0] == 0xcd && left >= 3) v = (p[1] << 8) | p[2];
        else if (p[0] == 0xce && left >= 5) v = ((long)p[1] << 24) | (p[2] << 16) | (p[3] << 8) | p[4];
        if (v > best) best = (int)v;
    }
    return best;
}

// ---- the compile pipeline: request -> traits -> options -> cache / hiprtc + occupancy ladder -> module -------------------------------
struct CompileRequest {  // the arguments of ptl_kernel_compile
    int device;
    const char* source;
    const ptl_uniform_desc* uniforms; int n_uniforms;
    size_t block_size;
    const char* const* defines; int n_defines;
    char* log; size_t log_cap;
};

bool has_define(const CompileRequest& rq, const char* name) {
    for (int k = 0; k < rq.n_defines; ++k)
        if (std::strcmp(rq.defines[k], name) == 0) return true;
    return false;
}

struct BuildTraits {  // what the generator's defines say about the build (codegen.cpp sets them; a layer-1 caller may)
    bool affine_rays;            // PTL_AFFINE_RAYS: see ptl_kernel::affine_rays
    bool split, teleport_only;   // PTL_RENDER_MODULE / PTL_TELEPORT_MODULE, the two halves of a split build: see ptl_kernel::split
    bool fast;                   // PTL_FAST_MATH, the tolerance mode (device/ptl_glsl.h): contraction and approximate / and sqrt allowed
    bool quick, module_inliner;  // PTL_QUICK_JIT, PTL_JIT_MODULE_INLINER: see opt_level, compile_options
};

BuildTraits read_traits(const CompileRequest& rq) {
    return {has_define(rq, "PTL_AFFINE_RAYS"), has_define(rq, "PTL_RENDER_MODULE"), has_define(rq, "PTL_TELEPORT_MODULE"),
            has_define(rq, "PTL_FAST_MATH"), has_define(rq, "PTL_QUICK_JIT"), has_define(rq, "PTL_JIT_MODULE_INLINER")};
}

Options compile_options(const CompileRequest& rq, const BuildTraits& t) {
    const char* arch = std::getenv("PTL_OFFLOAD_ARCH");
    Options o = {std::string("--offload-arch=") + (arch ? arch : "gfx950"),
                 // -O3 WITHOUT the SLP vectoriser, measured on the round-3 kernels (profiles/r03/variants9_opt_level.jsonl, same
                 // frame hashes): against -O1 the baked kernels are 10-23 % faster (portal_in_portal 4K 0.364 -> 0.327 ms,
                 // triple_portal 0.333 -> 0.300, monoportal 1080p 0.069 -> 0.055, plus_ultra 0.99 -> 0.76), the Int-baked and
                 // un-specialised ones 2-30 % (plus_ultra un-specialised 4.5 -> 2.0 ms) with ONE exception, the un-specialised
                 // portal_in_portal (0.78 -> 0.88: PTL_JIT_OPT=-O1 restores it; bench.py reports the better of the two).
                 // Rounds 1-2 shipped -O1: what lost then was the SLP vectoriser (v_pk_* pairs, long live ranges, spills --
                 // still true: plain -O3 is 0.362 / 0.361 / 1.27 on the first three), not the rest of -O2/-O3.
                 opt_level(t.quick),
                 "-fno-slp-vectorize",
                 "-std=c++20",
                 t.fast ? "-ffp-contract=fast" : "-ffp-contract=off",  // exact mode: FMAs only where device/ptl_glsl.h spells them
                 t.fast ? "-fno-hip-fp32-correctly-rounded-divide-sqrt" : "-fhip-fp32-correctly-rounded-divide-sqrt",
                 "-fno-gpu-approx-transcendentals" /* no-op on older clang, harmless */
                 // LLVM's default ("greedy") VGPR allocator MISCOMPILES divergent control flow now and then on this
                 // toolchain (ROCm 7.2): a value that is live across an exec-masked inner block gets its registers
                 // handed to temporaries of that block, so the lanes that skip the block's redefinition read garbage.
                 // Found by the GLSL fuzzer on gfx950 (tests/test_gpu_parity.py::test_greedy_regalloc_miscompile_stays_fixed:
                 // seed 105219, three pixels, reproduced down to a 3-branch kernel; host build and oracle agree with each
                 // other, every -O level, scheduler and machine-pass switch keeps the fault, `-vgpr-regalloc=basic` and
                 // `=fast` remove it).  The basic allocator does no live-range splitting; it costs 0-3 % of kernel time
                 // (profiles/r01/variants15_regalloc.jsonl), same frames.  PTL_VGPR_REGALLOC=default leaves the choice to the toolchain again.
                 };
    {
        const char* ra = std::getenv("PTL_VGPR_REGALLOC");  // "default": say nothing, i.e. the toolchain's own choice (the faulty one)
        if (!ra || std::string(ra) != "default") {
            o.push_back("-mllvm");
            o.push_back(std::string("-vgpr-regalloc=") + (ra ? ra : "basic"));
        }
    }
    {
        // LLVM's module inliner instead of its bottom-up (call-graph SCC) one, for the kernels that need it.  Every function of the generated
        // kernel is force-inlined into ONE body, eight call levels deep (kernel -> shade_pixel -> get_color -> get_color2 -> ray_tracing ->
        // trace_segment -> snippets -> library); the bottom-up pipeline re-runs its whole function simplification on that body at each level
        // on the way up (opt --time-trace of the headline: 0.25 s per level of a 5 s build).  The module inliner inlines first and simplifies
        // once: -28 ... -43 % hiprtc time where an intersection-material snippet has a force-unrolled loop (portal_in_portal with its Ints
        // baked: 10 nested portal copies per trip; codegen.cpp sets PTL_JIT_MODULE_INLINER), the same kernel time there.  Elsewhere it saves
        // 0-25 % of a 1-2 s build for a kernel that is 1.5-3 % slower (monoportal, triple_portal: profiles/r04/variants_module_inliner.jsonl)
        // or, with ~10 more VGPRs, a wave per SIMD poorer (portal_in_portal's un-baked builds with the slices entry: 120 -> 139 registers), so
        // those keep the toolchain's default.  Same source, same arithmetic, other instruction schedule: bit-identical frames.
        // PTL_MODULE_INLINER=0 / 1 forces the choice.
        const char* mi = std::getenv("PTL_MODULE_INLINER");
        if (mi ? (mi[0] != '0') : t.module_inliner) {
            o.push_back("-mllvm");
            o.push_back("-enable-module-inliner");
        }
    }
    if (t.fast && !std::getenv("PTL_FAST_KEEP_ZEROS")) {
        // Tolerance mode only: a product with a literal zero is zero.  With the scene state baked in, the portal matrices of most scenes are
        // translations and axis rotations -- 41 % of the multiplications in the headline snippet's loop have a literal +-0 operand, and
        // IEEE keeps every one of them alive (0 * x is -0, or NaN for an infinite x).  What this gives up beyond the rest of the mode:
        // the sign of exact zeros and NaN propagation through such products.
        o.push_back("-fno-signed-zeros");
        o.push_back("-fno-honor-nans");
    }
    if (const char* extra = std::getenv("PTL_HIPRTC_FLAGS")) {
        std::string e = extra;
        size_t pos = 0;
        while (pos < e.size()) {
            size_t sp = e.find(' ', pos);
            if (sp == std::string::npos) sp = e.size();
            if (sp > pos) o.push_back(e.substr(pos, sp - pos));
            pos = sp + 1;
        }
    }
    for (int k = 0; k < rq.n_defines; ++k) o.push_back(std::string("-D") + rq.defines[k]);
    return o;
}

// The code-object cache: same source + options -> same gfx950 binary.  "" when there is no cache directory.
std::string cache_path(const char* source, const Options& opts) {
    const char* cdir = std::getenv("PTL_CACHE_DIR");
    if (!cdir || !*cdir) return "";
    unsigned long long h = fnv1a(source);
    for (auto& o : opts) h = fnv1a(o, h);
    h = fnv1a("jit policy 6: occupancy retries end with an -O1 attempt", h);  // (what occupancy_ladder does to options on its own is part of the key)
    // ... produced by THIS toolchain: the cache travels between machines (build container -> GPU box), and the options above exist to
    // dodge a fault of one particular compiler.  hiprtc's version and the path it was loaded from go into the key.
    std::string err;
    if (const hip::Rtc* rc = hip::rtc(&err)) h = fnv1a("hiprtc " + rc->real_path, h);  // ".../libhiprtc.so.7.2.70200"
    char name[64];
    std::snprintf(name, sizeof name, "/ptl_%016llx.hsaco", h);
    return std::string(cdir) + name;
}

std::vector<char> cache_load(const std::string& path) {
    std::vector<char> code;
    std::ifstream f(path, std::ios::binary);
    if (f) code.assign(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
    if (code.size() < 64 || std::memcmp(code.data(), "\x7f" "ELF", 4) != 0) code.clear();  // truncated or foreign file: compile again
    return code;
}

void cache_store(const std::string& path, const std::vector<char>& code) {
    ::mkdir(path.substr(0, path.rfind('/')).c_str(), 0755);
    // one temp file per COMPILE, not per process: background re-JIT workers and the ranks of a frame group compile the same source on
    // several threads of one process, and a shared temp path would let one of them rename a file another is still writing
    static std::atomic<unsigned long> compile_serial{0};
    const std::string tmp = path + ".tmp" + std::to_string((long)getpid()) + "." + std::to_string(compile_serial.fetch_add(1));
    std::ofstream f(tmp, std::ios::binary);
    f.write(code.data(), (std::streamsize)code.size());
    f.close();
    if (f) std::rename(tmp.c_str(), path.c_str());
}

// One hiprtc run.  `report`: errors go to ptl_last_error and the compiler's log to the caller's buffer.
int run_hiprtc(const hip::Rtc* rc, const CompileRequest& rq, const Options& options, std::vector<char>& code, bool report) {
    hip::hiprtcProgram prog = nullptr;
    int r = rc->hiprtcCreateProgram(&prog, rq.source, "portal_scene.hip", 0, nullptr, nullptr);
    if (r != 0) {
        if (report) set_last_error(std::string("hiprtcCreateProgram: ") + rc->hiprtcGetErrorString(r));
        return PTL_ERR_COMPILE;
    }
    std::vector<const char*> copts;
    for (auto& o : options) copts.push_back(o.c_str());
    r = rc->hiprtcCompileProgram(prog, (int)copts.size(), copts.data());
    size_t log_size = 0;
    rc->hiprtcGetProgramLogSize(prog, &log_size);
    if (log_size > 1 && report) {
        std::vector<char> buf(log_size + 1, 0);
        rc->hiprtcGetProgramLog(prog, buf.data());
        if (rq.log && rq.log_cap) {
            std::strncpy(rq.log, buf.data(), rq.log_cap - 1);
            rq.log[rq.log_cap - 1] = '\0';
        }
        if (r != 0) set_last_error(std::string("hiprtc: ") + buf.data());
    }
    if (r != 0) {
        if (log_size <= 1 && report) set_last_error(std::string("hiprtcCompileProgram: ") + rc->hiprtcGetErrorString(r));
        rc->hiprtcDestroyProgram(&prog);
        return PTL_ERR_COMPILE;
    }
    size_t code_size = 0;
    rc->hiprtcGetCodeSize(prog, &code_size);
    code.resize(code_size);
    rc->hiprtcGetCode(prog, code.data());
    rc->hiprtcDestroyProgram(&prog);
    return PTL_OK;
}

// ---- the occupancy ladder ------------------------------------------------------------------------------------------------------------
// 128 VGPRs is where the fourth wave per SIMD goes.  A kernel that lands a few registers above it without having been told an occupancy
// is compiled again, rung by rung, until a build fits four waves (same source, same arithmetic, same frames): one to three more hiprtc
// runs for the rare kernel in that band, once -- the code object is cached under the key of the options the caller asked for.
// A rung gives the options of its attempt, or none where it does not apply.

// No PTL_WAVES_PER_EU: the module inliner's builds of portal_in_portal with the Panini switch and the slices entry, 130 VGPRs, 0.262 ->
// 0.314 ms per frame.  Once more with __launch_bounds__(256, 4), kept if the allocator got there without spilling.
Options under_the_cap(Options o) { return o.push_back("-DPTL_WAVES_PER_EU=4"), o; }

// ... and if the cap only produces spills while the build came from the module inliner -- whose schedule needs ~10 registers more than the
// bottom-up pipeline's (portal_in_portal_plus_ultra with its Ints baked: 139 against 128) -- the toolchain's own pipeline gets a try under
// the same cap.
Options bottom_up_under_the_cap(Options o) {
    const size_t before = o.size();
    for (size_t i = 0; i + 1 < o.size();)
        if (o[i] == "-mllvm" && o[i + 1] == "-enable-module-inliner") o.erase(o.begin() + i, o.begin() + i + 2);
        else ++i;
    return o.size() < before ? under_the_cap(o) : Options{};
}

// Round 6: ... and when no cap gets there without spilling, the -O1 pipeline gets a try without one.  What pushes a kernel into this band
// is -O3's appetite (hoisting and unrolling across the scene's loops): the un-specialised headline kernel is 139 VGPRs and three waves
// per SIMD at -O3, 128 + 8 bytes of scratch under the cap, and 117 VGPRs without a spill at -O1 -- 0.825 / 0.705 / 0.703 ms
// (profiles/r06/unspec_anatomy.jsonl): "-O1 beats -O3 on this kernel" (VERDICT r5 #5b) is an occupancy effect, and this is the rule that
// follows from it.  Not for a quick build, which is at -O1 already.
Options at_o1_without_a_cap(Options o) {
    bool lowered = false;
    for (auto& s : o) {
        if (s == "-O1") return {};
        if (s == "-O3") s = "-O1", lowered = true;
    }
    return lowered ? o : Options{};
}

struct Rung {
    Options (*attempt)(Options);
    bool check_vgprs;  // a rung that changes the pipeline has to land at 128 registers; the plain cap's build does if it does not spill
};
const Rung kLadder[] = {{under_the_cap, false}, {bottom_up_under_the_cap, true}, {at_o1_without_a_cap, true}};

int render_note(const std::vector<char>& code, const char* key) { return code_object_note_max(code, key, "ptl_render"); }  // the render entries only

// Does `candidate` fit four waves per SIMD no worse than the first build: no spills, no more scratch.
bool fits_four_waves(const std::vector<char>& candidate, const std::vector<char>& first, bool check_vgprs) {
    return (!check_vgprs || render_note(candidate, ".vgpr_count") <= 128) && render_note(candidate, ".vgpr_spill_count") == 0 &&
           render_note(candidate, ".private_segment_fixed_size") <= render_note(first, ".private_segment_fixed_size");
}

// `code`: the first build, made with `opts`; replaced by the first rung's build that fits.  Only the first build reports errors.
void occupancy_ladder(const hip::Rtc* rc, const CompileRequest& rq, const Options& opts, bool teleport_only, std::vector<char>& code) {
    bool hinted = false;
    for (auto& o : opts) hinted = hinted || o.find("PTL_WAVES_PER_EU") != std::string::npos;  // (a define of the caller's, or PTL_HIPRTC_FLAGS of an experiment)
    const int vgprs = render_note(code, ".vgpr_count");
    if (hinted || teleport_only || vgprs <= 128 || vgprs > 168 || std::getenv("PTL_NO_OCCUPANCY_RETRY")) return;
    for (const Rung& rung : kLadder) {
        const Options o = rung.attempt(opts);
        std::vector<char> candidate;
        if (!o.empty() && run_hiprtc(rc, rq, o, candidate, false) == PTL_OK && fits_four_waves(candidate, code, rung.check_vgprs)) {
            code.swap(candidate);
            return;
        }
    }
}

// The request's code object: the cache's when `read_cache`, else hiprtc's, which goes into the cache.  `read_from`: the cache file the object
// came from, "" otherwise.
int obtain_code(const CompileRequest& rq, const BuildTraits& traits, bool read_cache, std::vector<char>& code, std::string& read_from) {
    read_from.clear();
    const Options opts = compile_options(rq, traits);
    const std::string path = cache_path(rq.source, opts);
    code.clear();
    if (read_cache && !path.empty()) code = cache_load(path);
    if (!code.empty()) {
        read_from = path;
        return PTL_OK;
    }
    std::string err;
    const hip::Rtc* rc = hip::rtc(&err);
    if (!rc) {
        set_last_error(err);
        return PTL_ERR_COMPILE;
    }
    if (int r = run_hiprtc(rc, rq, opts, code, true); r != PTL_OK) return r;
    occupancy_ladder(rc, rq, opts, traits.teleport_only, code);
    if (!path.empty()) cache_store(path, code);
    return PTL_OK;
}

// Loads k->code on the current device and binds what the host side uses of it: entries, uniform block, events.  `Discover`: the plain render
// entry, else the slices entry (the `slices` sections of device/ptl_entry.h).  A code object the runtime refuses leaves k->module null.
enum class RenderEntry { None, Plain, Sliced, Discover };
int bind_module(ptl_kernel* k, const hip::Runtime* rt, RenderEntry entry, size_t declared_block_size) {
    if (!hip_ok(rt, rt->hipModuleLoadData(&k->module, k->code.data()), "hipModuleLoadData")) return k->module = nullptr, PTL_ERR_HIP;
    if (entry == RenderEntry::Plain || entry == RenderEntry::Discover) {
        const int e = rt->hipModuleGetFunction(&k->fn, k->module, "ptl_render_kernel");
        if (e != 0 && entry == RenderEntry::Discover) {
            rt->hipGetLastError();
            entry = RenderEntry::Sliced;
        } else if (!hip_ok(rt, e, "hipModuleGetFunction(ptl_render_kernel)"))
            return PTL_ERR_HIP;
    }
    if (entry == RenderEntry::Sliced) {
        if (!hip_ok(rt, rt->hipModuleGetFunction(&k->fn, k->module, "ptl_render_slices_kernel"), "hipModuleGetFunction(ptl_render_kernel / ptl_render_slices_kernel)"))
            return PTL_ERR_HIP;
        if (!hip_ok(rt, rt->hipModuleGetFunction(&k->derive_slices_fn, k->module, "ptl_derive_slices_kernel"), "hipModuleGetFunction(ptl_derive_slices_kernel)"))
            return PTL_ERR_HIP;
        k->sliced = true;
    }
    for (auto [fn, name] : {std::pair{&k->teleport_fn, "ptl_teleport_kernel"}, std::pair{&k->derive_fn, "ptl_derive_kernel"}, std::pair{&k->refine_fn, "ptl_render_refine_kernel"},
                           std::pair{&k->refine_slices_fn, "ptl_render_refine_slices_kernel"}})
        if (rt->hipModuleGetFunction(fn, k->module, name) != 0) {
            *fn = nullptr;          // hand-written layer-1 kernels need not have the other entry points
            rt->hipGetLastError();  // ... and the expected hipErrorNotFound must not stay behind as the thread's sticky
                                    // error: the next HIP user in the process (PyTorch) would report it as its own
        }
    if (!hip_ok(rt, rt->hipModuleGetGlobal(&k->dev_block, &k->dev_block_size, k->module, "_ZN4glsl5ptl_uE"), "hipModuleGetGlobal(ptl_u)"))
        return PTL_ERR_HIP;
    if (k->dev_block_size < declared_block_size) {
        set_last_error("uniform block in the code object is smaller than the declared layout");
        return PTL_ERR_INVALID;
    }
    rt->hipEventCreate(&k->ev0);
    rt->hipEventCreate(&k->ev1);
    rt->hipEventCreateWithFlags(&k->ev_done, hip::kEventDisableTiming);
    if (const char* e = std::getenv("PTL_BLOCK_WAVES")) k->block_waves = (e[0] == '1' || e[0] == '2') ? (unsigned)(e[0] - '0') : 4u;
    return PTL_OK;
}

// What both public compile entries do.  `prebuilt`: this code object instead of cache / hiprtc.  `read_cache`: may a cached one be used.
int compile_kernel(const CompileRequest& rq, const std::vector<char>* prebuilt, bool read_cache, ptl_kernel** out) {
    if (rq.log && rq.log_cap) rq.log[0] = '\0';
    if (!rq.source || !out) return PTL_ERR_INVALID;
    *out = nullptr;
    KernelPtr k(new ptl_kernel());
    k->device = rq.device;
    for (int i = 0; i < rq.n_uniforms; ++i) {
        const ptl_uniform_desc& u = rq.uniforms[i];
        k->slots[u.name] = {u.type, u.offset};
        if (u.offset + type_size(u.type) > rq.block_size) {
            set_last_error(std::string("uniform `") + u.name + "` lies outside the block");
            return PTL_ERR_INVALID;
        }
    }
    k->shadow.assign(rq.block_size, 0);
    const BuildTraits traits = read_traits(rq);
    k->affine_rays = traits.affine_rays;
    k->split = traits.split;
    k->has_refine = !traits.teleport_only && std::strstr(rq.source, "ptl_render_refine_kernel(") != nullptr;
    k->has_refine_slices = !traits.teleport_only && std::strstr(rq.source, "ptl_render_refine_slices_kernel(") != nullptr;
    k->has_passes = !traits.teleport_only && std::strstr(rq.source, "#define PTL_PASSES 1\n") != nullptr;
    if (k->split) {
        k->source = rq.source;
        k->defines.assign(rq.defines, rq.defines + rq.n_defines);
    }
    std::string read_from;
    if (prebuilt) k->code = *prebuilt;  // compiled elsewhere from this very source: nothing to look up, nothing to build or store
    else if (int rc = obtain_code(rq, traits, read_cache, k->code, read_from); rc != PTL_OK) return rc;
    if (rq.device < 0) {  // compile-only handle
        *out = k.release();
        return PTL_OK;
    }
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    if (!hip_ok(rt, rt->hipSetDevice(rq.device), "hipSetDevice")) return PTL_ERR_HIP;
    const RenderEntry entry = traits.teleport_only ? RenderEntry::None : RenderEntry::Discover;  // (the teleport half of a split build: no render entry by construction)
    int rc = bind_module(k.get(), rt, entry, rq.block_size);
    if (rc != PTL_OK && !k->module && !read_from.empty()) {
        // a cached code object this runtime refuses (other GPU, damaged file): drop it and build from source ONCE.  The retry does
        // not read the cache again -- the file may be undeletable (a read-only or shared cache directory travels from the build
        // container to the GPU box), and re-reading it would refuse without end.
        std::remove(read_from.c_str());
        if (int rc2 = obtain_code(rq, traits, false, k->code, read_from); rc2 != PTL_OK) return rc2;
        rc = bind_module(k.get(), rt, entry, rq.block_size);
    }
    if (rc != PTL_OK) return rc;
    *out = k.release();
    return PTL_OK;
}

}  // namespace

extern "C" const char* ptl_last_error(void) { return g_last_error.c_str(); }

extern "C" const char* ptl_version(void) {
    static std::string v;
    std::string e1, e2;
    const hip::Runtime* rt = hip::runtime(&e1);
    const hip::Rtc* rc = hip::rtc(&e2);
    std::string toolchain = "?";  // "7.2.70200" out of ".../libhiprtc.so.7.2.70200"
    if (rc) {
        size_t so = rc->real_path.rfind(".so.");
        if (so != std::string::npos) toolchain = rc->real_path.substr(so + 4);
    }
    v = std::string("portal_amd 0.2; hip=") + (rt ? rt->path : "<none>") + "; hiprtc=" + (rc ? rc->path : "<none>") + "; hiprtc_version=" + toolchain;
    return v.c_str();
}

extern "C" int ptl_device_count(void) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return 0;
    int n = 0;
    if (rt->hipGetDeviceCount(&n) != 0) return 0;
    return n;
}

extern "C" int ptl_kernel_compile(int device, const char* hip_source, const ptl_uniform_desc* uniforms, int n_uniforms,
                                  size_t uniform_block_size, const char* const* defines, int n_defines, ptl_kernel** out, char* log,
                                  size_t log_cap) {
    return compile_kernel({device, hip_source, uniforms, n_uniforms, uniform_block_size, defines, n_defines, log, log_cap}, nullptr, true, out);
}

// Layer-1 internal (renderer_builds.cpp's background re-JIT): load a code object that another thread compiled from exactly `hip_source` with
// exactly these defines (a compile-only handle, device = -1) instead of compiling again.
extern "C" int ptl_kernel_compile_prebuilt(int device, const char* hip_source, const ptl_uniform_desc* uniforms, int n_uniforms, size_t uniform_block_size,
                                           const char* const* defines, int n_defines, const void* code, size_t code_size, ptl_kernel** out, char* log,
                                           size_t log_cap) {
    if (!code || code_size < 64) return PTL_ERR_INVALID;
    const std::vector<char> copy(static_cast<const char*>(code), static_cast<const char*>(code) + code_size);
    return compile_kernel({device, hip_source, uniforms, n_uniforms, uniform_block_size, defines, n_defines, log, log_cap}, &copy, false, out);
}

// A second instance of a compiled kernel on the same device: the same code object loaded once more, hence a uniform block (and a
// prologue) of its OWN -- two instances can be in flight on two streams with two different sets of uniform values, which one module
// cannot (its block is one global).  Nothing is compiled.  The clone shares the original's textures: sampler records travel with
// ptl_kernel_copy_uniforms and the texel buffers stay owned by the original, which must outlive its clones.
extern "C" int ptl_kernel_clone(ptl_kernel* src, ptl_kernel** out) {
    if (!src || !out) return PTL_ERR_INVALID;
    if (src->device < 0 || !src->fn) return PTL_ERR_NO_DEVICE;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    KernelPtr k(new ptl_kernel());
    k->device = src->device;
    k->code = src->code;
    k->slots = src->slots;
    k->shadow = src->shadow;
    k->block_waves = src->block_waves;
    k->split = src->split;
    k->has_refine = src->has_refine;
    k->has_refine_slices = src->has_refine_slices;
    k->has_passes = src->has_passes;
    k->source = src->source;
    k->defines = src->defines;
    // (affine_rays is NOT inherited: a clone accepts matrices through ptl_kernel_set_uniform that its original refuses)
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    if (int rc = bind_module(k.get(), rt, src->sliced ? RenderEntry::Sliced : RenderEntry::Plain, k->shadow.size()); rc != PTL_OK) return rc;
    *out = k.release();
    return PTL_OK;
}

// The host copy of `src`'s uniform block -- every value set so far, sampler records included -- becomes `dst`'s; uploaded behind dst's next
// launch like any other change.  Both must come from the same source (ptl_kernel_clone).
extern "C" int ptl_kernel_copy_uniforms(ptl_kernel* dst, const ptl_kernel* src) {
    if (!dst || !src || dst->shadow.size() != src->shadow.size()) return PTL_ERR_INVALID;
    if (std::memcmp(dst->shadow.data(), src->shadow.data(), src->shadow.size()) != 0) {
        dst->shadow = src->shadow;
        dst->dirty = true;
        dst->slice0_dirty = true;
    }
    return PTL_OK;
}

extern "C" int ptl_kernel_code_object(ptl_kernel* k, const void** data, size_t* size) {
    if (!k) return PTL_ERR_INVALID;
    if (data) *data = k->code.data();
    if (size) *size = k->code.size();
    return PTL_OK;
}

// The kernel metadata of a code object (the one ptl_kernel_code_object hands out, or a file of the cache): the largest value of `key`
// (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".sgpr_count" ...) over the kernels whose name starts with
// `kernel_prefix` (NULL / "": all kernels); -1 when the key does not occur.  What the JIT's occupancy retry decides on; no device needed.
extern "C" int ptl_code_object_note(const void* code, size_t size, const char* key, const char* kernel_prefix) {
    if (!code || !key) return -1;
    // (a value is attributed to the kernel whose `.name` entry was seen last, which relies on the metadata map's alphabetical key order: right
    // for keys that sort AFTER ".name" only -- the documented ones all do; with a kernel prefix any other key is refused rather than mis-attributed)
    if (kernel_prefix && kernel_prefix[0] && std::strcmp(key, ".name") <= 0) return -1;
    std::vector<char> bytes(static_cast<const char*>(code), static_cast<const char*>(code) + size);
    return code_object_note_max(bytes, key, kernel_prefix);
}

extern "C" int ptl_kernel_resources(ptl_kernel* k, int* registers, int* scratch_bytes, int* lds_bytes) {
    if (!k) return PTL_ERR_INVALID;
    if (k->device < 0 && !k->code.empty()) {  // a compile-only handle: what the code object's metadata says about its render entries
        if (registers) *registers = render_note(k->code, ".vgpr_count");
        if (scratch_bytes) *scratch_bytes = render_note(k->code, ".private_segment_fixed_size");
        if (lds_bytes) *lds_bytes = render_note(k->code, ".group_segment_fixed_size");
        return PTL_OK;
    }
    if (k->device < 0 || !k->fn) return PTL_ERR_NO_DEVICE;
    const hip::Runtime* rt = hip::runtime(nullptr);
    int v = 0;
    if (registers) *registers = rt->hipFuncGetAttribute(&v, hip::kFuncAttrNumRegs, k->fn) == 0 ? v : -1;
    if (scratch_bytes) *scratch_bytes = rt->hipFuncGetAttribute(&v, hip::kFuncAttrLocalSizeBytes, k->fn) == 0 ? v : -1;
    if (lds_bytes) *lds_bytes = rt->hipFuncGetAttribute(&v, hip::kFuncAttrSharedSizeBytes, k->fn) == 0 ? v : -1;
    return PTL_OK;
}

// What ptl_kernel_set_uniform and ptl_kernel_set_staged_uniform check alike; PTL_OK: `*offset` is where the value goes in a block.
static int settable_uniform(ptl_kernel* k, const char* name, ptl_type type, const void* value, size_t* offset) {
    auto it = k->slots.find(name);
    if (it == k->slots.end()) return PTL_UNKNOWN_UNIFORM;
    if (it->second.type != type || type == PTL_SAMPLER) return PTL_ERR_TYPE;
    if (k->affine_rays && type == PTL_MAT4) {
        // a layer-1 caller owns `_camera` and every run-time `X_mat`; a kernel with affine rays is only valid for matrices that map
        // w = 1 to 1 and w = 0 to 0 (or are NaN throughout: a switched-off object).  The layer-2 renderer rebuilds BEFORE it uploads such a matrix
        // (renderer_camera.cpp `camera_is_affine`, renderer_builds.cpp `zero_patterns_broken`); a direct caller gets the refusal instead of silently wrong frames.
        const std::string nm = name;
        auto tail = [&](const char* e) { const size_t m = std::strlen(e); return nm.size() >= m && nm.compare(nm.size() - m, m, e) == 0; };
        if ((nm == "_camera" || tail("_mat") || tail("_mat_inv") || tail("_mat_teleport")) && !matrix_keeps_rays_affine(static_cast<const float*>(value))) {
            set_last_error("ptl_kernel_set_uniform: `" + nm + "` is not an affine matrix (bottom row 0 0 0 1) but this kernel was generated with PTL_AFFINE_RAYS; "
                           "regenerate with flag bit23 (NO AFFINE RAYS)");
            return PTL_ERR_INVALID;
        }
    }
    *offset = it->second.offset;
    return PTL_OK;
}

extern "C" int ptl_kernel_set_uniform(ptl_kernel* k, const char* name, ptl_type type, const void* value) {
    if (!k || !name || !value) return PTL_ERR_INVALID;
    size_t offset = 0;
    if (int rc = settable_uniform(k, name, type, value, &offset); rc != PTL_OK) return rc;
    const size_t n = type_size(type);
    if (std::memcmp(k->shadow.data() + offset, value, n) != 0) {
        std::memcpy(k->shadow.data() + offset, value, n);
        k->dirty = true;
        k->slice0_dirty = true;
    }
    return PTL_OK;
}

static void free_retired_textures(ptl_kernel* k, const hip::Runtime* rt) {
    for (void* t : k->retired_textures) rt->hipFree(t);  // waits for the device: the launch that read them has finished
    k->retired_textures.clear();
}

// While held (counted), re-binding a sampler keeps the previous texel buffer alive: the caller holds copies of the uniform block
// (ptl_kernel_snapshot_uniforms) that it will stage later.  Releasing the last hold frees what was retired meanwhile.
extern "C" int ptl_kernel_hold_textures(ptl_kernel* k, int hold) {
    if (!k) return PTL_ERR_INVALID;
    if (hold) {
        ++k->texture_holds;
        return PTL_OK;
    }
    if (k->texture_holds > 0) --k->texture_holds;
    if (k->texture_holds == 0 && !k->staged_since_launch && !k->retired_textures.empty() && k->device >= 0) {
        const hip::Runtime* rt = hip::runtime(nullptr);
        if (rt && rt->hipSetDevice(k->device) == 0) free_retired_textures(k, rt);
    }
    return PTL_OK;
}

extern "C" int ptl_kernel_set_texture(ptl_kernel* k, const char* sampler, const uint8_t* rgba8, int width, int height) {
    if (!k || !sampler || !rgba8 || width <= 0 || height <= 0) return PTL_ERR_INVALID;
    auto it = k->slots.find(sampler);
    if (it == k->slots.end()) return PTL_UNKNOWN_UNIFORM;
    if (it->second.type != PTL_SAMPLER) return PTL_ERR_TYPE;
    if (k->device < 0) return PTL_ERR_NO_DEVICE;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    void*& dev = k->textures[sampler];
    const bool held = k->staged_since_launch || k->texture_holds > 0;
    if (dev) {
        if (held)
            k->retired_textures.push_back(dev);  // a staged slice / a caller's snapshot may name it: it lives until the launch that reads it is behind us
        else
            rt->hipFree(dev);  // (hipFree waits for the device: a launch still reading it has finished)
        dev = nullptr;
    }
    if (!held) free_retired_textures(k, rt);
    size_t bytes = (size_t)width * height * 4;
    if (!hip_ok(rt, rt->hipMalloc(&dev, bytes), "hipMalloc(texture)")) return PTL_ERR_HIP;
    if (!hip_ok(rt, rt->hipMemcpy(dev, rgba8, bytes, hip::kMemcpyHostToDevice), "hipMemcpy(texture)")) return PTL_ERR_HIP;
    struct {
        void* texels;
        int w, h;
    } s{dev, width, height};
    static_assert(sizeof s == 16, "sampler2D layout");
    std::memcpy(k->shadow.data() + it->second.offset, &s, sizeof s);
    k->dirty = true;
    k->slice0_dirty = true;
    return PTL_OK;
}

extern "C" int ptl_frame_shard_rows(const ptl_frame* f) {
    if (!f || f->width <= 0 || f->height <= 0 || f->rb_stride <= 0 || f->rb_phase < 0 || f->rb_phase >= f->rb_stride) return -1;
    int blocks = (f->height + 7) / 8;
    int rows = 0;
    for (int b = f->rb_phase; b < blocks; b += f->rb_stride) rows += (b * 8 + 8 <= f->height) ? 8 : f->height - b * 8;
    return rows;
}

static int shard_blocks(const ptl_frame* f) {
    int blocks = (f->height + 7) / 8;
    return blocks > f->rb_phase ? (blocks - f->rb_phase + f->rb_stride - 1) / f->rb_stride : 0;
}

// Stream-ordered upload of the host's copy of the uniform block (one copy, a few KB) followed by the module's prologue
// kernel, which fills the derived uniforms behind it.
static int upload_uniforms(ptl_kernel* k, const hip::Runtime* rt, void* stream) {
    if (!k->dirty) return PTL_OK;
    if (!hip_ok(rt, rt->hipMemcpyAsync(k->dev_block, k->shadow.data(), k->shadow.size(), hip::kMemcpyHostToDevice, stream), "hipMemcpyAsync(uniform block)"))
        return PTL_ERR_HIP;
    // the shadow buffer is pageable host memory: the async copy has staged it before returning
    if (k->derive_fn) {
        void* block = k->dev_block;
        void* args[] = {&block};
        if (!hip_ok(rt, rt->hipModuleLaunchKernel(k->derive_fn, 1, 1, 1, 64, 1, 1, 0, stream, args, nullptr), "hipModuleLaunchKernel(ptl_derive_kernel)"))
            return PTL_ERR_HIP;
    }
    k->dirty = false;
    return PTL_OK;
}

// ---- modules with the slices entry -------------------------------------------------------------------------------------------
// Stream-ordered upload of `n` staged blocks (or, for a single draw, of the host copy as slice 0) into the module's buffer of blocks,
// followed by the prologue of every slice.
static int upload_slices(ptl_kernel* k, const hip::Runtime* rt, void* stream, int n, bool single) {
    const size_t stride = k->dev_block_size;
    if (!k->dev_slices && !hip_ok(rt, rt->hipMalloc(&k->dev_slices, stride * kMaxSlices), "hipMalloc(uniform block slices)")) return PTL_ERR_HIP;
    if (single) {
        if (!k->slice0_dirty) return PTL_OK;
        if (!hip_ok(rt, rt->hipMemcpyAsync(k->dev_slices, k->shadow.data(), k->shadow.size(), hip::kMemcpyHostToDevice, stream), "hipMemcpyAsync(uniform block -> slice 0)"))
            return PTL_ERR_HIP;
    } else {
        if (!hip_ok(rt, rt->hipMemcpyAsync(k->dev_slices, k->staged.data(), stride * (size_t)n, hip::kMemcpyHostToDevice, stream), "hipMemcpyAsync(uniform block slices)"))
            return PTL_ERR_HIP;
    }
    void* blocks = k->dev_slices;
    void* args[] = {&blocks};
    if (!hip_ok(rt, rt->hipModuleLaunchKernel(k->derive_slices_fn, (unsigned)n, 1, 1, 64, 1, 1, 0, stream, args, nullptr), "hipModuleLaunchKernel(ptl_derive_slices_kernel)"))
        return PTL_ERR_HIP;
    k->slice0_dirty = !single;  // (a batch leaves its own slice 0 behind)
    return PTL_OK;
}

static const char* const kSlicesLaunch = "hipModuleLaunchKernel(ptl_render_slices_kernel)";

// One launch of an entry of the module, timed between the kernel's two events when `elapsed_ms` is given (the call then waits for it), and
// marked as the kernel's most recent launch.  `label`: what a refused launch is reported as.
static int timed_launch(ptl_kernel* k, const hip::Runtime* rt, hip::hipFunction_t fn, unsigned gx, unsigned gy, unsigned gz, unsigned threads, void** args, void* stream,
                        float* elapsed_ms, const char* label) {
    if (elapsed_ms) rt->hipEventRecord(k->ev0, stream);
    if (!hip_ok(rt, rt->hipModuleLaunchKernel(fn, gx, gy, gz, threads, 1, 1, 0, stream, args, nullptr), label)) return PTL_ERR_HIP;
    k->last_stream = stream;
    k->launched = true;
    if (k->ev_done) rt->hipEventRecord(k->ev_done, stream);
    if (elapsed_ms) {
        rt->hipEventRecord(k->ev1, stream);
        if (!hip_ok(rt, rt->hipEventSynchronize(k->ev1), "hipEventSynchronize")) return PTL_ERR_HIP;
        rt->hipEventElapsedTime(elapsed_ms, k->ev0, k->ev1);
    }
    return PTL_OK;
}

// The one render launch.  A module with the slices entry traces slices 0 .. n-1 of its buffer of blocks, slice z into out_rgba8 + z * slice_pixels
// pixels; the plain entry (n = 1) reads the module's own block.  `label`: what a refused launch is reported as.
// `out_passes`: the pass records of a PTL_FLAG_PASSES module (null: none wanted); every other module's entry ends before that argument.
static int launch_render(ptl_kernel* k, const hip::Runtime* rt, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, unsigned long long slice_pixels,
                         void* segments, void* stream, float* elapsed_ms, const char* label) {
    int nby = shard_blocks(frame);
    if (nby == 0) {
        if (elapsed_ms) *elapsed_ms = 0.0f;
        return PTL_OK;
    }
    int width = frame->width, height = frame->height, phase = frame->rb_phase, stride = frame->rb_stride;
    int in_place = frame->in_place ? 1 : 0;
    void* blocks = k->dev_slices;
    void* args[] = {&blocks, &slice_pixels, &out_rgba8, &out_rgba32f, &width, &height, &phase, &stride, &segments, &in_place, &out_passes};  // the plain entry starts at out_rgba8
    // 256 threads = four 8x8 tiles side by side.  PTL_BLOCK_WAVES=1|2 (experiment, tools/variants.py) launches narrower workgroups.
    const unsigned waves = k->block_waves;
    unsigned gx = (unsigned)((width + 8 * waves - 1) / (8 * waves)), gy = (unsigned)nby;
    const int rc = timed_launch(k, rt, k->fn, gx, gy, (unsigned)n, 64 * waves, k->sliced ? args : args + 2, stream, elapsed_ms, label);
    if (rc == PTL_OK && k->sliced) k->staged_since_launch = false;  // what was staged is launched: retired texel buffers go with the next re-bind (hipFree waits for this launch)
    return rc;
}

extern "C" int ptl_kernel_max_slices(ptl_kernel* k) { return (k && k->sliced) ? kMaxSlices : 0; }

// The current uniform values (everything set with ptl_kernel_set_uniform / _set_texture so far) become slice `index` of the next batch.
extern "C" int ptl_kernel_stage_slice(ptl_kernel* k, int index) {
    if (!k) return PTL_ERR_INVALID;
    return ptl_kernel_stage_slice_from(k, index, k->shadow.data(), k->shadow.size());
}

// ... or a block saved earlier with ptl_kernel_snapshot_uniforms -- possibly from ANOTHER kernel of the same scene (every build of a scene has
// the same block layout; a renderer that had to rebuild its kernel between staging and launching re-stages its snapshots into the new one).
// Sampler records are taken from THIS kernel: they point at texel buffers each kernel owns.
extern "C" int ptl_kernel_stage_slice_from(ptl_kernel* k, int index, const void* block, size_t size) {
    if (!k || !block || index < 0 || index >= kMaxSlices) return PTL_ERR_INVALID;
    if (!k->sliced) {
        set_last_error("ptl_kernel_stage_slice: the kernel was not generated with the slices entry (PTL_FLAG_SLICES)");
        return PTL_ERR_INVALID;
    }
    if (k->device < 0) return PTL_ERR_NO_DEVICE;
    if (size != k->shadow.size()) {
        set_last_error("ptl_kernel_stage_slice_from: the block has another size than this kernel's uniform block (another scene?)");
        return PTL_ERR_INVALID;
    }
    const size_t stride = k->dev_block_size;
    if (k->staged.size() < stride * kMaxSlices) k->staged.assign(stride * kMaxSlices, 0);
    unsigned char* dst = k->staged.data() + stride * (size_t)index;
    std::memcpy(dst, block, size);
    for (auto& [name, slot] : k->slots)
        if (slot.type == PTL_SAMPLER) {
            // a record that names a texel buffer of THIS kernel (bound now, or bound when the block was taken and retired since) stays: a video
            // texture that stepped between two sub-frames is read by each slice as it was.  Anything else came from another kernel of the scene.
            void* texels = nullptr;
            std::memcpy(&texels, dst + slot.offset, sizeof texels);
            bool own = false;
            for (auto& t : k->textures) own = own || (texels && t.second == texels);
            for (void* t : k->retired_textures) own = own || (texels && t == texels);
            if (!own) std::memcpy(dst + slot.offset, k->shadow.data() + slot.offset, 16);
        }
    k->staged_since_launch = true;
    return PTL_OK;
}

extern "C" size_t ptl_kernel_uniform_block_size(ptl_kernel* k) { return k ? k->shadow.size() : 0; }
extern "C" int ptl_kernel_snapshot_uniforms(ptl_kernel* k, void* dst, size_t cap) {
    if (!k || !dst || cap < k->shadow.size()) return PTL_ERR_INVALID;
    std::memcpy(dst, k->shadow.data(), k->shadow.size());
    return PTL_OK;
}

// ONE launch for the staged slices 0 .. n-1: slice z renders `frame` with its own uniforms into out_rgba8 + z * slice_pixels pixels
// (and out_rgba32f + 4 * z * slice_pixels floats).
static int render_slices(ptl_kernel* k, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, unsigned long long slice_pixels, void* stream,
                         float* elapsed_ms) {
    if (!k || !frame || ptl_frame_shard_rows(frame) < 0 || n < 1 || n > kMaxSlices) return PTL_ERR_INVALID;
    if (!k->sliced || k->staged.empty()) {
        set_last_error("ptl_kernel_render_slices: no staged slices (PTL_FLAG_SLICES build + ptl_kernel_stage_slice)");
        return PTL_ERR_INVALID;
    }
    if (k->device < 0 || !k->fn) return PTL_ERR_NO_DEVICE;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    if (int rc = upload_slices(k, rt, stream, n, false); rc != PTL_OK) return rc;
    return launch_render(k, rt, frame, n, out_rgba8, out_rgba32f, out_passes, slice_pixels, nullptr, stream, elapsed_ms, kSlicesLaunch);
}

extern "C" int ptl_kernel_render_slices(ptl_kernel* k, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels,
                                        void* stream, float* elapsed_ms) {
    return render_slices(k, frame, n, out_rgba8, out_rgba32f, nullptr, slice_pixels, stream, elapsed_ms);
}

static int render_single(ptl_kernel* k, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* out_passes, void* segments, void* stream, float* elapsed_ms) {
    if (!k || !frame || ptl_frame_shard_rows(frame) < 0) return PTL_ERR_INVALID;
    if (k->device < 0 || !k->fn) return PTL_ERR_NO_DEVICE;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    // (a single draw of a module with the slices entry: slice 0 of its buffer, one slice)
    if (int rc = k->sliced ? upload_slices(k, rt, stream, 1, true) : upload_uniforms(k, rt, stream); rc != PTL_OK) return rc;
    return launch_render(k, rt, frame, 1, out_rgba8, out_rgba32f, out_passes, 0, segments, stream, elapsed_ms, k->sliced ? kSlicesLaunch : "hipModuleLaunchKernel");
}

extern "C" int ptl_kernel_render(ptl_kernel* k, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* segments,
                                 void* stream, float* elapsed_ms) {
    return render_single(k, frame, out_rgba8, out_rgba32f, nullptr, segments, stream, elapsed_ms);
}

// ---- trace passes: the same two launches with the records of a PTL_FLAG_PASSES module (the `passes` sections of device/ptl_entry.h) ------
extern "C" size_t ptl_pass_record_bytes(int width, int height) { return (width > 0 && height > 0) ? sizeof(ptl_pass_record) * (size_t)width * (size_t)height : 0; }

// What both refuse before any GPU call: a module without the records, a missing or misaligned buffer, one too small for what the launch stores
// (`pixels`: the last slice's offset plus the rows this shard writes -- all of the frame's when it stores in place).
static int check_passes(const char* who, const ptl_kernel* k, const ptl_frame* frame, const void* out_passes, size_t passes_bytes, unsigned long long slice_offset) {
    if (!k || !frame || ptl_frame_shard_rows(frame) < 0) return PTL_ERR_INVALID;
    if (!k->has_passes) {
        set_last_error(std::string(who) + ": the kernel was not generated with pass records (PTL_FLAG_PASSES)");
        return PTL_ERR_INVALID;
    }
    const unsigned long long rows = frame->in_place ? (unsigned long long)frame->height : (unsigned long long)ptl_frame_shard_rows(frame);
    if (!out_passes || (reinterpret_cast<uintptr_t>(out_passes) & 15u) || passes_bytes < sizeof(ptl_pass_record) * (slice_offset + rows * (unsigned long long)frame->width)) {
        set_last_error(std::string(who) + ": out_passes must be a 16-byte aligned buffer of 16 bytes per pixel the launch stores (ptl_pass_record_bytes)");
        return PTL_ERR_INVALID;
    }
    return PTL_OK;
}

extern "C" int ptl_kernel_render_passes(ptl_kernel* k, const ptl_frame* frame, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes, void* segments,
                                        void* stream, float* elapsed_ms) {
    if (int rc = check_passes("ptl_kernel_render_passes", k, frame, out_passes, passes_bytes, 0); rc != PTL_OK) return rc;
    return render_single(k, frame, out_rgba8, out_rgba32f, out_passes, segments, stream, elapsed_ms);
}

extern "C" int ptl_kernel_render_slices_passes(ptl_kernel* k, const ptl_frame* frame, int n, void* out_rgba8, void* out_rgba32f, void* out_passes, size_t passes_bytes,
                                               unsigned long long slice_pixels, void* stream, float* elapsed_ms) {
    if (n < 1 || n > kMaxSlices) return PTL_ERR_INVALID;
    if (int rc = check_passes("ptl_kernel_render_slices_passes", k, frame, out_passes, passes_bytes, (unsigned long long)(n - 1) * slice_pixels); rc != PTL_OK) return rc;
    return render_slices(k, frame, n, out_rgba8, out_rgba32f, out_passes, slice_pixels, stream, elapsed_ms);
}

// ---- the refine pass of the adaptive anti-aliasing: the list-driven entries (device/ptl_refine_common.h) -----------------------------
// A list names pixels of a whole frame, each as a 32-bit index.  `who`, `lists`: how the refusal names the caller and its argument.
static int check_listed_frame(const char* who, const char* lists, const ptl_frame* frame) {
    if (frame->rb_stride != 1 || frame->rb_phase != 0 || frame->in_place) {
        set_last_error(std::string(who) + ": " + lists + " pixels of a whole frame (rb_phase 0, rb_stride 1, not in_place)");
        return PTL_ERR_INVALID;
    }
    if ((long long)frame->width * frame->height > (1LL << 31)) return PTL_ERR_INVALID;  // an entry is a 32-bit pixel index
    return PTL_OK;
}

// The one refine launch: for every slice z < n, the counts[z] pixels of lists + z * list_stride -- both in device memory, read on the
// device -- are shaded again, each lane storing its own pixel into out_* + z * slice_pixels pixels.  `over_slices`: the entry over the
// module's buffer of blocks, whose staged slices are uploaded (with their prologue) like ptl_kernel_render_slices does; else the entry on
// the module's own block with the uniforms set now, n = 1.  A grid of fixed size (gx, 1, n): a chunk of 256 entries per workgroup and
// trip, at most 2 048 workgroups per launch (8 per CU) split evenly over the slices, which cover a frame's worth of entries in a few trips.
static int launch_refine(ptl_kernel* k, bool over_slices, const ptl_frame* frame, int n, const void* lists, unsigned long long list_stride, const void* counts,
                         void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels, void* segments, void* stream, float* elapsed_ms) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    if (int rc = over_slices ? upload_slices(k, rt, stream, n, false) : upload_uniforms(k, rt, stream); rc != PTL_OK) return rc;
    int width = frame->width, height = frame->height;
    void* blocks = k->dev_slices;
    void* own_block[] = {&lists, &counts, &out_rgba8, &out_rgba32f, &width, &height, &segments};
    void* slices[] = {&blocks, &slice_pixels, &lists, &list_stride, &counts, &out_rgba8, &out_rgba32f, &width, &height, &segments};
    const long long chunks = ((long long)width * height + 255) / 256;
    const unsigned gx = (unsigned)std::min<long long>(chunks, 2048 / n);
    return timed_launch(k, rt, over_slices ? k->refine_slices_fn : k->refine_fn, gx, 1, (unsigned)n, 256, over_slices ? slices : own_block, stream, elapsed_ms,
                        over_slices ? "hipModuleLaunchKernel(ptl_render_refine_slices_kernel)" : "hipModuleLaunchKernel(ptl_render_refine_kernel)");
}

// The refine pass of one frame: the `*count` pixels of `list`, with the uniforms set now.
extern "C" int ptl_kernel_render_refine(ptl_kernel* k, const ptl_frame* frame, const void* list, const void* count, void* out_rgba8, void* out_rgba32f,
                                        void* segments, void* stream, float* elapsed_ms) {
    if (!k || !frame || !list || !count || frame->width <= 0 || frame->height <= 0) return PTL_ERR_INVALID;
    if (int rc = check_listed_frame("ptl_kernel_render_refine", "the list names", frame); rc != PTL_OK) return rc;
    if (!k->has_refine) {
        set_last_error("ptl_kernel_render_refine: the kernel was not generated with the refine entry (PTL_FLAG_REFINE)");
        return PTL_ERR_INVALID;
    }
    if (k->device < 0 || !k->refine_fn) return PTL_ERR_NO_DEVICE;
    return launch_refine(k, false, frame, 1, list, 0, count, out_rgba8, out_rgba32f, 0, segments, stream, elapsed_ms);
}

// One uniform inside slice `index` as it is staged now (not the kernel's current values): what a caller changes between two launches over
// the same staged slices -- layer 2 sets `_aa_count` = 1 for pass 1 of an adaptive batch.  The codes of ptl_kernel_set_uniform.
extern "C" int ptl_kernel_set_staged_uniform(ptl_kernel* k, int index, const char* name, ptl_type type, const void* value) {
    if (!k || !name || !value || index < 0 || index >= kMaxSlices) return PTL_ERR_INVALID;
    size_t offset = 0;
    if (int rc = settable_uniform(k, name, type, value, &offset); rc != PTL_OK) return rc;
    if (k->staged.empty()) {
        set_last_error("ptl_kernel_set_staged_uniform: no staged slices (PTL_FLAG_SLICES build + ptl_kernel_stage_slice)");
        return PTL_ERR_INVALID;
    }
    std::memcpy(k->staged.data() + k->dev_block_size * (size_t)index + offset, value, type_size(type));
    return PTL_OK;
}

// The refine pass of an adaptive batch: for every staged slice z < n, the counts[z] pixels of lists + z * list_stride with that slice's
// uniforms into out_* + z * slice_pixels pixels.
extern "C" int ptl_kernel_render_slices_refine(ptl_kernel* k, const ptl_frame* frame, int n, const void* lists, unsigned long long list_stride, const void* counts,
                                               void* out_rgba8, void* out_rgba32f, unsigned long long slice_pixels, void* segments, void* stream, float* elapsed_ms) {
    if (!k || !frame || !lists || !counts || frame->width <= 0 || frame->height <= 0) return PTL_ERR_INVALID;
    if (int rc = check_listed_frame("ptl_kernel_render_slices_refine", "the lists name", frame); rc != PTL_OK) return rc;
    const unsigned long long pixels = (unsigned long long)frame->width * (unsigned long long)frame->height;
    if (list_stride < pixels || slice_pixels < pixels) {
        set_last_error("ptl_kernel_render_slices_refine: list_stride and slice_pixels must be at least width * height");
        return PTL_ERR_INVALID;
    }
    if (n < 1 || n > kMaxSlices) return PTL_ERR_INVALID;
    if (!k->has_refine_slices) {
        set_last_error("ptl_kernel_render_slices_refine: the kernel was not generated with the refine entry over slices (PTL_FLAG_REFINE_SLICES)");
        return PTL_ERR_INVALID;
    }
    if (k->staged.empty()) {
        set_last_error("ptl_kernel_render_slices_refine: no staged slices (ptl_kernel_stage_slice)");
        return PTL_ERR_INVALID;
    }
    if (k->device < 0 || !k->refine_slices_fn || !k->sliced) return PTL_ERR_NO_DEVICE;
    const int rc = launch_refine(k, true, frame, n, lists, list_stride, counts, out_rgba8, out_rgba32f, slice_pixels, segments, stream, elapsed_ms);
    if (rc == PTL_OK) k->staged_since_launch = false;  // what was staged is launched (launch_render)
    return rc;
}

extern "C" int ptl_kernel_render_to_host(ptl_kernel* k, const ptl_frame* frame, uint8_t* host_rgba8, float* host_rgba32f,
                                         uint64_t* host_segments, float* elapsed_ms) {
    if (!k || !frame) return PTL_ERR_INVALID;
    int rows = ptl_frame_shard_rows(frame);
    if (rows < 0) return PTL_ERR_INVALID;
    if (frame->in_place) {
        set_last_error("in_place frames are rendered into a caller-owned full-frame DEVICE buffer (ptl_kernel_render / ptl_renderer_draw)");
        return PTL_ERR_INVALID;
    }
    if (k->device < 0) return PTL_ERR_NO_DEVICE;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    size_t px = (size_t)rows * frame->width;
    void *d8 = nullptr, *d32 = nullptr, *dseg = nullptr;
    int rc = PTL_OK;
    auto cleanup = [&] {
        if (d8) rt->hipFree(d8);
        if (d32) rt->hipFree(d32);
        if (dseg) rt->hipFree(dseg);
    };
    if (host_rgba8 && !hip_ok(rt, rt->hipMalloc(&d8, px * 4 + 16), "hipMalloc(rgba8)")) rc = PTL_ERR_HIP;
    if (rc == PTL_OK && host_rgba32f && !hip_ok(rt, rt->hipMalloc(&d32, px * 16 + 16), "hipMalloc(rgba32f)")) rc = PTL_ERR_HIP;
    if (rc == PTL_OK && host_segments) {
        if (!hip_ok(rt, rt->hipMalloc(&dseg, 8), "hipMalloc(segments)")) rc = PTL_ERR_HIP;
        else rt->hipMemsetAsync(dseg, 0, 8, nullptr);
    }
    if (rc == PTL_OK) rc = ptl_kernel_render(k, frame, d8, d32, dseg, nullptr, elapsed_ms);
    if (rc == PTL_OK && !hip_ok(rt, rt->hipStreamSynchronize(nullptr), "hipStreamSynchronize")) rc = PTL_ERR_HIP;
    if (rc == PTL_OK && d8 && !hip_ok(rt, rt->hipMemcpy(host_rgba8, d8, px * 4, hip::kMemcpyDeviceToHost), "hipMemcpy(rgba8)")) rc = PTL_ERR_HIP;
    if (rc == PTL_OK && d32 && !hip_ok(rt, rt->hipMemcpy(host_rgba32f, d32, px * 16, hip::kMemcpyDeviceToHost), "hipMemcpy(rgba32f)")) rc = PTL_ERR_HIP;
    if (rc == PTL_OK && dseg && !hip_ok(rt, rt->hipMemcpy(host_segments, dseg, 8, hip::kMemcpyDeviceToHost), "hipMemcpy(segments)")) rc = PTL_ERR_HIP;
    cleanup();
    return rc;
}

// The teleport half of a split build (see ptl_kernel::split): compiled -- or found in the code-object cache -- once per kernel, on the
// kernel's device (a compile-only handle gets a compile-only companion: that fills the cache).
extern "C" int ptl_kernel_prebuild_teleport(ptl_kernel* k) {
    if (!k) return PTL_ERR_INVALID;
    if (!k->split || k->companion) return PTL_OK;
    std::vector<std::string> defs;
    for (auto& d : k->defines)
        if (d != "PTL_RENDER_MODULE") defs.push_back(d);
    defs.push_back("PTL_TELEPORT_MODULE");
    std::vector<const char*> cdefs;
    for (auto& d : defs) cdefs.push_back(d.c_str());
    std::vector<ptl_uniform_desc> descs;
    for (auto& sl : k->slots) descs.push_back(ptl_uniform_desc{sl.first.c_str(), sl.second.type, sl.second.offset});
    ptl_kernel* c = nullptr;
    int rc = ptl_kernel_compile(k->device, k->source.c_str(), descs.data(), (int)descs.size(), k->shadow.size(), cdefs.data(), (int)cdefs.size(), &c, nullptr, 0);
    if (rc != PTL_OK) return rc;
    if (k->device >= 0 && !c->teleport_fn) {
        ptl_kernel_destroy(c);
        set_last_error("the teleport half of the build has no ptl_teleport_kernel entry");
        return PTL_ERR_INVALID;
    }
    k->companion = c;
    return PTL_OK;
}

extern "C" int ptl_kernel_teleport_ray(ptl_kernel* k, const float a[3], const float b[3], float out_pos[3], int* hit_object,
                                       int* changed_subspace, int* teleported) {
    if (!k || !a || !b) return PTL_ERR_INVALID;
    if (k->device < 0 || (!k->fn && !k->teleport_fn)) return PTL_ERR_NO_DEVICE;
    if (!k->teleport_fn && k->split) {  // the query runs on the other half of the build, with this kernel's uniform values
        if (int rc = ptl_kernel_prebuild_teleport(k); rc != PTL_OK) return rc;
        ptl_kernel* c = k->companion;
        if (c->shadow.size() != k->shadow.size()) return PTL_ERR_INVALID;
        if (std::memcmp(c->shadow.data(), k->shadow.data(), k->shadow.size()) != 0) {
            c->shadow = k->shadow;
            c->dirty = true;
        }
        int rc = ptl_kernel_teleport_ray(c, a, b, out_pos, hit_object, changed_subspace, teleported);
        // (the segment end points the query wrote into the companion's block stay there; this kernel's block never sees them)
        return rc;
    }
    if (!k->teleport_fn) {
        set_last_error("the loaded code object has no ptl_teleport_kernel entry");
        return PTL_ERR_INVALID;
    }
    int rc = ptl_kernel_set_uniform(k, "_external_ray_a", PTL_VEC3, a);
    if (rc < 0) return rc;
    rc = ptl_kernel_set_uniform(k, "_external_ray_b", PTL_VEC3, b);
    if (rc < 0) return rc;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!hip_ok(rt, rt->hipSetDevice(k->device), "hipSetDevice")) return PTL_ERR_HIP;
    // The query rewrites the module's ONE uniform block (segment end points, teleport_light_u) and runs on the NULL stream; a frame
    // launched on a non-blocking stream may still be reading the block: wait for it first.
    if (k->launched && k->ev_done && !hip_ok(rt, rt->hipEventSynchronize(k->ev_done), "hipEventSynchronize(last render launch)")) return PTL_ERR_HIP;
    if (int rc2 = upload_uniforms(k, rt, nullptr); rc2 != PTL_OK) return rc2;
    void* dev_out = nullptr;
    if (!hip_ok(rt, rt->hipMalloc(&dev_out, 8 * sizeof(float)), "hipMalloc(teleport result)")) return PTL_ERR_HIP;
    void* args[] = {&dev_out};
    float out[6] = {0};
    bool ok = hip_ok(rt, rt->hipModuleLaunchKernel(k->teleport_fn, 1, 1, 1, 64, 1, 1, 0, nullptr, args, nullptr), "hipModuleLaunchKernel(teleport)") &&
              hip_ok(rt, rt->hipMemcpy(out, dev_out, sizeof out, hip::kMemcpyDeviceToHost), "hipMemcpy(teleport result)");
    rt->hipFree(dev_out);
    if (!ok) return PTL_ERR_HIP;
    if (out_pos) std::memcpy(out_pos, out, 3 * sizeof(float));
    if (teleported) *teleported = out[3] != 0.0f;
    if (hit_object) *hit_object = out[4] != 0.0f;
    if (changed_subspace) *changed_subspace = out[5] != 0.0f;
    return PTL_OK;
}

extern "C" void ptl_kernel_destroy(ptl_kernel* k) {
    if (!k) return;
    if (k->companion) ptl_kernel_destroy(k->companion);
    const hip::Runtime* rt = k->device >= 0 ? hip::runtime(nullptr) : nullptr;
    if (rt) {
        rt->hipSetDevice(k->device);
        if (k->launched && k->ev_done) rt->hipEventSynchronize(k->ev_done);  // a re-JIT replaces the handle: nothing may still run from the old module
        if (k->ev_done) rt->hipEventDestroy(k->ev_done);
        for (auto& t : k->textures)
            if (t.second) rt->hipFree(t.second);
        free_retired_textures(k, rt);
        if (k->dev_slices) rt->hipFree(k->dev_slices);
        if (k->ev0) rt->hipEventDestroy(k->ev0);
        if (k->ev1) rt->hipEventDestroy(k->ev1);
        if (k->module) rt->hipModuleUnload(k->module);
    }
    delete k;
}

extern "C" int ptl_deinterleave_rows(const uint8_t* shard, const ptl_frame* f, uint8_t* full) {
    if (!shard || !f || !full || ptl_frame_shard_rows(f) < 0) return PTL_ERR_INVALID;
    int blocks = (f->height + 7) / 8;
    size_t pitch = (size_t)f->width * 4;
    size_t src_row = 0;
    for (int b = f->rb_phase; b < blocks; b += f->rb_stride) {
        for (int r = 0; r < 8 && b * 8 + r < f->height; ++r) {
            std::memcpy(full + (size_t)(b * 8 + r) * pitch, shard + src_row * pitch, pitch);
            ++src_row;
        }
    }
    return PTL_OK;
}
