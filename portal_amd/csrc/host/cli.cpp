// cli.cpp -- the `portal-amd` command line, the offline counterpart of the reference CLI: argument parsing and `main`, `render-frame`
// (`portal render-frame <scene> ...` src/main.rs:2726-2755,2876-2946; one frame on one GPU, across the GPUs of a node, or across processes),
// `precompile`, `check`, `write` and `emit-source`.  `render` (clips to video frames, src/main.rs:2757-2874) is in cli_video.cpp; what both
// files share -- Options, the build flags, the scene / renderer / PNG helpers -- is in cli_common.h.  Everything goes through the C ABI
// (include/portal_amd.h); this file holds no rendering logic.
#include <sys/wait.h>
#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "cli_png.h"

namespace {

int usage() {  // (and the exit status that goes with it)
    std::fprintf(stderr,
                 "usage: portal-amd render-frame <scene.ron> [--stage NAME | --animation NAME] [--camera NAME] [--time T] [--output out.png]\n"
                 "                  [--width W] [--height H] [--aa-count N] [--render-depth D] [--device I] [--asset-root DIR] [--panini D --fov DEG]\n"
                 "                  [--gpus N | --devices a,b,..] [--transport stores|copy|rccl] [--multi-process]   one frame across the GPUs of a node\n"
                 "                  [--specialize 0] do NOT bake the scene state into the kernel   [--fast] tolerance mode   [--exact-cr] numerics contract 1   [--opt3] JIT at -O3 like the library default (render-frame: -O1)   [--timing] where the wall time went\n"
                 "                  [--adaptive-aa [T]]  one sample per pixel, --aa-count samples only where a pixel differs from a neighbour by more than T codes (default 4, -1 .. 255); one GPU\n"
                 "                  [--png-depth 8|16]   16: a 16-bit RGB file made on the GPU from the frame's float output (one quantisation, to 16 bits); one GPU\n"
                 "                  [--png-encoder host|gpu]  gpu: the 8-bit file's deflate stream is made on the GPU (fixed Huffman codes, runs only: about twice the size);\n"
                 "                                       the host adds the chunk framing and CRCs.  One GPU; not with --png-depth 16\n"
                 "                  [--png-codes fixed|dynamic]  with the gpu encoder: fixed (default) or dynamic, a Huffman code per band of the stream, made on the GPU:\n"
                 "                                       the same pixels in a file of about the host encoder's size at 4K\n"
                 "                  [--png16-encoder host|gpu]  with --png-depth 16: gpu deflates the 16-bit file's scanlines on the GPU (Up filter, matches at pixel distance,\n"
                 "                                       a Huffman code per band); the host adds the chunk framing and CRCs.  host (default): zlib\n"
                 "                  [--passes depth,trips,cut]  beside the frame: <output stem>.depth.png (nearest final depth, scaled between the scene's depth-map bounds),\n"
                 "                                       <output stem>.trips.png (bounce-loop trips per pixel) and <output stem>.cut.png (the share of the pixel's traced paths\n"
                 "                                       that --render-depth cut short: 0 none, 65535 all), 16-bit greyscale, from the tracer's pass records; one GPU\n"
                 "                  [--depth-report]     one line: how many paths --render-depth cut short (they are drawn black), in how many pixels; the deepest pixel; the depth range\n"
                 "       portal-amd precompile <scene.ron> [--stage NAME] [--specialize 0]      fill the code-object cache (no GPU needed; render's options choose render's kernels)\n"
                 "       portal-amd render <scene[,scene..]> [clip[,clip..]] [--width 3840] [--height 2160] [--fps 60] [--motion-blur-frames 1]\n"
                 "                  [--stereoimage] [--batch-subframes 0|1] [--no-skip-existing] [--filter-starts-with P] [--aa-count 4] [--render-depth 150]\n"
                 "                  [--scenes-dir DIR] [--out-dir DIR] [--device I] [--shard K/N] [--max-frames N] [--asset-root DIR]\n"
                 "                  [--specialize 0|1]   bake what is constant within a clip into the kernel (default: when it pays)\n"
                 "                  [--fast]             tolerance mode for the whole clip (hardware rcp / sqrt, FMA contraction)\n"
                 "                  [--timing]           wait for every kernel and report GPU time (no host/GPU overlap)\n"
                 "                  [--frames png|y4m]   png (default): anim/frame_%%d.png, then ffmpeg.  y4m: YUV 4:2:0 10-bit frames from the GPU, streamed in order\n"
                 "                                       into ffmpeg's stdin while the clip renders (or to video/<scene>/<clip>.y4m without ffmpeg, with --max-frames).\n"
                 "                                       Not with --shard K/N, N > 1 (a stream needs every frame, in order); a clip is not resumed, it starts at frame 0\n"
                 "                  [--deep-colour]      with --frames y4m: the 10-bit frames are made from the un-quantised float sub-frames (one quantisation, to 16 bits,\n"
                 "                                       instead of two to 8 bits): a smooth gradient keeps 1024 luma codes instead of 256.  16 more bytes per pixel and sub-frame on the card\n"
                 "                  [--chroma 420|422|444]  with --frames y4m: the chroma sampling of the stream (default 420).  422 keeps every row of chroma, 444 every sample:\n"
                 "                                       4 and 6 bytes per pixel leave the card instead of 3, and the encoder is told yuv422p10le / yuv444p10le\n"
                 "                  [--png-depth 8|16]   with --frames png: 16 makes anim/frame_%%d.png 16-bit RGB files from the un-quantised float sub-frames (the averaged\n"
                 "                                       frame of --deep-colour), Sub-filtered on the GPU; works with --shard K/N and resumes.  16 more bytes per pixel and\n"
                 "                                       sub-frame on the card, 6 instead of 4 bytes per pixel leave it, and the files are 4 - 7 times larger to deflate\n"
                 "                  [--png-encoder host|gpu]  with --frames png: gpu deflates every 8-bit frame on the GPU (fixed Huffman codes, runs only), so an encoder thread\n"
                 "                                       only frames the stream and computes its CRC; the files are about twice the size.  Works with --shard K/N and resumes;\n"
                 "                                       the stills stay host-encoded.  Not with --frames y4m or --png-depth 16\n"
                 "                  [--png-codes fixed|dynamic]  with the gpu encoder: fixed (default) or dynamic, a Huffman code per band of every frame's stream, made on\n"
                 "                                       the GPU: the same pixels, files of about the host encoder's size at 4K instead of twice that\n"
                 "                  [--png16-encoder host|gpu]  with --png-depth 16: gpu deflates every 16-bit frame on the GPU (Up filter, matches at pixel distance, a Huffman\n"
                 "                                       code per band), so an encoder thread only frames the stream and computes its CRC; files about 1.3 - 1.4 times the\n"
                 "                                       host encoder's.  Works with --shard K/N and resumes; host (default): zlib level 3 on the encoder threads\n"
                 "                  [--depth-report]     one line per clip: how many paths --render-depth cut short, in how many pixels, and the frame that lost most\n"
                 "                  [--clip-passes depth,trips,cut]  beside every frame_<i>.png: anim/depth_<i>.png (nearest final depth over the frame's blur sub-frames, scaled\n"
                 "                                       between the scene's depth-map bounds), anim/trips_<i>.png (bounce-loop trips, summed) and anim/cut_<i>.png (the share of\n"
                 "                                       the pixel's traced paths that --render-depth cut short), 16-bit greyscale, merged on the GPU from the sub-frames' pass\n"
                 "                                       records.  Works with --shard K/N, --frames y4m and the report line; a frame with a pass file missing is drawn again; one GPU\n"
                 "                  [--pass-encoder host|gpu]  with --clip-passes: gpu deflates every pass image on the GPU (its rows taken as W / 3 RGB pixels: Up filter, matches\n"
                 "                                       at distance 6, a Huffman code per band), so an encoder thread only frames the stream; W must be a multiple of 3.\n"
                 "                                       The default, host: zlib level 3 on the encoder threads\n"
                 "                  [--clip-adaptive-aa [T]]  adaptive anti-aliasing of every sub-frame: one sample per pixel, --aa-count samples only where a pixel differs\n"
                 "                                       from a neighbour by more than T codes (default 4, -1 .. 255); opt-in, approximate by design\n"
                 "       portal-amd emit-source <scene.ron> [--stage NAME]     print the generated HIP kernel source\n"
                 "       portal-amd check <scene.ron> [--stage NAME]           compile for gfx950 (no GPU needed); errors by scene element\n"
                 "       portal-amd write <scene.ron> [--stage NAME] [--set UNIFORM=VALUE ...] --output out.ron     the reference's RON writer\n"
                 "       portal-amd version\n");
    return 2;
}

int refuse(const char* why) {  // while the arguments are parsed: one line of reason, exit status 2, nothing done
    std::fprintf(stderr, "%s\n", why);
    return 2;
}

// Everything of `render-frame` between creating a renderer and drawing (src/main.rs:2893-2928): stage / clip, camera, options,
// one SceneRenderer::update at --time.  `scene_state` = false for ranks 1.. of a multi-GPU frame, which share rank 0's scene.
int setup_renderer(const Options& o, ptl_scene* scene, ptl_renderer* r, bool scene_state) {
    ptl_renderer_set_option(r, "aa_count", o.aa);
    ptl_renderer_set_option(r, "render_depth", o.depth);
    if (scene_state && !init_stage(o, scene)) return 1;
    if (!o.animation.empty()) {  // src/main.rs:2905-2917
        if (scene_state && ptl_scene_init_animation(scene, o.animation.c_str()) != PTL_OK) return scene_has_no(o.scene, "animation", o.animation);
        apply_clip_overrides(scene_state ? scene : nullptr, r, o.animation, nullptr);
    }
    if (o.have_camera && ptl_renderer_use_camera(r, o.camera.c_str()) != PTL_OK) return scene_has_no(o.scene, "camera", o.camera);  // --camera wins (src/main.rs:2918-2926)
    if (o.panini >= 0.0) {
        ptl_renderer_set_option(r, "use_panini_projection", 1);
        ptl_renderer_set_option(r, "panini_param", o.panini);
    }
    ptl_renderer_set_option(r, "view_angle", o.fov / 180.0 * 3.14159265358979323846);
    if (ptl_renderer_update(r, o.time, nullptr, nullptr) != PTL_OK) return fail("update");  // src/main.rs:2928
    return 0;
}

unsigned frame_flags(const Options& o) {
    unsigned f = kRenderFlags;
    // One frame of one scene state: baking the state in is the cheaper build (0.74 s against 1.08 s of hiprtc for the headline scene:
    // the folded source is smaller) AND the faster kernel (0.53 against 1.31 ms), so it is the default; --specialize 0 keeps every
    // scene uniform a run-time value (profiles/r02/render_frame_e2e.log).
    if (o.specialize != 0) f |= PTL_FLAG_SPECIALIZE_INTS | PTL_FLAG_SPECIALIZE_ALL;
    f |= numerics_flags(o) | quick_jit_flag(o);
    if (o.adaptive) f |= PTL_FLAG_REFINE;  // the kernel's second render entry, over the list of flagged pixels
    if (o.have_passes || o.depth_report) f |= PTL_FLAG_PASSES;  // the tracer's record per pixel, stored beside the colour
    return f;
}

std::string hex_of(const unsigned char* bytes, size_t n) {
    static const char* digits = "0123456789abcdef";
    std::string out;
    for (size_t k = 0; k < n; ++k) {
        out += digits[bytes[k] >> 4];
        out += digits[bytes[k] & 15];
    }
    return out;
}
bool unhex(const std::string& hex, unsigned char* out, size_t n) {
    if (hex.size() != 2 * n) return false;
    auto val = [](char c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1; };
    for (size_t k = 0; k < n; ++k) {
        int hi = val(hex[2 * k]), lo = val(hex[2 * k + 1]);
        if (hi < 0 || lo < 0) return false;
        out[k] = (unsigned char)(hi * 16 + lo);
    }
    return true;
}

std::vector<int> frame_devices(const Options& o) {
    std::vector<int> devices;
    for (auto& d : split_list(o.devices)) devices.push_back(std::atoi(d.c_str()));
    if (devices.empty())
        for (int k = 0; k < std::max(1, o.gpus); ++k) devices.push_back(o.gpus > 1 ? k : o.device);
    return devices;
}

// `render-frame --gpus N --multi-process`: rank 0 (this process) owns the frame in its GPU's memory and exports it (HIP IPC);
// ranks 1.. are child processes (`portal-amd render-shard`, the same command line + rank / device / handle) that map it and
// let their kernels store their row blocks straight into it over xGMI.  Completion = the children's exit.
int render_frame_processes(const Options& o, const std::vector<int>& devices) {
    const int n = (int)devices.size();
    auto t0 = std::chrono::steady_clock::now();
    ScenePtr scene = load_scene(o);
    if (!scene) return 1;
    size_t bytes = (size_t)o.width * o.height * 4;
    void* frame = nullptr;
    unsigned char handle[PTL_IPC_HANDLE_BYTES];
    if (ptl_device_alloc(devices[0], bytes, &frame) != PTL_OK || ptl_ipc_export(frame, handle) != PTL_OK) return fail("frame buffer / ipc export");
    std::vector<pid_t> children;
    // every failure path below reaps the shard processes already forked: they render into `frame`, which dies with this process
    auto reap = [&](int rc) {
        for (pid_t pid : children) {
            int status = 0;
            ::waitpid(pid, &status, 0);
        }
        children.clear();
        return rc;
    };
    for (int k = 1; k < n; ++k) {
        std::vector<std::string> args = o.argv;
        args[1] = "render-shard";
        for (auto extra : {std::string("--rank"), std::to_string(k), std::string("--world"), std::to_string(n), std::string("--device"),
                           std::to_string(devices[k]), std::string("--ipc-handle"), hex_of(handle, sizeof handle)})
            args.push_back(extra);
        pid_t pid = ::fork();
        if (pid == 0) {
            std::vector<char*> argv;
            for (auto& a : args) argv.push_back(const_cast<char*>(a.c_str()));
            argv.push_back(nullptr);
            ::execv("/proc/self/exe", argv.data());
            std::perror("execv");
            ::_exit(127);
        }
        if (pid < 0) return reap(fail("fork"));
        children.push_back(pid);
    }
    RendererPtr r = create_renderer(scene.get(), devices[0], o, frame_flags(o));
    if (!r) return reap(1);
    if (int rc = setup_renderer(o, scene.get(), r.get(), true)) return reap(rc);
    ptl_frame f{o.width, o.height, 0, n, 1};
    float ms = 0.0f;
    if (ptl_renderer_draw(r.get(), &f, frame, nullptr, nullptr, nullptr, &ms) != PTL_OK) return reap(fail("render"));
    int failed = 0;
    for (pid_t pid : children) {
        int status = 0;
        if (::waitpid(pid, &status, 0) < 0 || !WIFEXITED(status) || WEXITSTATUS(status) != 0) ++failed;
    }
    if (failed) {
        std::fprintf(stderr, "%d of %d shard processes failed\n", failed, n - 1);
        return 1;
    }
    std::vector<uint8_t> img(bytes);
    if (ptl_device_download(img.data(), frame, bytes, nullptr) != PTL_OK) return fail("download");
    if (int rc = write_png(o.output, img.data(), o.width, o.height)) return rc;
    std::printf("Rendered `%s` to `%s` (%dx%d, aa %d, depth %d) with %d processes, one per GPU, storing into rank 0's frame (HIP IPC): rank 0 kernel %.3f ms; total %.2f s\n",
                o.scene.c_str(), o.output.c_str(), o.width, o.height, o.aa, o.depth, n, ms, seconds_since(t0));
    r.reset();
    ptl_device_free(frame);
    return 0;
}

// One of those child processes.
int render_shard(const Options& o) {
    unsigned char handle[PTL_IPC_HANDLE_BYTES];
    if (o.world < 2 || o.rank < 1 || o.rank >= o.world || !unhex(o.ipc_handle, handle, sizeof handle)) return refuse("render-shard is started by `render-frame --gpus N --multi-process`");
    ScenePtr scene = open_scene(o.scene);
    if (!scene) return fail("scene");
    RendererPtr r = create_renderer(scene.get(), o.device, o, frame_flags(o));
    if (!r) return 1;
    if (int rc = setup_renderer(o, scene.get(), r.get(), true)) return rc;
    void* frame = nullptr;
    if (ptl_ipc_open(o.device, handle, &frame) != PTL_OK) return fail("ipc open");
    ptl_frame f{o.width, o.height, o.rank, o.world, 1};
    float ms = 0.0f;
    if (ptl_renderer_draw(r.get(), &f, frame, nullptr, nullptr, nullptr, &ms) != PTL_OK) return fail("render");  // timed: returns when the kernel (and its stores) have completed
    ptl_ipc_close(frame);
    return 0;
}

// --png-encoder gpu, --png16-encoder gpu: of a deflate's result buffer the header comes down first, then exactly the stream it announces.
// `deflate`: the entry that filled the buffer, which the bounds check names
int download_stream(const void* dev_result, size_t result_bytes, const char* deflate, std::vector<uint8_t>* out, unsigned int* stream_bytes) {
    const size_t header_bytes = PTL_PNG_STREAM_HEADER_BYTES;
    out->resize(header_bytes);
    if (ptl_device_download(out->data(), dev_result, header_bytes, nullptr) != PTL_OK) return fail("download");
    std::memcpy(stream_bytes, out->data() + 12, 4);
    if (header_bytes + *stream_bytes > result_bytes) return fail((std::string(deflate) + ": the header's byte count").c_str());
    out->resize(header_bytes + *stream_bytes);
    if (ptl_device_download(out->data() + header_bytes, static_cast<const char*>(dev_result) + header_bytes, *stream_bytes, nullptr) != PTL_OK) return fail("download");
    return 0;
}

int render_frame(const Options& o) {
    std::vector<int> devices = frame_devices(o);
    if (devices.size() > 1 && o.multi_process) return render_frame_processes(o, devices);
    auto t0 = std::chrono::steady_clock::now();
    ScenePtr scene = load_scene(o);
    if (!scene) return 1;
    double t_load = seconds_since(t0);
    if (devices.size() > 1 || o.transport == "rccl") {  // one process, one renderer per GPU (include/portal_amd.h layer 3); `--transport rccl` also with one
        std::vector<uint8_t> img((size_t)o.width * o.height * 4);
        std::vector<char> log(1 << 16);
        ptl_frame_group* g = nullptr;
        int transport = o.transport == "copy" ? PTL_GROUP_COPY_GATHER : o.transport == "rccl" ? PTL_GROUP_RCCL_GATHER : PTL_GROUP_PEER_STORES;
        if (ptl_frame_group_create(scene.get(), devices.data(), (int)devices.size(), o.asset_root.c_str(), frame_flags(o), transport, &g, log.data(), log.size()) != PTL_OK) {
            std::fprintf(stderr, "frame group: %s\n%s\n", ptl_last_error(), log.data());
            return 1;
        }
        double t_build = seconds_since(t0);
        for (int k = 0; k < ptl_frame_group_size(g); ++k)
            if (int rc = setup_renderer(o, scene.get(), ptl_frame_group_renderer(g, k), k == 0)) return rc;
        std::vector<float> ms(devices.size(), 0.0f);
        auto t_draw0 = std::chrono::steady_clock::now();
        if (ptl_frame_group_draw(g, o.width, o.height, nullptr, ms.data()) != PTL_OK) return fail("render");
        double draw_ms = seconds_since(t_draw0) * 1e3;
        if (ptl_frame_group_download(g, img.data()) != PTL_OK) return fail("download");
        if (int rc = write_png(o.output, img.data(), o.width, o.height)) return rc;
        std::string per_rank;
        for (float m : ms) per_rank += (per_rank.empty() ? "" : " ") + std::to_string(m).substr(0, 6);
        std::printf("Rendered `%s` to `%s` (%dx%d, aa %d, depth %d) on %zu GPUs (%s): kernel ms per rank [%s], frame %.3f ms wall; build %.2f s, total %.2f s\n",
                    o.scene.c_str(), o.output.c_str(), o.width, o.height, o.aa, o.depth, devices.size(),
                    transport == PTL_GROUP_COPY_GATHER ? "packed shards + one strided peer copy each" : transport == PTL_GROUP_RCCL_GATHER ? "packed shards + one RCCL gather" : "kernels store into GPU 0's frame", per_rank.c_str(), draw_ms,
                    t_build - t_load, seconds_since(t0));
        ptl_frame_group_destroy(g);
        return 0;
    }
    RendererPtr owned = create_renderer(scene.get(), devices[0], o, frame_flags(o));
    if (!owned) return 1;
    ptl_renderer* r = owned.get();
    double t_build = seconds_since(t0);
    if (int rc = setup_renderer(o, scene.get(), r, true)) return rc;
    ptl_frame frame{o.width, o.height, 0, 1, 0};
    const int device = devices[0];
    const PngForm form(o);
    // --passes / --depth-report: the draw also stores the pass records, which stay on the card for the two kernels that read them
    const bool with_records = o.have_passes || o.depth_report;
    const size_t n_px = (size_t)o.width * o.height, record_bytes = ptl_pass_record_bytes(o.width, o.height);
    // The plain file needs nothing on the card: its draw downloads the frame.  Every other run draws into an RGBA8 frame there (which the adaptive
    // classification reads), with an RGBA32F one beside it where the form wants floats, and the form makes its result of them with n = 1
    const bool to_host = form.draws_result(1) && !o.adaptive && !with_records, made = !form.draws_result(1);
    const size_t result_bytes = form.result_bytes(o.width, o.height), staging_bytes = form.staging_bytes(o.width, o.height, 1);
    if (form.gpu && result_bytes == 0) return fail(form.sixteen ? "--png16-encoder gpu: the frame's scanlines exceed 2^31 bytes" : "--png-encoder gpu: the frame's scanlines exceed 2^31 bytes");
    DevicePtr records, dev8, dev32, staging, result;
    if (with_records && !(records = device_alloc(device, record_bytes, "device records"))) return 1;
    if (!to_host && !(dev8 = device_alloc(device, n_px * 4, "device frame"))) return 1;
    if (form.wants_float() && !(dev32 = device_alloc(device, n_px * 16, "device frame"))) return 1;
    if (staging_bytes != 0 && !(staging = device_alloc(device, staging_bytes, "device frame"))) return 1;
    if (made && !(result = device_alloc(device, result_bytes, form.gpu ? "device stream" : "device frame"))) return 1;
    float ms = 0.0f, pass_ms[3] = {0.0f, 0.0f, 0.0f}, deflate_ms = 0.0f;
    unsigned int refined = 0;
    std::vector<uint8_t> img(to_host ? n_px * 4 : 0);  // what the form's host step gets
    if (o.adaptive) {  // one sample per pixel, classification, the flagged pixels again with --aa-count samples: three launches
        void *list = nullptr, *count = nullptr;
        ptl_renderer_set_option(r, "adaptive_aa_threshold", o.adaptive_t);
        if (ptl_renderer_draw_adaptive(r, &frame, dev8.get(), dev32.get(), nullptr, &ms) != PTL_OK) return fail("render");
        if (ptl_renderer_adaptive_result(r, &list, &count) != PTL_OK || ptl_device_download(&refined, count, sizeof refined, nullptr) != PTL_OK) return fail("refined count");
        ptl_renderer_adaptive_times(r, pass_ms);
    } else if ((to_host        ? ptl_renderer_draw_to_host(r, &frame, img.data(), nullptr, nullptr, &ms)
                : with_records ? ptl_renderer_draw_passes(r, &frame, dev8.get(), dev32.get(), records.get(), record_bytes, nullptr, nullptr, &ms)
                               : ptl_renderer_draw(r, &frame, dev8.get(), dev32.get(), nullptr, nullptr, &ms)) != PTL_OK)
        return fail("render");
    const void *one8[1] = {dev8.get()}, *one32[1] = {dev32.get()};
    if (made)
        if (int rc = form.make(device, one8, one32, 1, staging.get(), result.get(), o.width, o.height, nullptr, o.timing ? &deflate_ms : nullptr)) return rc;
    if (form.gpu) {
        unsigned int stream_bytes = 0;
        if (int rc = download_stream(result.get(), result_bytes, form.deflate_name(), &img, &stream_bytes)) return rc;
        if (o.timing) std::printf("%s encoder gpu: deflate %.3f ms, %u bytes of stream downloaded\n", form.sixteen ? "png16" : "png", deflate_ms, stream_bytes);
    } else if (!to_host) {
        img.resize(result_bytes);
        if (ptl_device_download(img.data(), made ? result.get() : dev8.get(), img.size(), nullptr) != PTL_OK) return fail("download");
    }
    // the pass images: the records as 16-bit grey scanlines, made on the card, 2 bytes per pixel downloaded
    const std::string stem = o.output.size() > 4 && o.output.compare(o.output.size() - 4, 4, ".png") == 0 ? o.output.substr(0, o.output.size() - 4) : o.output;
    std::vector<uint8_t> grey[2], grey_cut;
    if (o.have_passes) {
        const DevicePtr dev_grey = device_alloc(device, 2 * n_px, "device pass image");
        if (!dev_grey) return 1;
        float lo[16] = {0.0f}, hi[16] = {1.0f};  // the scene's depth-map bounds, as a draw uploads them
        ptl_renderer_uniform_value(r, o.width, o.height, "_depth_map_min", lo, nullptr);
        ptl_renderer_uniform_value(r, o.width, o.height, "_depth_map_max", hi, nullptr);
        for (int which : {PTL_PASS_DEPTH, PTL_PASS_TRIPS}) {
            if (!(which == PTL_PASS_DEPTH ? o.pass_depth : o.pass_trips)) continue;
            grey[which].resize(2 * n_px);
            if (ptl_passes_to_gray16(device, records.get(), (long)n_px, dev_grey.get(), which, lo[0], hi[0], nullptr, nullptr) != PTL_OK) return fail("passes_to_gray16");
            if (ptl_device_download(grey[which].data(), dev_grey.get(), grey[which].size(), nullptr) != PTL_OK) return fail("download");
        }
        if (o.pass_cut) {  // the share of cut paths: the clip's merge over ONE slice
            grey_cut.resize(2 * n_px);
            if (ptl_pass_slices_to_gray16(device, records.get(), 1, n_px, (long)n_px, nullptr, nullptr, dev_grey.get(), lo[0], hi[0], nullptr, nullptr) != PTL_OK) return fail("pass_slices_to_gray16");
            if (ptl_device_download(grey_cut.data(), dev_grey.get(), grey_cut.size(), nullptr) != PTL_OK) return fail("download");
        }
    }
    ptl_pass_stats_block stats{};
    if (o.depth_report) {
        const DevicePtr dev_stats = device_alloc(device, sizeof stats, "device statistics");
        if (!dev_stats) return 1;
        if (ptl_device_memset(dev_stats.get(), 0, sizeof stats, nullptr) != PTL_OK || ptl_pass_stats(device, records.get(), (long)n_px, dev_stats.get(), nullptr, 0, nullptr, nullptr) != PTL_OK ||
            ptl_device_download(&stats, dev_stats.get(), sizeof stats, nullptr) != PTL_OK)
            return fail("pass_stats");
    }
    double t_draw = seconds_since(t0);
    if (!dir_of(o.output).empty()) make_dirs(dir_of(o.output));
    if (form.write(o.output.c_str(), img.data(), o.width, o.height, 6) != PTL_OK) return fail("png");
    for (int which : {PTL_PASS_DEPTH, PTL_PASS_TRIPS})
        if (!grey[which].empty() && ptl_png_write_gray16((stem + (which == PTL_PASS_DEPTH ? ".depth.png" : ".trips.png")).c_str(), grey[which].data(), o.width, o.height, 6) != PTL_OK)
            return fail("png");
    if (!grey_cut.empty() && ptl_png_write_gray16((stem + ".cut.png").c_str(), grey_cut.data(), o.width, o.height, 6) != PTL_OK) return fail("png");
    double total = seconds_since(t0);
    std::printf("Rendered `%s` to `%s` (%dx%d, aa %d, depth %d): kernel %.3f ms, %.1f Mray/s; total %.2f s\n", o.scene.c_str(), o.output.c_str(),
                o.width, o.height, o.aa, o.depth, ms, (double)o.width * o.height * o.aa / (ms * 1e3), total);
    if (o.adaptive && o.timing)
        std::printf("adaptive aa: threshold %d, %u of %zu pixels refined (%.2f %%); GPU ms: one-sample pass %.3f, classification %.3f, refine pass %.3f\n", o.adaptive_t,
                    refined, (size_t)o.width * o.height, 100.0 * refined / ((double)o.width * o.height), pass_ms[0], pass_ms[1], pass_ms[2]);
    if (o.depth_report) print_depth_report(stats, render_depth_of(r, o.width, o.height));
    if (o.timing)  // where the wall time went: the JIT (or the code-object cache) dominates a single frame
        std::printf("timing: scene load %.3f s, generate + compile/load kernel %.3f s, update + draw + download %.3f s, png %.3f s\n", t_load,
                    t_build - t_load, t_draw - t_build, total - t_draw);
    return 0;
}

// `portal-amd precompile <scene>`: fill the code-object cache for a scene without a GPU (hiprtc only): the dynamic-uniform kernel
// `render-frame` / `render` start with and, with --specialize 1, the kernel with the scene's current state baked in.  A later
// run on a GPU box with the same toolchain finds them by source + option + toolchain hash and only loads them.
int precompile(const Options& o) {
    auto t0 = std::chrono::steady_clock::now();
    ScenePtr scene = load_scene(o);
    if (!scene) return 1;
    char stage_cam[256] = "";
    if (!o.stage.empty() && ptl_scene_init_stage(scene.get(), o.stage.c_str(), stage_cam, sizeof stage_cam) != PTL_OK) return fail("stage");
    std::vector<unsigned> variants = {frame_flags(o)};
    if (o.specialize != 0) variants.push_back(clip_flags(o, false) | quick_jit_flag(o));  // + the dynamic-uniform kernel `render` starts clips with
    for (unsigned flags : variants) {
        auto t1 = std::chrono::steady_clock::now();
        RendererPtr r = create_renderer(scene.get(), -1, o, flags, "compile");
        if (!r) return 1;
        const void* code = nullptr;
        size_t size = 0;
        ptl_kernel_code_object(ptl_renderer_kernel(r.get()), &code, &size);
        std::printf("flags 0x%x: %zu B code object in %.2f s\n", flags, size, seconds_since(t1));
    }
    std::printf("precompiled `%s` in %.2f s\n", o.scene.c_str(), seconds_since(t0));
    return 0;
}

// `check`: what the reference GUI shows when a scene does not compile (shader_error_parser + LineNumbersByKey,
// src/gui/scene.rs:1144-1171): every compiler diagnostic is attributed to the scene element whose snippet produced the
// line, with the line number inside that snippet.  Needs no GPU: hiprtc compiles for gfx950 anywhere.
int check(const Options& o) {
    ScenePtr owned = open_scene(o.scene);
    ptl_scene* scene = owned.get();
    if (!scene) {
        std::printf("%s: cannot load: %s\n", o.scene.c_str(), ptl_last_error());
        return 1;
    }
    char stage_cam[256] = "";
    if (!o.stage.empty() && ptl_scene_init_stage(scene, o.stage.c_str(), stage_cam, sizeof stage_cam) != PTL_OK) {
        std::printf("Scene `%s` has no stage named `%s`\n", o.scene.c_str(), o.stage.c_str());
        return 1;
    }
    std::vector<char> log(1 << 18);
    ptl_renderer* raw = nullptr;
    int rc = ptl_renderer_create(scene, -1, o.asset_root.c_str(), 0, &raw, log.data(), log.size());
    RendererPtr r(raw);
    if (rc == PTL_OK) {
        const ptl_uniform_desc* descs = nullptr;
        int n = 0;
        size_t block = 0;
        ptl_scene_uniform_layout(scene, &descs, &n, &block);
        std::printf("%s: ok (%d uniforms, %zu-byte block)\n", o.scene.c_str(), n, block);
        r.reset();
        // with a GPU: the build `render-frame` draws with (everything baked), and -- where it has affine rays -- the checking build of the same state
        // at 64 x 36: does any ray reach a product with a w the kernel assumes otherwise? (ptl_renderer_check_affine)
        if (ptl_device_count() > 0 && ptl_renderer_create(scene, o.device, o.asset_root.c_str(), PTL_FLAG_SPECIALIZE_INTS | PTL_FLAG_SPECIALIZE_ALL | PTL_FLAG_QUICK_JIT, &raw, log.data(), log.size()) == PTL_OK) {
            r.reset(raw);
            if (ptl_renderer_affine_rays(raw) != 1) {
                std::printf("  affine rays: off for this scene (general products)\n");
                return 0;
            }
            unsigned long long bad = 0;
            if (ptl_renderer_check_affine(raw, 64, 36, &bad) == PTL_OK)
                std::printf("  affine rays: %s\n", bad == 0 ? "hold on every ray of a 64x36 frame (checking build)" : "BROKEN by this scene's snippets -- switched off (please report: the snippet scan let it through)");
            else
                std::printf("  affine rays: not checked (%s)\n", ptl_last_error());
            if (bad != 0) return 3;
        }
        return 0;
    }
    std::string why = ptl_last_error();
    std::printf("%s: does not compile (%s)\n", o.scene.c_str(), why.substr(0, why.find(':')).c_str());
    int errors = 0;
    std::string text = log.data();
    size_t pos = 0;
    while (pos < text.size()) {
        size_t eol = text.find('\n', pos);
        if (eol == std::string::npos) eol = text.size();
        std::string line = text.substr(pos, eol - pos);
        pos = eol + 1;
        int src_line = 0, col = 0;
        size_t tag = line.find("portal_scene.hip:");
        if (tag == std::string::npos || std::sscanf(line.c_str() + tag, "portal_scene.hip:%d:%d:", &src_line, &col) != 2) continue;
        size_t msg = line.find(": ", tag + 17);
        std::string message = msg == std::string::npos ? line : line.substr(msg + 2);
        bool is_error = message.rfind("error", 0) == 0 || message.rfind("fatal error", 0) == 0;
        if (!is_error && message.rfind("warning", 0) != 0) continue;  // notes follow their error
        char kind[64] = "", name[256] = "";
        int local = 0;
        if (ptl_scene_source_line_owner(scene, src_line, kind, sizeof kind, name, sizeof name, &local) == PTL_OK)
            std::printf("  %s `%s`, line %d: %s\n", kind, name, local, message.c_str());
        else
            std::printf("  generated code, line %d: %s\n", src_line, message.c_str());
        errors += is_error;
    }
    if (errors == 0) std::printf("%s\n", log.data());
    return 1;
}

// `write`: load, apply --stage / --set, write the scene back in the reference's own .ron layout (an untouched scene comes
// back byte for byte; serialize_scene_new_format + ron pretty printer, src/gui/scene_serialized.rs:22-24,654-1100).
int write_scene(const Options& o) {
    ScenePtr scene = load_scene(o);
    if (!scene || !init_stage(o, scene.get())) return 1;
    for (auto& kv : o.sets)
        if (ptl_scene_set_uniform(scene.get(), kv.first.c_str(), kv.second) != PTL_OK) return scene_has_no(o.scene, "uniform", kv.first);
    char* text = nullptr;
    if (ptl_scene_to_ron(scene.get(), &text) != PTL_OK) return fail("write");
    std::FILE* f = o.output == "frame.png" ? stdout : std::fopen(o.output.c_str(), "wb");
    if (!f) {
        std::fprintf(stderr, "cannot open `%s`\n", o.output.c_str());
        return 1;
    }
    std::fwrite(text, 1, std::strlen(text), f);
    if (f != stdout) std::fclose(f);
    ptl_free(text);
    return 0;
}

// `emit-source`: the generated HIP kernel source on stdout
int emit_source(const Options& o) {
    ScenePtr scene = load_scene(o);
    if (!scene || !init_stage(o, scene.get())) return 1;
    char* src = nullptr;
    if (ptl_scene_generate_source(scene.get(), 0, &src) != PTL_OK) return fail("generate");
    std::fputs(src, stdout);
    ptl_free(src);
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) return usage();
    std::string cmd = argv[1];
    if (cmd == "version") {
        std::printf("%s\ndevices: %d\n", ptl_version(), ptl_device_count());
        return 0;
    }
    if (argc < 3 || (cmd != "render-frame" && cmd != "render" && cmd != "emit-source" && cmd != "check" && cmd != "write" && cmd != "precompile" &&
                     cmd != "render-shard"))
        return usage();
    Options o;
    o.scene = argv[2];
    o.argv.assign(argv, argv + argc);
    if (cmd == "render") {  // CLI defaults of RenderCliOptions (src/main.rs:2757-2805)
        o.width = 3840;
        o.height = 2160;
        o.aa = 4;
        o.depth = 150;
    }
    for (int i = 3; i < argc; ++i) {
        std::string a = argv[i];
        std::replace(a.begin(), a.end(), '_', '-');  // the reference accepts --aa_count etc. as aliases
        auto next = [&]() -> const char* {
            if (i + 1 >= argc) std::exit(usage());
            return argv[++i];
        };
        if (a == "--width") o.width = std::atoi(next());
        else if (a == "--height") o.height = std::atoi(next());
        else if (a == "--aa-count") o.aa = std::atoi(next());
        else if (a == "--render-depth") o.depth = std::atoi(next());
        else if (a == "--time") o.time = std::atof(next());
        else if (a == "--output") o.output = next();
        else if (a == "--device") o.device = std::atoi(next());
        else if (a == "--asset-root") o.asset_root = next();
        else if (a == "--stage") o.stage = next();
        else if (a == "--animation") o.animation = next();
        else if (a == "--camera") { o.camera = next(); o.have_camera = true; }
        else if (a == "--panini") o.panini = std::atof(next());
        else if (a == "--fov") o.fov = std::atof(next());
        else if (a == "--fps") o.fps = std::atoi(next());
        else if (a == "--motion-blur-frames") o.blur = std::atoi(next());
        else if (a == "--stereoimage" || a == "--stereo-image") o.stereo = true;
        else if (a == "--batch-subframes") o.batch = std::atoi(next());
        else if (a == "--no-skip-existing") o.skip_existing = false;
        else if (a == "--filter-starts-with" || a == "--starts-with") o.starts_with = next();
        else if (a == "--scenes-dir") o.scenes_dir = next();
        else if (a == "--out-dir") o.out_dir = next();
        else if (a == "--max-frames") o.max_frames = std::atoi(next());
        else if (a == "--specialize") o.specialize = std::atoi(next());
        else if (a == "--timing") o.timing = true;
        else if (a == "--frames") {
            std::string form = next();
            if (form != "png" && form != "y4m") return refuse("--frames png|y4m");
            o.y4m = form == "y4m";
        }
        else if (a == "--deep-colour") o.deep_colour = true;
        else if (a == "--chroma") {
            std::string sampling = next();
            if (sampling != "420" && sampling != "422" && sampling != "444") return refuse("--chroma 420|422|444");
            o.chroma = std::atoi(sampling.c_str());
            o.have_chroma = true;
        }
        else if (a == "--png-depth") {
            std::string depth = next();
            if (depth != "8" && depth != "16") return refuse("--png-depth 8|16");
            o.png_depth = std::atoi(depth.c_str());
            o.have_png_depth = true;
        }
        else if (a == "--png-encoder") {
            std::string encoder = next();
            if (encoder != "host" && encoder != "gpu") return refuse("--png-encoder host|gpu");
            o.png_gpu = encoder == "gpu";
            o.have_png_encoder = true;
        }
        else if (a == "--png-codes") {
            std::string codes = next();
            if (codes != "fixed" && codes != "dynamic") return refuse("--png-codes fixed|dynamic");
            o.png_codes = codes == "dynamic" ? PTL_PNG_CODES_DYNAMIC : PTL_PNG_CODES_FIXED;
            o.have_png_codes = true;
        }
        else if (a == "--png16-encoder") {
            std::string encoder = next();
            if (encoder != "host" && encoder != "gpu") return refuse("--png16-encoder host|gpu");
            o.png16_gpu = encoder == "gpu";
            o.have_png16_encoder = true;
        }
        else if (a == "--gpus") o.gpus = std::atoi(next());
        else if (a == "--devices") o.devices = next();
        else if (a == "--transport") o.transport = next();
        else if (a == "--multi-process") o.multi_process = true;
        else if (a == "--adaptive-aa") {
            o.adaptive = true;
            if (i + 1 < argc) {  // the threshold is optional: an integer right behind the switch is it ("-1" included)
                char* end = nullptr;
                const long t = std::strtol(argv[i + 1], &end, 10);
                if (end != argv[i + 1] && *end == '\0') {
                    ++i;
                    if (t < -1 || t > 255) return refuse("--adaptive-aa T: the threshold is an integer in -1 .. 255");
                    o.adaptive_t = (int)t;
                }
            }
        }
        else if (a == "--clip-adaptive-aa") {
            o.clip_adaptive = true;
            if (i + 1 < argc) {  // the optional threshold, as for --adaptive-aa
                char* end = nullptr;
                const long t = std::strtol(argv[i + 1], &end, 10);
                if (end != argv[i + 1] && *end == '\0') {
                    ++i;
                    if (t < -1 || t > 255) return refuse("--clip-adaptive-aa T: the threshold is an integer in -1 .. 255");
                    o.clip_adaptive_t = (int)t;
                }
            }
        }
        else if (a == "--passes") {
            const std::string list = next();
            for (const std::string& pass : split_list(list)) {
                if (pass == "depth") o.pass_depth = true;
                else if (pass == "trips") o.pass_trips = true;
                else if (pass == "cut") o.pass_cut = true;
                else {
                    std::fprintf(stderr, "--passes depth,trips,cut: unknown pass `%s`\n", pass.c_str());
                    return 2;
                }
            }
            if (!o.pass_depth && !o.pass_trips && !o.pass_cut) return refuse("--passes depth,trips,cut: name at least one pass");
            o.have_passes = true;
        }
        else if (a == "--clip-passes") {
            const std::string list = next();
            for (const std::string& pass : split_list(list)) {
                if (pass == "depth") o.clip_pass_depth = true;
                else if (pass == "trips") o.clip_pass_trips = true;
                else if (pass == "cut") o.clip_pass_cut = true;
                else {
                    std::fprintf(stderr, "--clip-passes depth,trips,cut: unknown pass `%s`\n", pass.c_str());
                    return 2;
                }
            }
            if (!o.clip_pass_depth && !o.clip_pass_trips && !o.clip_pass_cut) return refuse("--clip-passes depth,trips,cut: name at least one pass");
            o.have_clip_passes = true;
        }
        else if (a == "--pass-encoder") {
            std::string encoder = next();
            if (encoder != "host" && encoder != "gpu") return refuse("--pass-encoder host|gpu");
            o.pass_gpu = encoder == "gpu";
            o.have_pass_encoder = true;
        }
        else if (a == "--depth-report") o.depth_report = true;
        else if (a == "--fast") o.fast = true;
        else if (a == "--exact-cr") o.exact_cr = true;
        else if (a == "--opt3") o.opt3 = true;
        else if (a == "--rank") o.rank = std::atoi(next());
        else if (a == "--world") o.world = std::atoi(next());
        else if (a == "--ipc-handle") o.ipc_handle = next();
        else if (a == "--set") {
            std::string kv = next();
            size_t eq = kv.find('=');
            if (eq == std::string::npos) return refuse("--set name=value");
            o.sets.emplace_back(kv.substr(0, eq), std::atof(kv.c_str() + eq + 1));
        }
        else if (a == "--shard") {
            if (std::sscanf(next(), "%d/%d", &o.shard, &o.shards) != 2 || o.shards < 1 || o.shard < 0 || o.shard >= o.shards) return refuse("--shard K/N with 0 <= K < N");
        } else if (cmd == "render" && a.rfind("--", 0) != 0 && o.clips.empty()) o.clips = argv[i];
        else {
            std::fprintf(stderr, "unknown option %s\n", argv[i]);
            return 2;
        }
    }
    if (!o.stage.empty() && !o.animation.empty()) return refuse("--stage and --animation exclude each other");
    if (o.blur < 1 || o.blur > 256) return refuse("--motion-blur-frames must be 1..256");
    if (o.y4m && o.shards > 1) return refuse("--frames y4m cannot be combined with --shard K/N, N > 1: a stream needs every frame, in order");
    if (o.deep_colour && cmd != "render") return refuse("--deep-colour is an option of render: it chooses how the frames of a clip's Y4M stream are made");
    if (o.deep_colour && !o.y4m) return refuse("--deep-colour needs --frames y4m: PNG frames hold 8 bits per channel, only the 10-bit stream can carry what the float sub-frames add");
    if (o.have_chroma && cmd != "render") return refuse("--chroma is an option of render: it chooses the chroma sampling of a clip's Y4M stream");
    if (o.have_chroma && !o.y4m) return refuse("--chroma needs --frames y4m: it chooses the chroma sampling of the stream (4:2:0, 4:2:2 or 4:4:4); PNG frames have none");
    if (o.have_png_depth && cmd != "render" && cmd != "render-frame") return refuse("--png-depth is an option of render and render-frame: it chooses the bit depth of the PNG frames of a clip, or of the one frame");
    if (o.png_depth == 16 && o.y4m) return refuse("--png-depth 16 cannot be combined with --frames y4m: a stream holds no PNG frames (its deep-colour form is --deep-colour)");
    if (o.png_depth == 16 && cmd == "render-frame" && (o.gpus > 1 || split_list(o.devices).size() > 1 || o.multi_process || o.shards > 1 || o.transport == "rccl"))
        return refuse("render-frame --png-depth 16 draws the frame on one GPU: frame groups gather RGBA8, so it cannot be combined with --gpus N, N > 1, several --devices, --multi-process, --transport rccl or --shard");
    if (o.have_png16_encoder && cmd != "render" && cmd != "render-frame") return refuse("--png16-encoder is an option of render and render-frame: it chooses who deflates the 16-bit PNG frames of a clip, or the one frame");
    if (o.have_png16_encoder && o.png_depth != 16) return refuse("--png16-encoder needs --png-depth 16: it chooses who deflates the 16-bit frames (the encoder of 8-bit frames is --png-encoder)");
    if (o.png16_gpu && ptl_png_stream16_bytes(o.stereo ? 2 * o.width : o.width, o.height) == 0)
        return refuse("--png16-encoder gpu needs a frame of at most 2^28 pixels whose scanlines, H (6 W + 1) bytes, number at most 2^31: the kernels address them with 32-bit offsets");
    if (o.have_png_encoder && cmd != "render" && cmd != "render-frame") return refuse("--png-encoder is an option of render and render-frame: it chooses who deflates the PNG frames of a clip, or the one frame");
    if (o.have_png_codes && cmd != "render" && cmd != "render-frame") return refuse("--png-codes is an option of render and render-frame: it chooses the Huffman codes of the streams the gpu PNG encoder makes");
    if (o.have_png_codes && !o.png_gpu) return refuse("--png-codes needs --png-encoder gpu: it chooses the Huffman codes of the deflate streams made on the GPU; the host encoder is zlib");
    if (o.png_gpu && o.y4m) return refuse("--png-encoder gpu cannot be combined with --frames y4m: a stream holds no PNG frames");
    if (o.png_gpu && o.png_depth == 16) return refuse("--png-encoder gpu cannot be combined with --png-depth 16: the GPU deflates 8-bit frames only (runs at distance 1 do not catch the 16-bit rows)");
    if (o.png_gpu && cmd == "render-frame" && (o.gpus > 1 || split_list(o.devices).size() > 1 || o.multi_process || o.shards > 1 || o.transport == "rccl"))
        return refuse("render-frame --png-encoder gpu deflates the frame on the one GPU that drew it: it cannot be combined with --gpus N, N > 1, several --devices, --multi-process, --transport rccl or --shard");
    if (o.png_gpu && ptl_png_stream_bytes(o.stereo ? 2 * o.width : o.width, o.height) == 0)
        return refuse("--png-encoder gpu needs a frame whose scanlines, H (4 W + 1) bytes, number at most 2^31: the kernels address them with 32-bit offsets");
    if (o.adaptive && cmd != "render-frame") return refuse("--adaptive-aa is an option of render-frame: a clip's sub-frames go through the slices entry, whose adaptive form is `render --clip-adaptive-aa [T]`");
    if (o.clip_adaptive && cmd != "render" && cmd != "precompile") return refuse("--clip-adaptive-aa is an option of render (and of precompile, which builds render's kernels); a single frame takes render-frame --adaptive-aa");
    if (o.adaptive && (o.gpus > 1 || split_list(o.devices).size() > 1 || o.shards > 1)) return refuse("--adaptive-aa draws whole frames on one GPU: it cannot be combined with --gpus N, N > 1, several --devices or --shard");
    if (o.have_passes && cmd != "render-frame") return refuse("--passes is an option of render-frame: a clip writes no pass images per frame (render --depth-report gives a clip's line)");
    if (o.depth_report && cmd != "render" && cmd != "render-frame") return refuse("--depth-report is an option of render and render-frame");
    if ((o.have_passes || o.depth_report) && (o.adaptive || o.clip_adaptive))
        return refuse("--passes and --depth-report cannot be combined with --adaptive-aa / --clip-adaptive-aa: the list-driven refine entry stores no pass records");
    if ((o.have_passes || o.depth_report) && (o.gpus > 1 || split_list(o.devices).size() > 1 || o.multi_process || o.shards > 1 || o.transport == "rccl"))
        return refuse("--passes and --depth-report draw on one GPU: they cannot be combined with --gpus N, N > 1, several --devices, --multi-process, --transport rccl or --shard");
    if (o.have_clip_passes && cmd != "render") return refuse("--clip-passes is an option of render: it writes pass images beside every frame of a clip (one frame takes render-frame --passes)");
    if (o.have_clip_passes && (o.adaptive || o.clip_adaptive))
        return refuse("--clip-passes cannot be combined with --adaptive-aa / --clip-adaptive-aa: the list-driven refine entry stores no pass records");
    if (o.have_clip_passes && (o.gpus > 1 || split_list(o.devices).size() > 1))
        return refuse("--clip-passes draws a clip on one GPU: it cannot be combined with --gpus N, N > 1, or several --devices (--shard K/N splits a clip)");
    if (o.have_pass_encoder && !o.have_clip_passes) return refuse("--pass-encoder needs --clip-passes: it chooses who deflates the pass images of a clip's frames");
    if (o.pass_gpu && (o.stereo ? 2 * o.width : o.width) % 3 != 0)
        return refuse("--pass-encoder gpu needs a drawn width that is a multiple of 3: the GPU deflates a grey row of W samples as W / 3 RGB pixels (matches at distance 6)");
    if (o.pass_gpu && ptl_png_stream16_bytes((o.stereo ? 2 * o.width : o.width) / 3, o.height) == 0)
        return refuse("--pass-encoder gpu needs a frame whose pass image has at most 2^31 bytes of scanlines: the kernels address them with 32-bit offsets");
    if (cmd == "render") return render(o);
    if (o.transport != "stores" && o.transport != "copy" && o.transport != "rccl") return refuse("--transport stores|copy|rccl");
    if (cmd == "render-frame") return render_frame(o);
    if (cmd == "render-shard") return render_shard(o);
    if (cmd == "precompile") return precompile(o);
    if (cmd == "check") return check(o);
    if (cmd == "write") return write_scene(o);
    return emit_source(o);
}
