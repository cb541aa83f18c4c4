// cli_video.cpp -- `portal-amd render <scenes> [clips]`, the offline counterpart of the reference's `portal render` (src/main.rs:2757-2874 +
// render_animation src/main.rs:1758-1873).  What is here: what the clip loop keeps in flight (FramePipeline), the pass images of a clip (PassImages), the
// forms a clip's frames leave in (FrameOutput: PNG files for ffmpeg in one of the forms of cli_png.h, or one Y4M stream made from the RGBA8 or from the float sub-frames), what lives as long as a scene's clips (SceneRun)
// and as long as one clip (ClipRun), the sub-frame draws (SubframeDraws), the clip loop (trace_clip, render_clip), the workers that compile the next clips' kernels (Prefetcher) and `render`.
// Argument parsing and every other command are in cli.cpp; what both share is in cli_common.h and cli_png.h; the encoder pool, the page-locked
// buffers, child processes and the Y4M stream are in cli_host.h.
//
// Video pipeline: for every frame i of a clip, `motion_blur_frames` sub-frames are traced straight into device buffers (aa_start = j,
// time = subframe_time(i, j)), averaged on the GPU (ptl_average_images), downloaded once, and PNG-encoded on a pool of host threads while
// the GPU already traces the next frame.  With --frames y4m the averaging kernel is the fused one (ptl_average_to_yuv420p10): what is
// downloaded is the planar 10-bit frame the encoder consumes (4:2:0, or what --chroma asks for: ptl_average_to_yuv10), and one writer thread streams the frames in order into ffmpeg's stdin
// (or a .y4m file) while the clip is still rendering: no PNG files, no anim/ directory, no zscale pass.
// With --clip-passes every frame also gets up to three 16-bit grey pass images (PassImages: anim/depth_<i>.png, trips_<i>.png, cut_<i>.png), merged on
// the GPU from the pass records of its sub-frames (ptl_pass_slices_to_gray16), downloaded with the frame and encoded by the same pool.
#include <signal.h>

#include <algorithm>
#include <cstdlib>
#include <stop_token>

#include "cli_host.h"
#include "cli_png.h"

namespace {

bool exists(const std::string& path) {
    struct stat st;
    return ::stat(path.c_str(), &st) == 0;
}

// The reference compiles its scene list in (src/gui/scenes.rs); here a scene is a path, or a bare name under --scenes-dir.
std::string scene_file(const std::string& arg, const std::string& scenes_dir) {
    bool looks_like_a_path = arg.find('/') != std::string::npos || (arg.size() > 4 && arg.compare(arg.size() - 4, 4, ".ron") == 0);
    if (exists(arg) || looks_like_a_path) return arg;
    return scenes_dir + "/" + arg + ".ron";
}

std::string scene_link(const std::string& path) {  // "dir/name.ron" -> "name"
    size_t slash = path.rfind('/');
    std::string base = slash == std::string::npos ? path : path.substr(slash + 1);
    return base.size() > 4 && base.substr(base.size() - 4) == ".ron" ? base.substr(0, base.size() - 4) : base;
}

// frames of a clip are intermediates (ffmpeg reads them, then anim/ is removed): fast deflate, 2.3x the encode rate of level 6
constexpr int kFrameDeflateLevel = 3;

// the reference's encoder settings (src/main.rs:1843-1857), from -c:v onwards: what follows the input, whichever form the input has.
// `pix_fmt`: the reference's yuv420p10le, or what --chroma makes of the stream
std::vector<std::string> encoder_arguments(const std::string& video, const std::string& pix_fmt) {
    return {"-c:v", "libx265", "-pix_fmt", pix_fmt, "-crf", "15", "-preset", "slow", "-x265-params",
            "colorprim=bt709:transfer=iec61966-2-1:colormatrix=bt709:range=full", "-colorspace", "bt709", "-color_primaries", "bt709", "-color_trc",
            "iec61966-2-1", "-color_range", "pc", "-movflags", "+write_colr+faststart", "-tag:v", "hvc1", "-y", video};
}

// the reference's ffmpeg hand-off (src/main.rs:1829-1869), same arguments; frames are kept when there is no ffmpeg
int encode_video(const Options& o, const std::string& scene_name, const std::string& clip, int fps) {
    std::string anim = o.out_dir + "/anim", video = o.out_dir + "/video/" + scene_name + "/" + clip + ".mov";
    if (run_program({"ffmpeg", "-version"}, true) != 0) {
        // no encoder on this machine: park the clip's frames next to where the video would be, so the next clip starts
        // from an empty anim/ (the reference removes anim/ after ffmpeg; frame_%d.png of another clip would be "existing")
        std::string frames = o.out_dir + "/video/" + scene_name + "/" + clip + ".frames";
        remove_tree(frames);
        if (::rename(anim.c_str(), frames.c_str()) != 0) std::fprintf(stderr, "could not move anim/ to %s\n", frames.c_str());
        std::printf("ffmpeg not found: frames kept in `%s` (ffmpeg -framerate %d -i frame_%%d.png ... ../%s.mov)\n", frames.c_str(), fps, clip.c_str());
        return 0;
    }
    std::printf("Start ffmpeg to render video\n");
    auto started = std::chrono::steady_clock::now();
    std::vector<std::string> command = {
        "ffmpeg", "-framerate", std::to_string(fps), "-i", anim + "/frame_%d.png", "-vf",
        "zscale=primariesin=bt709:transferin=iec61966-2-1:matrixin=bt709:rangein=full:primaries=bt709:transfer=iec61966-2-1:matrix=bt709:range=full,"
        "format=yuv420p10le"};
    for (const std::string& a : encoder_arguments(video, "yuv420p10le")) command.push_back(a);
    int status = run_program(command, true);
    std::printf("ffmpeg status: %d\nffmpeg time: %.2f s\n", status, std::chrono::duration<double>(std::chrono::steady_clock::now() - started).count());
    remove_tree(anim);  // like the reference, whatever ffmpeg said (src/main.rs:1860)
    return 0;
}

// What the clip loop keeps in flight: the download of frame i runs on its own stream into page-locked memory while frame i+1
// is being traced; `kRing` result buffers so a frame is not overwritten before its copy has left.
struct FramePipeline {
    static constexpr int kRing = 3;
    int device = 0;
    void* copy_stream = nullptr;
    void* results[kRing] = {nullptr, nullptr, nullptr};   // device RGBA8 frames ready for download
    void* copied[kRing] = {nullptr, nullptr, nullptr};    // event: the copy out of results[k] has finished
    bool copy_pending[kRing] = {false, false, false};
    void* produced = nullptr;                             // event: results[k] is complete on the tracing stream

    bool create(int dev, size_t bytes) {
        device = dev;
        if (ptl_stream_create(dev, &copy_stream) != PTL_OK || ptl_event_create(dev, &produced) != PTL_OK) return false;
        for (int k = 0; k < kRing; ++k)
            if (ptl_device_alloc(dev, bytes, &results[k]) != PTL_OK || ptl_event_create(dev, &copied[k]) != PTL_OK) return false;
        return true;
    }
    // Hand results[k], complete on the tracing stream, to the copy stream and go on tracing: `bytes` of it into `pixels` (page-locked).  The host job
    // waits for `arrived`, an event of its own to destroy.  0, or 1 after "download: <error>"
    int hand_off(int k, uint8_t* pixels, size_t bytes, void** arrived) {
        if (ptl_event_record(produced, nullptr) != PTL_OK || ptl_stream_wait_event(copy_stream, produced) != PTL_OK ||
            ptl_device_download_async(pixels, results[k], bytes, copy_stream) != PTL_OK || ptl_event_create(device, arrived) != PTL_OK || ptl_event_record(*arrived, copy_stream) != PTL_OK)
            return fail("download");
        return 0;
    }
    int slot_left(int k) {  // slot k is free once what the copy stream holds now is done: the frame and its pass images have left
        if (ptl_event_record(copied[k], copy_stream) != PTL_OK) return fail("download");
        copy_pending[k] = true;
        return 0;
    }
    ~FramePipeline() {
        if (copy_stream) ptl_stream_destroy(copy_stream);
        if (produced) ptl_event_destroy(produced);
        for (int k = 0; k < kRing; ++k) {
            if (copied[k]) ptl_event_destroy(copied[k]);
            if (results[k]) ptl_device_free(results[k]);
        }
    }
};

// --clip-passes: the pass images of a scene's clips -- which of them a frame gets, the buffers they travel in, the files they become.
// ptl_pass_slices_to_gray16 writes the images asked for one behind the other as planes of 16-bit rows (each 16-byte aligned) in one sweep.
// --pass-encoder host: the planes are what leaves the card (one copy) and an encoder thread deflates each (ptl_png_write_gray16).
// --pass-encoder gpu: every plane goes through ptl_png_deflate_rgb48 as rows of W / 3 RGB pixels -- byte for byte the same rows -- into a result
// buffer of its own; what leaves the card is each buffer's header and stream, and an encoder thread only frames it (ptl_png_write_stream_gray16).
// On the card: a ring like FramePipeline::results (slot k is free when FramePipeline::copied[k] has happened: the images are copied out in front
// of that event) and, for the gpu encoder, the sweep's planes.  On the host: page-locked buffers of their own, new for every clip.
class PassImages {
public:
    static constexpr int kCount = 3;
    PassImages(const Options& o, int width, int height)
        : on(o.have_clip_passes),
          device_(o.device),
          width_(width),
          height_(height),
          timing_(o.timing),
          want_{o.clip_pass_depth, o.clip_pass_trips, o.clip_pass_cut},
          gpu_(o.pass_gpu),
          plane_bytes_(((size_t)2 * width * height + 15) & ~(size_t)15),
          device_stride_(gpu_ ? (ptl_png_stream16_bytes(width / 3, height) + 255) & ~(size_t)255 : plane_bytes_),
          download_bytes_(gpu_ ? ptl_png_stream16_download_bytes(width / 3, height) : plane_bytes_),
          host_stride_((download_bytes_ + 15) & ~(size_t)15),
          anim_dir_(o.out_dir + "/anim") {}
    const bool on;  // the option was given: nothing below is called without it
    int allocate() {  // the ring and the planes, once per scene.  0, or 1 after "alloc: <error>"
        for (DevicePtr& slot : results_)
            if (!(slot = device_alloc(device_, device_stride_ * (size_t)count(), "alloc"))) return 1;
        if (gpu_ && !(planes_ = device_alloc(device_, plane_bytes_ * (size_t)count(), "alloc"))) return 1;
        return 0;
    }
    bool open_clip(int in_flight) {  // the page-locked buffers of one clip (the last clip's encoders have finished with theirs)
        pinned_ = std::make_unique<PinnedFrames>(std::max<size_t>(16, host_stride_ * (size_t)count()), in_flight);
        return pinned_->ok();
    }
    const std::string& anim_dir() const { return anim_dir_; }
    bool have(int i) const {  // every image asked for is there
        for (int p = 0; p < kCount; ++p)
            if (want_[p] && !exists(file(p, i))) return false;
        return true;
    }
    // Behind a frame's last sub-frame on the tracing stream, before the next frame overwrites `records` (ALL `blur` sub-frames of the frame, slice j
    // where the batched launch puts it): one sweep merges them into the frame's images, in ring slot `slot`.  `gpu_ms`: + theirs, under --timing
    int make(ptl_renderer* r, const void* records, int blur, int slot, double* gpu_ms) {
        float lo[16] = {0.0f}, hi[16] = {1.0f}, ms = 0.0f;  // the scene's depth-map bounds, as the last sub-frame's draw uploaded them
        ptl_renderer_uniform_value(r, width_, height_, "_depth_map_min", lo, nullptr);
        ptl_renderer_uniform_value(r, width_, height_, "_depth_map_max", hi, nullptr);
        const long n_px = (long)width_ * height_;
        char* results = static_cast<char*>(results_[slot].get());
        char* planes = gpu_ ? static_cast<char*>(planes_.get()) : results;
        auto plane = [&](int p) -> void* { return want_[p] ? planes + index(p) * plane_bytes_ : nullptr; };
        if (ptl_pass_slices_to_gray16(device_, records, blur, (unsigned long long)n_px, n_px, plane(0), plane(1), plane(2), lo[0], hi[0], nullptr, timing_ ? &ms : nullptr) != PTL_OK)
            return fail("pass_slices_to_gray16");
        *gpu_ms += ms;
        for (int p = 0; p < kCount && gpu_; ++p) {  // the plane's rows as W / 3 RGB pixels: the same bytes, the filter-type bytes in the same places
            if (!want_[p]) continue;
            if (ptl_png_deflate_rgb48(device_, plane(p), width_ / 3, height_, PTL_PNG_CODES_DYNAMIC, results + index(p) * device_stride_, nullptr, timing_ ? &ms : nullptr) != PTL_OK)
                return fail("png_deflate_rgb48");
            *gpu_ms += ms;
        }
        return 0;
    }
    // On the copy stream, behind the frame's own copy and in front of the event that frees the slot.  host: the planes in one copy; gpu: of every
    // result buffer the header and the room for the stream
    int copy_out(int slot, void* copy_stream) {
        pixels_ = pinned_->take();
        const char* results = static_cast<const char*>(results_[slot].get());
        for (int k = 0; k < (gpu_ ? count() : 1); ++k)
            if (ptl_device_download_async(pixels_ + (size_t)k * host_stride_, results + (size_t)k * device_stride_, gpu_ ? download_bytes_ : plane_bytes_ * (size_t)count(), copy_stream) != PTL_OK)
                return fail("download");
        if (ptl_event_create(device_, &arrived_) != PTL_OK || ptl_event_record(arrived_, copy_stream) != PTL_OK) return fail("download");
        return 0;
    }
    void submit(int i, EncoderPool& pool) {  // the images copy_out() sent on their way become frame i's files
        pool.submit([this, i, pixels = pixels_, arrived = arrived_, &pinned = *pinned_] {
            bool ok = ptl_event_synchronize(arrived) == PTL_OK;
            for (int p = 0; p < kCount && ok; ++p)
                if (want_[p]) {
                    const uint8_t* image = pixels + index(p) * host_stride_;
                    ok = (gpu_ ? ptl_png_write_stream_gray16(file(p, i).c_str(), image, width_, height_) : ptl_png_write_gray16(file(p, i).c_str(), image, width_, height_, kFrameDeflateLevel)) == PTL_OK;
                }
            if (!ok) std::fprintf(stderr, "\n%s\n", ptl_last_error());
            ptl_event_destroy(arrived);
            pinned.give(pixels);
        });
    }
    // A clip that is whole: its pass files leave anim/ for `parked` (video/<scene>/<clip>.passes) before the frames are handed on -- anim/ is
    // removed behind ffmpeg (or parked as <clip>.frames without one), and the next clip must not find this clip's pass files "already there"
    void park(const std::string& parked, const std::string& clip) const {
        std::vector<std::string> names;
        if (DIR* d = opendir(anim_dir_.c_str())) {
            while (dirent* e = readdir(d)) {
                const std::string name = e->d_name;
                for (int p = 0; p < kCount; ++p)
                    if (name.rfind(std::string(pass_name(p)) + "_", 0) == 0) names.push_back(name);
            }
            closedir(d);
        }
        if (names.empty()) return;
        remove_tree(parked);
        make_dirs(parked);
        for (const std::string& name : names)
            if (::rename((anim_dir_ + "/" + name).c_str(), (parked + "/" + name).c_str()) != 0) std::fprintf(stderr, "could not move %s to %s\n", name.c_str(), parked.c_str());
        std::printf("Pass images of `%s` are in `%s`\n", clip.c_str(), parked.c_str());
    }

private:
    int count() const { return (int)want_[0] + (int)want_[1] + (int)want_[2]; }
    size_t index(int p) const { return (size_t)std::count(want_, want_ + p, true); }  // of image p among those asked for
    static const char* pass_name(int p) { return p == 0 ? "depth" : p == 1 ? "trips" : "cut"; }
    std::string file(int p, int i) const { return anim_dir_ + "/" + pass_name(p) + "_" + std::to_string(i) + ".png"; }  // (ffmpeg is given anim/frame_%d.png: no collision)
    const int device_, width_, height_;
    const bool timing_;
    const bool want_[kCount];
    const bool gpu_;
    // a plane the sweep writes; a ring slot's share per image (the plane, or the result buffer of its deflate); what of that leaves the card; its share of a page-locked buffer
    const size_t plane_bytes_, device_stride_, download_bytes_, host_stride_;
    const std::string anim_dir_;
    DevicePtr results_[FramePipeline::kRing], planes_;
    std::unique_ptr<PinnedFrames> pinned_;
    uint8_t* pixels_ = nullptr;  // between copy_out() and submit(): the frame's images on their way, and the event behind their copies
    void* arrived_ = nullptr;
};

// One clip of the run
struct Clip {
    std::string name;
    double duration;
    int fps = 0;              // --fps, or the clip's own (kClipOverrides)
    bool specialise = false;  // it gets a clip-constant kernel: that repays its extra JIT (~1 s) only on a clip with enough work
};

// What lives as long as a scene's clips.  Released in reverse order: the pipeline, the sub-frame blocks, the renderer, the scene.
struct SceneRun {
    SceneRun(const Options& o, std::string name) : o(o), name(std::move(name)) {}
    const Options& o;
    const std::string name;                                   // video/<name>/<clip>
    const int width = o.stereo ? o.width * 2 : o.width;      // src/main.rs:2822-2829
    const int height = o.height;
    const int threads = (int)std::min(64u, std::max(2u, std::thread::hardware_concurrency() * 3 / 4));  // PNG encoders
    const size_t frame_bytes = (size_t)width * height * 4;   // an RGBA8 frame: a sub-frame, a still
    size_t result_bytes = 0;                                  // a frame's result buffer on the card
    size_t download_bytes = 0;                                // what of it leaves the card
    ScenePtr scene;
    RendererPtr r;
    DevicePtr subframe_block;  // ONE allocation, sub-frame j at j * bytes: what the one-launch form writes (slice z behind slice z - 1)
    std::vector<void*> subframes;
    DevicePtr float_block;  // --deep-colour and --png-depth 16 only: the same sub-frames as RGBA32F (16 bytes per pixel), one allocation, laid out the same way
    std::vector<void*> float_subframes;             // (empty without the option)
    // --depth-report only: the sub-frames' pass records (16 bytes per pixel, laid out the same way), and what a clip accumulates from them on the
    // card: one statistics block and a counter per frame (ptl_pass_stats), downloaded once at the end of the clip
    DevicePtr record_block, pass_stats;
    PassImages passes{o, width, height};  // --clip-passes only: the record block is kept for the images as well
    FramePipeline pipe;
};

// ---- the forms a clip's frames leave in ------------------------------------------------------
// One object per clip.  It alone knows how the clip opens, whether a frame is already there, where a sub-frame is drawn and which kernel
// makes the result of them, how many bytes leave the card, what the host does with a downloaded frame, and how the clip ends.
class FrameOutput {
public:
    FrameOutput(const SceneRun& run, const Clip& clip)
        : video_base(run.o.out_dir + "/video/" + run.name + "/" + clip.name), run_(run), o_(run.o), clip_(clip.name), fps_(clip.fps) {}
    virtual ~FrameOutput() = default;
    virtual size_t result_bytes() const = 0;  // one frame's result buffer on the card
    virtual size_t download_bytes() const { return result_bytes(); }  // what of it leaves the card: the page-locked buffers and the copy
    virtual int open() = 0;                   // 0, or the exit status
    virtual int check() { return 0; }         // before every frame: 0 while frames can still leave, else the exit status (reported)
    virtual bool have(int i) const = 0;       // frame i is already there: it is not drawn again
    virtual bool wants_float() const { return false; }  // the sub-frames are also drawn as RGBA32F (run.float_subframes): make_result() reads those
    virtual bool draws_result() const = 0;    // a frame of ONE sub-frame that needs no kernel is drawn where the result is expected, make_result() not called
    virtual int make_result(void* result, float* ms) = 0;  // the kernel that turns the --motion-blur-frames sub-frames into the result
    // the host's part: `pixels` (page-locked, to give back) hold frame i once `arrived` (an event, to destroy) has happened
    virtual void submit(int i, uint8_t* pixels, void* arrived, EncoderPool& pool, PinnedFrames& pinned) = 0;
    // every frame that was submitted is where it goes, and what follows a clip that is whole; `rc`: what the clip loop returned
    virtual int close(int rc, EncoderPool& pool, std::chrono::steady_clock::time_point clip_start) = 0;
    const std::string video_base;

protected:
    void report_on_disk(std::chrono::steady_clock::time_point clip_start) const { std::printf("Clip `%s` on disk after %.2f s\n", clip_.c_str(), seconds_since(clip_start)); }
    const SceneRun& run_;
    const Options& o_;
    const std::string clip_;
    const int fps_;
};

// anim/frame_<i>.png, encoded in any order by the pool; then ffmpeg reads them (encode_video).  How the sub-frames become a file -- 8 or 16 bits,
// deflated by an encoder thread or on the card -- is the form's (cli_png.h); names, have(), shards, resume, stills and encode_video are the same
// for all.  The RGBA8 sub-frames are drawn in every form: the stills come from them, and the classification of --clip-adaptive-aa reads them.
class PngOutput : public FrameOutput {
public:
    using FrameOutput::FrameOutput;
    size_t result_bytes() const override { return form_.result_bytes(run_.width, run_.height); }
    size_t download_bytes() const override { return form_.download_bytes(run_.width, run_.height); }
    int open() override {
        make_dirs(anim_dir_);
        const size_t staging_bytes = form_.staging_bytes(run_.width, run_.height, o_.blur);
        if (staging_bytes != 0 && !(staging_ = device_alloc(o_.device, staging_bytes, "alloc"))) return 1;
        return 0;
    }
    bool have(int i) const override { return exists(frame_name(i)); }
    bool wants_float() const override { return form_.wants_float(); }
    bool draws_result() const override { return form_.draws_result(o_.blur); }
    int make_result(void* result, float* ms) override {
        float average_ms = 0.0f, deflate_ms = 0.0f;
        const int rc = form_.make(o_.device, run_.subframes.data(), run_.float_subframes.data(), o_.blur, staging_.get(), result, run_.width, run_.height, ms ? &average_ms : nullptr,
                                  ms ? &deflate_ms : nullptr);
        if (ms) *ms = average_ms + deflate_ms;
        return rc;
    }
    void submit(int i, uint8_t* pixels, void* arrived, EncoderPool& pool, PinnedFrames& pinned) override {
        pool.submit([form = form_, pixels, name = frame_name(i), width = run_.width, height = run_.height, arrived, &pinned] {
            if (ptl_event_synchronize(arrived) != PTL_OK || form.write(name.c_str(), pixels, width, height, kFrameDeflateLevel) != PTL_OK) std::fprintf(stderr, "\n%s\n", ptl_last_error());
            ptl_event_destroy(arrived);
            pinned.give(pixels);
        });
    }
    int close(int rc, EncoderPool& pool, std::chrono::steady_clock::time_point clip_start) override {
        pool.finish();  // joins the encoders: every frame file is on disk (and every pinned buffer is back)
        if (rc != 0) return rc;
        report_on_disk(clip_start);
        if (o_.shards == 1 && o_.max_frames < 0) encode_video(o_, run_.name, clip_, fps_);
        return 0;
    }

private:
    std::string frame_name(int i) const { return anim_dir_ + "/frame_" + std::to_string(i) + ".png"; }
    const std::string anim_dir_ = o_.out_dir + "/anim";
    const PngForm form_{o_};
    DevicePtr staging_;  // the form's staging buffer on the card (none for the host forms)
};

// One Y4M stream, written in frame order by a thread of its own.  (A stream is not resumed: it holds every frame, from frame 0.)
class Y4mOutput : public FrameOutput {
public:
    Y4mOutput(const SceneRun& run, const Clip& clip, size_t max_pending) : FrameOutput(run, clip), writer_(1, max_pending) {}
    size_t result_bytes() const override { return ptl_yuv10_frame_bytes(run_.width, run_.height, o_.chroma); }
    int open() override {
        ::signal(SIGPIPE, SIG_IGN);  // an encoder that dies is a failed write (EPIPE), reported by the clip
        // Where the stream goes: into an encoder when there is one and the clip is whole, else into a file an encoder can read later.
        // The encoder is told nothing about scaling or pixel formats: the stream is what it encodes, the -color_* tags say what it is.
        char header[128];
        int header_len = ptl_y4m_header_chroma(run_.width, run_.height, fps_, o_.chroma, header, sizeof header);
        if (header_len < 0) return fail("y4m header");
        std::vector<std::string> encode = {"ffmpeg", "-f", "yuv4mpegpipe", "-i", "-"};
        for (const std::string& a : encoder_arguments(video_base + ".mov", "yuv" + std::to_string(o_.chroma) + "p10le")) encode.push_back(a);
        if (o_.max_frames < 0 && o_.shards == 1 && run_program({"ffmpeg", "-version"}, true) == 0) {
            std::printf("Start ffmpeg to encode the frames as they arrive\n");
            stream_.open_program(encode);
        } else {
            std::string command;
            for (const std::string& a : encode) command += (command.empty() ? "" : " ") + (a == "-" ? clip_ + ".y4m" : a);
            std::printf("Frames go to `%s.y4m` (%s)\n", video_base.c_str(), command.c_str());
            stream_.open_file(video_base + ".y4m");
        }
        stream_.write(header, (size_t)header_len);
        return 0;
    }
    int check() override {
        if (stream_.failed()) std::fprintf(stderr, "\n%s\n", stream_.error().c_str());
        return stream_.failed();
    }
    bool have(int) const override { return false; }
    bool draws_result() const override { return false; }  // (one sub-frame is converted with n = 1)
    int make_result(void* result, float* ms) override {
        return ptl_average_to_yuv10(o_.device, run_.subframes.data(), o_.blur, result, run_.width, run_.height, o_.chroma, nullptr, ms) == PTL_OK ? 0 : fail("average_to_yuv10");
    }
    void submit(int, uint8_t* pixels, void* arrived, EncoderPool&, PinnedFrames& pinned) override {  // frames of a stream arrive in order: one writer thread, jobs in submission order
        writer_.submit([this, pixels, arrived, bytes = result_bytes(), &pinned] {
            if (ptl_event_synchronize(arrived) != PTL_OK) stream_.fail(ptl_last_error());
            stream_.write("FRAME\n", 6);
            stream_.write(pixels, bytes);
            ptl_event_destroy(arrived);
            pinned.give(pixels);
        });
    }
    int close(int rc, EncoderPool& pool, std::chrono::steady_clock::time_point clip_start) override {
        writer_.finish();  // the stream has every frame that was submitted
        pool.finish();     // the stills are on disk
        const bool to_program = stream_.to_program();
        const int status = stream_.close();  // end of stream: an encoder finishes the video now
        if (to_program) std::printf("ffmpeg status: %d\nffmpeg time: %.2f s\n", status, stream_.seconds());
        if (rc == 0 && stream_.failed()) {
            std::fprintf(stderr, "%s\n", stream_.error().c_str());
            rc = 1;
        }
        if (rc == 0 && status != 0) {
            std::fprintf(stderr, "the encoder of clip `%s` failed (status %d)\n", clip_.c_str(), status);
            rc = 1;
        }
        if (rc == 0) report_on_disk(clip_start);
        return rc;
    }

private:
    Y4mStream stream_;
    EncoderPool writer_;  // (declared behind the stream: it finishes before the stream closes)
};

// The same stream with frames made from the float sub-frames (--deep-colour): quantised once, to 16 bits, instead of twice to 8 bits.  The RGBA8
// sub-frames are still drawn: the stills come from them, and the classification of --clip-adaptive-aa reads them.
class DeepY4mOutput : public Y4mOutput {
public:
    using Y4mOutput::Y4mOutput;
    bool wants_float() const override { return true; }
    int make_result(void* result, float* ms) override {
        return ptl_average_f32_to_yuv10(o_.device, run_.float_subframes.data(), o_.blur, result, run_.width, run_.height, o_.chroma, nullptr, ms) == PTL_OK ? 0 : fail("average_f32_to_yuv10");
    }
};

std::unique_ptr<FrameOutput> make_output(const SceneRun& run, const Clip& clip, size_t max_pending) {  // the ONE place that knows there are three
    if (run.o.y4m && run.o.deep_colour) return std::make_unique<DeepY4mOutput>(run, clip, max_pending);
    if (run.o.y4m) return std::make_unique<Y4mOutput>(run, clip, max_pending);
    return std::make_unique<PngOutput>(run, clip);
}

// What lives as long as a clip.  Released in reverse order: the output (its writer finishes, its stream closes), the pool, the page-locked buffers.
struct ClipRun {
    PinnedFrames pinned;
    EncoderPool pool;
    std::unique_ptr<FrameOutput> out;
};

// where in the clip (0 .. 1) sub-frame j of frame i is: the shutter is open for half a frame.  Skipped and drawn frames step the camera
// through the same times: a shard, or a resumed run, depends on it
double subframe_time(int i, int j, int count, int blur) {
    const double exposure = 0.5;
    return ((double)i / count) + (double)j / blur / count * exposure;
}

// One of the clip's .start.png / .end.png stills: an RGBA8 sub-frame, through the clip's pool and, where one fits, its page-locked buffers
// (they hold frames as they leave the card; a 4:2:0 one is smaller than an RGBA8 one: the two stills of such a clip take pageable memory)
int write_still(const SceneRun& run, ClipRun& c, const void* device_frame, const std::string& name) {
    uint8_t* pinned = run.frame_bytes <= run.download_bytes ? c.pinned.take() : nullptr;
    auto pageable = std::make_shared<std::vector<uint8_t>>(pinned ? 0 : run.frame_bytes);
    uint8_t* still = pinned ? pinned : pageable->data();
    if (ptl_device_download(still, device_frame, run.frame_bytes, nullptr) != PTL_OK) return fail("download");
    c.pool.submit([still, pinned, pageable, name, width = run.width, height = run.height, &frames = c.pinned] {
        if (ptl_png_write(name.c_str(), still, width, height) != PTL_OK) std::fprintf(stderr, "\n%s\n", ptl_last_error());
        if (pinned) frames.give(pinned);
    });
    return 0;
}

// The sub-frame draws of one clip: "draw sub-frame j of frame i" in the form the options ask for -- staged and launched once per frame, adaptive,
// with pass records, or plain -- what --depth-report and --clip-adaptive-aa --timing account behind every launch, and their lines at the end.
struct SubframeDraws {
    SubframeDraws(SceneRun& run, const Clip& clip, int count, bool with_float)
        : run(run), o(run.o), r(run.r.get()), seconds((double)(float)clip.duration), clip_name(clip.name), count(count), with_float(with_float) {}
    SceneRun& run;
    const Options& o;
    ptl_renderer* const r;
    const double seconds;  // the clip's duration
    const std::string& clip_name;
    const int count;  // the clip's frames
    const bool with_float, batched = batch_subframes(o), with_records = clip_records(o);
    const size_t frame_records = ptl_pass_record_bytes(run.width, run.height);
    ptl_frame frame{run.width, run.height, 0, 1, 0};
    long traced = 0;
    // --clip-adaptive-aa under --timing: refined entries of all sub-frames, and the three passes' GPU ms summed (each frame is synchronised anyway)
    unsigned long long refined = 0;
    double pass_ms[3] = {0.0, 0.0, 0.0};
    DevicePtr per_launch;  // --depth-report: the stats kernel runs behind every launch into the clip's block; per_launch[i] collects frame i's exhausted paths

    int open() {
        if (o.clip_adaptive) ptl_renderer_set_option(r, "adaptive_aa_threshold", o.clip_adaptive_t);
        if (!o.depth_report) return 0;
        if (!(per_launch = device_alloc(o.device, sizeof(uint64_t) * (size_t)count, "alloc"))) return 1;
        if (ptl_device_memset(per_launch.get(), 0, sizeof(uint64_t) * (size_t)count, nullptr) != PTL_OK || ptl_device_memset(run.pass_stats.get(), 0, sizeof(ptl_pass_stats_block), nullptr) != PTL_OK)
            return fail("memset");
        return 0;
    }
    // The host step of sub-frame j of frame i: the camera is stateful, so a frame that is not drawn takes it as well
    int update(int i, int j) { return ptl_renderer_update(r, subframe_time(i, j, count, o.blur) * seconds, nullptr, nullptr) == PTL_OK ? 0 : fail("update"); }
    // Sub-frame j of frame i into `target` (an unbatched draw) or into slice j of run.subframes; the float and record slices beside it
    int draw(int i, int j, void* target, float* ms) {
        ptl_renderer_set_option(r, "aa_start", j);
        if (int rc = update(i, j)) return rc;
        void* target_f32 = with_float ? run.float_subframes[j] : nullptr;  // out_rgba32f of the draw
        void* block_f32 = with_float ? run.float_subframes[0] : nullptr;   // ... of a batched one: slice z behind slice z - 1
        float* timed = o.timing ? ms : nullptr;
        if (batched) {
            // everything a draw does short of launching; the launch follows behind the last sub-frame, once for all of them
            if (ptl_renderer_stage_slice(r, &frame, j) != PTL_OK) return fail("stage");
            const unsigned long long slice_pixels = (unsigned long long)run.width * run.height;
            if (j == o.blur - 1) {
                if ((o.clip_adaptive ? ptl_renderer_draw_slices_adaptive(r, &frame, o.blur, run.subframes[0], block_f32, slice_pixels, nullptr, timed)
                     : with_records  ? ptl_renderer_draw_slices_passes(r, &frame, o.blur, run.subframes[0], block_f32, run.record_block.get(), frame_records * (size_t)o.blur, slice_pixels, nullptr, timed)
                                     : ptl_renderer_draw_slices(r, &frame, o.blur, run.subframes[0], block_f32, slice_pixels, nullptr, timed)) != PTL_OK)
                    return fail("render");
                if (o.depth_report)
                    if (int rc = account_passes(i, run.record_block.get(), o.blur)) return rc;
                if (o.clip_adaptive && o.timing)
                    if (int rc = account_adaptive(true, o.blur)) return rc;
            }
        } else if (o.clip_adaptive) {  // (blur 1, blur > 16, --batch-subframes 0: the single-frame adaptive draw per sub-frame)
            if (ptl_renderer_draw_adaptive(r, &frame, target, target_f32, nullptr, timed) != PTL_OK) return fail("render");
            if (o.timing)
                if (int rc = account_adaptive(false, 1)) return rc;
        } else if (with_records) {  // (the unbatched sub-frame with its records, and the stats kernel behind it)
            // --clip-passes: the block keeps ALL sub-frames of a frame (an unbatched sub-frame j draws its records at slice j, where the batched launch
            // puts them), and one sweep behind the frame's last sub-frame merges them into the frame's pass images (PassImages::make)
            void* records = static_cast<char*>(run.record_block.get()) + (run.passes.on ? (size_t)j * frame_records : 0);
            if (ptl_renderer_draw_passes(r, &frame, target, target_f32, records, frame_records, nullptr, nullptr, timed) != PTL_OK) return fail("render");
            if (o.depth_report)
                if (int rc = account_passes(i, records, 1)) return rc;
        } else if (ptl_renderer_draw(r, &frame, target, target_f32, nullptr, nullptr, timed) != PTL_OK) {
            // (without --timing the launch is not waited for: the host evaluates the next sub-frame's uniforms while this one traces)
            return fail("render");
        }
        ++traced;
        return 0;
    }
    int account_adaptive(bool slices, int n) {
        unsigned int counts[16] = {};
        void* dev_counts = nullptr;
        if ((slices ? ptl_renderer_adaptive_slices_result(r, nullptr, nullptr, &dev_counts) : ptl_renderer_adaptive_result(r, nullptr, &dev_counts)) != PTL_OK ||
            ptl_device_download(counts, dev_counts, sizeof(unsigned int) * (size_t)n, nullptr) != PTL_OK)
            return fail("refined count");
        for (int z = 0; z < n; ++z) refined += counts[z];
        float ms3[3] = {0.0f, 0.0f, 0.0f};
        ptl_renderer_adaptive_times(r, ms3);
        for (int p = 0; p < 3; ++p) pass_ms[p] += ms3[p];
        return 0;
    }
    int account_passes(int i, const void* records, int n) {  // the records of the launch that just went out: n sub-frames of frame i, one behind the other
        return ptl_pass_stats(o.device, records, (long)n * run.width * run.height, run.pass_stats.get(), per_launch.get(), i, nullptr, nullptr) == PTL_OK ? 0 : fail("pass_stats");
    }
    int report() {  // at the end of the clip
        if (o.depth_report) {  // one download, one line: the clip's block, and the frame whose launches cut most paths
            ptl_pass_stats_block stats{};
            std::vector<uint64_t> cut((size_t)count, 0);
            if (ptl_device_download(&stats, run.pass_stats.get(), sizeof stats, nullptr) != PTL_OK || ptl_device_download(cut.data(), per_launch.get(), sizeof(uint64_t) * cut.size(), nullptr) != PTL_OK)
                return fail("download");
            const size_t worst = (size_t)(std::max_element(cut.begin(), cut.end()) - cut.begin());
            print_depth_report(stats, render_depth_of(r, run.width, run.height),
                               "; `" + clip_name + "`: " + std::to_string(traced) + " sub-frames, worst frame " + std::to_string(worst) + " (" + std::to_string(cut[worst]) + " paths cut)");
        }
        if (o.clip_adaptive && o.timing) {
            const unsigned long long pixels = (unsigned long long)traced * (unsigned long long)run.width * (unsigned long long)run.height;
            std::printf("adaptive aa: threshold %d, %llu of %llu pixels refined (%.2f %%); GPU ms: one-sample pass %.3f, classification %.3f, refine pass %.3f\n", o.clip_adaptive_t,
                        refined, pixels, pixels ? 100.0 * (double)refined / (double)pixels : 0.0, pass_ms[0], pass_ms[1], pass_ms[2]);
        }
        return 0;
    }
};

// render_animation (src/main.rs:1758-1873): every frame of the clip traced, made and handed to the output
int trace_clip(SceneRun& run, ClipRun& c, const Clip& clip) {
    const Options& o = run.o;
    ptl_renderer* r = run.r.get();
    FramePipeline& pipe = run.pipe;
    FrameOutput& out = *c.out;
    PassImages& passes = run.passes;
    auto started = std::chrono::steady_clock::now();
    int rejits_before = ptl_renderer_rejit_count(r);
    if (o.skip_existing && exists(out.video_base + ".mov")) {
        std::printf("Skip `%s/%s`, because it's already exists\n", run.name.c_str(), clip.name.c_str());
        return 0;
    }
    make_dirs(dir_of(out.video_base));
    if (int rc = out.open()) return rc;
    int count = std::max(1, (int)((float)clip.duration * (float)clip.fps));  // ((duration_seconds * fps as f32) as usize).max(1)
    int last = o.max_frames >= 0 ? std::min(count, o.max_frames) : count;
    double gpu_ms = 0.0;
    long drawn_frames = 0;
    SubframeDraws draws(run, clip, count, out.wants_float());
    if (int rc = draws.open()) return rc;
    if (passes.on) make_dirs(passes.anim_dir());  // (a Y4M clip has no other use for it)
    const bool direct = out.draws_result();
    for (int i = 0; i < last; ++i) {
        if (int rc = out.check()) return rc;
        if (i % o.shards != o.shard || (out.have(i) && (!passes.on || passes.have(i)))) {  // (a frame with a pass file missing is drawn again, all its files rewritten)
            // Not ours (shard K of N takes every N-th frame) or already on disk.  The camera is stateful -- where it is relative
            // to the portals depends on the path it took (teleport_camera) -- so the host step still runs for every sub-frame:
            // a shard, or a resumed run, then sees exactly the cameras of an uninterrupted run.  (The reference skips the
            // update as well, src/main.rs:1789-1792, and so renders a resumed clip from a different camera history.)
            for (int j = 0; j < o.blur; ++j)
                if (int rc = draws.update(i, j)) return rc;
            continue;
        }
        int slot = (int)(drawn_frames++ % FramePipeline::kRing);
        if (pipe.copy_pending[slot] && ptl_stream_wait_event(nullptr, pipe.copied[slot]) != PTL_OK) return fail("wait");  // GPU-side: slot is free
        // The sub-frames go one behind the other on one stream.  Several kernel instances in flight (the library's "concurrent_draws") gave identical
        // frames and NO gain here -- 1080p monoportal 0.0519 ms per sub-frame with one instance, 0.0522 with two, 0.0559 with four; 720p 0.031 -> 0.039;
        // 4K aa 4 0.884 -> 0.885 / 0.908: the cross-stream event waits cost what the overlapped tails save (profiles/r04/concurrent_draws.jsonl)
        for (int j = 0; j < o.blur; ++j) {
            void* target = direct ? pipe.results[slot] : run.subframes[j];
            float ms = 0.0f;
            if (int rc = draws.draw(i, j, target, &ms)) return rc;
            gpu_ms += ms;
            // the clip's stills: sub-frame 0 of the first frame (read behind the launch, which a batched frame has behind its last sub-frame), the
            // last of the last.  The download is on the default stream, like the draws
            if (i == 0 && j == (draws.batched ? o.blur - 1 : 0))
                if (int rc = write_still(run, c, draws.batched ? run.subframes[0] : target, out.video_base + ".start.png")) return rc;
            if (i == count - 1 && j == o.blur - 1)
                if (int rc = write_still(run, c, target, out.video_base + ".end.png")) return rc;
        }
        if (!direct) {
            float ms = 0.0f;
            if (int rc = out.make_result(pipe.results[slot], o.timing ? &ms : nullptr)) return rc;
            gpu_ms += ms;
        }
        if (passes.on)
            if (int rc = passes.make(r, run.record_block.get(), o.blur, slot, &gpu_ms)) return rc;
        // hand the finished frame to the copy stream and go on tracing; the host job waits for its own event
        uint8_t* pixels = c.pinned.take();  // blocks while every buffer is still being encoded
        void* arrived = nullptr;
        if (int rc = pipe.hand_off(slot, pixels, run.download_bytes, &arrived)) return rc;
        if (passes.on)
            if (int rc = passes.copy_out(slot, pipe.copy_stream)) return rc;
        if (int rc = pipe.slot_left(slot)) return rc;
        out.submit(i, pixels, arrived, c.pool, c.pinned);
        if (passes.on) passes.submit(i, c.pool);
        std::printf("\r%d/%d done      ", i, count);
        std::fflush(stdout);
    }
    std::printf("\n");
    char gpu_time[96] = "";
    if (o.timing) std::snprintf(gpu_time, sizeof gpu_time, ", GPU %.1f ms (%.3f ms each),", gpu_ms, draws.traced ? gpu_ms / draws.traced : 0.0);
    std::printf("Traced `%s/%s`: %ld sub-frames %dx%d%s submitted after %.2f s, kernel rebuilt %d times\n", run.name.c_str(), clip.name.c_str(), draws.traced, run.width,
                run.height, gpu_time, seconds_since(started), ptl_renderer_rejit_count(r) - rejits_before);
    return draws.report();
}

// One clip: its buffers, pools and output for as long as it takes, released on every way out
int render_clip(SceneRun& run, const Clip& clip) {
    auto clip_start = std::chrono::steady_clock::now();
    // frames in flight between download and encode: one per encoder thread, but no more than ~2 GB of page-locked memory
    int in_flight = (int)std::max<size_t>(4, std::min<size_t>((size_t)run.threads + 2, ((size_t)2 << 30) / run.download_bytes));
    ClipRun c{{run.download_bytes, in_flight}, {run.threads, (size_t)run.threads * 2}, make_output(run, clip, (size_t)in_flight)};
    if (!c.pinned.ok() || (run.passes.on && !run.passes.open_clip(in_flight))) return fail("pinned host memory");
    const int rc = trace_clip(run, c, clip);
    if (run.passes.on && rc == 0 && run.o.shards == 1 && run.o.max_frames < 0) {
        c.pool.finish();  // every pass file is on disk
        run.passes.park(c.out->video_base + ".passes", clip.name);
    }
    return c.out->close(rc, c.pool, clip_start);
}

// Warm the code-object cache for the NEXT clip's specialised kernel while the current clip renders: a private copy of the scene
// is taken through the same history (every clip initialised so far, with its overrides), then compiled for gfx950 without a
// device.  When the main thread gets to that clip it generates the same source and finds the binary on disk; if the histories
// ever disagree it just compiles as before.
void prefetch_clip_kernel(const std::string& path, const std::vector<std::string>& history, const Options& o) {
    ScenePtr scene = open_scene(path);
    if (!scene) return;
    for (const std::string& clip : history) {
        if (ptl_scene_init_animation(scene.get(), clip.c_str()) != PTL_OK) return;
        apply_clip_overrides(scene.get(), nullptr, clip, nullptr);
    }
    // (the mode switches are compiled into a specialised kernel: the compile-only renderer must have the ones the clip is drawn with)
    const char* names[] = {"draw_side_by_side"};
    const double values[] = {o.stereo ? 1.0 : 0.0};
    ptl_renderer* built = nullptr;
    if (ptl_renderer_create_with_options(scene.get(), -1, o.asset_root.c_str(), clip_flags(o, true), names, values, 1, &built, nullptr, 0) != PTL_OK) return;
    RendererPtr r(built);
    ptl_renderer_prebuild_teleport(r.get());  // the camera of a clip moves: its teleport queries need the other half of the build as well
}

// Specialised kernels of the clips to come are compiled ahead by a few background threads (in clip order), so a run of
// many short clips is not a run of JIT waits; the main thread only waits if it reaches a clip before its binary is ready.
class Prefetcher {
public:
    void start(const Options& o, const std::string& path, const std::vector<Clip>& clips) {  // (the first clip is compiled by the main thread right away)
        done_.assign(clips.size(), 0);
        if (o.specialize == 0 || clips.size() < 2) return;
        int n_workers = (int)std::min<size_t>({(size_t)6, clips.size() - 1, (size_t)std::max(1u, std::thread::hardware_concurrency() / 4)});
        next_ = 1;
        for (int wk = 0; wk < n_workers; ++wk) workers_.emplace_back([this, &o, path, clips](std::stop_token stop) { work(stop, o, path, clips); });
    }
    // Before the main thread builds clip k: waits for its binary if a worker is at it.  true: nobody has started it -- it is the
    // caller's to compile (the workers leave it alone from now on); false: it is in the cache.
    bool wait_or_claim(size_t k) {
        if (workers_.empty() || k < 1) return true;
        std::unique_lock<std::mutex> lock(mu_);
        cv_.wait(lock, [&] { return done_[k] || next_ <= k; });
        if (!done_[k]) next_ = k + 1;
        return !done_[k];
    }

private:
    void work(std::stop_token stop, const Options& o, const std::string& path, const std::vector<Clip>& clips) {
        for (;;) {
            size_t k;
            {
                std::unique_lock<std::mutex> lock(mu_);
                if (stop.stop_requested() || next_ >= clips.size()) return;
                k = next_++;
            }
            std::vector<std::string> history;
            for (size_t c = 0; c <= k; ++c) history.push_back(clips[c].name);
            if (clips[k].specialise) prefetch_clip_kernel(path, history, o);
            {
                std::unique_lock<std::mutex> lock(mu_);
                done_[k] = 1;
            }
            cv_.notify_all();
        }
    }
    std::mutex mu_;
    std::condition_variable cv_;
    std::vector<char> done_;
    size_t next_ = 0;
    std::vector<std::jthread> workers_;  // (last: they are asked to stop, and joined, before what they use goes)
};

// which clips: the named ones (render_named_animations) or all, optionally filtered (render_all_animations)
int clips_to_render(const SceneRun& run, std::vector<Clip>* todo) {  // 0, or the exit status
    const Options& o = run.o;
    std::vector<Clip> clips;
    char name[256];
    double duration = 0.0;
    for (int k = 0; ptl_scene_animation(run.scene.get(), k, name, sizeof name, &duration) == PTL_OK; ++k) clips.push_back({name, duration});
    if (o.clips.empty()) {
        for (auto& c : clips)
            if (o.starts_with.empty() || c.name.compare(0, o.starts_with.size(), o.starts_with) == 0) todo->push_back(c);
    }
    for (const std::string& want : split_list(o.clips)) {
        auto it = std::find_if(clips.begin(), clips.end(), [&](auto& c) { return c.name == want; });
        if (it == clips.end()) return scene_has_no(run.name, "animation", want);
        todo->push_back(*it);
    }
    for (Clip& c : *todo) {
        c.fps = o.fps;
        apply_clip_overrides(nullptr, nullptr, c.name, &c.fps);
        int count = std::max(1, (int)((float)c.duration * (float)c.fps));
        double samples = (double)run.width * run.height * o.aa * count * o.blur;
        c.specialise = o.specialize >= 0 ? o.specialize != 0 : samples >= 1e10;
    }
    return 0;
}

int render_scene(const Options& o, const std::string& path) {
    SceneRun run(o, scene_link(path));
    std::printf("Rendering scene %s\n", run.name.c_str());
    run.scene = load_scene(path, run.name);
    if (!run.scene) return 1;
    ptl_scene* scene = run.scene.get();
    std::vector<Clip> todo;
    if (int rc = clips_to_render(run, &todo)) return rc;
    // The un-baked kernel (every scene uniform a run-time value) is wanted NOW when a clip starts on it: the quick build.  When the first
    // clip gets a clip-constant kernel anyway, the renderer is created on that one directly (the scene taken into the clip first, as the
    // clip loop and prefetch_clip_kernel do) instead of building an un-baked kernel nothing would run on.  profiles/r03/video_*.log
    bool start_baked = !todo.empty() && todo[0].specialise;
    if (start_baked) {
        if (ptl_scene_init_animation(scene, todo[0].name.c_str()) != PTL_OK) return fail("init_animation");
        apply_clip_overrides(scene, nullptr, todo[0].name, nullptr);
    }
    run.r = create_renderer(scene, o.device, o, clip_flags(o, start_baked) | quick_jit_flag(o), "renderer",
                            {{"aa_count", (double)o.aa}, {"render_depth", (double)o.depth}, {"draw_side_by_side", o.stereo ? 1.0 : 0.0}});
    if (!run.r) return 1;
    ptl_renderer* r = run.r.get();
    ptl_renderer_set_option(r, "aa_count", o.aa);
    ptl_renderer_set_option(r, "render_depth", o.depth);
    ptl_renderer_set_option(r, "draw_side_by_side", o.stereo ? 1 : 0);
    const std::unique_ptr<FrameOutput> form = make_output(run, Clip{}, 1);  // (an output that is never opened)
    run.result_bytes = form->result_bytes();
    run.download_bytes = form->download_bytes();
    // one block per kind, sub-frame j at j * its bytes: RGBA8, RGBA32F where the form wants floats (16 bytes per pixel), the pass records
    const size_t slices = (size_t)std::max(1, o.blur), float_bytes = run.frame_bytes * 4;
    if (!(run.subframe_block = device_alloc(o.device, run.frame_bytes * slices, "alloc"))) return 1;
    if (form->wants_float() && !(run.float_block = device_alloc(o.device, float_bytes * slices, "alloc"))) return 1;
    for (size_t j = 0; j < slices; ++j) {
        run.subframes.push_back(static_cast<char*>(run.subframe_block.get()) + j * run.frame_bytes);
        if (run.float_block) run.float_subframes.push_back(static_cast<char*>(run.float_block.get()) + j * float_bytes);
    }
    if (clip_records(o) && !(run.record_block = device_alloc(o.device, ptl_pass_record_bytes(run.width, run.height) * slices, "alloc"))) return 1;
    if (o.depth_report && !(run.pass_stats = device_alloc(o.device, sizeof(ptl_pass_stats_block), "alloc"))) return 1;
    if (run.passes.on)
        if (int rc = run.passes.allocate()) return rc;
    if (!run.pipe.create(o.device, run.result_bytes)) return fail("pipeline");
    Prefetcher prefetch;
    prefetch.start(o, path, todo);
    for (size_t k = 0; k < todo.size(); ++k) {
        Clip& clip = todo[k];
        prefetch.wait_or_claim(k);  // either way the binary is there, or is built, when the renderer asks for it below
        if (ptl_scene_init_animation(scene, clip.name.c_str()) != PTL_OK) return fail("init_animation");
        if (ptl_renderer_update(r, 0.0, nullptr, nullptr) != PTL_OK) return fail("update");
        ptl_renderer_set_option(r, "render_depth", o.depth);
        apply_clip_overrides(scene, r, clip.name, &clip.fps);
        if (ptl_renderer_set_option(r, "specialize_static", clip.specialise ? 1 : 0) != PTL_OK) return fail("specialize");
        std::printf("Rendering animation %s, %zu/%zu\n", clip.name.c_str(), k + 1, todo.size());
        if (int rc = render_clip(run, clip)) return rc;
    }
    return 0;
}

}  // namespace

int render(const Options& o) {
    auto total_start = std::chrono::steady_clock::now();
    for (const std::string& scene_arg : split_list(o.scene))
        if (int rc = render_scene(o, scene_file(scene_arg, o.scenes_dir))) return rc;
    std::printf("Total render time: %.2f s\n", seconds_since(total_start));
    return 0;
}
