// postprocess.cpp -- C ABI for the fixed (ahead-of-time compiled) gfx950 helper kernels.
//
// ptl_average_images: the GPU form of the reference's average_images (src/main.rs:645-722), the
// motion-blur step of the video pipeline (src/main.rs:1787-1817).  The kernel is built by
// `make kernels` (hipcc --genco --offload-arch=gfx950, portal_amd/csrc/kernels/average_images.hip)
// into portal_amd/kernels/average_images.hsaco next to this library and loaded with hipModuleLoadData.
#include <dlfcn.h>

#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../../include/portal_amd.h"
#include "../kernels/pass_key.h"
#include "../kernels/png_deflate_shape.h"
#include "../kernels/rgb48_shape.h"
#include "../kernels/yuv_shape.h"
#include "hip_api.h"
#include "internal.h"

using namespace ptl;

namespace {

constexpr int kMaxSubframes = 64;        // PTL_MAX_SUBFRAMES in average_images.hip: pointers in the kernel arguments
constexpr int kMaxSubframesTable = 256;  // beyond: a pointer table in device memory; 256 is where the exact multiply-high mean ends

struct LoadedKernel {
    hip::hipFunction_t fn = nullptr;
    hip::hipEvent_t ev0 = nullptr, ev1 = nullptr;
};
struct LoadedModule {
    hip::hipModule_t module = nullptr;
    std::map<std::string, LoadedKernel> entries;
};

std::string library_dir() {
    Dl_info info;
    if (dladdr(reinterpret_cast<void*>(&library_dir), &info) == 0 || !info.dli_fname) return ".";
    std::string path = info.dli_fname;
    size_t p = path.rfind('/');
    return p == std::string::npos ? "." : path.substr(0, p);
}

// one module per (device, kernel file), read and loaded once; its functions by entry, each with its own pair of timing events
int load_kernel(int device, const char* file, const char* entry, LoadedKernel** out) {
    static std::mutex mu;
    static std::map<std::string, LoadedModule> cache;
    std::lock_guard<std::mutex> lock(mu);
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    LoadedModule& m = cache[std::to_string(device) + ":" + file];  // (a module that failed to load stays null here and is tried again)
    if (auto it = m.entries.find(entry); it != m.entries.end()) {
        *out = &it->second;
        return PTL_OK;
    }
    std::string path = library_dir() + "/kernels/" + file;
    LoadedKernel k;
    bool ok = rt->hipSetDevice(device) == 0;
    if (!m.module) {
        std::ifstream f(path, std::ios::binary);
        if (!f) {
            set_last_error("missing gfx950 code object `" + path + "`: run `make kernels` (no CPU fallback)");
            return PTL_ERR_INVALID;
        }
        std::vector<char> code((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
        ok = ok && rt->hipModuleLoadData(&m.module, code.data()) == 0;
    }
    if (!ok || rt->hipModuleGetFunction(&k.fn, m.module, entry) != 0) {
        set_last_error("cannot load `" + path + "` on device " + std::to_string(device));
        return PTL_ERR_HIP;
    }
    rt->hipEventCreate(&k.ev0);
    rt->hipEventCreate(&k.ev1);
    *out = &m.entries.emplace(entry, k).first->second;
    return PTL_OK;
}

// `launch` (the stream work of one call, -> a HIP error code) between the kernel's two events when `elapsed_ms` is given: the call then
// waits for it and reads the time.  -> what `launch` returned.
template <typename Launch>
int timed(const hip::Runtime* rt, LoadedKernel* k, void* stream, float* elapsed_ms, Launch launch) {
    if (elapsed_ms) rt->hipEventRecord(k->ev0, stream);
    const int err = launch();
    if (err == 0 && elapsed_ms) {
        rt->hipEventRecord(k->ev1, stream);
        rt->hipEventSynchronize(k->ev1);
        rt->hipEventElapsedTime(elapsed_ms, k->ev0, k->ev1);
    }
    return err;
}

// Workgroups of 256 for `lanes` lanes: the kernels stride over the grid beyond 16 workgroups per CU (PTL_AVERAGE_IMAGES_GRID_CAP, read at each
// call: tuning, and the tests that make the stride loops go round).
long grid_blocks(long lanes) {
    long cap = 256 * 16;
    if (const char* c = std::getenv("PTL_AVERAGE_IMAGES_GRID_CAP")) cap = std::atol(c) > 0 ? std::atol(c) : cap;
    return std::min(cap, std::max(1L, (lanes + 255) / 256));
}

// What ptl_average_images, the ptl_average_*_to_yuv* family and ptl_average_f32_to_rgb48 share: a kernel over N sub-frames with two entries (up to 64 pointers in the
// kernel arguments, beyond in a device table), launched as `lanes` lanes in workgroups of 256 (grid-stride beyond the cap) on `stream`.
// The kernel's arguments are (frames, n, tail...).
struct SubframeKernel {
    const char* file;
    const char* entry_list;
    const char* entry_table;
    const char* what;
};

int check_subframes(const void* const* frames_rgba8, int n_frames, const void* out, int width, int height) {
    if (!frames_rgba8 || !out || n_frames < 1 || n_frames > kMaxSubframesTable || width <= 0 || height <= 0) return PTL_ERR_INVALID;
    for (int k = 0; k < n_frames; ++k)
        if (!frames_rgba8[k] || (reinterpret_cast<uintptr_t>(frames_rgba8[k]) & 15u)) return PTL_ERR_INVALID;
    if (reinterpret_cast<uintptr_t>(out) & 15u) return PTL_ERR_INVALID;
    return PTL_OK;
}

int launch_over_subframes(int device, const SubframeKernel& kernel, const void* const* frames_rgba8, int n_frames, std::vector<void*> tail, long lanes,
                          void* stream, float* elapsed_ms) {
    LoadedKernel* k = nullptr;
    const bool table = n_frames > kMaxSubframes;
    int rc = load_kernel(device, kernel.file, table ? kernel.entry_table : kernel.entry_list, &k);
    if (rc != PTL_OK) return rc;
    const hip::Runtime* rt = hip::runtime(nullptr);
    rt->hipSetDevice(device);
    struct {
        const void* frame[kMaxSubframes];
    } list{};
    for (int i = 0; i < n_frames && !table; ++i) list.frame[i] = frames_rgba8[i];
    int n = n_frames;
    void* dev_table = nullptr;
    if (table) {  // rare (the reference's clips use <= 16): a pointer table per call, freed once the launch has gone through the stream
        if (rt->hipMalloc(&dev_table, sizeof(void*) * (size_t)n_frames) != 0 ||
            rt->hipMemcpyAsync(dev_table, frames_rgba8, sizeof(void*) * (size_t)n_frames, hip::kMemcpyHostToDevice, stream) != 0) {
            if (dev_table) rt->hipFree(dev_table);
            set_last_error(std::string(kernel.what) + ": cannot stage the sub-frame pointer table");
            return PTL_ERR_HIP;
        }
    }
    std::vector<void*> args = {table ? static_cast<void*>(&dev_table) : static_cast<void*>(&list), &n};
    args.insert(args.end(), tail.begin(), tail.end());
    const long blocks = grid_blocks(lanes);
    const int err = timed(rt, k, stream, elapsed_ms, [&] { return rt->hipModuleLaunchKernel(k->fn, (unsigned)blocks, 1, 1, 256, 1, 1, 0, stream, args.data(), nullptr); });
    if (err != 0) {
        if (dev_table) rt->hipFree(dev_table);
        set_last_error(std::string("hipModuleLaunchKernel(") + kernel.what + "): " + rt->hipGetErrorString(err));
        return PTL_ERR_HIP;
    }
    if (dev_table) {
        rt->hipStreamSynchronize(stream);  // hipFree would wait for the device anyway
        rt->hipFree(dev_table);
    }
    return PTL_OK;
}

// What ptl_aa_edges and ptl_aa_edges_slices share: the classification kernel in `file` over `n` frames, a 256-thread workgroup per 64x32
// pixel region and frame.  The `n` counts are reset on `stream` by the call itself, inside the time it reports.
int launch_aa_edges(int device, const char* file, const char* entry, const char* what, void** args, void* counts, int n, int width, int height, void* stream,
                    float* elapsed_ms) {
    LoadedKernel* k = nullptr;
    if (int rc = load_kernel(device, file, entry, &k); rc != PTL_OK) return rc;
    const hip::Runtime* rt = hip::runtime(nullptr);
    rt->hipSetDevice(device);
    const int err = timed(rt, k, stream, elapsed_ms, [&] {
        const int reset = rt->hipMemsetAsync(counts, 0, 4 * (size_t)n, stream);
        return reset != 0 ? reset : rt->hipModuleLaunchKernel(k->fn, (unsigned)((width + 63) / 64), (unsigned)((height + 31) / 32), (unsigned)n, 256, 1, 1, 0, stream, args, nullptr);
    });
    if (err != 0) {
        set_last_error(std::string("hipModuleLaunchKernel(") + what + "): " + rt->hipGetErrorString(err));
        rt->hipGetLastError();
        return PTL_ERR_HIP;
    }
    return PTL_OK;
}

}  // namespace

extern "C" int ptl_average_images(int device, const void* const* frames_rgba8, int n_frames, void* out_rgba8, int width, int height,
                                  void* stream, float* elapsed_ms) {
    if (int rc = check_subframes(frames_rgba8, n_frames, out_rgba8, width, height)) return rc;
    const char* variant = std::getenv("PTL_AVERAGE_IMAGES_HSACO");  // tuning only: another build of the same kernel (tools/average_variants.py)
    const SubframeKernel kernel{variant && *variant ? variant : "average_images.hsaco", "ptl_average_images_kernel", "ptl_average_images_table_kernel", "average_images"};
    long n_px = (long)width * height;
    return launch_over_subframes(device, kernel, frames_rgba8, n_frames, {&out_rgba8, &n_px}, n_px / 4, stream, elapsed_ms);  // a lane per 16-byte vector
}

// The Y4M hand-off: the same averaging fused with the conversion to planar Y'CbCr 10 bit, from RGBA8 sub-frames (portal_amd/csrc/kernels/yuv10.hip)
// or from the RGBA32F frames a render call stores as out_rgba32f (yuv10_f32.hip), at 4:2:0, 4:2:2 or 4:4:4; the contract is in
// include/portal_amd.h.  Which frames take the fast path, and how many lanes a frame needs either way, is yuv_shape.h's to say: the kernels'
// dispatcher reads the same header.
namespace {
#define PTL_YUV_KERNEL(file, name) SubframeKernel{file, "ptl_" name "_kernel", "ptl_" name "_table_kernel", name}
const SubframeKernel kYuvKernels[2][3] = {
    {PTL_YUV_KERNEL("yuv10.hsaco", "average_to_yuv420p10"), PTL_YUV_KERNEL("yuv10.hsaco", "average_to_yuv422p10"), PTL_YUV_KERNEL("yuv10.hsaco", "average_to_yuv444p10")},
    {PTL_YUV_KERNEL("yuv10_f32.hsaco", "average_f32_to_yuv420p10"), PTL_YUV_KERNEL("yuv10_f32.hsaco", "average_f32_to_yuv422p10"),
     PTL_YUV_KERNEL("yuv10_f32.hsaco", "average_f32_to_yuv444p10")}};
#undef PTL_YUV_KERNEL

bool is_chroma(int chroma) { return chroma == PTL_CHROMA_420 || chroma == PTL_CHROMA_422 || chroma == PTL_CHROMA_444; }
bool known_chroma(int chroma, const char* what) {
    if (is_chroma(chroma)) return true;
    set_last_error(std::string(what) + ": chroma " + std::to_string(chroma) + " is none of 420, 422, 444");
    return false;
}

int average_to_yuv(bool f32, int chroma, int device, const void* const* frames, int n_frames, void* out_yuv, int width, int height, void* stream, float* elapsed_ms) {
    if (!known_chroma(chroma, f32 ? "average_f32_to_yuv10" : "average_to_yuv10")) return PTL_ERR_INVALID;
    if (int rc = check_subframes(frames, n_frames, out_yuv, width, height)) return rc;
    if ((long)width * height > ptl_yuv_max_pixels(f32)) return PTL_ERR_INVALID;  // the kernel addresses a sub-frame with 32-bit byte offsets
    const SubframeKernel& kernel = kYuvKernels[f32][chroma == PTL_CHROMA_420 ? 0 : chroma == PTL_CHROMA_422 ? 1 : 2];
    const long lanes = ptl_yuv_lanes(f32, chroma, (unsigned)width, (unsigned)height);
    return launch_over_subframes(device, kernel, frames, n_frames, {&out_yuv, &width, &height}, lanes, stream, elapsed_ms);
}
}  // namespace

extern "C" size_t ptl_yuv10_frame_bytes(int width, int height, int chroma) {
    if (width <= 0 || height <= 0 || !is_chroma(chroma)) return 0;
    const size_t cw = ptl_yuv_cw(chroma, (unsigned)width), ch = ptl_yuv_ch(chroma, (unsigned)height);
    return 2 * ((size_t)width * (size_t)height + 2 * cw * ch);
}
extern "C" size_t ptl_yuv420p10_frame_bytes(int width, int height) { return ptl_yuv10_frame_bytes(width, height, PTL_CHROMA_420); }

extern "C" int ptl_average_to_yuv10(int device, const void* const* frames_rgba8, int n_frames, void* out_yuv, int width, int height, int chroma, void* stream,
                                    float* elapsed_ms) {
    return average_to_yuv(false, chroma, device, frames_rgba8, n_frames, out_yuv, width, height, stream, elapsed_ms);
}
extern "C" int ptl_average_f32_to_yuv10(int device, const void* const* frames_rgba32f, int n_frames, void* out_yuv, int width, int height, int chroma, void* stream,
                                        float* elapsed_ms) {
    return average_to_yuv(true, chroma, device, frames_rgba32f, n_frames, out_yuv, width, height, stream, elapsed_ms);
}
extern "C" int ptl_average_to_yuv420p10(int device, const void* const* frames_rgba8, int n_frames, void* out_yuv, int width, int height, void* stream,
                                        float* elapsed_ms) {
    return average_to_yuv(false, PTL_CHROMA_420, device, frames_rgba8, n_frames, out_yuv, width, height, stream, elapsed_ms);
}
extern "C" int ptl_average_f32_to_yuv420p10(int device, const void* const* frames_rgba32f, int n_frames, void* out_yuv, int width, int height, void* stream,
                                            float* elapsed_ms) {
    return average_to_yuv(true, PTL_CHROMA_420, device, frames_rgba32f, n_frames, out_yuv, width, height, stream, elapsed_ms);
}

// The 16-bit PNG hand-off: the averaged frame of the float sub-frames as RGB scanlines, unfiltered or with PNG's Sub filter applied
// (portal_amd/csrc/kernels/rgb48_f32.hip; the contract is in include/portal_amd.h).  The fast path and the lane count are rgb48_shape.h's to say.
extern "C" size_t ptl_rgb48_frame_bytes(int width, int height) { return width <= 0 || height <= 0 ? 0 : 6 * (size_t)width * (size_t)height; }

extern "C" int ptl_average_f32_to_rgb48(int device, const void* const* frames_rgba32f, int n_frames, void* out_rows, int width, int height, int filter, void* stream,
                                        float* elapsed_ms) {
    if (!ptl_rgb48_is_filter(filter)) {
        set_last_error("average_f32_to_rgb48: filter " + std::to_string(filter) + " is neither PTL_PNG_FILTER_NONE (0) nor PTL_PNG_FILTER_SUB (1)");
        return PTL_ERR_INVALID;
    }
    if (int rc = check_subframes(frames_rgba32f, n_frames, out_rows, width, height)) return rc;
    if ((long)width * height > ptl_rgb48_max_pixels()) return PTL_ERR_INVALID;  // the kernel addresses a sub-frame with 32-bit byte offsets
    static const SubframeKernel kKernels[2] = {
        {"rgb48_f32.hsaco", "ptl_average_f32_to_rgb48_none_kernel", "ptl_average_f32_to_rgb48_none_table_kernel", "average_f32_to_rgb48"},
        {"rgb48_f32.hsaco", "ptl_average_f32_to_rgb48_sub_kernel", "ptl_average_f32_to_rgb48_sub_table_kernel", "average_f32_to_rgb48"}};
    const long lanes = ptl_rgb48_lanes((unsigned)width, (unsigned)height);
    return launch_over_subframes(device, kKernels[filter == PTL_PNG_FILTER_SUB], frames_rgba32f, n_frames, {&out_rows, &width, &height}, lanes, stream, elapsed_ms);
}

// The GPU deflate of a PNG frame (portal_amd/csrc/kernels/png_deflate.hip, png_huffman.hip; the stream contracts are in include/portal_amd.h):
// a bands kernel, a workgroup per band (grid-stride beyond the cap), then the one pack kernel, on the same stream.  The cut into bands and the
// layout of the result buffer are png_deflate_shape.h's to say: the kernels read the same header.
namespace {
static_assert(PTL_PNG_STREAM_HEADER_BYTES == ptl_png_header_bytes, "the header the kernels write");

// What the three entry points differ in: the bytes of a pixel, the bands kernel and whether it takes `codes`, and what error texts call them.
// (The three names are the error texts of before, message for message: test_entry_point_refuses_before_any_gpu_call of test_png_deflate.py,
// test_png_huffman.py and test_png16_deflate.py pins them.)
struct DeflateFormat {
    unsigned pixel;
    const char *file, *bands_entry;
    bool codes_argument;
    const char *codes_name, *name, *launch_name;
};
const DeflateFormat kDeflateFixed8 = {ptl_png_pixel8, "png_deflate.hsaco", "ptl_png_deflate_bands_kernel", false, "png_deflate_rgba8_codes", "png_deflate_rgba8", "png_deflate"};
const DeflateFormat kDeflateDynamic8 = {ptl_png_pixel8, "png_huffman.hsaco", "ptl_png_huffman_bands_kernel", false, "png_deflate_rgba8_codes", "png_deflate_rgba8", "png_deflate"};
const DeflateFormat kDeflate16 = {ptl_png_pixel16, "png_huffman.hsaco", "ptl_png_deflate16_bands_kernel", true, "png_deflate_rgb48", "png_deflate_rgb48", "png_deflate16"};

// 0 for a frame that does not fit, else `size` of it.
size_t deflate_size(unsigned pixel, int width, int height, ptl_png_u64 (*size)(unsigned, unsigned, unsigned)) {
    return width > 0 && height > 0 && ptl_png_fits(pixel, (unsigned)width, (unsigned)height) ? (size_t)size(pixel, (unsigned)width, (unsigned)height) : 0;
}

int deflate(const DeflateFormat& f, int device, const void* frame, int width, int height, int codes, void* out, void* stream, float* elapsed_ms) {
    if (codes != PTL_PNG_CODES_FIXED && codes != PTL_PNG_CODES_DYNAMIC) {
        set_last_error(std::string(f.codes_name) + ": codes " + std::to_string(codes) + " is neither PTL_PNG_CODES_FIXED (0) nor PTL_PNG_CODES_DYNAMIC (1)");
        return PTL_ERR_INVALID;
    }
    if (!frame || !out || width <= 0 || height <= 0) return PTL_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(frame) | reinterpret_cast<uintptr_t>(out)) & 15u) return PTL_ERR_INVALID;
    const std::string size = std::string(f.name) + ": " + std::to_string(width) + " x " + std::to_string(height);
    if (f.pixel == ptl_png_pixel16 && (long)width * height > ptl_rgb48_max_pixels()) {  // the rows' own limit
        set_last_error(size + " has more than 2^28 pixels");
        return PTL_ERR_INVALID;
    }
    if (!ptl_png_fits(f.pixel, (unsigned)width, (unsigned)height)) {  // the kernels address the raw scanlines with 32-bit offsets
        set_last_error(size + " has more than 2^31 bytes of scanlines");
        return PTL_ERR_INVALID;
    }
    if (device < 0) return PTL_ERR_NO_DEVICE;
    LoadedKernel *bands_kernel = nullptr, *pack_kernel = nullptr;
    if (int rc = load_kernel(device, f.file, f.bands_entry, &bands_kernel); rc != PTL_OK) return rc;
    if (int rc = load_kernel(device, "png_deflate.hsaco", "ptl_png_deflate_pack_kernel", &pack_kernel); rc != PTL_OK) return rc;
    const hip::Runtime* rt = hip::runtime(nullptr);
    rt->hipSetDevice(device);
    unsigned w = (unsigned)width, h = (unsigned)height, pixel = f.pixel, magic = ptl_png_magic(pixel), mode = (unsigned)codes;
    unsigned rows = ptl_png_band_rows(pixel, w), n_bands = ptl_png_bands(pixel, w, h);
    unsigned long long table_offset = ptl_png_table_offset(pixel, w, h), slots_offset = ptl_png_slots_offset(pixel, w, h), slot_stride = ptl_png_slot_stride(pixel, w);
    unsigned long long stream_room = table_offset - ptl_png_header_bytes;
    void* table = static_cast<char*>(out) + table_offset;
    void* slots = static_cast<char*>(out) + slots_offset;
    std::vector<void*> bands_args = {&frame, &w, &h, &rows, &n_bands, &table, &slots, &slot_stride};
    if (f.codes_argument) bands_args.insert(bands_args.begin() + 5, &mode);
    void* pack_args[] = {&out, &w, &h, &rows, &n_bands, &pixel, &magic, &table_offset, &slots_offset, &slot_stride, &stream_room};
    const unsigned blocks = (unsigned)grid_blocks(256L * n_bands);  // a workgroup per band
    const int err = timed(rt, bands_kernel, stream, elapsed_ms, [&] {
        const int e = rt->hipModuleLaunchKernel(bands_kernel->fn, blocks, 1, 1, 256, 1, 1, 0, stream, bands_args.data(), nullptr);
        return e != 0 ? e : rt->hipModuleLaunchKernel(pack_kernel->fn, blocks, 1, 1, 256, 1, 1, 0, stream, pack_args, nullptr);
    });
    if (err != 0) {
        set_last_error(std::string("hipModuleLaunchKernel(") + f.launch_name + "): " + rt->hipGetErrorString(err));
        rt->hipGetLastError();
        return PTL_ERR_HIP;
    }
    return PTL_OK;
}
}  // namespace

extern "C" size_t ptl_png_stream_bytes(int width, int height) { return deflate_size(ptl_png_pixel8, width, height, ptl_png_result_bytes); }
extern "C" size_t ptl_png_stream_download_bytes(int width, int height) { return deflate_size(ptl_png_pixel8, width, height, ptl_png_table_offset); }
extern "C" int ptl_png_stream_band_rows(int width) { return width > 0 && width <= (1 << 29) ? (int)ptl_png_band_rows(ptl_png_pixel8, (unsigned)width) : 0; }
extern "C" size_t ptl_png_stream16_bytes(int width, int height) { return deflate_size(ptl_png_pixel16, width, height, ptl_png_result_bytes); }
extern "C" size_t ptl_png_stream16_download_bytes(int width, int height) { return deflate_size(ptl_png_pixel16, width, height, ptl_png_table_offset); }
extern "C" int ptl_png_stream16_band_rows(int width) { return width > 0 && width <= (1 << 28) ? (int)ptl_png_band_rows(ptl_png_pixel16, (unsigned)width) : 0; }

// `codes`: PTL_PNG_CODES_FIXED launches the one-pass bands kernel of png_deflate.hip, PTL_PNG_CODES_DYNAMIC the two-pass one of png_huffman.hip,
// which writes the same table entries and slots.  The 16-bit frames go through the two-pass kernel in both modes.
extern "C" int ptl_png_deflate_rgba8_codes(int device, const void* frame_rgba8, int width, int height, int codes, void* out, void* stream, float* elapsed_ms) {
    return deflate(codes == PTL_PNG_CODES_DYNAMIC ? kDeflateDynamic8 : kDeflateFixed8, device, frame_rgba8, width, height, codes, out, stream, elapsed_ms);
}
extern "C" int ptl_png_deflate_rgba8(int device, const void* frame_rgba8, int width, int height, void* out, void* stream, float* elapsed_ms) {
    return deflate(kDeflateFixed8, device, frame_rgba8, width, height, PTL_PNG_CODES_FIXED, out, stream, elapsed_ms);
}
extern "C" int ptl_png_deflate_rgb48(int device, const void* rows_rgb48, int width, int height, int codes, void* out, void* stream, float* elapsed_ms) {
    return deflate(kDeflate16, device, rows_rgb48, width, height, codes, out, stream, elapsed_ms);
}

// ---- trace passes: the records a PTL_FLAG_PASSES render entry stores (portal_amd/csrc/kernels/pass_stats.hip, pass_gray16.hip; the contracts are
// in include/portal_amd.h).  Both kernels sweep `n` records with a strided grid of 256-thread workgroups.
namespace {
static_assert(sizeof(ptl_pass_record) == 16 && sizeof(ptl_pass_stats_block) == 64 + 16 + 8 * PTL_PASS_HIST_BINS, "the layouts the kernels read and write");
// pass_stats.hip adds its totals as eight uint64 from `pixels` on and its maxima as three uint32 from `max_trips` on (pass_key.h)
static_assert(offsetof(ptl_pass_stats_block, pixels) == ptl_pass_block_totals && offsetof(ptl_pass_stats_block, exhausted_pixels) == ptl_pass_block_totals + 56 &&
                  offsetof(ptl_pass_stats_block, max_trips) == ptl_pass_block_maxima && offsetof(ptl_pass_stats_block, depth_min_key_inv) == ptl_pass_block_maxima + 8 &&
                  offsetof(ptl_pass_stats_block, trips_histogram) == ptl_pass_block_histogram && PTL_PASS_HIST_BINS == ptl_pass_hist_bins,
              "");
static_assert(PTL_PASS_DEPTH == ptl_pass_which_depth && PTL_PASS_TRIPS == ptl_pass_which_trips, "");

int launch_over_records(int device, const char* file, const char* entry, const char* what, void** args, long lanes, void* stream, float* elapsed_ms) {
    if (device < 0) return PTL_ERR_NO_DEVICE;
    LoadedKernel* k = nullptr;
    if (int rc = load_kernel(device, file, entry, &k); rc != PTL_OK) return rc;
    const hip::Runtime* rt = hip::runtime(nullptr);
    rt->hipSetDevice(device);
    const int err = timed(rt, k, stream, elapsed_ms, [&] { return rt->hipModuleLaunchKernel(k->fn, (unsigned)grid_blocks(lanes), 1, 1, 256, 1, 1, 0, stream, args, nullptr); });
    if (err != 0) {
        set_last_error(std::string("hipModuleLaunchKernel(") + what + "): " + rt->hipGetErrorString(err));
        rt->hipGetLastError();
        return PTL_ERR_HIP;
    }
    return PTL_OK;
}
}  // namespace

extern "C" int ptl_pass_stats(int device, const void* records, long n, void* stats_block, void* per_launch, int slot, void* stream, float* elapsed_ms) {
    if (!records || !stats_block || n < 1 || n > (1L << 31) || slot < 0) return PTL_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(records) & 15u) || (reinterpret_cast<uintptr_t>(stats_block) & 7u) || (reinterpret_cast<uintptr_t>(per_launch) & 7u)) return PTL_ERR_INVALID;
    void* args[] = {&records, &n, &stats_block, &per_launch, &slot};
    return launch_over_records(device, "pass_stats.hsaco", "ptl_pass_stats_kernel", "pass_stats", args, n, stream, elapsed_ms);
}

extern "C" int ptl_pass_stats_depth_range(const ptl_pass_stats_block* block, float* lo, float* hi) {
    if (!block || !lo || !hi || block->depth_max_key == 0u || block->depth_min_key_inv == 0u) return 0;
    const unsigned int lo_bits = ptl_pass_depth_bits(~block->depth_min_key_inv), hi_bits = ptl_pass_depth_bits(block->depth_max_key);
    std::memcpy(lo, &lo_bits, 4);
    std::memcpy(hi, &hi_bits, 4);
    return 1;
}

extern "C" int ptl_passes_to_gray16(int device, const void* records, long n, void* out_rows, int which, float lo, float hi, void* stream, float* elapsed_ms) {
    if (which != PTL_PASS_DEPTH && which != PTL_PASS_TRIPS) {
        set_last_error("passes_to_gray16: which " + std::to_string(which) + " is neither PTL_PASS_DEPTH (0) nor PTL_PASS_TRIPS (1)");
        return PTL_ERR_INVALID;
    }
    if (!records || !out_rows || n < 1 || n > (1L << 31)) return PTL_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(out_rows)) & 15u) return PTL_ERR_INVALID;
    void* args[] = {&records, &n, &out_rows, &which, &lo, &hi};
    return launch_over_records(device, "pass_gray16.hsaco", "ptl_passes_to_gray16_kernel", "passes_to_gray16", args, (n + 3) / 4, stream, elapsed_ms);  // a lane per four records
}

// The pass images of a clip's frame: the records of its N blur sub-frames merged per pixel into up to three grey images in one sweep
// (portal_amd/csrc/kernels/pass_slices_gray16.hip; the contract is in include/portal_amd.h).
extern "C" int ptl_pass_slices_to_gray16(int device, const void* records, int n_slices, unsigned long long slice_records, long n, void* out_depth, void* out_trips,
                                         void* out_cut, float lo, float hi, void* stream, float* elapsed_ms) {
    const auto refuse = [](const std::string& why) {
        set_last_error("pass_slices_to_gray16: " + why);
        return PTL_ERR_INVALID;
    };
    if (!records) return refuse("records is null");
    if (!out_depth && !out_trips && !out_cut) return refuse("none of out_depth, out_trips, out_cut is given");
    if ((reinterpret_cast<uintptr_t>(records) | reinterpret_cast<uintptr_t>(out_depth) | reinterpret_cast<uintptr_t>(out_trips) | reinterpret_cast<uintptr_t>(out_cut)) & 15u)
        return refuse("records and the outputs must be 16-byte aligned");
    if (n_slices < 1 || n_slices > kMaxSubframesTable) return refuse("n_slices " + std::to_string(n_slices) + " is outside 1 .. 256");
    if (n < 1 || n > (1L << 31)) return refuse("n " + std::to_string(n) + " is outside 1 .. 2^31");
    if (n_slices > 1 && slice_records < (unsigned long long)n) return refuse("slice_records " + std::to_string(slice_records) + " is less than n: the slices would overlap");
    void* args[] = {&records, &n_slices, &slice_records, &n, &out_depth, &out_trips, &out_cut, &lo, &hi};
    return launch_over_records(device, "pass_slices_gray16.hsaco", "ptl_pass_slices_to_gray16_kernel", "pass_slices_to_gray16", args, (n + 3) / 4, stream,
                               elapsed_ms);  // a lane per four pixels
}

// ptl_aa_edges: the classification pass of the adaptive anti-aliasing (portal_amd/csrc/kernels/aa_edges.hip; the contract is in
// include/portal_amd.h).  The count is reset on `stream` by the call itself; a 256-thread workgroup per 64x32 pixel region.
extern "C" int ptl_aa_edges(int device, const void* frame_rgba8, int width, int height, int threshold, void* list, void* count, void* stream,
                            float* elapsed_ms) {
    if (!frame_rgba8 || !list || !count || width <= 0 || height <= 0 || threshold < -1 || threshold > 255) return PTL_ERR_INVALID;
    if ((long long)width * height > (1LL << 31)) return PTL_ERR_INVALID;  // an entry is a 32-bit pixel index
    if ((reinterpret_cast<uintptr_t>(frame_rgba8) | reinterpret_cast<uintptr_t>(list) | reinterpret_cast<uintptr_t>(count)) & 3u) return PTL_ERR_INVALID;
    void* args[] = {&frame_rgba8, &width, &height, &threshold, &list, &count};
    return launch_aa_edges(device, "aa_edges.hsaco", "ptl_aa_edges_kernel", "aa_edges", args, count, 1, width, height, stream, elapsed_ms);
}

// ptl_aa_edges_slices: the same classification over a stack of `n` frames in one launch (portal_amd/csrc/kernels/aa_edges_slices.hip):
// slice z reads frames + z * slice_pixels pixels, appends to lists + z * list_stride entries and counts in counts[z].  counts[0 .. n) are
// reset on `stream` by the call itself.
extern "C" int ptl_aa_edges_slices(int device, const void* frames_rgba8, unsigned long long slice_pixels, int n, int width, int height, int threshold, void* lists,
                                   unsigned long long list_stride, void* counts, void* stream, float* elapsed_ms) {
    if (!frames_rgba8 || !lists || !counts || n < 1 || n > 16 || width <= 0 || height <= 0 || threshold < -1 || threshold > 255) return PTL_ERR_INVALID;
    if ((long long)width * height > (1LL << 31)) return PTL_ERR_INVALID;  // an entry is a 32-bit pixel index
    const unsigned long long pixels = (unsigned long long)width * (unsigned long long)height;
    if (slice_pixels < pixels || list_stride < pixels) return PTL_ERR_INVALID;  // a slice's frame and list hold a whole frame: neighbours never overlap
    if ((reinterpret_cast<uintptr_t>(frames_rgba8) | reinterpret_cast<uintptr_t>(lists) | reinterpret_cast<uintptr_t>(counts)) & 3u) return PTL_ERR_INVALID;
    if (device < 0) return PTL_ERR_NO_DEVICE;
    void* args[] = {&frames_rgba8, &slice_pixels, &width, &height, &threshold, &lists, &list_stride, &counts};
    return launch_aa_edges(device, "aa_edges_slices.hsaco", "ptl_aa_edges_slices_kernel", "aa_edges_slices", args, counts, n, width, height, stream, elapsed_ms);
}

extern "C" int ptl_y4m_header_chroma(int width, int height, int fps, int chroma, char* buf, size_t cap) {
    if (!known_chroma(chroma, "y4m_header") || width <= 0 || height <= 0 || fps <= 0 || !buf) return PTL_ERR_INVALID;
    int len = std::snprintf(buf, cap, "YUV4MPEG2 W%d H%d F%d:1 Ip A1:1 C%dp10 XYSCSS=%dP10 XCOLORRANGE=FULL\n", width, height, fps, chroma, chroma);
    return len > 0 && (size_t)len < cap ? len : PTL_ERR_INVALID;  // (the terminating NUL has to fit as well)
}
extern "C" int ptl_y4m_header(int width, int height, int fps, char* buf, size_t cap) { return ptl_y4m_header_chroma(width, height, fps, PTL_CHROMA_420, buf, cap); }

// Device frame buffers for callers that keep frames on the GPU between kernels (the video pipeline: sub-frames ->
// ptl_average_images -> one download).  The reference's counterpart is the macroquad render target and
// Texture2D::get_texture_data() (src/main.rs:1041-1042,1803-1816).
extern "C" int ptl_device_alloc(int device, size_t bytes, void** out) {
    if (!out || bytes == 0) return PTL_ERR_INVALID;
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    int e = rt->hipSetDevice(device);
    if (e == 0) e = rt->hipMalloc(out, bytes);
    if (e != 0) {
        set_last_error(std::string("hipMalloc: ") + rt->hipGetErrorString(e));
        return PTL_ERR_HIP;
    }
    return PTL_OK;
}

extern "C" int ptl_device_free(void* p) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    return rt->hipFree(p) == 0 ? PTL_OK : PTL_ERR_HIP;
}

extern "C" int ptl_device_download(void* host_dst, const void* device_src, size_t bytes, void* stream) {
    if (!host_dst || !device_src) return PTL_ERR_INVALID;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    int e = rt->hipMemcpyAsync(host_dst, device_src, bytes, hip::kMemcpyDeviceToHost, stream);
    if (e == 0) e = rt->hipStreamSynchronize(stream);
    if (e != 0) {
        set_last_error(std::string("hipMemcpy(D2H): ") + rt->hipGetErrorString(e));
        return PTL_ERR_HIP;
    }
    return PTL_OK;
}

// Page-locked host memory: a download into it runs at PCIe speed (a 4K RGBA8 frame in < 1 ms instead of ~10 ms pageable).
extern "C" int ptl_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return PTL_ERR_INVALID;
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    int e = rt->hipHostMalloc(out, bytes, 0);
    if (e != 0) {
        set_last_error(std::string("hipHostMalloc: ") + rt->hipGetErrorString(e));
        rt->hipGetLastError();
        return PTL_ERR_HIP;
    }
    return PTL_OK;
}

extern "C" int ptl_host_free(void* p) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    return rt->hipHostFree(p) == 0 ? PTL_OK : PTL_ERR_HIP;
}

// Streams and events for callers that overlap downloads with tracing (the video pipeline: the copy of frame i runs on its
// own stream while frame i+1 is traced).  Thin, 1:1 over HIP; a stream is created non-blocking (no implicit ordering
// against the default stream), an event without timing.
namespace {
int hip_status(const hip::Runtime* rt, int e, const char* what) {
    if (e == 0) return PTL_OK;
    set_last_error(std::string(what) + ": " + rt->hipGetErrorString(e));
    rt->hipGetLastError();
    return PTL_ERR_HIP;
}
}  // namespace

extern "C" int ptl_stream_create(int device, void** stream) {
    if (!stream) return PTL_ERR_INVALID;
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    int e = rt->hipSetDevice(device);
    if (e == 0) e = rt->hipStreamCreateWithFlags(stream, hip::kStreamNonBlocking);
    return hip_status(rt, e, "hipStreamCreate");
}
extern "C" int ptl_stream_destroy(void* stream) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    return rt ? hip_status(rt, rt->hipStreamDestroy(stream), "hipStreamDestroy") : PTL_ERR_NO_DEVICE;
}
extern "C" int ptl_event_create(int device, void** event) {
    if (!event) return PTL_ERR_INVALID;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    int e = rt->hipSetDevice(device);
    if (e == 0) e = rt->hipEventCreateWithFlags(event, hip::kEventDisableTiming);
    return hip_status(rt, e, "hipEventCreate");
}
extern "C" int ptl_event_destroy(void* event) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    return rt ? hip_status(rt, rt->hipEventDestroy(event), "hipEventDestroy") : PTL_ERR_NO_DEVICE;
}
extern "C" int ptl_event_record(void* event, void* stream) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    return rt ? hip_status(rt, rt->hipEventRecord(event, stream), "hipEventRecord") : PTL_ERR_NO_DEVICE;
}
extern "C" int ptl_event_synchronize(void* event) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    return rt ? hip_status(rt, rt->hipEventSynchronize(event), "hipEventSynchronize") : PTL_ERR_NO_DEVICE;
}
extern "C" int ptl_stream_wait_event(void* stream, void* event) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    return rt ? hip_status(rt, rt->hipStreamWaitEvent(stream, event, 0), "hipStreamWaitEvent") : PTL_ERR_NO_DEVICE;
}
extern "C" int ptl_device_memset(void* device_dst, int value, size_t bytes, void* stream) {
    if (!device_dst) return PTL_ERR_INVALID;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    return hip_status(rt, rt->hipMemsetAsync(device_dst, value, bytes, stream), "hipMemsetAsync");
}
extern "C" int ptl_device_download_async(void* host_dst, const void* device_src, size_t bytes, void* stream) {
    if (!host_dst || !device_src) return PTL_ERR_INVALID;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    return hip_status(rt, rt->hipMemcpyAsync(host_dst, device_src, bytes, hip::kMemcpyDeviceToHost, stream), "hipMemcpyAsync(D2H)");
}

// A strided device-to-device copy on `stream` (hipMemcpy2DAsync, direction from the pointers): `rows` rows of `width_bytes`, source
// and destination pitches in bytes.  With a packed shard as the source (pitch = one 8-row block) and another GPU's frame as the
// destination (pitch = G blocks, mapped through ptl_ipc_open or peer access) ONE such copy gathers a rank's shard over its xGMI link
// with the SDMA engine and de-interleaves it in the same transfer.
extern "C" int ptl_device_copy2d_async(void* dst, size_t dst_pitch, const void* src, size_t src_pitch, size_t width_bytes, size_t rows, void* stream) {
    if (!dst || !src || width_bytes == 0 || dst_pitch < width_bytes || src_pitch < width_bytes) return PTL_ERR_INVALID;
    if (rows == 0) return PTL_OK;
    const hip::Runtime* rt = hip::runtime(nullptr);
    if (!rt) return PTL_ERR_NO_DEVICE;
    return hip_status(rt, rt->hipMemcpy2DAsync(dst, dst_pitch, src, src_pitch, width_bytes, rows, hip::kMemcpyDefault, stream), "hipMemcpy2DAsync");
}

// Frame buffers shared between the processes of a node (one process per GPU): the destination rank allocates the full frame
// with ptl_device_alloc, exports it, and every other rank maps it into its own address space; their render kernels then store
// their row blocks straight into the destination GPU's HBM over xGMI (ptl_frame.in_place), no gather, no de-interleave copy.
// 1:1 over hipIpcGetMemHandle / hipIpcOpenMemHandle / hipIpcCloseMemHandle.  The pointer must come from ptl_device_alloc
// (a whole hipMalloc allocation), and a handle cannot be opened by the process that exported it.
extern "C" int ptl_ipc_export(void* device_ptr, unsigned char handle[PTL_IPC_HANDLE_BYTES]) {
    if (!device_ptr || !handle) return PTL_ERR_INVALID;
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    hip::IpcMemHandle h;
    static_assert(sizeof h == PTL_IPC_HANDLE_BYTES, "hipIpcMemHandle_t is 64 bytes");
    int e = rt->hipIpcGetMemHandle(&h, device_ptr);
    if (e == 0) std::memcpy(handle, &h, sizeof h);
    return hip_status(rt, e, "hipIpcGetMemHandle");
}

extern "C" int ptl_ipc_open(int device, const unsigned char handle[PTL_IPC_HANDLE_BYTES], void** device_ptr) {
    if (!handle || !device_ptr) return PTL_ERR_INVALID;
    std::string err;
    const hip::Runtime* rt = hip::runtime(&err);
    if (!rt) {
        set_last_error(err);
        return PTL_ERR_NO_DEVICE;
    }
    hip::IpcMemHandle h;
    std::memcpy(&h, handle, sizeof h);
    int e = rt->hipSetDevice(device);
    if (e == 0) e = rt->hipIpcOpenMemHandle(device_ptr, h, hip::kIpcMemLazyEnablePeerAccess);
    return hip_status(rt, e, "hipIpcOpenMemHandle");
}

extern "C" int ptl_ipc_close(void* device_ptr) {
    const hip::Runtime* rt = hip::runtime(nullptr);
    return rt ? hip_status(rt, rt->hipIpcCloseMemHandle(device_ptr), "hipIpcCloseMemHandle") : PTL_ERR_NO_DEVICE;
}
