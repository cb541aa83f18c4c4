// cli_png.h -- how drawn sub-frames become ONE PNG file: the form `render-frame` (one sub-frame, deflate level 6) and the PNG frames of
// `render` (--motion-blur-frames sub-frames, level 3) share, and the only place that knows there are four of them:
//   host, 8 bits   the RGBA8 sub-frames averaged (ptl_average_images; one sub-frame IS the result: no kernel), deflated by zlib
//   host, 16 bits  --png-depth 16: the float sub-frames averaged into the file's Sub-filtered scanlines (ptl_average_f32_to_rgb48), deflated by zlib
//   gpu, 8 bits    --png-encoder gpu: the averaged frame deflated on the card (ptl_png_deflate_rgba8, or _codes with --png-codes dynamic); the host
//                  only frames the stream (ptl_png_write_stream)
//   gpu, 16 bits   --png-depth 16 --png16-encoder gpu: the float sub-frames averaged into unfiltered 16-bit rows, those deflated on the card
//                  (ptl_png_deflate_rgb48: Up filter, matches at pixel distance, a Huffman code per band); the host frames the stream
#pragma once

#include "cli_common.h"

struct PngForm {
    explicit PngForm(const Options& o) : sixteen(o.png_depth == 16), gpu(sixteen ? o.png16_gpu : o.png_gpu), codes(o.png_codes) {}
    const bool sixteen, gpu;
    const int codes;  // gpu, 8 bits: PTL_PNG_CODES_FIXED or _DYNAMIC

    bool wants_float() const { return sixteen; }  // the sub-frames are also drawn as RGBA32F: make() reads those
    // a frame of ONE sub-frame that needs no kernel: the RGBA8 sub-frame is the result, make() is not called
    bool draws_result(int n) const { return !sixteen && !gpu && n == 1; }
    const char* deflate_name() const { return sixteen ? "png_deflate_rgb48" : "png_deflate_rgba8"; }  // gpu: the C ABI entry whose result buffer make() fills
    size_t result_bytes(int width, int height) const {  // the result buffer on the card
        if (gpu) return sixteen ? ptl_png_stream16_bytes(width, height) : ptl_png_stream_bytes(width, height);
        return sixteen ? ptl_rgb48_frame_bytes(width, height) : (size_t)width * height * 4;
    }
    // what of it leaves the card in a clip: of a deflate result the header and the room for the stream, not the kernels' scratch behind them
    // (a still downloads the header first, then exactly the stream it announces; for a clip that is a follow-up)
    size_t download_bytes(int width, int height) const {
        if (gpu) return sixteen ? ptl_png_stream16_download_bytes(width, height) : ptl_png_stream_download_bytes(width, height);
        return result_bytes(width, height);
    }
    size_t staging_bytes(int width, int height, int n) const {  // gpu: the averaged frame the deflate reads (8 bits, one sub-frame: deflated where it was drawn)
        if (!gpu) return 0;
        return sixteen ? ptl_rgb48_frame_bytes(width, height) : n > 1 ? (size_t)width * height * 4 : 0;
    }
    // The device step, on the default stream: `n` sub-frames (`rgba8`, and `rgba32f` where wants_float()) into `result`, through `staging`.
    // Timed where a pointer is given: the averaging kernel and the deflate apart.  0, or 1 after "<kernel>: <error>"
    int make(int device, const void* const* rgba8, const void* const* rgba32f, int n, void* staging, void* result, int width, int height, float* average_ms, float* deflate_ms) const {
        if (sixteen) {
            if (ptl_average_f32_to_rgb48(device, rgba32f, n, gpu ? staging : result, width, height, gpu ? PTL_PNG_FILTER_NONE : PTL_PNG_FILTER_SUB, nullptr, average_ms) != PTL_OK)
                return fail("average_f32_to_rgb48");
            if (gpu && ptl_png_deflate_rgb48(device, staging, width, height, PTL_PNG_CODES_DYNAMIC, result, nullptr, deflate_ms) != PTL_OK) return fail("png_deflate_rgb48");
            return 0;
        }
        const void* frame = rgba8[0];
        if (n > 1) {
            frame = gpu ? staging : result;
            if (ptl_average_images(device, rgba8, n, gpu ? staging : result, width, height, nullptr, average_ms) != PTL_OK) return fail("average_images");
        }
        if (gpu && (codes == PTL_PNG_CODES_FIXED ? ptl_png_deflate_rgba8(device, frame, width, height, result, nullptr, deflate_ms)
                                                 : ptl_png_deflate_rgba8_codes(device, frame, width, height, codes, result, nullptr, deflate_ms)) != PTL_OK)
            return fail("png_deflate_rgba8");
        return 0;
    }
    // The host step: the downloaded bytes as the file `path`.  PTL_OK, or the error (ptl_last_error())
    int write(const char* path, const uint8_t* bytes, int width, int height, int level) const {
        if (gpu) return sixteen ? ptl_png_write_stream_rgb48(path, bytes, width, height) : ptl_png_write_stream(path, bytes, width, height);
        return sixteen ? ptl_png_write_rgb48(path, bytes, width, height, PTL_PNG_FILTER_SUB, level) : ptl_png_write_level(path, bytes, width, height, level);
    }
};
