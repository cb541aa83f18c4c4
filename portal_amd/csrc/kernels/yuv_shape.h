// yuv_shape.h -- the shape of the planar Y'CbCr 10-bit hand-off, stated once for the kernels' dispatcher (yuv_common.h) and for the host
// that sizes their launches (postprocess.cpp): what a sampling is, which frames take the fast path, and how many lanes a frame needs.
// Plain constexpr C++, no HIP.  `chroma` is 420, 422 or 444 (PTL_CHROMA_*); `f32` says that the sub-frames are RGBA32F, not RGBA8.
#pragma once

// A sampling: the tap window of a chroma sample (columns 2i-1, 2i, 2i+1 weighted 1-2-1, or the pixel itself; one row or two), log2 of the
// window's weights (8, 4, 1), and the chroma plane's size.
constexpr int ptl_yuv_tap_cols(int chroma) { return chroma == 444 ? 1 : 3; }
constexpr int ptl_yuv_tap_rows(int chroma) { return chroma == 420 ? 2 : 1; }
constexpr int ptl_yuv_shift(int chroma) { return chroma == 420 ? 3 : chroma == 422 ? 2 : 0; }
constexpr unsigned int ptl_yuv_cw(int chroma, unsigned int w) { return chroma == 444 ? w : (w + 1u) >> 1; }
constexpr unsigned int ptl_yuv_ch(int chroma, unsigned int h) { return chroma == 420 ? (h + 1u) >> 1 : h; }

// A sub-frame is addressed with 32-bit byte offsets: W*H is at most this (4 and 16 bytes per pixel).
constexpr long ptl_yuv_max_pixels(bool f32) { return f32 ? 1L << 28 : 1L << 29; }

// The fast path: a lane owns a block of cols x rows pixels where the frame is made of whole blocks (and, for RGBA8 4:2:0, of whole
// pairs of them: W % 16 == 0).  Everything else goes through the general path, a lane per chroma sample.
//   RGBA8 4:2:0  8x2      RGBA8 4:2:2 / 4:4:4  8x1      float 4:2:0  2x2      float 4:2:2 / 4:4:4  4x1
constexpr unsigned int ptl_yuv_block_cols(bool f32, int chroma) { return !f32 ? 8u : chroma == 420 ? 2u : 4u; }
constexpr unsigned int ptl_yuv_block_rows(int chroma) { return chroma == 420 ? 2u : 1u; }
constexpr bool ptl_yuv_fast(bool f32, int chroma, unsigned int w, unsigned int h) {
    return w % (!f32 && chroma == 420 ? 16u : ptl_yuv_block_cols(f32, chroma)) == 0u && h % ptl_yuv_block_rows(chroma) == 0u;
}
constexpr unsigned int ptl_yuv_lanes(bool f32, int chroma, unsigned int w, unsigned int h) {
    return ptl_yuv_fast(f32, chroma, w, h) ? (w / ptl_yuv_block_cols(f32, chroma)) * (h / ptl_yuv_block_rows(chroma)) : ptl_yuv_cw(chroma, w) * ptl_yuv_ch(chroma, h);
}
