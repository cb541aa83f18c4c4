// rgb48_shape.h -- the shape of the 16-bit RGB hand-off (PNG colour type 2, bit depth 16), stated once for the kernel (rgb48_f32.hip) and
// for the host that sizes its launch (postprocess.cpp): which frames take the fast path, how many lanes a frame needs, and the two byte
// transforms of a scanline -- the per-byte difference of PNG's Sub filter and the byte order of a sample.  Plain constexpr C++, no HIP; the
// byte transforms are checked below, at compile time, on the pairs where a borrow between bytes would show.
#pragma once

// `filter` of ptl_average_f32_to_rgb48 and ptl_png_write_rgb48 (PTL_PNG_FILTER_* in include/portal_amd.h): PNG's filter types 0 and 1.
constexpr int ptl_rgb48_filter_none = 0, ptl_rgb48_filter_sub = 1;
constexpr bool ptl_rgb48_is_filter(int filter) { return filter == ptl_rgb48_filter_none || filter == ptl_rgb48_filter_sub; }

// A sub-frame is addressed with 32-bit byte offsets, 16 bytes per pixel: W*H is at most this (6 W*H output bytes fit 32 bits as well).
constexpr long ptl_rgb48_max_pixels() { return 1L << 28; }

// The fast path: a lane owns 4x1 pixels = 24 output bytes where a row is made of whole blocks (rows then start 8-byte aligned).
// Everything else goes through the general path, a lane per pixel.
constexpr unsigned int ptl_rgb48_block_cols() { return 4u; }
constexpr bool ptl_rgb48_fast(unsigned int w) { return w % ptl_rgb48_block_cols() == 0u; }
constexpr unsigned int ptl_rgb48_lanes(unsigned int w, unsigned int h) { return ptl_rgb48_fast(w) ? (w / ptl_rgb48_block_cols()) * h : w * h; }

// x - y in each of the four bytes of a dword, mod 256, no borrow from one byte into the next: the low seven bits of every byte are
// subtracted with bit 7 of x forced on (so no byte borrows from its neighbour), then bit 7 is put right.
constexpr unsigned int ptl_rgb48_sub_bytes(unsigned int x, unsigned int y) {
    return ((x | 0x80808080u) - (y & 0x7f7f7f7fu)) ^ ((x ^ ~y) & 0x80808080u);
}
// Two 16-bit samples in a dword, each with its bytes exchanged: stored little-endian they lie in memory high byte first, as PNG wants them.
constexpr unsigned int ptl_rgb48_swap16(unsigned int v) { return ((v & 0x00ff00ffu) << 8) | ((v >> 8) & 0x00ff00ffu); }

static_assert(ptl_rgb48_sub_bytes(0x01000100u, 0x00ff00ffu) == 0x01010101u, "0x00ff -> 0x0100: high byte +1, low byte 0x00 - 0xff = 0x01");
static_assert(ptl_rgb48_sub_bytes(0x00000000u, 0xffffffffu) == 0x01010101u, "0xffff -> 0x0000");
static_assert(ptl_rgb48_sub_bytes(0xff00ff00u, 0x00ff00ffu) == 0xff01ff01u, "0x00ff -> 0xff00");
static_assert(ptl_rgb48_sub_bytes(0x00ff80ffu, 0xff008000u) == 0x01ff00ffu && ptl_rgb48_sub_bytes(0x12345678u, 0u) == 0x12345678u, "");
static_assert(ptl_rgb48_swap16(0x12345678u) == 0x34127856u, "");
