// png_deflate_shape.h -- the shape of the GPU deflate of a PNG frame, stated once for the kernels (png_deflate.hip, png_huffman.hip), for the
// host that sizes the result buffer and the launch (postprocess.cpp) and for the writer that checks a result's header (png_io.cpp): the cut
// of the raw scanlines into bands and segments, the bound of a band's slot, and the layout of the result buffer, as functions of the bytes
// of a pixel -- 4: an RGBA8 frame, 6: the RGB rows of 16-bit samples.  Plain constexpr C++, no HIP.  The stream contracts themselves are the
// header comments of ptl_png_deflate_rgba8 and ptl_png_deflate_rgb48 in include/portal_amd.h.
#pragma once

typedef unsigned long long ptl_png_u64;

constexpr unsigned int ptl_png_segment_bytes = 4096u;  // runs never cross a multiple of this inside a band: 255 * 4096 * 4097 / 2 < 2^32
constexpr unsigned int ptl_png_band_target = 16384u;   // a band is as many whole rows as fit into this many raw bytes, at least one
constexpr unsigned int ptl_png_header_bytes = 64u;     // sixteen little-endian uint32 in front of the stream
constexpr unsigned int ptl_png_table_entry_bytes = 16u;  // per band: bytes used, Adler s1, Adler s2, raw bytes
constexpr unsigned int ptl_png_adler_mod = 65521u;
constexpr unsigned int ptl_png_pixel8 = 4u, ptl_png_pixel16 = 6u;  // the bytes of a pixel; a 16-bit pixel is three big-endian samples
// Word 0 of the header, "PTLZ" or "PTL6"; words 1 .. 6: W, H, stream bytes, Adler-32, rows per band, bands.
constexpr unsigned int ptl_png_magic(unsigned int pixel) { return pixel == ptl_png_pixel16 ? 0x364c5450u : 0x5a4c5450u; }

// The raw scanlines are addressed with 32-bit offsets: H (pixel W + 1) is at most this.  The 16-bit rows are those of
// ptl_average_f32_to_rgb48, at most 2^28 pixels.
constexpr ptl_png_u64 ptl_png_max_raw_bytes() { return 1ull << 31; }
constexpr ptl_png_u64 ptl_png_row_bytes(unsigned int pixel, unsigned int w) { return (ptl_png_u64)pixel * w + 1ull; }
constexpr ptl_png_u64 ptl_png_raw_bytes(unsigned int pixel, unsigned int w, unsigned int h) { return ptl_png_row_bytes(pixel, w) * h; }
constexpr bool ptl_png_fits(unsigned int pixel, unsigned int w, unsigned int h) {
    return w >= 1u && h >= 1u && (pixel == ptl_png_pixel16 ? (ptl_png_u64)w * h <= (1ull << 28) : w <= (1u << 29)) && ptl_png_raw_bytes(pixel, w, h) <= ptl_png_max_raw_bytes();
}

constexpr unsigned int ptl_png_band_rows(unsigned int pixel, unsigned int w) {
    return ptl_png_row_bytes(pixel, w) >= ptl_png_band_target ? 1u : (unsigned int)(ptl_png_band_target / ptl_png_row_bytes(pixel, w));
}
constexpr unsigned int ptl_png_bands(unsigned int pixel, unsigned int w, unsigned int h) { return (h + ptl_png_band_rows(pixel, w) - 1u) / ptl_png_band_rows(pixel, w); }
constexpr ptl_png_u64 ptl_png_full_band_bytes(unsigned int pixel, unsigned int w) { return ptl_png_band_rows(pixel, w) * ptl_png_row_bytes(pixel, w); }

// A token never costs more than 9 bits per raw byte it covers (a fixed-code match: at most 8 + 5 bits and a distance of 5 bits, or of 5 and
// an extra bit at distance 6, for at least 3 bytes); a band adds its 3-bit block header, 7 bits of end-of-block, the 3-bit header of the
// empty stored block, at most 7 bits of padding and the four bytes 00 00 FF FF.
constexpr ptl_png_u64 ptl_png_band_capacity(ptl_png_u64 n) { return (9ull * n + 20ull + 7ull) / 8ull + 4ull; }
// A band's slot: the bound of a full band, rounded up so that every slot starts 16-byte aligned.
constexpr ptl_png_u64 ptl_png_slot_stride(unsigned int pixel, unsigned int w) { return (ptl_png_band_capacity(ptl_png_full_band_bytes(pixel, w)) + 15ull) & ~15ull; }
// The longest the packed stream (the bands, one behind the other) can get.
constexpr ptl_png_u64 ptl_png_stream_capacity(unsigned int pixel, unsigned int w, unsigned int h) {
    const ptl_png_u64 full = ptl_png_full_band_bytes(pixel, w);
    const unsigned int bands = ptl_png_bands(pixel, w, h);
    return (bands - 1u) * ptl_png_band_capacity(full) + ptl_png_band_capacity(ptl_png_raw_bytes(pixel, w, h) - (bands - 1u) * full);
}
// The result buffer: header | stream (room for its capacity, rounded up to 16) | table, one entry per band | slots, one per band.
constexpr ptl_png_u64 ptl_png_table_offset(unsigned int pixel, unsigned int w, unsigned int h) {
    return ptl_png_header_bytes + ((ptl_png_stream_capacity(pixel, w, h) + 15ull) & ~15ull);
}
constexpr ptl_png_u64 ptl_png_slots_offset(unsigned int pixel, unsigned int w, unsigned int h) {
    return ptl_png_table_offset(pixel, w, h) + (ptl_png_u64)ptl_png_table_entry_bytes * ptl_png_bands(pixel, w, h);
}
constexpr ptl_png_u64 ptl_png_result_bytes(unsigned int pixel, unsigned int w, unsigned int h) {
    return ptl_png_slots_offset(pixel, w, h) + ptl_png_slot_stride(pixel, w) * ptl_png_bands(pixel, w, h);
}

// x - y in each of the four bytes of a dword, mod 256, no borrow from one byte into the next (the Up filter on a whole 8-bit pixel): the low
// seven bits of every byte are subtracted with bit 7 of x forced on, then bit 7 is put right.
constexpr unsigned int ptl_png_sub_bytes(unsigned int x, unsigned int y) { return ((x | 0x80808080u) - (y & 0x7f7f7f7fu)) ^ ((x ^ ~y) & 0x80808080u); }
// The same in each of the two bytes of a 16-bit sample as it lies in memory.
constexpr unsigned int ptl_png_sub_bytes16(unsigned int x, unsigned int y) { return ((x - (y & 0x00ffu)) & 0x00ffu) | ((x - (y & 0xff00u)) & 0xff00u); }

static_assert(ptl_png_sub_bytes(0x01000100u, 0x00ff00ffu) == 0x01010101u && ptl_png_sub_bytes(0x00000000u, 0xffffffffu) == 0x01010101u, "");
static_assert(ptl_png_sub_bytes(0x00ff80ffu, 0xff008000u) == 0x01ff00ffu && ptl_png_sub_bytes(0x12345678u, 0u) == 0x12345678u, "");
static_assert(ptl_png_sub_bytes16(0x0100u, 0x00ffu) == 0x0101u && ptl_png_sub_bytes16(0x0000u, 0xffffu) == 0x0101u && ptl_png_sub_bytes16(0xff00u, 0x00ffu) == 0xff01u, "");
static_assert(255ull * ptl_png_segment_bytes * (ptl_png_segment_bytes + 1ull) / 2ull < (1ull << 32), "a segment's Adler sums stay within 32 bits");
static_assert(ptl_png_band_rows(4u, 3840u) == 1u && ptl_png_band_rows(4u, 640u) == 6u && ptl_png_band_rows(4u, 1u) == 3276u, "");
static_assert(ptl_png_band_rows(6u, 3840u) == 1u && ptl_png_band_rows(6u, 640u) == 4u && ptl_png_band_rows(6u, 1u) == 2340u && ptl_png_band_rows(6u, 2731u) == 1u, "");
static_assert(ptl_png_fits(6u, 1u << 14, 1u << 14) && !ptl_png_fits(6u, (1u << 14) + 1u, 1u << 14) && ptl_png_fits(6u, 1u, 1u << 28) && !ptl_png_fits(6u, 1u, (1u << 28) + 1u), "");
static_assert(ptl_png_fits(4u, (1u << 29) - 1u, 1u) && !ptl_png_fits(4u, 1u << 29, 1u) && !ptl_png_fits(4u, 1u << 15, 1u << 15), "");
static_assert(ptl_png_band_capacity(1u) == 8u && ptl_png_slot_stride(4u, 1u) % 16u == 0u && ptl_png_slot_stride(6u, 1u) % 16u == 0u, "");
static_assert(8u + 5u + 5u <= 9u * 3u && 8u + 5u + 5u + 1u <= 9u * 3u, "the bound of a band holds at both distances");
