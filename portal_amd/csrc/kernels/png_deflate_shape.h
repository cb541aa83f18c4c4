// png_deflate_shape.h -- the shape of the GPU deflate of an 8-bit PNG frame, stated once for the kernels (png_deflate.hip), for the host that
// sizes the result buffer and the launch (postprocess.cpp) and for the writer that checks a result's header (png_io.cpp): the cut of the raw
// scanlines into bands and segments, the bound of a band's slot, and the layout of the result buffer.  Plain constexpr C++, no HIP.  The
// stream contract itself is the header comment of ptl_png_deflate_rgba8 in include/portal_amd.h.
#pragma once

typedef unsigned long long ptl_png_u64;

constexpr unsigned int ptl_png_segment_bytes = 4096u;  // runs never cross a multiple of this inside a band: 255 * 4096 * 4097 / 2 < 2^32
constexpr unsigned int ptl_png_band_target = 16384u;   // a band is as many whole rows as fit into this many raw bytes, at least one
constexpr unsigned int ptl_png_header_bytes = 64u;     // sixteen little-endian uint32 in front of the stream
constexpr unsigned int ptl_png_magic = 0x5a4c5450u;    // "PTLZ", word 0 of the header; words 1 .. 6: W, H, stream bytes, Adler-32, rows per band, bands
constexpr unsigned int ptl_png_table_entry_bytes = 16u;  // per band: bytes used, Adler s1, Adler s2, raw bytes
constexpr unsigned int ptl_png_adler_mod = 65521u;

// The raw scanlines are addressed with 32-bit offsets: H (4 W + 1) is at most this.
constexpr ptl_png_u64 ptl_png_max_raw_bytes() { return 1ull << 31; }
constexpr ptl_png_u64 ptl_png_row_bytes(unsigned int w) { return 4ull * w + 1ull; }
constexpr ptl_png_u64 ptl_png_raw_bytes(unsigned int w, unsigned int h) { return ptl_png_row_bytes(w) * h; }
constexpr bool ptl_png_fits(unsigned int w, unsigned int h) { return w >= 1u && h >= 1u && w <= (1u << 29) && ptl_png_raw_bytes(w, h) <= ptl_png_max_raw_bytes(); }

constexpr unsigned int ptl_png_band_rows(unsigned int w) {
    return ptl_png_row_bytes(w) >= ptl_png_band_target ? 1u : (unsigned int)(ptl_png_band_target / ptl_png_row_bytes(w));
}
constexpr unsigned int ptl_png_bands(unsigned int w, unsigned int h) { return (h + ptl_png_band_rows(w) - 1u) / ptl_png_band_rows(w); }

// A token never costs more than 9 bits per raw byte it covers (a match: at most 18 bits for at least 3 bytes); a band adds its 3-bit block
// header, 7 bits of end-of-block, the 3-bit header of the empty stored block, at most 7 bits of padding and the four bytes 00 00 FF FF.
constexpr ptl_png_u64 ptl_png_band_capacity(ptl_png_u64 n) { return (9ull * n + 20ull + 7ull) / 8ull + 4ull; }
// A band's slot: the bound of a full band, rounded up so that every slot starts 16-byte aligned.
constexpr ptl_png_u64 ptl_png_slot_stride(unsigned int w) { return (ptl_png_band_capacity(ptl_png_band_rows(w) * ptl_png_row_bytes(w)) + 15ull) & ~15ull; }
// The longest the packed stream (the bands, one behind the other) can get.
constexpr ptl_png_u64 ptl_png_stream_capacity(unsigned int w, unsigned int h) {
    const ptl_png_u64 full = ptl_png_band_rows(w) * ptl_png_row_bytes(w);
    const unsigned int bands = ptl_png_bands(w, h);
    return (bands - 1u) * ptl_png_band_capacity(full) + ptl_png_band_capacity(ptl_png_raw_bytes(w, h) - (bands - 1u) * full);
}
// The result buffer: header | stream (room for its capacity, rounded up to 16) | table, one entry per band | slots, one per band.
constexpr ptl_png_u64 ptl_png_table_offset(unsigned int w, unsigned int h) { return ptl_png_header_bytes + ((ptl_png_stream_capacity(w, h) + 15ull) & ~15ull); }
constexpr ptl_png_u64 ptl_png_slots_offset(unsigned int w, unsigned int h) { return ptl_png_table_offset(w, h) + (ptl_png_u64)ptl_png_table_entry_bytes * ptl_png_bands(w, h); }
constexpr ptl_png_u64 ptl_png_result_bytes(unsigned int w, unsigned int h) { return ptl_png_slots_offset(w, h) + ptl_png_slot_stride(w) * ptl_png_bands(w, h); }

// x - y in each of the four bytes of a dword, mod 256, no borrow from one byte into the next (the Up filter on a whole pixel): the low seven
// bits of every byte are subtracted with bit 7 of x forced on, then bit 7 is put right.
constexpr unsigned int ptl_png_sub_bytes(unsigned int x, unsigned int y) { return ((x | 0x80808080u) - (y & 0x7f7f7f7fu)) ^ ((x ^ ~y) & 0x80808080u); }

static_assert(ptl_png_sub_bytes(0x01000100u, 0x00ff00ffu) == 0x01010101u && ptl_png_sub_bytes(0x00000000u, 0xffffffffu) == 0x01010101u, "");
static_assert(ptl_png_sub_bytes(0x00ff80ffu, 0xff008000u) == 0x01ff00ffu && ptl_png_sub_bytes(0x12345678u, 0u) == 0x12345678u, "");
static_assert(255ull * ptl_png_segment_bytes * (ptl_png_segment_bytes + 1ull) / 2ull < (1ull << 32), "a segment's Adler sums stay within 32 bits");
static_assert(ptl_png_band_rows(3840u) == 1u && ptl_png_band_rows(640u) == 6u && ptl_png_band_rows(1u) == 3276u, "");
static_assert(ptl_png_band_capacity(1u) == 8u && ptl_png_slot_stride(1u) % 16u == 0u, "");
