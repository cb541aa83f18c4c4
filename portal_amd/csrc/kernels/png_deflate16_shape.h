// png_deflate16_shape.h -- the shape of the GPU deflate of a 16-bit PNG frame, stated once for the kernels (png_deflate16.hip), for the host
// that sizes the result buffer and the launch (postprocess.cpp) and for the writer that checks a result's header (png_io.cpp).  Segments, the
// band target, the bound of a band, the 64-byte header and the table entry are png_deflate_shape.h's; what differs is the row -- 6 W bytes
// behind its filter-type byte -- and with it the band cut, the sizes, and the header's magic word.  Plain constexpr C++, no HIP.  The stream
// contract itself is the header comment of ptl_png_deflate_rgb48 in include/portal_amd.h.
#pragma once

#include "png_deflate_shape.h"

constexpr unsigned int ptl_png16_magic = 0x364c5450u;  // "PTL6", word 0 of the header; words 1 .. 6 as in png_deflate_shape.h
constexpr unsigned int ptl_png16_distance = 6u;        // a pixel: three big-endian 16-bit samples; every match is at this distance

// The rows are those of ptl_average_f32_to_rgb48 (at most 2^28 pixels); the raw scanlines are addressed with 32-bit offsets.
constexpr ptl_png_u64 ptl_png16_row_bytes(unsigned int w) { return 6ull * w + 1ull; }
constexpr ptl_png_u64 ptl_png16_raw_bytes(unsigned int w, unsigned int h) { return ptl_png16_row_bytes(w) * h; }
constexpr bool ptl_png16_fits(unsigned int w, unsigned int h) {
    return w >= 1u && h >= 1u && (ptl_png_u64)w * h <= (1ull << 28) && ptl_png16_raw_bytes(w, h) <= ptl_png_max_raw_bytes();
}

constexpr unsigned int ptl_png16_band_rows(unsigned int w) {
    return ptl_png16_row_bytes(w) >= ptl_png_band_target ? 1u : (unsigned int)(ptl_png_band_target / ptl_png16_row_bytes(w));
}
constexpr unsigned int ptl_png16_bands(unsigned int w, unsigned int h) { return (h + ptl_png16_band_rows(w) - 1u) / ptl_png16_band_rows(w); }

// A fixed-code match costs at most 8 + 5 + 5 + 1 bits for at least 3 bytes, a literal at most 9: ptl_png_band_capacity holds as it is.
constexpr ptl_png_u64 ptl_png16_slot_stride(unsigned int w) { return (ptl_png_band_capacity(ptl_png16_band_rows(w) * ptl_png16_row_bytes(w)) + 15ull) & ~15ull; }
constexpr ptl_png_u64 ptl_png16_stream_capacity(unsigned int w, unsigned int h) {
    const ptl_png_u64 full = ptl_png16_band_rows(w) * ptl_png16_row_bytes(w);
    const unsigned int bands = ptl_png16_bands(w, h);
    return (bands - 1u) * ptl_png_band_capacity(full) + ptl_png_band_capacity(ptl_png16_raw_bytes(w, h) - (bands - 1u) * full);
}
// The result buffer: header | stream (room for its capacity, rounded up to 16) | table, one entry per band | slots, one per band.
constexpr ptl_png_u64 ptl_png16_table_offset(unsigned int w, unsigned int h) { return ptl_png_header_bytes + ((ptl_png16_stream_capacity(w, h) + 15ull) & ~15ull); }
constexpr ptl_png_u64 ptl_png16_slots_offset(unsigned int w, unsigned int h) { return ptl_png16_table_offset(w, h) + (ptl_png_u64)ptl_png_table_entry_bytes * ptl_png16_bands(w, h); }
constexpr ptl_png_u64 ptl_png16_result_bytes(unsigned int w, unsigned int h) { return ptl_png16_slots_offset(w, h) + ptl_png16_slot_stride(w) * ptl_png16_bands(w, h); }

// x - y in each of the two bytes of a 16-bit sample as it lies in memory, mod 256, no borrow from one byte into the other (the Up filter).
constexpr unsigned int ptl_png16_sub_bytes(unsigned int x, unsigned int y) { return ((x - (y & 0x00ffu)) & 0x00ffu) | ((x - (y & 0xff00u)) & 0xff00u); }

static_assert(ptl_png16_sub_bytes(0x0100u, 0x00ffu) == 0x0101u && ptl_png16_sub_bytes(0x0000u, 0xffffu) == 0x0101u && ptl_png16_sub_bytes(0xff00u, 0x00ffu) == 0xff01u, "");
static_assert(ptl_png16_band_rows(3840u) == 1u && ptl_png16_band_rows(640u) == 4u && ptl_png16_band_rows(1u) == 2340u && ptl_png16_band_rows(2731u) == 1u, "");
static_assert(ptl_png16_fits(1u << 14, 1u << 14) && !ptl_png16_fits((1u << 14) + 1u, 1u << 14) && ptl_png16_fits(1u, 1u << 28) && !ptl_png16_fits(1u, (1u << 28) + 1u), "");
static_assert(ptl_png16_slot_stride(1u) % 16u == 0u && (8u + 5u + 5u + 1u) <= 9u * 3u, "");
