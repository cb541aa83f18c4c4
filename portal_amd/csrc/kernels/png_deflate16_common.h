// png_deflate16_common.h -- beside png_deflate_common.h, the two steps of a band's workgroup that differ for rows of 16-bit RGB pixels
// (png_deflate16.hip): a segment's raw bytes into LDS from 6-byte pixels, and the run-start scan with the comparison against the byte six
// back.  Everything behind them -- the token rule as symbols, the bit-count scan, the dword-ORing writer, the Adler pair -- is
// png_deflate_common.h's, unchanged: a byte that is not covered starts a run.  (ptl_png_find_runs itself is left as it is, scans included, so
// that png_huffman.hip builds to the same code object; the scans are repeated here.)
#pragma once
#include "png_deflate16_shape.h"
#include "png_deflate_common.h"

// 1. The raw bytes g0 .. g0 + n of the frame's scanlines into raw[0 .. n) (LDS): a lane per pixel = three 16-bit loads of the row and three
// of the row above (rows are only 2-byte aligned when W is odd), subtracted per byte without borrow, stored as six bytes behind the row's
// filter-type byte; the filter-type bytes by a lane per row.  The band ends at row y_end.  No barrier: the caller puts one behind it.
__device__ __forceinline__ void ptl_png16_raw_to_lds(const unsigned short* __restrict__ rows, ptl_u32 w, ptl_u32 y_end, ptl_u32 g0, ptl_u32 n, unsigned char* raw) {
    const ptl_u32 t = threadIdx.x, row_bytes = 6u * w + 1u, g1 = g0 + n;
    const ptl_u32 y0 = g0 / row_bytes, c0 = g0 - y0 * row_bytes;
    const ptl_u32 p_first = y0 * w + (c0 == 0u ? 0u : (c0 - 1u) / 6u);
    for (ptl_u32 k = t; k < ptl_png_segment_bytes / 6u + 2u; k += 256u) {
        const ptl_u32 p = p_first + k, y = p / w;
        const ptl_u32 r = 6u * p + y + 1u;  // the raw offset of the pixel's first byte (at most 2^31)
        if (y >= y_end || r >= g1) break;
        const unsigned short* const cur = rows + 3ull * p;
        const unsigned short* const up = y > 0u ? cur - 3ull * w : cur;  // (row 0 is left as it is)
#pragma unroll
        for (ptl_u32 c = 0u; c < 3u; ++c) {
            const ptl_u32 d = ptl_png16_sub_bytes(cur[c], y > 0u ? up[c] : 0u);  // (a big-endian sample as it lies in memory: its high byte is the load's low byte)
            const ptl_u32 o = r + 2u * c - g0;  // (wraps for the bytes of the first pixel that lie before the segment)
            if (o < n) raw[o] = (unsigned char)d;
            if (o + 1u < n) raw[o + 1u] = (unsigned char)(d >> 8);
        }
    }
    for (ptl_u32 y = y0 + (c0 != 0u) + t; y < y_end && y * row_bytes < g1; y += 256u) raw[y * row_bytes - g0] = y > 0u ? 2u : 0u;
}

// 2. + 3. Byte i is covered -- it starts no run -- when i >= 6 and raw[i] == raw[i - 6]; every other byte starts a run.  Then the scans of
// ptl_png_find_runs: the last start at or before a lane's first byte, the first run end behind its last byte.  raw[-8 .. -1] has to be
// readable (one 8-byte LDS read; the bytes in front of the segment are never compared: i < 6 starts a run).  ONE barrier inside.
__device__ __forceinline__ void ptl_png16_find_runs(const unsigned char* raw, ptl_u32 n, ptl_u32* wave_a, ptl_u32* wave_b, ptl_png_lane_runs& r) {
    const ptl_u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const ptl_u32 i0 = t * ptl_png_lane_bytes;
    const uint4 q = *reinterpret_cast<const uint4*>(raw + i0);
    const ptl_u32 qd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) r.b[j] = (qd[j >> 2] >> (8u * (j & 3u))) & 255u;
    const uint2 f = *reinterpret_cast<const uint2*>(raw + (int)i0 - 8);
    const ptl_u32 front[ptl_png16_distance] = {(f.x >> 16) & 255u, f.x >> 24, f.y & 255u, (f.y >> 8) & 255u, (f.y >> 16) & 255u, f.y >> 24};  // bytes i0 - 6 .. i0 - 1
    ptl_u32 starts = 0u, last_start = 0u, first_bound = n;  // the scans' neutral elements: byte 0 starts a run, the segment's end ends one
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        const ptl_u32 i = i0 + j;
        const ptl_u32 back = j < ptl_png16_distance ? front[j % ptl_png16_distance] : r.b[j < ptl_png16_distance ? 0u : j - ptl_png16_distance];
        if (i < n && (i < ptl_png16_distance || r.b[j] != back)) {
            starts |= 1u << j;
            last_start = i;
            first_bound = min(first_bound, i);
        }
    }
    ptl_u32 a = last_start, z = first_bound;
#pragma unroll
    for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
        const ptl_u32 x = (ptl_u32)__shfl_up((int)a, d), y = (ptl_u32)__shfl_down((int)z, d);
        if (lane >= d) a = max(a, x);
        if (lane + d < 64u) z = min(z, y);
    }
    if (lane == 63u) wave_a[wave] = a;
    if (lane == 0u) wave_b[wave] = z;
    ptl_u32 start_in = (ptl_u32)__shfl_up((int)a, 1), end_in = (ptl_u32)__shfl_down((int)z, 1);
    if (lane == 0u) start_in = 0u;
    if (lane == 63u) end_in = n;
    __syncthreads();
#pragma unroll
    for (ptl_u32 v = 0u; v < 4u; ++v) {
        if (v < wave) start_in = max(start_in, wave_a[v]);
        if (v > wave) end_in = min(end_in, wave_b[v]);
    }
    ptl_u32 next = end_in;
#pragma unroll
    for (int j = (int)ptl_png_lane_bytes - 1; j >= 0; --j) {
        r.run_end[j] = next;
        if (starts & (1u << j)) next = i0 + (ptl_u32)j;
    }
    r.starts = starts;
    r.start_in = start_in;
}
