// png_deflate_common.h -- the steps of a band's workgroup that do not depend on the Huffman code, for the kernels that deflate the Up-filtered
// scanlines of an RGBA8 frame with runs only (png_huffman.hip; the steps are those png_deflate.hip numbers 1 .. 7 in its header comment): a
// segment's raw bytes into LDS, the run-start scan, the token rule as symbols, the prefix sum of the lanes' bit counts, the dword-ORing bit
// writer and the Adler pair.  256 threads, a lane owns 16 raw bytes of the 4096-byte segment.  Barriers are named where a function has one.
#pragma once
#include <hip/hip_runtime.h>

#include "png_deflate_shape.h"

typedef unsigned int ptl_u32;
typedef unsigned long long ptl_u64;

constexpr ptl_u32 ptl_png_lane_bytes = ptl_png_segment_bytes / 256u;
static_assert(ptl_png_lane_bytes == 16u, "a lane reads its bytes as one uint4");

// 1. The raw bytes g0 .. g0 + n of the frame's scanlines into raw[0 .. n) (LDS): a lane per pixel = one dword of the row and one of the row
// above, subtracted per byte without borrow, stored as four bytes behind the row's filter-type byte; the filter-type bytes by a lane per row.
// The band ends at row y_end.  No barrier: the caller puts one behind it.
__device__ __forceinline__ void ptl_png_raw_to_lds(const ptl_u32* __restrict__ frame, ptl_u32 w, ptl_u32 y_end, ptl_u32 g0, ptl_u32 n, unsigned char* raw) {
    const ptl_u32 t = threadIdx.x, row_bytes = 4u * w + 1u, g1 = g0 + n;
    const ptl_u32 y0 = g0 / row_bytes, c0 = g0 - y0 * row_bytes;
    const ptl_u32 p_first = y0 * w + (c0 == 0u ? 0u : (c0 - 1u) >> 2);
    for (ptl_u32 k = t; k < ptl_png_segment_bytes / 4u + 2u; k += 256u) {
        const ptl_u32 p = p_first + k, y = p / w;
        const ptl_u32 r = 4u * p + y + 1u;  // the raw offset of the pixel's first byte
        if (y >= y_end || r >= g1) break;
        const ptl_u32 cur = frame[p], up = y > 0u ? frame[p - w] : 0u;
        const ptl_u32 d = ptl_png_sub_bytes(cur, up);
#pragma unroll
        for (ptl_u32 j = 0u; j < 4u; ++j) {
            const ptl_u32 o = r + j - g0;  // (wraps for the bytes of the first pixel that lie before the segment)
            if (o < n) raw[o] = (unsigned char)(d >> (8u * j));
        }
    }
    for (ptl_u32 y = y0 + (c0 != 0u) + t; y < y_end && y * row_bytes < g1; y += 256u) raw[y * row_bytes - g0] = y > 0u ? 2u : 0u;
}

// What a lane knows about its 16 bytes after the scan.
struct ptl_png_lane_runs {
    ptl_u32 b[ptl_png_lane_bytes];        // the bytes
    ptl_u32 run_end[ptl_png_lane_bytes];  // the end of the run each byte lies in: the next start behind it, or the segment's end
    ptl_u32 starts;                       // bit j: byte j is inside the segment and starts a run
    ptl_u32 start_in;                     // the last run start below the lane's first byte
};

// 2. + 3. Run starts by comparison with the previous byte; the last start at or before a lane's first byte (max-scan over the lanes below) and
// the first run end behind its last byte (min-scan over the lanes above): wave shuffles, then the four wave totals through wave_a / wave_b
// (four dwords of LDS each).  raw[-1] has to be readable.  ONE barrier inside, between the writes and the reads of the wave totals.
__device__ __forceinline__ void ptl_png_find_runs(const unsigned char* raw, ptl_u32 n, ptl_u32* wave_a, ptl_u32* wave_b, ptl_png_lane_runs& r) {
    const ptl_u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const ptl_u32 i0 = t * ptl_png_lane_bytes;
    const uint4 q = *reinterpret_cast<const uint4*>(raw + i0);
    const ptl_u32 qd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) r.b[j] = (qd[j >> 2] >> (8u * (j & 3u))) & 255u;
    ptl_u32 before = raw[(int)i0 - 1];
    ptl_u32 starts = 0u, last_start = 0u, first_bound = n;  // the scans' neutral elements: byte 0 starts a run, the segment's end ends one
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        const ptl_u32 i = i0 + j;
        const bool start = i < n && (i == 0u || r.b[j] != before);
        before = r.b[j];
        if (start) {
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

// 4. Tokens as symbols: bit 31 set, the literal/length symbol in bits 0 .. 8, the value of a match's extra bits in bits 9 .. 13, their number in
// bits 14 .. 16.  0: the byte is covered by a match that started before it.
constexpr ptl_u32 ptl_png_token_flag = 1u << 31;
__device__ __forceinline__ ptl_u32 ptl_png_token_symbol(ptl_u32 token) { return token & 511u; }
__device__ __forceinline__ ptl_u32 ptl_png_token_extra(ptl_u32 token) { return (token >> 9) & 31u; }
__device__ __forceinline__ ptl_u32 ptl_png_token_extra_bits(ptl_u32 token) { return (token >> 14) & 7u; }

__device__ __forceinline__ ptl_u32 ptl_png_match_token(ptl_u32 length) {  // 3 .. 258 (RFC 1951 3.2.5)
    const ptl_u32 l = length - 3u;
    ptl_u32 sym, extra = 0u, e = 0u;
    if (length == 258u) {
        sym = 285u;
    } else if (l < 8u) {
        sym = 257u + l;
    } else {
        e = 29u - (ptl_u32)__clz((int)l);  // floor(log2 l) - 2: 1 .. 5 extra bits
        sym = 261u + 4u * e + ((l >> e) & 3u);
        extra = l & ((1u << e) - 1u);
    }
    return ptl_png_token_flag | sym | (extra << 9) | (e << 14);
}

// The token rule for the byte `pos` bytes into a run of m + 1 bytes v: the literal at position 0, matches of 258 at positions 1 + 258 k, the
// last match or up to two literals.
__device__ __forceinline__ ptl_u32 ptl_png_token_at(ptl_u32 pos, ptl_u32 m, ptl_u32 v) {
    if (pos == 0u) return ptl_png_token_flag | v;
    const ptl_u32 whole = m / 258u, rest = m - whole * 258u;
    const ptl_u32 at = (pos - 1u) / 258u, off = (pos - 1u) - at * 258u;
    const bool match = at < whole || rest >= 3u;  // else: one of the run's last one or two literals
    return !match ? (ptl_png_token_flag | v) : off == 0u ? ptl_png_match_token(at < whole ? 258u : rest) : 0u;
}

__device__ __forceinline__ void ptl_png_lane_tokens(const ptl_png_lane_runs& r, ptl_u32 n, ptl_u32 (&token)[ptl_png_lane_bytes]) {
    const ptl_u32 i0 = threadIdx.x * ptl_png_lane_bytes;
    ptl_u32 run_start = r.start_in;
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        const ptl_u32 i = i0 + j;
        if (r.starts & (1u << j)) run_start = i;
        token[j] = i < n ? ptl_png_token_at(i - run_start, r.run_end[j] - run_start - 1u, r.b[j]) : 0u;
    }
}

// 5. A lane's 32-bit value summed over the lanes below it and over the workgroup.  `store`: four dwords of LDS.  ONE barrier inside; the
// caller has one between two uses of the same store.
__device__ __forceinline__ void ptl_png_scan(ptl_u32 mine, ptl_u32* store, ptl_u32& below, ptl_u32& total) {
    const ptl_u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    ptl_u32 inc = mine;
#pragma unroll
    for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
        const ptl_u32 x = (ptl_u32)__shfl_up((int)inc, d);
        if (lane >= d) inc += x;
    }
    if (lane == 63u) store[wave] = inc;
    __syncthreads();
    below = inc - mine;
    total = 0u;
#pragma unroll
    for (ptl_u32 v = 0u; v < 4u; ++v) {
        if (v < wave) below += store[v];
        total += store[v];
    }
}

// A 64-bit value summed over the workgroup, in every lane.  `store`: eight dwords of LDS; a barrier before the store is written and one behind.
__device__ __forceinline__ ptl_u64 ptl_png_sum64(ptl_u64 v, ptl_u32* store) {
    const ptl_u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
        const ptl_u32 lo = (ptl_u32)__shfl_xor((int)(ptl_u32)v, d), hi = (ptl_u32)__shfl_xor((int)(ptl_u32)(v >> 32), d);
        v += ((ptl_u64)hi << 32) | lo;
    }
    __syncthreads();
    if (lane == 0u) {
        store[2u * wave] = (ptl_u32)v;
        store[2u * wave + 1u] = (ptl_u32)(v >> 32);
    }
    __syncthreads();
    ptl_u64 sum = 0ull;
#pragma unroll
    for (ptl_u32 k = 0u; k < 4u; ++k) sum += ((ptl_u64)store[2u * k + 1u] << 32) | store[2u * k];
    return sum;
}

// 6. The lane's tokens -- the bits in the low 24 bits of token[j], their number (at most 24, 0 for none) above them -- shifted together in a
// 64-bit register from bit `at_bit` of the LDS bit buffer on and ORed in as whole dwords (ds_or: the first and the last dword of a lane are
// shared with its neighbours).
__device__ __forceinline__ void ptl_png_or_bits(ptl_u32* bits, ptl_u32 at_bit, const ptl_u32 (&token)[ptl_png_lane_bytes]) {
    ptl_u32 dw = at_bit >> 5, have = at_bit & 31u;
    ptl_u64 acc = 0ull;
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        acc |= (ptl_u64)(token[j] & 0xffffffu) << have;
        have += token[j] >> 24;
        if (have >= 32u) {
            atomicOr(&bits[dw], (ptl_u32)acc);
            acc >>= 32;
            have -= 32u;
            ++dw;
        }
    }
    if (acc != 0ull) atomicOr(&bits[dw], (ptl_u32)acc);
}

// The Adler pair of a band with a segment of n bytes appended, whose own sums are seg_s1 = sum b and seg_s2 = sum (n - i) b.
__device__ __forceinline__ void ptl_png_adler_append(ptl_u32& band_s1, ptl_u32& band_s2, ptl_u32 n, ptl_u32 seg_s1, ptl_u32 seg_s2) {
    band_s2 = (ptl_u32)(((ptl_u64)band_s2 + (ptl_u64)n * band_s1 + seg_s2) % ptl_png_adler_mod);
    band_s1 = (band_s1 + seg_s1) % ptl_png_adler_mod;
}
