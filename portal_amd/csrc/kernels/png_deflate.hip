// png_deflate.hip -- an RGBA8 frame in, the deflate stream of its Up-filtered scanlines out: fixed Huffman codes, literals and matches at
// distance 1 (runs) only, so that the host's part of an 8-bit PNG file is a CRC and an fwrite (ptl_png_write_stream).  Two kernels on one
// stream; the contract is the header comment of ptl_png_deflate_rgba8 in include/portal_amd.h (tests/png_deflate_reference.py
// restates it in numpy), the cut into bands and segments and the layout of the result buffer are png_deflate_shape.h's to say.
//
// ptl_png_deflate_bands_kernel: a 256-thread workgroup per band (whole rows; grid-stride over the bands).  Per 4096-byte segment of the band:
//   1. the raw bytes into LDS: a lane per pixel = one dword of the row and one of the row above (consecutive lanes, consecutive dwords),
//      subtracted per byte without borrow, stored as four bytes behind the row's filter-type byte; the filter-type bytes by a lane per row;
//   2. a lane owns 16 raw bytes (one 16-byte LDS read): run starts by comparison with the previous byte;
//   3. the last run start at or before a lane's first byte (max-scan over the lanes below) and the first run end behind its last byte
//      (min-scan over the lanes above): wave shuffles, then the four wave totals through LDS -- position in run and run length per byte;
//   4. token heads and their bits: the literal at position 0, matches of 258 at positions 1 + 258 k, the last match or up to two literals;
//   5. prefix sum of the lanes' bit counts behind the band's running bit offset (the same pass sums the segment's Adler pair);
//   6. each lane shifts its tokens together in a 64-bit register and ORs whole dwords into the LDS bit buffer (ds_or: the first and the
//      last dword of a lane are shared with its neighbours);
//   7. the full dwords go to the band's slot, a dword per lane, the partial dword is carried into the next segment.
// The band ends with end-of-block and an empty stored block (byte alignment); lane 0 stores those last bytes and the band's table entry.
// LDS: 4112 bytes raw + 4624 bytes bits + 80 bytes of wave totals = 8816 bytes.  No scratch, no inline assembly, no atomics on global memory:
// nothing has to be cleared between frames.
//
// ptl_png_deflate_pack_kernel: workgroup c copies the bands of chunk c to their byte offsets in the stream (the sum of the sizes before the
// chunk by a workgroup reduction over the table; byte-granular copies, about 2 MB at 4K); workgroup 0 also combines the bands' Adler pairs
// -- a band's s1 weighs in s2 with the number of raw bytes behind the band, so no prefix is needed -- and writes the 64-byte header.
#include <hip/hip_runtime.h>

#include "png_deflate_shape.h"

typedef unsigned int ptl_u32;
typedef unsigned long long ptl_u64;

constexpr ptl_u32 kSeg = ptl_png_segment_bytes;
constexpr ptl_u32 kLaneBytes = kSeg / 256u;                       // 16
constexpr ptl_u32 kBitDwords = (31u + 9u * kSeg + 31u) / 32u + 3u;  // 1156: the carried partial dword and 9 bits per raw byte
static_assert(kLaneBytes == 16u && kBitDwords == 1156u, "");

// The bits of one token, Huffman codes reversed (they are packed most-significant bit first), count in bits 24 ..
__device__ __forceinline__ ptl_u32 ptl_png_literal(ptl_u32 v) {
    const bool nine = v >= 144u;
    const ptl_u32 code = nine ? v + 256u : v + 0x30u, len = nine ? 9u : 8u;  // 0x190 + (v - 144) = v + 256
    return (__brev(code) >> (32u - len)) | (len << 24);
}
__device__ __forceinline__ ptl_u32 ptl_png_match(ptl_u32 length) {  // 3 .. 258 at distance 1
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
    const bool eight = sym >= 280u;
    const ptl_u32 code = eight ? 0xC0u + (sym - 280u) : sym - 256u, len = eight ? 8u : 7u;
    const ptl_u32 bits = (__brev(code) >> (32u - len)) | (extra << len);  // the distance code 0: five zero bits on top
    return bits | ((len + e + 5u) << 24);
}

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate_bands_kernel(const ptl_u32* __restrict__ frame, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows,
                                                                                ptl_u32 n_bands, uint4* __restrict__ table, unsigned char* __restrict__ slots,
                                                                                ptl_u64 slot_stride) {
    __shared__ __attribute__((aligned(16))) unsigned char raw_store[16u + kSeg];  // raw[-1] is readable (never used: byte 0 starts a run)
    __shared__ ptl_u32 bits[kBitDwords];
    __shared__ ptl_u32 wave_a[4], wave_b[4], wave_c[4], wave_d[4], wave_e[4];
    unsigned char* const raw = raw_store + 16;
    const ptl_u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const ptl_u32 row_bytes = 4u * w + 1u;

    for (ptl_u32 band = blockIdx.x; band < n_bands; band += gridDim.x) {
        const ptl_u32 y_first = band * band_rows, y_end = min(h, y_first + band_rows);
        const ptl_u32 g_begin = y_first * row_bytes, g_end = y_end * row_bytes;  // at most 2^31
        ptl_u32* const slot = reinterpret_cast<ptl_u32*>(slots + (ptl_u64)band * slot_stride);
        ptl_u32 n_bits = 3u, carry = 2u;  // BFINAL = 0, BTYPE = 01: bits 0, 1, 0 in the order they are packed
        ptl_u32 flushed = 0u;             // dwords of the band in its slot
        ptl_u32 band_s1 = 0u, band_s2 = 0u;

        for (ptl_u32 g0 = g_begin; g0 < g_end; g0 += kSeg) {
            const ptl_u32 n = min(kSeg, g_end - g0), g1 = g0 + n;
            // (the barrier that ended the last segment -- or the last band -- lets `bits` and `raw` be written again)
            for (ptl_u32 k = t; k < kBitDwords; k += 256u) bits[k] = k == 0u ? carry : 0u;
            // 1. raw bytes
            const ptl_u32 y0 = g0 / row_bytes, c0 = g0 - y0 * row_bytes;
            const ptl_u32 p_first = y0 * w + (c0 == 0u ? 0u : (c0 - 1u) >> 2);
            for (ptl_u32 k = t; k < kSeg / 4u + 2u; k += 256u) {
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
            __syncthreads();

            // 2. this lane's 16 bytes, run starts
            const ptl_u32 i0 = t * kLaneBytes;
            const uint4 q = *reinterpret_cast<const uint4*>(raw + i0);
            const ptl_u32 qd[4] = {q.x, q.y, q.z, q.w};
            ptl_u32 b[kLaneBytes];
#pragma unroll
            for (ptl_u32 j = 0u; j < kLaneBytes; ++j) b[j] = (qd[j >> 2] >> (8u * (j & 3u))) & 255u;
            ptl_u32 before = raw[(int)i0 - 1];
            ptl_u32 starts = 0u;  // bit j: byte i0 + j is inside the segment and starts a run
            ptl_u32 last_start = 0u, first_bound = n;  // the scans' neutral elements: byte 0 starts a run, the segment's end ends one
#pragma unroll
            for (ptl_u32 j = 0u; j < kLaneBytes; ++j) {
                const ptl_u32 i = i0 + j;
                const bool start = i < n && (i == 0u || b[j] != before);
                before = b[j];
                if (start) {
                    starts |= 1u << j;
                    last_start = i;
                    first_bound = min(first_bound, i);
                }
            }
            // 3. the last start below this lane, the first run end above it
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
            // the end of the run each byte lies in: the next start behind it, or the segment's end
            ptl_u32 run_end[kLaneBytes];
            {
                ptl_u32 next = end_in;
#pragma unroll
                for (int j = (int)kLaneBytes - 1; j >= 0; --j) {
                    run_end[j] = next;
                    if (starts & (1u << j)) next = i0 + (ptl_u32)j;
                }
            }
            // 4. tokens: bits | count << 24, 0 where the byte is covered by a match that started before it
            ptl_u32 token[kLaneBytes];
            ptl_u32 lane_bits = 0u, s1 = 0u, s2 = 0u;
            {
                ptl_u32 run_start = start_in;
#pragma unroll
                for (ptl_u32 j = 0u; j < kLaneBytes; ++j) {
                    const ptl_u32 i = i0 + j;
                    if (starts & (1u << j)) run_start = i;
                    const ptl_u32 pos = i - run_start;
                    ptl_u32 tok = 0u;
                    if (i < n) {
                        if (pos == 0u) {
                            tok = ptl_png_literal(b[j]);
                        } else {
                            const ptl_u32 m = run_end[j] - run_start - 1u;  // what follows the run's first literal
                            const ptl_u32 whole = m / 258u, rest = m - whole * 258u;
                            const ptl_u32 at = (pos - 1u) / 258u, off = (pos - 1u) - at * 258u;
                            const bool match = at < whole || rest >= 3u;  // else: one of the run's last one or two literals
                            tok = !match ? ptl_png_literal(b[j]) : off == 0u ? ptl_png_match(at < whole ? 258u : rest) : 0u;
                        }
                        s1 += b[j];
                        s2 += (n - i) * b[j];
                    }
                    token[j] = tok;
                    lane_bits += tok >> 24;
                }
            }
            // 5. where this lane's bits start; the segment's bit count and Adler pair
            ptl_u32 inc = lane_bits;
#pragma unroll
            for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
                const ptl_u32 x = (ptl_u32)__shfl_up((int)inc, d);
                if (lane >= d) inc += x;
                s1 += (ptl_u32)__shfl_xor((int)s1, d);
                s2 += (ptl_u32)__shfl_xor((int)s2, d);
            }
            if (lane == 63u) {
                wave_c[wave] = inc;
                wave_d[wave] = s1;
                wave_e[wave] = s2;
            }
            __syncthreads();
            ptl_u32 at_bit = (n_bits & 31u) + inc - lane_bits, seg_bits = 0u, seg_s1 = 0u, seg_s2 = 0u;
#pragma unroll
            for (ptl_u32 v = 0u; v < 4u; ++v) {
                if (v < wave) at_bit += wave_c[v];
                seg_bits += wave_c[v];
                seg_s1 += wave_d[v];
                seg_s2 += wave_e[v];
            }
            // 6. the lane's bits
            {
                ptl_u32 dw = at_bit >> 5, have = at_bit & 31u;
                ptl_u64 acc = 0ull;
#pragma unroll
                for (ptl_u32 j = 0u; j < kLaneBytes; ++j) {
                    const ptl_u32 count = token[j] >> 24;
                    acc |= (ptl_u64)(token[j] & 0xffffffu) << have;
                    have += count;
                    if (have >= 32u) {
                        atomicOr(&bits[dw], (ptl_u32)acc);
                        acc >>= 32;
                        have -= 32u;
                        ++dw;
                    }
                }
                if (acc != 0ull) atomicOr(&bits[dw], (ptl_u32)acc);
            }
            __syncthreads();
            // 7. full dwords to the slot, the partial one into the next segment
            const ptl_u32 in_buffer = (n_bits & 31u) + seg_bits, full = in_buffer >> 5;
            for (ptl_u32 k = t; k < full; k += 256u) slot[flushed + k] = bits[k];
            carry = bits[full];
            flushed += full;
            n_bits += seg_bits;
            band_s2 = (ptl_u32)(((ptl_u64)band_s2 + (ptl_u64)n * band_s1 + seg_s2) % ptl_png_adler_mod);
            band_s1 = (band_s1 + seg_s1) % ptl_png_adler_mod;
            __syncthreads();
        }
        if (t == 0u) {
            // end-of-block (7 zero bits), the empty stored block: 3 zero bits, padding to the byte, LEN = 0, NLEN = 0xffff
            const ptl_u32 tail = ((n_bits & 31u) + 10u + 7u) >> 3;  // 2 .. 6 bytes, the carried bits in the first of them
            unsigned char* const p = reinterpret_cast<unsigned char*>(slot + flushed);
            for (ptl_u32 k = 0u; k < tail; ++k) p[k] = k < 4u ? (unsigned char)(carry >> (8u * k)) : 0u;
            p[tail] = 0u;
            p[tail + 1u] = 0u;
            p[tail + 2u] = 255u;
            p[tail + 3u] = 255u;
            table[band] = make_uint4(4u * flushed + tail + 4u, band_s1, band_s2, g_end - g_begin);
        }
    }
}

// The sum of a 64-bit value over the workgroup, in every lane.  `store`: eight dwords of LDS; barriers inside.
__device__ __forceinline__ ptl_u64 ptl_png_workgroup_sum(ptl_u64 v, ptl_u32* store) {
    const ptl_u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
        const ptl_u32 lo = (ptl_u32)__shfl_xor((int)(ptl_u32)v, d), hi = (ptl_u32)__shfl_xor((int)(ptl_u32)(v >> 32), d);
        v += ((ptl_u64)hi << 32) | lo;
    }
    __syncthreads();  // (the store may still be read from the call before)
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

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate_pack_kernel(unsigned char* __restrict__ out, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows, ptl_u32 n_bands,
                                                                               ptl_u64 table_offset, ptl_u64 slots_offset, ptl_u64 slot_stride) {
    __shared__ ptl_u32 store[8];
    const uint4* const table = reinterpret_cast<const uint4*>(out + table_offset);
    const unsigned char* const slots = out + slots_offset;
    const ptl_u32 t = threadIdx.x;
    const ptl_u32 per = (n_bands + gridDim.x - 1u) / gridDim.x;  // bands per workgroup, a contiguous chunk each
    const ptl_u64 first64 = (ptl_u64)blockIdx.x * per;
    const ptl_u32 first = (ptl_u32)min(first64, (ptl_u64)n_bands), last = (ptl_u32)min(first64 + per, (ptl_u64)n_bands);
    ptl_u64 before = 0ull;
    for (ptl_u32 b = t; b < first; b += 256u) before += table[b].x;
    ptl_u64 at = ptl_png_workgroup_sum(before, store);
    unsigned char* const stream = out + ptl_png_header_bytes;
    for (ptl_u32 b = first; b < last; ++b) {
        const ptl_u32 used = table[b].x;
        const unsigned char* const src = slots + (ptl_u64)b * slot_stride;
        for (ptl_u32 i = t; i < used; i += 256u) stream[at + i] = src[i];
        at += used;
    }
    if (blockIdx.x != 0u) return;
    // the whole stream's size and Adler-32: A = 1 + sum s1, B = N + sum (s2 + s1 * raw bytes behind the band), mod 65521
    const ptl_u64 row_bytes = 4ull * w + 1ull, n_raw = row_bytes * h;
    ptl_u64 bytes = 0ull, sum1 = 0ull, sum2 = 0ull;
    for (ptl_u32 b = t; b < n_bands; b += 256u) {
        const uint4 e = table[b];
        const ptl_u64 end_row = min((ptl_u64)h, ((ptl_u64)b + 1ull) * band_rows);
        const ptl_u64 behind = (n_raw - end_row * row_bytes) % ptl_png_adler_mod;
        bytes += e.x;
        sum1 += e.y;
        sum2 += (e.z + (ptl_u64)e.y * behind) % ptl_png_adler_mod;
    }
    bytes = ptl_png_workgroup_sum(bytes, store);
    sum1 = ptl_png_workgroup_sum(sum1, store);
    sum2 = ptl_png_workgroup_sum(sum2, store);
    if (t == 0u) {
        const ptl_u32 a = (ptl_u32)((1ull + sum1) % ptl_png_adler_mod), b = (ptl_u32)((n_raw + sum2) % ptl_png_adler_mod);
        ptl_u32* const header = reinterpret_cast<ptl_u32*>(out);
        const ptl_u32 words[16] = {ptl_png_magic, w, h, (ptl_u32)bytes, (b << 16) | a, band_rows, n_bands, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (ptl_u32 k = 0u; k < 16u; ++k) header[k] = words[k];
    }
}
