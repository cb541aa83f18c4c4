// png_deflate_common.h -- the steps of a band's workgroup that do not depend on the Huffman code, for the kernels that deflate the Up-filtered
// scanlines of a frame with matches at one distance only (png_deflate.hip, png_huffman.hip; the steps are those png_deflate.hip numbers 1 .. 7
// in its header comment): a segment's raw bytes into LDS from 8-bit and from 16-bit pixels, the run-start scan at a distance, the token rule,
// the prefix sum of the lanes' bit counts, the dword-ORing bit writer, the Adler pair, the flush to the band's slot and the band's last bytes;
// the fixed code and the code-length code of RFC 1951.  256 threads, a lane owns 16 raw bytes of the 4096-byte segment.  Barriers are named
// where a function has one.
#pragma once
#include <hip/hip_runtime.h>

#include "png_deflate_shape.h"

typedef unsigned int ptl_u32;
typedef unsigned long long ptl_u64;

constexpr ptl_u32 ptl_png_lane_bytes = ptl_png_segment_bytes / 256u;
static_assert(ptl_png_lane_bytes == 16u, "a lane reads its bytes as one uint4");

// What a segment needs in LDS: the raw bytes with 16 readable bytes in front of them, the bit buffer (the carried partial dword and `BitsPerByte`
// bits per raw byte) and five times four wave totals.  It is the first member of a 16-byte aligned __shared__ variable: raw() is 16-byte aligned.
template <ptl_u32 BitsPerByte>
struct ptl_png_segment_lds {
    static constexpr ptl_u32 bit_dwords = (31u + BitsPerByte * ptl_png_segment_bytes + 31u) / 32u + 3u;
    unsigned char raw_store[16u + ptl_png_segment_bytes];
    ptl_u32 bits[bit_dwords];
    ptl_u32 wave_a[4], wave_b[4], wave_c[4], wave_d[4], wave_e[4];
    __device__ __forceinline__ unsigned char* raw() { return raw_store + 16; }
};

// The filter-type bytes of the rows that begin inside raw bytes g0 .. g1, by a lane per row: 0 (None) for row 0, 2 (Up) below it.
__device__ __forceinline__ void ptl_png_filter_bytes_to_lds(ptl_u32 row_bytes, ptl_u32 y_end, ptl_u32 g0, ptl_u32 g1, unsigned char* raw) {
    const ptl_u32 y0 = g0 / row_bytes;
    for (ptl_u32 y = y0 + (g0 != y0 * row_bytes) + threadIdx.x; y < y_end && y * row_bytes < g1; y += 256u) raw[y * row_bytes - g0] = y > 0u ? 2u : 0u;
}

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
    ptl_png_filter_bytes_to_lds(row_bytes, y_end, g0, g1, raw);
}

// 1. for rows of 16-bit RGB pixels: a lane per pixel = three 16-bit loads of the row and three of the row above (rows are only 2-byte aligned
// when W is odd), subtracted per byte without borrow, stored as six bytes behind the row's filter-type byte.  No barrier either.
__device__ __forceinline__ void ptl_png_raw_to_lds(const unsigned short* __restrict__ rows, ptl_u32 w, ptl_u32 y_end, ptl_u32 g0, ptl_u32 n, unsigned char* raw) {
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
            const ptl_u32 d = ptl_png_sub_bytes16(cur[c], y > 0u ? up[c] : 0u);  // (a big-endian sample as it lies in memory: its high byte is the load's low byte)
            const ptl_u32 o = r + 2u * c - g0;  // (wraps for the bytes of the first pixel that lie before the segment)
            if (o < n) raw[o] = (unsigned char)d;
            if (o + 1u < n) raw[o + 1u] = (unsigned char)(d >> 8);
        }
    }
    ptl_png_filter_bytes_to_lds(row_bytes, y_end, g0, g1, raw);
}

// What a lane knows about its 16 bytes after the scan.
struct ptl_png_lane_runs {
    ptl_u32 b[ptl_png_lane_bytes];        // the bytes
    ptl_u32 run_end[ptl_png_lane_bytes];  // the end of the run each byte lies in: the next start behind it, or the segment's end
    ptl_u32 starts;                       // bit j: byte j is inside the segment and starts a run
    ptl_u32 start_in;                     // the last run start below the lane's first byte
};

// 2. + 3. Byte i is covered -- it starts no run -- when i >= D and raw[i] == raw[i - D]; every other byte starts a run (D = 1: the runs of
// equal bytes).  Then the last start at or before a lane's first byte (max-scan over the lanes below) and the first run end behind its last
// byte (min-scan over the lanes above): wave shuffles, then the four wave totals through wave_a / wave_b (four dwords of LDS each).
// raw[-8 .. -1] has to be readable: the D bytes in front of the lane's 16 come from one 8-byte LDS read.  In front of the segment -- lane 0 --
// that read touches LDS nobody wrote, and the value is never compared: i < D starts a run.  ONE barrier inside, between the writes and the
// reads of the wave totals.
template <ptl_u32 D>
__device__ __forceinline__ void ptl_png_find_runs(const unsigned char* raw, ptl_u32 n, ptl_u32* wave_a, ptl_u32* wave_b, ptl_png_lane_runs& r) {
    static_assert(D >= 1u && D <= 8u, "the bytes in front of a lane come from one 8-byte read");
    const ptl_u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const ptl_u32 i0 = t * ptl_png_lane_bytes;
    const uint4 q = *reinterpret_cast<const uint4*>(raw + i0);
    const ptl_u32 qd[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) r.b[j] = (qd[j >> 2] >> (8u * (j & 3u))) & 255u;
    const uint2 f = *reinterpret_cast<const uint2*>(raw + (int)i0 - 8);
    const ptl_u64 front = (((ptl_u64)f.y << 32) | f.x) >> (8u * (8u - D));  // bytes i0 - D .. i0 - 1
    ptl_u32 starts = 0u, last_start = 0u, first_bound = n;  // the scans' neutral elements: byte 0 starts a run, the segment's end ends one
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        const ptl_u32 i = i0 + j;
        const ptl_u32 back = j < D ? (ptl_u32)(front >> (8u * (j % D))) & 255u : r.b[j < D ? 0u : j - D];
        if (i < n && (i < D || r.b[j] != back)) {
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

struct ptl_png_symbol_tokens {
    static __device__ __forceinline__ ptl_u32 literal(ptl_u32 v) { return ptl_png_token_flag | v; }
    static __device__ __forceinline__ ptl_u32 match(ptl_u32 length) {  // 3 .. 258 (RFC 1951 3.2.5)
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
};

// The token rule for the lane's bytes: in a run of m + 1 bytes the literal at position 0, matches of 258 at positions 1 + 258 k, the last
// match or up to two literals.  `Tokens` says what a literal and a match of a length are: symbols (above), or their bits at once
// (png_deflate.hip).
template <class Tokens>
__device__ __forceinline__ void ptl_png_lane_tokens(const ptl_png_lane_runs& r, ptl_u32 n, ptl_u32 (&token)[ptl_png_lane_bytes]) {
    const ptl_u32 i0 = threadIdx.x * ptl_png_lane_bytes;
    ptl_u32 run_start = r.start_in;
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        const ptl_u32 i = i0 + j;
        if (r.starts & (1u << j)) run_start = i;
        const ptl_u32 pos = i - run_start;
        ptl_u32 tok = 0u;
        if (i < n) {
            if (pos == 0u) {
                tok = Tokens::literal(r.b[j]);
            } else {
                const ptl_u32 m = r.run_end[j] - run_start - 1u;  // what follows the run's first literal
                const ptl_u32 whole = m / 258u, rest = m - whole * 258u;
                const ptl_u32 at = (pos - 1u) / 258u, off = (pos - 1u) - at * 258u;
                const bool match = at < whole || rest >= 3u;  // else: one of the run's last one or two literals
                tok = !match ? Tokens::literal(r.b[j]) : off == 0u ? Tokens::match(at < whole ? 258u : rest) : 0u;
            }
        }
        token[j] = tok;
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

// A 64-bit value summed over the workgroup, in every lane.  `store`: eight dwords of LDS; a barrier before the store is written (it may still
// be read from the call before) and one behind.
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

// A band on its way into its slot: the bits so far, the partial dword that is carried into the next segment's bit buffer, the whole dwords
// already in the slot, and the Adler pair of the raw bytes so far.
struct ptl_png_band_state {
    ptl_u32 n_bits, carry, flushed, s1, s2;
};

// Before a segment's first barrier: the bit buffer cleared but for the carried dword.
template <class Lds>
__device__ __forceinline__ void ptl_png_clear_bits(Lds& lds, const ptl_png_band_state& band) {
    for (ptl_u32 k = threadIdx.x; k < Lds::bit_dwords; k += 256u) lds.bits[k] = k == 0u ? band.carry : 0u;
}

// 5. - 7. for a segment of n bytes whose tokens are bits (the value in the low 24 bits of token[j], their number above): where each lane's
// bits start, by the prefix sum of the bit counts, and in the same pass the segment's Adler sums s1 = sum b, s2 = sum (n - i) b; the bits
// ORed into the bit buffer; the full dwords to the band's slot, a dword per lane and never beyond the slot, the partial dword carried.
// THREE barriers inside: ptl_png_scan's (also behind wave_d and wave_e), one between the ORs and the reads of the bit buffer, and one at the
// end, which lets the raw bytes, the bit buffer and the wave totals be written again.
template <class Lds>
__device__ __forceinline__ void ptl_png_emit_segment(Lds& lds, const ptl_png_lane_runs& runs, ptl_u32 n, const ptl_u32 (&token)[ptl_png_lane_bytes], ptl_u32* slot,
                                                     ptl_u32 slot_dwords, ptl_png_band_state& band) {
    const ptl_u32 t = threadIdx.x, i0 = t * ptl_png_lane_bytes;
    ptl_u32 lane_bits = 0u, s1 = 0u, s2 = 0u;
#pragma unroll
    for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
        if (i0 + j < n) {
            s1 += runs.b[j];
            s2 += (n - (i0 + j)) * runs.b[j];
        }
        lane_bits += token[j] >> 24;
    }
#pragma unroll
    for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
        s1 += (ptl_u32)__shfl_xor((int)s1, d);
        s2 += (ptl_u32)__shfl_xor((int)s2, d);
    }
    if ((t & 63u) == 63u) {
        lds.wave_d[t >> 6] = s1;
        lds.wave_e[t >> 6] = s2;
    }
    ptl_u32 below, seg_bits;
    ptl_png_scan(lane_bits, lds.wave_c, below, seg_bits);
    const ptl_u32 seg_s1 = lds.wave_d[0] + lds.wave_d[1] + lds.wave_d[2] + lds.wave_d[3], seg_s2 = lds.wave_e[0] + lds.wave_e[1] + lds.wave_e[2] + lds.wave_e[3];
    const ptl_u32 at_bit = (band.n_bits & 31u) + below;
    if (at_bit + lane_bits <= 32u * (Lds::bit_dwords - 2u)) ptl_png_or_bits(lds.bits, at_bit, token);  // (always: the buffer holds the dearest segment)
    __syncthreads();
    const ptl_u32 in_buffer = (band.n_bits & 31u) + seg_bits, full = min(in_buffer >> 5, Lds::bit_dwords - 1u);
    for (ptl_u32 k = t; k < full; k += 256u)
        if (band.flushed + k < slot_dwords) slot[band.flushed + k] = lds.bits[k];
    band.carry = lds.bits[full];
    band.flushed += full;
    band.n_bits += seg_bits;
    band.s2 = (ptl_u32)(((ptl_u64)band.s2 + (ptl_u64)n * band.s1 + seg_s2) % ptl_png_adler_mod);  // the pair with the segment appended
    band.s1 = (band.s1 + seg_s1) % ptl_png_adler_mod;
    __syncthreads();
}

// The band's last bytes and its table entry, by ONE lane: end-of-block (`end`: its code, the length in bits 24 ..), the empty stored block
// -- 3 zero bits, padding to the byte, LEN = 0, NLEN = 0xffff -- behind the carried bits, never beyond the slot.
__device__ __forceinline__ void ptl_png_end_band(const ptl_png_band_state& band, ptl_u32 end, ptl_u32* slot, ptl_u64 slot_stride, uint4* entry, ptl_u32 raw_bytes) {
    const ptl_u64 last = (ptl_u64)band.carry | ((ptl_u64)(end & 0xffffffu) << (band.n_bits & 31u));
    const ptl_u32 tail = ((band.n_bits & 31u) + (end >> 24) + 3u + 7u) >> 3;  // 1 .. 7 bytes, the carried bits in the first of them
    if ((ptl_u64)4u * band.flushed + tail + 4u <= slot_stride) {
        unsigned char* const p = reinterpret_cast<unsigned char*>(slot + band.flushed);
        for (ptl_u32 k = 0u; k < tail; ++k) p[k] = (unsigned char)(last >> (8u * k));
        p[tail] = 0u;
        p[tail + 1u] = 0u;
        p[tail + 2u] = 255u;
        p[tail + 3u] = 255u;
    }
    *entry = make_uint4(4u * band.flushed + tail + 4u, band.s1, band.s2, raw_bytes);
}

// The fixed code (RFC 1951 3.2.6): a literal/length symbol's length, and its entry -- the code bit-reversed (codes are packed most-significant
// bit first), the length in bits 24 ..
__device__ __forceinline__ ptl_u32 ptl_png_fixed_length(ptl_u32 s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
__device__ __forceinline__ ptl_u32 ptl_png_fixed_entry(ptl_u32 s) {
    const ptl_u32 len = ptl_png_fixed_length(s);
    const ptl_u32 code = s < 144u ? 0x30u + s : s < 256u ? 0x190u + (s - 144u) : s < 280u ? s - 256u : 0xC0u + (s - 280u);
    return (__brev(code) >> (32u - len)) | (len << 24);
}

// The contract's code-length code, symbol 0 .. 18: the canonical code of the lengths 3 7 4 4 4 4 4 4 4 4 5 5 6 6 6 7 4 4 3, bit-reversed,
// its length in bits 24 ..; and the 19 lengths, three bits each, in the order RFC 1951 3.2.7 stores them.
__device__ const ptl_u32 ptl_png_code_length_code[19] = {0x3000000u, 0x700003fu, 0x4000002u, 0x400000au, 0x4000006u, 0x400000eu, 0x4000001u, 0x4000009u, 0x4000005u, 0x400000du,
                                                         0x5000007u, 0x5000017u, 0x600000fu, 0x600002fu, 0x600001fu, 0x700007fu, 0x4000003u, 0x400000bu, 0x3000004u};
constexpr ptl_u64 ptl_png_code_length_lengths = 0x1fe9a69659246e4ull;  // 57 bits
