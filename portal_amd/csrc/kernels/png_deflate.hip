// png_deflate.hip -- an RGBA8 frame in, the deflate stream of its Up-filtered scanlines out: fixed Huffman codes, literals and matches at
// distance 1 (runs) only, so that the host's part of an 8-bit PNG file is a CRC and an fwrite (ptl_png_write_stream); and the pack kernel of
// every GPU deflate path.  Two kernels on one stream; the contract is the header comment of ptl_png_deflate_rgba8 in include/portal_amd.h
// (tests/png_deflate_reference.py restates it in numpy), the cut into bands and segments and the layout of the result
// buffer are png_deflate_shape.h's to say, the steps are png_deflate_common.h's.
//
// ptl_png_deflate_bands_kernel: a 256-thread workgroup per band (whole rows; grid-stride over the bands), ONE pass.  Per 4096-byte segment
// of the band:
//   1. the raw bytes into LDS: a lane per pixel = one dword of the row and one of the row above (consecutive lanes, consecutive dwords),
//      subtracted per byte without borrow, stored as four bytes behind the row's filter-type byte; the filter-type bytes by a lane per row;
//   2. a lane owns 16 raw bytes (one 16-byte LDS read): run starts by comparison with the previous byte;
//   3. the last run start at or before a lane's first byte (max-scan over the lanes below) and the first run end behind its last byte
//      (min-scan over the lanes above): wave shuffles, then the four wave totals through LDS -- position in run and run length per byte;
//   4. token heads and their bits: the literal at position 0, matches of 258 at positions 1 + 258 k, the last match or up to two literals.
//      The rule is the common header's; the bits of a token come straight from ptl_png_fixed_tokens below, with no code table
//      and no second pass -- that is what this kernel is for;
//   5. prefix sum of the lanes' bit counts behind the band's running bit offset (the same pass sums the segment's Adler pair);
//   6. each lane shifts its tokens together in a 64-bit register and ORs whole dwords into the LDS bit buffer (ds_or: the first and the
//      last dword of a lane are shared with its neighbours);
//   7. the full dwords go to the band's slot, a dword per lane, the partial dword is carried into the next segment.
// The band ends with end-of-block and an empty stored block (byte alignment); lane 0 stores those last bytes and the band's table entry.
// Stores to the slot are guarded by its size, so a band can never write outside its slot.
// LDS: 4112 bytes raw + 4624 bytes bits + 80 bytes of wave totals = 8816 bytes.  No scratch, no inline assembly, no atomics on global memory:
// nothing has to be cleared between frames.
//
// ptl_png_deflate_pack_kernel: for the bands of this file's kernel and of png_huffman.hip's two, of pixels of `pixel` bytes.  Workgroup c
// copies the bands of chunk c to their byte offsets in the stream (the sum of the sizes before the chunk by a workgroup reduction over the
// table; byte-granular copies, about 2 MB at 4K, never beyond the room for the stream); workgroup 0 also combines the bands' Adler pairs
// -- a band's s1 weighs in s2 with the number of raw bytes behind the band, rows of pixel W + 1 bytes, so no prefix is needed -- and writes
// the 64-byte header with the magic word it is given.
#include <hip/hip_runtime.h>

#include "png_deflate_common.h"

typedef ptl_png_segment_lds<9u> ptl_png_fixed_lds;  // a fixed-code token never costs more than 9 bits per raw byte
static_assert(ptl_png_fixed_lds::bit_dwords == 1156u && sizeof(ptl_png_fixed_lds) == 8816u, "");

// The bits of one token, Huffman codes reversed (they are packed most-significant bit first), count in bits 24 ..
struct ptl_png_fixed_tokens {
    static __device__ __forceinline__ ptl_u32 literal(ptl_u32 v) {
        const bool nine = v >= 144u;
        const ptl_u32 code = nine ? v + 256u : v + 0x30u, len = nine ? 9u : 8u;  // 0x190 + (v - 144) = v + 256
        return (__brev(code) >> (32u - len)) | (len << 24);
    }
    static __device__ __forceinline__ ptl_u32 match(ptl_u32 length) {  // 3 .. 258 at distance 1
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
};

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate_bands_kernel(const ptl_u32* __restrict__ frame, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows,
                                                                                ptl_u32 n_bands, uint4* __restrict__ table, unsigned char* __restrict__ slots,
                                                                                ptl_u64 slot_stride) {
    __shared__ __attribute__((aligned(16))) ptl_png_fixed_lds lds;
    unsigned char* const raw = lds.raw();
    const ptl_u32 row_bytes = 4u * w + 1u;
    const ptl_u32 slot_dwords = (ptl_u32)min(slot_stride >> 2, (ptl_u64)0xffffffffu);

    for (ptl_u32 band = blockIdx.x; band < n_bands; band += gridDim.x) {
        const ptl_u32 y_first = band * band_rows, y_end = min(h, y_first + band_rows);
        const ptl_u32 g_begin = y_first * row_bytes, g_end = y_end * row_bytes;  // at most 2^31
        ptl_u32* const slot = reinterpret_cast<ptl_u32*>(slots + (ptl_u64)band * slot_stride);
        ptl_png_band_state state = {3u, 2u, 0u, 0u, 0u};  // BFINAL = 0, BTYPE = 01: bits 0, 1, 0 in the order they are packed

        for (ptl_u32 g0 = g_begin; g0 < g_end; g0 += ptl_png_segment_bytes) {
            const ptl_u32 n = min(ptl_png_segment_bytes, g_end - g0);
            // (the barrier that ended the last segment -- or the last band -- lets `bits` and `raw` be written again)
            ptl_png_clear_bits(lds, state);
            ptl_png_raw_to_lds(frame, w, y_end, g0, n, raw);
            __syncthreads();
            ptl_png_lane_runs runs;
            ptl_png_find_runs<1u>(raw, n, lds.wave_a, lds.wave_b, runs);
            ptl_u32 token[ptl_png_lane_bytes];  // bits | count << 24, 0 where the byte is covered by a match that started before it
            ptl_png_lane_tokens<ptl_png_fixed_tokens>(runs, n, token);
            ptl_png_emit_segment(lds, runs, n, token, slot, slot_dwords, state);
        }
        if (threadIdx.x == 0u) ptl_png_end_band(state, ptl_png_fixed_entry(256u), slot, slot_stride, &table[band], g_end - g_begin);  // end-of-block: 7 zero bits
    }
}

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate_pack_kernel(unsigned char* __restrict__ out, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows, ptl_u32 n_bands,
                                                                               ptl_u32 pixel, ptl_u32 magic, ptl_u64 table_offset, ptl_u64 slots_offset,
                                                                               ptl_u64 slot_stride, ptl_u64 stream_room) {
    __shared__ ptl_u32 store[8];
    const uint4* const table = reinterpret_cast<const uint4*>(out + table_offset);
    const unsigned char* const slots = out + slots_offset;
    const ptl_u32 t = threadIdx.x;
    const ptl_u32 per = (n_bands + gridDim.x - 1u) / gridDim.x;  // bands per workgroup, a contiguous chunk each
    const ptl_u64 first64 = (ptl_u64)blockIdx.x * per;
    const ptl_u32 first = (ptl_u32)min(first64, (ptl_u64)n_bands), last = (ptl_u32)min(first64 + per, (ptl_u64)n_bands);
    ptl_u64 before = 0ull;
    for (ptl_u32 b = t; b < first; b += 256u) before += table[b].x;
    ptl_u64 at = ptl_png_sum64(before, store);
    unsigned char* const stream = out + ptl_png_header_bytes;
    for (ptl_u32 b = first; b < last; ++b) {
        const ptl_u32 used = (ptl_u32)min((ptl_u64)table[b].x, slot_stride);
        const ptl_u32 fits = (ptl_u32)min((ptl_u64)used, stream_room - min(at, stream_room));  // (all of it: a band stays within its bound, the room is the sum of the bounds)
        const unsigned char* const src = slots + (ptl_u64)b * slot_stride;
        for (ptl_u32 i = t; i < fits; i += 256u) stream[at + i] = src[i];
        at += used;
    }
    if (blockIdx.x != 0u) return;
    // the whole stream's size and Adler-32: A = 1 + sum s1, B = N + sum (s2 + s1 * raw bytes behind the band), mod 65521
    const ptl_u64 row_bytes = (ptl_u64)pixel * w + 1ull, n_raw = row_bytes * h;
    ptl_u64 bytes = 0ull, sum1 = 0ull, sum2 = 0ull;
    for (ptl_u32 b = t; b < n_bands; b += 256u) {
        const uint4 e = table[b];
        const ptl_u64 end_row = min((ptl_u64)h, ((ptl_u64)b + 1ull) * band_rows);
        const ptl_u64 behind = (n_raw - end_row * row_bytes) % ptl_png_adler_mod;
        bytes += e.x;
        sum1 += e.y;
        sum2 += (e.z + (ptl_u64)e.y * behind) % ptl_png_adler_mod;
    }
    bytes = ptl_png_sum64(bytes, store);
    sum1 = ptl_png_sum64(sum1, store);
    sum2 = ptl_png_sum64(sum2, store);
    if (t == 0u) {
        const ptl_u32 a = (ptl_u32)((1ull + sum1) % ptl_png_adler_mod), b = (ptl_u32)((n_raw + sum2) % ptl_png_adler_mod);
        ptl_u32* const header = reinterpret_cast<ptl_u32*>(out);
        const ptl_u32 words[16] = {magic, w, h, (ptl_u32)bytes, (b << 16) | a, band_rows, n_bands, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (ptl_u32 k = 0u; k < 16u; ++k) header[k] = words[k];
    }
}
