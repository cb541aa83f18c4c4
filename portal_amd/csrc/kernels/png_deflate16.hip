// png_deflate16.hip -- the unfiltered rows of a 16-bit RGB frame (ptl_average_f32_to_rgb48 with PTL_PNG_FILTER_NONE) in, the deflate stream of
// its Up-filtered scanlines out: literals and matches at distance 6 -- one pixel -- only, a Huffman code per band, so that the host's part of
// a 16-bit PNG file is a CRC and an fwrite (ptl_png_write_stream_rgb48).  Two kernels on one stream; the contract is the header comment of
// ptl_png_deflate_rgb48 in include/portal_amd.h (tests/png16_deflate_reference.py restates it), the cut into bands and the
// layout of the result buffer are png_deflate16_shape.h's to say.
//
// ptl_png_deflate16_bands_kernel: a 256-thread workgroup per band (grid-stride over the bands), two passes over the band, in the shape of
// png_huffman.hip.  What differs from it:
//   raw    the segment's bytes come from 6-byte pixels, three 16-bit loads of the row and of the row above (a row is only 2-byte aligned when
//          W is odd), Up per byte without borrow (png_deflate16_common.h);
//   scan   a byte is covered when it equals the byte six back; a byte that is not covered starts a run, and from there on the scans and the
//          token rule are png_deflate_common.h's.  Eight bytes in front of the LDS segment are readable;
//   build  the block header says HDIST = 4 and codes the distance lengths 0 0 0 0 1 behind the literal/length lengths as one sequence;
//   emit   a match carries its distance on top of the length's extra bits: the one-bit code and the extra bit 1 (2 bits) in a dynamic
//          block, 00100 and the extra bit (6 bits) in a fixed one;
//   codes  PTL_PNG_CODES_FIXED forces the fixed block in every band, through the same passes.
// Stores to the slot are guarded by its size, so a band can never write outside its slot.
// LDS: 4112 bytes raw + 7696 bytes bits + 1152 histogram + 1152 code table + 2304 node weights + 1152 parents + 576 order + 296 lengths +
// 280 header + 64 per-length counts + 124 of wave totals and shared words = 18908 bytes.  No scratch, no inline assembly, no atomics on global
// memory: nothing has to be cleared between frames.
//
// ptl_png_deflate16_pack_kernel: workgroup c copies the bands of chunk c to their byte offsets in the stream; workgroup 0 also combines the
// bands' Adler pairs -- a band's s1 weighs in s2 with the number of raw bytes behind the band, rows of 6 W + 1 bytes -- and writes the 64-byte
// header with the magic word "PTL6".
#include <hip/hip_runtime.h>

#include "png_deflate16_common.h"

constexpr ptl_u32 kSeg = ptl_png_segment_bytes;
constexpr ptl_u32 kBitDwords = (31u + 15u * kSeg + 31u) / 32u + 3u;  // the carried partial dword and 15 bits per raw byte
constexpr ptl_u32 kSymbols = 286u, kSymbolSlots = 288u, kNodes = 2u * kSymbolSlots, kLimit = 15u, kEndOfBlock = 256u;
constexpr ptl_u32 kDistanceLengths = 5u;                     // HDIST = 4: the lengths 0 0 0 0 1
constexpr ptl_u32 kLengthSlots = kSymbolSlots + 8u;          // the literal/length lengths and behind the last used symbol the five distance lengths
constexpr ptl_u32 kHeaderDwords = 70u;                       // 74 bits, then at most 7 bits for each of 291 lengths
constexpr ptl_u32 kDynamicDistance = 2u, kDynamicDistanceBits = 2u;          // the code 0, then the extra bit 1, in the order they are packed
constexpr ptl_u32 kFixedDistance = 4u | (1u << 5), kFixedDistanceBits = 6u;  // 00100 most-significant bit first, then the extra bit 1
static_assert(kBitDwords == 1924u && 74u + 7u * (kSymbols + kDistanceLengths) <= 32u * (kHeaderDwords - 2u) && kSymbols + kDistanceLengths <= kLengthSlots, "");
// the longest token: a 15-bit length code, 5 extra bits, 2 distance bits (dynamic), or 8 + 5 + 6 (fixed) -- ptl_png_or_bits holds 24
static_assert(kLimit + 5u + kDynamicDistanceBits <= 24u && 8u + 5u + kFixedDistanceBits <= 24u, "the token field of ptl_png_or_bits");
// a segment's bits: a literal at most 15 per byte, a match at most 22 for at least 3 bytes
static_assert(kLimit + 5u + kDynamicDistanceBits <= 3u * 15u, "the bit buffer holds 15 bits per raw byte");

// The contract's code-length code, symbol 0 .. 18: the canonical code of the lengths 3 7 4 4 4 4 4 4 4 4 5 5 6 6 6 7 4 4 3, bit-reversed,
// its length in bits 24 ..; and the 19 lengths, three bits each, in the order RFC 1951 3.2.7 stores them.
__device__ const ptl_u32 kCodeLengthCode[19] = {0x3000000u, 0x700003fu, 0x4000002u, 0x400000au, 0x4000006u, 0x400000eu, 0x4000001u, 0x4000009u, 0x4000005u, 0x400000du,
                                                0x5000007u, 0x5000017u, 0x600000fu, 0x600002fu, 0x600001fu, 0x700007fu, 0x4000003u, 0x400000bu, 0x3000004u};
constexpr ptl_u64 kCodeLengthLengths = 0x1fe9a69659246e4ull;  // 57 bits

__device__ __forceinline__ ptl_u32 ptl_png_fixed_length(ptl_u32 s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }
__device__ __forceinline__ ptl_u32 ptl_png_fixed_entry(ptl_u32 s) {  // RFC 1951 3.2.6, bit-reversed, the length in bits 24 ..
    const ptl_u32 len = ptl_png_fixed_length(s);
    const ptl_u32 code = s < 144u ? 0x30u + s : s < 256u ? 0x190u + (s - 144u) : s < 280u ? s - 256u : 0xC0u + (s - 280u);
    return (__brev(code) >> (32u - len)) | (len << 24);
}

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate16_bands_kernel(const unsigned short* __restrict__ rows, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows,
                                                                                  ptl_u32 n_bands, ptl_u32 codes, uint4* __restrict__ table,
                                                                                  unsigned char* __restrict__ slots, ptl_u64 slot_stride) {
    __shared__ __attribute__((aligned(16))) unsigned char raw_store[16u + kSeg];  // raw[-8 .. -1] are readable (never compared: the first six bytes start runs)
    __shared__ ptl_u32 bits[kBitDwords];
    __shared__ ptl_u32 hist[kSymbolSlots];
    __shared__ ptl_u32 code[kSymbolSlots];       // per symbol: the bit-reversed code, its length in bits 24 ..
    __shared__ ptl_u32 weight[kNodes];           // the leaves in order, the merged nodes behind them; after the merge a merged node's depth
    __shared__ unsigned short parent[kNodes];
    __shared__ unsigned short order[kSymbolSlots];  // the used symbols by (count, symbol)
    __shared__ unsigned char lens[kLengthSlots];    // the code lengths, and behind the last used symbol the five distance lengths
    __shared__ ptl_u32 header[kHeaderDwords];
    __shared__ ptl_u32 per_length[16];
    __shared__ ptl_u32 wave_a[4], wave_b[4], wave_c[4], wave_d[4], wave_e[4], sum_store[8];
    __shared__ ptl_u32 n_used, last_used, header_bits;
    unsigned char* const raw = raw_store + 16;
    const ptl_u32 t = threadIdx.x, lane = t & 63u;
    const ptl_u32 row_bytes = 6u * w + 1u;
    const ptl_u32 slot_dwords = (ptl_u32)min(slot_stride >> 2, (ptl_u64)0xffffffffu);

    for (ptl_u32 band = blockIdx.x; band < n_bands; band += gridDim.x) {
        const ptl_u32 y_first = band * band_rows, y_end = min(h, y_first + band_rows);
        const ptl_u32 g_begin = y_first * row_bytes, g_end = y_end * row_bytes;  // at most 2^31
        ptl_u32* const slot = reinterpret_cast<ptl_u32*>(slots + (ptl_u64)band * slot_stride);

        // (the barrier that ended the last band lets everything be written again)
        for (ptl_u32 k = t; k < kLengthSlots; k += 256u) {
            if (k < kSymbolSlots) {
                hist[k] = 0u;
                code[k] = 0u;
            }
            lens[k] = 0u;
        }
        if (t < 16u) per_length[t] = 0u;
        if (t == 0u) {
            n_used = 0u;
            last_used = 0u;
        }
        __syncthreads();

        // ---- count ----
        for (ptl_u32 g0 = g_begin; g0 < g_end; g0 += kSeg) {
            const ptl_u32 n = min(kSeg, g_end - g0);
            ptl_png16_raw_to_lds(rows, w, y_end, g0, n, raw);
            __syncthreads();
            ptl_png_lane_runs runs;
            ptl_png16_find_runs(raw, n, wave_a, wave_b, runs);
            ptl_u32 token[ptl_png_lane_bytes];
            ptl_png_lane_tokens(runs, n, token);
#pragma unroll
            for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j)
                if (token[j] != 0u) atomicAdd(&hist[ptl_png_token_symbol(token[j])], 1u);
            __syncthreads();
        }
        if (t == 0u) hist[kEndOfBlock] += 1u;
        __syncthreads();

        // ---- build ----
        // the used symbols in order of (count, symbol)
        for (ptl_u32 s = t; s < kSymbols; s += 256u) {
            const ptl_u32 c = hist[s];
            if (c == 0u) continue;
            ptl_u32 rank = 0u;
            for (ptl_u32 q = 0u; q < kSymbols; ++q) {
                const ptl_u32 cq = hist[q];
                rank += (cq != 0u && (cq < c || (cq == c && q < s))) ? 1u : 0u;
            }
            order[rank] = (unsigned short)s;
            weight[rank] = c;
            atomicAdd(&n_used, 1u);
            atomicMax(&last_used, s);
        }
        __syncthreads();
        const ptl_u32 n_leaves = n_used;       // 2 .. 286: at least one literal, and end-of-block
        const ptl_u32 n_lit = last_used + 1u;  // 257 .. 286
        if (t == 0u && n_leaves >= 2u) {
            // two queues: the leaves in order, the merged nodes in the order they are made; the lighter head, the leaf on a tie
            ptl_u32 leaf = 0u, head = n_leaves;
            for (ptl_u32 made = n_leaves; made + 1u < 2u * n_leaves && made < kNodes; ++made) {
                ptl_u32 pick[2];
#pragma unroll
                for (ptl_u32 k = 0u; k < 2u; ++k) {
                    const bool take_leaf = leaf < n_leaves && (head >= made || weight[leaf] <= weight[head]);
                    pick[k] = take_leaf ? leaf : head;
                    leaf += take_leaf ? 1u : 0u;
                    head += take_leaf ? 0u : 1u;
                }
                weight[made] = weight[pick[0]] + weight[pick[1]];
                parent[pick[0]] = (unsigned short)made;
                parent[pick[1]] = (unsigned short)made;
            }
            // the depths of the merged nodes, root first: a parent is made after its children
            const ptl_u32 root = 2u * n_leaves - 2u;
            weight[root] = 0u;
            for (ptl_u32 node = root; node-- > n_leaves;) weight[node] = weight[min((ptl_u32)parent[node], kNodes - 1u)] + 1u;
        }
        __syncthreads();
        for (ptl_u32 j = t; j < n_leaves; j += 256u) atomicAdd(&per_length[min(weight[min((ptl_u32)parent[j], kNodes - 1u)] + 1u, kLimit)], 1u);
        __syncthreads();
        if (t == 0u) {
            // depths beyond 15 were counted at 15: while the code is over-full, one leaf less at 15, and the deepest shorter length that has a
            // leaf gives one up to make two of the next length -- one unit of 2^-15 less each round, the number of leaves kept
            ptl_u32 total = 0u;
            for (ptl_u32 l = 1u; l <= kLimit; ++l) total += per_length[l] << (kLimit - l);
            for (ptl_u32 round = 0u; round < kSymbols && total > (1u << kLimit); ++round) {
                ptl_u32 l = kLimit - 1u;
                while (l > 1u && per_length[l] == 0u) --l;
                per_length[kLimit] -= 1u;
                per_length[l] -= 1u;
                per_length[l + 1u] += 2u;
                total -= 1u;
            }
        }
        __syncthreads();
        // lengths by place in the order: the first per_length[15] symbols get 15, the next per_length[14] get 14 ...
        for (ptl_u32 j = t; j < n_leaves; j += 256u) {
            ptl_u32 before = 0u, len = 0u;
            for (ptl_u32 l = kLimit; l >= 1u; --l) {
                const ptl_u32 c = per_length[l];
                if (len == 0u && j < before + c) len = l;
                before += c;
            }
            lens[min((ptl_u32)order[j], kSymbols - 1u)] = (unsigned char)len;
        }
        __syncthreads();
        // canonical codes (RFC 1951 3.2.2): the first code of the length, plus the number of smaller symbols of that length; and both blocks' bits
        ptl_u64 dynamic_sum = 0ull, fixed_sum = 0ull;
        for (ptl_u32 s = t; s < kSymbols; s += 256u) {
            const ptl_u32 len = lens[s];
            if (len == 0u) continue;
            ptl_u32 first = 0u, mine = 0u;
            for (ptl_u32 l = 1u; l <= kLimit; ++l) {
                first = (first + (l > 1u ? per_length[l - 1u] : 0u)) << 1;
                if (l == len) mine = first;
            }
            for (ptl_u32 q = 0u; q < s; ++q) mine += lens[q] == len ? 1u : 0u;
            code[s] = ((__brev(mine) >> (32u - len)) & ((1u << len) - 1u)) | (len << 24);
            const ptl_u32 c = hist[s], match = s > kEndOfBlock ? 1u : 0u;  // (the length's extra bits are the same in both blocks)
            dynamic_sum += (ptl_u64)c * (len + kDynamicDistanceBits * match);
            fixed_sum += (ptl_u64)c * (ptl_png_fixed_length(s) + kFixedDistanceBits * match);
        }
        dynamic_sum = ptl_png_sum64(dynamic_sum, sum_store);
        fixed_sum = ptl_png_sum64(fixed_sum, sum_store);  // (its first barrier is behind every read of the first sum)
        if (t == 0u) {
            // the block header: BFINAL = 0, BTYPE = 10, HLIT, HDIST = 4, HCLEN = 15, the code-length code's lengths, then the n_lit lengths and
            // the distance lengths 0 0 0 0 1 as one sequence, run by run
            const ptl_u32 at = min(n_lit, kSymbols);
#pragma unroll
            for (ptl_u32 k = 0u; k < kDistanceLengths; ++k) lens[at + k] = k + 1u == kDistanceLengths ? 1u : 0u;
            const ptl_u32 n_seq = at + kDistanceLengths;
            ptl_u64 acc = 4ull | ((ptl_u64)(n_lit - 257u) << 3) | ((ptl_u64)(kDistanceLengths - 1u) << 8) | (15ull << 13);  // 17 bits
            ptl_u32 have = 17u, dw = 0u;
            auto put = [&](ptl_u32 value, ptl_u32 count) {
                acc |= (ptl_u64)value << have;
                have += count;
                if (have >= 32u) {
                    if (dw < kHeaderDwords - 1u) header[dw++] = (ptl_u32)acc;
                    acc >>= 32;
                    have -= 32u;
                }
            };
            auto put_symbol = [&](ptl_u32 symbol, ptl_u32 extra, ptl_u32 extra_bits) {
                const ptl_u32 e = kCodeLengthCode[symbol], len = e >> 24;
                put((e & 0xffffffu) | (extra << len), len + extra_bits);
            };
            put((ptl_u32)kCodeLengthLengths & 0xffffffu, 24u);
            put((ptl_u32)(kCodeLengthLengths >> 24) & 0xffffffu, 24u);
            put((ptl_u32)(kCodeLengthLengths >> 48), 9u);
            ptl_u32 p = 0u;
            for (ptl_u32 guard = 0u; guard < kLengthSlots && p < n_seq; ++guard) {
                const ptl_u32 v = lens[p];
                ptl_u32 e = p + 1u;
                while (e < n_seq && lens[e] == v) ++e;
                ptl_u32 r = e - p;
                p = e;
                if (v == 0u) {
                    for (; r >= 138u; r -= 138u) put_symbol(18u, 127u, 7u);
                    if (r >= 11u)
                        put_symbol(18u, r - 11u, 7u);
                    else if (r >= 3u)
                        put_symbol(17u, r - 3u, 3u);
                    else
                        for (; r > 0u; --r) put_symbol(0u, 0u, 0u);
                } else {
                    const ptl_u32 s = min(v, 15u);
                    put_symbol(s, 0u, 0u);
                    ptl_u32 m = r - 1u;
                    for (; m >= 6u; m -= 6u) put_symbol(16u, 3u, 2u);
                    if (m >= 3u)
                        put_symbol(16u, m - 3u, 2u);
                    else
                        for (; m > 0u; --m) put_symbol(s, 0u, 0u);
                }
            }
            header[dw] = (ptl_u32)acc;  // the partial dword (0 where the header ends on a dword)
            header_bits = 32u * dw + have;
        }
        __syncthreads();
        // ---- the choice: the dynamic block only where it has fewer bits, and never with PTL_PNG_CODES_FIXED ----
        const bool dynamic = codes != 0u && (ptl_u64)header_bits + dynamic_sum < 3ull + fixed_sum;
        const ptl_u32 distance = dynamic ? kDynamicDistance : kFixedDistance, distance_bits = dynamic ? kDynamicDistanceBits : kFixedDistanceBits;
        ptl_u32 n_bits, carry, flushed;
        if (dynamic) {
            flushed = header_bits >> 5;
            for (ptl_u32 k = t; k < flushed; k += 256u)
                if (k < slot_dwords) slot[k] = header[k];
            carry = header[flushed];
            n_bits = header_bits;
        } else {
            for (ptl_u32 s = t; s < kSymbols; s += 256u) code[s] = ptl_png_fixed_entry(s);
            n_bits = 3u;  // BFINAL = 0, BTYPE = 01: bits 0, 1, 0 in the order they are packed
            carry = 2u;
            flushed = 0u;
        }
        ptl_u32 band_s1 = 0u, band_s2 = 0u;
        __syncthreads();

        // ---- emit ----
        for (ptl_u32 g0 = g_begin; g0 < g_end; g0 += kSeg) {
            const ptl_u32 n = min(kSeg, g_end - g0);
            for (ptl_u32 k = t; k < kBitDwords; k += 256u) bits[k] = k == 0u ? carry : 0u;
            ptl_png16_raw_to_lds(rows, w, y_end, g0, n, raw);
            __syncthreads();
            ptl_png_lane_runs runs;
            ptl_png16_find_runs(raw, n, wave_a, wave_b, runs);
            ptl_u32 token[ptl_png_lane_bytes];  // first as symbols, then as bits: the value in the low 24 bits, their number above
            ptl_u32 lane_bits = 0u, s1 = 0u, s2 = 0u;
            {
                ptl_png_lane_tokens(runs, n, token);
                const ptl_u32 i0 = t * ptl_png_lane_bytes;
#pragma unroll
                for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
                    if (token[j] != 0u) {
                        const ptl_u32 s = ptl_png_token_symbol(token[j]), e = code[min(s, kSymbols - 1u)], len = e >> 24;
                        const ptl_u32 own = len + ptl_png_token_extra_bits(token[j]);  // the code and the length's extra bits; a match's distance on top
                        const bool match = s > kEndOfBlock;
                        token[j] = (e & 0xffffffu) | (ptl_png_token_extra(token[j]) << len) | (match ? distance << own : 0u) | ((own + (match ? distance_bits : 0u)) << 24);
                    }
                    if (i0 + j < n) {
                        s1 += runs.b[j];
                        s2 += (n - (i0 + j)) * runs.b[j];
                    }
                    lane_bits += token[j] >> 24;
                }
            }
#pragma unroll
            for (ptl_u32 d = 1u; d < 64u; d <<= 1) {
                s1 += (ptl_u32)__shfl_xor((int)s1, d);
                s2 += (ptl_u32)__shfl_xor((int)s2, d);
            }
            if (lane == 63u) {
                wave_d[t >> 6] = s1;
                wave_e[t >> 6] = s2;
            }
            ptl_u32 below, seg_bits;
            ptl_png_scan(lane_bits, wave_c, below, seg_bits);  // (its barrier is also behind wave_d and wave_e)
            const ptl_u32 seg_s1 = wave_d[0] + wave_d[1] + wave_d[2] + wave_d[3], seg_s2 = wave_e[0] + wave_e[1] + wave_e[2] + wave_e[3];
            const ptl_u32 at_bit = (n_bits & 31u) + below;
            if (at_bit + lane_bits <= 32u * (kBitDwords - 2u)) ptl_png_or_bits(bits, at_bit, token);  // (always: 15 bits per byte at most)
            __syncthreads();
            // the full dwords to the slot, the partial one into the next segment
            const ptl_u32 in_buffer = (n_bits & 31u) + seg_bits, full = min(in_buffer >> 5, kBitDwords - 1u);
            for (ptl_u32 k = t; k < full; k += 256u)
                if (flushed + k < slot_dwords) slot[flushed + k] = bits[k];
            carry = bits[full];
            flushed += full;
            n_bits += seg_bits;
            ptl_png_adler_append(band_s1, band_s2, n, seg_s1, seg_s2);
            __syncthreads();
        }
        if (t == 0u) {
            // end-of-block, the empty stored block: 3 zero bits, padding to the byte, LEN = 0, NLEN = 0xffff
            const ptl_u32 end = code[kEndOfBlock], end_bits = end >> 24;
            const ptl_u64 last = (ptl_u64)carry | ((ptl_u64)(end & 0xffffffu) << (n_bits & 31u));
            const ptl_u32 tail = ((n_bits & 31u) + end_bits + 3u + 7u) >> 3;  // 1 .. 7 bytes, the carried bits in the first of them
            if ((ptl_u64)4u * flushed + tail + 4u <= slot_stride) {
                unsigned char* const p = reinterpret_cast<unsigned char*>(slot + flushed);
                for (ptl_u32 k = 0u; k < tail; ++k) p[k] = (unsigned char)(last >> (8u * k));
                p[tail] = 0u;
                p[tail + 1u] = 0u;
                p[tail + 2u] = 255u;
                p[tail + 3u] = 255u;
            }
            table[band] = make_uint4(4u * flushed + tail + 4u, band_s1, band_s2, g_end - g_begin);
        }
        __syncthreads();
    }
}

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate16_pack_kernel(unsigned char* __restrict__ out, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows, ptl_u32 n_bands,
                                                                                 ptl_u64 table_offset, ptl_u64 slots_offset, ptl_u64 slot_stride, ptl_u64 stream_room) {
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
        const unsigned char* const src = slots + (ptl_u64)b * slot_stride;
        for (ptl_u32 i = t; i < used; i += 256u)
            if (at + i < stream_room) stream[at + i] = src[i];  // (always: a band stays within its bound, the room is the sum of the bounds)
        at += used;
    }
    if (blockIdx.x != 0u) return;
    // the whole stream's size and Adler-32: A = 1 + sum s1, B = N + sum (s2 + s1 * raw bytes behind the band), mod 65521
    const ptl_u64 row_bytes = 6ull * w + 1ull, n_raw = row_bytes * h;
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
        const ptl_u32 words[16] = {ptl_png16_magic, w, h, (ptl_u32)bytes, (b << 16) | a, band_rows, n_bands, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
        for (ptl_u32 k = 0u; k < 16u; ++k) header[k] = words[k];
    }
}
