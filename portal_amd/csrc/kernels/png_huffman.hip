// png_huffman.hip -- the bands of the two deflate paths that build a Huffman code per band, as one two-pass body over a pixel format:
//   ptl_png_huffman_bands_kernel    ptl_png_deflate_rgba8_codes(PTL_PNG_CODES_DYNAMIC): an RGBA8 frame, the same tokens as png_deflate.hip
//                                   (literals and matches at distance 1; DESIGN.md 2.3.6, tests/png_huffman_reference.py restates it);
//   ptl_png_deflate16_bands_kernel  ptl_png_deflate_rgb48: the unfiltered rows of a 16-bit RGB frame (ptl_average_f32_to_rgb48 with
//                                   PTL_PNG_FILTER_NONE), literals and matches at distance 6 -- one pixel (DESIGN.md 2.3.7,
//                                   tests/png16_deflate_reference.py restates it).  `codes` = PTL_PNG_CODES_FIXED forces the fixed block in
//                                   every band, through the same passes.
// Every band is emitted as the dynamic block (RFC 1951 3.2.7) with its own length-limited code or as the fixed block, whichever has fewer
// bits.  The contracts are the header comments of those two functions in include/portal_amd.h; a band's table entry is the one
// ptl_png_deflate_pack_kernel (png_deflate.hip) reads, so that kernel packs these bands.  The steps a band shares with the fixed kernel are
// png_deflate_common.h's.
//
// ptl_png_two_pass_bands: a 256-thread workgroup per band (grid-stride over the bands), two passes over the band, in three parts.
//   count  per segment the raw bytes into LDS, the run scan at the format's distance, the tokens as symbols; the lane that holds a token's
//          first byte adds it to the 286-entry LDS histogram (ds_add per token, not per byte).  End-of-block counts once.
//   build  in LDS.  The used symbols in order of (count, symbol) by ranking (a lane per symbol, 286 comparisons each); the two-queue merge and
//          the depths of the merged nodes serially on lane 0 (at most 285 steps each); leaf depths and the per-length counts by a lane per leaf;
//          the repair of the counts where the tree is deeper than 15 on lane 0 (at most 286 rounds); lengths by place in the order, canonical
//          codes by rank among the symbols of the same length, bit-reversed; the sizes of both blocks by two workgroup sums; the block header
//          -- HDIST and the distance lengths behind the literal/length lengths are the format's: the one length 1, or 0 0 0 0 1 -- serially
//          on lane 0 into an LDS buffer of its own.  Every loop is bounded by a constant, whatever the histogram holds.
//   emit   the header's whole dwords to the slot; the band tokenised again (its rows come from L2), the token bits looked up in the LDS code
//          table -- filled with the fixed code where the fixed block won -- with the format's distance bits for that block type on top of a
//          match's extra bits, shifted together per lane and ORed into the LDS bit buffer, which holds 15 bits per raw byte: a segment may
//          cost that much even though its band stays under the fixed bound; end-of-block, the empty stored block and the table entry by lane 0.
// Stores to the slot are guarded by its size, so a band can never write outside its slot.
// LDS of ptl_png_huffman_bands_kernel: 4112 bytes raw + 7696 bytes bits + 1152 histogram + 1152 code table + 2304 node weights + 1152 parents +
// 576 order + 288 lengths + 272 header + 64 per-length counts + 124 of wave totals and shared words = 18892 bytes.  No scratch, no inline
// assembly, no atomics on global memory: nothing has to be cleared between frames.
// LDS of ptl_png_deflate16_bands_kernel: 296 lengths and 280 header, the rest the same, 4 bytes between two arrays = 18912 bytes.  No scratch either.
#include <hip/hip_runtime.h>

#include "png_deflate_common.h"

constexpr ptl_u32 kSymbols = 286u, kSymbolSlots = 288u, kNodes = 2u * kSymbolSlots, kLimit = 15u, kEndOfBlock = 256u;

// A pixel format: the type the rows are read as (ptl_png_raw_to_lds has an overload for each), the bytes of a pixel, the one distance of its
// matches, the distance lengths the block header codes (all 0 but the last, which is 1: HDIST + 1 of them), what a match carries for its
// distance on top of the length's extra bits in a dynamic and in a fixed block -- the value in the order it is packed, and its bits -- and
// the sizes of the two LDS arrays that depend on the number of lengths.
struct ptl_png_rgba8 {
    typedef ptl_u32 sample;  // a whole pixel
    static constexpr ptl_u32 pixel = ptl_png_pixel8, distance = 1u, distance_lengths = 1u;
    static constexpr ptl_u32 dynamic_distance = 0u, dynamic_distance_bits = 1u;  // the one-bit code 0
    static constexpr ptl_u32 fixed_distance = 0u, fixed_distance_bits = 5u;      // 00000
    static constexpr ptl_u32 length_slots = kSymbolSlots, header_dwords = 68u;   // 74 bits, then at most 7 bits for each of 287 lengths
};
struct ptl_png_rgb48 {
    typedef unsigned short sample;  // big-endian, three to a pixel
    static constexpr ptl_u32 pixel = ptl_png_pixel16, distance = 6u, distance_lengths = 5u;
    static constexpr ptl_u32 dynamic_distance = 2u, dynamic_distance_bits = 2u;          // the code 0, then the extra bit 1
    static constexpr ptl_u32 fixed_distance = 4u | (1u << 5), fixed_distance_bits = 6u;  // 00100 most-significant bit first, then the extra bit 1
    static constexpr ptl_u32 length_slots = kSymbolSlots + 8u, header_dwords = 70u;      // 74 bits, then at most 7 bits for each of 291 lengths
};

// A band's LDS, as the three parts of the body see it.  The arrays are __shared__ variables of their own (ptl_png_two_pass_bands declares
// them) and this struct only refers to them: as members of one __shared__ struct they cost the build of a band with many used symbols about
// 3 us, because the compiler can then no longer tell a store to one array from a load of another (measured: profiles/r22).
template <class F>
struct ptl_png_two_pass_lds {
    ptl_png_segment_lds<15u>& seg;
    ptl_u32 (&hist)[kSymbolSlots];
    ptl_u32 (&code)[kSymbolSlots];    // per symbol: the bit-reversed code, its length in bits 24 ..
    ptl_u32 (&weight)[kNodes];        // the leaves in order, the merged nodes behind them; after the merge a merged node's depth
    unsigned short (&parent)[kNodes];
    unsigned short (&order)[kSymbolSlots];  // the used symbols by (count, symbol)
    ptl_u32 (&per_length)[16];
    ptl_u32 (&sum_store)[8];
    unsigned char (&lens)[F::length_slots];  // the code lengths, and behind the last used symbol the distance lengths
    ptl_u32 (&header)[F::header_dwords];
    ptl_u32 &n_used, &last_used, &header_bits;

    static_assert(74u + 7u * (kSymbols + F::distance_lengths) <= 32u * (F::header_dwords - 2u) && kSymbols + F::distance_lengths <= F::length_slots, "the header's room");
    // the longest token: a 15-bit length code, 5 extra bits and the distance bits (dynamic), or 8 + 5 and the distance bits (fixed)
    static_assert(kLimit + 5u + F::dynamic_distance_bits <= 24u && 8u + 5u + F::fixed_distance_bits <= 24u, "the token field of ptl_png_or_bits");
    // a segment's bits: a literal at most 15 per byte, a match at most 15 + 5 and its distance bits for at least 3 bytes
    static_assert(kLimit + 5u + F::dynamic_distance_bits <= 3u * 15u && ptl_png_segment_lds<15u>::bit_dwords == 1924u, "the bit buffer holds 15 bits per raw byte");
};

// A band: its rows end at y_end, its raw bytes are g_begin .. g_end of the frame's.
struct ptl_png_band {
    ptl_u32 y_end, g_begin, g_end;
};

// count: everything of the last band cleared, then the histogram of the band's tokens.  Barriers: ONE behind the clearing; per segment ONE
// behind the raw bytes, ptl_png_find_runs' ONE, and ONE behind the adds (the raw bytes and the wave totals may be written again); ONE behind
// end-of-block's count.
template <class F>
__device__ __forceinline__ void ptl_png_count(const ptl_png_two_pass_lds<F>& lds, const typename F::sample* __restrict__ frame, ptl_u32 w, const ptl_png_band& band) {
    const ptl_u32 t = threadIdx.x;
    // (the barrier that ended the last band lets everything be written again)
    for (ptl_u32 k = t; k < F::length_slots; k += 256u) {
        if (k < kSymbolSlots) {
            lds.hist[k] = 0u;
            lds.code[k] = 0u;
        }
        lds.lens[k] = 0u;
    }
    if (t < 16u) lds.per_length[t] = 0u;
    if (t == 0u) {
        lds.n_used = 0u;
        lds.last_used = 0u;
    }
    __syncthreads();
    for (ptl_u32 g0 = band.g_begin; g0 < band.g_end; g0 += ptl_png_segment_bytes) {
        const ptl_u32 n = min(ptl_png_segment_bytes, band.g_end - g0);
        ptl_png_raw_to_lds(frame, w, band.y_end, g0, n, lds.seg.raw());
        __syncthreads();
        ptl_png_lane_runs runs;
        ptl_png_find_runs<F::distance>(lds.seg.raw(), n, lds.seg.wave_a, lds.seg.wave_b, runs);
        ptl_u32 token[ptl_png_lane_bytes];
        ptl_png_lane_tokens<ptl_png_symbol_tokens>(runs, n, token);
#pragma unroll
        for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j)
            if (token[j] != 0u) atomicAdd(&lds.hist[ptl_png_token_symbol(token[j])], 1u);
        __syncthreads();
    }
    if (t == 0u) lds.hist[kEndOfBlock] += 1u;
    __syncthreads();
}

// build: the band's code into lds.code, its block header into lds.header, and the choice: true where the dynamic block has fewer bits than
// the fixed one, never with PTL_PNG_CODES_FIXED (`codes` = 0).  Barriers: ONE behind each of the ranking, the merge, the leaf depths, the
// repair and the lengths; ptl_png_sum64's TWO, twice; ONE behind the header.
template <class F>
__device__ __forceinline__ bool ptl_png_build(const ptl_png_two_pass_lds<F>& lds, ptl_u32 codes) {
    const ptl_u32 t = threadIdx.x;
    // the used symbols in order of (count, symbol)
    for (ptl_u32 s = t; s < kSymbols; s += 256u) {
        const ptl_u32 c = lds.hist[s];
        if (c == 0u) continue;
        ptl_u32 rank = 0u;
        for (ptl_u32 q = 0u; q < kSymbols; ++q) {
            const ptl_u32 cq = lds.hist[q];
            rank += (cq != 0u && (cq < c || (cq == c && q < s))) ? 1u : 0u;
        }
        lds.order[rank] = (unsigned short)s;
        lds.weight[rank] = c;
        atomicAdd(&lds.n_used, 1u);
        atomicMax(&lds.last_used, s);
    }
    __syncthreads();
    const ptl_u32 n_leaves = lds.n_used;       // 2 .. 286: at least one literal, and end-of-block
    const ptl_u32 n_lit = lds.last_used + 1u;  // 257 .. 286
    if (t == 0u && n_leaves >= 2u) {
        // two queues: the leaves in order, the merged nodes in the order they are made; the lighter head, the leaf on a tie
        ptl_u32 leaf = 0u, head = n_leaves;
        for (ptl_u32 made = n_leaves; made + 1u < 2u * n_leaves && made < kNodes; ++made) {
            ptl_u32 pick[2];
#pragma unroll
            for (ptl_u32 k = 0u; k < 2u; ++k) {
                const bool take_leaf = leaf < n_leaves && (head >= made || lds.weight[leaf] <= lds.weight[head]);
                pick[k] = take_leaf ? leaf : head;
                leaf += take_leaf ? 1u : 0u;
                head += take_leaf ? 0u : 1u;
            }
            lds.weight[made] = lds.weight[pick[0]] + lds.weight[pick[1]];
            lds.parent[pick[0]] = (unsigned short)made;
            lds.parent[pick[1]] = (unsigned short)made;
        }
        // the depths of the merged nodes, root first: a parent is made after its children
        const ptl_u32 root = 2u * n_leaves - 2u;
        lds.weight[root] = 0u;
        for (ptl_u32 node = root; node-- > n_leaves;) lds.weight[node] = lds.weight[min((ptl_u32)lds.parent[node], kNodes - 1u)] + 1u;
    }
    __syncthreads();
    for (ptl_u32 j = t; j < n_leaves; j += 256u) atomicAdd(&lds.per_length[min(lds.weight[min((ptl_u32)lds.parent[j], kNodes - 1u)] + 1u, kLimit)], 1u);
    __syncthreads();
    if (t == 0u) {
        // depths beyond 15 were counted at 15: while the code is over-full, one leaf less at 15, and the deepest shorter length that has a
        // leaf gives one up to make two of the next length -- one unit of 2^-15 less each round, the number of leaves kept
        ptl_u32 total = 0u;
        for (ptl_u32 l = 1u; l <= kLimit; ++l) total += lds.per_length[l] << (kLimit - l);
        for (ptl_u32 round = 0u; round < kSymbols && total > (1u << kLimit); ++round) {
            ptl_u32 l = kLimit - 1u;
            while (l > 1u && lds.per_length[l] == 0u) --l;
            lds.per_length[kLimit] -= 1u;
            lds.per_length[l] -= 1u;
            lds.per_length[l + 1u] += 2u;
            total -= 1u;
        }
    }
    __syncthreads();
    // lengths by place in the order: the first per_length[15] symbols get 15, the next per_length[14] get 14 ...
    for (ptl_u32 j = t; j < n_leaves; j += 256u) {
        ptl_u32 before = 0u, len = 0u;
        for (ptl_u32 l = kLimit; l >= 1u; --l) {
            const ptl_u32 c = lds.per_length[l];
            if (len == 0u && j < before + c) len = l;
            before += c;
        }
        lds.lens[min((ptl_u32)lds.order[j], kSymbols - 1u)] = (unsigned char)len;
    }
    __syncthreads();
    // canonical codes (RFC 1951 3.2.2): the first code of the length, plus the number of smaller symbols of that length; and both blocks' bits
    ptl_u64 dynamic_sum = 0ull, fixed_sum = 0ull;
    for (ptl_u32 s = t; s < kSymbols; s += 256u) {
        const ptl_u32 len = lds.lens[s];
        if (len == 0u) continue;
        ptl_u32 first = 0u, mine = 0u;
        for (ptl_u32 l = 1u; l <= kLimit; ++l) {
            first = (first + (l > 1u ? lds.per_length[l - 1u] : 0u)) << 1;
            if (l == len) mine = first;
        }
        for (ptl_u32 q = 0u; q < s; ++q) mine += lds.lens[q] == len ? 1u : 0u;
        lds.code[s] = ((__brev(mine) >> (32u - len)) & ((1u << len) - 1u)) | (len << 24);
        const ptl_u32 c = lds.hist[s], match = s > kEndOfBlock ? 1u : 0u;  // (the length's extra bits are the same in both blocks)
        dynamic_sum += (ptl_u64)c * (len + F::dynamic_distance_bits * match);
        fixed_sum += (ptl_u64)c * (ptl_png_fixed_length(s) + F::fixed_distance_bits * match);
    }
    dynamic_sum = ptl_png_sum64(dynamic_sum, lds.sum_store);
    fixed_sum = ptl_png_sum64(fixed_sum, lds.sum_store);  // (its first barrier is behind every read of the first sum)
    if (t == 0u) {
        // the block header: BFINAL = 0, BTYPE = 10, HLIT, HDIST, HCLEN = 15, the code-length code's lengths, then the n_lit lengths and the
        // distance lengths as one sequence, run by run
        const ptl_u32 at = min(n_lit, kSymbols);
#pragma unroll
        for (ptl_u32 k = 0u; k < F::distance_lengths; ++k) lds.lens[at + k] = k + 1u == F::distance_lengths ? 1u : 0u;
        const ptl_u32 n_seq = at + F::distance_lengths;
        ptl_u64 acc = 4ull | ((ptl_u64)(n_lit - 257u) << 3) | ((ptl_u64)(F::distance_lengths - 1u) << 8) | (15ull << 13);  // 17 bits
        ptl_u32 have = 17u, dw = 0u;
        auto put = [&](ptl_u32 value, ptl_u32 count) {
            acc |= (ptl_u64)value << have;
            have += count;
            if (have >= 32u) {
                if (dw < F::header_dwords - 1u) lds.header[dw++] = (ptl_u32)acc;
                acc >>= 32;
                have -= 32u;
            }
        };
        auto put_symbol = [&](ptl_u32 symbol, ptl_u32 extra, ptl_u32 extra_bits) {
            const ptl_u32 e = ptl_png_code_length_code[symbol], len = e >> 24;
            put((e & 0xffffffu) | (extra << len), len + extra_bits);
        };
        put((ptl_u32)ptl_png_code_length_lengths & 0xffffffu, 24u);
        put((ptl_u32)(ptl_png_code_length_lengths >> 24) & 0xffffffu, 24u);
        put((ptl_u32)(ptl_png_code_length_lengths >> 48), 9u);
        ptl_u32 p = 0u;
        for (ptl_u32 guard = 0u; guard < F::length_slots && p < n_seq; ++guard) {
            const ptl_u32 v = lds.lens[p];
            ptl_u32 e = p + 1u;
            while (e < n_seq && lds.lens[e] == v) ++e;
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
        lds.header[dw] = (ptl_u32)acc;  // the partial dword (0 where the header ends on a dword)
        lds.header_bits = 32u * dw + have;
    }
    __syncthreads();
    return codes != 0u && (ptl_u64)lds.header_bits + dynamic_sum < 3ull + fixed_sum;
}

// emit: the chosen block into the band's slot, and the band's table entry.  Barriers: ONE behind the header's dwords or the fixed code in
// the table; per segment ONE behind the raw bytes, ptl_png_find_runs' ONE and ptl_png_emit_segment's THREE; ONE behind lane 0's last bytes,
// which read the code table.
template <class F>
__device__ __forceinline__ void ptl_png_emit(const ptl_png_two_pass_lds<F>& lds, bool dynamic, const typename F::sample* __restrict__ frame, ptl_u32 w, const ptl_png_band& band,
                                             ptl_u32* slot, ptl_u64 slot_stride, uint4* entry) {
    const ptl_u32 t = threadIdx.x;
    const ptl_u32 slot_dwords = (ptl_u32)min(slot_stride >> 2, (ptl_u64)0xffffffffu);
    const ptl_u32 distance = dynamic ? F::dynamic_distance : F::fixed_distance, distance_bits = dynamic ? F::dynamic_distance_bits : F::fixed_distance_bits;
    ptl_png_band_state state = {3u, 2u, 0u, 0u, 0u};  // the fixed block.  BFINAL = 0, BTYPE = 01: bits 0, 1, 0 in the order they are packed
    if (dynamic) {
        state.flushed = lds.header_bits >> 5;
        for (ptl_u32 k = t; k < state.flushed; k += 256u)
            if (k < slot_dwords) slot[k] = lds.header[k];
        state.carry = lds.header[state.flushed];
        state.n_bits = lds.header_bits;
    } else {
        for (ptl_u32 s = t; s < kSymbols; s += 256u) lds.code[s] = ptl_png_fixed_entry(s);
    }
    __syncthreads();
    for (ptl_u32 g0 = band.g_begin; g0 < band.g_end; g0 += ptl_png_segment_bytes) {
        const ptl_u32 n = min(ptl_png_segment_bytes, band.g_end - g0);
        ptl_png_clear_bits(lds.seg, state);
        ptl_png_raw_to_lds(frame, w, band.y_end, g0, n, lds.seg.raw());
        __syncthreads();
        ptl_png_lane_runs runs;
        ptl_png_find_runs<F::distance>(lds.seg.raw(), n, lds.seg.wave_a, lds.seg.wave_b, runs);
        ptl_u32 token[ptl_png_lane_bytes];  // first as symbols, then as bits: the value in the low 24 bits, their number above
        ptl_png_lane_tokens<ptl_png_symbol_tokens>(runs, n, token);
#pragma unroll
        for (ptl_u32 j = 0u; j < ptl_png_lane_bytes; ++j) {
            if (token[j] == 0u) continue;
            const ptl_u32 s = ptl_png_token_symbol(token[j]), e = lds.code[min(s, kSymbols - 1u)], len = e >> 24;
            const ptl_u32 own = len + ptl_png_token_extra_bits(token[j]);  // the code and the length's extra bits; a match's distance on top
            const bool match = s > kEndOfBlock;
            token[j] = (e & 0xffffffu) | (ptl_png_token_extra(token[j]) << len) | (match ? distance << own : 0u) | ((own + (match ? distance_bits : 0u)) << 24);
        }
        ptl_png_emit_segment(lds.seg, runs, n, token, slot, slot_dwords, state);
    }
    if (t == 0u) ptl_png_end_band(state, lds.code[kEndOfBlock], slot, slot_stride, entry, band.g_end - band.g_begin);
    __syncthreads();
}

template <class F>
__device__ __forceinline__ void ptl_png_two_pass_bands(const typename F::sample* __restrict__ frame, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows, ptl_u32 n_bands, ptl_u32 codes,
                                                       uint4* __restrict__ table, unsigned char* __restrict__ slots, ptl_u64 slot_stride) {
    __shared__ __attribute__((aligned(16))) ptl_png_segment_lds<15u> seg;
    __shared__ ptl_u32 hist[kSymbolSlots], code[kSymbolSlots], weight[kNodes], header[F::header_dwords], per_length[16], sum_store[8];
    __shared__ unsigned short parent[kNodes], order[kSymbolSlots];
    __shared__ unsigned char lens[F::length_slots];
    __shared__ ptl_u32 n_used, last_used, header_bits;
    const ptl_png_two_pass_lds<F> lds = {seg, hist, code, weight, parent, order, per_length, sum_store, lens, header, n_used, last_used, header_bits};
    const ptl_u32 row_bytes = F::pixel * w + 1u;
    for (ptl_u32 b = blockIdx.x; b < n_bands; b += gridDim.x) {
        const ptl_u32 y_first = b * band_rows, y_end = min(h, y_first + band_rows);
        const ptl_png_band band = {y_end, y_first * row_bytes, y_end * row_bytes};  // at most 2^31
        ptl_png_count(lds, frame, w, band);
        const bool dynamic = ptl_png_build(lds, codes);
        ptl_png_emit(lds, dynamic, frame, w, band, reinterpret_cast<ptl_u32*>(slots + (ptl_u64)b * slot_stride), slot_stride, &table[b]);
    }
}

extern "C" __global__ __launch_bounds__(256) void ptl_png_huffman_bands_kernel(const ptl_u32* __restrict__ frame, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows,
                                                                                ptl_u32 n_bands, uint4* __restrict__ table, unsigned char* __restrict__ slots,
                                                                                ptl_u64 slot_stride) {
    ptl_png_two_pass_bands<ptl_png_rgba8>(frame, w, h, band_rows, n_bands, 1u, table, slots, slot_stride);  // always PTL_PNG_CODES_DYNAMIC
}

extern "C" __global__ __launch_bounds__(256) void ptl_png_deflate16_bands_kernel(const unsigned short* __restrict__ rows, ptl_u32 w, ptl_u32 h, ptl_u32 band_rows,
                                                                                  ptl_u32 n_bands, ptl_u32 codes, uint4* __restrict__ table,
                                                                                  unsigned char* __restrict__ slots, ptl_u64 slot_stride) {
    ptl_png_two_pass_bands<ptl_png_rgb48>(rows, w, h, band_rows, n_bands, codes, table, slots, slot_stride);
}
