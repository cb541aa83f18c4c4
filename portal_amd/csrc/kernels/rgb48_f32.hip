// rgb48_f32.hip -- N RGBA32F sub-frames in (the un-quantised vec4 the render entries store as out_rgba32f), the scanlines of one 16-bit
// RGB PNG out (colour type 2, bit depth 16), unfiltered or with PNG's Sub filter already applied: what ptl_png_write_rgb48 deflates as it
// is.  The averaged frame is the one of yuv10_f32.hip; it leaves the card as RGB instead of Y'CbCr.
//
// Contract (include/portal_amd.h; tests/png16_reference.py restates it in numpy on top of yuv_deep_reference.encode16).
// A(x, y) = (E_R, E_G, E_B) is exactly the averaged frame of ptl_average_f32_to_yuv420p10 (q, M, E of yuv_common.h; n == 1: E = q; alpha
// is ignored).  Raw row y, bytes 6x .. 6x+5:
//   E_R >> 8, E_R & 255, E_G >> 8, E_G & 255, E_B >> 8, E_B & 255                        big-endian samples
// and the row as it is written, `Filter` (a template parameter: an entry pair per filter):
//   none  out[y][i] = raw[y][i]
//   sub   out[y][i] = (raw[y][i] - (i >= 6 ? raw[y][i - 6] : 0)) mod 256                  per byte, no borrow; every row starts from zero
// out: H rows of 6 W bytes, packed, no filter-type bytes (the writer adds them: rows stay 8-byte aligned for W % 4 == 0).  HBM-bound: reads
// 16 N bytes and writes 6 bytes per pixel -- the traffic of ptl_average_f32_to_yuv444p10_kernel.
//
// gfx950 mapping, fast path (W % 4 == 0, any H; rgb48_shape.h): a lane owns 4x1 pixels = four adjacent 16-byte loads per sub-frame (eight in
// flight with the loop unrolled x2; a wave reads 4 KiB contiguous), 12 64-bit sums, 24 output bytes at byte offset 24 b as three 8-byte
// stores (a wave writes 1.5 KiB contiguous).  Sub: the pixel left of the block is the neighbouring lane's last pixel AFTER encoding (three
// 16-bit values = two cross-lane dwords), under the rule of yuv10_f32.hip's 4:2:2 block: only the first lane of a wave loads and encodes
// that pixel itself, the first block of a row takes zero.  The difference is taken on dwords of two samples (ptl_rgb48_sub_bytes), the byte
// order is set last.  General path (any W): a lane per pixel, three 2-byte stores; for Sub the pixel left of it is loaded and encoded again
// (slow, like the YUV general paths).  The functions of average_common.h and yuv_common.h stay what they are.  No LDS, no atomics, no scratch.
#include "average_common.h"  // the pointer lists
#include "yuv_common.h"      // ptl_accumulate_f32, ptl_encode16, ptl_load_pixel; the n == 1 split and the entries (PTL_YUV_ENTRIES)
#include "rgb48_shape.h"     // the fast-path predicate, the filters, the two byte transforms: the host sizes the launch by the same text

#ifndef PTL_RGB48_UNROLL
#define PTL_RGB48_UNROLL 2  // sub-frames per group: 4 x 16-byte loads per lane each (the factor of ptl_yuvxf_block; measured beside 1 in profiles/r15)
#endif

// The format of this source for yuv_common.h's split: One as for ptl_rgba32f, and the filter.  The sampling slot of the dispatcher holds 48.
template <bool One, int Filter>
struct ptl_rgb48 {
    static __device__ __forceinline__ int param(int) { return 0; }
    static constexpr int kParamOne = 0;
};

// Fast path: block b = (row y, 4-pixel column group bx), bw = W / 4 groups per row; its 24 bytes start at byte 24 b (4 b = y W + 4 bx).
template <int Filter, bool One, class Frames>
__device__ __forceinline__ void ptl_rgb48_block(const Frames& frames, int n, double inv_n, ptl_u32x2* __restrict__ out, unsigned int b, unsigned int bw) {
    constexpr bool kSub = Filter == ptl_rgb48_filter_sub;
    const unsigned int y = b / bw, bx = b - y * bw;
    const unsigned int v0 = 64u * b;  // byte offset of the block's first pixel
    // Sub only: the pixel left of the block.  The neighbouring lane has it, except for the first lane of a wave; the first block of a row has none (zero)
    const bool load_left = kSub && (threadIdx.x & 63u) == 0u && bx != 0u;
    ptl_u64 sum[4][3] = {};  // [pixel][channel]
    ptl_u64 left[3] = {};
    int f = 0;
    for (; f + PTL_RGB48_UNROLL <= n; f += PTL_RGB48_UNROLL) {
        ptl_f32x4 v[PTL_RGB48_UNROLL][4];
#pragma unroll
        for (int k = 0; k < PTL_RGB48_UNROLL; ++k) {
            const ptl_u32x4* p = frames.frame[f + k];
#pragma unroll
            for (int x = 0; x < 4; ++x) v[k][x] = ptl_load_pixel(p, v0 + 16u * x);
        }
        if (load_left) {
#pragma unroll
            for (int k = 0; k < PTL_RGB48_UNROLL; ++k) ptl_accumulate_f32<One>(left, ptl_load_pixel(frames.frame[f + k], v0 - 16u));
        }
#pragma unroll
        for (int k = 0; k < PTL_RGB48_UNROLL; ++k)
#pragma unroll
            for (int x = 0; x < 4; ++x) ptl_accumulate_f32<One>(sum[x], v[k][x]);
    }
    for (; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        ptl_f32x4 v[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) v[x] = ptl_load_pixel(p, v0 + 16u * x);
        if (load_left) ptl_accumulate_f32<One>(left, ptl_load_pixel(p, v0 - 16u));
#pragma unroll
        for (int x = 0; x < 4; ++x) ptl_accumulate_f32<One>(sum[x], v[x]);
    }
    unsigned int a[5][3] = {};  // [column + 1][channel], column -1 = left of the block (Sub only; zero otherwise)
#pragma unroll
    for (int x = 0; x < 4; ++x) ptl_encode16<One>(a[x + 1], sum[x], inv_n);
    if constexpr (kSub) {
        // the last pixel, encoded, goes one lane up.  Every lane of a block's wave below this one is active: blocks are handed out in lane order and
        // the grid stride is a multiple of the wave, so a trip that ends inside a wave ends above this lane's lower neighbour
        const unsigned int r0 = a[4][0] | (a[4][1] << 16), r1 = a[4][2];
        const unsigned int n0 = (unsigned int)__shfl_up((int)r0, 1), n1 = (unsigned int)__shfl_up((int)r1, 1);
        const unsigned int from_lane[3] = {n0 & 0xffffu, n0 >> 16, n1 & 0xffffu};
        unsigned int mine[3] = {};
        if (load_left) ptl_encode16<One>(mine, left, inv_n);  // (one lane of a wave: the rest does not pay for these three values)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[0][c] = bx == 0u ? 0u : load_left ? mine[c] : from_lane[c];
    }
    // the 15 samples left, p0 .. p3 as a stream of 16-bit values s[0 .. 15): output dword k holds samples s[3 + 2k], s[4 + 2k], and the
    // samples one pixel (three values) before them are s[2k], s[2k + 1]
    unsigned int s[15], d[6];
#pragma unroll
    for (int i = 0; i < 15; ++i) s[i] = a[i / 3][i % 3];
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const unsigned int cur = s[3 + 2 * k] | (s[4 + 2 * k] << 16);
        const unsigned int before = s[2 * k] | (s[2 * k + 1] << 16);
        d[k] = ptl_rgb48_swap16(kSub ? ptl_rgb48_sub_bytes(cur, before) : cur);
    }
    const ptl_u32x2 s0 = {d[0], d[1]}, s1 = {d[2], d[3]}, s2 = {d[4], d[5]};
    out[3u * b] = s0;
    out[3u * b + 1u] = s1;
    out[3u * b + 2u] = s2;
}

// General path: pixel t of row-major order, column x; one 16-byte load per sub-frame (two for Sub), three 2-byte stores at byte 6 t.
template <int Filter, bool One, class Frames>
__device__ __forceinline__ void ptl_rgb48_pixel(const Frames& frames, int n, double inv_n, unsigned short* __restrict__ out, unsigned int t, unsigned int w) {
    constexpr bool kSub = Filter == ptl_rgb48_filter_sub;
    const bool has_left = kSub && t % w != 0u;
    const unsigned int at = 16u * t, at_left = has_left ? at - 16u : at;  // (a row's first pixel reads itself again and takes zero)
    ptl_u64 sum[3] = {}, left[3] = {};
    for (int f = 0; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        const ptl_f32x4 v = ptl_load_pixel(p, at);
        if constexpr (kSub) ptl_accumulate_f32<One>(left, ptl_load_pixel(p, at_left));
        ptl_accumulate_f32<One>(sum, v);
    }
    unsigned int a[3], before[3] = {};
    ptl_encode16<One>(a, sum, inv_n);
    if constexpr (kSub) {
        ptl_encode16<One>(before, left, inv_n);
#pragma unroll
        for (int c = 0; c < 3; ++c) before[c] = has_left ? before[c] : 0u;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) out[3u * t + c] = (unsigned short)ptl_rgb48_swap16(kSub ? ptl_rgb48_sub_bytes(a[c], before[c]) : a[c]);
}

// A frame: whole 4x1 blocks where rgb48_shape.h says so, else pixels; grid-stride either way (the host caps the grid).
template <bool One, int Filter>
struct ptl_yuv_frame<ptl_rgb48<One, Filter>, 48> {
template <class Frames>
static __device__ __forceinline__ void run(const Frames& frames, int n, int, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const unsigned int n_px = (unsigned)w * (unsigned)h;
    const double inv_n = 1.0 / (double)n;
    if (ptl_rgb48_fast((unsigned)w)) {
        const unsigned int bw = (unsigned)w >> 2, n_blocks = n_px >> 2;
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_rgb48_block<Filter, One>(frames, n, inv_n, reinterpret_cast<ptl_u32x2*>(out), b, bw);
    } else {
        for (unsigned int t = first; t < n_px; t += stride) ptl_rgb48_pixel<Filter, One>(frames, n, inv_n, out, t, (unsigned)w);
    }
}
};

// (the template arguments hold commas: named here, so that each is one argument of the macro)
typedef ptl_rgb48<false, ptl_rgb48_filter_none> ptl_rgb48_none_many;
typedef ptl_rgb48<true, ptl_rgb48_filter_none> ptl_rgb48_none_one;
typedef ptl_rgb48<false, ptl_rgb48_filter_sub> ptl_rgb48_sub_many;
typedef ptl_rgb48<true, ptl_rgb48_filter_sub> ptl_rgb48_sub_one;
PTL_YUV_ENTRIES(ptl_average_f32_to_rgb48_none, ptl_rgb48_none_many, ptl_rgb48_none_one, 48)
PTL_YUV_ENTRIES(ptl_average_f32_to_rgb48_sub, ptl_rgb48_sub_many, ptl_rgb48_sub_one, 48)
