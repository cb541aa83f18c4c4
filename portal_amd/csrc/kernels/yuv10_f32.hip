// yuv10_f32.hip -- the deep-colour form of yuv10.hip: N RGBA32F sub-frames in (the un-quantised vec4 the render entries store as
// out_rgba32f), one planar Y'CbCr 10-bit frame out at 4:2:0, 4:2:2 or 4:4:4.  The only quantisation before the 10-bit result is one to 16
// bits per sub-frame.
//
// Contract (include/portal_amd.h; tests/yuv_deep_reference.py and tests/yuv_chroma_reference.py restate it in
// numpy).  Per channel value v of a sub-frame
//   q(v) = 0 if !(v > 0), 65535 if v >= 1, else (u32) floor(v * 65535.0f + 0.5f)       product and sum each rounded to binary32, no FMA
// and per pixel and channel, integers from here on:
//   M = floor(sum_k q_k^2 / n),   E = the e with e (e - 1) < M <= e (e + 1)             E = floor(sqrt(M) + 1/2); n == 1: E = q
// A(x, y) = (E_R, E_G, E_B); alpha is ignored.  BT.709 on the gamma-encoded values, full range, 10 bit:
//   Y  = (13920 E_R + 46826 E_G + 4727 E_B + (1 << 21)) >> 22                                             32-bit unsigned, per pixel
//   Cb = min(1023, (-15003 S_R - 50470 S_G + 65473 S_B + (512 << k) + (1 << (k-1))) >> k)                  64-bit, always positive
//   Cr = min(1023, ( 65473 S_R - 59470 S_G -  6003 S_B + (512 << k) + (1 << (k-1))) >> k)                  k = 26 at 4:2:0, 25 at 4:2:2, 23 at 4:4:4
// with S_c (0 .. 524 280 at 4:2:0), the plane sizes and the layout of yuv_common.h.  HBM-bound: reads 16 N bytes and writes 3 (4:2:0),
// 4 (4:2:2) or 6 (4:4:4) bytes per pixel.
//
// gfx950 mapping, fast path.  4:2:0 (W and H even): a lane owns one chroma sample = a 2x2 pixel block = two adjacent 16-byte loads per row
// and sub-frame (four in flight, eight with the loop unrolled x2; a wave reads 2 KiB contiguous per row), 12 64-bit sums, one 4-byte Y
// store per row and one 2-byte store per chroma plane.  The column left of the block is the neighbouring lane's right pixel AFTER
// encoding: six 16-bit values = three cross-lane dwords.  Only the first lane of a wave loads and encodes that column itself; the first
// block of a row clamps to its own column 0.  4:2:2 and 4:4:4 (W % 4 == 0, any H): a lane owns 4x1 pixels = four adjacent 16-byte loads per
// sub-frame (eight in flight with the loop unrolled x2; a wave reads 4 KiB contiguous), 12 64-bit sums, one 8-byte Y store.  4:4:4: two
// more 8-byte stores, no neighbour.  4:2:2: one 4-byte store per chroma plane; the pixel left of the block is the neighbouring lane's last
// pixel after encoding (three 16-bit values = two cross-lane dwords), under the rule of the 2x2 block.  General path (any W, H >= 1):
// the lane ownership of yuv10.hip's, 16-byte loads, 2-byte stores, every coordinate clamped.  The functions stay what they were, as there.  No LDS, no atomics, no scratch.
#include "average_common.h"  // the pointer lists (a sub-frame pointer is typed as 16-byte vectors there; here the four words are floats)
#include "yuv_common.h"      // ptl_q16 .. ptl_encode16, luma, the chroma pair by shift, ptl_load_pixel; the n == 1 split and the entries

#ifndef PTL_YUVF_UNROLL
#define PTL_YUVF_UNROLL 2  // 4:2:0, sub-frames per group: 4 x 16-byte loads per lane each.  Measured at 4K, N = 4 (profiles/r11): 1 (95 VGPRs, five waves per SIMD) 5.53 TB/s,
                           // 2 (107, four waves) 5.12, 4 (150, three waves) 4.90; N = 1 and N = 16 do not tell them apart.  1 is the candidate; 2 is what the tests ran on
#endif

#ifndef PTL_YUVXF_UNROLL
#define PTL_YUVXF_UNROLL 2  // 4:2:2 and 4:4:4, sub-frames per group: 4 x 16-byte loads per lane each
#endif

// Fast path, 4:2:0: block b = (row pair j, column pair i), bw = W / 2 blocks per row; b is also the index of its chroma sample.
template <bool One, class Frames>
__device__ __forceinline__ void ptl_yuvf_block(const Frames& frames, int n, double inv_n, unsigned short* __restrict__ out, int w, int h, unsigned int b,
                                               unsigned int bw) {
    const unsigned int j = b / bw, i = b - j * bw;
    const unsigned int px0 = 2u * j * (unsigned)w + 2u * i;          // first pixel of the block's upper row; even
    const unsigned int v0 = 16u * px0, v1 = v0 + 16u * (unsigned)w;  // ... its byte offset, and the lower row's
    // the column left of the block: the neighbouring lane has it, except for the first lane of a wave; the first block of a row has none (it clamps)
    const bool load_left = (threadIdx.x & 63u) == 0u && i != 0u;
    ptl_u64 sum[2][2][3] = {};  // [row][column][channel]
    ptl_u64 left[2][3] = {};
    int f = 0;
    for (; f + PTL_YUVF_UNROLL <= n; f += PTL_YUVF_UNROLL) {
        ptl_f32x4 v[PTL_YUVF_UNROLL][4];
#pragma unroll
        for (int k = 0; k < PTL_YUVF_UNROLL; ++k) {
            const ptl_u32x4* p = frames.frame[f + k];
            v[k][0] = ptl_load_pixel(p, v0);
            v[k][1] = ptl_load_pixel(p, v0 + 16u);
            v[k][2] = ptl_load_pixel(p, v1);
            v[k][3] = ptl_load_pixel(p, v1 + 16u);
        }
        if (load_left) {
#pragma unroll
            for (int k = 0; k < PTL_YUVF_UNROLL; ++k) {
                ptl_accumulate_f32<One>(left[0], ptl_load_pixel(frames.frame[f + k], v0 - 16u));
                ptl_accumulate_f32<One>(left[1], ptl_load_pixel(frames.frame[f + k], v1 - 16u));
            }
        }
#pragma unroll
        for (int k = 0; k < PTL_YUVF_UNROLL; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) ptl_accumulate_f32<One>(sum[q >> 1][q & 1], v[k][q]);
    }
    for (; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        const ptl_f32x4 a = ptl_load_pixel(p, v0), b2 = ptl_load_pixel(p, v0 + 16u), c = ptl_load_pixel(p, v1), d = ptl_load_pixel(p, v1 + 16u);
        if (load_left) {
            ptl_accumulate_f32<One>(left[0], ptl_load_pixel(p, v0 - 16u));
            ptl_accumulate_f32<One>(left[1], ptl_load_pixel(p, v1 - 16u));
        }
        ptl_accumulate_f32<One>(sum[0][0], a);
        ptl_accumulate_f32<One>(sum[0][1], b2);
        ptl_accumulate_f32<One>(sum[1][0], c);
        ptl_accumulate_f32<One>(sum[1][1], d);
    }
    unsigned int a[2][3][3];  // [row][column + 1][channel], column -1 = left of the block
#pragma unroll
    for (int row = 0; row < 2; ++row)
#pragma unroll
        for (int x = 0; x < 2; ++x) ptl_encode16<One>(a[row][x + 1], sum[row][x], inv_n);
    // the right column, encoded, goes one lane up.  Every lane of a block's wave below this one is active: blocks are handed out in lane order and
    // the grid stride is a multiple of the wave, so a trip that ends inside a wave ends above this lane's lower neighbour
    const unsigned int r0 = a[0][2][0] | (a[0][2][1] << 16), r1 = a[0][2][2] | (a[1][2][0] << 16), r2 = a[1][2][1] | (a[1][2][2] << 16);
    const unsigned int n0 = (unsigned int)__shfl_up((int)r0, 1), n1 = (unsigned int)__shfl_up((int)r1, 1), n2 = (unsigned int)__shfl_up((int)r2, 1);
    const unsigned int from_lane[2][3] = {{n0 & 0xffffu, n0 >> 16, n1 & 0xffffu}, {n1 >> 16, n2 & 0xffffu, n2 >> 16}};
    unsigned int mine[2][3] = {};
    if (load_left) {  // (one lane of a wave: the rest does not pay for these six values)
        ptl_encode16<One>(mine[0], left[0], inv_n);
        ptl_encode16<One>(mine[1], left[1], inv_n);
    }
#pragma unroll
    for (int row = 0; row < 2; ++row)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[row][0][c] = i == 0u ? a[row][1][c] : load_left ? mine[row][c] : from_lane[row][c];
    unsigned int* y_out = reinterpret_cast<unsigned int*>(out);
    unsigned int s[3] = {};
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        y_out[(px0 + (row ? (unsigned)w : 0u)) >> 1] = ptl_luma10_16(a[row][1]) | (ptl_luma10_16(a[row][2]) << 16);
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += a[row][0][c] + 2u * a[row][1][c] + a[row][2][c];
    }
    const unsigned int n_px = (unsigned)w * (unsigned)h, c_px = n_px >> 2;  // cw * ch with both even
    out[n_px + b] = (unsigned short)ptl_cb10_16<26>(s);
    out[n_px + c_px + b] = (unsigned short)ptl_cr10_16<26>(s);
}

// General path, 4:2:0: chroma sample t = (i, j) with its up-to-2x2 luma pixels; coordinates clamped, 2-byte stores.
template <bool One, class Frames>
__device__ __forceinline__ void ptl_yuvf_sample(const Frames& frames, int n, double inv_n, unsigned short* __restrict__ out, int w, int h, unsigned int t,
                                                unsigned int cw, unsigned int ch) {
    const unsigned int j = t / cw, i = t - j * cw;
    const int x1 = 2 * (int)i, x0 = max(x1 - 1, 0), x2 = min(x1 + 1, w - 1);
    const int y0 = 2 * (int)j, y1 = min(y0 + 1, h - 1);
    const unsigned int r0 = (unsigned)y0 * (unsigned)w, r1 = (unsigned)y1 * (unsigned)w;
    const unsigned int at[2][3] = {{r0 + x0, r0 + x1, r0 + x2}, {r1 + x0, r1 + x1, r1 + x2}};
    ptl_u64 sum[2][3][3] = {};
    for (int f = 0; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        ptl_f32x4 px[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) px[r][k] = ptl_load_pixel(p, 16u * at[r][k]);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) ptl_accumulate_f32<One>(sum[r][k], px[r][k]);
    }
    unsigned int a[2][3][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) ptl_encode16<One>(a[r][k], sum[r][k], inv_n);
    const bool right = x1 + 1 < w, below = y0 + 1 < h;
    out[at[0][1]] = (unsigned short)ptl_luma10_16(a[0][1]);
    if (right) out[at[0][2]] = (unsigned short)ptl_luma10_16(a[0][2]);
    if (below) out[at[1][1]] = (unsigned short)ptl_luma10_16(a[1][1]);
    if (below && right) out[at[1][2]] = (unsigned short)ptl_luma10_16(a[1][2]);
    unsigned int s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = a[0][0][c] + 2u * a[0][1][c] + a[0][2][c] + a[1][0][c] + 2u * a[1][1][c] + a[1][2][c];
    const unsigned int n_px = (unsigned)w * (unsigned)h, c_px = cw * ch;
    out[n_px + t] = (unsigned short)ptl_cb10_16<26>(s);
    out[n_px + c_px + t] = (unsigned short)ptl_cr10_16<26>(s);
}

// A 4:2:0 frame: whole 2x2 blocks where yuv_shape.h says so, chroma samples otherwise; grid-stride either way (the host caps the grid).
template <bool One>
struct ptl_yuv_frame<ptl_rgba32f<One>, 420> {
template <class Frames>
static __device__ __forceinline__ void run(const Frames& frames, int n, int, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const double inv_n = 1.0 / (double)n;
    if (ptl_yuv_fast(true, 420, (unsigned)w, (unsigned)h)) {
        const unsigned int bw = (unsigned)w >> 1, n_blocks = bw * ((unsigned)h >> 1);
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuvf_block<One>(frames, n, inv_n, out, w, h, b, bw);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, ch = ((unsigned)h + 1u) >> 1, n_samples = cw * ch;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuvf_sample<One>(frames, n, inv_n, out, w, h, t, cw, ch);
    }
}
};

// Fast path, 4:2:2 and 4:4:4: block b = (row y, 4-pixel column group bx), bw = W / 4 groups per row.  Chroma: 422 or 444.
template <int Chroma, bool One, class Frames>
__device__ __forceinline__ void ptl_yuvxf_block(const Frames& frames, int n, double inv_n, unsigned short* __restrict__ out, int w, int h, unsigned int b,
                                                unsigned int bw) {
    constexpr bool kHalf = Chroma == 422;
    const unsigned int y = b / bw, bx = b - y * bw;
    const unsigned int v0 = 64u * b;  // byte offset of the block's first pixel, 4 b = y * W + 4 bx
    // 4:2:2 only: the pixel left of the block.  The neighbouring lane has it, except for the first lane of a wave; the first block of a row has none (it clamps)
    const bool load_left = kHalf && (threadIdx.x & 63u) == 0u && bx != 0u;
    ptl_u64 sum[4][3] = {};  // [pixel][channel]
    ptl_u64 left[3] = {};
    int f = 0;
    for (; f + PTL_YUVXF_UNROLL <= n; f += PTL_YUVXF_UNROLL) {
        ptl_f32x4 v[PTL_YUVXF_UNROLL][4];
#pragma unroll
        for (int k = 0; k < PTL_YUVXF_UNROLL; ++k) {
            const ptl_u32x4* p = frames.frame[f + k];
#pragma unroll
            for (int x = 0; x < 4; ++x) v[k][x] = ptl_load_pixel(p, v0 + 16u * x);
        }
        if (load_left) {
#pragma unroll
            for (int k = 0; k < PTL_YUVXF_UNROLL; ++k) ptl_accumulate_f32<One>(left, ptl_load_pixel(frames.frame[f + k], v0 - 16u));
        }
#pragma unroll
        for (int k = 0; k < PTL_YUVXF_UNROLL; ++k)
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
    unsigned int a[5][3];  // [column + 1][channel], column -1 = left of the block (4:2:2 only)
#pragma unroll
    for (int x = 0; x < 4; ++x) ptl_encode16<One>(a[x + 1], sum[x], inv_n);
    unsigned int yv[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) yv[x] = ptl_luma10_16(a[x + 1]);
    const ptl_u32x2 y_packed = {yv[0] | (yv[1] << 16), yv[2] | (yv[3] << 16)};
    reinterpret_cast<ptl_u32x2*>(out)[b] = y_packed;
    const unsigned int n_px = (unsigned)w * (unsigned)h;  // a multiple of 4
    if constexpr (kHalf) {
        // the last pixel, encoded, goes one lane up.  Every lane of a block's wave below this one is active: blocks are handed out in lane order and
        // the grid stride is a multiple of the wave, so a trip that ends inside a wave ends above this lane's lower neighbour
        const unsigned int r0 = a[4][0] | (a[4][1] << 16), r1 = a[4][2];
        const unsigned int n0 = (unsigned int)__shfl_up((int)r0, 1), n1 = (unsigned int)__shfl_up((int)r1, 1);
        const unsigned int from_lane[3] = {n0 & 0xffffu, n0 >> 16, n1 & 0xffffu};
        unsigned int mine[3] = {};
        if (load_left) ptl_encode16<One>(mine, left, inv_n);  // (one lane of a wave: the rest does not pay for these three values)
#pragma unroll
        for (int c = 0; c < 3; ++c) a[0][c] = bx == 0u ? a[1][c] : load_left ? mine[c] : from_lane[c];
        unsigned int cb[2], cr[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            unsigned int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = a[2 * i][c] + 2u * a[2 * i + 1][c] + a[2 * i + 2][c];
            cb[i] = ptl_cb10_16<25>(s);
            cr[i] = ptl_cr10_16<25>(s);
        }
        const unsigned int c_px = n_px >> 1;  // cw * ch with W even; even, as is the sample index 2 b: 4-byte stores
        unsigned int* c_out = reinterpret_cast<unsigned int*>(out + n_px);
        c_out[b] = cb[0] | (cb[1] << 16);
        c_out[(c_px >> 1) + b] = cr[0] | (cr[1] << 16);
    } else {
        unsigned int cb[4], cr[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            cb[x] = ptl_cb10_16<23>(a[x + 1]);
            cr[x] = ptl_cr10_16<23>(a[x + 1]);
        }
        ptl_u32x2* c_out = reinterpret_cast<ptl_u32x2*>(out + n_px);
        const ptl_u32x2 cb_packed = {cb[0] | (cb[1] << 16), cb[2] | (cb[3] << 16)}, cr_packed = {cr[0] | (cr[1] << 16), cr[2] | (cr[3] << 16)};
        c_out[b] = cb_packed;
        c_out[(n_px >> 2) + b] = cr_packed;
    }
}

// General path, 4:4:4: pixel t; one 16-byte load per sub-frame, three 2-byte stores.
template <bool One, class Frames>
__device__ __forceinline__ void ptl_yuvxf_pixel(const Frames& frames, int n, double inv_n, unsigned short* __restrict__ out, unsigned int t, unsigned int n_px) {
    ptl_u64 sum[3] = {};
    for (int f = 0; f < n; ++f) ptl_accumulate_f32<One>(sum, ptl_load_pixel(frames.frame[f], 16u * t));
    unsigned int a[3];
    ptl_encode16<One>(a, sum, inv_n);
    out[t] = (unsigned short)ptl_luma10_16(a);
    out[n_px + t] = (unsigned short)ptl_cb10_16<23>(a);
    out[2u * n_px + t] = (unsigned short)ptl_cr10_16<23>(a);
}

// General path, 4:2:2: chroma sample t = (i, y) with its up-to-two luma pixels; columns clamped, 2-byte stores.
template <bool One, class Frames>
__device__ __forceinline__ void ptl_yuvxf_sample(const Frames& frames, int n, double inv_n, unsigned short* __restrict__ out, int w, int h, unsigned int t,
                                                 unsigned int cw) {
    const unsigned int y = t / cw, i = t - y * cw;
    const int x1 = 2 * (int)i, x0 = max(x1 - 1, 0), x2 = min(x1 + 1, w - 1);
    const unsigned int r0 = y * (unsigned)w;
    const unsigned int at[3] = {r0 + x0, r0 + x1, r0 + x2};
    ptl_u64 sum[3][3] = {};
    for (int f = 0; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        ptl_f32x4 px[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = ptl_load_pixel(p, 16u * at[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) ptl_accumulate_f32<One>(sum[k], px[k]);
    }
    unsigned int a[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ptl_encode16<One>(a[k], sum[k], inv_n);
    out[at[1]] = (unsigned short)ptl_luma10_16(a[1]);
    if (x1 + 1 < w) out[at[2]] = (unsigned short)ptl_luma10_16(a[2]);
    unsigned int s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = a[0][c] + 2u * a[1][c] + a[2][c];
    const unsigned int n_px = (unsigned)w * (unsigned)h, c_px = cw * (unsigned)h;
    out[n_px + t] = (unsigned short)ptl_cb10_16<25>(s);
    out[n_px + c_px + t] = (unsigned short)ptl_cr10_16<25>(s);
}

// A 4:2:2 or 4:4:4 frame: whole 4x1 blocks where yuv_shape.h says so, else pixels (4:4:4) or chroma samples (4:2:2).
template <bool One, int Chroma>
struct ptl_yuv_frame<ptl_rgba32f<One>, Chroma> {
template <class Frames>
static __device__ __forceinline__ void run(const Frames& frames, int n, int, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const unsigned int n_px = (unsigned)w * (unsigned)h;
    const double inv_n = 1.0 / (double)n;
    if (ptl_yuv_fast(true, Chroma, (unsigned)w, (unsigned)h)) {
        const unsigned int bw = (unsigned)w >> 2, n_blocks = n_px >> 2;
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuvxf_block<Chroma, One>(frames, n, inv_n, out, w, h, b, bw);
    } else if (Chroma == 444) {
        for (unsigned int t = first; t < n_px; t += stride) ptl_yuvxf_pixel<One>(frames, n, inv_n, out, t, n_px);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, n_samples = cw * (unsigned)h;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuvxf_sample<One>(frames, n, inv_n, out, w, h, t, cw);
    }
}
};

PTL_YUV_ENTRIES(ptl_average_f32_to_yuv420p10, ptl_rgba32f<false>, ptl_rgba32f<true>, 420)
PTL_YUV_ENTRIES(ptl_average_f32_to_yuv422p10, ptl_rgba32f<false>, ptl_rgba32f<true>, 422)
PTL_YUV_ENTRIES(ptl_average_f32_to_yuv444p10, ptl_rgba32f<false>, ptl_rgba32f<true>, 444)
