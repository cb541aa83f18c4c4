// yuv10.hip -- motion-blur averaging fused with the conversion to what a video encoder consumes: N RGBA8 sub-frames in, one planar
// Y'CbCr 10-bit frame out (the payload of one Y4M frame) at 4:2:0, 4:2:2 or 4:4:4.
//
// Contract (tests/yuv_reference.py and tests/yuv_chroma_reference.py restate it in numpy).  Let A(x, y) = (R, G, B)
// be the RGBA8 frame ptl_average_images would have written (n >= 2: integer mean of c*c, (u8)(sqrt + 0.5); n == 1: the input's own RGB;
// alpha ignored).  BT.709 matrix on the gamma-encoded values, full range, 10 bit, 32-bit integer arithmetic:
//   Y  = (55896 R + 188037 G + 18982 B + 32768) >> 16                                      per pixel
//   Cb = min(1023, (-30123 S_R - 101335 S_G + 131458 S_B + (512 << k) + (1 << (k-1))) >> k)  k = 19 at 4:2:0, 18 at 4:2:2, 16 at 4:4:4
//   Cr = min(1023, (131458 S_R - 119404 S_G -  12054 S_B + (512 << k) + (1 << (k-1))) >> k)
// with S_c, the plane sizes and the layout of yuv_common.h.  HBM-bound: reads 4 N bytes and writes 3 (4:2:0), 4 (4:2:2) or 6 (4:4:4)
// bytes per pixel; the averaged RGBA8 frame never exists in memory.
//
// gfx950 mapping, fast path.  4:2:0 (W % 16 == 0, H even: every video size): a lane owns an 8x2 pixel block = two 16-byte loads per
// row and sub-frame (four in flight per sub-frame, eight with the loop unrolled x2), 48 u32 sums in registers, one 16-byte Y
// store per row and one 8-byte store per chroma plane.  4:2:2 and 4:4:4 (W % 8 == 0, any H): a lane owns 8x1 pixels = two 16-byte loads
// per sub-frame (eight in flight with the loop unrolled x4), 24 u32 sums, one 16-byte Y store; 4:2:2: one 8-byte store per chroma plane;
// 4:4:4: two more 16-byte stores, no neighbour.  Where chroma has taps, the column left of the block is the neighbouring lane's last
// pixel (one cross-lane move per row); only the first lane of a wave and the first block of a row load it themselves
// (4-byte loads that hit the lines the neighbours stream anyway).  General path (any W, H >= 1): a lane owns one chroma
// sample with its up-to-2x2 (4:2:0) or up-to-two (4:2:2) luma pixels, at 4:4:4 one pixel; 4-byte loads, 2-byte stores, every coordinate
// clamped.  The block shapes, the general paths and the two dispatchers stay the functions they were: folded, every entry compiled to
// other code, and measured against this form the folds lost bandwidth (profiles/r14).  No LDS, no atomics, no scratch.
#include "average_common.h"  // pointer lists, ptl_accumulate, ptl_div_n, ptl_l_to_s -- the same functions ptl_average_images runs
#include "yuv_common.h"      // luma, the chroma pair by shift, the 32-bit-offset loads, ptl_encode3; the n == 1 split and the entries

#ifndef PTL_YUV_UNROLL
#define PTL_YUV_UNROLL 2  // 4:2:0, sub-frames per group: 4 x 16-byte loads per lane each
#endif
#ifndef PTL_YUVX_UNROLL
#define PTL_YUVX_UNROLL 4  // 4:2:2 and 4:4:4, sub-frames per group: 2 x 16-byte loads per lane each
#endif

// Fast path, 4:2:0: block b = (row pair j, 8-pixel column group bx), bw = W / 8 groups per row.
template <class Frames>
__device__ __forceinline__ void ptl_yuv_block_8x2(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h,
                                              unsigned int b, unsigned int bw) {
    const unsigned int j = b / bw, bx = b - j * bw;
    const unsigned int px0 = 2u * j * (unsigned)w + 8u * bx;        // first pixel of the block's upper row; a multiple of 8
    const unsigned int v0 = 4u * px0, v1 = v0 + 4u * (unsigned)w;   // ... its byte offset, and the lower row's
    // the column left of the block: the neighbouring lane has it, except for the first lane of a wave; the first block of a row clamps to its own column 0
    const bool own_left = (threadIdx.x & 63u) == 0u || bx == 0u;
    const unsigned int l0 = v0 - (bx ? 4u : 0u), l1 = l0 + 4u * (unsigned)w;
    unsigned int sum[4][12] = {};  // [row * 2 + half][3 * pixel + channel]
    unsigned int left[2][3] = {};
    int f = 0;
    for (; f + PTL_YUV_UNROLL <= n; f += PTL_YUV_UNROLL) {
        ptl_u32x4 v[PTL_YUV_UNROLL][4];
#pragma unroll
        for (int k = 0; k < PTL_YUV_UNROLL; ++k) {
            const ptl_u32x4* p = frames.frame[f + k];
            v[k][0] = ptl_load16(p, v0);
            v[k][1] = ptl_load16(p, v0 + 16u);
            v[k][2] = ptl_load16(p, v1);
            v[k][3] = ptl_load16(p, v1 + 16u);
        }
        if (own_left) {
#pragma unroll
            for (int k = 0; k < PTL_YUV_UNROLL; ++k) {
                ptl_accumulate_pixel(left[0], ptl_load4(frames.frame[f + k], l0));
                ptl_accumulate_pixel(left[1], ptl_load4(frames.frame[f + k], l1));
            }
        }
#pragma unroll
        for (int k = 0; k < PTL_YUV_UNROLL; ++k)
#pragma unroll
            for (int q = 0; q < 4; ++q) ptl_accumulate(sum[q], v[k][q]);
    }
    for (; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        const ptl_u32x4 a = ptl_load16(p, v0), b2 = ptl_load16(p, v0 + 16u), c = ptl_load16(p, v1), d = ptl_load16(p, v1 + 16u);
        if (own_left) {
            ptl_accumulate_pixel(left[0], ptl_load4(p, l0));
            ptl_accumulate_pixel(left[1], ptl_load4(p, l1));
        }
        ptl_accumulate(sum[0], a);
        ptl_accumulate(sum[1], b2);
        ptl_accumulate(sum[2], c);
        ptl_accumulate(sum[3], d);
    }
    // row by row, so that a row's sums are dead before the next row's are touched: the averaged frame's bytes, their luma, and
    // the row's share of the four chroma samples' weighted sums
    ptl_u32x4* y_out = reinterpret_cast<ptl_u32x4*>(out);
    int s[4][3] = {};
#pragma unroll
    for (int row = 0; row < 2; ++row) {
        unsigned int a[9][3];  // [column + 1][channel], column -1 = left of the block
#pragma unroll
        for (int x = 0; x < 8; ++x) ptl_encode3(a[x + 1], &sum[row * 2 + (x >> 2)][3 * (x & 3)], magic);
        unsigned int mine[3];
        ptl_encode3(mine, left[row], magic);
        const unsigned int last = a[8][0] | (a[8][1] << 8) | (a[8][2] << 16);
        const unsigned int from_lane = (unsigned int)__shfl_up((int)last, 1);  // every lane of a block's wave below this one is active
#pragma unroll
        for (int c = 0; c < 3; ++c) a[0][c] = own_left ? mine[c] : (from_lane >> (8 * c)) & 0xffu;
        unsigned int y[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) y[x] = ptl_luma10(a[x + 1]);
        const ptl_u32x4 packed = {y[0] | (y[1] << 16), y[2] | (y[3] << 16), y[4] | (y[5] << 16), y[6] | (y[7] << 16)};
        y_out[(px0 + (row ? (unsigned)w : 0u)) >> 3] = packed;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) s[i][c] += (int)(a[2 * i][c] + 2u * a[2 * i + 1][c] + a[2 * i + 2][c]);
    }
    unsigned int cb[4], cr[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        cb[i] = ptl_cb10<19>(s[i]);
        cr[i] = ptl_cr10<19>(s[i]);
    }
    const unsigned int n_px = (unsigned)w * (unsigned)h, c_px = n_px >> 2;  // cw * ch with both even
    const unsigned int ci = j * ((unsigned)w >> 1) + 4u * bx;                // a multiple of 4: 8-byte stores
    ptl_u32x2* c_out = reinterpret_cast<ptl_u32x2*>(out + n_px);
    const ptl_u32x2 cb_packed = {cb[0] | (cb[1] << 16), cb[2] | (cb[3] << 16)}, cr_packed = {cr[0] | (cr[1] << 16), cr[2] | (cr[3] << 16)};
    c_out[ci >> 2] = cb_packed;
    c_out[(c_px + ci) >> 2] = cr_packed;
}

// General path, 4:2:0: chroma sample t = (i, j) with its up-to-2x2 luma pixels; 4-byte loads, 2-byte stores, coordinates clamped.
template <class Frames>
__device__ __forceinline__ void ptl_yuv_sample(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h,
                                               unsigned int t, unsigned int cw, unsigned int ch) {
    const unsigned int j = t / cw, i = t - j * cw;
    const int x1 = 2 * (int)i, x0 = max(x1 - 1, 0), x2 = min(x1 + 1, w - 1);
    const int y0 = 2 * (int)j, y1 = min(y0 + 1, h - 1);
    const unsigned int r0 = (unsigned)y0 * (unsigned)w, r1 = (unsigned)y1 * (unsigned)w;
    const unsigned int at[2][3] = {{r0 + x0, r0 + x1, r0 + x2}, {r1 + x0, r1 + x1, r1 + x2}};
    unsigned int sum[2][3][3] = {};
    for (int f = 0; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        unsigned int px[2][3];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) px[r][k] = ptl_load4(p, 4u * at[r][k]);
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int k = 0; k < 3; ++k) ptl_accumulate_pixel(sum[r][k], px[r][k]);
    }
    unsigned int a[2][3][3];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) ptl_encode3(a[r][k], sum[r][k], magic);
    const bool right = x1 + 1 < w, below = y0 + 1 < h;
    out[at[0][1]] = (unsigned short)ptl_luma10(a[0][1]);
    if (right) out[at[0][2]] = (unsigned short)ptl_luma10(a[0][2]);
    if (below) out[at[1][1]] = (unsigned short)ptl_luma10(a[1][1]);
    if (below && right) out[at[1][2]] = (unsigned short)ptl_luma10(a[1][2]);
    int s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = (int)(a[0][0][c] + 2u * a[0][1][c] + a[0][2][c] + a[1][0][c] + 2u * a[1][1][c] + a[1][2][c]);
    const unsigned int n_px = (unsigned)w * (unsigned)h, c_px = cw * ch;
    out[n_px + t] = (unsigned short)ptl_cb10<19>(s);
    out[n_px + c_px + t] = (unsigned short)ptl_cr10<19>(s);
}

// A 4:2:0 frame: whole 8x2 blocks where yuv_shape.h says so, chroma samples otherwise; grid-stride either way (the host caps the grid).
constexpr bool ptl_yuv_fast_420_as_spelled() {
    for (unsigned int w = 1; w <= 64; ++w)
        for (unsigned int h = 1; h <= 4; ++h)
            if (ptl_yuv_fast(false, 420, w, h) != ((w & 15) == 0 && (h & 1) == 0)) return false;
    return true;
}
static_assert(ptl_yuv_fast_420_as_spelled(), "the 4:2:0 dispatcher's fast-path test is not yuv_shape.h's");
template <>
struct ptl_yuv_frame<ptl_rgba8, 420> {
template <class Frames>
static __device__ __forceinline__ void run(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    if ((w & 15) == 0 && (h & 1) == 0) {  // ptl_yuv_fast(false, 420, w, h), spelled out: through the helper the entry compiles to other code; held to it below
        const unsigned int bw = (unsigned)w >> 3, n_blocks = bw * ((unsigned)h >> 1);
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuv_block_8x2(frames, n, magic, out, w, h, b, bw);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, ch = ((unsigned)h + 1u) >> 1, n_samples = cw * ch;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuv_sample(frames, n, magic, out, w, h, t, cw, ch);
    }
}
};

// Fast path, 4:2:2 and 4:4:4: block b = (row y, 8-pixel column group bx), bw = W / 8 groups per row.  Chroma: 422 or 444.
template <int Chroma, class Frames>
__device__ __forceinline__ void ptl_yuv_block_8x1(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h,
                                               unsigned int b, unsigned int bw) {
    constexpr bool kHalf = Chroma == 422;
    const unsigned int y = b / bw, bx = b - y * bw;
    const unsigned int px0 = 8u * b;  // first pixel of the block = y * W + 8 bx; a multiple of 8
    const unsigned int v0 = 4u * px0;
    // 4:2:2 only: the column left of the block.  The neighbouring lane has it, except for the first lane of a wave; the first block of a row clamps to its own column 0
    const bool own_left = kHalf && ((threadIdx.x & 63u) == 0u || bx == 0u);
    const unsigned int l0 = v0 - (bx ? 4u : 0u);
    unsigned int sum[2][12] = {};  // [half][3 * pixel + channel]
    unsigned int left[3] = {};
    int f = 0;
    for (; f + PTL_YUVX_UNROLL <= n; f += PTL_YUVX_UNROLL) {
        ptl_u32x4 v[PTL_YUVX_UNROLL][2];
#pragma unroll
        for (int k = 0; k < PTL_YUVX_UNROLL; ++k) {
            const ptl_u32x4* p = frames.frame[f + k];
            v[k][0] = ptl_load16(p, v0);
            v[k][1] = ptl_load16(p, v0 + 16u);
        }
        if (own_left) {
#pragma unroll
            for (int k = 0; k < PTL_YUVX_UNROLL; ++k) ptl_accumulate_pixel(left, ptl_load4(frames.frame[f + k], l0));
        }
#pragma unroll
        for (int k = 0; k < PTL_YUVX_UNROLL; ++k) {
            ptl_accumulate(sum[0], v[k][0]);
            ptl_accumulate(sum[1], v[k][1]);
        }
    }
    for (; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        const ptl_u32x4 a = ptl_load16(p, v0), b2 = ptl_load16(p, v0 + 16u);
        if (own_left) ptl_accumulate_pixel(left, ptl_load4(p, l0));
        ptl_accumulate(sum[0], a);
        ptl_accumulate(sum[1], b2);
    }
    unsigned int a[9][3];  // [column + 1][channel], column -1 = left of the block (4:2:2 only)
#pragma unroll
    for (int x = 0; x < 8; ++x) ptl_encode3(a[x + 1], &sum[x >> 2][3 * (x & 3)], magic);
    unsigned int yv[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) yv[x] = ptl_luma10(a[x + 1]);
    const ptl_u32x4 packed = {yv[0] | (yv[1] << 16), yv[2] | (yv[3] << 16), yv[4] | (yv[5] << 16), yv[6] | (yv[7] << 16)};
    reinterpret_cast<ptl_u32x4*>(out)[b] = packed;
    const unsigned int n_px = (unsigned)w * (unsigned)h;  // a multiple of 8
    if constexpr (kHalf) {
        unsigned int mine[3];
        ptl_encode3(mine, left, magic);
        const unsigned int last = a[8][0] | (a[8][1] << 8) | (a[8][2] << 16);
        const unsigned int from_lane = (unsigned int)__shfl_up((int)last, 1);  // every lane of a block's wave below this one is active
#pragma unroll
        for (int c = 0; c < 3; ++c) a[0][c] = own_left ? mine[c] : (from_lane >> (8 * c)) & 0xffu;
        unsigned int cb[4], cr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int s[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = (int)(a[2 * i][c] + 2u * a[2 * i + 1][c] + a[2 * i + 2][c]);
            cb[i] = ptl_cb10<18>(s);
            cr[i] = ptl_cr10<18>(s);
        }
        const unsigned int c_px = n_px >> 1;  // cw * ch with W even; a multiple of 4, as is the sample index 4 b: 8-byte stores
        ptl_u32x2* c_out = reinterpret_cast<ptl_u32x2*>(out + n_px);
        const ptl_u32x2 cb_packed = {cb[0] | (cb[1] << 16), cb[2] | (cb[3] << 16)}, cr_packed = {cr[0] | (cr[1] << 16), cr[2] | (cr[3] << 16)};
        c_out[b] = cb_packed;
        c_out[(c_px >> 2) + b] = cr_packed;
    } else {
        unsigned int cb[8], cr[8];
#pragma unroll
        for (int x = 0; x < 8; ++x) {
            const int s[3] = {(int)a[x + 1][0], (int)a[x + 1][1], (int)a[x + 1][2]};
            cb[x] = ptl_cb10<16>(s);
            cr[x] = ptl_cr10<16>(s);
        }
        ptl_u32x4* c_out = reinterpret_cast<ptl_u32x4*>(out + n_px);
        const ptl_u32x4 cb_packed = {cb[0] | (cb[1] << 16), cb[2] | (cb[3] << 16), cb[4] | (cb[5] << 16), cb[6] | (cb[7] << 16)};
        const ptl_u32x4 cr_packed = {cr[0] | (cr[1] << 16), cr[2] | (cr[3] << 16), cr[4] | (cr[5] << 16), cr[6] | (cr[7] << 16)};
        c_out[b] = cb_packed;
        c_out[(n_px >> 3) + b] = cr_packed;
    }
}

// General path, 4:4:4: pixel t; one 4-byte load per sub-frame, three 2-byte stores.
template <class Frames>
__device__ __forceinline__ void ptl_yuvx_pixel(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, unsigned int t,
                                               unsigned int n_px) {
    unsigned int sum[3] = {};
    for (int f = 0; f < n; ++f) ptl_accumulate_pixel(sum, ptl_load4(frames.frame[f], 4u * t));
    unsigned int a[3];
    ptl_encode3(a, sum, magic);
    const int s[3] = {(int)a[0], (int)a[1], (int)a[2]};
    out[t] = (unsigned short)ptl_luma10(a);
    out[n_px + t] = (unsigned short)ptl_cb10<16>(s);
    out[2u * n_px + t] = (unsigned short)ptl_cr10<16>(s);
}

// General path, 4:2:2: chroma sample t = (i, y) with its up-to-two luma pixels; 4-byte loads, 2-byte stores, columns clamped.
template <class Frames>
__device__ __forceinline__ void ptl_yuvx_sample(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h,
                                                unsigned int t, unsigned int cw) {
    const unsigned int y = t / cw, i = t - y * cw;
    const int x1 = 2 * (int)i, x0 = max(x1 - 1, 0), x2 = min(x1 + 1, w - 1);
    const unsigned int r0 = y * (unsigned)w;
    const unsigned int at[3] = {r0 + x0, r0 + x1, r0 + x2};
    unsigned int sum[3][3] = {};
    for (int f = 0; f < n; ++f) {
        const ptl_u32x4* p = frames.frame[f];
        unsigned int px[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) px[k] = ptl_load4(p, 4u * at[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) ptl_accumulate_pixel(sum[k], px[k]);
    }
    unsigned int a[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ptl_encode3(a[k], sum[k], magic);
    out[at[1]] = (unsigned short)ptl_luma10(a[1]);
    if (x1 + 1 < w) out[at[2]] = (unsigned short)ptl_luma10(a[2]);
    int s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = (int)(a[0][c] + 2u * a[1][c] + a[2][c]);
    const unsigned int n_px = (unsigned)w * (unsigned)h, c_px = cw * (unsigned)h;
    out[n_px + t] = (unsigned short)ptl_cb10<18>(s);
    out[n_px + c_px + t] = (unsigned short)ptl_cr10<18>(s);
}

// A 4:2:2 or 4:4:4 frame: whole 8x1 blocks where yuv_shape.h says so, else pixels (4:4:4) or chroma samples (4:2:2).
template <int Chroma>
struct ptl_yuv_frame<ptl_rgba8, Chroma> {
template <class Frames>
static __device__ __forceinline__ void run(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const unsigned int n_px = (unsigned)w * (unsigned)h;
    if (ptl_yuv_fast(false, Chroma, (unsigned)w, (unsigned)h)) {
        const unsigned int bw = (unsigned)w >> 3, n_blocks = n_px >> 3;
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuv_block_8x1<Chroma>(frames, n, magic, out, w, h, b, bw);
    } else if (Chroma == 444) {
        for (unsigned int t = first; t < n_px; t += stride) ptl_yuvx_pixel(frames, n, magic, out, t, n_px);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, n_samples = cw * (unsigned)h;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuvx_sample(frames, n, magic, out, w, h, t, cw);
    }
}
};

PTL_YUV_ENTRIES(ptl_average_to_yuv420p10, ptl_rgba8, ptl_rgba8, 420)
PTL_YUV_ENTRIES(ptl_average_to_yuv422p10, ptl_rgba8, ptl_rgba8, 422)
PTL_YUV_ENTRIES(ptl_average_to_yuv444p10, ptl_rgba8, ptl_rgba8, 444)
