// yuv420p10.hip -- motion-blur averaging fused with the conversion to what a video encoder consumes:
// N RGBA8 sub-frames in, one planar Y'CbCr 4:2:0 10-bit frame out (the payload of one Y4M frame).
//
// Contract (tests/yuv_reference.py restates it in numpy).  Let A(x, y) = (R, G, B) be the RGBA8 frame
// ptl_average_images would have written (n >= 2: integer mean of c*c, (u8)(sqrt + 0.5); n == 1: the input's own RGB;
// alpha ignored).  BT.709 matrix on the gamma-encoded values, full range, 10 bit, 32-bit integer arithmetic:
//   Y  = (55896 R + 188037 G + 18982 B + 32768) >> 16                                      per pixel
//   S_c = sum over rows 2j, 2j+1 of A_c(2i-1, .) + 2 A_c(2i, .) + A_c(2i+1, .)              coordinates clamped to the frame
//   Cb = min(1023, (-30123 S_R - 101335 S_G + 131458 S_B + (512 << 19) + (1 << 18)) >> 19)  MPEG-2 ("left") siting
//   Cr = min(1023, (131458 S_R - 119404 S_G -  12054 S_B + (512 << 19) + (1 << 18)) >> 19)
// Layout: Y plane W*H little-endian u16, then Cb and Cr, cw*ch each with cw = (W+1)/2, ch = (H+1)/2.
// HBM-bound: reads 4 N bytes and writes 3 bytes per pixel; the averaged RGBA8 frame never exists in memory.
//
// gfx950 mapping, fast path (W % 16 == 0, H even: every video size): a lane owns an 8x2 pixel block = two 16-byte loads per
// row and sub-frame (four in flight per sub-frame, eight with the loop unrolled x2), 48 u32 sums in registers, one 16-byte Y
// store per row and one 8-byte store per chroma plane.  The column left of the block is the neighbouring lane's last
// pixel (one cross-lane move per row); only the first lane of a wave and the first block of a row load it themselves
// (4-byte loads that hit the lines the neighbours stream anyway).  General path (any W, H >= 1): a lane owns one chroma
// sample = a 2x2 luma block with 4-byte loads and 2-byte stores, every coordinate clamped.  No LDS, no atomics, no scratch.
#include "average_common.h"  // pointer lists, ptl_accumulate, ptl_div_n, ptl_l_to_s -- the same functions ptl_average_images runs
#include "yuv_common.h"      // luma, the chroma pair (shift 19 here), the 32-bit-offset loads, ptl_encode3: shared with yuv4xxp10.hip

#ifndef PTL_YUV_UNROLL
#define PTL_YUV_UNROLL 2  // sub-frames per group: 4 x 16-byte loads per lane each
#endif

// Fast path: block b = (row pair j, 8-pixel column group bx), bw = W / 8 groups per row.
template <class Frames>
__device__ __forceinline__ void ptl_yuv_block(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h,
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

// General path: chroma sample t = (i, j) with its up-to-2x2 luma pixels; 4-byte loads, 2-byte stores, coordinates clamped.
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

template <class Frames>
__device__ __forceinline__ void ptl_yuv_frame(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    if ((w & 15) == 0 && (h & 1) == 0) {
        const unsigned int bw = (unsigned)w >> 3, n_blocks = bw * ((unsigned)h >> 1);
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuv_block(frames, n, magic, out, w, h, b, bw);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, ch = ((unsigned)h + 1u) >> 1, n_samples = cw * ch;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuv_sample(frames, n, magic, out, w, h, t, cw, ch);
    }
}

template <class Frames>
__device__ __forceinline__ void ptl_yuv_all(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    // wave-uniform, as in ptl_average_all.  ptl_div_n tests its magic per value (54 of them per block here): one test per launch instead,
    // each side with the answer compiled in -- n == 1, a plain conversion, has no multiply at all
    if (n > 1) ptl_yuv_frame(frames, n, 0xffffffffu / (unsigned)n + 1u, out, w, h);
    else ptl_yuv_frame(frames, n, 0u, out, w, h);
}

extern "C" __global__ void __launch_bounds__(256)
ptl_average_to_yuv420p10_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuv_all(frames, n, out, w, h);
}

// 65..256 sub-frames: the pointers no longer fit the kernel arguments (as for ptl_average_images_table_kernel)
extern "C" __global__ void __launch_bounds__(256)
ptl_average_to_yuv420p10_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuv_all(ptl_frame_table{table}, n, out, w, h);
}
