// yuv420p10_f32.hip -- deep-colour sibling of yuv420p10.hip: N RGBA32F sub-frames in (the un-quantised vec4 the render entries store as
// out_rgba32f), one planar Y'CbCr 4:2:0 10-bit frame out.  The only quantisation before the 10-bit result is one to 16 bits per sub-frame.
//
// Contract (include/portal_amd.h; tests/yuv_deep_reference.py restates it in numpy).  Per channel value v of a sub-frame
//   q(v) = 0 if !(v > 0), 65535 if v >= 1, else (u32) floor(v * 65535.0f + 0.5f)       product and sum each rounded to binary32, no FMA
// and per pixel and channel, integers from here on:
//   M = floor(sum_k q_k^2 / n),   E = the e with e (e - 1) < M <= e (e + 1)             E = floor(sqrt(M) + 1/2); n == 1: E = q
// A(x, y) = (E_R, E_G, E_B); alpha is ignored.  BT.709 on the gamma-encoded values, full range, 10 bit:
//   Y  = (13920 E_R + 46826 E_G + 4727 E_B + (1 << 21)) >> 22                                             32-bit unsigned, per pixel
//   S_c = sum over rows 2j, 2j+1 of A_c(2i-1, .) + 2 A_c(2i, .) + A_c(2i+1, .)     coordinates clamped to the frame, 0 .. 524 280
//   Cb = min(1023, (-15003 S_R - 50470 S_G + 65473 S_B + (512 << 26) + (1 << 25)) >> 26)                  64-bit, always positive
//   Cr = min(1023, ( 65473 S_R - 59470 S_G -  6003 S_B + (512 << 26) + (1 << 25)) >> 26)
// Layout: that of yuv420p10.hip (Y plane W*H little-endian u16, then Cb and Cr, cw*ch each).
// HBM-bound: reads 16 N bytes and writes 3 bytes per pixel.
//
// gfx950 mapping, fast path (W and H even): a lane owns one chroma sample = a 2x2 pixel block = two adjacent 16-byte loads per row and
// sub-frame (four in flight, eight with the loop unrolled x2; a wave reads 2 KiB contiguous per row), 12 64-bit sums, one 4-byte Y store
// per row and one 2-byte store per chroma plane.  The column left of the block is the neighbouring lane's right pixel AFTER encoding: six
// 16-bit values = three cross-lane dwords.  Only the first lane of a wave loads and encodes that column itself; the first block of a row
// clamps to its own column 0.  General path (any W, H >= 1): a lane owns one chroma sample with every coordinate clamped, six 16-byte
// loads per sub-frame, 2-byte stores.  No LDS, no atomics, no scratch.
#include "average_common.h"     // the pointer lists (a sub-frame pointer is typed as 16-byte vectors there; here the four words are floats)
#include "yuv_common.h"         // ptl_q16 .. ptl_encode16, luma, the chroma pair (shift 26 here), ptl_load_pixel: shared with yuv4xxp10_f32.hip

#ifndef PTL_YUVF_UNROLL
#define PTL_YUVF_UNROLL 2  // sub-frames per group: 4 x 16-byte loads per lane each.  Measured at 4K, N = 4 (profiles/r11): 1 (95 VGPRs, five waves per SIMD) 5.53 TB/s,
                           // 2 (107, four waves) 5.12, 4 (150, three waves) 4.90; N = 1 and N = 16 do not tell them apart.  1 is the candidate; 2 is what the tests ran on
#endif

// Fast path: block b = (row pair j, column pair i), bw = W / 2 blocks per row; b is also the index of its chroma sample.
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

// General path: chroma sample t = (i, j) with its up-to-2x2 luma pixels; coordinates clamped, 2-byte stores.
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

template <bool One, class Frames>
__device__ __forceinline__ void ptl_yuvf_frame(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const double inv_n = 1.0 / (double)n;
    if (((w | h) & 1) == 0) {
        const unsigned int bw = (unsigned)w >> 1, n_blocks = bw * ((unsigned)h >> 1);
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuvf_block<One>(frames, n, inv_n, out, w, h, b, bw);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, ch = ((unsigned)h + 1u) >> 1, n_samples = cw * ch;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuvf_sample<One>(frames, n, inv_n, out, w, h, t, cw, ch);
    }
}

template <class Frames>
__device__ __forceinline__ void ptl_yuvf_all(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    // wave-uniform, as in ptl_yuv_all: one test per launch, each side with the answer compiled in
    if (n > 1) ptl_yuvf_frame<false>(frames, n, out, w, h);
    else ptl_yuvf_frame<true>(frames, n, out, w, h);
}

extern "C" __global__ void __launch_bounds__(256)
ptl_average_f32_to_yuv420p10_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvf_all(frames, n, out, w, h);
}

// 65..256 sub-frames: the pointers no longer fit the kernel arguments (as for ptl_average_to_yuv420p10_table_kernel)
extern "C" __global__ void __launch_bounds__(256)
ptl_average_f32_to_yuv420p10_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvf_all(ptl_frame_table{table}, n, out, w, h);
}
