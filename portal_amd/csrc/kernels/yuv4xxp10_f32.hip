// yuv4xxp10_f32.hip -- the 4:2:2 and 4:4:4 siblings of yuv420p10_f32.hip: N RGBA32F sub-frames in, one planar Y'CbCr 10-bit frame out with
// chroma at half the horizontal resolution (4:2:2) or at full resolution (4:4:4).
//
// Contract (include/portal_amd.h; tests/yuv_chroma_reference.py restates it in numpy).  q, M, E, A(x, y) = (E_R, E_G, E_B),
// the luma formula, the plane order and the full-range 10-bit coding are those of yuv420p10_f32.hip; only the chroma sampling differs:
//   4:2:2  cw = (W+1)/2, ch = H   S_c = A_c(2i-1, y) + 2 A_c(2i, y) + A_c(2i+1, y)   columns clamped, co-sited with luma column 2i    k = 25
//   4:4:4  cw = W,       ch = H   S_c = A_c(x, y)                                                                                      k = 23
//   Cb = min(1023, (-15003 S_R - 50470 S_G + 65473 S_B + (512 << k) + (1 << (k-1))) >> k)                  64-bit, always positive
//   Cr = min(1023, ( 65473 S_R - 59470 S_G -  6003 S_B + (512 << k) + (1 << (k-1))) >> k)
// HBM-bound: reads 16 N bytes and writes 4 (4:2:2) or 6 (4:4:4) bytes per pixel.
//
// gfx950 mapping, fast path (W % 4 == 0, any H): a lane owns 4x1 pixels = four adjacent 16-byte loads per sub-frame (eight in flight with
// the loop unrolled x2; a wave reads 4 KiB contiguous), 12 64-bit sums, one 8-byte Y store.  4:4:4: two more 8-byte stores, no neighbour.
// 4:2:2: one 4-byte store per chroma plane; the pixel left of the block is the neighbouring lane's last pixel AFTER encoding (three 16-bit
// values = two cross-lane dwords), only the first lane of a wave loads and encodes it itself, and the first block of a row clamps to its
// own column 0 -- the rule of ptl_yuvf_block.  General path (any W, H >= 1): at 4:4:4 a lane owns one pixel, at 4:2:2 one chroma sample
// with its up-to-two luma pixels; 16-byte loads, 2-byte stores, every coordinate clamped.  No LDS, no atomics, no scratch.
#include "average_common.h"
#include "yuv_common.h"  // ptl_q16 .. ptl_encode16, luma, the chroma pair by shift, ptl_load_pixel: shared with yuv420p10_f32.hip

#ifndef PTL_YUVXF_UNROLL
#define PTL_YUVXF_UNROLL 2  // sub-frames per group: 4 x 16-byte loads per lane each
#endif

// Fast path: block b = (row y, 4-pixel column group bx), bw = W / 4 groups per row.  Chroma: 422 or 444.
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

template <int Chroma, bool One, class Frames>
__device__ __forceinline__ void ptl_yuvxf_frame(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const unsigned int n_px = (unsigned)w * (unsigned)h;
    const double inv_n = 1.0 / (double)n;
    if ((w & 3) == 0) {
        const unsigned int bw = (unsigned)w >> 2, n_blocks = n_px >> 2;
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuvxf_block<Chroma, One>(frames, n, inv_n, out, w, h, b, bw);
    } else if (Chroma == 444) {
        for (unsigned int t = first; t < n_px; t += stride) ptl_yuvxf_pixel<One>(frames, n, inv_n, out, t, n_px);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, n_samples = cw * (unsigned)h;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuvxf_sample<One>(frames, n, inv_n, out, w, h, t, cw);
    }
}

template <int Chroma, class Frames>
__device__ __forceinline__ void ptl_yuvxf_all(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    // wave-uniform, as in ptl_yuvf_all: one test per launch, each side with the answer compiled in
    if (n > 1) ptl_yuvxf_frame<Chroma, false>(frames, n, out, w, h);
    else ptl_yuvxf_frame<Chroma, true>(frames, n, out, w, h);
}

extern "C" __global__ void __launch_bounds__(256)
ptl_average_f32_to_yuv422p10_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvxf_all<422>(frames, n, out, w, h);
}
extern "C" __global__ void __launch_bounds__(256)
ptl_average_f32_to_yuv444p10_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvxf_all<444>(frames, n, out, w, h);
}

// 65..256 sub-frames: the pointers no longer fit the kernel arguments (as for ptl_average_f32_to_yuv420p10_table_kernel)
extern "C" __global__ void __launch_bounds__(256)
ptl_average_f32_to_yuv422p10_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvxf_all<422>(ptl_frame_table{table}, n, out, w, h);
}
extern "C" __global__ void __launch_bounds__(256)
ptl_average_f32_to_yuv444p10_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvxf_all<444>(ptl_frame_table{table}, n, out, w, h);
}
