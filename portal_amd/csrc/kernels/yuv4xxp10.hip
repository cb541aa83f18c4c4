// yuv4xxp10.hip -- the 4:2:2 and 4:4:4 siblings of yuv420p10.hip: N RGBA8 sub-frames in, one planar Y'CbCr 10-bit frame out with chroma at
// half the horizontal resolution (4:2:2) or at full resolution (4:4:4).
//
// Contract (include/portal_amd.h; tests/yuv_chroma_reference.py restates it in numpy).  A(x, y), the luma formula, the
// plane order and the full-range 10-bit coding are those of yuv420p10.hip; only the chroma sampling differs:
//   4:2:2  cw = (W+1)/2, ch = H   S_c = A_c(2i-1, y) + 2 A_c(2i, y) + A_c(2i+1, y)   columns clamped, co-sited with luma column 2i    k = 18
//   4:4:4  cw = W,       ch = H   S_c = A_c(x, y)                                                                                      k = 16
//   Cb = min(1023, (-30123 S_R - 101335 S_G + 131458 S_B + (512 << k) + (1 << (k-1))) >> k)
//   Cr = min(1023, (131458 S_R - 119404 S_G -  12054 S_B + (512 << k) + (1 << (k-1))) >> k)
// HBM-bound: reads 4 N bytes and writes 4 (4:2:2) or 6 (4:4:4) bytes per pixel.
//
// gfx950 mapping, fast path (W % 8 == 0, any H): a lane owns 8x1 pixels = two 16-byte loads per sub-frame (eight in flight with the loop
// unrolled x4), 24 u32 sums, one 16-byte Y store.  4:4:4: two more 16-byte stores, no neighbour.  4:2:2: one 8-byte store per chroma plane;
// the column left of the block is the neighbouring lane's last pixel (one cross-lane move), only the first lane of a wave and the first
// block of a row load it themselves, block 0 of a row clamps to its own column 0 -- the rule of ptl_yuv_block.  General path (any W,
// H >= 1): at 4:4:4 a lane owns one pixel, at 4:2:2 one chroma sample with its up-to-two luma pixels; 4-byte loads, 2-byte stores, every
// coordinate clamped.  No LDS, no atomics, no scratch.
#include "average_common.h"
#include "yuv_common.h"  // luma, the chroma pair by shift, the 32-bit-offset loads, ptl_encode3: shared with yuv420p10.hip

#ifndef PTL_YUVX_UNROLL
#define PTL_YUVX_UNROLL 4  // sub-frames per group: 2 x 16-byte loads per lane each
#endif

// Fast path: block b = (row y, 8-pixel column group bx), bw = W / 8 groups per row.  Chroma: 422 or 444.
template <int Chroma, class Frames>
__device__ __forceinline__ void ptl_yuvx_block(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h,
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

template <int Chroma, class Frames>
__device__ __forceinline__ void ptl_yuvx_frame(const Frames& frames, int n, unsigned int magic, unsigned short* __restrict__ out, int w, int h) {
    const unsigned int stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const unsigned int n_px = (unsigned)w * (unsigned)h;
    if ((w & 7) == 0) {
        const unsigned int bw = (unsigned)w >> 3, n_blocks = n_px >> 3;
        for (unsigned int b = first; b < n_blocks; b += stride) ptl_yuvx_block<Chroma>(frames, n, magic, out, w, h, b, bw);
    } else if (Chroma == 444) {
        for (unsigned int t = first; t < n_px; t += stride) ptl_yuvx_pixel(frames, n, magic, out, t, n_px);
    } else {
        const unsigned int cw = ((unsigned)w + 1u) >> 1, n_samples = cw * (unsigned)h;
        for (unsigned int t = first; t < n_samples; t += stride) ptl_yuvx_sample(frames, n, magic, out, w, h, t, cw);
    }
}

template <int Chroma, class Frames>
__device__ __forceinline__ void ptl_yuvx_all(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    // wave-uniform, as in ptl_yuv_all: one test per launch, each side with the answer compiled in -- n == 1, a plain conversion, has no multiply at all
    if (n > 1) ptl_yuvx_frame<Chroma>(frames, n, 0xffffffffu / (unsigned)n + 1u, out, w, h);
    else ptl_yuvx_frame<Chroma>(frames, n, 0u, out, w, h);
}

extern "C" __global__ void __launch_bounds__(256)
ptl_average_to_yuv422p10_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvx_all<422>(frames, n, out, w, h);
}
extern "C" __global__ void __launch_bounds__(256)
ptl_average_to_yuv444p10_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvx_all<444>(frames, n, out, w, h);
}

// 65..256 sub-frames: the pointers no longer fit the kernel arguments (as for ptl_average_to_yuv420p10_table_kernel)
extern "C" __global__ void __launch_bounds__(256)
ptl_average_to_yuv422p10_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvx_all<422>(ptl_frame_table{table}, n, out, w, h);
}
extern "C" __global__ void __launch_bounds__(256)
ptl_average_to_yuv444p10_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {
    ptl_yuvx_all<444>(ptl_frame_table{table}, n, out, w, h);
}
