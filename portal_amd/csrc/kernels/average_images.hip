// average_images.hip -- motion-blur sub-frame averaging in linear light, on the GPU.
//
// Reference: average_images (src/main.rs:645-722), a CPU loop over RGBA8 frames using two LUTs:
// S_TO_L[c] = c*c (gamma-2 decode to 0..65025), integer mean over the N sub-frames, then
// L_TO_S[l] = (u8)(sqrt(l as f32) + 0.5) (gamma-2 encode, rounded), alpha = 255.
// This is byte/integer work and HBM-bound: per output pixel it reads 4 N bytes and writes 4.
//
// gfx950 mapping: one lane handles 4 consecutive pixels = one 16-byte load per sub-frame
// (64 lanes x 16 B = 1 KiB per wave-instruction, fully coalesced), accumulates 12 u32 sums in
// registers, and issues one 16-byte store.  The sub-frame loop is unrolled x4 so at least four
// independent 16-byte loads per lane are in flight.  No LDS, no atomics.  The LUTs are arithmetic here:
// c*c is exact in u32, the integer mean is a multiply-high by a per-launch constant, and sqrt + 0.5 truncated equals
// the reference's table entry for every l <= 65025 (see ptl_l_to_s).
#include "average_common.h"  // pointer lists, ptl_accumulate, ptl_div_n, ptl_l_to_s, the tuning knobs

template <class Frames>
__device__ __forceinline__ void ptl_average_one(const Frames& frames, int n, unsigned int magic, ptl_u32x4* __restrict__ out, long i) {
    unsigned int sum[12] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    int f = 0;
    for (; f + PTL_AVG_UNROLL <= n; f += PTL_AVG_UNROLL) {
        ptl_u32x4 v[PTL_AVG_UNROLL];
#pragma unroll
        for (int k = 0; k < PTL_AVG_UNROLL; ++k) v[k] = ptl_stream_load(frames.frame[f + k] + i);
#pragma unroll
        for (int k = 0; k < PTL_AVG_UNROLL; ++k) ptl_accumulate(sum, v[k]);
    }
    for (; f < n; ++f) ptl_accumulate(sum, ptl_stream_load(frames.frame[f] + i));
    unsigned int px[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int r = ptl_l_to_s(ptl_div_n(sum[3 * k + 0], magic));
        const unsigned int g = ptl_l_to_s(ptl_div_n(sum[3 * k + 1], magic));
        const unsigned int b = ptl_l_to_s(ptl_div_n(sum[3 * k + 2], magic));
        px[k] = r | (g << 8) | (b << 16) | 0xff000000u;
    }
    const ptl_u32x4 packed = {px[0], px[1], px[2], px[3]};
#if PTL_AVG_NT
    __builtin_nontemporal_store(packed, out + i);
#else
    out[i] = packed;
#endif
}

// One pixel with 4-byte accesses: the up-to-three pixels behind the last whole 16-byte vector of a frame.
template <class Frames>
__device__ __forceinline__ void ptl_average_tail_pixel(const Frames& frames, int n, unsigned int magic, unsigned int* __restrict__ out, long px) {
    unsigned int r = 0u, g = 0u, b = 0u;
    for (int f = 0; f < n; ++f) {
        const unsigned int w = reinterpret_cast<const unsigned int*>(frames.frame[f])[px];
        const unsigned int cr = w & 0xffu, cg = (w >> 8) & 0xffu, cb = (w >> 16) & 0xffu;
        r += cr * cr;
        g += cg * cg;
        b += cb * cb;
    }
    out[px] = ptl_l_to_s(ptl_div_n(r, magic)) | (ptl_l_to_s(ptl_div_n(g, magic)) << 8) | (ptl_l_to_s(ptl_div_n(b, magic)) << 16) | 0xff000000u;
}

template <class Frames>
__device__ __forceinline__ void ptl_average_all(const Frames& frames, int n, ptl_u32x4* __restrict__ out, long n_px) {
    const long stride = (long)gridDim.x * 256;
    const long n_vec = n_px >> 2;  // whole 4-pixel vectors
    const unsigned int magic = n > 1 ? 0xffffffffu / (unsigned)n + 1u : 0u;  // wave-uniform: one division on the scalar side of things
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_vec; i += stride * PTL_AVG_VPT) {
#pragma unroll
        for (int v = 0; v < PTL_AVG_VPT; ++v)
            if (i + v * stride < n_vec) ptl_average_one(frames, n, magic, out, i + v * stride);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n_px & 3)) ptl_average_tail_pixel(frames, n, magic, reinterpret_cast<unsigned int*>(out), n_vec * 4 + threadIdx.x);
}

extern "C" __global__ void __launch_bounds__(256)
ptl_average_images_kernel(ptl_frame_list frames, int n, ptl_u32x4* __restrict__ out, long n_px) {
    ptl_average_all(frames, n, out, n_px);
}

// The reference takes any motion_blur_frames (src/main.rs:1766); beyond 64 the pointers no longer fit the kernel arguments.
extern "C" __global__ void __launch_bounds__(256)
ptl_average_images_table_kernel(const ptl_u32x4* const* table, int n, ptl_u32x4* __restrict__ out, long n_px) {
    ptl_average_all(ptl_frame_table{table}, n, out, n_px);
}
