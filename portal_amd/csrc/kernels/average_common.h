// average_common.h -- what the kernels that average RGBA8 sub-frames in linear light share (average_images.hip,
// yuv10.hip): the sub-frame pointer lists, the 16-byte accumulate, the multiply-high mean and the gamma-2 encode.
#pragma once
#ifndef __HIPCC_RTC__
#include <hip/hip_runtime.h>
#endif

#define PTL_MAX_SUBFRAMES 64

typedef unsigned int ptl_u32x4 __attribute__((ext_vector_type(4)));  // native vector: what the nontemporal builtins accept

struct ptl_frame_list {  // up to 64 sub-frames: the pointers travel in the kernel arguments
    const ptl_u32x4* frame[PTL_MAX_SUBFRAMES];
};
struct ptl_frame_table {  // 65..256 sub-frames: a pointer table in device memory (scalar loads)
    const ptl_u32x4* const* frame;
};

__device__ __forceinline__ void ptl_accumulate(unsigned int (&sum)[12], ptl_u32x4 p) {
    const unsigned int w[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const unsigned int r = w[k] & 0xffu, g = (w[k] >> 8) & 0xffu, b = (w[k] >> 16) & 0xffu;
        sum[3 * k + 0] += r * r;
        sum[3 * k + 1] += g * g;
        sum[3 * k + 2] += b * b;
    }
}

// L_TO_S[l] = ((l as f32).sqrt() + 0.5) as u8 for l <= 65025.  The hardware v_sqrt_f32 (1 ulp) is enough: the value only
// changes where sqrt(l) + 0.5 crosses an integer, i.e. near l = k*k + k + 1/4, and the nearest integers l = k*k + k and
// k*k + k + 1 keep sqrt(l) at least 1/(8k+4) >= 4.9e-4 away from k + 0.5 -- against an ulp of 3e-5 at 256.  (Checked for
// every l in tests/test_gpu_parity.py::test_average_images_every_linear_value.)
__device__ __forceinline__ unsigned int ptl_l_to_s(unsigned int linear) {
    return (unsigned int)(__builtin_amdgcn_sqrtf((float)linear) + 0.5f);  // truncation, like `as u8` on a value <= 255.5
}

// sum / n for sum <= 65025 * n and 2 <= n <= 256 as one multiply-high: with m = floor(2^32 / n) + 1,
// m*n - 2^32 = e in (0, n], and floor(sum * m / 2^32) == floor(sum / n) whenever sum * e < 2^32
// (65025 * 256 * 256 = 4.26e9 < 2^32 = 4.29e9: n = 256 is the last one that fits; checked for every n in tests/test_host_logic.py).
// A runtime `/` would be ~30 VALU instructions, twelve times per lane -- more than the whole rest of the kernel.
__device__ __forceinline__ unsigned int ptl_div_n(unsigned int sum, unsigned int magic) {
    return magic ? __umulhi(sum, magic) : sum;  // magic == 0 encodes n == 1
}

// Tuning knobs (tools/average_variants.py builds the alternatives; the defaults are what ships):
#ifndef PTL_AVG_UNROLL
#define PTL_AVG_UNROLL 4  // independent 16-byte loads in flight per lane and sub-frame group
#endif
#ifndef PTL_AVG_NT
#define PTL_AVG_NT 0      // 1: non-temporal (streaming) loads and store.  Measured slower (5.3 vs 6.1 TB/s at 4K, N = 4): the
                          // sub-frames were written by the tracer a moment ago and part of them is still in the 256 MB MALL
#endif
#ifndef PTL_AVG_VPT
#define PTL_AVG_VPT 1     // 16-byte vectors per lane per grid-stride step
#endif

__device__ __forceinline__ ptl_u32x4 ptl_stream_load(const ptl_u32x4* p) {
#if PTL_AVG_NT
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}

// one RGBA8 pixel (4-byte access): the scalar counterpart of ptl_accumulate
__device__ __forceinline__ void ptl_accumulate_pixel(unsigned int (&sum)[3], unsigned int w) {
    const unsigned int r = w & 0xffu, g = (w >> 8) & 0xffu, b = (w >> 16) & 0xffu;
    sum[0] += r * r;
    sum[1] += g * g;
    sum[2] += b * b;
}
