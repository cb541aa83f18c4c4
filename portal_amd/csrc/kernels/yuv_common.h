// yuv_common.h -- what the kernels that turn N sub-frames into one planar Y'CbCr 10-bit frame share (yuv10.hip: RGBA8 sub-frames,
// yuv10_f32.hip: RGBA32F ones).  Per sub-frame format: the loads through a 32-bit lane offset, the encode of the averaged frame A (8 bit
// from RGBA8 sums, 16 bit from RGBA32F sub-frames), luma, and the chroma pair with the shift of the sampling as a template parameter.  Written
// once for both formats, at the end: the n == 1 split and the entries, over each source's dispatchers.  The weights of a chroma sample's sum S_c add up to 2^(K - 16) (RGBA8) or 2^(K - 23) (float): 8 at 4:2:0, 4 at
// 4:2:2, 1 at 4:4:4.
//
// Contract (include/portal_amd.h).  A(x, y) is the averaged frame of the format (yuv10.hip, yuv10_f32.hip).  Layout:
// Y plane W*H little-endian u16, then Cb and Cr, cw*ch each.  The samplings differ in the chroma sample's tap window alone (yuv_shape.h):
//   4:2:0  cw = (W+1)/2, ch = (H+1)/2   S_c = sum over rows 2j, 2j+1 of A_c(2i-1, .) + 2 A_c(2i, .) + A_c(2i+1, .)   MPEG-2 ("left") siting
//   4:2:2  cw = (W+1)/2, ch = H         S_c = A_c(2i-1, y) + 2 A_c(2i, y) + A_c(2i+1, y)                             co-sited with luma column 2i
//   4:4:4  cw = W,       ch = H         S_c = A_c(x, y)
// with every coordinate clamped to the frame.
#pragma once
#include "average_common.h"  // pointer lists, ptl_accumulate, ptl_div_n, ptl_l_to_s -- the same functions ptl_average_images runs
#include "yuv_shape.h"       // the samplings, the fast-path predicate and the block shapes: the host sizes the launch by the same text

typedef unsigned int ptl_u32x2 __attribute__((ext_vector_type(2)));
typedef float ptl_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long ptl_u64;

// ---- RGBA8 sub-frames: A holds 8-bit values, 32-bit integer arithmetic ----------------------------------------------------------------
__device__ __forceinline__ unsigned int ptl_luma10(const unsigned int (&a)[3]) {
    return (55896u * a[0] + 188037u * a[1] + 18982u * a[2] + 32768u) >> 16;
}
// s: the weighted sums of a chroma sample, 0 .. 255 * 2^(K - 16).  Both accumulators stay positive (>= 65 410 << (K - 16)), so >> is a plain shift.
template <int K>
__device__ __forceinline__ unsigned int ptl_cb10(const int (&s)[3]) {
    return (unsigned int)min(1023, (-30123 * s[0] - 101335 * s[1] + 131458 * s[2] + (512 << K) + (1 << (K - 1))) >> K);
}
template <int K>
__device__ __forceinline__ unsigned int ptl_cr10(const int (&s)[3]) {
    return (unsigned int)min(1023, (131458 * s[0] - 119404 * s[1] - 12054 * s[2] + (512 << K) + (1 << (K - 1))) >> K);
}
// A sub-frame is addressed as "uniform base + 32-bit byte offset of the lane" (W*H <= 2^29, the entry point refuses more): the base stays
// in scalar registers and a lane keeps one 32-bit offset per row instead of a 64-bit address per load.
__device__ __forceinline__ ptl_u32x4 ptl_load16(const ptl_u32x4* frame, unsigned int byte_offset) {
    return ptl_stream_load(reinterpret_cast<const ptl_u32x4*>(reinterpret_cast<const char*>(frame) + byte_offset));
}
__device__ __forceinline__ unsigned int ptl_load4(const ptl_u32x4* frame, unsigned int byte_offset) {
    return *reinterpret_cast<const unsigned int*>(reinterpret_cast<const char*>(frame) + byte_offset);
}

// channel sums of the sub-frames -> the bytes ptl_average_images writes
__device__ __forceinline__ void ptl_encode3(unsigned int (&a)[3], const unsigned int* sum, unsigned int magic) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = ptl_l_to_s(ptl_div_n(sum[c], magic));
}

// ---- RGBA32F sub-frames: A holds 16-bit values, chroma in 64-bit integers -------------------------------------------------------------
// unorm8 of the render entries at 16 bits.  v >= 1 (+inf too) goes through 1.0f: 65535.0f + 0.5f = 65535.5 exactly, truncated to 65535; the
// largest v < 1 gives 65535.496.  The value converted is never negative, so the truncation is the floor.
// The product and the sum are each rounded to binary32.  A --genco build contracts by default, and this toolchain's __fmul_rn / __fadd_rn are
// a plain `*` and `+` compiled WITH that default (they came out as one v_pk_fma_f32): the two operations stand here, under the pragma.
__device__ __forceinline__ unsigned int ptl_q16(float v) {
#pragma clang fp contract(off)
    const float above = v > 0.0f ? v : 0.0f;  // NaN, -0, negatives, -inf -> 0
    const float c = above >= 1.0f ? 1.0f : above;
    const float scaled = c * 65535.0f;
    return (unsigned int)(scaled + 0.5f);
}

// One: n == 1, decided once per launch.  E = q then (q (q - 1) < q^2 <= q (q + 1)), so a "sum" holds q itself and nothing is squared,
// divided or rooted: a plain conversion.
template <bool One>
__device__ __forceinline__ void ptl_accumulate_f32(ptl_u64 (&sum)[3], ptl_f32x4 p) {
    const unsigned int q[3] = {ptl_q16(p.x), ptl_q16(p.y), ptl_q16(p.z)};
#pragma unroll
    for (int c = 0; c < 3; ++c) sum[c] += One ? (ptl_u64)q[c] : (ptl_u64)q[c] * q[c];  // (one v_mad_u64_u32)
}

// floor(sum / n) for sum <= 256 * 65535^2 < 2^40 and 2 <= n <= 256, with inv_n = 1.0 / n (binary64, once per lane).  (double)sum is exact.
// x = sum * inv_n + 2^-10 carries two roundings of 2^-53 relative on a value < 2^39 and inv_n's own: off by less than 2^-12 from
// sum / n + 2^-10.  sum / n is an integer k, or at least 1/n >= 2^-8 away from one: x lies in (k, k + 1) either way and truncates to k.
// k <= 65535^2 fits 32 bits.  (A 64-bit `/` would be a call's worth of VALU, twelve times per lane.)
__device__ __forceinline__ unsigned int ptl_mean_n(ptl_u64 sum, double inv_n) {
    return (unsigned int)__fma_rn((double)sum, inv_n, 0x1p-10);
}

// floor(sqrt(m) + 1/2) in integers for m <= 65535^2: the hardware estimate of the root is within 0.02 of it ((float)m and v_sqrt_f32 are
// good to 2^-24 relative each, the sum to 2^-9 absolute), so e is at most one off and the two comparisons of the definition settle it.
// e <= 65535 here (sqrt(m) + 0.52 < 65536), so e (e + 1) <= 65535 * 65536 fits 32 bits.
__device__ __forceinline__ unsigned int ptl_root_nearest(unsigned int m) {
    unsigned int e = (unsigned int)(__builtin_amdgcn_sqrtf((float)m) + 0.5f);
    const unsigned int above = e * e + e;  // e (e + 1); e (e - 1) = above - 2 e
    if (m > above) ++e;
    else if (e != 0u && m <= above - 2u * e) --e;
    return e;
}

template <bool One>
__device__ __forceinline__ void ptl_encode16(unsigned int (&a)[3], const ptl_u64 (&sum)[3], double inv_n) {
#pragma unroll
    for (int c = 0; c < 3; ++c) a[c] = One ? (unsigned int)sum[c] : ptl_root_nearest(ptl_mean_n(sum[c], inv_n));
}

// The largest accumulator is 65473 * 65535 + 2^21 = 4 292 870 207 < 2^32.
__device__ __forceinline__ unsigned int ptl_luma10_16(const unsigned int (&a)[3]) {
    return (13920u * a[0] + 46826u * a[1] + 4727u * a[2] + (1u << 21)) >> 22;
}
// s: the weighted sums of a chroma sample, 0 .. 65535 * 2^(K - 23).  Both accumulators stay positive (>= 8 388 545 << (K - 23)), so >> is a plain shift.
template <int K>
__device__ __forceinline__ unsigned int ptl_cb10_16(const unsigned int (&s)[3]) {
    const long long acc = -15003ll * s[0] - 50470ll * s[1] + 65473ll * s[2] + (512ll << K) + (1ll << (K - 1));
    return (unsigned int)min(1023ll, acc >> K);
}
template <int K>
__device__ __forceinline__ unsigned int ptl_cr10_16(const unsigned int (&s)[3]) {
    const long long acc = 65473ll * s[0] - 59470ll * s[1] - 6003ll * s[2] + (512ll << K) + (1ll << (K - 1));
    return (unsigned int)min(1023ll, acc >> K);
}

// A float sub-frame through the same kind of offset (16 W*H <= 2^32, the entry point refuses more), 16 bytes per pixel.
__device__ __forceinline__ ptl_f32x4 ptl_load_pixel(const ptl_u32x4* frame, unsigned int byte_offset) {
    return *reinterpret_cast<const ptl_f32x4*>(reinterpret_cast<const char*>(frame) + byte_offset);
}

// ---- what a launch is, written once for both formats: the n == 1 split and the entries ----------------------------------------------------
// A format: what a launch computes once for its encode -- the multiply-high magic of ptl_div_n (RGBA8) or nothing (float: the dispatcher
// takes 1.0 / n itself) -- and One (float only): n == 1, compiled in.  Each source specialises ptl_yuv_frame<format, sampling>, its
// dispatcher, once for 4:2:0 and once for the other two samplings: the split below reaches them without a forwarding layer.
struct ptl_rgba8 {
    static __device__ __forceinline__ unsigned int param(int n) { return 0xffffffffu / (unsigned)n + 1u; }
    static constexpr unsigned int kParamOne = 0u;  // ptl_div_n's "no division"
};
template <bool One>
struct ptl_rgba32f {
    static __device__ __forceinline__ int param(int) { return 0; }
    static constexpr int kParamOne = 0;
};
template <class Format, int Chroma>
struct ptl_yuv_frame;  // run(frames, n, param, out, w, h): one frame, grid-stride

// Many, Single: the format for n > 1 and for n == 1 (the same struct where the format has no One).
template <class Many, class Single, int Chroma, class Frames>
__device__ __forceinline__ void ptl_yuv_all(const Frames& frames, int n, unsigned short* __restrict__ out, int w, int h) {
    // wave-uniform, as in ptl_average_all.  ptl_div_n tests its magic per value (54 of them per 8x2 block): one test per launch instead,
    // each side with the answer compiled in -- n == 1, a plain conversion, has no multiply at all
    if (n > 1) ptl_yuv_frame<Many, Chroma>::run(frames, n, Many::param(n), out, w, h);
    else ptl_yuv_frame<Single, Chroma>::run(frames, n, Single::kParamOne, out, w, h);
}

// The two entries of a sampling: up to 64 sub-frames travel in the kernel arguments; for 65..256 the pointers no longer fit them and
// come from a table in device memory (as for ptl_average_images_table_kernel).
#define PTL_YUV_ENTRIES(name, Many, Single, Chroma)                                                                                               \
    extern "C" __global__ void __launch_bounds__(256) name##_kernel(ptl_frame_list frames, int n, unsigned short* __restrict__ out, int w, int h) { \
        ptl_yuv_all<Many, Single, Chroma>(frames, n, out, w, h);                                                                         \
    }                                                                                                                                        \
    extern "C" __global__ void __launch_bounds__(256)                                                                                        \
    name##_table_kernel(const ptl_u32x4* const* table, int n, unsigned short* __restrict__ out, int w, int h) {                             \
        ptl_yuv_all<Many, Single, Chroma>(ptl_frame_table{table}, n, out, w, h);                                                         \
    }
