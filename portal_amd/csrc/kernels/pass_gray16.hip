// pass_gray16.hip -- pass records in (ptl_pass_record, 16 bytes per pixel), the scanlines of one 16-bit greyscale PNG out (colour type 0, bit
// depth 16, filter None): what ptl_png_write_gray16 deflates as it is.
//
// Contract (include/portal_amd.h; tests/pass_reference.py restates it in numpy).  Sample g of a record, `which`:
//   PTL_PASS_DEPTH  0 where the record has no final path (final_escaped & 0xffff == 0), else q((depth_near - lo) / max(1e-6f, hi - lo)) with the
//                   difference, the divisor and the quotient each rounded to binary32 -- ONE IEEE division -- and q the 16-bit quantisation of the
//                   deep-colour kernels (yuv_common.h ptl_q16): 0 if !(v > 0), 65535 if v >= 1, else (u32)(v * 65535.0f + 0.5f), no FMA
//   PTL_PASS_TRIPS  min(trips, 65535): lossless up to there
// out: n samples as bytes g >> 8, g & 255 (big-endian), packed; rows of a frame follow each other without filter-type bytes, so the frame's
// width does not matter here and a wave may start anywhere in a row.
//
// gfx950 mapping: a lane owns four records = four adjacent 16-byte loads (a wave reads 4 KiB contiguous) and one 8-byte store; the n % 4 records
// left over get a lane each and a 2-byte store.  Grid-stride (the host caps the grid).  HBM-bound: 16 bytes in, 2 out per pixel.  No LDS, no
// atomics, no scratch.
#include "average_common.h"  // ptl_u32x4
#include "yuv_common.h"      // ptl_q16
#include "rgb48_shape.h"     // ptl_rgb48_swap16: two samples of a dword into PNG's byte order
#include "pass_key.h"        // the two values of `which`

typedef unsigned int ptl_u32x2 __attribute__((ext_vector_type(2)));

template <int Which>
__device__ __forceinline__ unsigned int ptl_pass_sample(ptl_u32x4 r, float lo, float span) {
    if constexpr (Which == ptl_pass_which_trips) {
        return r.y < 65535u ? r.y : 65535u;
    } else {
        const float t = (__uint_as_float(r.x) - lo) / span;  // correctly rounded: this build keeps hipcc's default IEEE division
        return (r.z & 0xffffu) != 0u ? ptl_q16(t) : 0u;
    }
}

template <int Which>
__device__ __forceinline__ void ptl_passes_to_gray16(const ptl_u32x4* __restrict__ records, long n, unsigned short* __restrict__ out, float lo, float hi) {
    const float span = hi - lo > 1e-6f ? hi - lo : 1e-6f;  // max(1e-6f, hi - lo); a NaN range gives 1e-6
    const long stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_blocks = n >> 2;
    for (long b = first; b < n_blocks; b += stride) {
        ptl_u32x4 r[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) r[x] = records[4 * b + x];
        unsigned int g[4];
#pragma unroll
        for (int x = 0; x < 4; ++x) g[x] = ptl_pass_sample<Which>(r[x], lo, span);
        const ptl_u32x2 v = {ptl_rgb48_swap16(g[0] | (g[1] << 16)), ptl_rgb48_swap16(g[2] | (g[3] << 16))};
        reinterpret_cast<ptl_u32x2*>(out)[b] = v;
    }
    for (long i = 4 * n_blocks + first; i < n; i += stride) out[i] = (unsigned short)ptl_rgb48_swap16(ptl_pass_sample<Which>(records[i], lo, span));
}

extern "C" __global__ void __launch_bounds__(256)
ptl_passes_to_gray16_kernel(const ptl_u32x4* __restrict__ records, long n, unsigned short* __restrict__ out, int which, float lo, float hi) {
    if (which == ptl_pass_which_trips) ptl_passes_to_gray16<ptl_pass_which_trips>(records, n, out, lo, hi);
    else ptl_passes_to_gray16<ptl_pass_which_depth>(records, n, out, lo, hi);
}
