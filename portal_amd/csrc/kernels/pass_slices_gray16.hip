// pass_slices_gray16.hip -- the pass records of the N blur sub-frames of one output frame in (ptl_pass_record, 16 bytes per pixel and slice, slice z
// of pixel p at index z * slice_records + p: what the slices entry stores), up to three 16-bit greyscale images of that frame out, each the packed
// big-endian scanlines that pass_gray16.hip writes and ptl_png_write_gray16 deflates.
//
// Contract (include/portal_amd.h ptl_pass_slices_to_gray16; tests/pass_slices_reference.py restates it in numpy).  Per pixel, over the slices in
// order, integers exact:
//   depth  0 where no slice has a final path; else D = depth_near of the first slice that has one, replaced by every later such slice whose
//          depth_near < D (a NaN that came first stays; a slice without a final path is not looked at), then q((D - lo) / max(1e-6f, hi - lo)) with
//          pass_gray16.hip's arithmetic: one IEEE division in binary32, ptl_q16
//   trips  min(sum of min(trips_z, 65535), 65535): clamping the terms first gives the same value and keeps the sum below 2^32 for N <= 256
//   cut    E = sum of exhausted, P = sum of final + escaped + exhausted (outside samples do not count): 0 where P = 0, else ceil(65535 E / P)
//
// gfx950 mapping: a lane owns four adjacent pixels = per slice four adjacent 16-byte loads (a wave reads 4 KiB contiguous per slice), the slice loop
// goes four slices at a time so sixteen loads are in flight per lane (a scheduling barrier keeps them in front of the sums: 112 VGPRs, four waves
// per SIMD), the running depth, its flag and three sums per pixel stay in registers, and every output that was asked for (a wave-uniform choice: the
// pointers are kernel arguments) gets one 8-byte store.  The n % 4 pixels left over get a lane each and 2-byte stores.  Grid-stride (the host caps
// the grid).  16 N bytes in, 2 per output out: at 4K it runs at the rate of pass_gray16.hip for N = 1 and at 0.8 - 0.9 of it for N = 4 and 16
// (profiles/r21/README.md).  No LDS, no atomics, no scratch.
#include "average_common.h"  // ptl_u32x4
#include "yuv_common.h"      // ptl_q16
#include "rgb48_shape.h"     // ptl_rgb48_swap16: two samples of a dword into PNG's byte order

typedef unsigned int ptl_u32x2 __attribute__((ext_vector_type(2)));

struct ptl_pass_merge {  // what a pixel carries from slice to slice
    float depth = 0.0f;  // D, valid once has_final
    unsigned int has_final = 0u, trips = 0u, exhausted = 0u, paths = 0u;
};

__device__ __forceinline__ void ptl_pass_merge_add(ptl_pass_merge& m, ptl_u32x4 r) {
    const unsigned int final_paths = r.z & 0xffffu, exhausted = r.w & 0xffffu;
    const float depth = __uint_as_float(r.x);
    const bool takes = final_paths != 0u && (m.has_final == 0u || depth < m.depth);  // the first one as it is, NaN included; later ones with `<`
    m.depth = takes ? depth : m.depth;
    m.has_final |= final_paths != 0u ? 1u : 0u;
    m.trips += r.y < 65535u ? r.y : 65535u;
    m.exhausted += exhausted;
    m.paths += final_paths + (r.z >> 16) + exhausted;  // <= 256 * 3 * 65535 < 2^26
}

__device__ __forceinline__ unsigned int ptl_pass_merge_depth(const ptl_pass_merge& m, float lo, float span) {
    const float t = (m.depth - lo) / span;  // correctly rounded: this build keeps hipcc's default IEEE division
    return m.has_final != 0u ? ptl_q16(t) : 0u;
}
__device__ __forceinline__ unsigned int ptl_pass_merge_trips(const ptl_pass_merge& m) { return m.trips < 65535u ? m.trips : 65535u; }

// ceil(65535 E / P) for E <= P < 2^26, exact.  num = 65535 E < 2^42 and P are exact in binary64, so the rounded quotient truncates to floor(num / P)
// or to one more (never less: floor(num / P) is representable and rounding is monotonic); one step either way puts q right whatever the
// division's last bit, and the remainder says whether to round up.  (A 64-bit `/` would be a call's worth of VALU, four times per lane.)
__device__ __forceinline__ unsigned int ptl_pass_merge_cut(const ptl_pass_merge& m) {
    if (m.paths == 0u) return 0u;
    const unsigned long long num = 65535ull * m.exhausted, den = m.paths;
    long long q = (long long)((double)num / (double)den);
    long long rem = (long long)num - q * (long long)den;
    if (rem < 0) {
        --q;
        rem += (long long)den;
    } else if (rem >= (long long)den) {
        ++q;
        rem -= (long long)den;
    }
    return (unsigned int)q + (rem != 0 ? 1u : 0u);
}

// the X adjacent pixels from `first_pixel` on, merged over the slices: four slices' loads go out before the first of them is used
template <int X>
__device__ __forceinline__ void ptl_pass_merge_slices(const ptl_u32x4* __restrict__ records, int n_slices, unsigned long long slice_records, long first_pixel, ptl_pass_merge (&m)[X]) {
    const ptl_u32x4* p = records + first_pixel;
    int z = 0;
    for (; z + 4 <= n_slices; z += 4) {
        ptl_u32x4 r[4][X];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int x = 0; x < X; ++x) r[s][x] = p[(unsigned long long)s * slice_records + x];
        __builtin_amdgcn_sched_barrier(0);  // left alone the scheduler spreads the loads between the sums, six in flight at most: 4.6 instead of 5.6 TB/s at N = 4
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int x = 0; x < X; ++x) ptl_pass_merge_add(m[x], r[s][x]);
        p += 4ull * slice_records;
    }
    for (; z < n_slices; ++z) {
        ptl_u32x4 r[X];
#pragma unroll
        for (int x = 0; x < X; ++x) r[x] = p[x];
#pragma unroll
        for (int x = 0; x < X; ++x) ptl_pass_merge_add(m[x], r[x]);
        p += slice_records;
    }
}

__device__ __forceinline__ ptl_u32x2 ptl_pass_pack4(const unsigned int (&g)[4]) {
    return {ptl_rgb48_swap16(g[0] | (g[1] << 16)), ptl_rgb48_swap16(g[2] | (g[3] << 16))};
}

extern "C" __global__ void __launch_bounds__(256)
ptl_pass_slices_to_gray16_kernel(const ptl_u32x4* __restrict__ records, int n_slices, unsigned long long slice_records, long n, unsigned short* __restrict__ out_depth,
                                 unsigned short* __restrict__ out_trips, unsigned short* __restrict__ out_cut, float lo, float hi) {
    const float span = hi - lo > 1e-6f ? hi - lo : 1e-6f;  // max(1e-6f, hi - lo); a NaN range gives 1e-6
    const long stride = (long)gridDim.x * 256, first = (long)blockIdx.x * 256 + threadIdx.x;
    const long n_blocks = n >> 2;
    for (long b = first; b < n_blocks; b += stride) {
        ptl_pass_merge m[4];
        ptl_pass_merge_slices<4>(records, n_slices, slice_records, 4 * b, m);
        unsigned int g[4];
        if (out_depth) {
#pragma unroll
            for (int x = 0; x < 4; ++x) g[x] = ptl_pass_merge_depth(m[x], lo, span);
            reinterpret_cast<ptl_u32x2*>(out_depth)[b] = ptl_pass_pack4(g);
        }
        if (out_trips) {
#pragma unroll
            for (int x = 0; x < 4; ++x) g[x] = ptl_pass_merge_trips(m[x]);
            reinterpret_cast<ptl_u32x2*>(out_trips)[b] = ptl_pass_pack4(g);
        }
        if (out_cut) {
#pragma unroll
            for (int x = 0; x < 4; ++x) g[x] = ptl_pass_merge_cut(m[x]);
            reinterpret_cast<ptl_u32x2*>(out_cut)[b] = ptl_pass_pack4(g);
        }
    }
    for (long i = 4 * n_blocks + first; i < n; i += stride) {
        ptl_pass_merge m[1];
        ptl_pass_merge_slices<1>(records, n_slices, slice_records, i, m);
        if (out_depth) out_depth[i] = (unsigned short)ptl_rgb48_swap16(ptl_pass_merge_depth(m[0], lo, span));
        if (out_trips) out_trips[i] = (unsigned short)ptl_rgb48_swap16(ptl_pass_merge_trips(m[0]));
        if (out_cut) out_cut[i] = (unsigned short)ptl_rgb48_swap16(ptl_pass_merge_cut(m[0]));
    }
}
