// pass_stats.hip -- one sweep over the pass records of a launch (ptl_pass_record, 16 bytes per pixel: what a PTL_FLAG_PASSES render entry
// stores through out_passes), accumulated into a ptl_pass_stats_block that the caller zeroed once and keeps on the card: a clip adds every
// launch of every frame to one block and downloads it at its end.
//
// Contract (include/portal_amd.h; tests/pass_reference.py restates it in numpy).  Per record: final = final_escaped & 0xffff, escaped =
// final_escaped >> 16, exhausted = exhausted_outside & 0xffff, outside = exhausted_outside >> 16, paths = their sum.  The block receives the
// sums of pixels (records), paths, trips, final, escaped, exhausted and outside, the number of records with exhausted > 0, the largest
// trips of a record, a 256-bin histogram of trips per record (bin 255: trips >= 255), and the range of depth_near over the records whose
// depth_near is finite -- as the largest order-preserving key and the largest complemented key (pass_key.h), so that zero stands for "none"
// in both.  per_launch[slot] receives this launch's exhausted paths.  All integers: the result does not depend on the order of the adds.
//
// gfx950 mapping: a lane per record and grid-stride step (one 16-byte load: a wave reads 1 KiB contiguous), eight 64-bit sums and three
// 32-bit maxima in registers; the histogram is private to the workgroup in LDS (ds_add_u32, 256 bins).  A record's bin depends on the scene and
// neighbouring pixels mostly share one, so the adds of a wave to one bin are serialised by the LDS: measured, this and the single load in
// flight keep the kernel at 1.1 TB/s on a 4K frame (profiles/r16/README.md), far from the HBM bound the 16 bytes per record would allow.
// At the end the sums are reduced within the wave by shuffles, the wave leaders add them to LDS, and after one
// barrier lane t adds bin t and eleven lanes a total or a maximum each to the block: at most one global atomic per workgroup, per bin or total that is not zero.
// Traffic: 16 bytes per record in, nothing out.  No scratch.
#include <hip/hip_runtime.h>

#include "pass_key.h"

typedef unsigned int ptl_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long ptl_u64;

namespace {

enum { kPixels, kPaths, kTrips, kFinal, kEscaped, kExhausted, kOutside, kExhaustedPixels, kSums };  // the block's uint64 totals, in its order

__device__ __forceinline__ ptl_u64 wave_sum(ptl_u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned int wave_max(unsigned int v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned int other = (unsigned int)__shfl_down((int)v, off, 64);
        v = other > v ? other : v;
    }
    return v;
}

}  // namespace

extern "C" __global__ void __launch_bounds__(256)
ptl_pass_stats_kernel(const ptl_u32x4* __restrict__ records, long n, unsigned char* __restrict__ block, ptl_u64* __restrict__ per_launch, int slot) {
    __shared__ unsigned int hist[ptl_pass_hist_bins];
    __shared__ ptl_u64 sums[kSums];
    __shared__ unsigned int maxima[3];  // trips, depth key, complemented depth key
    const unsigned int t = threadIdx.x;
    hist[t] = 0u;  // (256 threads, 256 bins)
    if (t < kSums) sums[t] = 0ull;
    if (t < 3) maxima[t] = 0u;
    __syncthreads();

    ptl_u64 sum[kSums] = {};
    unsigned int max_trips = 0u, max_key = 0u, max_inv_key = 0u;
    const long stride = (long)gridDim.x * 256;
    for (long i = (long)blockIdx.x * 256 + t; i < n; i += stride) {
        const ptl_u32x4 r = records[i];
        const unsigned int trips = r.y, final_paths = r.z & 0xffffu, escaped = r.z >> 16, exhausted = r.w & 0xffffu, outside = r.w >> 16;
        sum[kPixels] += 1ull;
        sum[kPaths] += (ptl_u64)(final_paths + escaped + exhausted + outside);
        sum[kTrips] += (ptl_u64)trips;
        sum[kFinal] += (ptl_u64)final_paths;
        sum[kEscaped] += (ptl_u64)escaped;
        sum[kExhausted] += (ptl_u64)exhausted;
        sum[kOutside] += (ptl_u64)outside;
        sum[kExhaustedPixels] += exhausted != 0u ? 1ull : 0ull;
        max_trips = trips > max_trips ? trips : max_trips;
        if (ptl_pass_depth_is_finite(r.x)) {
            const unsigned int key = ptl_pass_depth_key(r.x);
            max_key = key > max_key ? key : max_key;
            max_inv_key = ~key > max_inv_key ? ~key : max_inv_key;
        }
        atomicAdd(&hist[trips < ptl_pass_hist_bins - 1 ? trips : ptl_pass_hist_bins - 1], 1u);
    }

    // within the wave by shuffles, across the four waves through LDS
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = wave_sum(sum[k]);
    max_trips = wave_max(max_trips);
    max_key = wave_max(max_key);
    max_inv_key = wave_max(max_inv_key);
    if ((t & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < kSums; ++k)
            if (sum[k] != 0ull) atomicAdd(&sums[k], sum[k]);
        atomicMax(&maxima[0], max_trips);
        atomicMax(&maxima[1], max_key);
        atomicMax(&maxima[2], max_inv_key);
    }
    __syncthreads();

    // the workgroup's share into the block: lane t its bin, the first lanes the totals
    if (hist[t] != 0u) atomicAdd(reinterpret_cast<ptl_u64*>(block + ptl_pass_block_histogram) + t, (ptl_u64)hist[t]);
    if (t < kSums && sums[t] != 0ull) {
        atomicAdd(reinterpret_cast<ptl_u64*>(block + ptl_pass_block_totals) + t, sums[t]);
        if (t == kExhausted && per_launch != nullptr) atomicAdd(&per_launch[slot], sums[t]);
    }
    if (t >= kSums && t < kSums + 3 && maxima[t - kSums] != 0u) atomicMax(reinterpret_cast<unsigned int*>(block + ptl_pass_block_maxima) + (t - kSums), maxima[t - kSums]);
}
