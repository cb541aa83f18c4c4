// aa_edges_common.h -- the classification of ONE RGBA8 frame by one grid of 64x32 regions: what kernels/aa_edges.hip (a frame) and
// kernels/aa_edges_slices.hip (a stack of frames, one per blockIdx.z) both run.  The rule, the LDS tile and the slot reservation are
// described at the top of aa_edges.hip.
#pragma once
#include <hip/hip_runtime.h>

#define PTL_AA_REGION_W 64
#define PTL_AA_REGION_H 32
#define PTL_AA_LDS_W (PTL_AA_REGION_W + 2)
#define PTL_AA_LDS_PITCH 72  // row pitch = 8 mod 64 banks: the 8 rows x 8 columns a wave reads at once fall into 64 different banks
#define PTL_AA_LDS_H (PTL_AA_REGION_H + 2)

__device__ __forceinline__ int ptl_aa_channel_distance(unsigned int a, unsigned int b) {
    const int dr = abs((int)(a & 255u) - (int)(b & 255u));
    const int dg = abs((int)((a >> 8) & 255u) - (int)((b >> 8) & 255u));
    const int db = abs((int)((a >> 16) & 255u) - (int)((b >> 16) & 255u));
    return max(dr, max(dg, db));
}

// The workgroup (blockIdx.x, blockIdx.y) classifies its region of `frame` and appends the refined pixels to `list`, reserving their
// slots with ONE returning add on `*count`.  Every argument is workgroup-uniform.
__device__ __forceinline__ void ptl_aa_edges_region(const unsigned int* __restrict__ frame, int width, int height, int threshold,
                                                    unsigned int* __restrict__ list, unsigned int* __restrict__ count) {
    __shared__ unsigned int tile[PTL_AA_LDS_H][PTL_AA_LDS_PITCH];
    __shared__ unsigned int wave_total[4];
    __shared__ unsigned int region_base;
    const int t = (int)threadIdx.x;
    const int wave = t >> 6, lane = t & 63;
    const int x0 = (int)blockIdx.x * PTL_AA_REGION_W, y0 = (int)blockIdx.y * PTL_AA_REGION_H;

    for (int i = t; i < PTL_AA_LDS_W * PTL_AA_LDS_H; i += 256) {
        const int ly = i / PTL_AA_LDS_W, lx = i - ly * PTL_AA_LDS_W;
        const int gx = min(max(x0 + lx - 1, 0), width - 1), gy = min(max(y0 + ly - 1, 0), height - 1);  // always inside the frame
        tile[ly][lx] = frame[(size_t)gy * (size_t)width + (size_t)gx];
    }
    __syncthreads();

    // tile k of this wave: columns 8k .. 8k+7 of region rows 8*wave .. 8*wave+7; the lane's pixel is (lane & 7, lane >> 3) in it
    const int ly = wave * 8 + (lane >> 3);
    const int py = y0 + ly;
    unsigned int mine = 0u;        // bit k: my pixel of tile k is refined
    unsigned int offset[8];        // my slot within the wave's run, per tile (indexed by the unrolled k only: registers)
    unsigned int total = 0u;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int lx = k * 8 + (lane & 7);
        const int px = x0 + lx;
        const unsigned int c = tile[ly + 1][lx + 1];
        int d = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) d = max(d, ptl_aa_channel_distance(tile[ly + dy][lx + dx], c));
        // (a halo word outside the frame holds the clamped pixel, which is what the rule reads there)
        const bool refine = px < width && py < height && d > threshold;
        const unsigned long long ballot = __ballot(refine);
        offset[k] = total + __builtin_amdgcn_mbcnt_hi((unsigned int)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)ballot, 0u));
        total += (unsigned int)__popcll(ballot);
        mine |= refine ? (1u << k) : 0u;
    }
    if (lane == 0) wave_total[wave] = total;
    __syncthreads();
    if (t == 0) {
        const unsigned int n = wave_total[0] + wave_total[1] + wave_total[2] + wave_total[3];
        region_base = n != 0u ? atomicAdd(count, n) : 0u;  // the one reservation of this workgroup
    }
    __syncthreads();
    unsigned int base = region_base;
    for (int w = 0; w < wave; ++w) base += wave_total[w];
#pragma unroll
    for (int k = 0; k < 8; ++k)
        if (mine >> k & 1u) list[base + offset[k]] = (unsigned int)py * (unsigned int)width + (unsigned int)(x0 + k * 8 + (lane & 7));
}
